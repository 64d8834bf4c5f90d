// The one statistic of the model that the KL-optimal reverse variance needs (Bao et al. 2022, "Analytic-DPM"): for every
// sample the squared norm of the model's noise prediction eps_hat = ex x_t + eo out - the network's output for an
// eps-model (ex, eo) = (0, 1), sqrt(1 - abar) x_t + sqrt(abar) out for a v-model.  One pass over x_t and out
// (8 B/element), one workgroup per sample, in the pattern of vlb_terms_kernel (likelihood.hip).
#include "internal.h"

#define SQN_BLOCK 256

__device__ __forceinline__ float sqn_elem(float acc, float x, float o, float ex, float eo) {
  const float e = __fadd_rn(__fmul_rn(ex, x), __fmul_rn(eo, o));
  return __fadd_rn(acc, __fmul_rn(e, e));
}

// Thread i of the block takes the float4s i, i + 256, ... of its sample; the sum is folded inside the wave by a
// butterfly and the four wave totals are added by thread 0 in wave order: the same order for every batch size, so a
// sample's number depends on that sample alone.
__global__ void __launch_bounds__(SQN_BLOCK)
eps_sqnorm_kernel(const float* __restrict__ x_t, const float* __restrict__ out, const int64_t* __restrict__ t,
                  const float* __restrict__ rows, int per4, float* __restrict__ sums, int64_t sample_stride) {
  __shared__ float part[SQN_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const float* row = rows + 2 * t[b];
  const float ex = row[0], eo = row[1];
  const int64_t base = b * (int64_t)per4;
  const float4* ax = (const float4*)x_t + base;
  const float4* ao = (const float4*)out + base;
  float acc = 0.0f;
  for (int i = tid; i < per4; i += SQN_BLOCK) {
    const float4 vx = ax[i], vo = ao[i];
    acc = sqn_elem(acc, vx.x, vo.x, ex, eo);
    acc = sqn_elem(acc, vx.y, vo.y, ex, eo);
    acc = sqn_elem(acc, vx.z, vo.z, ex, eo);
    acc = sqn_elem(acc, vx.w, vo.w, ex, eo);
  }
  const float s = wave_sum(acc);
  if (lane == 0) part[wave] = s;
  __syncthreads();
  if (tid == 0) {
    float v = part[0];
#pragma unroll
    for (int w = 1; w < SQN_BLOCK / 64; ++w) v = __fadd_rn(v, part[w]);
    sums[b * sample_stride] = v;
  }
}

extern "C" int tdx_eps_sqnorm(const float* x_t, const float* out, const int64_t* t, const float* rows, int batch,
                              int per_sample, float* sums, int64_t sample_stride, tdx_stream_t stream) {
  if (!x_t || !out || !t || !rows || !sums || batch <= 0 || per_sample <= 0 || per_sample % 4 || sample_stride < 1)
    return TDX_E_BADARG;
  eps_sqnorm_kernel<<<batch, SQN_BLOCK, 0, to_stream(stream)>>>(x_t, out, t, rows, per_sample / 4, sums,
                                                                  sample_stride);
  TDX_CHECK_LAUNCH();
  return 0;
}
