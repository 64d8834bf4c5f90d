// The per-sample sums of the variational bound (Ho et al. 2020 eq. 5; Nichol & Dhariwal 2021, calc_bpd_loop): for every
// sample the squared eps error, the squared distance of x0 from the model's (clamped) x0 prediction - the posterior KL
// of a timestep up to two host-side constants - and, on the row of t = 0, the negative log-likelihood of the
// discretised Gaussian decoder.  One pass over x0, x_t, out and the noise (16 B/element), one workgroup per sample.
#include "internal.h"

#define VLB_BLOCK 256

// -log of the probability the decoder N(x0c, sigma^2) gives to the bin of x0, from d = x0 - x0c and s = 1 / sigma:
// a = (d + half) s and b = (d - half) s are the standardised upper and lower edge of the bin, the first bin extends to
// -inf and the last to +inf.  Every CDF is taken as a tail, Phi(z) = erfc(-z / sqrt 2) / 2, on the side where it is
// small: Phi(a) - Phi(b) = Phi(-b) - Phi(-a), and for d > 0 both -b and -a lie left of where a and b do.  The textbook
// form (1 + erf) / 2 rounds every CDF to 6e-8 absolute, which is the whole probability of a bin three sigma out.
// The two tails are subtracted before the floor.  Each operation is rounded separately.
__device__ __forceinline__ float vlb_dec_nll(float x0, float d, float s, float half, float lo_edge, float hi_edge) {
  const float RS2 = 0.70710678118654752f;
  const float a = __fmul_rn(__fmul_rn(__fadd_rn(d, half), s), RS2);
  const float b = __fmul_rn(__fmul_rn(__fsub_rn(d, half), s), RS2);
  float P;
  if (x0 < lo_edge) P = erfcf(-a);
  else if (x0 > hi_edge) P = erfcf(b);
  else if (d > 0.0f) P = __fsub_rn(erfcf(b), erfcf(a));
  else P = __fsub_rn(erfcf(-a), erfcf(-b));
  P = fmaxf(__fmul_rn(0.5f, P), 1e-12f);
  return -logf(P);
}

struct VlbAcc { float e2, d2, nll; };

template <bool NOISE>
__device__ __forceinline__ void vlb_elem(float x0, float x, float o, float n, float p, float q, float ex, float eo,
                                         float clip_lo, float clip_hi, bool dec, float s, float half, float lo_edge,
                                         float hi_edge, VlbAcc& acc) {
  const float d = __fsub_rn(x0, x0_clamped(x, o, p, q, clip_lo, clip_hi));
  acc.d2 = __fadd_rn(acc.d2, __fmul_rn(d, d));
  if (NOISE) {
    const float e = __fsub_rn(n, __fadd_rn(__fmul_rn(ex, x), __fmul_rn(eo, o)));
    acc.e2 = __fadd_rn(acc.e2, __fmul_rn(e, e));
  }
  if (dec) acc.nll = __fadd_rn(acc.nll, vlb_dec_nll(x0, d, s, half, lo_edge, hi_edge));
}

// Thread i of the block takes the float4s i, i + 256, ... of its sample and keeps three sums; the sums are folded
// inside the wave by a butterfly and the four wave totals are added by thread 0 in wave order: the same order for every
// batch size, so a sample's three numbers depend on that sample alone.
template <bool NOISE>
__global__ void __launch_bounds__(VLB_BLOCK)
vlb_terms_kernel(const float* __restrict__ x0, const float* __restrict__ x_t, const float* __restrict__ out,
                 const float* __restrict__ noise, const int64_t* __restrict__ t, const float* __restrict__ rows,
                 int per4, float clip_lo, float clip_hi, int use_bins, float half, float lo_edge, float hi_edge,
                 float* __restrict__ terms, int64_t sample_stride) {
  __shared__ float part[VLB_BLOCK / 64][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const float* row = rows + 5 * t[b];
  const float p = row[0], q = row[1], ex = row[2], eo = row[3], s = row[4];
  const bool dec = use_bins && s > 0.0f;
  const int64_t base = b * (int64_t)per4;
  const float4* a0 = (const float4*)x0 + base;
  const float4* ax = (const float4*)x_t + base;
  const float4* ao = (const float4*)out + base;
  const float4* an = (const float4*)noise + base;   // read when NOISE only
  VlbAcc acc{0.0f, 0.0f, 0.0f};
  for (int i = tid; i < per4; i += VLB_BLOCK) {
    const float4 v0 = a0[i], vx = ax[i], vo = ao[i];
    float4 vn = make_float4(0.f, 0.f, 0.f, 0.f);
    if (NOISE) vn = an[i];
    vlb_elem<NOISE>(v0.x, vx.x, vo.x, vn.x, p, q, ex, eo, clip_lo, clip_hi, dec, s, half, lo_edge, hi_edge, acc);
    vlb_elem<NOISE>(v0.y, vx.y, vo.y, vn.y, p, q, ex, eo, clip_lo, clip_hi, dec, s, half, lo_edge, hi_edge, acc);
    vlb_elem<NOISE>(v0.z, vx.z, vo.z, vn.z, p, q, ex, eo, clip_lo, clip_hi, dec, s, half, lo_edge, hi_edge, acc);
    vlb_elem<NOISE>(v0.w, vx.w, vo.w, vn.w, p, q, ex, eo, clip_lo, clip_hi, dec, s, half, lo_edge, hi_edge, acc);
  }
  const float e2 = wave_sum(acc.e2), d2 = wave_sum(acc.d2), nll = wave_sum(acc.nll);
  if (lane == 0) {
    part[wave][0] = e2;
    part[wave][1] = d2;
    part[wave][2] = nll;
  }
  __syncthreads();
  if (tid < 3) {
    float v = part[0][tid];
#pragma unroll
    for (int w = 1; w < VLB_BLOCK / 64; ++w) v = __fadd_rn(v, part[w][tid]);
    terms[b * sample_stride + tid] = v;
  }
}

extern "C" int tdx_vlb_terms(const float* x0, const float* x_t, const float* out, const float* noise, const int64_t* t,
                             const float* rows, int batch, int per_sample, float clip_lo, float clip_hi, float data_lo,
                             float data_hi, int bins, float* terms, int64_t sample_stride, tdx_stream_t stream) {
  if (!x0 || !x_t || !out || !t || !rows || !terms || batch <= 0 || per_sample <= 0 || per_sample % 4 ||
      sample_stride < 3)
    return TDX_E_BADARG;
  if (!(clip_lo < clip_hi)) return TDX_E_BADARG;   // rejects a NaN bound
  if (bins == 1 || bins < 0) return TDX_E_BADARG;
  float half = 0.0f, lo_edge = 0.0f, hi_edge = 0.0f;
  if (bins >= 2) {
    if (!std::isfinite(data_lo) || !std::isfinite(data_hi) || !(data_lo < data_hi) || !std::isfinite(data_hi - data_lo))
      return TDX_E_BADARG;
    half = (data_hi - data_lo) / (2.0f * (float)(bins - 1));
    lo_edge = data_lo + half;
    hi_edge = data_hi - half;
  }
  const hipStream_t st = to_stream(stream);
  if (noise)
    vlb_terms_kernel<true><<<batch, VLB_BLOCK, 0, st>>>(x0, x_t, out, noise, t, rows, per_sample / 4, clip_lo, clip_hi,
                                                        bins, half, lo_edge, hi_edge, terms, sample_stride);
  else
    vlb_terms_kernel<false><<<batch, VLB_BLOCK, 0, st>>>(x0, x_t, out, noise, t, rows, per_sample / 4, clip_lo, clip_hi,
                                                         bins, half, lo_edge, hi_edge, terms, sample_stride);
  TDX_CHECK_LAUNCH();
  return 0;
}
