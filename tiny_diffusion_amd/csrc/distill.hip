// Progressive distillation (Salimans & Ho 2022, Algorithm 2): the two deterministic DDIM steps of the
// frozen teacher at PER-SAMPLE timesteps and the target of the student, as two HBM-bound elementwise kernels.  Sample b
// reads row t[b] of a (T, 12) table
//     (p1, q1, A1, B1,  p2, q2, A2, B2,  W2, W1, G, H)              schedule.distill_tables
// whose first eight entries are two rows of the x0 form (schedule.x0_form) of the teacher's grid:
//     x1c    = clamp(p1 z_t + q1 out1)          z_mid = A1 x1c + B1 z_t                      kernel 1
//     x2c    = clamp(p2 z_mid + q2 out2)        x~ = W2 x2c + W1 x1c     target = G x~ + H z_t   kernel 2
// Every product and sum is rounded on its own and in this order - x0_clamped and the (A x0 + Bx x) of x0_step_noise
// (common.h), i.e. pstep_elem<TDX_STEP_X0> without its noise term - so a CPU fp32 expression with one operation per
// rounding reproduces each bit.  float4 accesses, per_sample % 4 == 0 (a float4 never straddles two samples), the
// 48-byte row is loaded once per float4 and is uniform over per_sample / 4 consecutive lanes; grid-stride under the
// elementwise cap of 2048 x 256; no LDS, no atomics.  Kernel 1 moves 16 B per element (reads z_t, out1; writes z_mid,
// x1c), kernel 2 20 B (24 B with x_tilde).
//
// Guided distillation (Meng et al. 2023): the teacher is sampled under classifier-free guidance, so its
// output is the combination e = cfg_eps(out[i], out[i + n], w) of the two halves of a 2n-element buffer - the rows
// under the caller's condition, then the rows under the null condition, the layout of the guided sampler updates - and
// the arithmetic above runs on e.  GD is a template parameter of both kernels: the GD = false instantiations are the
// kernels as they were.  The guided kernel 1 writes z_mid to both halves of a 2n-element buffer and t_mid to both
// halves of a 2B vector: the input of the teacher's second forward (24 B per element; kernel 2 24 B, 28 B with
// x_tilde).  Kernel 3 is the same-timestep step (stage one of Meng et al.): sample b reads row t[b] of a (T, 4) table
//     (p, q, G, H)                                                   schedule.guidance_distill_table
//     x0c = clamp(p z_t + q e)                  target = G x0c + H z_t                        kernel 3
// with e the combination (GD) or out itself: 12 B per element, 16 B guided, 4 B more with x0c.
#include "internal.h"

static int distill_grid(int64_t n_items, int block) {   // elementwise.hip's ew_grid
  int64_t g = (n_items + block - 1) / block;
  if (g > 2048) g = 2048;  // 256 CUs x 8 blocks, grid-stride the rest
  if (g < 1) g = 1;
  return (int)g;
}

#define DISTILL_COLS 12

// z' = A x0 + Bx x: the deterministic part of x0_step_noise
__device__ __forceinline__ float distill_mix(float a, float x, float b, float y) {
  return __fadd_rn(__fmul_rn(a, x), __fmul_rn(b, y));
}

// the network's output of float4 i: out[i], or under guidance the cfg_eps combination with the null-condition half
template <bool GD>
__device__ __forceinline__ float4 distill_out(const float4* __restrict__ out, int64_t i, int64_t n4, float w) {
  float4 e = out[i];
  if (GD) {
    const float4 u = out[i + n4];
    e.x = cfg_eps(e.x, u.x, w);
    e.y = cfg_eps(e.y, u.y, w);
    e.z = cfg_eps(e.z, u.z, w);
    e.w = cfg_eps(e.w, u.w, w);
  }
  return e;
}

template <bool GD>
__global__ void __launch_bounds__(256)
distill_teacher_step_kernel(const float4* __restrict__ z_t, const float4* __restrict__ out1,
                            const int64_t* __restrict__ t, const float* __restrict__ rows,
                            const int64_t* __restrict__ t_mid_table, float4* __restrict__ z_mid,
                            float4* __restrict__ x1c, int64_t* __restrict__ t_mid, int batch, int64_t n4,
                            int per_sample4, float lo, float hi, float w) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  // the second teacher forward's timesteps: one look-up per sample, grid-strided like the elements
  for (int64_t b = tid; b < batch; b += stride) {
    const int64_t tm = t_mid_table[t[b]];
    t_mid[b] = tm;
    if (GD) t_mid[b + batch] = tm;
  }
  for (int64_t i = tid; i < n4; i += stride) {
    const int s = (int)(i / per_sample4);
    const float4 r = *(const float4*)(rows + DISTILL_COLS * t[s]);   // (p1, q1, A1, B1): 48-byte rows, 16-byte aligned
    const float4 z = z_t[i], o = distill_out<GD>(out1, i, n4, w);
    float4 c, m;
    c.x = x0_clamped(z.x, o.x, r.x, r.y, lo, hi);
    c.y = x0_clamped(z.y, o.y, r.x, r.y, lo, hi);
    c.z = x0_clamped(z.z, o.z, r.x, r.y, lo, hi);
    c.w = x0_clamped(z.w, o.w, r.x, r.y, lo, hi);
    m.x = distill_mix(r.z, c.x, r.w, z.x);
    m.y = distill_mix(r.z, c.y, r.w, z.y);
    m.z = distill_mix(r.z, c.z, r.w, z.z);
    m.w = distill_mix(r.z, c.w, r.w, z.w);
    x1c[i] = c;
    z_mid[i] = m;
    if (GD) z_mid[i + n4] = m;
  }
}

__device__ __forceinline__ float distill_target_elem(float z, float zm, float o2, float c1, const float4& r2,
                                                     const float4& r3, float lo, float hi, float* xt) {
  const float c2 = x0_clamped(zm, o2, r2.x, r2.y, lo, hi);
  const float x = distill_mix(r3.x, c2, r3.y, c1);       // x~ = W2 x2c + W1 x1c
  *xt = x;
  return distill_mix(r3.z, x, r3.w, z);                  // G x~ + H z_t
}

template <bool GD, bool XT>
__global__ void __launch_bounds__(256)
distill_target_kernel(const float4* __restrict__ z_t, const float4* __restrict__ z_mid,
                      const float4* __restrict__ out2, const float4* __restrict__ x1c,
                      const int64_t* __restrict__ t, const float* __restrict__ rows, float4* __restrict__ target,
                      float4* __restrict__ x_tilde, int64_t n4, int per_sample4, float lo, float hi, float w) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int s = (int)(i / per_sample4);
    const float4* row = (const float4*)(rows + DISTILL_COLS * t[s]);
    const float4 r2 = row[1], r3 = row[2];               // (p2, q2, A2, B2), (W2, W1, G, H)
    const float4 z = z_t[i], zm = z_mid[i], o = distill_out<GD>(out2, i, n4, w), c1 = x1c[i];
    float4 tg, xt;
    tg.x = distill_target_elem(z.x, zm.x, o.x, c1.x, r2, r3, lo, hi, &xt.x);
    tg.y = distill_target_elem(z.y, zm.y, o.y, c1.y, r2, r3, lo, hi, &xt.y);
    tg.z = distill_target_elem(z.z, zm.z, o.z, c1.z, r2, r3, lo, hi, &xt.z);
    tg.w = distill_target_elem(z.w, zm.w, o.w, c1.w, r2, r3, lo, hi, &xt.w);
    target[i] = tg;
    if (XT) x_tilde[i] = xt;
  }
}

#define GUIDANCE_COLS 4

template <bool GD, bool XC>
__global__ void __launch_bounds__(256)
distill_guidance_target_kernel(const float4* __restrict__ z_t, const float4* __restrict__ out,
                               const int64_t* __restrict__ t, const float* __restrict__ rows,
                               float4* __restrict__ target, float4* __restrict__ x0c, int64_t n4, int per_sample4,
                               float lo, float hi, float w) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int s = (int)(i / per_sample4);
    const float4 r = *(const float4*)(rows + GUIDANCE_COLS * t[s]);   // (p, q, G, H): 16-byte rows
    const float4 z = z_t[i], o = distill_out<GD>(out, i, n4, w);
    float4 c, tg;
    c.x = x0_clamped(z.x, o.x, r.x, r.y, lo, hi);
    c.y = x0_clamped(z.y, o.y, r.x, r.y, lo, hi);
    c.z = x0_clamped(z.z, o.z, r.x, r.y, lo, hi);
    c.w = x0_clamped(z.w, o.w, r.x, r.y, lo, hi);
    tg.x = distill_mix(r.z, c.x, r.w, z.x);                           // G x0c + H z_t
    tg.y = distill_mix(r.z, c.y, r.w, z.y);
    tg.z = distill_mix(r.z, c.z, r.w, z.z);
    tg.w = distill_mix(r.z, c.w, r.w, z.w);
    target[i] = tg;
    if (XC) x0c[i] = c;
  }
}

// what every entry refuses before any GPU call (the pointers are the entry's own business)
static bool distill_bad_sizes(int batch, int per_sample, float lo, float hi) {
  return batch <= 0 || per_sample <= 0 || per_sample % 4 || !(lo < hi);   // !(lo < hi) rejects a NaN bound
}

template <bool GD>
static int distill_teacher_step(const float* z_t, const float* out1, const int64_t* t, const float* rows,
                                const int64_t* t_mid_table, float* z_mid, float* x1c, int64_t* t_mid, int batch,
                                int per_sample, float w, float lo, float hi, tdx_stream_t stream) {
  if (!z_t || !out1 || !t || !rows || !t_mid_table || !z_mid || !x1c || !t_mid ||
      distill_bad_sizes(batch, per_sample, lo, hi))
    return TDX_E_BADARG;
  const int64_t n4 = (int64_t)batch * per_sample / 4;
  distill_teacher_step_kernel<GD><<<distill_grid(n4, 256), 256, 0, to_stream(stream)>>>(
      (const float4*)z_t, (const float4*)out1, t, rows, t_mid_table, (float4*)z_mid, (float4*)x1c, t_mid, batch, n4,
      per_sample / 4, lo, hi, w);
  TDX_CHECK_LAUNCH();
  return 0;
}

template <bool GD>
static int distill_target(const float* z_t, const float* z_mid, const float* out2, const float* x1c, const int64_t* t,
                          const float* rows, float* target, float* x_tilde, int batch, int per_sample, float w,
                          float lo, float hi, tdx_stream_t stream) {
  if (!z_t || !z_mid || !out2 || !x1c || !t || !rows || !target || distill_bad_sizes(batch, per_sample, lo, hi))
    return TDX_E_BADARG;
  const int64_t n4 = (int64_t)batch * per_sample / 4;
  const int grid = distill_grid(n4, 256);
  const hipStream_t st = to_stream(stream);
  if (x_tilde)
    distill_target_kernel<GD, true><<<grid, 256, 0, st>>>((const float4*)z_t, (const float4*)z_mid,
                                                          (const float4*)out2, (const float4*)x1c, t, rows,
                                                          (float4*)target, (float4*)x_tilde, n4, per_sample / 4, lo,
                                                          hi, w);
  else
    distill_target_kernel<GD, false><<<grid, 256, 0, st>>>((const float4*)z_t, (const float4*)z_mid,
                                                           (const float4*)out2, (const float4*)x1c, t, rows,
                                                           (float4*)target, nullptr, n4, per_sample / 4, lo, hi, w);
  TDX_CHECK_LAUNCH();
  return 0;
}

template <bool GD>
static int distill_guidance_target(const float* z_t, const float* out, const int64_t* t, const float* rows,
                                   float* target, float* x0c, int batch, int per_sample, float w, float lo, float hi,
                                   tdx_stream_t stream) {
  const int64_t n4 = (int64_t)batch * per_sample / 4;
  const int grid = distill_grid(n4, 256);
  const hipStream_t st = to_stream(stream);
  if (x0c)
    distill_guidance_target_kernel<GD, true><<<grid, 256, 0, st>>>((const float4*)z_t, (const float4*)out, t, rows,
                                                                   (float4*)target, (float4*)x0c, n4, per_sample / 4,
                                                                   lo, hi, w);
  else
    distill_guidance_target_kernel<GD, false><<<grid, 256, 0, st>>>((const float4*)z_t, (const float4*)out, t, rows,
                                                                    (float4*)target, nullptr, n4, per_sample / 4, lo,
                                                                    hi, w);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_distill_teacher_step(const float* z_t, const float* out1, const int64_t* t, const float* rows,
                                        const int64_t* t_mid_table, float* z_mid, float* x1c, int64_t* t_mid,
                                        int batch, int per_sample, float lo, float hi, tdx_stream_t stream) {
  return distill_teacher_step<false>(z_t, out1, t, rows, t_mid_table, z_mid, x1c, t_mid, batch, per_sample, 0.0f, lo,
                                     hi, stream);
}

extern "C" int tdx_distill_target(const float* z_t, const float* z_mid, const float* out2, const float* x1c,
                                  const int64_t* t, const float* rows, float* target, float* x_tilde, int batch,
                                  int per_sample, float lo, float hi, tdx_stream_t stream) {
  return distill_target<false>(z_t, z_mid, out2, x1c, t, rows, target, x_tilde, batch, per_sample, 0.0f, lo, hi,
                               stream);
}

extern "C" int tdx_distill_teacher_step_guided(const float* z_t, const float* out1, const int64_t* t,
                                               const float* rows, const int64_t* t_mid_table, float* z_mid,
                                               float* x1c, int64_t* t_mid, int batch, int per_sample, float w,
                                               float lo, float hi, tdx_stream_t stream) {
  if (!std::isfinite(w)) return TDX_E_BADARG;
  return distill_teacher_step<true>(z_t, out1, t, rows, t_mid_table, z_mid, x1c, t_mid, batch, per_sample, w, lo, hi,
                                    stream);
}

extern "C" int tdx_distill_target_guided(const float* z_t, const float* z_mid, const float* out2, const float* x1c,
                                         const int64_t* t, const float* rows, float* target, float* x_tilde,
                                         int batch, int per_sample, float w, float lo, float hi,
                                         tdx_stream_t stream) {
  if (!std::isfinite(w)) return TDX_E_BADARG;
  return distill_target<true>(z_t, z_mid, out2, x1c, t, rows, target, x_tilde, batch, per_sample, w, lo, hi, stream);
}

extern "C" int tdx_distill_guidance_target(const float* z_t, const float* out, const int64_t* t, const float* rows,
                                           float* target, float* x0c, int batch, int per_sample, int guided, float w,
                                           float lo, float hi, tdx_stream_t stream) {
  if (!z_t || !out || !t || !rows || !target || distill_bad_sizes(batch, per_sample, lo, hi)) return TDX_E_BADARG;
  if (guided && !std::isfinite(w)) return TDX_E_BADARG;   // w is not read without guidance
  if (guided) return distill_guidance_target<true>(z_t, out, t, rows, target, x0c, batch, per_sample, w, lo, hi, stream);
  return distill_guidance_target<false>(z_t, out, t, rows, target, x0c, batch, per_sample, 0.0f, lo, hi, stream);
}
