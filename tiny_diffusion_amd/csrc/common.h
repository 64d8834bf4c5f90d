// Shared host/device helpers for libtdx (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/tdx.h"

#define TDX_CHECK_LAUNCH()                           \
  do {                                               \
    hipError_t e__ = hipGetLastError();              \
    if (e__ != hipSuccess) return (int)e__;          \
  } while (0)

#define TDX_HIP(call)                                \
  do {                                               \
    hipError_t e__ = (call);                         \
    if (e__ != hipSuccess) return (int)e__;          \
  } while (0)

static inline hipStream_t to_stream(tdx_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- Philox4x32-10 (counter-based RNG), one 128-bit block per call ----------
struct Philox4 {
  uint32_t v[4];
};
__host__ __device__ static inline Philox4 philox4x32_10(uint64_t ctr_lo, uint64_t ctr_hi,
                                                        uint64_t key) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  uint32_t c0 = (uint32_t)ctr_lo, c1 = (uint32_t)(ctr_lo >> 32), c2 = (uint32_t)ctr_hi,
           c3 = (uint32_t)(ctr_hi >> 32);
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    uint32_t n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += W0; k1 += W1;
  }
  Philox4 o; o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
  return o;
}

// Four N(0,1) samples from one Philox block (Box-Muller, fp32).
__device__ static inline float4 philox_normal4(uint64_t ctr, uint64_t stream, uint64_t seed) {
  Philox4 r = philox4x32_10(ctr, stream, seed);
  const float S = 2.3283064365386963e-10f;  // 2^-32
  float u0 = ((float)r.v[0] + 0.5f) * S, u1 = ((float)r.v[1] + 0.5f) * S;
  float u2 = ((float)r.v[2] + 0.5f) * S, u3 = ((float)r.v[3] + 0.5f) * S;
  float ra = sqrtf(-2.0f * __logf(u0)), rb = sqrtf(-2.0f * __logf(u2));
  float sa, ca, sb, cb;
  __sincosf(6.283185307179586f * u1, &sa, &ca);
  __sincosf(6.283185307179586f * u3, &sb, &cb);
  return make_float4(ra * ca, ra * sa, rb * cb, rb * sb);
}

// x' = c1*(x - c2*eps) + sigma*z in the reference's operation order (diffusion.py:272-274): mul, sub, mul, mul, add,
// each rounded separately
__device__ static inline float p_step(float x, float e, float z, float c1, float c2, float sg) {
  float inner = __fsub_rn(x, __fmul_rn(c2, e));
  return __fadd_rn(__fmul_rn(c1, inner), __fmul_rn(sg, z));
}

// The x0-form updates (schedule.py x0_form / multistep_form) share three pieces, every product and sum rounded
// separately and in this order - a CPU fp32 tensor expression reproduces each bit for bit, as it does p_step.
// 1. The implied x0, clamped to [lo, hi] (clipped-x0 sampling, "static thresholding"; infinite bounds never bind):
//      x0c = min(max(p*x + q*out, lo), hi)
__device__ static inline float x0_clamped(float x, float o, float p, float q, float lo, float hi) {
  return fminf(fmaxf(__fadd_rn(__fmul_rn(p, x), __fmul_rn(q, o)), lo), hi);
}

// 1b. The same with a bound per sample (dynamic thresholding, include/tdx.h): u = x0 - c is clamped to the sample's
//      [-s, s], scaled back by r = h / s around the centre c of the data range, and clamped to [lo, hi]:
//      x0c = min(max(c + min(max(p*x + q*out - c, -s), s) * r, lo), hi)
// With s = h, r = 1 (the quantile does not exceed h) this is x0_clamped up to the sign of a zero.
__device__ static inline float x0_dyn_u(float x, float o, float p, float q, float c) {
  return __fsub_rn(__fadd_rn(__fmul_rn(p, x), __fmul_rn(q, o)), c);
}
__device__ static inline float x0_thresholded(float x, float o, float p, float q, float lo, float hi, float c, float s,
                                              float r) {
  const float v = fminf(fmaxf(x0_dyn_u(x, o, p, q, c), -s), s);
  return fminf(fmaxf(__fadd_rn(c, __fmul_rn(v, r)), lo), hi);
}

// 2. Inpainting: the blend with the caller's data between the clamp and the step,  x0m = (1 - m)*x0c + m*known.
// m == 1 gives `known` and m == 0 gives x0c bit for bit ((1-1)*x0c = +-0, 1*known = known; 1*x0c = x0c, 0*known = +-0:
// for finite operands); a fractional m is a soft edge.  `known` is not clamped.  The known region steps from x0 = known
// with the chain's own x and z - the posterior step of the forward process given x_0 = known.
__device__ static inline float x0_blend(float x0c, float known, float m) {
  return __fadd_rn(__fmul_rn(__fsub_rn(1.0f, m), x0c), __fmul_rn(m, known));
}

// 3a. The stochastic step from a (p, q, A, Bx, sigma) row:  x' = (A*x0 + Bx*x) + sigma*z.  On row 0 (A = 1, Bx = 0,
// z = 0) it returns x0 itself.
__device__ static inline float x0_step_noise(float x0, float x, float z, float A, float Bx, float sg) {
  return __fadd_rn(__fadd_rn(__fmul_rn(A, x0), __fmul_rn(Bx, x)), __fmul_rn(sg, z));
}

// 3b. The second-order multistep step (DPM-Solver++(2M), Lu et al. 2022) from a (p, q, A, Bx, H) row, with the x0 of
// the step before as history:  x' = (A*x0 + Bx*x) + H*hprev.  H == 0 (the first and the last step, every step of
// order 1): the history term is not added and the callers do not load hprev (H is uniform over a launch), so an
// uninitialised history buffer is harmless there.
__device__ static inline float x0_step_hist(float x0, float x, float hprev, float A, float Bx, float H) {
  float r = __fadd_rn(__fmul_rn(A, x0), __fmul_rn(Bx, x));
  if (H != 0.0f) r = __fadd_rn(r, __fmul_rn(H, hprev));
  return r;
}

// One row of a table: (S,5) rows (p, q, A, Bx, e = sigma | H), or the (S,3) rows (c1, c2, sigma) of p_step in A, Bx, e
struct PRow { float p, q, A, Bx, e; };
template <int FORM>
__device__ static inline PRow pstep_row(const float* coef, int t) {
  if (FORM == TDX_STEP_EPS) return PRow{0.f, 0.f, coef[3 * t + 0], coef[3 * t + 1], coef[3 * t + 2]};
  return PRow{coef[5 * t + 0], coef[5 * t + 1], coef[5 * t + 2], coef[5 * t + 3], coef[5 * t + 4]};
}

// The update of one element, for pstep_kernel (elementwise.hip) and the epilogue of final_conv (edge_conv.hip).  o: the
// network's output (guided: the cfg_eps combination); zh: the noise (EPS, X0; 0 for none) or the history (MS; not
// loaded when r.e == 0); known / m: read when MK only.  MS: *x0_out is what the caller stores as the next step's
// history - the BLENDED prediction when MK, which keeps the known region on the forward marginal of the deterministic
// chain (with the clamped prediction as history it leaves it).  DT (X0, MS): the clamp is x0_thresholded with the
// sample's (s, r) and the centre c.
template <int FORM, bool MK, bool DT = false>
__device__ static inline float pstep_elem(float x, float o, float zh, float known, float m, const PRow& r, float lo,
                                          float hi, float* x0_out, float c = 0.f, float ts = 0.f, float tr = 0.f) {
  if (FORM == TDX_STEP_EPS) return p_step(x, o, zh, r.A, r.Bx, r.e);
  float x0 = DT ? x0_thresholded(x, o, r.p, r.q, lo, hi, c, ts, tr) : x0_clamped(x, o, r.p, r.q, lo, hi);
  if (MK) x0 = x0_blend(x0, known, m);
  if (FORM == TDX_STEP_MS) *x0_out = x0;
  return FORM == TDX_STEP_MS ? x0_step_hist(x0, x, zh, r.A, r.Bx, r.e) : x0_step_noise(x0, x, zh, r.A, r.Bx, r.e);
}

// classifier-free guidance (Ho & Salimans 2021): eps_u + w (eps_c - eps_u), each operation rounded separately - the
// one expression both guided updates evaluate (elementwise.hip, the epilogue of final_conv in edge_conv.hip)
__device__ static inline float cfg_eps(float e_c, float e_u, float w) {
  return __fadd_rn(e_u, __fmul_rn(w, __fsub_rn(e_c, e_u)));
}

__device__ static inline float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
