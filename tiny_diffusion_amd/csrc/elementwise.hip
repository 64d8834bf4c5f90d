// HBM-bound elementwise kernels of the DDPM path: q_sample (diffusion.py:177-190),
// the reverse-process update (diffusion.py:272-274), MSE loss (diffusion.py:231),
// Adam (diffusion.py:211/236), plus the roofline probes used by bench.py.
#include "internal.h"

// ------------------------------------------------------------------ q_sample
// x_t = sqrt_ac[t[n]] * x0 + sqrt_1mac[t[n]] * noise ; 16 B per lane per tensor.
__global__ void q_sample_kernel(const float4* __restrict__ x0, const float4* __restrict__ noise,
                                const int64_t* __restrict__ t, const float* __restrict__ sqrt_ac,
                                const float* __restrict__ sqrt_1mac, float4* __restrict__ x_t,
                                int64_t n4, int per_sample4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    int s = (int)(i / per_sample4);
    int64_t ts = t[s];
    float a = sqrt_ac[ts], b = sqrt_1mac[ts];
    float4 x = x0[i], e = noise[i], o;
    // two roundings per term like the reference's a*x0 + b*noise (no fma contraction)
    o.x = __fadd_rn(__fmul_rn(a, x.x), __fmul_rn(b, e.x));
    o.y = __fadd_rn(__fmul_rn(a, x.y), __fmul_rn(b, e.y));
    o.z = __fadd_rn(__fmul_rn(a, x.z), __fmul_rn(b, e.z));
    o.w = __fadd_rn(__fmul_rn(a, x.w), __fmul_rn(b, e.w));
    x_t[i] = o;
  }
}

__global__ void q_sample_philox_kernel(const float4* __restrict__ x0, const int64_t* __restrict__ t,
                                       const float* __restrict__ sqrt_ac,
                                       const float* __restrict__ sqrt_1mac,
                                       float4* __restrict__ x_t, float4* __restrict__ noise_out,
                                       int64_t n4, int per_sample4, uint64_t seed, uint64_t offset) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    int s = (int)(i / per_sample4);
    int64_t ts = t[s];
    float a = sqrt_ac[ts], b = sqrt_1mac[ts];
    float4 e = philox_normal4((uint64_t)i, offset, seed);
    float4 x = x0[i], o;
    o.x = __fadd_rn(__fmul_rn(a, x.x), __fmul_rn(b, e.x));
    o.y = __fadd_rn(__fmul_rn(a, x.y), __fmul_rn(b, e.y));
    o.z = __fadd_rn(__fmul_rn(a, x.z), __fmul_rn(b, e.z));
    o.w = __fadd_rn(__fmul_rn(a, x.w), __fmul_rn(b, e.w));
    x_t[i] = o;
    noise_out[i] = e;
  }
}

static int ew_grid(int64_t n_items, int block) {
  int64_t g = (n_items + block - 1) / block;
  if (g > 2048) g = 2048;  // 256 CUs x 8 blocks, grid-stride the rest
  if (g < 1) g = 1;
  return (int)g;
}

extern "C" int tdx_q_sample(const float* x0, const float* noise, const int64_t* t,
                            const float* sqrt_ac, const float* sqrt_1mac, float* x_t, int batch,
                            int per_sample, tdx_stream_t stream) {
  if (!x0 || !noise || !t || !sqrt_ac || !sqrt_1mac || !x_t || batch <= 0 || per_sample <= 0)
    return TDX_E_BADARG;
  if (per_sample % 4) return TDX_E_SHAPE;
  int64_t n4 = (int64_t)batch * per_sample / 4;
  q_sample_kernel<<<ew_grid(n4, 256), 256, 0, to_stream(stream)>>>(
      (const float4*)x0, (const float4*)noise, t, sqrt_ac, sqrt_1mac, (float4*)x_t, n4,
      per_sample / 4);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_q_sample_philox(const float* x0, const int64_t* t, const float* sqrt_ac,
                                   const float* sqrt_1mac, float* x_t, float* noise_out, int batch,
                                   int per_sample, uint64_t seed, uint64_t offset,
                                   tdx_stream_t stream) {
  if (!x0 || !t || !sqrt_ac || !sqrt_1mac || !x_t || !noise_out || batch <= 0 || per_sample <= 0)
    return TDX_E_BADARG;
  if (per_sample % 4) return TDX_E_SHAPE;
  int64_t n4 = (int64_t)batch * per_sample / 4;
  q_sample_philox_kernel<<<ew_grid(n4, 256), 256, 0, to_stream(stream)>>>(
      (const float4*)x0, t, sqrt_ac, sqrt_1mac, (float4*)x_t, (float4*)noise_out, n4,
      per_sample / 4, seed, offset);
  TDX_CHECK_LAUNCH();
  return 0;
}

// q_sample that also writes the training target of the chosen parameterisation (TrainStep(prediction=...)):
// kind 0 (eps): target = noise; kind 1 (v, Salimans & Ho 2022): target = a*noise - b*x0, the two products and the
// subtraction rounded separately like x_t.  x_t is the expression of q_sample_kernel, element for element.
// noise / target carry no __restrict__: target may be the noise buffer (each lane reads its element before it writes
// it).  target == null (kind 0 in place): nothing to write.
#define TDX_TARGET_EPS 0
#define TDX_TARGET_V 1

__device__ __forceinline__ float4 q_mix(float a, float b, const float4 x, const float4 e) {
  float4 o;
  o.x = __fadd_rn(__fmul_rn(a, x.x), __fmul_rn(b, e.x));
  o.y = __fadd_rn(__fmul_rn(a, x.y), __fmul_rn(b, e.y));
  o.z = __fadd_rn(__fmul_rn(a, x.z), __fmul_rn(b, e.z));
  o.w = __fadd_rn(__fmul_rn(a, x.w), __fmul_rn(b, e.w));
  return o;
}

__device__ __forceinline__ float4 v_target(float a, float b, const float4 x, const float4 e) {
  float4 o;
  o.x = __fsub_rn(__fmul_rn(a, e.x), __fmul_rn(b, x.x));
  o.y = __fsub_rn(__fmul_rn(a, e.y), __fmul_rn(b, x.y));
  o.z = __fsub_rn(__fmul_rn(a, e.z), __fmul_rn(b, x.z));
  o.w = __fsub_rn(__fmul_rn(a, e.w), __fmul_rn(b, x.w));
  return o;
}

template <bool PHILOX>
__global__ void __launch_bounds__(256)
q_sample_target_kernel(const float4* __restrict__ x0, const float4* noise, const int64_t* __restrict__ t,
                       const float* __restrict__ sqrt_ac, const float* __restrict__ sqrt_1mac,
                       float4* __restrict__ x_t, float4* target, int64_t n4, int per_sample4, int kind,
                       uint64_t seed, uint64_t offset) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    int s = (int)(i / per_sample4);
    int64_t ts = t[s];
    float a = sqrt_ac[ts], b = sqrt_1mac[ts];
    const float4 e = PHILOX ? philox_normal4((uint64_t)i, offset, seed) : noise[i];
    const float4 x = x0[i];
    x_t[i] = q_mix(a, b, x, e);
    if (target) target[i] = kind == TDX_TARGET_V ? v_target(a, b, x, e) : e;
  }
}

extern "C" int tdx_q_sample_target(const float* x0, const float* noise, const int64_t* t, const float* sqrt_ac,
                                   const float* sqrt_1mac, float* x_t, float* target, int batch, int per_sample,
                                   int kind, tdx_stream_t stream) {
  if (!x0 || !noise || !t || !sqrt_ac || !sqrt_1mac || !x_t || !target || batch <= 0 || per_sample <= 0)
    return TDX_E_BADARG;
  if (kind != TDX_TARGET_EPS && kind != TDX_TARGET_V) return TDX_E_BADARG;
  if (per_sample % 4) return TDX_E_SHAPE;
  int64_t n4 = (int64_t)batch * per_sample / 4;
  // the eps target in place is the noise as it stands
  float4* tg = (kind == TDX_TARGET_EPS && target == noise) ? nullptr : (float4*)target;
  q_sample_target_kernel<false><<<ew_grid(n4, 256), 256, 0, to_stream(stream)>>>(
      (const float4*)x0, (const float4*)noise, t, sqrt_ac, sqrt_1mac, (float4*)x_t, tg, n4, per_sample / 4, kind, 0, 0);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_q_sample_target_philox(const float* x0, const int64_t* t, const float* sqrt_ac,
                                          const float* sqrt_1mac, float* x_t, float* target, int batch,
                                          int per_sample, int kind, uint64_t seed, uint64_t offset,
                                          tdx_stream_t stream) {
  if (!x0 || !t || !sqrt_ac || !sqrt_1mac || !x_t || !target || batch <= 0 || per_sample <= 0)
    return TDX_E_BADARG;
  if (kind != TDX_TARGET_EPS && kind != TDX_TARGET_V) return TDX_E_BADARG;
  if (per_sample % 4) return TDX_E_SHAPE;
  int64_t n4 = (int64_t)batch * per_sample / 4;
  q_sample_target_kernel<true><<<ew_grid(n4, 256), 256, 0, to_stream(stream)>>>(
      (const float4*)x0, nullptr, t, sqrt_ac, sqrt_1mac, (float4*)x_t, (float4*)target, n4, per_sample / 4, kind, seed,
      offset);
  TDX_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------- p_sample step
// One reverse-process update (PStep, internal.h) over n4 float4, grid-strided; xo may alias x (in-place update).
// t = the coefficient row.  With a timestep schedule (tau != null, DDIM) it is the step index k and the Philox stream
// is the network's timestep tau[k], so the identity schedule draws the identity chain's noise; block i, component of
// the float4.  The noise term is skipped at t == 0 (diffusion.py:267-270) and MS has none: H is uniform over the
// launch and at H == 0 the history is not loaded at all (the first step's buffer may hold anything).  An element's
// history is read and written by the same thread, as x is when xo aliases it.
// GD: x and out hold 2 n4 float4 whose halves ran under the caller's and under the null condition; the two outputs are
// combined first (cfg_eps is linear in the network's output, whatever it predicts) and the one update is written to
// both halves.  z, hist, known, mask and the Philox index are the first half's - the guided chain of n samples
// consumes the stream of the unguided chain of n samples.
// DT (X0, MS): dynamic thresholding - float4 i lies in sample i / (per / 4) (per % 4 == 0: it never straddles two), whose
// (s, r) x0_threshold_kernel wrote to s.thr before this launch.
template <int FORM, bool GD, bool MK, bool PHILOX, bool DT = false>
__global__ void pstep_kernel(float4* xo, const float4* x, const float4* __restrict__ out, int64_t n4, const PStep s) {
  const float4* __restrict__ z = (const float4*)s.z;
  const float4* __restrict__ known = (const float4*)s.known;
  const float4* __restrict__ mask = (const float4*)s.mask;
  float4* hist = (float4*)s.hist;
  const int t = *s.t_idx;
  const uint64_t nt = s.tau ? (uint64_t)s.tau[t] : (uint64_t)t;
  // table-mode sampling (tdx_unet_eval_step): the step counter is advanced HERE, by the last kernel of the
  // step, because the head kernel of the step reads it from every workgroup (nobody else touches it in between)
  if (s.counter_dec && blockIdx.x == 0 && threadIdx.x == 0) *s.counter_dec = (int64_t)t - 1;
  const PRow r = pstep_row<FORM>(s.coef, t);
  const float w = s.w, lo = s.lo, hi = s.hi;
  const float2* __restrict__ thr = (const float2*)s.thr;
  const int64_t per4 = s.per >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float4 xv = x[i];
    float2 sr = make_float2(0.f, 0.f);
    if (DT) sr = thr[i / per4];
    float4 e = out[i], zh = make_float4(0.f, 0.f, 0.f, 0.f), kn = zh, mv = zh, o, h;
    if (FORM == TDX_STEP_MS) {
      if (r.e != 0.0f) zh = hist[i];
    } else if (PHILOX) {
      if (t > 0) zh = philox_normal4((uint64_t)i, nt, s.seed);
    } else if (z && t > 0) {
      zh = z[i];
    }
    if (MK) { kn = known[i]; mv = mask[i]; }
    if (GD) {
      const float4 eu = out[i + n4];
      e.x = cfg_eps(e.x, eu.x, w);
      e.y = cfg_eps(e.y, eu.y, w);
      e.z = cfg_eps(e.z, eu.z, w);
      e.w = cfg_eps(e.w, eu.w, w);
    }
    o.x = pstep_elem<FORM, MK, DT>(xv.x, e.x, zh.x, kn.x, mv.x, r, lo, hi, &h.x, s.c, sr.x, sr.y);
    o.y = pstep_elem<FORM, MK, DT>(xv.y, e.y, zh.y, kn.y, mv.y, r, lo, hi, &h.y, s.c, sr.x, sr.y);
    o.z = pstep_elem<FORM, MK, DT>(xv.z, e.z, zh.z, kn.z, mv.z, r, lo, hi, &h.z, s.c, sr.x, sr.y);
    o.w = pstep_elem<FORM, MK, DT>(xv.w, e.w, zh.w, kn.w, mv.w, r, lo, hi, &h.w, s.c, sr.x, sr.y);
    xo[i] = o;
    if (GD) xo[i + n4] = o;
    if (FORM == TDX_STEP_MS) hist[i] = h;
  }
}

// the 16 live instantiations: EPS has no masked update, MS no noise (one value of PHILOX); and the 12 of X0 and MS
// once more with the thresholded clamp (s.thr)
template <int FORM, bool GD, bool MK, bool PHILOX>
static void pstep_launch_thr(const PStep& s, float4* xo, const float4* x, const float4* out, int64_t n4, hipStream_t st) {
  const int grid = ew_grid(n4, 256);
  if constexpr (FORM != TDX_STEP_EPS) {
    if (s.thr) {
      pstep_kernel<FORM, GD, MK, PHILOX, true><<<grid, 256, 0, st>>>(xo, x, out, n4, s);
      return;
    }
  }
  pstep_kernel<FORM, GD, MK, PHILOX><<<grid, 256, 0, st>>>(xo, x, out, n4, s);
}
template <int FORM, bool GD, bool MK>
static void pstep_launch_noise(const PStep& s, float4* xo, const float4* x, const float4* out, int64_t n4, hipStream_t st) {
  if constexpr (FORM != TDX_STEP_MS) {
    if (s.philox) {
      pstep_launch_thr<FORM, GD, MK, true>(s, xo, x, out, n4, st);
      return;
    }
  }
  pstep_launch_thr<FORM, GD, MK, false>(s, xo, x, out, n4, st);
}
template <int FORM>
static void pstep_launch_form(const PStep& s, float4* xo, const float4* x, const float4* out, int64_t n4, hipStream_t st) {
  if (FORM != TDX_STEP_EPS && s.known) {
    if (s.guided) pstep_launch_noise<FORM, true, FORM != TDX_STEP_EPS>(s, xo, x, out, n4, st);
    else pstep_launch_noise<FORM, false, FORM != TDX_STEP_EPS>(s, xo, x, out, n4, st);
  } else {
    if (s.guided) pstep_launch_noise<FORM, true, false>(s, xo, x, out, n4, st);
    else pstep_launch_noise<FORM, false, false>(s, xo, x, out, n4, st);
  }
}

int tdx_pstep_launch(const PStep& s, float* x_out, const float* x, const float* out, int64_t n, hipStream_t st) {
  if (!x_out || !x || !out || (s.guided && x_out != x)) return TDX_E_BADARG;
  const int rc = pstep_valid(s, n);
  if (rc) return rc;
  if (s.form == TDX_STEP_EPS) pstep_launch_form<TDX_STEP_EPS>(s, (float4*)x_out, (const float4*)x, (const float4*)out, n / 4, st);
  else if (s.form == TDX_STEP_X0) pstep_launch_form<TDX_STEP_X0>(s, (float4*)x_out, (const float4*)x, (const float4*)out, n / 4, st);
  else pstep_launch_form<TDX_STEP_MS>(s, (float4*)x_out, (const float4*)x, (const float4*)out, n / 4, st);
  TDX_CHECK_LAUNCH();
  return 0;
}

static PStep pstep_of(int form, const float* coef, const int32_t* t_idx, const int64_t* tau, const float* z, int philox,
                      uint64_t seed, int guided, float w, float lo, float hi, float* hist, const float* known,
                      const float* mask, int64_t* counter_dec) {
  PStep s{};
  s.form = form; s.coef = coef; s.t_idx = t_idx; s.tau = tau;
  s.z = z; s.philox = philox != 0; s.seed = seed;
  s.guided = guided != 0; s.w = w;
  s.lo = lo; s.hi = hi;
  s.hist = hist; s.known = known; s.mask = mask; s.counter_dec = counter_dec;
  return s;
}

extern "C" int tdx_p_sample_update(float* x_out, const float* x, const float* out, int64_t n, int form,
                                   const float* coef, const int32_t* t_idx, const int64_t* tau, const float* z,
                                   int use_philox, uint64_t philox_seed, int guided, float w, float lo, float hi,
                                   float* hist, const float* known, const float* mask, int64_t* counter_dec,
                                   tdx_stream_t stream) {
  const PStep s = pstep_of(form, coef, t_idx, tau, z, use_philox, philox_seed, guided, w, lo, hi, hist, known, mask,
                           counter_dec);
  return tdx_pstep_launch(s, x_out, x, out, n, to_stream(stream)) ? TDX_E_BADARG : 0;
}

extern "C" int tdx_p_sample_update_dyn(float* x_out, const float* x, const float* out, int64_t n, int form,
                                       const float* coef, const int32_t* t_idx, const int64_t* tau, const float* z,
                                       int use_philox, uint64_t philox_seed, int guided, float w, float lo, float hi,
                                       float* hist, const float* known, const float* mask, int64_t* counter_dec,
                                       float* thr, int per, tdx_stream_t stream) {
  if (!thr) return TDX_E_BADARG;
  PStep s = pstep_of(form, coef, t_idx, tau, z, use_philox, philox_seed, guided, w, lo, hi, hist, known, mask,
                     counter_dec);
  s.thr = thr; s.per = per; s.c = dyn_centre(lo, hi);
  return tdx_pstep_launch(s, x_out, x, out, n, to_stream(stream)) ? TDX_E_BADARG : 0;
}

// ------------------------------------------------------- dynamic thresholding
// (s_b, r_b) of include/tdx.h for sample b = blockIdx.x: the key of element j is the bit pattern of |u_j| (ordered as the
// floats are, a NaN last), and a[rank] is found by radix selection, most significant byte first.  Each of the four
// passes recomputes the keys from x / out (a sample is L2-resident; keeping per / 256 keys per thread in registers would
// fix `per` at compile time), counts the byte under inspection of the keys that match the bytes chosen so far in an
// LDS histogram, and a block-wide scan of the 256 counts picks the bin that holds the rank.  Integer LDS adds only:
// the result does not depend on the order of arrival.  A sample's keys crowd into a few bins (the exponent byte in the
// first pass), so every bin is kept THR_REP times, in THR_REP different banks, lane % THR_REP choosing the copy: a wave's
// adds to one bin serialise 64 / THR_REP deep, not 64.  a[rank + 1] comes from the last pass: it is a[rank] again when
// the bins up to the chosen one hold more than the rank left over + 1 keys; otherwise the lowest occupied bin above
// it or, when there is none, the smallest key with higher upper bytes (a minimum each thread keeps in that pass).
// Thread t owns bin t: the block size is the number of bins.
#define THR_BLOCK 256
#define THR_REP 16

template <bool GD>
__device__ __forceinline__ void thr_keys(const float4* __restrict__ x, const float4* __restrict__ oc,
                                         const float4* __restrict__ ou, int i, float p, float q, float c, float w,
                                         uint32_t k[4]) {
  const float4 xv = x[i];
  float4 e = oc[i];
  if (GD) {
    const float4 eu = ou[i];
    e.x = cfg_eps(e.x, eu.x, w);
    e.y = cfg_eps(e.y, eu.y, w);
    e.z = cfg_eps(e.z, eu.z, w);
    e.w = cfg_eps(e.w, eu.w, w);
  }
  k[0] = __float_as_uint(x0_dyn_u(xv.x, e.x, p, q, c)) & 0x7fffffffu;
  k[1] = __float_as_uint(x0_dyn_u(xv.y, e.y, p, q, c)) & 0x7fffffffu;
  k[2] = __float_as_uint(x0_dyn_u(xv.z, e.z, p, q, c)) & 0x7fffffffu;
  k[3] = __float_as_uint(x0_dyn_u(xv.w, e.w, p, q, c)) & 0x7fffffffu;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t u = (uint32_t)__shfl_xor((int)v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}

template <bool GD>
__global__ void __launch_bounds__(THR_BLOCK)
x0_threshold_kernel(const float* __restrict__ x, const float* __restrict__ out, int n_samples, int per,
                    const float* __restrict__ coef5, const int32_t* __restrict__ t_idx, float w, float c, float h,
                    int rank, float frac, float2* __restrict__ thr) {
  __shared__ uint32_t hist[256 * THR_REP];
  __shared__ uint32_t wtot[THR_BLOCK / 64], wmin[THR_BLOCK / 64];
  __shared__ uint32_t sel[3];   // the chosen bin, the rank left inside it, whether the next key up equals the chosen one
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int t = *t_idx;
  const float p = coef5[5 * t + 0], q = coef5[5 * t + 1];
  const int per4 = per >> 2;
  const float4* xs = (const float4*)(x + (int64_t)b * per);
  const float4* oc = (const float4*)(out + (int64_t)b * per);
  const float4* ou = (const float4*)(out + ((int64_t)n_samples + b) * per);   // read when GD only
  uint32_t prefix = 0, left = (uint32_t)rank, cnt = 0;
  uint32_t above = 0xffffffffu;   // last pass: the smallest key whose upper three bytes exceed the chosen ones
  if (tid < 3) sel[tid] = 0;      // (every pass, one thread writes all three: valid arguments always select a bin)
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int j = tid; j < 256 * THR_REP; j += THR_BLOCK) hist[j] = 0;
    __syncthreads();
    for (int i = tid; i < per4; i += THR_BLOCK) {
      uint32_t k[4];
      thr_keys<GD>(xs, oc, ou, i, p, q, c, w, k);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t upper = pass ? k[e] >> (shift + 8) : 0u;
        if (upper == prefix) atomicAdd(&hist[((k[e] >> shift) & 255u) * THR_REP + (lane & (THR_REP - 1))], 1u);
        else if (pass == 3 && upper > prefix && k[e] < above) above = k[e];
      }
    }
    __syncthreads();
    cnt = 0;
#pragma unroll
    for (int r = 0; r < THR_REP; ++r) cnt += hist[tid * THR_REP + r];
    uint32_t incl = cnt;   // inclusive scan over the bins: within the wave, then across the waves
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    for (int v = 0; v < wave; ++v) incl += wtot[v];
    const uint32_t excl = incl - cnt;
    if (cnt && excl <= left && left < incl) {   // one thread: the counts of the matching keys sum to more than `left`
      sel[0] = (uint32_t)tid;
      sel[1] = left - excl;
      sel[2] = incl > left + 1u;
    }
    __syncthreads();
    prefix = (prefix << 8) | sel[0];
    left = sel[1];
  }
  // prefix is the key a[rank]; the candidates for a[rank + 1] above it
  const uint32_t bin = prefix & 255u;
  uint32_t cand = above;
  if ((uint32_t)tid > bin && cnt) cand = (prefix & ~255u) | (uint32_t)tid;   // below every key with higher upper bytes
  cand = wave_min_u32(cand);
  if (lane == 0) wmin[wave] = cand;
  __syncthreads();
  if (tid == 0) {
    uint32_t nxt = wmin[0];
#pragma unroll
    for (int v = 1; v < THR_BLOCK / 64; ++v) nxt = wmin[v] < nxt ? wmin[v] : nxt;
    if (sel[2] || rank + 1 >= per || nxt == 0xffffffffu) nxt = prefix;
    const float a0 = __uint_as_float(prefix), a1 = __uint_as_float(nxt);
    const float sq = __fadd_rn(a0, __fmul_rn(frac, __fsub_rn(a1, a0)));
    const float s = !(sq <= h) ? sq : h;   // max(s_q, h); a NaN quantile is written as it is
    thr[b] = make_float2(s, __fdiv_rn(h, s));
  }
}

int tdx_x0_threshold_launch(const PStep& s, const float* x, const float* out, int n_samples, int rank, float frac,
                            hipStream_t st) {
  if (!x || !out || !s.coef || !s.t_idx || !s.thr || n_samples <= 0 || s.per <= 0 || s.per % 4) return TDX_E_BADARG;
  if (!(s.lo < s.hi) || !std::isfinite(s.lo) || !std::isfinite(s.hi) || !std::isfinite(s.hi - s.lo)) return TDX_E_BADARG;
  if (rank < 0 || rank >= s.per || !(frac >= 0.0f && frac <= 1.0f)) return TDX_E_BADARG;
  const float c = dyn_centre(s.lo, s.hi), h = dyn_half(s.lo, s.hi);
  if (s.guided)
    x0_threshold_kernel<true><<<n_samples, THR_BLOCK, 0, st>>>(x, out, n_samples, s.per, s.coef, s.t_idx, s.w, c, h,
                                                               rank, frac, (float2*)s.thr);
  else
    x0_threshold_kernel<false><<<n_samples, THR_BLOCK, 0, st>>>(x, out, n_samples, s.per, s.coef, s.t_idx, s.w, c, h,
                                                                rank, frac, (float2*)s.thr);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_x0_dyn_threshold(const float* x, const float* out, int n_samples, int per, const float* coef5,
                                    const int32_t* t_idx, int guided, float w, float lo, float hi, int rank, float frac,
                                    float* thr, tdx_stream_t stream) {
  PStep s{};
  s.coef = coef5; s.t_idx = t_idx;
  s.guided = guided != 0; s.w = w;
  s.lo = lo; s.hi = hi;
  s.thr = thr; s.per = per;
  return tdx_x0_threshold_launch(s, x, out, n_samples, rank, frac, to_stream(stream)) ? TDX_E_BADARG : 0;
}

// The entries of each form (include/tdx.h): the null checks that are the entry's own, then the one launcher.
extern "C" int tdx_p_sample_step(float* x_out, const float* x, const float* eps, const float* z,
                                 const float* coef, const int32_t* t_idx, int64_t n,
                                 tdx_stream_t stream) {
  const PStep s = pstep_of(TDX_STEP_EPS, coef, t_idx, nullptr, z, 0, 0, 0, 0.f, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr);
  return tdx_pstep_launch(s, x_out, x, eps, n, to_stream(stream));
}

extern "C" int tdx_p_sample_step_philox(float* x_out, const float* x, const float* eps,
                                        const float* coef, const int32_t* t_idx, int64_t n,
                                        uint64_t seed, tdx_stream_t stream) {
  const PStep s = pstep_of(TDX_STEP_EPS, coef, t_idx, nullptr, nullptr, 1, seed, 0, 0.f, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr);
  return tdx_pstep_launch(s, x_out, x, eps, n, to_stream(stream));
}

extern "C" int tdx_p_sample_step_sched(float* x_out, const float* x, const float* eps, const float* z,
                                       const float* coef, const int64_t* tau, const int32_t* k_idx, int64_t n,
                                       tdx_stream_t stream) {
  if (!tau) return TDX_E_BADARG;
  const PStep s = pstep_of(TDX_STEP_EPS, coef, k_idx, tau, z, 0, 0, 0, 0.f, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr);
  return tdx_pstep_launch(s, x_out, x, eps, n, to_stream(stream));
}

extern "C" int tdx_p_sample_step_sched_philox(float* x_out, const float* x, const float* eps, const float* coef,
                                              const int64_t* tau, const int32_t* k_idx, int64_t n, uint64_t seed,
                                              tdx_stream_t stream) {
  if (!tau) return TDX_E_BADARG;
  const PStep s = pstep_of(TDX_STEP_EPS, coef, k_idx, tau, nullptr, 1, seed, 0, 0.f, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr);
  return tdx_pstep_launch(s, x_out, x, eps, n, to_stream(stream));
}

extern "C" int tdx_p_sample_step_guided(float* x, const float* eps, const float* z, const float* coef,
                                        const int64_t* tau, const int32_t* t_idx, int64_t n_half_elems, float w,
                                        int use_philox, uint64_t philox_seed, int64_t* counter_dec,
                                        tdx_stream_t stream) {
  const PStep s = pstep_of(TDX_STEP_EPS, coef, t_idx, tau, z, use_philox, philox_seed, 1, w, 0.f, 0.f, nullptr, nullptr, nullptr, counter_dec);
  return tdx_pstep_launch(s, x, x, eps, n_half_elems, to_stream(stream));
}

extern "C" int tdx_p_sample_step_x0(float* x_out, const float* x, const float* out, const float* z, const float* coef5,
                                    const int64_t* tau, const int32_t* t_idx, int64_t n, float lo, float hi,
                                    int use_philox, uint64_t philox_seed, int64_t* counter_dec, tdx_stream_t stream) {
  const PStep s = pstep_of(TDX_STEP_X0, coef5, t_idx, tau, z, use_philox, philox_seed, 0, 0.f, lo, hi, nullptr, nullptr, nullptr, counter_dec);
  return tdx_pstep_launch(s, x_out, x, out, n, to_stream(stream));
}

extern "C" int tdx_p_sample_step_x0_guided(float* x, const float* out, const float* z, const float* coef5,
                                           const int64_t* tau, const int32_t* t_idx, int64_t n_half_elems, float w,
                                           float lo, float hi, int use_philox, uint64_t philox_seed,
                                           int64_t* counter_dec, tdx_stream_t stream) {
  const PStep s = pstep_of(TDX_STEP_X0, coef5, t_idx, tau, z, use_philox, philox_seed, 1, w, lo, hi, nullptr, nullptr, nullptr, counter_dec);
  return tdx_pstep_launch(s, x, x, out, n_half_elems, to_stream(stream));
}

extern "C" int tdx_p_sample_step_ms(float* x_out, const float* x, const float* out, float* hist, const float* coef5,
                                    const int32_t* t_idx, int64_t n, float lo, float hi, int64_t* counter_dec,
                                    tdx_stream_t stream) {
  const PStep s = pstep_of(TDX_STEP_MS, coef5, t_idx, nullptr, nullptr, 0, 0, 0, 0.f, lo, hi, hist, nullptr, nullptr, counter_dec);
  return tdx_pstep_launch(s, x_out, x, out, n, to_stream(stream));
}

extern "C" int tdx_p_sample_step_ms_guided(float* x, const float* out, float* hist, const float* coef5,
                                           const int32_t* t_idx, int64_t n_half_elems, float w, float lo, float hi,
                                           int64_t* counter_dec, tdx_stream_t stream) {
  const PStep s = pstep_of(TDX_STEP_MS, coef5, t_idx, nullptr, nullptr, 0, 0, 1, w, lo, hi, hist, nullptr, nullptr, counter_dec);
  return tdx_pstep_launch(s, x, x, out, n_half_elems, to_stream(stream));
}

extern "C" int tdx_p_sample_step_x0_masked(float* x_out, const float* x, const float* out, const float* z,
                                           const float* known, const float* mask, const float* coef5,
                                           const int64_t* tau, const int32_t* t_idx, int64_t n, float lo, float hi,
                                           int use_philox, uint64_t philox_seed, int64_t* counter_dec,
                                           tdx_stream_t stream) {
  if (!known || !mask) return TDX_E_BADARG;
  const PStep s = pstep_of(TDX_STEP_X0, coef5, t_idx, tau, z, use_philox, philox_seed, 0, 0.f, lo, hi, nullptr, known, mask, counter_dec);
  return tdx_pstep_launch(s, x_out, x, out, n, to_stream(stream));
}

extern "C" int tdx_p_sample_step_x0_guided_masked(float* x, const float* out, const float* z, const float* known,
                                                  const float* mask, const float* coef5, const int64_t* tau,
                                                  const int32_t* t_idx, int64_t n_half_elems, float w, float lo,
                                                  float hi, int use_philox, uint64_t philox_seed, int64_t* counter_dec,
                                                  tdx_stream_t stream) {
  if (!known || !mask) return TDX_E_BADARG;
  const PStep s = pstep_of(TDX_STEP_X0, coef5, t_idx, tau, z, use_philox, philox_seed, 1, w, lo, hi, nullptr, known, mask, counter_dec);
  return tdx_pstep_launch(s, x, x, out, n_half_elems, to_stream(stream));
}

extern "C" int tdx_p_sample_step_ms_masked(float* x_out, const float* x, const float* out, float* hist,
                                           const float* known, const float* mask, const float* coef5,
                                           const int32_t* t_idx, int64_t n, float lo, float hi, int64_t* counter_dec,
                                           tdx_stream_t stream) {
  if (!known || !mask) return TDX_E_BADARG;
  const PStep s = pstep_of(TDX_STEP_MS, coef5, t_idx, nullptr, nullptr, 0, 0, 0, 0.f, lo, hi, hist, known, mask, counter_dec);
  return tdx_pstep_launch(s, x_out, x, out, n, to_stream(stream));
}

extern "C" int tdx_p_sample_step_ms_guided_masked(float* x, const float* out, float* hist, const float* known,
                                                  const float* mask, const float* coef5, const int32_t* t_idx,
                                                  int64_t n_half_elems, float w, float lo, float hi,
                                                  int64_t* counter_dec, tdx_stream_t stream) {
  if (!known || !mask) return TDX_E_BADARG;
  const PStep s = pstep_of(TDX_STEP_MS, coef5, t_idx, nullptr, nullptr, 0, 0, 1, w, lo, hi, hist, known, mask, counter_dec);
  return tdx_pstep_launch(s, x, x, out, n_half_elems, to_stream(stream));
}

// Device-side step counter for graph-captured sampling: t = *counter; t_idx = t; t_vec[:] = t;
// *counter = t - 1.  One block; lets a HIP graph hold several consecutive reverse steps with no
// host work between them (diffusion.py:259-260 builds the same t tensor on the host each step).
// tau != null (timestep schedule): the counter is the step index k, t_idx = k, t_vec[:] = tau[k].
__global__ void step_begin_kernel(int64_t* __restrict__ counter, int32_t* __restrict__ t_idx,
                                  int64_t* __restrict__ t_vec, int n, const int64_t* __restrict__ tau = nullptr) {
  const int64_t t = *counter;
  const int64_t tv = tau ? tau[t] : t;
  for (int i = threadIdx.x; i < n; i += blockDim.x) t_vec[i] = tv;
  __syncthreads();
  if (threadIdx.x == 0) {
    *t_idx = (int32_t)t;
    *counter = t - 1;
  }
}

extern "C" int tdx_step_begin(int64_t* counter, int32_t* t_idx, int64_t* t_vec, int n, tdx_stream_t stream) {
  if (!counter || !t_idx || !t_vec || n <= 0) return TDX_E_BADARG;
  step_begin_kernel<<<1, 256, 0, to_stream(stream)>>>(counter, t_idx, t_vec, n);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_step_begin_sched(int64_t* counter, const int64_t* tau, int32_t* t_idx, int64_t* t_vec, int n,
                                    tdx_stream_t stream) {
  if (!counter || !tau || !t_idx || !t_vec || n <= 0) return TDX_E_BADARG;
  step_begin_kernel<<<1, 256, 0, to_stream(stream)>>>(counter, t_idx, t_vec, n, tau);
  TDX_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------- on-device input path
// out[b] = ((u8[idx[b]] / 255) - mean) / std : torchvision ToTensor + Normalize((0.5,),(0.5,))
// (diffusion.py:202-204) fused with the minibatch gather, so the whole uint8 dataset
// (MNIST: 47 MB) stays in HBM and no host DataLoader sits in front of the training step.
// Same operation order and IEEE division as the reference's two transforms: bit-exact.
__global__ void gather_normalize_kernel(const uint8_t* __restrict__ data,
                                        const int64_t* __restrict__ idx, float* __restrict__ out,
                                        int64_t n4, int per4, float mean, float stdv) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / per4;
    const int k = (int)(i - b * per4);
    const int64_t row = idx ? idx[b] : b;
    const uchar4 u = reinterpret_cast<const uchar4*>(data + row * (int64_t)per4 * 4)[k];
    float4 o;
    o.x = __fdiv_rn(__fsub_rn(__fdiv_rn((float)u.x, 255.0f), mean), stdv);
    o.y = __fdiv_rn(__fsub_rn(__fdiv_rn((float)u.y, 255.0f), mean), stdv);
    o.z = __fdiv_rn(__fsub_rn(__fdiv_rn((float)u.z, 255.0f), mean), stdv);
    o.w = __fdiv_rn(__fsub_rn(__fdiv_rn((float)u.w, 255.0f), mean), stdv);
    reinterpret_cast<float4*>(out)[i] = o;
  }
}

extern "C" int tdx_u8_gather_normalize(const uint8_t* data, const int64_t* idx, float* out, int batch,
                                       int per_sample, float mean, float stdv, tdx_stream_t stream) {
  if (!data || !out || batch <= 0 || per_sample <= 0 || stdv == 0.f) return TDX_E_BADARG;
  if (per_sample % 4) return TDX_E_SHAPE;
  const int64_t n4 = (int64_t)batch * per_sample / 4;
  gather_normalize_kernel<<<ew_grid(n4, 256), 256, 0, to_stream(stream)>>>(data, idx, out, n4,
                                                                         per_sample / 4, mean, stdv);
  TDX_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------- condition dropout
// Training the unconditional branch of classifier-free guidance: sample b loses its condition iff a Philox uniform in
// [0, 1) keyed by (seed, offset, b) is < p, so p == 0 is a copy and p == 1 drops every sample.  A dropped sample gets the
// null label -1 (y != null: dim == 1) or a zeroed embedding row (c).  Elementwise: y_out == y / c_out == c is allowed.
__global__ void cond_drop_kernel(const int64_t* y, int64_t* y_out, const float* c, float* c_out, int64_t n, int dim,
                                 float p, uint64_t seed, uint64_t offset) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t b = (uint64_t)(i / dim);
    const Philox4 r = philox4x32_10(b, offset, seed);
    const bool drop = (float)(r.v[0] >> 8) * 5.9604644775390625e-8f < p;   // 24 bits: exact in fp32, never 1
    if (y) y_out[i] = drop ? (int64_t)-1 : y[i];
    else c_out[i] = drop ? 0.f : c[i];
  }
}

extern "C" int tdx_cond_drop_labels(const int64_t* y, int64_t* y_out, int B, float p, uint64_t seed, uint64_t offset,
                                    tdx_stream_t stream) {
  if (!y || !y_out || B <= 0 || !(p >= 0.f && p <= 1.f)) return TDX_E_BADARG;
  cond_drop_kernel<<<ew_grid(B, 256), 256, 0, to_stream(stream)>>>(y, y_out, nullptr, nullptr, B, 1, p, seed, offset);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_cond_drop_rows(const float* c, float* c_out, int B, int dim, float p, uint64_t seed, uint64_t offset,
                                  tdx_stream_t stream) {
  if (!c || !c_out || B <= 0 || dim <= 0 || !(p >= 0.f && p <= 1.f)) return TDX_E_BADARG;
  const int64_t n = (int64_t)B * dim;
  cond_drop_kernel<<<ew_grid(n, 256), 256, 0, to_stream(stream)>>>(nullptr, nullptr, c, c_out, n, dim, p, seed, offset);
  TDX_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ MSE loss
__global__ void mse_grad_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                float* __restrict__ d_a, float k, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    d_a[i] = (a[i] - b[i]) * k;
}

// single block, fixed summation order -> deterministic; 4 independent float4 streams per
// thread keep ~8 KB of loads in flight per wave (the kernel is pure latency otherwise)
__global__ void __launch_bounds__(1024) mse_loss_kernel(const float* __restrict__ a,
                                                        const float* __restrict__ b,
                                                        float* __restrict__ out, int64_t n) {
  __shared__ double red[16];
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t n4 = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) ? 0 : n / 4;
  const float4* a4 = reinterpret_cast<const float4*>(a);
  const float4* b4 = reinterpret_cast<const float4*>(b);
  int64_t i = threadIdx.x;
  for (; i + 3 * 1024 < n4; i += 4 * 1024) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 x = a4[i + k * 1024], y = b4[i + k * 1024];
      const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
      acc[k] += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
  }
  for (; i < n4; i += 1024) {
    const float4 x = a4[i], y = b4[i];
    const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
    acc[0] += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
  }
  for (int64_t j = n4 * 4 + threadIdx.x; j < n; j += 1024) {
    const float d = a[j] - b[j];
    acc[1] += d * d;
  }
  double s = (double)acc[0] + (double)acc[1] + (double)acc[2] + (double)acc[3];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    long long v = __double_as_longlong(s);
    int lo = __shfl_xor((int)(v & 0xffffffffll), o, 64);
    int hi = __shfl_xor((int)(v >> 32), o, 64);
    s += __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += red[w];
    out[0] = (float)(t / (double)n);
  }
}

extern "C" int tdx_mse_loss(const float* a, const float* b, float* loss_out, float* d_a,
                            float gscale, int64_t n, tdx_stream_t stream) {
  if (!a || !b || n <= 0) return TDX_E_BADARG;
  if (loss_out) {
    mse_loss_kernel<<<1, 1024, 0, to_stream(stream)>>>(a, b, loss_out, n);
    TDX_CHECK_LAUNCH();
  }
  if (d_a) {
    mse_grad_kernel<<<ew_grid(n, 256), 256, 0, to_stream(stream)>>>(a, b, d_a,
                                                                     2.0f * gscale / (float)n, n);
    TDX_CHECK_LAUNCH();
  }
  return 0;
}

// Loss and its gradient in ONE multi-block pass (the training step's form): every block writes its slice of
// d_a = 2 (a - b) / n * gscale and one double partial of sum (a - b)^2; a second, one-block launch adds the
// partials in a fixed order.  (The single-block loss kernel above is latency-bound: 28 us for the 200 k
// elements of the MNIST step and 131 / 520 us for the LAION step at 32 / 64 - on the critical path between
// forward and backward, where nothing else runs.)  Deterministic: fixed grid, fixed order.
#define MSE_BLOCKS 512
__global__ void __launch_bounds__(256)
mse_loss_grad_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ d_a,
                     float scale, int64_t n, double* __restrict__ partials) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float d = a[i] - b[i];
    if (d_a) d_a[i] = d * scale;
    s += (double)d * (double)d;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    long long v = __double_as_longlong(s);
    int lo = __shfl_xor((int)(v & 0xffffffffll), o, 64);
    int hi = __shfl_xor((int)(v >> 32), o, 64);
    s += __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void __launch_bounds__(256)
mse_finish_kernel(const double* __restrict__ partials, int nblk, float* __restrict__ out, double inv_n) {
  __shared__ double red[256];
  double s = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 256) s += partials[k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(red[0] * inv_n);
}

extern "C" size_t tdx_mse_scratch_bytes(void) { return MSE_BLOCKS * sizeof(double); }

extern "C" int tdx_mse_loss_grad(const float* a, const float* b, float* loss_out, float* d_a, float gscale,
                                 int64_t n, void* scratch, tdx_stream_t stream) {
  if (!a || !b || !loss_out || !scratch || n <= 0) return TDX_E_BADARG;
  hipStream_t st = to_stream(stream);
  int grid = (int)((n + 1023) / 1024);
  if (grid > MSE_BLOCKS) grid = MSE_BLOCKS;
  mse_loss_grad_kernel<<<grid, 256, 0, st>>>(a, b, d_a, 2.0f * gscale / (float)n, n, static_cast<double*>(scratch));
  TDX_CHECK_LAUNCH();
  mse_finish_kernel<<<1, 256, 0, st>>>(static_cast<const double*>(scratch), grid, loss_out, 1.0 / (double)n);
  TDX_CHECK_LAUNCH();
  return 0;
}

// The same pass with a per-timestep loss weight (TrainStep(loss_weighting=...)): sample s = i / per_sample carries
// w = w_table[t[s]];  loss = sum w (a-b)^2 / n,  d_a = fl(fl(a-b) * fl(scale * w)) with scale as above.  The grid, the
// element -> block mapping, the double partials and the finish are those of mse_loss_grad_kernel, so a table of ones
// gives its loss and gradient bit for bit (1.0 * x is exact in both precisions).
template <typename IDX>
__global__ void __launch_bounds__(256)
mse_loss_grad_weighted_kernel(const float* __restrict__ a, const float* __restrict__ b, const int64_t* __restrict__ t,
                              const float* __restrict__ w_table, float* __restrict__ d_a, float scale, int64_t n,
                              int per_sample, double* __restrict__ partials) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float w = w_table[t[(IDX)i / (IDX)per_sample]];
    const float d = a[i] - b[i];
    if (d_a) d_a[i] = __fmul_rn(d, __fmul_rn(scale, w));
    s += (double)w * ((double)d * (double)d);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    long long v = __double_as_longlong(s);
    int lo = __shfl_xor((int)(v & 0xffffffffll), o, 64);
    int hi = __shfl_xor((int)(v >> 32), o, 64);
    s += __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

extern "C" int tdx_mse_loss_grad_weighted(const float* a, const float* b, const int64_t* t, const float* w_table,
                                          float* loss_out, float* d_a, float gscale, int batch, int per_sample,
                                          void* scratch, tdx_stream_t stream) {
  if (!a || !b || !t || !w_table || !loss_out || !scratch || batch <= 0 || per_sample <= 0) return TDX_E_BADARG;
  hipStream_t st = to_stream(stream);
  const int64_t n = (int64_t)batch * per_sample;
  int grid = (int)((n + 1023) / 1024);
  if (grid > MSE_BLOCKS) grid = MSE_BLOCKS;
  const float scale = 2.0f * gscale / (float)n;
  double* partials = static_cast<double*>(scratch);
  if (n <= 0x7fffffff)   // the sample index by a 32-bit division
    mse_loss_grad_weighted_kernel<uint32_t><<<grid, 256, 0, st>>>(a, b, t, w_table, d_a, scale, n, per_sample, partials);
  else
    mse_loss_grad_weighted_kernel<int64_t><<<grid, 256, 0, st>>>(a, b, t, w_table, d_a, scale, n, per_sample, partials);
  TDX_CHECK_LAUNCH();
  mse_finish_kernel<<<1, 256, 0, st>>>(partials, grid, loss_out, 1.0 / (double)n);
  TDX_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------- Adam
// torch.optim.Adam defaults, single-tensor formulation:
//   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g
//   p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v, int64_t n, float lr_bc1,
                            float b1, float b2, float eps, float inv_sqrt_bc2, float gs) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gi = g[i] * gs;
    float mi = m[i] * b1 + (1.0f - b1) * gi;
    float vi = v[i] * b2 + (1.0f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
    p[i] = p[i] - lr_bc1 * (mi / denom);
  }
}

extern "C" int tdx_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                             int64_t n, float lr, float beta1, float beta2, float eps, int step,
                             float grad_scale, tdx_stream_t stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step <= 0) return TDX_E_BADARG;
  double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  adam_kernel<<<ew_grid(n, 256), 256, 0, to_stream(stream)>>>(
      param, grad, exp_avg, exp_avg_sq, n, (float)(lr / bc1), beta1, beta2, eps,
      (float)(1.0 / sqrt(bc2)), grad_scale);
  TDX_CHECK_LAUNCH();
  return 0;
}

// Same update with the step-dependent scalars read from device memory, so the launch can sit in a
// HIP graph that is replayed every step: hyper = {lr/bc1, 1/sqrt(bc2), grad_scale}.
__global__ void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                float* __restrict__ m, float* __restrict__ v, int64_t n,
                                const float* __restrict__ hyper, float b1, float b2, float eps) {
  const float lr_bc1 = hyper[0], inv_sqrt_bc2 = hyper[1], gs = hyper[2];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gi = g[i] * gs;
    float mi = m[i] * b1 + (1.0f - b1) * gi;
    float vi = v[i] * b2 + (1.0f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
    p[i] = p[i] - lr_bc1 * (mi / denom);
  }
}

extern "C" int tdx_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                 int64_t n, const float* hyper, float beta1, float beta2, float eps,
                                 tdx_stream_t stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !hyper || n <= 0) return TDX_E_BADARG;
  adam_dev_kernel<<<ew_grid(n, 256), 256, 0, to_stream(stream)>>>(param, grad, exp_avg, exp_avg_sq, n, hyper,
                                                                 beta1, beta2, eps);
  TDX_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------- Adam with fused clip_grad_norm_
// torch.nn.utils.clip_grad_norm_(parameters, max_norm) followed by Adam
// (conditional_diffusion_laion.py:469-472) in two launches over the flat gradient: (1) fixed-grid
// sum of squares -> CLIP_BLOCKS double partials (fixed order, no atomics); (2) the Adam kernel, whose
// every block re-adds the partials in the same fixed order, forms
//     total_norm = sqrt(sum g^2) * grad_scale ;  clip = min(1, max_norm / (total_norm + 1e-6))
// (torch's formula, the 1/world of the data-parallel mean folded in through grad_scale) and applies
// g * grad_scale * clip on the fly: the clipped gradient is never written, which saves the
// read-modify-write pass over it that the torch call makes (8 B/param) and four small launches.
#define CLIP_BLOCKS 1024

__global__ void __launch_bounds__(256)
grad_sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partials) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = (double)g[i];
    s += v * v;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

template <bool DEV_HYPER>
__global__ void __launch_bounds__(256)
adam_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                 float* __restrict__ v, int64_t n, float lr_bc1, float b1, float b2, float eps,
                 float inv_sqrt_bc2, float gs, const float* __restrict__ hyper,
                 const double* __restrict__ partials, float max_norm) {
  __shared__ double red[256];
  if (DEV_HYPER) { lr_bc1 = hyper[0]; inv_sqrt_bc2 = hyper[1]; gs = hyper[2]; }
  {
    double s = 0.0;
    for (int k = threadIdx.x; k < CLIP_BLOCKS; k += 256) s += partials[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
      if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
      __syncthreads();
    }
  }
  const float total_norm = (float)sqrt(red[0]) * fabsf(gs);
  const float clip = fminf(1.0f, max_norm / (total_norm + 1e-6f));
  const float ge = gs * clip;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float gi = g[i] * ge;
    float mi = m[i] * b1 + (1.0f - b1) * gi;
    float vi = v[i] * b2 + (1.0f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
    p[i] = p[i] - lr_bc1 * (mi / denom);
  }
}

extern "C" size_t tdx_adam_clip_scratch_bytes(void) { return CLIP_BLOCKS * sizeof(double); }

extern "C" int tdx_adam_step_clip(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                  int64_t n, float lr, float beta1, float beta2, float eps, int step,
                                  float grad_scale, float max_norm, const float* hyper_dev, void* scratch,
                                  tdx_stream_t stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !scratch || n <= 0 || !(max_norm > 0.f)) return TDX_E_BADARG;
  if (!hyper_dev && step <= 0) return TDX_E_BADARG;
  hipStream_t st = to_stream(stream);
  double* partials = static_cast<double*>(scratch);
  grad_sumsq_kernel<<<CLIP_BLOCKS, 256, 0, st>>>(grad, n, partials);
  TDX_CHECK_LAUNCH();
  if (hyper_dev) {
    adam_clip_kernel<true><<<ew_grid(n, 256), 256, 0, st>>>(param, grad, exp_avg, exp_avg_sq, n, 0.f, beta1, beta2,
                                                            eps, 0.f, 0.f, hyper_dev, partials, max_norm);
  } else {
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    adam_clip_kernel<false><<<ew_grid(n, 256), 256, 0, st>>>(param, grad, exp_avg, exp_avg_sq, n, (float)(lr / bc1),
                                                             beta1, beta2, eps, (float)(1.0 / sqrt(bc2)), grad_scale,
                                                             nullptr, partials, max_norm);
  }
  TDX_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------- Adam with a fused EMA of the parameters
// The Adam update of the kernels above and, for the same element, the exponential moving average
//     e = e + a * (p_new - e) ,  a = 1 - decay
// of the parameter value just computed (Ho et al. 2020 sample from it): the average costs its own read and
// write, 8 B/param on top of Adam's 28, where a pass of its own would read p again (12 B/param) and launch.
// adam_elem holds the expressions of adam_kernel in the same order, so p, m and v come out bit-identical
// to the entries without the average; the average is three separately rounded fp32 operations, like
// torch's e + a * (p - e) on tensors.
__device__ __forceinline__ float adam_elem(float p, float g, float& m, float& v, float gs, float lr_bc1, float b1,
                                           float b2, float eps, float inv_sqrt_bc2) {
  float gi = g * gs;
  float mi = m * b1 + (1.0f - b1) * gi;
  float vi = v * b2 + (1.0f - b2) * gi * gi;
  m = mi;
  v = vi;
  float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
  return p - lr_bc1 * (mi / denom);
}

__device__ __forceinline__ float ema_elem(float e, float p, float a) {
  return __fadd_rn(e, __fmul_rn(a, __fsub_rn(p, e)));
}

static bool overlap(const float* a, const float* b, int64_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = (uintptr_t)n * sizeof(float);
  return x < y + len && y < x + len;
}

// Five streams of 4 B per element, one float per lane like adam_kernel: a float4 body for 16-byte aligned buffers was
// measured and not kept (0.6 - 1.7 % faster in isolation, inside the spread in one of two runs).
// DEV_HYPER: the scalars come from hyper = {lr/bc1, 1/sqrt(bc2), grad_scale, a}.  CLIP: clip_grad_norm_ from
// grad_sumsq_kernel's partials, re-added in adam_clip_kernel's order.
template <bool DEV_HYPER, bool CLIP>
__global__ void __launch_bounds__(256)
adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                float* __restrict__ v, float* __restrict__ e, int64_t n, float lr_bc1, float b1, float b2,
                float eps, float inv_sqrt_bc2, float gs, float a, const float* __restrict__ hyper,
                const double* __restrict__ partials, float max_norm) {
  if (DEV_HYPER) { lr_bc1 = hyper[0]; inv_sqrt_bc2 = hyper[1]; gs = hyper[2]; a = hyper[3]; }
  float ge = gs;
  if (CLIP) {
    __shared__ double red[256];
    double s = 0.0;
    for (int k = threadIdx.x; k < CLIP_BLOCKS; k += 256) s += partials[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
      if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
      __syncthreads();
    }
    const float total_norm = (float)sqrt(red[0]) * fabsf(gs);
    const float clip = fminf(1.0f, max_norm / (total_norm + 1e-6f));
    ge = gs * clip;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float mi = m[i], vi = v[i];
    const float pi = adam_elem(p[i], g[i], mi, vi, ge, lr_bc1, b1, b2, eps, inv_sqrt_bc2);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
    e[i] = ema_elem(e[i], pi, a);
  }
}

static bool ema_args_ok(const float* param, const float* grad, const float* exp_avg, const float* exp_avg_sq,
                        const float* ema, int64_t n) {
  return param && grad && exp_avg && exp_avg_sq && ema && n > 0 && !overlap(param, ema, n);
}

extern "C" int tdx_adam_ema_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                                 int64_t n, float lr, float beta1, float beta2, float eps, int step,
                                 float grad_scale, float ema_one_minus_decay, tdx_stream_t stream) {
  if (!ema_args_ok(param, grad, exp_avg, exp_avg_sq, ema, n) || step <= 0) return TDX_E_BADARG;
  if (!(ema_one_minus_decay >= 0.f && ema_one_minus_decay <= 1.f)) return TDX_E_BADARG;
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  adam_ema_kernel<false, false><<<ew_grid(n, 256), 256, 0, to_stream(stream)>>>(
      param, grad, exp_avg, exp_avg_sq, ema, n, (float)(lr / bc1), beta1, beta2, eps, (float)(1.0 / sqrt(bc2)),
      grad_scale, ema_one_minus_decay, nullptr, nullptr, 0.f);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_adam_ema_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                                     int64_t n, const float* hyper4, float beta1, float beta2, float eps,
                                     tdx_stream_t stream) {
  if (!ema_args_ok(param, grad, exp_avg, exp_avg_sq, ema, n) || !hyper4) return TDX_E_BADARG;
  adam_ema_kernel<true, false><<<ew_grid(n, 256), 256, 0, to_stream(stream)>>>(
      param, grad, exp_avg, exp_avg_sq, ema, n, 0.f, beta1, beta2, eps, 0.f, 0.f, 0.f, hyper4, nullptr, 0.f);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_adam_ema_step_clip(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                                      int64_t n, float lr, float beta1, float beta2, float eps, int step,
                                      float grad_scale, float max_norm, float ema_one_minus_decay,
                                      const float* hyper4_dev, void* scratch, tdx_stream_t stream) {
  if (!ema_args_ok(param, grad, exp_avg, exp_avg_sq, ema, n) || !scratch || !(max_norm > 0.f)) return TDX_E_BADARG;
  if (!hyper4_dev && (step <= 0 || !(ema_one_minus_decay >= 0.f && ema_one_minus_decay <= 1.f))) return TDX_E_BADARG;
  hipStream_t st = to_stream(stream);
  double* partials = static_cast<double*>(scratch);
  grad_sumsq_kernel<<<CLIP_BLOCKS, 256, 0, st>>>(grad, n, partials);
  TDX_CHECK_LAUNCH();
  const int grid = ew_grid(n, 256);
  if (hyper4_dev) {
    adam_ema_kernel<true, true><<<grid, 256, 0, st>>>(param, grad, exp_avg, exp_avg_sq, ema, n, 0.f, beta1, beta2,
                                                      eps, 0.f, 0.f, 0.f, hyper4_dev, partials, max_norm);
  } else {
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    adam_ema_kernel<false, true><<<grid, 256, 0, st>>>(param, grad, exp_avg, exp_avg_sq, ema, n, (float)(lr / bc1),
                                                       beta1, beta2, eps, (float)(1.0 / sqrt(bc2)), grad_scale,
                                                       ema_one_minus_decay, nullptr, partials, max_norm);
  }
  TDX_CHECK_LAUNCH();
  return 0;
}

// Exchange the contents of two buffers (TrainStep.ema_weights: the parameters and their average trade
// places, no pointer changes).  Each lane reads both values and writes both: exact, order-free.
__global__ void __launch_bounds__(256) swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float x = a[i], y = b[i];
    a[i] = y;
    b[i] = x;
  }
}

extern "C" int tdx_swap_f32(float* a, float* b, int64_t n, tdx_stream_t stream) {
  if (!a || !b || n <= 0 || overlap(a, b, n)) return TDX_E_BADARG;
  swap_f32_kernel<<<ew_grid(n, 256), 256, 0, to_stream(stream)>>>(a, b, n);
  TDX_CHECK_LAUNCH();
  return 0;
}

// -------------------------------------------------------------------- probes
// fp32 MFMA peak: 4 independent 32x32x2 accumulator chains per wave, 4 waves per block.
__global__ void __launch_bounds__(256) probe_mfma_kernel(float* out, int iters, unsigned long long* stamps) {
  f32x16 acc0 = {0}, acc1 = {0}, acc2 = {0}, acc3 = {0};
  float a = (float)(threadIdx.x & 7) * 0.001f, b = (float)(threadIdx.x & 3) * 0.002f;
  unsigned long long c0 = 0, r0 = 0;
  if (stamps) { c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
  for (int i = 0; i < iters; ++i) {
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc1, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc2, 0, 0, 0);
    acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc3, 0, 0, 0);
  }
  if (stamps && threadIdx.x == 0) {
    stamps[8 * blockIdx.x] = __builtin_amdgcn_s_memtime() - c0;
    stamps[8 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - r0;
  }
  float s = 0.f;
  for (int r = 0; r < 16; ++r) s += acc0[r] + acc1[r] + acc2[r] + acc3[r];
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

extern "C" int tdx_probe_mfma_f32(float* out, int iters, int blocks, tdx_stream_t stream) {
  if (!out || iters <= 0 || blocks <= 0) return TDX_E_BADARG;
  probe_mfma_kernel<<<blocks, 256, 0, to_stream(stream)>>>(
      out, iters, g_knobs.conv_stamp && g_tdx_diag_buffer && (size_t)blocks * 64 <= g_tdx_diag_bytes
                       ? reinterpret_cast<unsigned long long*>(g_tdx_diag_buffer) : nullptr);
  TDX_CHECK_LAUNCH();
  return 0;
}

// four independent 16-byte loads per thread in flight, one pass (no grid-stride loop: the dependent
// loop of the first version reached 4.8 TB/s where the Adam kernel streams 6.8)
__global__ void __launch_bounds__(256)
probe_copy_kernel(const float4* __restrict__ src, float4* __restrict__ dst, int64_t n4) {
  const int64_t base = (int64_t)blockIdx.x * 1024 + threadIdx.x;
  float4 v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = base + k * 256;
    if (i < n4) v[k] = src[i];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = base + k * 256;
    if (i < n4) dst[i] = v[k];
  }
}

extern "C" int tdx_probe_stream_copy(const float* src, float* dst, int64_t n, tdx_stream_t stream) {
  if (!src || !dst || n <= 0 || (n % 4)) return TDX_E_BADARG;
  const int64_t n4 = n / 4;
  probe_copy_kernel<<<(unsigned)((n4 + 1023) / 1024), 256, 0, to_stream(stream)>>>((const float4*)src, (float4*)dst, n4);
  TDX_CHECK_LAUNCH();
  return 0;
}

// up to three device copies in ONE launch (the per-step copies of x, t and the labels: unet.hip).  Segments are
// float counts; a workgroup belongs to exactly one segment (the grid is the sum of the per-segment grids).
struct CopySeg { const float* src; float* dst; unsigned n; unsigned blocks; };
struct CopySegs { CopySeg s[3]; };

__global__ void copy_segments_kernel(CopySegs a) {
  unsigned b = blockIdx.x;
  int k = 0;
  while (k < 2 && b >= a.s[k].blocks) { b -= a.s[k].blocks; ++k; }
  const CopySeg sg = a.s[k];
  const unsigned i0 = b * 1024 + threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned i = i0 + j * 256;
    if (i < sg.n) sg.dst[i] = sg.src[i];
  }
}

int tdx_copy_segments(const float* const* src, float* const* dst, const size_t* n, int count, hipStream_t st) {
  if (count < 1 || count > 3) return TDX_E_BADARG;
  CopySegs a{};
  unsigned total = 0;
  for (int k = 0; k < 3; ++k) {
    if (k < count && n[k] > 0) {
      if (!src[k] || !dst[k] || n[k] > 0xffffffffu - 1024) return TDX_E_BADARG;
      a.s[k] = CopySeg{src[k], dst[k], (unsigned)n[k], (unsigned)((n[k] + 1023) / 1024)};
    }
    total += a.s[k].blocks;
  }
  if (!total) return 0;
  copy_segments_kernel<<<total, 256, 0, st>>>(a);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_version(void) { return TDX_VERSION; }

extern "C" const char* tdx_error_string(int code) {
  switch (code) {
    case 0: return "ok";
    case TDX_E_BADARG: return "tdx: bad argument";
    case TDX_E_SHAPE: return "tdx: unsupported shape";
    case TDX_E_WORKSPACE: return "tdx: workspace too small";
    case TDX_E_STATE: return "tdx: invalid state";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "tdx: unknown error";
  }
}
