// Time / class / text conditioning path (tiny FLOPs, latency-bound).
// kind 0 (MNIST models):
//   emb = Linear(256,256)(SiLU(Linear(1,256)(float(t)))) [+ Embedding(10,256)[y]]
//         diffusion.py:21-25, 111-113; conditional_diffusion.py:31, 121-125
//   t_k = time_proj_k(emb), 1x1 convs on a (B,256,1,1) map == linear 256 -> 128|256|512
//         diffusion.py:105-107, 130-132
// kind 1 (LAION latent model):
//   emb = Linear(768,768)(SiLU(Linear(768,768)(sinusoid(t)))) + text_embeds
//         conditional_diffusion_laion.py:222-232, 239-243, 306-308
//   t_k = time_proj_k(emb): linear 768 -> 64|128|256, conditional_diffusion_laion.py:297-299
// and the backward of all of it.  Kept in fp32 throughout: for kind 0 t is the raw integer
// step (0..999), so pre-activations reach the hundreds.
#include "internal.h"

#define TD 256   // time_dim of kind 0
#define TDL 768  // time_dim of kind 1

__device__ static inline float silu_f(float x) { return x / (1.0f + expf(-x)); }
__device__ static inline float silu_grad_f(float x) {
  const float s = 1.0f / (1.0f + expf(-x));
  return s * (1.0f + x * (1.0f - s));
}

// Dot products are computed cooperatively by a wave (4 floats per lane of a 256-long row, then
// a wave reduction) so weight rows are read as full 1 KiB lines; four rows are in flight per
// wave at a time.  Two launches: the embedding (grid B x 4) and the three projections
// (grid B x 14, 64 of the 896 outputs per block) - the serial depth is 4 row-groups per wave.
__device__ static inline void wave_dot4(const float* __restrict__ w0, int row_stride, const float4 v,
                                        int lane, float (&out)[4]) {
  float4 a[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) a[k] = *reinterpret_cast<const float4*>(w0 + (size_t)k * row_stride + lane * 4);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = wave_sum(a[k].x * v.x + a[k].y * v.y + a[k].z * v.z + a[k].w * v.w);
}

__global__ void __launch_bounds__(256)
time_emb_kernel(const int64_t* __restrict__ t, const int64_t* __restrict__ y,
                const float* __restrict__ w1, const float* __restrict__ b1,
                const float* __restrict__ w2, const float* __restrict__ b2,
                const float* __restrict__ cls, float* __restrict__ pre_out,
                float* __restrict__ emb_out, float* __restrict__ tf_out) {
  __shared__ __attribute__((aligned(16))) float h[TD];
  const int n = blockIdx.x, q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float tf = (float)t[n];
  if (tf_out && q == 0 && tid == 0) tf_out[n] = tf;  // float(t) kept for the backward (dW1 = sum g_pre * t)
  const float pre = fmaf(w1[tid], tf, b1[tid]);  // Linear(1, 256): weight (256,1)
  if (pre_out && q == 0) pre_out[(size_t)n * TD + tid] = pre;
  h[tid] = silu_f(pre);
  __syncthreads();
  const float4 hv = *reinterpret_cast<const float4*>(h + lane * 4);
  const int i0 = q * 64 + wave * 16;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int i = i0 + g * 4;
    float d[4];
    wave_dot4(w2 + (size_t)i * TD, TD, hv, lane, d);
    if (lane < 4) {
      float e = d[lane] + b2[i + lane];
      if (y) {
        const int64_t c = y[n];   // c < 0: the null condition (classifier-free guidance), emb = t_emb, no read of cls
        if (c >= 0) e += cls[(size_t)c * TD + i + lane];
      }
      emb_out[(size_t)n * TD + i + lane] = e;
    }
  }
}

__global__ void __launch_bounds__(256)
time_proj_kernel(const float* __restrict__ emb, const float* __restrict__ pw1,
                 const float* __restrict__ pb1, const float* __restrict__ pw2,
                 const float* __restrict__ pb2, const float* __restrict__ pw3,
                 const float* __restrict__ pb3, float* __restrict__ t1, float* __restrict__ t2,
                 float* __restrict__ t3) {
  const int n = blockIdx.x, q = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float4 ev = *reinterpret_cast<const float4*>(emb + (size_t)n * TD + lane * 4);
  // block q covers outputs [64q, 64q+64) of the concatenated (128 | 256 | 512) projections
  const float* w; const float* b; float* dst; int o0, width;
  if (q < 2) { w = pw1; b = pb1; dst = t1; o0 = q * 64; width = 128; }
  else if (q < 6) { w = pw2; b = pb2; dst = t2; o0 = (q - 2) * 64; width = 256; }
  else { w = pw3; b = pb3; dst = t3; o0 = (q - 6) * 64; width = 512; }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int o = o0 + wave * 16 + g * 4;
    float d[4];
    wave_dot4(w + (size_t)o * TD, TD, ev, lane, d);
    if (lane < 4) dst[(size_t)n * width + o + lane] = d[lane] + b[o + lane];
  }
}

// ------------------------------------------------------------------ kind 1
// sinusoid[n][j] = sin(t * f_j) for j < 384, cos(t * f_{j-384}) after;
// f_j = exp(-ln(10000) * j / 383), every operation rounded to fp32 in the reference's order
template <typename T>
__global__ void sinusoid_kernel(const T* __restrict__ t, float* __restrict__ out, int B, int dim) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * dim) return;
  const int n = i / dim, j = i - n * dim, half = dim / 2;
  if (j >= 2 * half) { out[i] = 0.f; return; }  // odd width: one trailing zero column (reference :230-231)
  const int k = j < half ? j : j - half;
  const float f = expf(-logf(10000.0f) * (float)k / (float)(half - 1));
  const float a = (float)t[n] * f;
  out[i] = j < half ? sinf(a) : cosf(a);
}

// get_timestep_embedding(timesteps, embedding_dim), conditional_diffusion_laion.py:222-232, as an
// entry point of its own (the model's forward runs the same kernel at dim = 768)
extern "C" int tdx_timestep_embedding(const int64_t* t, float* out, int B, int dim, tdx_stream_t stream) {
  if (!t || !out || B <= 0 || dim < 4) return TDX_E_BADARG;
  if ((int64_t)B * dim >= (1ll << 31)) return TDX_E_SHAPE;
  sinusoid_kernel<int64_t><<<cdiv((int64_t)B * dim, 256), 256, 0, to_stream(stream)>>>(t, out, B, dim);
  TDX_CHECK_LAUNCH();
  return 0;
}

// the same for floating-point timesteps (the reference takes `timesteps[:, None].float()`, so a fractional
// t - a guidance / interpolation utility - keeps its fraction)
extern "C" int tdx_timestep_embedding_f32(const float* t, float* out, int B, int dim, tdx_stream_t stream) {
  if (!t || !out || B <= 0 || dim < 4) return TDX_E_BADARG;
  if ((int64_t)B * dim >= (1ll << 31)) return TDX_E_SHAPE;
  sinusoid_kernel<float><<<cdiv((int64_t)B * dim, 256), 256, 0, to_stream(stream)>>>(t, out, B, dim);
  TDX_CHECK_LAUNCH();
  return 0;
}

// out[n][o] = dot(W[o,:], act(in[n,:])) + b[o] (+ addend[n][o]);  rows of W are 256*R long.
// One wave computes 16 output rows for NB samples: weight rows are read as full lines, four
// rows in flight, and every row is reused for NB samples.  grid (ceil(B/NB), O/64).
template <int R, int NB, bool IN_SILU>
__global__ void __launch_bounds__(256)
linear_rows_kernel(const float* __restrict__ in, const float* __restrict__ w,
                   const float* __restrict__ b, const float* __restrict__ addend,
                   float* __restrict__ out, int B, int O) {
  constexpr int J = 256 * R;
  const int n0 = blockIdx.x * NB, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 v[NB][R];
#pragma unroll
  for (int s = 0; s < NB; ++s) {
    const int n = min(n0 + s, B - 1);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float4 x = *reinterpret_cast<const float4*>(in + (size_t)n * J + r * 256 + lane * 4);
      if (IN_SILU) { x.x = silu_f(x.x); x.y = silu_f(x.y); x.z = silu_f(x.z); x.w = silu_f(x.w); }
      v[s][r] = x;
    }
  }
  const int o0 = blockIdx.y * 64 + wave * 16;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int o = o0 + g * 4;
    float4 a[4][R];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int r = 0; r < R; ++r)
        a[k][r] = *reinterpret_cast<const float4*>(w + (size_t)(o + k) * J + r * 256 + lane * 4);
    float res = 0.f;  // lane 4*s + k keeps the result of (sample s, row k)
#pragma unroll
    for (int s = 0; s < NB; ++s)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float d = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r)
          d += a[k][r].x * v[s][r].x + a[k][r].y * v[s][r].y + a[k][r].z * v[s][r].z + a[k][r].w * v[s][r].w;
        d = wave_sum(d);
        if (lane == 4 * s + k) res = d;
      }
    if (lane < 4 * NB) {
      const int s = lane >> 2, k = lane & 3, n = n0 + s;
      if (n < B) {
        float e = b ? res + b[o + k] : res;   // b == null: the bias-free product (sampling tables)
        if (addend) e += addend[(size_t)n * O + o + k];
        out[(size_t)n * O + o + k] = e;
      }
    }
  }
}

// Any width (time_dim is a constructor argument of the reference's NoiseModel and nothing in
// diffusion.py:16-25 / conditional_diffusion_laion.py:236-243 restricts it): one thread per (sample, output),
// scalar loads.  Widths that are not a multiple of 256 are not performance cases; the multiples up to 1024
// (the reference's 256 and 768 among them) take the row kernels above.
template <bool IN_SILU>
__global__ void linear_generic_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                      const float* __restrict__ b, const float* __restrict__ addend,
                                      float* __restrict__ out, int B, int O, int J) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * O) return;
  const int n = idx / O, o = idx - n * O;
  const float* x = in + (size_t)n * J;
  const float* wr = w + (size_t)o * J;
  float s = 0.f;
  for (int j = 0; j < J; ++j) s = fmaf(wr[j], IN_SILU ? silu_f(x[j]) : x[j], s);
  if (b) s += b[o];
  if (addend) s += addend[idx];
  out[idx] = s;
}

static inline bool td_fast(int td) { return td % 256 == 0 && td <= 1024; }
static inline bool td_ok(int kind, int td) { return td >= (kind == 1 ? 4 : 1) && td <= 4096; }

// out = act(in) W^T + b (+ addend) for an input width td
template <bool IN_SILU>
static int linear_rows(const float* in, const float* w, const float* b, const float* addend, float* out, int B,
                       int O, int td, hipStream_t st) {
  constexpr int NB = 4;
  if (!td_fast(td) || O % 64) {
    if ((int64_t)B * O >= (1ll << 31)) return TDX_E_SHAPE;
    linear_generic_kernel<IN_SILU><<<cdiv((int64_t)B * O, 256), 256, 0, st>>>(in, w, b, addend, out, B, O, td);
    TDX_CHECK_LAUNCH();
    return 0;
  }
  const dim3 grid(cdiv(B, NB), O / 64);
  switch (td / 256) {
    case 1: linear_rows_kernel<1, NB, IN_SILU><<<grid, 256, 0, st>>>(in, w, b, addend, out, B, O); break;
    case 2: linear_rows_kernel<2, NB, IN_SILU><<<grid, 256, 0, st>>>(in, w, b, addend, out, B, O); break;
    case 3: linear_rows_kernel<3, NB, IN_SILU><<<grid, 256, 0, st>>>(in, w, b, addend, out, B, O); break;
    case 4: linear_rows_kernel<4, NB, IN_SILU><<<grid, 256, 0, st>>>(in, w, b, addend, out, B, O); break;
    default: return TDX_E_SHAPE;
  }
  TDX_CHECK_LAUNCH();
  return 0;
}

static int time_embed_fwd_laion(const int64_t* t, const float* cond, const float* const* P, float* sin,
                                float* pre, float* emb, float* t1, float* t2, float* t3, int B, int td,
                                hipStream_t st) {
  sinusoid_kernel<int64_t><<<cdiv((int64_t)B * td, 256), 256, 0, st>>>(t, sin, B, td);
  TDX_CHECK_LAUNCH();
  int rc = linear_rows<false>(sin, P[TDX_P_TE0_W], P[TDX_P_TE0_B], nullptr, pre, B, td, td, st);
  if (rc) return rc;
  rc = linear_rows<true>(pre, P[TDX_P_TE2_W], P[TDX_P_TE2_B], cond, emb, B, td, td, st);
  if (rc) return rc;
  float* dst[3] = {t1, t2, t3};
  const int width[3] = {64, 128, 256};
  const int pw[3] = {TDX_P_TP1_W, TDX_P_TP2_W, TDX_P_TP3_W};
  for (int k = 0; k < 3; ++k) {
    rc = linear_rows<false>(emb, P[pw[k]], P[pw[k] + 1], nullptr, dst[k], B, width[k], td, st);
    if (rc) return rc;
  }
  return 0;
}

// kind 0 at a width other than 256: pre = w1 * float(t) + b1 (Linear(1, td)), tf = float(t)
__global__ void time_l1_fwd_kernel(const int64_t* __restrict__ t, const float* __restrict__ w1,
                                   const float* __restrict__ b1, float* __restrict__ pre, float* __restrict__ tf,
                                   int B, int td) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * td) return;
  const int n = i / td, j = i - n * td;
  const float v = (float)t[n];
  pre[i] = fmaf(w1[j], v, b1[j]);
  if (tf && j == 0) tf[n] = v;
}

// emb[n][:] += E[y[n]][:]   (nn.Embedding lookup added to the time embedding, conditional_diffusion.py:121-125)
// y[n] < 0 is the null condition (classifier-free guidance; -1 is the documented value): the row stays t_emb
__global__ void add_class_emb_kernel(float* __restrict__ emb, const float* __restrict__ cls,
                                     const int64_t* __restrict__ y, int B, int td) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * td) return;
  const int n = i / td, j = i - n * td;
  const int64_t c = y[n];
  if (c >= 0) emb[i] += cls[(size_t)c * td + j];
}

static int time_embed_fwd_generic0(const int64_t* t, const int64_t* y, const float* const* P, float* tf,
                                   float* pre, float* emb, float* t1, float* t2, float* t3, int B, int td,
                                   hipStream_t st) {
  time_l1_fwd_kernel<<<cdiv((int64_t)B * td, 256), 256, 0, st>>>(t, P[TDX_P_TE0_W], P[TDX_P_TE0_B], pre, tf, B, td);
  TDX_CHECK_LAUNCH();
  int rc = linear_rows<true>(pre, P[TDX_P_TE2_W], P[TDX_P_TE2_B], nullptr, emb, B, td, td, st);
  if (rc) return rc;
  if (y) {
    add_class_emb_kernel<<<cdiv((int64_t)B * td, 256), 256, 0, st>>>(emb, P[TDX_P_CLASS_EMB], y, B, td);
    TDX_CHECK_LAUNCH();
  }
  float* dst[3] = {t1, t2, t3};
  const int width[3] = {128, 256, 512};
  const int pw[3] = {TDX_P_TP1_W, TDX_P_TP2_W, TDX_P_TP3_W};
  for (int k = 0; k < 3; ++k) {
    rc = linear_rows<false>(emb, P[pw[k]], P[pw[k] + 1], nullptr, dst[k], B, width[k], td, st);
    if (rc) return rc;
  }
  return 0;
}

int tdx_time_embed_fwd(int kind, const int64_t* t, const int64_t* y, const float* cond,
                       const float* const* P, float* sin, float* pre, float* emb, float* t1, float* t2,
                       float* t3, int B, hipStream_t st, int td) {
  if (td <= 0) td = kind == 1 ? TDL : TD;
  if (!td_ok(kind, td)) return TDX_E_SHAPE;
  if (kind == 1) return time_embed_fwd_laion(t, cond, P, sin, pre, emb, t1, t2, t3, B, td, st);
  if (td != TD) return time_embed_fwd_generic0(t, y, P, sin, pre, emb, t1, t2, t3, B, td, st);
  time_emb_kernel<<<dim3(B, 4), 256, 0, st>>>(t, y, P[TDX_P_TE0_W], P[TDX_P_TE0_B], P[TDX_P_TE2_W],
                                              P[TDX_P_TE2_B], P[TDX_P_CLASS_EMB], pre, emb, sin);
  TDX_CHECK_LAUNCH();
  time_proj_kernel<<<dim3(B, 14), 256, 0, st>>>(emb, P[TDX_P_TP1_W], P[TDX_P_TP1_B], P[TDX_P_TP2_W],
                                                P[TDX_P_TP2_B], P[TDX_P_TP3_W], P[TDX_P_TP3_B], t1,
                                                t2, t3);
  TDX_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ backward
// dW[o][j] = sum_n g[n][o] * x[n][j];  db[o] = sum_n g[n][o]     (thread per (o, j))
__global__ void lin_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                 float* __restrict__ dw, float* __restrict__ db, int B, int O, int J,
                                 int ldg) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= O * J) return;
  const int o = idx / J, j = idx - o * J;
  float s = 0.f, sb = 0.f;
#pragma unroll 8
  for (int n = 0; n < B; ++n) {
    const float gv = g[(size_t)n * ldg + o];
    s = fmaf(gv, x[(size_t)n * J + j], s);
    sb += gv;
  }
  dw[idx] = s;
  if (j == 0 && db) db[o] = sb;
}

// gx[n][j] (+)= sum_o g[n][o] * W[o][j]     (thread per (n, j))
__global__ void lin_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                 float* __restrict__ gx, int B, int O, int J, int accumulate, int ldg) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * J) return;
  const int n = idx / J, j = idx - n * J;
  float s = accumulate ? gx[idx] : 0.f;
#pragma unroll 8
  for (int o = 0; o < O; ++o) s = fmaf(g[(size_t)n * ldg + o], w[(size_t)o * J + j], s);
  gx[idx] = s;
}

// g_pre = g_h * silu'(pre);  dW1[j] = sum_n g_pre[n][j] * t[n];  db1[j] = sum_n g_pre[n][j]
// tf = float(t) as the forward computed and stored it (no int64 -> float sequence in the loop)
// block = 32 columns j x 8 interleaved slices of n
__global__ void __launch_bounds__(256)
time_l1_bwd_kernel(const float* __restrict__ g_h, const float* __restrict__ pre,
                   const float* tf, float* __restrict__ dw1, float* __restrict__ db1,
                   int B, int td) {
  __shared__ float red[2][8][32];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int j = blockIdx.x * 32 + cl;
  const bool live = j < td;   // any width: the last workgroup may be ragged
  float sw = 0.f, sb = 0.f;
#pragma unroll 4
  for (int n = sl; n < B && live; n += 8) {
    const float gp = g_h[(size_t)n * td + j] * silu_grad_f(pre[(size_t)n * td + j]);
    // agent-scope load: served by the coherent point, whatever line of this address the XCD's L2 may hold.  The
    // one unexplained miscompute of this path was exactly ONE 128-byte line of the step indices read wrong by one
    // workgroup (13 of 400 runs with plain loads of the int64 copy, 0 of 200 with this form)
    sw = fmaf(gp, __hip_atomic_load(tf + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), sw);
    sb += gp;
  }
  red[0][sl][cl] = sw;
  red[1][sl][cl] = sb;
  __syncthreads();
  if (sl == 0) {
    sw = 0.f; sb = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) { sw += red[0][k][cl]; sb += red[1][k][cl]; }
    if (live) {
      dw1[j] = sw;
      db1[j] = sb;
    }
  }
}

unsigned* g_tdx_diag_buffer = nullptr;  // set by tdx_diag_set_buffer together with its size:
size_t g_tdx_diag_bytes = 0;            // every diagnostic path checks what it is about to write against it
extern "C" int tdx_diag_set_buffer(void* p, size_t bytes) {
  if (p && !bytes) return TDX_E_BADARG;
  g_tdx_diag_buffer = static_cast<unsigned*>(p);
  g_tdx_diag_bytes = p ? bytes : 0;
  return 0;
}

// g[i] *= silu'(pre[i])
__global__ void silu_bwd_kernel(float* __restrict__ g, const float* __restrict__ pre, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) g[i] *= silu_grad_f(pre[i]);
}

// h[n][j] = silu(pre[n][j])
__global__ void silu_kernel(const float* __restrict__ pre, float* __restrict__ h, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) h[i] = silu_f(pre[i]);
}

// dE[c][j] = sum_{n : y[n] == c} g_emb[n][j]   (nn.Embedding backward, fixed order)
__global__ void class_emb_bwd_kernel(const float* __restrict__ g_emb, const int64_t* y,
                                     float* __restrict__ de, int B, int ncls, int td) {
  __shared__ int ys[256];
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = idx < ncls * td;
  const int c = live ? idx / td : 0, j = live ? idx - c * td : 0;
  // labels are read as the LOW dwords of the int64 copy (values < num_classes; the null condition, a negative label,
  // has a negative low dword for every value down to -2^31 and so matches no class), 256 at a time into LDS, by
  // agent-scope loads: served by the coherent point, whatever line of that address this XCD's L2 may hold (the one
  // unexplained miscompute of this path was one stale-looking 128-byte line of such a copy)
  const int* y32 = reinterpret_cast<const int*>(y);
  float s = 0.f;
  for (int n0 = 0; n0 < B; n0 += 256) {
    __syncthreads();
    if (n0 + (int)threadIdx.x < B)
      ys[threadIdx.x] = __hip_atomic_load(y32 + 2 * (n0 + threadIdx.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int nn = min(256, B - n0);
    if (live)
      for (int n = 0; n < nn; ++n)
        if (ys[n] == c) s += g_emb[(size_t)(n0 + n) * td + j];
  }
  if (live) de[idx] = s;
}

// the text embeddings of kind 1 come from a frozen encoder (conditional_diffusion_laion.py:216-218):
// no gradient flows to them
static int time_embed_bwd_laion(const float* const* P, float* const* G, const float* sin, const float* pre,
                                const float* emb, const float* g_t1, const float* g_t2, const float* g_t3,
                                float* scratch, int B, int td, hipStream_t st, int parts) {
  float* g_emb = scratch;
  float* h = scratch + (size_t)B * td;
  float* g_h = scratch + (size_t)2 * B * td;
  const float* gk[3] = {g_t1, g_t2, g_t3};
  const int ok[3] = {64, 128, 256};
  const int pw[3] = {TDX_P_TP1_W, TDX_P_TP2_W, TDX_P_TP3_W};
  for (int k = 0; k < 3 && (parts & TDX_TIME_PROJ); ++k) {
    lin_wgrad_kernel<<<cdiv(ok[k] * td, 256), 256, 0, st>>>(gk[k], emb, G[pw[k]], G[pw[k] + 1], B, ok[k], td, ok[k]);
    TDX_CHECK_LAUNCH();
    lin_dgrad_kernel<<<cdiv(B * td, 256), 256, 0, st>>>(gk[k], P[pw[k]], g_emb, B, ok[k], td, k > 0, ok[k]);
    TDX_CHECK_LAUNCH();
  }
  if (!(parts & TDX_TIME_MID)) return 0;   // this kind has no separate first-layer part: MID is the rest
  silu_kernel<<<cdiv(B * td, 256), 256, 0, st>>>(pre, h, B * td);
  TDX_CHECK_LAUNCH();
  lin_wgrad_kernel<<<cdiv(td * td, 256), 256, 0, st>>>(g_emb, h, G[TDX_P_TE2_W], G[TDX_P_TE2_B], B, td, td, td);
  TDX_CHECK_LAUNCH();
  lin_dgrad_kernel<<<cdiv(B * td, 256), 256, 0, st>>>(g_emb, P[TDX_P_TE2_W], g_h, B, td, td, 0, td);
  TDX_CHECK_LAUNCH();
  silu_bwd_kernel<<<cdiv(B * td, 256), 256, 0, st>>>(g_h, pre, B * td);
  TDX_CHECK_LAUNCH();
  lin_wgrad_kernel<<<cdiv(td * td, 256), 256, 0, st>>>(g_h, sin, G[TDX_P_TE0_W], G[TDX_P_TE0_B], B, td, td, td);
  TDX_CHECK_LAUNCH();
  return 0;
}

// kind-0 time path backward with the three projection gradients given as strided views
// (g_tk[n*ldg[k] + o], o < widths[k]).  scratch: g_emb (B*256) | h (B*256) | g_h (B*256)
int tdx_time_embed_bwd_ex(const float* tf, const int64_t* y, const float* const* P, float* const* G,
                          const float* pre, const float* emb, const float* const* gk, const int* ldg,
                          const int* widths, float* scratch, int B, int ncls, hipStream_t st, int td, int parts) {
  if (td <= 0) td = TD;
  float* g_emb = scratch;
  float* h = scratch + (size_t)B * td;
  float* g_h = scratch + (size_t)2 * B * td;
  const int pw[3] = {TDX_P_TP1_W, TDX_P_TP2_W, TDX_P_TP3_W};
  for (int k = 0; k < 3 && (parts & TDX_TIME_PROJ); ++k) {
    lin_wgrad_kernel<<<cdiv(widths[k] * td, 256), 256, 0, st>>>(gk[k], emb, G[pw[k]], G[pw[k] + 1], B,
                                                                widths[k], td, ldg[k]);
    TDX_CHECK_LAUNCH();
    lin_dgrad_kernel<<<cdiv(B * td, 256), 256, 0, st>>>(gk[k], P[pw[k]], g_emb, B, widths[k], td, k > 0,
                                                        ldg[k]);
    TDX_CHECK_LAUNCH();
  }
  if (parts & TDX_TIME_MID) {
    if (ncls > 0 && y) {
      class_emb_bwd_kernel<<<cdiv(ncls * td, 256), 256, 0, st>>>(g_emb, y, G[TDX_P_CLASS_EMB], B, ncls, td);
      TDX_CHECK_LAUNCH();
    }
    silu_kernel<<<cdiv(B * td, 256), 256, 0, st>>>(pre, h, B * td);
    TDX_CHECK_LAUNCH();
    lin_wgrad_kernel<<<cdiv(td * td, 256), 256, 0, st>>>(g_emb, h, G[TDX_P_TE2_W], G[TDX_P_TE2_B], B, td, td, td);
    TDX_CHECK_LAUNCH();
    lin_dgrad_kernel<<<cdiv(B * td, 256), 256, 0, st>>>(g_emb, P[TDX_P_TE2_W], g_h, B, td, td, 0, td);
    TDX_CHECK_LAUNCH();
  }
  if (!(parts & TDX_TIME_L1)) return 0;
  time_l1_bwd_kernel<<<cdiv(td, 32), 256, 0, st>>>(g_h, pre, tf, G[TDX_P_TE0_W], G[TDX_P_TE0_B], B, td);
  TDX_CHECK_LAUNCH();
  return 0;
}

int tdx_time_embed_bwd(int kind, const int64_t* y, const float* const* P, float* const* G,
                       const float* sin, const float* pre, const float* emb, const float* g_t1,
                       const float* g_t2, const float* g_t3, float* scratch, int B, int ncls,
                       hipStream_t st, int td, int parts) {
  if (td <= 0) td = kind == 1 ? TDL : TD;
  if (!td_ok(kind, td)) return TDX_E_SHAPE;
  if (kind == 1)
    return time_embed_bwd_laion(P, G, sin, pre, emb, g_t1, g_t2, g_t3, scratch, B, td, st, parts);
  const float* gk[3] = {g_t1, g_t2, g_t3};
  const int widths[3] = {128, 256, 512};
  return tdx_time_embed_bwd_ex(sin, y, P, G, pre, emb, gk, widths, widths, scratch, B, ncls, st, td, parts);
}

// Backward of ONE time projection (k = 0, 1, 2 <-> time_proj1/2/3), for a caller that has the three
// pixel sums at different times: dW_k, db_k and the projection's contribution to g_emb = scratch[0 : B*td]
// (k = 0 overwrites, k > 0 accumulates: call in the order 0, 1, 2, the summation order of the whole-path
// function above, then that function without TDX_TIME_PROJ in `parts`).
int tdx_time_proj_bwd(int kind, int k, const float* const* P, float* const* G, const float* emb,
                      const float* g_tk, float* scratch, int B, hipStream_t st, int td) {
  if (td <= 0) td = kind == 1 ? TDL : TD;
  if (k < 0 || k > 2 || !td_ok(kind, td)) return TDX_E_SHAPE;
  const int w = (kind == 1 ? 64 : 128) << k;
  const int pw = k == 0 ? TDX_P_TP1_W : k == 1 ? TDX_P_TP2_W : TDX_P_TP3_W;
  lin_wgrad_kernel<<<cdiv(w * td, 256), 256, 0, st>>>(g_tk, emb, G[pw], G[pw + 1], B, w, td, w);
  TDX_CHECK_LAUNCH();
  lin_dgrad_kernel<<<cdiv(B * td, 256), 256, 0, st>>>(g_tk, P[pw], scratch, B, w, td, k > 0, w);
  TDX_CHECK_LAUNCH();
  return 0;
}

// emb only (kind-0 formula): the latent model applies its own projection widths
int tdx_time_embed_only(const int64_t* t, const int64_t* y, const float* const* P, float* pre, float* emb,
                        float* tf_out, int B, hipStream_t st) {
  time_emb_kernel<<<dim3(B, 4), 256, 0, st>>>(t, y, P[TDX_P_TE0_W], P[TDX_P_TE0_B], P[TDX_P_TE2_W],
                                              P[TDX_P_TE2_B], P[TDX_P_CLASS_EMB], pre, emb, tf_out);
  TDX_CHECK_LAUNCH();
  return 0;
}

__global__ void t_to_float_kernel(const int64_t* __restrict__ t, float* __restrict__ tf, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) tf[i] = (float)t[i];
}

// ------------------------------------------------------------------ sampling tables
// The time / class signal enters the network only through the three projections time_proj_k(emb) (diffusion.py:
// 130-132), which are LINEAR in emb = MLP(t) [+ E[y] | + text]: time_proj_k(emb) = (W_k MLP(t) + b_k) + W_k c.
// Inside sample() the weights are frozen, every sample of a step shares t and the conditioning does not change
// from step to step, so the first term is a table over t = 0..T-1 and the second a table over the samples, both
// built ONCE per sample() call; a reverse step then adds two rows per sample instead of running the MLP and the
// projections (two launches of the 37 of a step at n = 16, where a launch boundary costs as much as a small
// kernel).  Exact up to fp32 reassociation of that one sum ("legitimate algebraic shortcuts").
__global__ void iota_i64_kernel(int64_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = i;
}

// floats taken by the int64 step indices at the head of the table-build scratch: 2*T rounded up to 16 bytes, so that
// the sin / pre / emb rows behind them keep the float4 alignment the row kernels read them with (odd T)
size_t tdx_time_tables_index_floats(int T) { return (2 * (size_t)T + 3) & ~(size_t)3; }

// tab_t{1,2,3}[t][:] = W_k MLP(t) + b_k for t < T.  scratch: tdx_time_tables_index_floats(T) + 3*T*td floats.
// tau != null (a timestep schedule of T steps): row k is built at the timestep tau[k] - the schedule is the index list.
int tdx_time_tables_build(int kind, const float* const* P, int T, int td, float* tab1, float* tab2, float* tab3,
                          float* scratch, hipStream_t st, const int64_t* tau) {
  if (td <= 0) td = kind == 1 ? TDL : TD;
  int64_t* tt = reinterpret_cast<int64_t*>(scratch);
  float* sin = scratch + tdx_time_tables_index_floats(T);
  float* pre = sin + (size_t)T * td;
  float* emb = pre + (size_t)T * td;
  if (tau) {
    TDX_HIP(hipMemcpyAsync(tt, tau, (size_t)T * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  } else {
    iota_i64_kernel<<<cdiv(T, 256), 256, 0, st>>>(tt, T);
    TDX_CHECK_LAUNCH();
  }
  return tdx_time_embed_fwd(kind, tt, nullptr, nullptr, P, sin, pre, emb, tab1, tab2, tab3, T, st, td);
}

// e_c[b][:] = E[y[b]][:]  (kind 0, class-conditional); a zero row for the null condition y[b] < 0
__global__ void class_rows_kernel(const float* __restrict__ cls, const int64_t* __restrict__ y, float* __restrict__ out,
                                  int B, int td) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * td) return;
  const int n = i / td, j = i - n * td;
  const int64_t c = y[n];
  out[i] = c >= 0 ? cls[(size_t)c * td + j] : 0.f;
}

// tabc{1,2,3}[b][:] = W_k c_b (no bias), c_b = E[y_b] (kind 0, labels) or the text embedding of sample b (kind 1).
// scratch: B*td floats (kind 0).
int tdx_time_tables_cond(int kind, const float* const* P, const void* cond, int B, int td, float* tabc1, float* tabc2,
                         float* tabc3, float* scratch, hipStream_t st) {
  if (td <= 0) td = kind == 1 ? TDL : TD;
  const float* c = static_cast<const float*>(cond);
  if (kind == 0) {
    class_rows_kernel<<<cdiv((int64_t)B * td, 256), 256, 0, st>>>(P[TDX_P_CLASS_EMB], static_cast<const int64_t*>(cond),
                                                                  scratch, B, td);
    TDX_CHECK_LAUNCH();
    c = scratch;
  }
  float* dst[3] = {tabc1, tabc2, tabc3};
  const int pw[3] = {TDX_P_TP1_W, TDX_P_TP2_W, TDX_P_TP3_W};
  for (int k = 0; k < 3; ++k) {
    const int width = (kind == 1 ? 64 : 128) << k;
    const int rc = linear_rows<false>(c, P[pw[k]], nullptr, nullptr, dst[k], B, width, td, st);
    if (rc) return rc;
  }
  return 0;
}

// Head of a reverse step in table mode: t = *counter (read only: the decrement moved to the END of the step, into
// the update kernel, so that every workgroup here sees the same value); t_idx = t; t_vec[:] = t;
// tp_k[b][:] = tab_tk[t][:] + tabc_k[b][:].  One launch in place of step_begin + the time MLP + the projections.
// With a timestep schedule (tau != null) the counter is the step index k: t_idx = k, t_vec[:] = tau[k], and the
// table (built at the schedule's timesteps) is read at row k.
__global__ void __launch_bounds__(256)
sample_head_kernel(const int64_t* __restrict__ counter, int32_t* __restrict__ t_idx, int64_t* __restrict__ t_vec,
                   int B, int T, int w1, int w2, int w3, const float* __restrict__ tab1,
                   const float* __restrict__ tab2, const float* __restrict__ tab3, const float* __restrict__ tc1,
                   const float* __restrict__ tc2, const float* __restrict__ tc3, float* __restrict__ o1,
                   float* __restrict__ o2, float* __restrict__ o3, int B0, float* __restrict__ o1b,
                   float* __restrict__ o2b, float* __restrict__ o3b, const int64_t* __restrict__ tau) {
  const int64_t t64 = *counter;
  const int t = (int)(t64 < 0 ? 0 : t64 >= T ? T - 1 : t64);   // the tables hold T rows
  const int wsum = w1 + w2 + w3;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) t_vec[i] = tau ? tau[t] : t64;
  if (i == 0) *t_idx = (int32_t)t64;
  if (i >= B * wsum) return;
  const int b = i / wsum, j = i - b * wsum;
  // destination row: samples >= B0 belong to the second half-batch, whose projection slots live in its own workspace
  const bool second = b >= B0;
  const int bd = second ? b - B0 : b;
  if (j < w1) (second ? o1b : o1)[bd * w1 + j] = tab1[(size_t)t * w1 + j] + (tc1 ? tc1[b * w1 + j] : 0.f);
  else if (j < w1 + w2) {
    const int q = j - w1;
    (second ? o2b : o2)[bd * w2 + q] = tab2[(size_t)t * w2 + q] + (tc2 ? tc2[b * w2 + q] : 0.f);
  } else {
    const int q = j - w1 - w2;
    (second ? o3b : o3)[bd * w3 + q] = tab3[(size_t)t * w3 + q] + (tc3 ? tc3[b * w3 + q] : 0.f);
  }
}

int tdx_sample_head(const int64_t* counter, int32_t* t_idx, int64_t* t_vec, int B, int T, int kind, const float* tab1,
                    const float* tab2, const float* tab3, const float* tc1, const float* tc2, const float* tc3,
                    float* o1, float* o2, float* o3, hipStream_t st, int B0, float* o1b, float* o2b, float* o3b,
                    const int64_t* tau) {
  const int w1 = kind == 1 ? 64 : 128, w2 = 2 * w1, w3 = 4 * w1;
  if (B0 <= 0 || B0 >= B || !o1b) { B0 = B; o1b = o1; o2b = o2; o3b = o3; }
  sample_head_kernel<<<cdiv((int64_t)B * (w1 + w2 + w3), 256), 256, 0, st>>>(counter, t_idx, t_vec, B, T, w1, w2, w3,
                                                                              tab1, tab2, tab3, tc1, tc2, tc3, o1, o2, o3,
                                                                              B0, o1b, o2b, o3b, tau);
  TDX_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ C ABI (the path on its own)
static inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// the row kernels (and, at kind 0 width 256, time_emb_kernel / time_proj_kernel) read the activations and the
// weight rows as float4: at the widths that take them these must sit on 16-byte boundaries
static bool time_path_fwd_misaligned(int td, const float* const* P, const float* aux, const float* pre,
                                     const float* emb) {
  if (!td_fast(td)) return false;
  return misaligned16(aux) || misaligned16(pre) || misaligned16(emb) || misaligned16(P[TDX_P_TE0_W]) ||
         misaligned16(P[TDX_P_TE2_W]) || misaligned16(P[TDX_P_TP1_W]) || misaligned16(P[TDX_P_TP2_W]) ||
         misaligned16(P[TDX_P_TP3_W]);
}

extern "C" int tdx_time_path_fwd(int kind, int time_dim, const int64_t* t, const void* cond,
                                 const void* const* params, float* aux, float* pre, float* emb, float* t1,
                                 float* t2, float* t3, int batch, tdx_stream_t stream) {
  if ((kind != 0 && kind != 1) || !t || !params || !aux || !pre || !emb || !t1 || !t2 || !t3 || batch <= 0)
    return TDX_E_BADARG;
  if (kind == 1 && !cond) return TDX_E_BADARG;
  if (time_dim <= 0 || !td_ok(kind, time_dim)) return TDX_E_SHAPE;
  const float* const* P = reinterpret_cast<const float* const*>(params);
  for (int s : {TDX_P_TE0_W, TDX_P_TE0_B, TDX_P_TE2_W, TDX_P_TE2_B, TDX_P_TP1_W, TDX_P_TP1_B, TDX_P_TP2_W,
                TDX_P_TP2_B, TDX_P_TP3_W, TDX_P_TP3_B})
    if (!P[s]) return TDX_E_BADARG;
  if (kind == 0 && cond && !P[TDX_P_CLASS_EMB]) return TDX_E_BADARG;
  if (time_path_fwd_misaligned(time_dim, P, kind == 1 ? aux : nullptr, pre, emb)) return TDX_E_BADARG;
  if (kind == 1 && td_fast(time_dim) && misaligned16(cond)) return TDX_E_BADARG;
  return tdx_time_embed_fwd(kind, t, kind == 0 ? static_cast<const int64_t*>(cond) : nullptr,
                            kind == 1 ? static_cast<const float*>(cond) : nullptr, P, aux, pre, emb, t1, t2, t3,
                            batch, to_stream(stream), time_dim);
}

extern "C" int tdx_time_path_bwd(int kind, int time_dim, int parts, const int64_t* y, const void* const* params,
                                 void* const* grads, const float* aux, const float* pre, const float* emb,
                                 const float* g_t1, const float* g_t2, const float* g_t3, float* scratch, int batch,
                                 int num_classes, tdx_stream_t stream) {
  if ((kind != 0 && kind != 1) || !params || !grads || !aux || !pre || !emb || !scratch || batch <= 0)
    return TDX_E_BADARG;
  if (parts <= 0 || (parts & ~(TDX_TIME_PROJ | TDX_TIME_MID | TDX_TIME_L1))) return TDX_E_BADARG;
  if ((parts & TDX_TIME_PROJ) && (!g_t1 || !g_t2 || !g_t3)) return TDX_E_BADARG;
  if (kind == 0 && y && num_classes <= 0) return TDX_E_BADARG;
  if (time_dim <= 0 || !td_ok(kind, time_dim)) return TDX_E_SHAPE;
  const float* const* P = reinterpret_cast<const float* const*>(params);
  float* const* G = reinterpret_cast<float* const*>(grads);
  for (int s : {TDX_P_TE0_W, TDX_P_TE0_B, TDX_P_TE2_W, TDX_P_TE2_B, TDX_P_TP1_W, TDX_P_TP1_B, TDX_P_TP2_W,
                TDX_P_TP2_B, TDX_P_TP3_W, TDX_P_TP3_B})
    if (!P[s] || !G[s]) return TDX_E_BADARG;
  if (kind == 0 && y && !G[TDX_P_CLASS_EMB]) return TDX_E_BADARG;
  return tdx_time_embed_bwd(kind, kind == 0 ? y : nullptr, P, G, aux, pre, emb, g_t1, g_t2, g_t3, scratch, batch,
                            kind == 0 && y ? num_classes : 0, to_stream(stream), time_dim, parts);
}

extern "C" int tdx_time_path_proj_bwd(int kind, int time_dim, int k, const void* const* params, void* const* grads,
                                      const float* emb, const float* g_tk, float* scratch, int batch,
                                      tdx_stream_t stream) {
  if ((kind != 0 && kind != 1) || k < 0 || k > 2 || !params || !grads || !emb || !g_tk || !scratch || batch <= 0)
    return TDX_E_BADARG;
  if (time_dim <= 0 || !td_ok(kind, time_dim)) return TDX_E_SHAPE;
  const float* const* P = reinterpret_cast<const float* const*>(params);
  float* const* G = reinterpret_cast<float* const*>(grads);
  const int pw = k == 0 ? TDX_P_TP1_W : k == 1 ? TDX_P_TP2_W : TDX_P_TP3_W;
  if (!P[pw] || !G[pw] || !G[pw + 1]) return TDX_E_BADARG;
  return tdx_time_proj_bwd(kind, k, P, G, emb, g_tk, scratch, batch, to_stream(stream), time_dim);
}

extern "C" int tdx_time_mlp_fwd(const int64_t* t, const int64_t* y, const void* const* params, float* pre,
                                float* emb, float* t1, float* t2, float* t3, int batch, tdx_stream_t stream) {
  if (!t || !params || !pre || !emb || !t1 || !t2 || !t3 || batch <= 0) return TDX_E_BADARG;
  return tdx_time_embed_fwd(0, t, y, nullptr, reinterpret_cast<const float* const*>(params), nullptr, pre, emb,
                            t1, t2, t3, batch, to_stream(stream));
}

extern "C" int tdx_time_mlp_bwd(const int64_t* t, const int64_t* y, const void* const* params,
                                void* const* grads, const float* pre, const float* emb, const float* g_t1,
                                const float* g_t2, const float* g_t3, float* scratch, int batch,
                                int num_classes, tdx_stream_t stream) {
  if (!t || !params || !grads || !pre || !emb || !g_t1 || !g_t2 || !g_t3 || !scratch || batch <= 0)
    return TDX_E_BADARG;
  if (y && num_classes <= 0) return TDX_E_BADARG;
  // float(t) behind the three B x 256 scratch blocks (the network keeps it from its forward)
  float* tf = scratch + (size_t)3 * batch * TD;
  t_to_float_kernel<<<cdiv(batch, 256), 256, 0, to_stream(stream)>>>(t, tf, batch);
  TDX_CHECK_LAUNCH();
  return tdx_time_embed_bwd(0, y, reinterpret_cast<const float* const*>(params),
                            reinterpret_cast<float* const*>(grads), tf, pre, emb, g_t1, g_t2, g_t3, scratch,
                            batch, y ? num_classes : 0, to_stream(stream));
}
