// Latent-space DDPM: the MLP noise predictor of latent_diffusion.py:16-128,
// its autograd backward, and the MLP VAE of vae.py:37-62.
//
// 2.8 MFLOP per sample forward: nothing here is throughput-bound, the cost is the length of the
// dependent launch chain.  So the building blocks are few and generic:
//   * one fp32 GEMM shaped for latency (32x32 tiles, split-K over the waves of a workgroup,
//     register prefetch; see gemm_kernel) with operand-layout template flags, serving Linear forward (X W^T), input gradient (gY W) and weight gradient (gY^T X),
//     with a fused epilogue: + bias, eval-mode BatchNorm folded to scale/shift, ReLU / sigmoid,
//     + per-row addend (the time signal), strided output (writes straight into the concat
//     buffers, latent_diffusion.py:124-126);
//   * BatchNorm1d (train) forward / backward as ONE kernel each: a workgroup owns 32 features
//     for ALL rows, so batch statistics and the two backward reductions never leave the block.
#include "internal.h"
#include <algorithm>
#include <cstdlib>
#include <string>

namespace {

constexpr int GT = 32;    // output tile edge (one workgroup)
constexpr int GKC = 128;  // k-chunk staged per iteration; each of the 4 waves reduces a quarter of it
constexpr int GLD = GT + 4;
constexpr float BN1_EPS = 1e-5f;
constexpr float BN1_MOMENTUM = 0.1f;

struct GemmArgs {
  const float* A; const float* B; float* C;
  int M, N, K, lda, ldb, ldc;
  const float* bias;     // [N] or null
  const float* scale;    // [N] or null: y = (acc + bias) * scale + shift
  const float* shift;
  const float* addrow;   // [M x N] (ldr) added after the activation, or null
  int ldr;
  int act;               // 0 none, 1 relu, 2 sigmoid
  int accumulate;        // C += result
  int bf16;              // operands rounded to bf16 (nearest even) and multiplied on v_mfma_f32_32x32x16_bf16, fp32 accumulation
};

// These GEMMs are tiny (<= 128 x 512 x 512) and sit on a dependent chain, so the kernel is
// shaped for latency, not throughput: a 32x32 output tile per workgroup (many workgroups even
// for a 128-row batch), the reduction dimension split over the four waves (each thread keeps a
// 4x4 partial tile for its wave's quarter of every 128-deep chunk), the next chunk's global
// loads in flight in registers while the current one is reduced, and one LDS reduction of the
// four partial tiles at the end.  K = 512 is four dependent load round trips instead of 32.
// A_KC: A(m,k) = A[m*lda + k] else A[k*lda + m];  B_KC: B(k,n) = B[n*ldb + k] else B[k*ldb + n]
__device__ inline void load4(const float* __restrict__ src, bool vec, bool row_ok, int c, int C, float* v) {
  if (vec && row_ok && c + 3 < C) {  // one 16-byte load
    const float4 q = *reinterpret_cast<const float4*>(src);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (row_ok && c + i < C) ? src[i] : 0.f;
  }
}

template <bool KC>
__device__ inline void stage_load(const float* __restrict__ P, int ld, int r0, int R, int k0, int K, int t,
                                  float (&v)[16]) {
  const bool vec = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(P) & 15) == 0);
  if (KC) {  // element (r, k) at P[r*ld + k]: consecutive lanes take consecutive ROWS (16 B each), so the
             // transposing LDS store below is conflict-free; the data is L2-resident and tiny, the
             // partially used cache lines cost less than 32-way bank conflicts did
    const int r = r0 + (t & 31);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + ((t >> 5) + 8 * j) * 4;
      load4(P + (size_t)r * ld + k, vec, r < R, k, K, &v[j * 4]);
    }
  } else {   // element (r, k) at P[k*ld + r]: 8 threads x float4 along r, 32 k per pass
    const int r = r0 + (t & 7) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + (t >> 3) + 32 * j;
      load4(P + (size_t)k * ld + r, vec, k < K, r, R, &v[j * 4]);
    }
  }
}

template <bool KC>
__device__ inline void stage_store(float (*S)[GLD], int t, const float (&v)[16]) {
  if (KC) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) S[((t >> 5) + 8 * j) * 4 + i][t & 31] = v[j * 4 + i];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<float4*>(&S[(t >> 3) + 32 * j][(t & 7) * 4]) =
          make_float4(v[j * 4], v[j * 4 + 1], v[j * 4 + 2], v[j * 4 + 3]);
  }
}

template <bool A_KC, bool B_KC>
__global__ void __launch_bounds__(256) gemm_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float As[GKC][GLD];
  __shared__ __attribute__((aligned(16))) float Bs[GKC][GLD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, tx = lane & 7, ty = lane >> 3;
  const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  float pa[16], pb[16];
  stage_load<A_KC>(g.A, g.lda, m0, g.M, 0, g.K, t, pa);
  stage_load<B_KC>(g.B, g.ldb, n0, g.N, 0, g.K, t, pb);
  for (int k0 = 0; k0 < g.K; k0 += GKC) {
    __syncthreads();  // the previous chunk has been consumed
    stage_store<A_KC>(As, t, pa);
    stage_store<B_KC>(Bs, t, pb);
    __syncthreads();
    if (k0 + GKC < g.K) {  // next chunk's loads fly while this one is reduced
      stage_load<A_KC>(g.A, g.lda, m0, g.M, k0 + GKC, g.K, t, pa);
      stage_load<B_KC>(g.B, g.ldb, n0, g.N, k0 + GKC, g.K, t, pb);
    }
    const int kb = wave * (GKC / 4);
#pragma unroll 8
    for (int kk = 0; kk < GKC / 4; ++kk) {
      const float4 a = *reinterpret_cast<const float4*>(&As[kb + kk][ty * 4]);
      const float4 b = *reinterpret_cast<const float4*>(&Bs[kb + kk][tx * 4]);
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    }
  }
  // reduce the four waves' partial tiles (fixed order: deterministic), then the epilogue
  __syncthreads();
  float(*Red)[GT * GT] = reinterpret_cast<float(*)[GT * GT]>(&As[0][0]);  // 4 x 1024 floats <= sizeof(As)
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<float4*>(&Red[wave][(ty * 4 + i) * GT + tx * 4]) =
        make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = q * 256 + t, mi = e >> 5, ni = e & 31;  // consecutive threads -> consecutive columns
    const int m = m0 + mi, n = n0 + ni;
    if (m >= g.M || n >= g.N) continue;
    float v = ((Red[0][e] + Red[1][e]) + Red[2][e]) + Red[3][e];
    if (g.bias) v += g.bias[n];
    if (g.scale) v = fmaf(v, g.scale[n], g.shift[n]);
    if (g.act == 1) v = fmaxf(v, 0.f);
    else if (g.act == 2) v = 1.0f / (1.0f + expf(-v));
    if (g.addrow) v += g.addrow[(size_t)m * g.ldr + n];
    float* dst = g.C + (size_t)m * g.ldc + n;
    *dst = g.accumulate ? *dst + v : v;
  }
}

// ---- bf16 mode (BASELINE.json configs[3] names latent_diffusion.py in bf16; the reference has no reduced precision:
// tests/golden/bf16_autocast.npz is the yardstick).  The same 32 x 32 tile, K-chunks and wave split as gemm_kernel, but
// the staged chunk is rounded to bf16 into [row][k] tiles and each wave multiplies its quarter of the chunk (32 deep)
// with TWO v_mfma_f32_32x32x16_bf16 instead of 32 x 16 fp32 FMAs; accumulation, the cross-wave reduction and the
// epilogue (bias, folded BatchNorm, activation, time signal) stay fp32 as above.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
constexpr int GLD16 = GKC + 8;   // bf16 elements per LDS row (272 bytes: 16-byte aligned fragment reads)

template <bool KC>
__device__ inline void stage_store16(__bf16 (*S)[GLD16], int t, const float (&v)[16]) {
  if (KC) {   // thread holds 4 consecutive k of row t & 31, four times
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x4 h;
#pragma unroll
      for (int i = 0; i < 4; ++i) h[i] = (__bf16)v[j * 4 + i];
      *reinterpret_cast<bf16x4*>(&S[t & 31][((t >> 5) + 8 * j) * 4]) = h;
    }
  } else {    // thread holds 4 consecutive ROWS at one k, four times
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) S[(t & 7) * 4 + i][(t >> 3) + 32 * j] = (__bf16)v[j * 4 + i];
  }
}

template <bool A_KC, bool B_KC>
__global__ void __launch_bounds__(256) gemm_bf16_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) __bf16 As[GT][GLD16];
  __shared__ __attribute__((aligned(16))) __bf16 Bs[GT][GLD16];
  __shared__ __attribute__((aligned(16))) float Red[4][GT * GT];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
  const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float pa[16], pb[16];
  stage_load<A_KC>(g.A, g.lda, m0, g.M, 0, g.K, t, pa);
  stage_load<B_KC>(g.B, g.ldb, n0, g.N, 0, g.K, t, pb);
  for (int k0 = 0; k0 < g.K; k0 += GKC) {
    __syncthreads();  // the previous chunk has been consumed
    stage_store16<A_KC>(As, t, pa);
    stage_store16<B_KC>(Bs, t, pb);
    __syncthreads();
    if (k0 + GKC < g.K) {
      stage_load<A_KC>(g.A, g.lda, m0, g.M, k0 + GKC, g.K, t, pa);
      stage_load<B_KC>(g.B, g.ldb, n0, g.N, k0 + GKC, g.K, t, pb);
    }
    const int kb = wave * (GKC / 4);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {   // lane -> row l31, k = kb + 16 s2 + 8 half .. +7 (A and B alike)
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(&As[l31][kb + 16 * s2 + 8 * half]);
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(&Bs[l31][kb + 16 * s2 + 8 * half]);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
  }
  // C/D map of the 32x32 MFMA: column (n) = lane & 31, row (m) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int r = 0; r < 16; ++r) Red[wave][((r & 3) + 8 * (r >> 2) + 4 * half) * GT + l31] = acc[r];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = q * 256 + t, mi = e >> 5, ni = e & 31;
    const int m = m0 + mi, n = n0 + ni;
    if (m >= g.M || n >= g.N) continue;
    float v = ((Red[0][e] + Red[1][e]) + Red[2][e]) + Red[3][e];   // fixed order: deterministic
    if (g.bias) v += g.bias[n];
    if (g.scale) v = fmaf(v, g.scale[n], g.shift[n]);
    if (g.act == 1) v = fmaxf(v, 0.f);
    else if (g.act == 2) v = 1.0f / (1.0f + expf(-v));
    if (g.addrow) v += g.addrow[(size_t)m * g.ldr + n];
    float* dst = g.C + (size_t)m * g.ldc + n;
    *dst = g.accumulate ? *dst + v : v;
  }
}

int launch_gemm(const GemmArgs& g, bool a_kc, bool b_kc, hipStream_t st) {
  if (g.M <= 0 || g.N <= 0 || g.K <= 0) return TDX_E_BADARG;
  dim3 grid(cdiv(g.N, GT), cdiv(g.M, GT));
  if (g.bf16) {
    if (a_kc && b_kc) gemm_bf16_kernel<true, true><<<grid, 256, 0, st>>>(g);
    else if (a_kc) gemm_bf16_kernel<true, false><<<grid, 256, 0, st>>>(g);
    else if (b_kc) gemm_bf16_kernel<false, true><<<grid, 256, 0, st>>>(g);
    else gemm_bf16_kernel<false, false><<<grid, 256, 0, st>>>(g);
    TDX_CHECK_LAUNCH();
    return 0;
  }
  if (a_kc && b_kc) gemm_kernel<true, true><<<grid, 256, 0, st>>>(g);
  else if (a_kc) gemm_kernel<true, false><<<grid, 256, 0, st>>>(g);
  else if (b_kc) gemm_kernel<false, true><<<grid, 256, 0, st>>>(g);
  else gemm_kernel<false, false><<<grid, 256, 0, st>>>(g);
  TDX_CHECK_LAUNCH();
  return 0;
}

// out[M x N] (ldo) = epilogue(X[M x K] (ldx) . W[N x K]^T)
int linear_fwd(const float* x, int ldx, const float* w, const float* bias, float* out, int ldo, int M,
               int N, int K, int act, const float* scale, const float* shift, const float* addrow, int ldr,
               hipStream_t st, int bf16 = 0) {
  GemmArgs g{x, w, out, M, N, K, ldx, K, ldo, bias, scale, shift, addrow, ldr, act, 0, bf16};
  return launch_gemm(g, true, true, st);
}
// gx[M x K] (ldgx) (+)= gy[M x N] (ldgy) . W[N x K]
int linear_dgrad(const float* gy, int ldgy, const float* w, float* gx, int ldgx, int M, int N, int K,
                 int accumulate, hipStream_t st, int bf16 = 0) {
  GemmArgs g{gy, w, gx, M, K, N, ldgy, K, ldgx, nullptr, nullptr, nullptr, nullptr, 0, 0, accumulate, bf16};
  return launch_gemm(g, true, false, st);
}
// dw[N x K] = gy[M x N]^T (ldgy) . x[M x K] (ldx)
int linear_wgrad(const float* gy, int ldgy, const float* x, int ldx, float* dw, int M, int N, int K,
                 hipStream_t st, int bf16 = 0) {
  GemmArgs g{gy, x, dw, N, K, M, ldgy, ldx, K, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, bf16};
  return launch_gemm(g, false, false, st);
}

// out[n] = sum_m g[m*ld + n]   (bias gradient); block = 32 columns x 8 row slices
__global__ void __launch_bounds__(256)
colsum_kernel(const float* __restrict__ g, int ld, int M, int N, float* __restrict__ out) {
  __shared__ float red[8][32];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5, n = blockIdx.x * 32 + cl;
  float s = 0.f;
  if (n < N)
    for (int m = sl; m < M; m += 8) s += g[(size_t)m * ld + n];
  red[sl][cl] = s;
  __syncthreads();
  if (sl == 0 && n < N) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) v += red[k][cl];
    out[n] = v;
  }
}

int colsum(const float* g, int ld, int M, int N, float* out, hipStream_t st) {
  colsum_kernel<<<cdiv(N, 32), 256, 0, st>>>(g, ld, M, N, out);
  TDX_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------- BatchNorm1d + ReLU
// block = 32 features x 8 interleaved row slices; the block sees every row of its features.
__device__ inline float block_colsum(float v, float (*red)[32], int sl, int cl) {
  __syncthreads();
  red[sl][cl] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += red[k][cl];
  return s;
}

// ss = scale | shift | mean | rstd (4N).  out = relu(y*scale + shift) (+ addrow).
__global__ void __launch_bounds__(256)
bn1d_relu_fwd_kernel(const float* __restrict__ y, int M, int N, const float* __restrict__ gamma,
                     const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar,
                     int64_t* __restrict__ nbt, float* __restrict__ ss, float* __restrict__ out, int ldo,
                     const float* __restrict__ addrow, int ldr, int training) {
  __shared__ float red[8][32];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5, n = blockIdx.x * 32 + cl;
  const bool ok = n < N;
  float mean, rstd;
  if (training) {
    float s = 0.f;
    if (ok)
      for (int m = sl; m < M; m += 8) s += y[(size_t)m * N + n];
    mean = block_colsum(s, red, sl, cl) / (float)M;
    float q = 0.f;
    if (ok)
      for (int m = sl; m < M; m += 8) {
        const float d = y[(size_t)m * N + n] - mean;
        q = fmaf(d, d, q);
      }
    const float m2 = block_colsum(q, red, sl, cl);
    const float var = m2 / (float)M;  // biased, used to normalise
    rstd = 1.0f / sqrtf(var + BN1_EPS);
    if (ok && sl == 0 && rmean) {
      const float unbiased = M > 1 ? m2 / (float)(M - 1) : var;
      rmean[n] = (1.0f - BN1_MOMENTUM) * rmean[n] + BN1_MOMENTUM * mean;
      rvar[n] = (1.0f - BN1_MOMENTUM) * rvar[n] + BN1_MOMENTUM * unbiased;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && nbt) nbt[0] += 1;
  } else {
    mean = ok ? rmean[n] : 0.f;
    rstd = ok ? 1.0f / sqrtf(rvar[n] + BN1_EPS) : 0.f;
  }
  if (!ok) return;
  const float sc = gamma[n] * rstd, sh = beta[n] - mean * sc;
  if (sl == 0) { ss[n] = sc; ss[N + n] = sh; ss[2 * N + n] = mean; ss[3 * N + n] = rstd; }
  for (int m = sl; m < M; m += 8) {
    float a = fmaxf(fmaf(y[(size_t)m * N + n], sc, sh), 0.f);
    if (addrow) a += addrow[(size_t)m * ldr + n];
    out[(size_t)m * ldo + n] = a;
  }
}

// g = (relu mask) * (ga1 + ga2);  train: gy = gamma*rstd*(g - mean(g) - xhat*mean(g*xhat));
// eval: gy = g*gamma*rstd.  dgamma = sum g*xhat, dbeta = sum g, dbias(linear) = sum gy.
__global__ void __launch_bounds__(256)
bn1d_relu_bwd_kernel(const float* __restrict__ ga1, int ld1, const float* __restrict__ ga2, int ld2,
                     const float* __restrict__ y, int M, int N, const float* __restrict__ ss,
                     const float* __restrict__ gamma, float* __restrict__ gy, float* __restrict__ dgamma,
                     float* __restrict__ dbeta, float* __restrict__ dbias, int training) {
  __shared__ float red[8][32];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5, n = blockIdx.x * 32 + cl;
  const bool ok = n < N;
  float sc = 0.f, sh = 0.f, mean = 0.f, rstd = 0.f, gm = 0.f;
  if (ok) { sc = ss[n]; sh = ss[N + n]; mean = ss[2 * N + n]; rstd = ss[3 * N + n]; gm = gamma[n]; }
  float s1 = 0.f, s2 = 0.f;
  if (ok)
    for (int m = sl; m < M; m += 8) {
      const float yv = y[(size_t)m * N + n];
      float g = ga1[(size_t)m * ld1 + n];
      if (ga2) g += ga2[(size_t)m * ld2 + n];
      g = fmaf(yv, sc, sh) > 0.f ? g : 0.f;
      s1 += g;
      s2 = fmaf(g, (yv - mean) * rstd, s2);
    }
  s1 = block_colsum(s1, red, sl, cl);
  s2 = block_colsum(s2, red, sl, cl);
  if (!ok) return;
  if (sl == 0) {
    dgamma[n] = s2;
    dbeta[n] = s1;
    dbias[n] = training ? 0.f : s1 * gm * rstd;  // train: the batch mean absorbs the bias exactly
  }
  const float k1 = s1 / (float)M, k2 = s2 / (float)M, gr = gm * rstd;
  for (int m = sl; m < M; m += 8) {
    const float yv = y[(size_t)m * N + n];
    float g = ga1[(size_t)m * ld1 + n];
    if (ga2) g += ga2[(size_t)m * ld2 + n];
    g = fmaf(yv, sc, sh) > 0.f ? g : 0.f;
    gy[(size_t)m * N + n] = training ? gr * (g - k1 - (yv - mean) * rstd * k2) : g * gr;
  }
}

// Register-resident variants for M <= 16*R: block = 16 features x 16 row slices, every thread
// loads its <= R rows ONCE (all loads in flight together), so the kernel costs one global round
// trip instead of three dependent sweeps.
__device__ inline float block_colsum16(float v, float (*red)[16], int sl, int cl) {
  __syncthreads();
  red[sl][cl] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) s += red[k][cl];
  return s;
}

template <int R>
__global__ void __launch_bounds__(256)
bn1d_relu_fwd_reg_kernel(const float* __restrict__ y, int M, int N, const float* __restrict__ gamma,
                         const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar,
                         int64_t* __restrict__ nbt, float* __restrict__ ss, float* __restrict__ out, int ldo,
                         const float* __restrict__ addrow, int ldr, int training) {
  __shared__ float red[16][16];
  const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4, n = blockIdx.x * 16 + cl;
  const bool ok = n < N;
  float v[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int m = sl + 16 * i;
    v[i] = (ok && m < M) ? y[(size_t)m * N + n] : 0.f;
  }
  float mean, rstd;
  if (training) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < R; ++i) s += v[i];
    mean = block_colsum16(s, red, sl, cl) / (float)M;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const float d = (sl + 16 * i < M) ? v[i] - mean : 0.f;
      q = fmaf(d, d, q);
    }
    const float m2 = block_colsum16(q, red, sl, cl);
    const float var = m2 / (float)M;
    rstd = 1.0f / sqrtf(var + BN1_EPS);
    if (ok && sl == 0 && rmean) {
      const float unbiased = M > 1 ? m2 / (float)(M - 1) : var;
      rmean[n] = (1.0f - BN1_MOMENTUM) * rmean[n] + BN1_MOMENTUM * mean;
      rvar[n] = (1.0f - BN1_MOMENTUM) * rvar[n] + BN1_MOMENTUM * unbiased;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && nbt) nbt[0] += 1;
  } else {
    mean = ok ? rmean[n] : 0.f;
    rstd = ok ? 1.0f / sqrtf(rvar[n] + BN1_EPS) : 0.f;
  }
  if (!ok) return;
  const float sc = gamma[n] * rstd, sh = beta[n] - mean * sc;
  if (sl == 0) { ss[n] = sc; ss[N + n] = sh; ss[2 * N + n] = mean; ss[3 * N + n] = rstd; }
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int m = sl + 16 * i;
    if (m < M) {
      float a = fmaxf(fmaf(v[i], sc, sh), 0.f);
      if (addrow) a += addrow[(size_t)m * ldr + n];
      out[(size_t)m * ldo + n] = a;
    }
  }
}

template <int R>
__global__ void __launch_bounds__(256)
bn1d_relu_bwd_reg_kernel(const float* __restrict__ ga1, int ld1, const float* __restrict__ ga2, int ld2,
                         const float* __restrict__ y, int M, int N, const float* __restrict__ ss,
                         const float* __restrict__ gamma, float* __restrict__ gy, float* __restrict__ dgamma,
                         float* __restrict__ dbeta, float* __restrict__ dbias, int training) {
  __shared__ float red[16][16];
  const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4, n = blockIdx.x * 16 + cl;
  const bool ok = n < N;
  float sc = 0.f, sh = 0.f, mean = 0.f, rstd = 0.f, gm = 0.f;
  if (ok) { sc = ss[n]; sh = ss[N + n]; mean = ss[2 * N + n]; rstd = ss[3 * N + n]; gm = gamma[n]; }
  float g[R], z[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int m = sl + 16 * i;
    float yv = 0.f, gv = 0.f;
    if (ok && m < M) {
      yv = y[(size_t)m * N + n];
      gv = ga1[(size_t)m * ld1 + n];
      if (ga2) gv += ga2[(size_t)m * ld2 + n];
    }
    g[i] = fmaf(yv, sc, sh) > 0.f ? gv : 0.f;
    z[i] = (yv - mean) * rstd;
  }
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    if (sl + 16 * i < M) { s1 += g[i]; s2 = fmaf(g[i], z[i], s2); }
  }
  s1 = block_colsum16(s1, red, sl, cl);
  s2 = block_colsum16(s2, red, sl, cl);
  if (!ok) return;
  if (sl == 0) {
    dgamma[n] = s2;
    dbeta[n] = s1;
    dbias[n] = training ? 0.f : s1 * gm * rstd;
  }
  const float k1 = s1 / (float)M, k2 = s2 / (float)M, gr = gm * rstd;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int m = sl + 16 * i;
    if (m < M) gy[(size_t)m * N + n] = training ? gr * (g[i] - k1 - z[i] * k2) : g[i] * gr;
  }
}

int bn1d_relu_fwd(const float* y, int M, int N, const float* gamma, const float* beta, float* rmean, float* rvar,
                  int64_t* nbt, float* ss, float* out, int ldo, const float* addrow, int ldr, int training,
                  hipStream_t st) {
#define TDX_BN1_FWD(R_)                                                                            \
  bn1d_relu_fwd_reg_kernel<R_><<<cdiv(N, 16), 256, 0, st>>>(y, M, N, gamma, beta, rmean, rvar, nbt, ss, out, ldo, \
                                                            addrow, ldr, training)
  if (M <= 32) TDX_BN1_FWD(2);
  else if (M <= 128) TDX_BN1_FWD(8);
  else if (M <= 256) TDX_BN1_FWD(16);
  else if (M <= 1024) TDX_BN1_FWD(64);
  else
    bn1d_relu_fwd_kernel<<<cdiv(N, 32), 256, 0, st>>>(y, M, N, gamma, beta, rmean, rvar, nbt, ss, out, ldo, addrow,
                                                      ldr, training);
#undef TDX_BN1_FWD
  TDX_CHECK_LAUNCH();
  return 0;
}

int bn1d_relu_bwd(const float* ga1, int ld1, const float* ga2, int ld2, const float* y, int M, int N,
                  const float* ss, const float* gamma, float* gy, float* dgamma, float* dbeta, float* dbias,
                  int training, hipStream_t st) {
#define TDX_BN1_BWD(R_)                                                                             \
  bn1d_relu_bwd_reg_kernel<R_><<<cdiv(N, 16), 256, 0, st>>>(ga1, ld1, ga2, ld2, y, M, N, ss, gamma, gy, dgamma, \
                                                            dbeta, dbias, training)
  if (M <= 32) TDX_BN1_BWD(2);
  else if (M <= 128) TDX_BN1_BWD(8);
  else if (M <= 256) TDX_BN1_BWD(16);
  else if (M <= 1024) TDX_BN1_BWD(64);
  else
    bn1d_relu_bwd_kernel<<<cdiv(N, 32), 256, 0, st>>>(ga1, ld1, ga2, ld2, y, M, N, ss, gamma, gy, dgamma, dbeta,
                                                      dbias, training);
#undef TDX_BN1_BWD
  TDX_CHECK_LAUNCH();
  return 0;
}

// z = mu + eps * exp(0.5 * logvar)   (vae.py:55-58)
__global__ void reparam_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                               const float* __restrict__ eps, float* __restrict__ z, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) z[i] = mu[i] + eps[i] * expf(0.5f * logvar[i]);
}

// --------------------------------------------------------------------- network
constexpr int LATENT = 20;
constexpr int TDM = 256;

struct LUnit { int cin, cout; };
// enc1.0 enc1.3 enc2.0 enc2.3 enc3.0 enc3.3 bottleneck dec3.0 dec3.3 dec2.0 dec2.3 dec1.0 dec1.3
const LUnit LU[13] = {{512, 512}, {512, 256}, {256, 256}, {256, 128}, {128, 128}, {128, 64}, {64, 64},
                      {128, 128}, {128, 128}, {256, 256}, {256, 256}, {512, 512}, {512, 512}};
const int TPW[3] = {64, 128, 256};  // time_proj widths

inline size_t al64(size_t n) { return (n + 63) / 64 * 64; }

struct LLayout {
  size_t z, t, tf, y, pre, emb, tp[3], x0, Y[13], ss[13], cat[3], a[13];  // a[u]: dense post-activation (where used)
  size_t gA[13], gY, gcat[3], gx0, timescr, total;
};

LLayout latent_layout(int B) {
  LLayout L;
  size_t o = 0;
  auto take = [&](size_t n) { size_t r = o; o += al64(n); return r; };
  const size_t b = (size_t)B;
  L.z = take(b * LATENT); L.t = take(2 * b); L.tf = take(b); L.y = take(2 * b);
  L.pre = take(b * TDM); L.emb = take(b * TDM);
  for (int k = 0; k < 3; ++k) L.tp[k] = take(b * TPW[k]);
  L.x0 = take(b * 512);
  for (int u = 0; u < 13; ++u) {
    L.Y[u] = take(b * LU[u].cout);
    L.ss[u] = take(4 * (size_t)LU[u].cout);
    L.a[u] = take(b * LU[u].cout);
    L.gA[u] = take(b * LU[u].cout);
  }
  L.cat[0] = take(b * 128); L.cat[1] = take(b * 256); L.cat[2] = take(b * 512);  // dec3, dec2, dec1 inputs
  L.gcat[0] = take(b * 128); L.gcat[1] = take(b * 256); L.gcat[2] = take(b * 512);
  L.gY = take(b * 512);
  L.gx0 = take(b * 512);
  L.timescr = take(3 * b * TDM);
  L.total = o;
  return L;
}

// where the post-activation output of unit u is written, and where unit u reads its input
struct Route { size_t off; int ld; };

}  // namespace

size_t tdx_latent_workspace_floats(int B) { return latent_layout(B).total; }
size_t tdx_latent_infer_ss_floats(void) {
  size_t n = 0;
  for (int u = 0; u < 13; ++u) n += al64(2 * (size_t)LU[u].cout);
  return n;
}

int tdx_latent_pack(const float* const* P, void* const* buffers, float* infer_ss, hipStream_t st) {
  size_t o = 0;
  for (int u = 0; u < 13; ++u) {
    const int C = LU[u].cout;
    float* ss = infer_ss + o;
    int rc = tdx_bn_finalize(nullptr, 0, 0, 0, C, P[TDX_P_UNIT0 + 4 * u + 2], P[TDX_P_UNIT0 + 4 * u + 3],
                             (float*)buffers[3 * u], (float*)buffers[3 * u + 1], nullptr, ss, ss + C, nullptr,
                             nullptr, 0, reinterpret_cast<tdx_stream_t>(st));
    if (rc) return rc;
    o += al64(2 * (size_t)C);
  }
  return 0;
}

#define RC(call)            \
  do {                      \
    int rc__ = (call);      \
    if (rc__) return rc__;  \
  } while (0)

namespace {
// input of unit u and destination of its activation, as (offset, ld) into the workspace
void routes(const LLayout& L, Route in[13], Route out[13]) {
  // e1 -> cat1[:, 256:], e2 -> cat2[:, 128:], e3 -> cat3[:, 64:]; b+t1 -> cat3[:, :64];
  // d3+t2 -> cat2[:, :128]; d2+t3 -> cat1[:, :256]
  out[0] = {L.a[0], 512};          in[0] = {L.x0, 512};
  out[1] = {L.cat[2] + 256, 512};  in[1] = out[0];
  out[2] = {L.a[2], 256};          in[2] = out[1];
  out[3] = {L.cat[1] + 128, 256};  in[3] = out[2];
  out[4] = {L.a[4], 128};          in[4] = out[3];
  out[5] = {L.cat[0] + 64, 128};   in[5] = out[4];
  out[6] = {L.cat[0], 128};        in[6] = out[5];
  out[7] = {L.a[7], 128};          in[7] = {L.cat[0], 128};
  out[8] = {L.cat[1], 256};        in[8] = out[7];
  out[9] = {L.a[9], 256};          in[9] = {L.cat[1], 256};
  out[10] = {L.cat[2], 512};       in[10] = out[9];
  out[11] = {L.a[11], 512};        in[11] = {L.cat[2], 512};
  out[12] = {L.a[12], 512};        in[12] = out[11];
}
// time projection added to the activation of unit u (after the ReLU), or -1
inline int addend_of(int u) { return u == 6 ? 0 : u == 8 ? 1 : u == 10 ? 2 : -1; }
}  // namespace

// bf16 != 0 (tdx_unet_set_precision): the Linear layers of the network proper - initial_fc, the 13 units, final_fc -
// multiply bf16-rounded operands on the bf16 MFMA with fp32 accumulation; the time / class path (pre-activations in the
// hundreds at t = 999: SURVEY.md 7), its projections, BatchNorm1d and every stored tensor stay fp32
int tdx_latent_forward(const float* const* P, void* const* buffers, const float* z, const int64_t* t,
                       const int64_t* y, float* out, float* ws, int B, int mode, const float* infer_ss,
                       hipStream_t st, int bf16) {
  if (B > 4096) return TDX_E_SHAPE;
  const LLayout L = latent_layout(B);
  const bool infer = mode == TDX_MODE_INFER;
  const int training = mode == TDX_MODE_TRAIN ? 1 : 0;
  if (!infer) {
    // keep the inputs for backward: one copy kernel, as in the UNet (the int64 tensors count as 2*B floats)
    const float* src[3] = {z, reinterpret_cast<const float*>(t), reinterpret_cast<const float*>(y)};
    float* dst[3] = {ws + L.z, ws + L.t, ws + L.y};
    const size_t cnt[3] = {(size_t)B * LATENT, 2 * (size_t)B, 2 * (size_t)B};
    RC(tdx_copy_segments(src, dst, cnt, 3, st));
  }
  RC(tdx_time_embed_only(t, y, P, ws + L.pre, ws + L.emb, ws + L.tf, B, st));
  const int pw[3] = {TDX_P_TP1_W, TDX_P_TP2_W, TDX_P_TP3_W};
  for (int k = 0; k < 3; ++k)
    RC(linear_fwd(ws + L.emb, TDM, P[pw[k]], P[pw[k] + 1], ws + L.tp[k], TPW[k], B, TPW[k], TDM, 0, nullptr,
                  nullptr, nullptr, 0, st));
  RC(linear_fwd(z, LATENT, P[TDX_P_INIT_W], P[TDX_P_INIT_B], ws + L.x0, 512, B, 512, LATENT, 0, nullptr, nullptr,
                nullptr, 0, st, bf16));
  Route in[13], o[13];
  routes(L, in, o);
  size_t iss = 0;
  for (int u = 0; u < 13; ++u) {
    const int K = LU[u].cin, N = LU[u].cout, ad = addend_of(u);
    const float* w = P[TDX_P_UNIT0 + 4 * u];
    const float* bias = P[TDX_P_UNIT0 + 4 * u + 1];
    const float* addrow = ad >= 0 ? ws + L.tp[ad] : nullptr;
    const int ldr = ad >= 0 ? TPW[ad] : 0;
    if (infer) {
      // eval-mode BatchNorm folded into the GEMM epilogue: one launch per layer
      const float* ss = infer_ss + iss;
      RC(linear_fwd(ws + in[u].off, in[u].ld, w, bias, ws + o[u].off, o[u].ld, B, N, K, 1, ss, ss + N, addrow, ldr, st, bf16));
      iss += al64(2 * (size_t)N);
      continue;
    }
    RC(linear_fwd(ws + in[u].off, in[u].ld, w, bias, ws + L.Y[u], N, B, N, K, 0, nullptr, nullptr, nullptr, 0, st, bf16));
    RC(bn1d_relu_fwd(ws + L.Y[u], B, N, P[TDX_P_UNIT0 + 4 * u + 2], P[TDX_P_UNIT0 + 4 * u + 3],
                     (float*)buffers[3 * u], (float*)buffers[3 * u + 1], (int64_t*)buffers[3 * u + 2], ws + L.ss[u],
                     ws + o[u].off, o[u].ld, addrow, ldr, training, st));
  }
  return linear_fwd(ws + o[12].off, 512, P[TDX_P_FINAL_W], P[TDX_P_FINAL_B], out, LATENT, B, LATENT, 512, 0, nullptr,
                    nullptr, nullptr, 0, st, bf16);
}

int tdx_latent_backward(const float* const* P, float* const* G, const float* d_out, float* ws, int B,
                        int training, int stage_lo, int stage_hi, int ncls, hipStream_t st, int bf16) {
  const LLayout L = latent_layout(B);
  Route in[13], o[13];
  routes(L, in, o);
  // gradient w.r.t. the activation of unit u: (pointer, ld), plus an optional second addend (skip path)
  struct GSrc { size_t off; int ld; long off2; int ld2; };
  GSrc gs[13];
  for (int u = 0; u < 13; ++u) gs[u] = {L.gA[u], LU[u].cout, -1, 0};
  gs[10] = {L.gcat[2], 512, -1, 0};                    // d(d2 + t3) = gcat1[:, :256]
  gs[8] = {L.gcat[1], 256, -1, 0};                     // d(d3 + t2) = gcat2[:, :128]
  gs[6] = {L.gcat[0], 128, -1, 0};                     // d(b + t1)  = gcat3[:, :64]
  gs[5].off2 = (long)(L.gcat[0] + 64); gs[5].ld2 = 128;   // e3: from the bottleneck + the skip into dec3
  gs[3].off2 = (long)(L.gcat[1] + 128); gs[3].ld2 = 256;  // e2
  gs[1].off2 = (long)(L.gcat[2] + 256); gs[1].ld2 = 512;  // e1
  // where the input gradient of unit u goes
  auto gin = [&](int u) -> Route {
    switch (u) {
      case 11: return {L.gcat[2], 512};
      case 9: return {L.gcat[1], 256};
      case 7: return {L.gcat[0], 128};
      case 0: return {L.gx0, 512};
      default: return {L.gA[u - 1], LU[u - 1].cout};
    }
  };
  float* gY = ws + L.gY;
  for (int s = stage_lo; s < stage_hi; ++s) {
    if (s == 0) {  // final_fc
      RC(linear_wgrad(d_out, LATENT, ws + o[12].off, 512, G[TDX_P_FINAL_W], B, LATENT, 512, st, bf16));
      RC(colsum(d_out, LATENT, B, LATENT, G[TDX_P_FINAL_B], st));
      RC(linear_dgrad(d_out, LATENT, P[TDX_P_FINAL_W], ws + L.gA[12], 512, B, LATENT, 512, 0, st, bf16));
    } else if (s <= 13) {
      const int u = 13 - s, K = LU[u].cin, N = LU[u].cout;
      const int pi = TDX_P_UNIT0 + 4 * u;
      RC(bn1d_relu_bwd(ws + gs[u].off, gs[u].ld, gs[u].off2 >= 0 ? ws + gs[u].off2 : nullptr, gs[u].ld2,
                       ws + L.Y[u], B, N, ws + L.ss[u], P[pi + 2], gY, G[pi + 2], G[pi + 3], G[pi + 1], training, st));
      RC(linear_wgrad(gY, N, ws + in[u].off, in[u].ld, G[pi], B, N, K, st, bf16));
      const Route gi = gin(u);
      RC(linear_dgrad(gY, N, P[pi], ws + gi.off, gi.ld, B, N, K, 0, st, bf16));
    } else {  // initial_fc and the time / class path
      RC(linear_wgrad(ws + L.gx0, 512, ws + L.z, LATENT, G[TDX_P_INIT_W], B, 512, LATENT, st, bf16));
      RC(colsum(ws + L.gx0, 512, B, 512, G[TDX_P_INIT_B], st));
      const float* gt[3] = {ws + L.gcat[0], ws + L.gcat[1], ws + L.gcat[2]};
      const int ldg[3] = {128, 256, 512};
      RC(tdx_time_embed_bwd_ex(ws + L.tf, reinterpret_cast<const int64_t*>(ws + L.y),
                               P, G, ws + L.pre, ws + L.emb, gt, ldg, TPW, ws + L.timescr, B, ncls, st));
    }
  }
  return 0;
}

int tdx_latent_tensor(int B, const char* name, size_t* off, size_t* numel) {
  const LLayout L = latent_layout(B);
  const size_t b = (size_t)B;
  std::string n(name);
  struct { const char* nm; size_t off, cnt; } fixed[] = {
      {"x0", L.x0, b * 512}, {"emb", L.emb, b * TDM}, {"t1", L.tp[0], b * 64}, {"t2", L.tp[1], b * 128},
      {"t3", L.tp[2], b * 256}, {"cat3", L.cat[0], b * 128}, {"cat2", L.cat[1], b * 256}, {"cat1", L.cat[2], b * 512}};
  for (auto& f : fixed)
    if (n == f.nm) { *off = f.off; *numel = f.cnt; return 0; }
  if (n.size() >= 3 && n.rfind("ss", 0) == 0) {  // scale | shift | mean | rstd of unit i, as tdx_unet_tensor's "ssN"
    const int i = atoi(n.c_str() + 2);
    if (i < 0 || i > 12) return TDX_E_BADARG;
    *off = L.ss[i]; *numel = 4 * (size_t)LU[i].cout; return 0;
  }
  if (n.size() >= 2 && n[0] == 'Y') {
    const int i = atoi(n.c_str() + 1);
    if (i < 0 || i > 12) return TDX_E_BADARG;
    *off = L.Y[i]; *numel = b * LU[i].cout; return 0;
  }
  return TDX_E_BADARG;
}

// ------------------------------------------------------------------- C ABI pieces
extern "C" int tdx_linear_fwd(const float* x, int ldx, const float* w, const float* bias, float* out, int ldo,
                              int M, int N, int K, int act, tdx_stream_t stream) {
  if (!x || !w || !out || ldx < K || ldo < N || act < 0 || act > 2) return TDX_E_BADARG;
  return linear_fwd(x, ldx, w, bias, out, ldo, M, N, K, act, nullptr, nullptr, nullptr, 0, to_stream(stream));
}

extern "C" int tdx_linear_bwd_prec(const float* gy, int ldgy, const float* x, int ldx, const float* w, float* gx,
                                   int ldgx, float* dw, float* db, int M, int N, int K, int precision,
                                   tdx_stream_t stream) {
  if (!gy || M <= 0 || N <= 0 || K <= 0 || ldgy < N) return TDX_E_BADARG;
  if (precision != TDX_PREC_F32 && precision != TDX_PREC_BF16) return TDX_E_BADARG;
  const int bf16 = precision == TDX_PREC_BF16;
  hipStream_t st = to_stream(stream);
  if (dw) {
    if (!x || ldx < K) return TDX_E_BADARG;
    RC(linear_wgrad(gy, ldgy, x, ldx, dw, M, N, K, st, bf16));
  }
  if (db) RC(colsum(gy, ldgy, M, N, db, st));   // (a plain fp32 column sum in either precision)
  if (gx) {
    if (!w || ldgx < K) return TDX_E_BADARG;
    RC(linear_dgrad(gy, ldgy, w, gx, ldgx, M, N, K, 0, st, bf16));
  }
  return 0;
}

extern "C" int tdx_linear_bwd(const float* gy, int ldgy, const float* x, int ldx, const float* w, float* gx,
                              int ldgx, float* dw, float* db, int M, int N, int K, tdx_stream_t stream) {
  return tdx_linear_bwd_prec(gy, ldgy, x, ldx, w, gx, ldgx, dw, db, M, N, K, TDX_PREC_F32, stream);
}

extern "C" int tdx_linear_fwd_prec(const float* x, int ldx, const float* w, const float* bias, float* out, int ldo,
                                   int M, int N, int K, int act, int precision, tdx_stream_t stream) {
  if (!x || !w || !out || ldx < K || ldo < N || act < 0 || act > 2) return TDX_E_BADARG;
  if (precision != TDX_PREC_F32 && precision != TDX_PREC_BF16) return TDX_E_BADARG;
  return linear_fwd(x, ldx, w, bias, out, ldo, M, N, K, act, nullptr, nullptr, nullptr, 0, to_stream(stream),
                    precision == TDX_PREC_BF16);
}

extern "C" size_t tdx_vae_workspace_floats(int batch, int hidden_dim) {
  return batch > 0 && hidden_dim > 0 ? al64((size_t)batch * hidden_dim) : 0;
}

// vae.py:51-53.  params: fc1.w fc1.b fc21.w fc21.b fc22.w fc22.b
extern "C" int tdx_vae_encode(const float* x, const void* const* params, float* mu, float* logvar,
                              float* workspace, int batch, int input_dim, int hidden_dim, int latent_dim,
                              tdx_stream_t stream) {
  if (!x || !params || !mu || !logvar || !workspace || batch <= 0) return TDX_E_BADARG;
  const float* const* P = reinterpret_cast<const float* const*>(params);
  hipStream_t st = to_stream(stream);
  RC(linear_fwd(x, input_dim, P[0], P[1], workspace, hidden_dim, batch, hidden_dim, input_dim, 1, nullptr, nullptr,
                nullptr, 0, st));
  RC(linear_fwd(workspace, hidden_dim, P[2], P[3], mu, latent_dim, batch, latent_dim, hidden_dim, 0, nullptr,
                nullptr, nullptr, 0, st));
  return linear_fwd(workspace, hidden_dim, P[4], P[5], logvar, latent_dim, batch, latent_dim, hidden_dim, 0, nullptr,
                    nullptr, nullptr, 0, st);
}

// vae.py:55-58 with the noise supplied by the caller
extern "C" int tdx_vae_reparameterize(const float* mu, const float* logvar, const float* eps, float* z,
                                      int64_t n, tdx_stream_t stream) {
  if (!mu || !logvar || !eps || !z || n <= 0) return TDX_E_BADARG;
  reparam_kernel<<<cdiv(n, 256), 256, 0, to_stream(stream)>>>(mu, logvar, eps, z, n);
  TDX_CHECK_LAUNCH();
  return 0;
}

// vae.py:60-62.  params: fc3.w fc3.b fc4.w fc4.b
extern "C" int tdx_vae_decode(const float* z, const void* const* params, float* out, float* workspace,
                              int batch, int input_dim, int hidden_dim, int latent_dim, tdx_stream_t stream) {
  if (!z || !params || !out || !workspace || batch <= 0) return TDX_E_BADARG;
  const float* const* P = reinterpret_cast<const float* const*>(params);
  hipStream_t st = to_stream(stream);
  RC(linear_fwd(z, latent_dim, P[0], P[1], workspace, hidden_dim, batch, hidden_dim, latent_dim, 1, nullptr, nullptr,
                nullptr, 0, st));
  return linear_fwd(workspace, hidden_dim, P[2], P[3], out, input_dim, batch, input_dim, hidden_dim, 2, nullptr,
                    nullptr, nullptr, 0, st);
}

// ------------------------------------------------------------------------------------------
// VAE training (vae.py:70-76, 104-115): the sum-reduced BCE + KLD loss, its gradient and the backward of
// the five Linear layers.  Elementwise / reduction kernels on at most B x 784 floats; like everything in
// this file the cost is the length of the launch chain.  Both loss sums use the reduction of
// mse_loss_grad_kernel (elementwise.hip): a fixed grid, a fixed element -> block map, one double partial per
// block and a one-block finish that adds them in a fixed order, so the loss is bit-reproducible.
namespace {

constexpr int VAE_LOSS_BLOCKS = 512;   // double partials per loss term

__device__ inline void block_dsum_store(double s, double* red, double* dst) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    long long v = __double_as_longlong(s);
    int lo = __shfl_xor((int)(v & 0xffffffffll), o, 64);
    int hi = __shfl_xor((int)(v >> 32), o, 64);
    s += __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *dst = ((red[0] + red[1]) + red[2]) + red[3];
}

// One element of the BCE from the logit a and the image value x in [-1, 1] (target t = (x + 1) / 2, vae.py:73):
//   BCE = max(a, 0) - a t + log1p(exp(-|a|)),   dBCE/da = sigmoid(a) - t
// exp / log1p / the division are fp32; the target, the product a t and the two differences are formed in double
// from the fp32 operands (exact), because a t cancels against max(a, 0) where the decoder is confident.
struct BceElem { double term; float d, r; };
__device__ inline BceElem bce_elem(float a, float x, float gscale) {
  const float e = expf(-fabsf(a));
  const float r = 1.0f / (1.0f + e);
  const float s = a >= 0.f ? r : e * r;            // sigmoid(a) without overflow on either side
  const double t = ((double)x + 1.0) * 0.5;
  BceElem o;
  o.r = s;
  o.d = gscale * (float)((double)s - t);
  o.term = ((double)fmaxf(a, 0.f) - (double)a * t) + (double)log1pf(e);
  return o;
}

template <bool VEC>
__global__ void __launch_bounds__(256)
vae_bce_logits_grad_kernel(const float* __restrict__ a, const float* __restrict__ x, float* __restrict__ d_a,
                           float* __restrict__ recon, float gscale, int64_t n, double* __restrict__ partials) {
  __shared__ double red[4];
  const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = VEC ? n >> 2 : 0;   // float4 body, then the scalar tail (n need not be a multiple of 4)
  double s = 0.0;
  for (int64_t i = gtid; i < n4; i += stride) {
    const float4 av = reinterpret_cast<const float4*>(a)[i], xv = reinterpret_cast<const float4*>(x)[i];
    const BceElem e0 = bce_elem(av.x, xv.x, gscale), e1 = bce_elem(av.y, xv.y, gscale);
    const BceElem e2 = bce_elem(av.z, xv.z, gscale), e3 = bce_elem(av.w, xv.w, gscale);
    s += e0.term;
    s += e1.term;
    s += e2.term;
    s += e3.term;
    if (d_a) reinterpret_cast<float4*>(d_a)[i] = make_float4(e0.d, e1.d, e2.d, e3.d);
    if (recon) reinterpret_cast<float4*>(recon)[i] = make_float4(e0.r, e1.r, e2.r, e3.r);
  }
  for (int64_t i = 4 * n4 + gtid; i < n; i += stride) {
    const BceElem e = bce_elem(a[i], x[i], gscale);
    s += e.term;
    if (d_a) d_a[i] = e.d;
    if (recon) recon[i] = e.r;
  }
  block_dsum_store(s, red, partials + blockIdx.x);
}

// KLD = -0.5 sum (1 + logvar - mu^2 - exp(logvar)) and, with the decoder's input gradient g_z, the backward of
// z = mu + eps exp(0.5 logvar) together with beta * dKLD:
//   g_mu = g_z + beta mu,   g_logvar = 0.5 g_z eps exp(0.5 logvar) + 0.5 beta (exp(logvar) - 1)
// B x latent_dim elements (2560 at B = 128): evaluated in double and rounded once - the two terms of g_logvar
// cancel where the reconstruction pulls against the prior, and 1 + logvar - exp(logvar) cancels near logvar = 0.
__global__ void __launch_bounds__(256)
vae_kld_reparam_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                           const float* __restrict__ eps, const float* __restrict__ g_z, float* __restrict__ g_mu,
                           float* __restrict__ g_logvar, float beta, int64_t n, double* __restrict__ partials) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double m = mu[i], lv = logvar[i], ev = exp(lv);
    s += -0.5 * (((1.0 + lv) - m * m) - ev);
    if (g_z) {
      const double gz = g_z[i];
      g_mu[i] = (float)(gz + (double)beta * m);
      g_logvar[i] = (float)(0.5 * gz * (double)eps[i] * exp(0.5 * lv) + 0.5 * (double)beta * (ev - 1.0));
    }
  }
  block_dsum_store(s, red, partials + blockIdx.x);
}

// out = {BCE + beta KLD, BCE, KLD} (p_kld null: out[0] = the one sum).  One block, fixed order.
__global__ void __launch_bounds__(256)
vae_loss_finish_kernel(const double* __restrict__ p_bce, int nb_bce, const double* __restrict__ p_kld, int nb_kld,
                       float beta, float* __restrict__ out) {
  __shared__ double red[2][256];
  double s0 = 0.0, s1 = 0.0;
  for (int k = threadIdx.x; k < nb_bce; k += 256) s0 += p_bce[k];
  if (p_kld)
    for (int k = threadIdx.x; k < nb_kld; k += 256) s1 += p_kld[k];
  red[0][threadIdx.x] = s0;
  red[1][threadIdx.x] = s1;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) {
      red[0][threadIdx.x] += red[0][threadIdx.x + half];
      red[1][threadIdx.x] += red[1][threadIdx.x + half];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (p_kld) {
      out[0] = (float)(red[0][0] + (double)beta * red[1][0]);
      out[1] = (float)red[0][0];
      out[2] = (float)red[1][0];
    } else {
      out[0] = (float)red[0][0];
    }
  }
}

// reparam_kernel with the noise drawn in the kernel (one Philox block per 4 elements, as q_sample_philox_kernel);
// the drawn eps is written out for the backward pass
__global__ void __launch_bounds__(256)
reparam_philox_kernel(const float* __restrict__ mu, const float* __restrict__ logvar, float* __restrict__ z,
                      float* __restrict__ eps_out, int64_t n, uint64_t seed, uint64_t offset) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q * 4 >= n) return;
  const float4 e4 = philox_normal4((uint64_t)q, offset, seed);
  const float e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = q * 4 + k;
    if (i < n) {
      z[i] = mu[i] + e[k] * expf(0.5f * logvar[i]);
      eps_out[i] = e[k];
    }
  }
}

// ReLU backward in place with the bias gradient of the layer below: g = h > 0 ? g : 0, db[n] = sum_m g[m][n]
// (h is the post-activation output, dense M x N like g).  colsum_kernel's block shape and order.
__global__ void __launch_bounds__(256)
relu_bwd_colsum_kernel(float* __restrict__ g, const float* __restrict__ h, int M, int N, float* __restrict__ db) {
  __shared__ float red[8][32];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5, n = blockIdx.x * 32 + cl;
  float s = 0.f;
  if (n < N)
    for (int m = sl; m < M; m += 8) {
      const size_t i = (size_t)m * N + n;
      const float v = h[i] > 0.f ? g[i] : 0.f;
      g[i] = v;
      s += v;
    }
  red[sl][cl] = s;
  __syncthreads();
  if (sl == 0 && n < N) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) v += red[k][cl];
    db[n] = v;
  }
}

inline int vae_loss_grid(int64_t n) {
  const int64_t g = (n + 1023) / 1024;
  return (int)(g > VAE_LOSS_BLOCKS ? VAE_LOSS_BLOCKS : g);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int vae_bce_launch(const float* a, const float* x, float* d_a, float* recon, float gscale, int64_t n, double* partials,
                   int grid, hipStream_t st) {
  if (al16(a) && al16(x) && al16(d_a) && al16(recon))
    vae_bce_logits_grad_kernel<true><<<grid, 256, 0, st>>>(a, x, d_a, recon, gscale, n, partials);
  else
    vae_bce_logits_grad_kernel<false><<<grid, 256, 0, st>>>(a, x, d_a, recon, gscale, n, partials);
  TDX_CHECK_LAUNCH();
  return 0;
}

struct VaeLayout {
  size_t h1, mu, logvar, eps, z, h3, a, d_a, g_h3, g_z, g_mu, g_logvar, g_h1, partials, total;
};

VaeLayout vae_train_layout(int B, int D, int H, int L) {
  VaeLayout V;
  size_t o = 0;
  auto take = [&](size_t n) { size_t r = o; o += al64(n); return r; };
  const size_t b = (size_t)B;
  V.h1 = take(b * H); V.mu = take(b * L); V.logvar = take(b * L); V.eps = take(b * L); V.z = take(b * L);
  V.h3 = take(b * H); V.a = take(b * D); V.d_a = take(b * D); V.g_h3 = take(b * H); V.g_z = take(b * L);
  V.g_mu = take(b * L); V.g_logvar = take(b * L); V.g_h1 = take(b * H);
  V.partials = take(2 * VAE_LOSS_BLOCKS * (sizeof(double) / sizeof(float)));   // BCE | KLD double partials
  V.total = o;
  return V;
}

}  // namespace

extern "C" size_t tdx_vae_loss_scratch_bytes(void) { return VAE_LOSS_BLOCKS * sizeof(double); }

extern "C" int tdx_vae_bce_logits_grad(const float* logits, const float* x, float* loss_out, float* d_logits,
                                       float* recon, float gscale, int64_t n, void* scratch, tdx_stream_t stream) {
  if (!logits || !x || !loss_out || !scratch || n <= 0 || (reinterpret_cast<uintptr_t>(scratch) & 7)) return TDX_E_BADARG;
  hipStream_t st = to_stream(stream);
  double* partials = static_cast<double*>(scratch);
  const int grid = vae_loss_grid(n);
  RC(vae_bce_launch(logits, x, d_logits, recon, gscale, n, partials, grid, st));
  vae_loss_finish_kernel<<<1, 256, 0, st>>>(partials, grid, nullptr, 0, 0.f, loss_out);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_vae_kld_reparam_bwd(const float* mu, const float* logvar, const float* eps, const float* g_z,
                                       float* kld_out, float* g_mu, float* g_logvar, float kld_weight, int64_t n,
                                       void* scratch, tdx_stream_t stream) {
  if (!mu || !logvar || !kld_out || !scratch || n <= 0 || (reinterpret_cast<uintptr_t>(scratch) & 7)) return TDX_E_BADARG;
  if (g_z && (!eps || !g_mu || !g_logvar)) return TDX_E_BADARG;
  hipStream_t st = to_stream(stream);
  double* partials = static_cast<double*>(scratch);
  const int grid = vae_loss_grid(n);
  vae_kld_reparam_bwd_kernel<<<grid, 256, 0, st>>>(mu, logvar, eps, g_z, g_mu, g_logvar, kld_weight, n, partials);
  TDX_CHECK_LAUNCH();
  vae_loss_finish_kernel<<<1, 256, 0, st>>>(partials, grid, nullptr, 0, 0.f, kld_out);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_vae_reparameterize_philox(const float* mu, const float* logvar, float* z, float* eps_out,
                                             int64_t n, uint64_t seed, uint64_t offset, tdx_stream_t stream) {
  if (!mu || !logvar || !z || !eps_out || n <= 0) return TDX_E_BADARG;
  reparam_philox_kernel<<<cdiv(cdiv(n, 4), 256), 256, 0, to_stream(stream)>>>(mu, logvar, z, eps_out, n, seed, offset);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t tdx_vae_train_workspace_floats(int batch, int input_dim, int hidden_dim, int latent_dim) {
  if (batch <= 0 || input_dim <= 0 || hidden_dim <= 0 || latent_dim <= 0) return 0;
  return vae_train_layout(batch, input_dim, hidden_dim, latent_dim).total;
}

// vae.py:64-76 and loss.backward() in one call.  params / grads: fc1.w fc1.b fc21.w fc21.b fc22.w fc22.b fc3.w
// fc3.b fc4.w fc4.b; grads == NULL: forward and losses only.  eps == NULL: drawn from Philox (seed, offset).
// out3 = {BCE + kld_weight KLD, BCE, KLD}; the gradients are those of gscale * out3[0].
extern "C" int tdx_vae_loss_grads(const float* x, const void* const* params, void* const* grads, const float* eps,
                                  uint64_t seed, uint64_t offset, float kld_weight, float gscale, float* out3,
                                  float* workspace, int batch, int input_dim, int hidden_dim, int latent_dim,
                                  tdx_stream_t stream) {
  if (!x || !params || !out3 || !workspace || batch <= 0 || input_dim <= 0 || hidden_dim <= 0 || latent_dim <= 0)
    return TDX_E_BADARG;
  if (!(kld_weight >= 0.f)) return TDX_E_BADARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return TDX_E_BADARG;   // the double partials live inside it
  const float* const* P = reinterpret_cast<const float* const*>(params);
  float* const* G = reinterpret_cast<float* const*>(grads);
  for (int i = 0; i < 10; ++i)
    if (!P[i] || (G && !G[i])) return TDX_E_BADARG;
  hipStream_t st = to_stream(stream);
  const int B = batch, D = input_dim, H = hidden_dim, L = latent_dim;
  const VaeLayout V = vae_train_layout(B, D, H, L);
  float* ws = workspace;
  double* p_bce = reinterpret_cast<double*>(ws + V.partials);
  double* p_kld = p_bce + VAE_LOSS_BLOCKS;
  const int64_t nz = (int64_t)B * L;
  // forward (vae.py:51-67; the last layer without its sigmoid: the loss works on the logit)
  RC(linear_fwd(x, D, P[0], P[1], ws + V.h1, H, B, H, D, 1, nullptr, nullptr, nullptr, 0, st));
  RC(linear_fwd(ws + V.h1, H, P[2], P[3], ws + V.mu, L, B, L, H, 0, nullptr, nullptr, nullptr, 0, st));
  RC(linear_fwd(ws + V.h1, H, P[4], P[5], ws + V.logvar, L, B, L, H, 0, nullptr, nullptr, nullptr, 0, st));
  if (eps) {
    reparam_kernel<<<cdiv(nz, 256), 256, 0, st>>>(ws + V.mu, ws + V.logvar, eps, ws + V.z, nz);
  } else {
    reparam_philox_kernel<<<cdiv(cdiv(nz, 4), 256), 256, 0, st>>>(ws + V.mu, ws + V.logvar, ws + V.z, ws + V.eps, nz,
                                                                   seed, offset);
    eps = ws + V.eps;
  }
  TDX_CHECK_LAUNCH();
  RC(linear_fwd(ws + V.z, L, P[6], P[7], ws + V.h3, H, B, H, L, 1, nullptr, nullptr, nullptr, 0, st));
  RC(linear_fwd(ws + V.h3, H, P[8], P[9], ws + V.a, D, B, D, H, 0, nullptr, nullptr, nullptr, 0, st));
  // vae.py:71-76
  const int g_bce = vae_loss_grid((int64_t)B * D), g_kld = vae_loss_grid(nz);
  RC(vae_bce_launch(ws + V.a, x, G ? ws + V.d_a : nullptr, nullptr, gscale, (int64_t)B * D, p_bce, g_bce, st));
  if (!G) {
    vae_kld_reparam_bwd_kernel<<<g_kld, 256, 0, st>>>(ws + V.mu, ws + V.logvar, nullptr, nullptr, nullptr, nullptr,
                                                      0.f, nz, p_kld);
    TDX_CHECK_LAUNCH();
    vae_loss_finish_kernel<<<1, 256, 0, st>>>(p_bce, g_bce, p_kld, g_kld, kld_weight, out3);
    TDX_CHECK_LAUNCH();
    return 0;
  }
  // backward: fc4, fc3
  RC(linear_wgrad(ws + V.d_a, D, ws + V.h3, H, G[8], B, D, H, st));
  RC(colsum(ws + V.d_a, D, B, D, G[9], st));
  RC(linear_dgrad(ws + V.d_a, D, P[8], ws + V.g_h3, H, B, D, H, 0, st));
  relu_bwd_colsum_kernel<<<cdiv(H, 32), 256, 0, st>>>(ws + V.g_h3, ws + V.h3, B, H, G[7]);
  TDX_CHECK_LAUNCH();
  RC(linear_wgrad(ws + V.g_h3, H, ws + V.z, L, G[6], B, H, L, st));
  RC(linear_dgrad(ws + V.g_h3, H, P[6], ws + V.g_z, L, B, H, L, 0, st));
  // KLD and the reparameterisation
  vae_kld_reparam_bwd_kernel<<<g_kld, 256, 0, st>>>(ws + V.mu, ws + V.logvar, eps, ws + V.g_z, ws + V.g_mu,
                                                    ws + V.g_logvar, kld_weight * gscale, nz, p_kld);
  TDX_CHECK_LAUNCH();
  vae_loss_finish_kernel<<<1, 256, 0, st>>>(p_bce, g_bce, p_kld, g_kld, kld_weight, out3);
  TDX_CHECK_LAUNCH();
  // fc21, fc22: the encoder-side input gradient is one accumulate chain
  RC(linear_wgrad(ws + V.g_mu, L, ws + V.h1, H, G[2], B, L, H, st));
  RC(colsum(ws + V.g_mu, L, B, L, G[3], st));
  RC(linear_wgrad(ws + V.g_logvar, L, ws + V.h1, H, G[4], B, L, H, st));
  RC(colsum(ws + V.g_logvar, L, B, L, G[5], st));
  RC(linear_dgrad(ws + V.g_mu, L, P[2], ws + V.g_h1, H, B, L, H, 0, st));
  RC(linear_dgrad(ws + V.g_logvar, L, P[4], ws + V.g_h1, H, B, L, H, 1, st));
  relu_bwd_colsum_kernel<<<cdiv(H, 32), 256, 0, st>>>(ws + V.g_h1, ws + V.h1, B, H, G[1]);
  TDX_CHECK_LAUNCH();
  // fc1 (no input gradient of x)
  return linear_wgrad(ws + V.g_h1, H, x, D, G[0], B, H, D, st);
}

// ------------------------------------------------------------------------------------------
// Building blocks of the "transformer" noise model of diffusion_transformer.py:16-107 (sequence
// length 1: attention(x) == out_proj(v_proj(x)); LayerNorm, GELU, SiLU, dropout, residual adds).
// All latency-bound elementwise / row kernels on (B, 256..1024) activations.
namespace {

// one wave per row; a lane keeps its N/64 values in registers (N % 64 == 0, N <= 1024)
template <int PER>
__global__ void __launch_bounds__(256)
layernorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                     const float* __restrict__ beta, float* __restrict__ out, float* __restrict__ mean_out,
                     float* __restrict__ rstd_out, int M, float eps) {
  constexpr int N = PER * 64;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  float v[PER];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < PER; ++i) { v[i] = x[(size_t)row * N + lane + 64 * i]; s += v[i]; }
  const float mean = wave_sum(s) / (float)N;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < PER; ++i) { const float d = v[i] - mean; q = fmaf(d, d, q); }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)N + eps);
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = lane + 64 * i;
    out[(size_t)row * N + c] = (v[i] - mean) * rstd * gamma[c] + beta[c];
  }
  if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
}

// gx = rstd * (a - mean(a) - xhat * mean(a * xhat)),  a = gy * gamma
template <int PER>
__global__ void __launch_bounds__(256)
layernorm_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ gamma,
                     const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ gx,
                     int M) {
  constexpr int N = PER * 64;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float mu = mean[row], rs = rstd[row];
  float a[PER], xh[PER];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = lane + 64 * i;
    xh[i] = (x[(size_t)row * N + c] - mu) * rs;
    a[i] = gy[(size_t)row * N + c] * gamma[c];
    s1 += a[i];
    s2 = fmaf(a[i], xh[i], s2);
  }
  s1 = wave_sum(s1) / (float)N;
  s2 = wave_sum(s2) / (float)N;
#pragma unroll
  for (int i = 0; i < PER; ++i) gx[(size_t)row * N + lane + 64 * i] = rs * (a[i] - s1 - xh[i] * s2);
}

// dgamma[c] = sum_rows gy * xhat, dbeta[c] = sum_rows gy; block = 32 columns x 8 row slices
__global__ void __launch_bounds__(256)
layernorm_param_grad_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                            const float* __restrict__ mean, const float* __restrict__ rstd,
                            float* __restrict__ dgamma, float* __restrict__ dbeta, int M, int N) {
  __shared__ float red[2][8][32];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
  float sg = 0.f, sb = 0.f;
  if (c < N)
    for (int m = sl; m < M; m += 8) {
      const float g = gy[(size_t)m * N + c];
      sg = fmaf(g, (x[(size_t)m * N + c] - mean[m]) * rstd[m], sg);
      sb += g;
    }
  red[0][sl][cl] = sg;
  red[1][sl][cl] = sb;
  __syncthreads();
  if (sl == 0 && c < N) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) { a += red[0][k][cl]; b += red[1][k][cl]; }
    dgamma[c] = a;
    dbeta[c] = b;
  }
}

__device__ inline float act_f(float x, int kind) {
  if (kind == 0) return x / (1.0f + expf(-x));                      // SiLU
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));     // GELU (erf form, nn.GELU default)
}
__device__ inline float act_grad_f(float x, int kind) {
  if (kind == 0) {
    const float s = 1.0f / (1.0f + expf(-x));
    return s * (1.0f + x * (1.0f - s));
  }
  const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
  return cdf + x * 0.39894228040143267794f * expf(-0.5f * x * x);
}
__global__ void act_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n, int kind) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = act_f(x[i], kind);
}
__global__ void act_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                               float* __restrict__ gx, int64_t n, int kind) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) gx[i] = gy[i] * act_grad_f(x[i], kind);
}

// out = x * keep / (1 - p); one Bernoulli(1-p) draw per `group` consecutive elements
// (group = 1: nn.Dropout; group = head_dim: dropout of the single attention weight of a head)
__global__ void dropout_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n, int group,
                               float p, float scale, uint64_t seed, uint64_t offset) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t gidx = (uint64_t)(i / group);
  const Philox4 r = philox4x32_10(gidx >> 2, offset, seed);
  const float u = ((float)r.v[gidx & 3] + 0.5f) * 2.3283064365386963e-10f;
  out[i] = u < p ? 0.f : x[i] * scale;
}

__global__ void add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                           int64_t n, int64_t period) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + b[period ? i % period : i];
}

__global__ void embedding_fwd_kernel(const float* __restrict__ w, const int64_t* __restrict__ idx,
                                     float* __restrict__ out, int M, int N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (int64_t)M * N) out[i] = w[(size_t)idx[i / N] * N + i % N];
}
// dE[c][j] = sum_{m : idx[m] == c} g[m][j]   (fixed order: deterministic)
__global__ void embedding_bwd_kernel(const float* __restrict__ g, const int64_t* __restrict__ idx,
                                     float* __restrict__ dw, int M, int N, int num) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num * N) return;
  const int c = i / N, j = i - c * N;
  float s = 0.f;
  for (int m = 0; m < M; ++m)
    if ((int)idx[m] == c) s += g[(size_t)m * N + j];
  dw[i] = s;
}

}  // namespace

// every N % 64 == 0, N <= 1024 (the contract of include/tdx.h): one instantiation per N / 64
#define TDX_LN_CASE(KERNEL, P_, ...) \
  case P_: KERNEL<P_><<<cdiv(M, 4), 256, 0, st>>>(__VA_ARGS__); break;
#define TDX_LN_DISPATCH(KERNEL, ...)                                              \
  switch (N / 64) {                                                               \
    TDX_LN_CASE(KERNEL, 1, __VA_ARGS__) TDX_LN_CASE(KERNEL, 2, __VA_ARGS__)       \
    TDX_LN_CASE(KERNEL, 3, __VA_ARGS__) TDX_LN_CASE(KERNEL, 4, __VA_ARGS__)       \
    TDX_LN_CASE(KERNEL, 5, __VA_ARGS__) TDX_LN_CASE(KERNEL, 6, __VA_ARGS__)       \
    TDX_LN_CASE(KERNEL, 7, __VA_ARGS__) TDX_LN_CASE(KERNEL, 8, __VA_ARGS__)       \
    TDX_LN_CASE(KERNEL, 9, __VA_ARGS__) TDX_LN_CASE(KERNEL, 10, __VA_ARGS__)      \
    TDX_LN_CASE(KERNEL, 11, __VA_ARGS__) TDX_LN_CASE(KERNEL, 12, __VA_ARGS__)     \
    TDX_LN_CASE(KERNEL, 13, __VA_ARGS__) TDX_LN_CASE(KERNEL, 14, __VA_ARGS__)     \
    TDX_LN_CASE(KERNEL, 15, __VA_ARGS__) TDX_LN_CASE(KERNEL, 16, __VA_ARGS__)     \
    default: return TDX_E_SHAPE;                                                  \
  }

extern "C" int tdx_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* out,
                                 float* mean, float* rstd, int M, int N, float eps, tdx_stream_t stream) {
  if (!x || !gamma || !beta || !out || !mean || !rstd || M <= 0 || N <= 0) return TDX_E_BADARG;
  if (N % 64) return TDX_E_SHAPE;
  hipStream_t st = to_stream(stream);
  TDX_LN_DISPATCH(layernorm_fwd_kernel, x, gamma, beta, out, mean, rstd, M, eps)
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_layernorm_bwd(const float* gy, const float* x, const float* gamma, const float* mean,
                                 const float* rstd, float* gx, float* dgamma, float* dbeta, int M, int N,
                                 tdx_stream_t stream) {
  if (!gy || !x || !gamma || !mean || !rstd || M <= 0 || N <= 0) return TDX_E_BADARG;
  if (N % 64) return TDX_E_SHAPE;
  hipStream_t st = to_stream(stream);
  if (gx) {
    TDX_LN_DISPATCH(layernorm_bwd_kernel, gy, x, gamma, mean, rstd, gx, M)
    TDX_CHECK_LAUNCH();
  }
  if (dgamma && dbeta) {
    layernorm_param_grad_kernel<<<cdiv(N, 32), 256, 0, st>>>(gy, x, mean, rstd, dgamma, dbeta, M, N);
    TDX_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int tdx_act_fwd(const float* x, float* out, int64_t n, int kind, tdx_stream_t stream) {
  if (!x || !out || n <= 0 || kind < 0 || kind > 1) return TDX_E_BADARG;
  act_fwd_kernel<<<cdiv(n, 256), 256, 0, to_stream(stream)>>>(x, out, n, kind);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_act_bwd(const float* gy, const float* x, float* gx, int64_t n, int kind, tdx_stream_t stream) {
  if (!gy || !x || !gx || n <= 0 || kind < 0 || kind > 1) return TDX_E_BADARG;
  act_bwd_kernel<<<cdiv(n, 256), 256, 0, to_stream(stream)>>>(gy, x, gx, n, kind);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_dropout(const float* x, float* out, int64_t n, int group, float p, uint64_t seed,
                           uint64_t offset, tdx_stream_t stream) {
  if (!x || !out || n <= 0 || group <= 0 || !(p >= 0.f && p < 1.f)) return TDX_E_BADARG;
  dropout_kernel<<<cdiv(n, 256), 256, 0, to_stream(stream)>>>(x, out, n, group, p, 1.0f / (1.0f - p), seed, offset);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_add(const float* a, const float* b, float* out, int64_t n, int64_t b_period, tdx_stream_t stream) {
  if (!a || !b || !out || n <= 0 || b_period < 0) return TDX_E_BADARG;
  add_kernel<<<cdiv(n, 256), 256, 0, to_stream(stream)>>>(a, b, out, n, b_period);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_embedding_fwd(const float* weight, const int64_t* idx, float* out, int M, int N,
                                 tdx_stream_t stream) {
  if (!weight || !idx || !out || M <= 0 || N <= 0) return TDX_E_BADARG;
  embedding_fwd_kernel<<<cdiv((int64_t)M * N, 256), 256, 0, to_stream(stream)>>>(weight, idx, out, M, N);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_embedding_bwd(const float* g, const int64_t* idx, float* dweight, int M, int N, int num,
                                 tdx_stream_t stream) {
  if (!g || !idx || !dweight || M <= 0 || N <= 0 || num <= 0) return TDX_E_BADARG;
  embedding_bwd_kernel<<<cdiv((int64_t)num * N, 256), 256, 0, to_stream(stream)>>>(g, idx, dweight, M, N, num);
  TDX_CHECK_LAUNCH();
  return 0;
}
