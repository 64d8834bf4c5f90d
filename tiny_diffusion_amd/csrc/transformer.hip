// Training of the "transformer" noise model (diffusion_transformer.py:16-107): forward, F.mse_loss and the whole
// backward in one call, tdx_transformer_loss_grads.  The model runs nn.MultiheadAttention on a length-1 sequence, so a
// block is  x1 = LN(x + drop(out_proj(drop_head(v_proj(x))))),  x2 = LN(x1 + drop(drop(ff2(gelu(ff1(x1)))))).
//
// As in mlp.hip nothing here is throughput-bound: every tensor is (B, 256..1024) with B ~ 128 and the cost is the
// length of the dependent launch chain.  The op-by-op module takes 13 launches per block forward and 21 backward; this
// file takes 6 and 6 (DESIGN.md has the counted table):
//   * the latency GEMM of mlp.hip (32 x 32 tiles, split-K over the four waves, register prefetch) with the epilogues
//     this model needs: GELU with the pre-activation kept, the head dropout, the gathered class embedding + the
//     position row, act'(saved) on an input gradient, a residual addend; a weight gradient also emits the bias
//     gradient (the column sums of the operand it stages anyway) and clears the Q / K thirds of in_proj;
//   * the weight gradient and the input gradient of one Linear share ONE launch (they read the same gy and do not
//     depend on each other): the first workgroups of the grid run one problem, the rest the other;
//   * residual add + dropout + LayerNorm as one row kernel (one wave per row, dim / 64 values per lane in registers),
//     and its backward - LayerNorm input gradient, residual gradient added, dropout masks on the branch gradient - as
//     one more, whose trailing workgroups reduce dgamma / dbeta over the rows in a fixed order.
// Dropout masks are never stored: forward and backward draw them from Philox (tdx_dropout's element -> draw map).
#include "internal.h"

namespace {

constexpr int GT = 32;    // output tile edge (one workgroup)
constexpr int GKC = 128;  // k-chunk staged per iteration; each of the 4 waves reduces a quarter of it
constexpr int GLD = GT + 4;

// where the kernels find (seed, offset): two device words (a captured step refreshes them between replays) or by value
struct RngRef { const uint64_t* dev; uint64_t seed, offset; };

__device__ inline void rng_load(const RngRef& r, int site, uint64_t& seed, uint64_t& stream) {
  seed = r.dev ? r.dev[0] : r.seed;
  stream = (r.dev ? r.dev[1] : r.offset) + (uint64_t)site;
}

// dropout_kernel's draw (mlp.hip): element group gidx takes lane gidx & 3 of Philox block gidx >> 2; kept iff u >= p
__device__ inline bool drop_keep(uint64_t gidx, uint64_t stream, uint64_t seed, float p) {
  const Philox4 r = philox4x32_10(gidx >> 2, stream, seed);
  const uint32_t k = (uint32_t)(gidx & 3);
  const uint32_t w = k == 0 ? r.v[0] : k == 1 ? r.v[1] : k == 2 ? r.v[2] : r.v[3];
  const float u = ((float)w + 0.5f) * 2.3283064365386963e-10f;
  return !(u < p);
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

// C[M x N] (ldc) = epilogue(sum_k A(m, k) B(k, n)); the operand layouts are template flags as in mlp.hip
struct TG {
  const float* A; const float* B; float* C;
  int M, N, K, lda, ldb, ldc;
  const float* bias;      // [N] or null
  float* pre;             // [M x N] (ldc) or null: acc + bias is stored here too (the pre-activation, for backward)
  int act;                // 0 none, 1 GELU
  const float* gact;      // [M x N] (ldc) or null: v *= act'(gact) - an input gradient through the activation
  int gkind;              //   0 SiLU, 1 GELU
  int drop_site;          // 0 none; else v = keep ? v * drop_scale : 0, one draw per drop_group elements of the
  int drop_group;         //   dense (M, N) tensor (ldc == N), Philox stream offset + drop_site
  float drop_p, drop_scale;
  const float* gtab;      // v += gtab[gidx[m] * N + n] (the class embedding), or null
  const int64_t* gidx;
  const float* rowvec;    // v += rowvec[n], or null
  const float* addrow;    // v += addrow[m * ldr + n], or null
  int ldr;
  float* dbias;           // [M] or null: sum_k A(m, k), written by the workgroups of the first tile column
  float* zero0; float* zero1;   // buffers this launch clears (grid-strided over its workgroups), or null
  int nzero0, nzero1;
};

__device__ inline void load4(const float* __restrict__ src, bool vec, bool row_ok, int c, int C, float* v) {
  if (vec && row_ok && c + 3 < C) {  // one 16-byte load
    const float4 q = *reinterpret_cast<const float4*>(src);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {                           // unaligned leading dimension / edge: scalar, bounds-checked
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (row_ok && c + i < C) ? src[i] : 0.f;
  }
}

// KC: element (r, k) at P[r*ld + k], else at P[k*ld + r]
template <bool KC>
__device__ inline void stage_load(const float* __restrict__ P, int ld, int r0, int R, int k0, int K, int t,
                                  float (&v)[16]) {
  const bool vec = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(P) & 15) == 0);
  if (KC) {
    const int r = r0 + (t & 31);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + ((t >> 5) + 8 * j) * 4;
      load4(P + (size_t)r * ld + k, vec, r < R, k, K, &v[j * 4]);
    }
  } else {
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

inline int tg_blocks(const TG& g) { return cdiv(g.N, GT) * cdiv(g.M, GT); }

// one 32 x 32 tile of problem g by the calling workgroup; blk in [0, nblk) is its index among the problem's workgroups
template <bool A_KC, bool B_KC>
__device__ inline void gemm_tile(const TG& g, const RngRef& rng, int blk, int nblk, float (*As)[GLD],
                                 float (*Bs)[GLD]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, tx = lane & 7, ty = lane >> 3;
  const int tiles_n = (g.N + GT - 1) / GT;
  const int m0 = (blk / tiles_n) * GT, n0 = (blk % tiles_n) * GT;
  if (g.zero0)
    for (int i = blk * 256 + t; i < g.nzero0; i += nblk * 256) g.zero0[i] = 0.f;
  if (g.zero1)
    for (int i = blk * 256 + t; i < g.nzero1; i += nblk * 256) g.zero1[i] = 0.f;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
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
      for (int i = 0; i < 4; ++i) {
        bsum[i] += av[i];   // rows of A past K are staged as zeros
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
      }
    }
  }
  // reduce the four waves' partial tiles (fixed order: deterministic), then the epilogue
  __syncthreads();
  float(*Red)[GT * GT] = reinterpret_cast<float(*)[GT * GT]>(&As[0][0]);  // 4 x 1024 floats <= sizeof(As)
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<float4*>(&Red[wave][(ty * 4 + i) * GT + tx * 4]) =
        make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
  const bool want_db = g.dbias != nullptr && n0 == 0;
  if (want_db && tx == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) Bs[wave][ty * 4 + i] = bsum[i];
  }
  __syncthreads();
  if (want_db && t < GT && m0 + t < g.M) g.dbias[m0 + t] = ((Bs[0][t] + Bs[1][t]) + Bs[2][t]) + Bs[3][t];
  uint64_t seed = 0, stream = 0;
  if (g.drop_site) rng_load(rng, g.drop_site, seed, stream);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = q * 256 + t, mi = e >> 5, ni = e & 31;  // consecutive threads -> consecutive columns
    const int m = m0 + mi, n = n0 + ni;
    if (m >= g.M || n >= g.N) continue;
    const size_t ci = (size_t)m * g.ldc + n;
    float v = ((Red[0][e] + Red[1][e]) + Red[2][e]) + Red[3][e];
    if (g.bias) v += g.bias[n];
    if (g.pre) g.pre[ci] = v;
    if (g.act == 1) v = act_f(v, 1);
    if (g.gact) v *= act_grad_f(g.gact[ci], g.gkind);
    if (g.drop_site) v = drop_keep((uint64_t)ci / (uint64_t)g.drop_group, stream, seed, g.drop_p) ? v * g.drop_scale : 0.f;
    if (g.gtab) v += g.gtab[(size_t)g.gidx[m] * g.N + n];
    if (g.rowvec) v += g.rowvec[n];
    if (g.addrow) v += g.addrow[(size_t)m * g.ldr + n];
    g.C[ci] = v;
  }
}

template <bool A_KC, bool B_KC>
__global__ void __launch_bounds__(256) tgemm_kernel(TG g, RngRef rng) {
  __shared__ __attribute__((aligned(16))) float As[GKC][GLD];
  __shared__ __attribute__((aligned(16))) float Bs[GKC][GLD];
  gemm_tile<A_KC, B_KC>(g, rng, blockIdx.x, gridDim.x, As, Bs);
}

// The two gradients of one Linear from the same gy: workgroups [0, nw) compute dW = gy^T x (+ db), the rest
// gx = gy W (+ its epilogue).  The branch is uniform per workgroup.
__global__ void __launch_bounds__(256) tgemm_bwd_pair_kernel(TG w, TG d, int nw, RngRef rng) {
  __shared__ __attribute__((aligned(16))) float As[GKC][GLD];
  __shared__ __attribute__((aligned(16))) float Bs[GKC][GLD];
  if ((int)blockIdx.x < nw) gemm_tile<false, false>(w, rng, blockIdx.x, nw, As, Bs);
  else gemm_tile<true, false>(d, rng, blockIdx.x - nw, gridDim.x - nw, As, Bs);
}

TG tg(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K) {
  TG g{};
  g.A = A; g.B = B; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  return g;
}

// out = epilogue(X W^T): X (M, K) ldx, W (N, K)
int launch_fwd(const TG& g, const RngRef& rng, hipStream_t st) {
  tgemm_kernel<true, true><<<tg_blocks(g), 256, 0, st>>>(g, rng);
  TDX_CHECK_LAUNCH();
  return 0;
}
int launch_wgrad(const TG& w, const RngRef& rng, hipStream_t st) {
  tgemm_kernel<false, false><<<tg_blocks(w), 256, 0, st>>>(w, rng);
  TDX_CHECK_LAUNCH();
  return 0;
}
int launch_bwd_pair(const TG& w, const TG& d, const RngRef& rng, hipStream_t st) {
  const int nw = tg_blocks(w);
  tgemm_bwd_pair_kernel<<<nw + tg_blocks(d), 256, 0, st>>>(w, d, nw, rng);
  TDX_CHECK_LAUNCH();
  return 0;
}
// dW (N, K) = gy (M, N)^T x (M, K), db (N) = column sums of gy
TG tg_wgrad(const float* gy, int ldgy, const float* x, int ldx, float* dw, float* db, int M, int N, int K) {
  TG g = tg(gy, ldgy, x, ldx, dw, K, N, K, M);
  g.dbias = db;
  return g;
}
// gx (M, K) ldgx = gy (M, N) W (N, K)
TG tg_dgrad(const float* gy, int ldgy, const float* w, float* gx, int ldgx, int M, int N, int K) {
  return tg(gy, ldgy, w, K, gx, ldgx, M, K, N);
}

// ------------------------------------------------------------------ row kernels
// the dropout sites a row kernel applies to its branch operand: nsites consecutive Philox streams from site0, group 1
struct DropRow { int nsites, site0; float p, scale; };

// s = x + drop(a) (a null: s = x), out = LN(s); one wave per row, PER = N / 64 values per lane
template <int PER>
__global__ void __launch_bounds__(256)
rowln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ a, float* __restrict__ s_out,
                 const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ out,
                 float* __restrict__ mean_out, float* __restrict__ rstd_out, int M, float eps, DropRow dr, RngRef rng) {
  constexpr int N = PER * 64;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  uint64_t seed = 0, stream = 0;
  if (dr.nsites) rng_load(rng, dr.site0, seed, stream);
  float v[PER];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const size_t idx = (size_t)row * N + lane + 64 * i;
    v[i] = x[idx];
    if (a) {
      float av = a[idx];
      for (int k = 0; k < dr.nsites; ++k) av = drop_keep(idx, stream + k, seed, dr.p) ? av * dr.scale : 0.f;
      v[i] += av;
      s_out[idx] = v[i];
    }
    s += v[i];
  }
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

// gy = gy1 (+ gy2: the residual gradient that bypasses the next sub-layer).  Workgroups [0, rowblocks): one wave per row,
//   gs = rstd (g - mean(g) - xhat mean(g xhat)), g = gy gamma     (the gradient of s, which is also the residual's)
//   gbr = gs under the dropout masks of the branch (gbr_out null: no dropout, the caller uses gs).
// The workgroups after them: dgamma[c] = sum_rows gy xhat, dbeta[c] = sum_rows gy for 32 columns each, 8 row slices
// added in a fixed order.
template <int PER>
__global__ void __launch_bounds__(256)
rowln_bwd_kernel(const float* __restrict__ gy1, const float* __restrict__ gy2, const float* __restrict__ s,
                 const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ rstd,
                 float* __restrict__ gs_out, float* __restrict__ gbr_out, float* __restrict__ dgamma,
                 float* __restrict__ dbeta, int M, int rowblocks, DropRow dr, RngRef rng) {
  constexpr int N = PER * 64;
  __shared__ float red[2][8][32];
  if ((int)blockIdx.x >= rowblocks) {
    const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5, c = ((int)blockIdx.x - rowblocks) * 32 + cl;   // c < N
    float sg = 0.f, sb = 0.f;
    for (int m = sl; m < M; m += 8) {
      const size_t idx = (size_t)m * N + c;
      float g = gy1[idx];
      if (gy2) g += gy2[idx];
      sg = fmaf(g, (s[idx] - mean[m]) * rstd[m], sg);
      sb += g;
    }
    red[0][sl][cl] = sg;
    red[1][sl][cl] = sb;
    __syncthreads();
    if (sl == 0) {
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) { a += red[0][k][cl]; b += red[1][k][cl]; }
      dgamma[c] = a;
      dbeta[c] = b;
    }
    return;
  }
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  uint64_t seed = 0, stream = 0;
  if (gbr_out && dr.nsites) rng_load(rng, dr.site0, seed, stream);
  const float mu = mean[row], rs = rstd[row];
  float a[PER], xh[PER];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = lane + 64 * i;
    const size_t idx = (size_t)row * N + c;
    float g = gy1[idx];
    if (gy2) g += gy2[idx];
    xh[i] = (s[idx] - mu) * rs;
    a[i] = g * gamma[c];
    s1 += a[i];
    s2 = fmaf(a[i], xh[i], s2);
  }
  s1 = wave_sum(s1) / (float)N;
  s2 = wave_sum(s2) / (float)N;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const size_t idx = (size_t)row * N + lane + 64 * i;
    float g = rs * (a[i] - s1 - xh[i] * s2);
    gs_out[idx] = g;
    if (gbr_out) {
      for (int k = 0; k < dr.nsites; ++k) g = drop_keep(idx, stream + k, seed, dr.p) ? g * dr.scale : 0.f;
      gbr_out[idx] = g;
    }
  }
}

#define TDX_TF_CASE(KERNEL, GRID, P_, ...) \
  case P_: KERNEL<P_><<<GRID, 256, 0, st>>>(__VA_ARGS__); break;
#define TDX_TF_DISPATCH(KERNEL, GRID, ...)                                                          \
  switch (N / 64) {                                                                                 \
    TDX_TF_CASE(KERNEL, GRID, 1, __VA_ARGS__) TDX_TF_CASE(KERNEL, GRID, 2, __VA_ARGS__)             \
    TDX_TF_CASE(KERNEL, GRID, 3, __VA_ARGS__) TDX_TF_CASE(KERNEL, GRID, 4, __VA_ARGS__)             \
    TDX_TF_CASE(KERNEL, GRID, 5, __VA_ARGS__) TDX_TF_CASE(KERNEL, GRID, 6, __VA_ARGS__)             \
    TDX_TF_CASE(KERNEL, GRID, 7, __VA_ARGS__) TDX_TF_CASE(KERNEL, GRID, 8, __VA_ARGS__)             \
    TDX_TF_CASE(KERNEL, GRID, 9, __VA_ARGS__) TDX_TF_CASE(KERNEL, GRID, 10, __VA_ARGS__)            \
    TDX_TF_CASE(KERNEL, GRID, 11, __VA_ARGS__) TDX_TF_CASE(KERNEL, GRID, 12, __VA_ARGS__)           \
    TDX_TF_CASE(KERNEL, GRID, 13, __VA_ARGS__) TDX_TF_CASE(KERNEL, GRID, 14, __VA_ARGS__)           \
    TDX_TF_CASE(KERNEL, GRID, 15, __VA_ARGS__) TDX_TF_CASE(KERNEL, GRID, 16, __VA_ARGS__)           \
    default: return TDX_E_SHAPE;                                                                    \
  }

int rowln_fwd(const float* x, const float* a, float* s_out, const float* gamma, const float* beta, float* out,
              float* mean, float* rstd, int M, int N, float eps, DropRow dr, const RngRef& rng, hipStream_t st) {
  TDX_TF_DISPATCH(rowln_fwd_kernel, cdiv(M, 4), x, a, s_out, gamma, beta, out, mean, rstd, M, eps, dr, rng)
  TDX_CHECK_LAUNCH();
  return 0;
}

int rowln_bwd(const float* gy1, const float* gy2, const float* s, const float* gamma, const float* mean,
              const float* rstd, float* gs_out, float* gbr_out, float* dgamma, float* dbeta, int M, int N, DropRow dr,
              const RngRef& rng, hipStream_t st) {
  const int rowblocks = cdiv(M, 4);
  TDX_TF_DISPATCH(rowln_bwd_kernel, rowblocks + N / 32, gy1, gy2, s, gamma, mean, rstd, gs_out, gbr_out, dgamma, dbeta,
                  M, rowblocks, dr, rng)
  TDX_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------ stem
// time_embedding.0 has K = 1: pre = (t / 1000) w0 + b0 is an outer product, hs = silu(pre)
__global__ void stem_fwd_kernel(const int64_t* __restrict__ t, const float* __restrict__ w0,
                                const float* __restrict__ b0, float* __restrict__ pre, float* __restrict__ hs, int M,
                                int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * N) return;
  const int m = i / N, j = i - m * N;
  const float tn = (float)t[m] / 1000.0f;
  const float p = tn * w0[j] + b0[j];
  pre[i] = p;
  hs[i] = act_f(p, 0);
}

// The column sums of the stem's backward, one thread per output element, rows added in order (deterministic):
//   c <  ncls     dE[c][j]  = sum_{m : y[m] == c} gh[m][j]        (class_embedding; absent labels: exact zeros)
//   c == ncls     dpos[j]   = sum_m gh[m][j]
//   c == ncls + 1 dw0[j]    = sum_m gpre[m][j] t[m] / 1000        (time_embedding.0.weight)
//   c == ncls + 2 db0[j]    = sum_m gpre[m][j]
__global__ void stem_col_kernel(const float* __restrict__ gh, const float* __restrict__ gpre,
                                const int64_t* __restrict__ y, const int64_t* __restrict__ t, float* __restrict__ dE,
                                float* __restrict__ dpos, float* __restrict__ dw0, float* __restrict__ db0, int M,
                                int N, int ncls) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (ncls + 3) * N) return;
  const int c = i / N, j = i - c * N;
  float s = 0.f;
  if (c < ncls) {
    for (int m = 0; m < M; ++m)
      if ((int)y[m] == c) s += gh[(size_t)m * N + j];
    dE[i] = s;
  } else if (c == ncls) {
    for (int m = 0; m < M; ++m) s += gh[(size_t)m * N + j];
    dpos[j] = s;
  } else if (c == ncls + 1) {
    for (int m = 0; m < M; ++m) s = fmaf(gpre[(size_t)m * N + j], (float)t[m] / 1000.0f, s);
    dw0[j] = s;
  } else {
    for (int m = 0; m < M; ++m) s += gpre[(size_t)m * N + j];
    db0[j] = s;
  }
}

// ---------------------------------------------------------------------- layout
inline size_t al64(size_t n) { return (n + 63) / 64 * 64; }

struct BlockBuf { size_t v, a, s1, x1, u, g, f, s2, mean1, rstd1, mean2, rstd2; };
struct TLayout {
  size_t pre, hs, tmp, xf, meanf, rstdf, eps, dout, g0, g1, g2, g3, gF, mse, total;
  size_t X(int l) const { return x0 + (size_t)l * xstride; }
  BlockBuf blk(int l) const {
    BlockBuf b = b0;
    const size_t o = (size_t)l * bstride;
    b.v += o; b.a += o; b.s1 += o; b.x1 += o; b.u += o; b.g += o; b.f += o; b.s2 += o;
    b.mean1 += o; b.rstd1 += o; b.mean2 += o; b.rstd2 += o;
    return b;
  }
  size_t x0, xstride, bstride;
  BlockBuf b0;
};

bool shape_ok(const tdx_transformer_shape& s) {
  if (s.batch <= 0 || s.latent_dim <= 0 || s.dim <= 0 || s.num_heads <= 0 || s.num_layers <= 0 || s.num_classes <= 0)
    return false;
  if (s.dim % 64 || s.dim > 1024 || s.dim % s.num_heads) return false;
  if (!(s.dropout_p >= 0.f && s.dropout_p < 1.f) || !(s.ln_eps > 0.f)) return false;
  if ((int64_t)s.batch * s.dim * 4 > 0x7fffffff) return false;   // the kernels index (B, 4 dim) tensors with int
  return true;
}

TLayout layout(const tdx_transformer_shape& s) {
  TLayout Y;
  size_t o = 0;
  auto take = [&](size_t n) { size_t r = o; o += al64(n); return r; };
  const size_t b = (size_t)s.batch, D = (size_t)s.dim, F = 4 * D, Ld = (size_t)s.latent_dim;
  Y.pre = take(b * D); Y.hs = take(b * D); Y.tmp = take(b * D);
  Y.x0 = o; Y.xstride = al64(b * D);
  o += Y.xstride * (size_t)(s.num_layers + 1);
  const size_t blk0 = o;
  Y.b0.v = take(b * D); Y.b0.a = take(b * D); Y.b0.s1 = take(b * D); Y.b0.x1 = take(b * D);
  Y.b0.u = take(b * F); Y.b0.g = take(b * F); Y.b0.f = take(b * D); Y.b0.s2 = take(b * D);
  Y.b0.mean1 = take(b); Y.b0.rstd1 = take(b); Y.b0.mean2 = take(b); Y.b0.rstd2 = take(b);
  Y.bstride = o - blk0;
  o = blk0 + Y.bstride * (size_t)s.num_layers;
  Y.xf = take(b * D); Y.meanf = take(b); Y.rstdf = take(b);
  Y.eps = take(b * Ld); Y.dout = take(b * Ld);
  Y.g0 = take(b * D); Y.g1 = take(b * D); Y.g2 = take(b * D); Y.g3 = take(b * D); Y.gF = take(b * F);
  Y.mse = take(tdx_mse_scratch_bytes() / sizeof(float));
  Y.total = o;
  return Y;
}

}  // namespace

#define RC(call)            \
  do {                      \
    int rc__ = (call);      \
    if (rc__) return rc__;  \
  } while (0)

extern "C" size_t tdx_transformer_train_workspace_floats(const tdx_transformer_shape* shape) {
  return shape && shape_ok(*shape) ? layout(*shape).total : 0;
}

extern "C" int tdx_transformer_loss_grads(const tdx_transformer_shape* shape, const void* const* params,
                                          void* const* grads, const float* z_t, const int64_t* t, const int64_t* y,
                                          const float* target, const float* w_table, int train, uint64_t seed,
                                          uint64_t offset, const uint64_t* rng_dev, float gscale, float* loss_out,
                                          float* eps_hat_out, float* workspace, tdx_stream_t stream) {
  if (!shape || !params || !z_t || !t || !y || !target || !loss_out || !workspace) return TDX_E_BADARG;
  if (!shape_ok(*shape)) return TDX_E_SHAPE;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return TDX_E_BADARG;
  const int B = shape->batch, Ld = shape->latent_dim, D = shape->dim, F = 4 * D, L = shape->num_layers;
  const int hd = D / shape->num_heads, ncls = shape->num_classes;
  const float* const* P = reinterpret_cast<const float* const*>(params);
  float* const* G = reinterpret_cast<float* const*>(grads);
  for (int i = 0; i < 12 + 12 * L; ++i)
    if (!P[i] || (G && !G[i])) return TDX_E_BADARG;
  hipStream_t st = to_stream(stream);
  const bool drop = train != 0 && shape->dropout_p > 0.f;
  const float p = shape->dropout_p, scale = 1.0f / (1.0f - p);
  const RngRef rng{rng_dev, seed, offset};
  const DropRow none{0, 0, 0.f, 1.f};
  const TLayout Y = layout(*shape);
  float* ws = workspace;
  const size_t DD = (size_t)D * D;

  // ---- forward.  Stem (lines 86-98): h0 = input_proj(z) + (time_mlp(t) + class_emb[y] + pos)
  stem_fwd_kernel<<<cdiv((int64_t)B * D, 256), 256, 0, st>>>(t, P[1], P[2], ws + Y.pre, ws + Y.hs, B, D);
  TDX_CHECK_LAUNCH();
  {
    TG g = tg(ws + Y.hs, D, P[3], D, ws + Y.tmp, D, B, D, D);
    g.bias = P[4]; g.gtab = P[5]; g.gidx = y; g.rowvec = P[0];
    RC(launch_fwd(g, rng, st));
    g = tg(z_t, Ld, P[6], Ld, ws + Y.X(0), D, B, D, Ld);
    g.bias = P[7]; g.addrow = ws + Y.tmp; g.ldr = D;
    RC(launch_fwd(g, rng, st));
  }
  for (int l = 0; l < L; ++l) {
    const float* const* Pb = P + 8 + 12 * l;
    const BlockBuf b = Y.blk(l);
    const float* x = ws + Y.X(l);
    TG g = tg(x, D, Pb[0] + 2 * DD, D, ws + b.v, D, B, D, D);               // v_proj, dropout of the head weight
    g.bias = Pb[1] + 2 * D;
    if (drop) { g.drop_site = 4 * l + 1; g.drop_group = hd; g.drop_p = p; g.drop_scale = scale; }
    RC(launch_fwd(g, rng, st));
    g = tg(ws + b.v, D, Pb[2], D, ws + b.a, D, B, D, D);                     // out_proj
    g.bias = Pb[3];
    RC(launch_fwd(g, rng, st));
    RC(rowln_fwd(x, ws + b.a, ws + b.s1, Pb[4], Pb[5], ws + b.x1, ws + b.mean1, ws + b.rstd1, B, D, shape->ln_eps,
                 DropRow{drop ? 1 : 0, 4 * l + 2, p, scale}, rng, st));
    g = tg(ws + b.x1, D, Pb[6], D, ws + b.g, F, B, F, D);                    // ff.0 + GELU, pre-activation kept
    g.bias = Pb[7]; g.pre = ws + b.u; g.act = 1;
    RC(launch_fwd(g, rng, st));
    g = tg(ws + b.g, F, Pb[8], F, ws + b.f, D, B, D, F);                     // ff.2
    g.bias = Pb[9];
    RC(launch_fwd(g, rng, st));
    RC(rowln_fwd(ws + b.x1, ws + b.f, ws + b.s2, Pb[10], Pb[11], ws + Y.X(l + 1), ws + b.mean2, ws + b.rstd2, B, D,
                 shape->ln_eps, DropRow{drop ? 2 : 0, 4 * l + 3, p, scale}, rng, st));
  }
  const float* const* Pf = P + 8 + 12 * L;
  float* eps_hat = eps_hat_out ? eps_hat_out : ws + Y.eps;
  RC(rowln_fwd(ws + Y.X(L), nullptr, nullptr, Pf[0], Pf[1], ws + Y.xf, ws + Y.meanf, ws + Y.rstdf, B, D, shape->ln_eps,
               none, rng, st));
  {
    TG g = tg(ws + Y.xf, D, Pf[2], D, eps_hat, Ld, B, Ld, D);
    g.bias = Pf[3];
    RC(launch_fwd(g, rng, st));
  }
  // ---- loss (F.mse_loss, or the per-timestep weighted form) and d loss / d eps_hat
  float* d_out = G ? ws + Y.dout : nullptr;
  if (w_table)
    RC(tdx_mse_loss_grad_weighted(eps_hat, target, t, w_table, loss_out, d_out, gscale, B, Ld, ws + Y.mse, stream));
  else
    RC(tdx_mse_loss_grad(eps_hat, target, loss_out, d_out, gscale, (int64_t)B * Ld, ws + Y.mse, stream));
  if (!G) return 0;

  // ---- backward.  cur: the gradient of the current block's output; t1..t3: scratch of the same shape
  float *cur = ws + Y.g0, *t1 = ws + Y.g1, *t2 = ws + Y.g2, *t3 = ws + Y.g3, *gF = ws + Y.gF;
  float* const* Gf = G + 8 + 12 * L;
  RC(launch_bwd_pair(tg_wgrad(d_out, Ld, ws + Y.xf, D, Gf[2], Gf[3], B, Ld, D),
                     tg_dgrad(d_out, Ld, Pf[2], t1, D, B, Ld, D), rng, st));
  RC(rowln_bwd(t1, nullptr, ws + Y.X(L), Pf[0], ws + Y.meanf, ws + Y.rstdf, cur, nullptr, Gf[0], Gf[1], B, D, none,
               rng, st));
  for (int l = L - 1; l >= 0; --l) {
    const float* const* Pb = P + 8 + 12 * l;
    float* const* Gb = G + 8 + 12 * l;
    const BlockBuf b = Y.blk(l);
    // norm2 and the two dropouts of the ff branch: t1 = d s2 (also the residual's share of d x1), gf = the branch's
    RC(rowln_bwd(cur, nullptr, ws + b.s2, Pb[10], ws + b.mean2, ws + b.rstd2, t1, drop ? t2 : nullptr, Gb[10], Gb[11],
                 B, D, DropRow{drop ? 2 : 0, 4 * l + 3, p, scale}, rng, st));
    const float* gf = drop ? t2 : t1;
    TG d = tg_dgrad(gf, D, Pb[8], gF, F, B, D, F);                            // ff.2, then GELU' of the pre-activation
    d.gact = ws + b.u; d.gkind = 1;
    RC(launch_bwd_pair(tg_wgrad(gf, D, ws + b.g, F, Gb[8], Gb[9], B, D, F), d, rng, st));
    RC(launch_bwd_pair(tg_wgrad(gF, F, ws + b.x1, D, Gb[6], Gb[7], B, F, D),   // ff.0
                       tg_dgrad(gF, F, Pb[6], cur, D, B, F, D), rng, st));
    // norm1: d x1 = cur + t1;  t3 = d s1 (also the residual's share of d x), ga = the attention branch's
    RC(rowln_bwd(cur, t1, ws + b.s1, Pb[4], ws + b.mean1, ws + b.rstd1, t3, drop ? t2 : nullptr, Gb[4], Gb[5], B, D,
                 DropRow{drop ? 1 : 0, 4 * l + 2, p, scale}, rng, st));
    const float* ga = drop ? t2 : t3;
    d = tg_dgrad(ga, D, Pb[2], cur, D, B, D, D);                              // out_proj, then the head dropout
    if (drop) { d.drop_site = 4 * l + 1; d.drop_group = hd; d.drop_p = p; d.drop_scale = scale; }
    RC(launch_bwd_pair(tg_wgrad(ga, D, ws + b.v, D, Gb[2], Gb[3], B, D, D), d, rng, st));
    TG w = tg_wgrad(cur, D, ws + Y.X(l), D, Gb[0] + 2 * DD, Gb[1] + 2 * D, B, D, D);   // v_proj; Q / K: zeros
    w.zero0 = Gb[0]; w.nzero0 = (int)(2 * DD); w.zero1 = Gb[1]; w.nzero1 = 2 * D;
    d = tg_dgrad(cur, D, Pb[0] + 2 * DD, t1, D, B, D, D);
    d.addrow = t3; d.ldr = D;                                                 // + the residual
    RC(launch_bwd_pair(w, d, rng, st));
    float* sw = cur; cur = t1; t1 = sw;
  }
  // stem: cur = d h0
  {
    TG d = tg_dgrad(cur, D, P[3], t1, D, B, D, D);                            // time_embedding.2, then SiLU'
    d.gact = ws + Y.pre; d.gkind = 0;
    RC(launch_bwd_pair(tg_wgrad(cur, D, ws + Y.hs, D, G[3], G[4], B, D, D), d, rng, st));
    RC(launch_wgrad(tg_wgrad(cur, D, z_t, Ld, G[6], G[7], B, D, Ld), rng, st));   // input_proj
    stem_col_kernel<<<cdiv((int64_t)(ncls + 3) * D, 256), 256, 0, st>>>(cur, t1, y, t, G[5], G[0], G[1], G[2], B, D,
                                                                         ncls);
    TDX_CHECK_LAUNCH();
  }
  return 0;
}
