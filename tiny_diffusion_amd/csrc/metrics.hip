// Pairwise kernels of the sample-quality metrics (Frechet distance, KID, precision / recall; include/tdx.h): the inner
// products g_ij = a_i . b_j of two row-major fp32 feature matrices on the fp32 MFMA (v_mfma_f32_32x32x2_f32: exact fp32
// products, a k-ordered fmaf chain), with what the metric needs from the pair matrix taken in the epilogue - the pair
// matrix itself is written by the plain store (tdx_pair_gram) only.
//
// One workgroup of four waves owns 128 queries (rows of A) and walks a chunk of the candidates (rows of B) in tiles of
// 128, K in slices of 32 staged through LDS (row stride 33 floats: the operand reads of a k-step and the staging
// writes both fall on distinct banks).  The candidates are the MFMA's A operand and the queries its B operand, so the
// accumulator has the QUERY on the lane (column = lane & 31) and 16 candidates in registers: a wave keeps the k
// smallest distances, the membership flag or the row sum of its 32 queries as per-lane state over all 128 candidates
// of a tile (four accumulators), and the two lane halves - which hold different candidates of the same query - merge
// once after the last tile.  The next slice is fetched into registers while the current one is multiplied.
#include "internal.h"

#define PAIR_T 128        // queries per workgroup, candidates per tile
#define PAIR_K 32         // K slice
#define PAIR_LD 33        // LDS row stride (floats)
#define PAIR_BLOCK 256
#define PAIR_KMAX 8
#define PAIR_TARGET_BLOCKS 1024   // workgroups aimed at when the library chooses col_chunks (256 CUs, 4 per CU)

enum { PAIR_GRAM = 0, PAIR_KTH = 1, PAIR_MEMBER = 2, PAIR_POLY = 3 };

struct PairArgs {
  const float* a; const float* b;     // queries (na, d), candidates (nb, d)
  int na, nb, d;
  int tiles_per_chunk, vec4;
  const float* an; const float* bn;   // squared row norms (KTH, MEMBER)
  const float* r2;                    // MEMBER: squared radius of every candidate
  int k, excl;
  float gamma, coef0;
  float* gram;                        // GRAM: (na, nb)
  void* part;                         // per-chunk partial results: KTH [chunk][na][k] float, MEMBER [chunk][na] int32,
                                      // POLY [chunk][na] double
};

// the chunking both the entries and tdx_pair_scratch_bytes use: whole tiles per chunk, no empty chunk
static inline int pair_chunks(int na, int nb, int col_chunks, int* tiles_per_chunk) {
  const int tiles = cdiv(nb, PAIR_T), rowblocks = cdiv(na, PAIR_T);
  int c = col_chunks > 0 ? col_chunks : cdiv(PAIR_TARGET_BLOCKS, rowblocks);
  if (c > tiles) c = tiles;
  if (c > 65535) c = 65535;   // gridDim.y
  const int per = cdiv(tiles, c);
  if (tiles_per_chunk) *tiles_per_chunk = per;
  return cdiv(tiles, per);
}

static inline size_t pair_norm_bytes(int na, int nb) { return (((size_t)na + (size_t)nb) * sizeof(float) + 15) & ~(size_t)15; }

extern "C" size_t tdx_pair_scratch_bytes(int na, int nb, int k, int col_chunks) {
  if (na <= 0 || nb <= 0 || col_chunks < 0 || k > PAIR_KMAX) return 0;
  const int chunks = pair_chunks(na, nb, col_chunks, nullptr);
  size_t per_row = (size_t)(k > 0 ? k : 1) * sizeof(float);
  if (per_row < sizeof(double)) per_row = sizeof(double);
  return pair_norm_bytes(na, nb) + (size_t)chunks * (size_t)na * per_row;
}

// n_i = fma(x_{d-1}, x_{d-1}, ... fma(x_0, x_0, 0)): the chain the MFMA runs for g_ii, so a row's norm equals its
// inner product with an identical row bit for bit
__global__ void __launch_bounds__(256) pair_norm_kernel(const float* __restrict__ x, int n, int d, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* row = x + (int64_t)i * d;
  float s = 0.0f;
  for (int k = 0; k < d; ++k) s = __fmaf_rn(row[k], row[k], s);
  out[i] = s;
}

// insert v into the ascending list of the PAIR_KMAX smallest values seen (a multiset: ties are kept)
__device__ __forceinline__ void pair_insert(float (&l)[PAIR_KMAX], float v) {
#pragma unroll
  for (int i = 0; i < PAIR_KMAX; ++i) {
    const float lo = fminf(l[i], v);
    v = fmaxf(l[i], v);
    l[i] = lo;
  }
}

// d2 = max(0, (|a|^2 + |b|^2) - 2 g), each operation rounded separately (2 g is exact)
__device__ __forceinline__ float pair_dist2(float an, float bn, float g) {
  return fmaxf(0.0f, __fsub_rn(__fadd_rn(an, bn), __fmul_rn(2.0f, g)));
}

// one K slice of a 128-row tile, global -> registers (zero outside the matrix)
__device__ __forceinline__ void pair_fetch(const float* __restrict__ x, int n, int d, int row0, int k0, int vec4, int tid,
                                           float (&r)[16]) {
  if (vec4) {   // d % 4 == 0 and a 16-byte aligned base: k < d implies k + 3 < d
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + PAIR_BLOCK * i, row = row0 + (idx >> 3), k = k0 + (idx & 7) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < n && k < d) v = *(const float4*)(x + (int64_t)row * d + k);
      r[4 * i + 0] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int idx = tid + PAIR_BLOCK * i, row = row0 + (idx >> 5), k = k0 + (idx & 31);
      r[i] = (row < n && k < d) ? x[(int64_t)row * d + k] : 0.0f;
    }
  }
}

__device__ __forceinline__ void pair_stage(float* __restrict__ s, int vec4, int tid, const float (&r)[16]) {
  if (vec4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + PAIR_BLOCK * i;
      float* p = s + (idx >> 3) * PAIR_LD + (idx & 7) * 4;
      p[0] = r[4 * i + 0]; p[1] = r[4 * i + 1]; p[2] = r[4 * i + 2]; p[3] = r[4 * i + 3];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int idx = tid + PAIR_BLOCK * i;
      s[(idx >> 5) * PAIR_LD + (idx & 31)] = r[i];
    }
  }
}

template <int MODE>
__global__ void __launch_bounds__(PAIR_BLOCK, 2) pair_kernel(PairArgs p) {   // two workgroups per CU: 256 registers
  __shared__ float sa[PAIR_T * PAIR_LD], sb[PAIR_T * PAIR_LD];
  __shared__ float sbn[PAIR_T], sr2[PAIR_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  const int a0 = blockIdx.x * PAIR_T, chunk = blockIdx.y;
  const int tiles = (p.nb + PAIR_T - 1) / PAIR_T;
  const int t0 = chunk * p.tiles_per_chunk, t1 = min(t0 + p.tiles_per_chunk, tiles);
  const int slices = (p.d + PAIR_K - 1) / PAIR_K;
  const int qi = a0 + wave * 32 + col;   // this lane's query
  const bool q_ok = qi < p.na;
  float an = 0.0f;
  if ((MODE == PAIR_KTH || MODE == PAIR_MEMBER) && q_ok) an = p.an[qi];

  float best[PAIR_KMAX];
#pragma unroll
  for (int i = 0; i < PAIR_KMAX; ++i) best[i] = INFINITY;
  int flag = 0;
  double sum = 0.0;
  const double gam = (double)p.gamma, c0 = (double)p.coef0;

  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

  float ra[16], rb[16];
  const int steps = (t1 - t0) * slices;
  if (steps > 0) {
    pair_fetch(p.a, p.na, p.d, a0, 0, p.vec4, tid, ra);
    pair_fetch(p.b, p.nb, p.d, t0 * PAIR_T, 0, p.vec4, tid, rb);
  }
  int tile = t0, slice = 0;
  for (int s = 0; s < steps; ++s) {
    const int b0 = tile * PAIR_T, k0 = slice * PAIR_K;
    __syncthreads();   // the slice before (and its tile's epilogue) is done with the LDS
    pair_stage(sa, p.vec4, tid, ra);
    pair_stage(sb, p.vec4, tid, rb);
    if (slice == 0 && tid < PAIR_T) {
      const int j = b0 + tid;
      if (MODE == PAIR_KTH || MODE == PAIR_MEMBER) sbn[tid] = j < p.nb ? p.bn[j] : 0.0f;
      if (MODE == PAIR_MEMBER) sr2[tid] = j < p.nb ? p.r2[j] : 0.0f;
    }
    __syncthreads();
    int ntile = tile, nslice = slice + 1;
    if (nslice == slices) { nslice = 0; ++ntile; }
    if (s + 1 < steps) {
      pair_fetch(p.a, p.na, p.d, a0, nslice * PAIR_K, p.vec4, tid, ra);
      pair_fetch(p.b, p.nb, p.d, ntile * PAIR_T, nslice * PAIR_K, p.vec4, tid, rb);
    }
    const int nk = (min(PAIR_K, p.d - k0) + 1) >> 1;   // an odd tail multiplies one staged zero
    const float* qa = sa + (wave * 32 + col) * PAIR_LD + half;
    const float* qb = sb + col * PAIR_LD + half;
    for (int kk = 0; kk < nk; ++kk) {
      const float q = qa[2 * kk];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(qb[t * 32 * PAIR_LD + 2 * kk], q, acc[t], 0, 0, 0);
    }
    if (slice == slices - 1) {
      // accumulator (tile t, register r) of this lane: candidate b0 + 32 t + (r & 3) + 8 (r >> 2) + 4 half
      const bool edge = b0 + PAIR_T > p.nb || (p.excl && b0 < a0 + PAIR_T && a0 < b0 + PAIR_T);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int jl = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half, j = b0 + jl;
          const float g = acc[t][r];
          const bool ok = !edge || (j < p.nb && !(p.excl && j == qi));
          if (MODE == PAIR_GRAM) {
            if (q_ok && j < p.nb) p.gram[(int64_t)qi * p.nb + j] = g;
          } else if (MODE == PAIR_KTH) {
            const float d2 = pair_dist2(an, sbn[jl], g);
            if (ok && d2 < best[PAIR_KMAX - 1]) pair_insert(best, d2);
          } else if (MODE == PAIR_MEMBER) {
            const float d2 = pair_dist2(an, sbn[jl], g);
            if (ok && d2 <= sr2[jl]) flag = 1;
          } else {
            if (ok) {
              const double v = fma(gam, (double)g, c0);
              sum += (v * v) * v;
            }
          }
          acc[t][r] = 0.0f;
        }
      }
    }
    tile = ntile;
    slice = nslice;
  }

  // the two lane halves of a query merge; the lower half writes the chunk's partial result
  if (MODE == PAIR_KTH) {
    float other[PAIR_KMAX];
#pragma unroll
    for (int i = 0; i < PAIR_KMAX; ++i) other[i] = __shfl_xor(best[i], 32, 64);
#pragma unroll
    for (int i = 0; i < PAIR_KMAX; ++i) pair_insert(best, other[i]);
    if (half == 0 && q_ok) {
      float* out = (float*)p.part + ((int64_t)chunk * p.na + qi) * p.k;
#pragma unroll
      for (int i = 0; i < PAIR_KMAX; ++i)
        if (i < p.k) out[i] = best[i];
    }
  } else if (MODE == PAIR_MEMBER) {
    flag |= __shfl_xor(flag, 32, 64);
    if (half == 0 && q_ok) ((int32_t*)p.part)[(int64_t)chunk * p.na + qi] = flag;
  } else if (MODE == PAIR_POLY) {
    const double hi = __shfl_xor(sum, 32, 64);
    if (half == 0 && q_ok) ((double*)p.part)[(int64_t)chunk * p.na + qi] = sum + hi;
  }
}

// the second launch: one thread per query folds the chunks in ascending order
template <int MODE>
__global__ void __launch_bounds__(256) pair_merge_kernel(const void* __restrict__ part, int na, int chunks, int k,
                                                         void* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= na) return;
  if (MODE == PAIR_KTH) {
    float best[PAIR_KMAX];
#pragma unroll
    for (int e = 0; e < PAIR_KMAX; ++e) best[e] = INFINITY;
    for (int c = 0; c < chunks; ++c) {
      const float* src = (const float*)part + ((int64_t)c * na + i) * k;
      for (int e = 0; e < k; ++e) pair_insert(best, src[e]);
    }
    float res = best[0];
#pragma unroll
    for (int e = 1; e < PAIR_KMAX; ++e)
      if (e == k - 1) res = best[e];
    ((float*)out)[i] = res;
  } else if (MODE == PAIR_MEMBER) {
    int flag = 0;
    for (int c = 0; c < chunks; ++c) flag |= ((const int32_t*)part)[(int64_t)c * na + i];
    ((int32_t*)out)[i] = flag;
  } else {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += ((const double*)part)[(int64_t)c * na + i];
    ((double*)out)[i] = s;
  }
}

static inline int pair_vec4(const float* a, const float* b, int d) {
  return d % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

template <int MODE>
static int pair_run(PairArgs p, int col_chunks, void* out, void* scratch, size_t scratch_bytes, bool norms, hipStream_t st) {
  if (!scratch || ((uintptr_t)scratch & 15)) return TDX_E_BADARG;
  if (scratch_bytes < tdx_pair_scratch_bytes(p.na, p.nb, p.k, col_chunks)) return TDX_E_WORKSPACE;
  const int chunks = pair_chunks(p.na, p.nb, col_chunks, &p.tiles_per_chunk);
  float* an = (float*)scratch;
  float* bn = an + p.na;
  p.part = (char*)scratch + pair_norm_bytes(p.na, p.nb);
  p.vec4 = pair_vec4(p.a, p.b, p.d);
  if (norms) {
    pair_norm_kernel<<<cdiv(p.na, 256), 256, 0, st>>>(p.a, p.na, p.d, an);
    TDX_CHECK_LAUNCH();
    pair_norm_kernel<<<cdiv(p.nb, 256), 256, 0, st>>>(p.b, p.nb, p.d, bn);
    TDX_CHECK_LAUNCH();
    p.an = an;
    p.bn = bn;
  }
  pair_kernel<MODE><<<dim3(cdiv(p.na, PAIR_T), chunks), PAIR_BLOCK, 0, st>>>(p);
  TDX_CHECK_LAUNCH();
  pair_merge_kernel<MODE><<<cdiv(p.na, 256), 256, 0, st>>>(p.part, p.na, chunks, p.k, out);
  TDX_CHECK_LAUNCH();
  return 0;
}

static inline bool pair_shape_ok(const float* a, const float* b, int na, int nb, int d, int col_chunks) {
  return a && b && na > 0 && nb > 0 && d > 0 && col_chunks >= 0;
}

extern "C" int tdx_pair_gram(const float* a, const float* b, int na, int nb, int d, float* out, tdx_stream_t stream) {
  if (!pair_shape_ok(a, b, na, nb, d, 0) || !out) return TDX_E_BADARG;
  PairArgs p{};
  p.a = a; p.b = b; p.na = na; p.nb = nb; p.d = d;
  p.gram = out;
  p.vec4 = pair_vec4(a, b, d);
  const int chunks = pair_chunks(na, nb, 0, &p.tiles_per_chunk);
  pair_kernel<PAIR_GRAM><<<dim3(cdiv(na, PAIR_T), chunks), PAIR_BLOCK, 0, to_stream(stream)>>>(p);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_pair_kth_dist2(const float* a, const float* b, int na, int nb, int d, int k, int exclude_diag,
                                  int col_chunks, float* out, void* scratch, size_t scratch_bytes, tdx_stream_t stream) {
  if (!pair_shape_ok(a, b, na, nb, d, col_chunks) || !out || k < 1 || k > PAIR_KMAX) return TDX_E_BADARG;
  if (nb < k + (exclude_diag ? 1 : 0)) return TDX_E_BADARG;
  PairArgs p{};
  p.a = a; p.b = b; p.na = na; p.nb = nb; p.d = d; p.k = k; p.excl = exclude_diag != 0;
  return pair_run<PAIR_KTH>(p, col_chunks, out, scratch, scratch_bytes, true, to_stream(stream));
}

extern "C" int tdx_pair_member(const float* a, const float* b, const float* r2, int na, int nb, int d, int col_chunks,
                               int32_t* flag, void* scratch, size_t scratch_bytes, tdx_stream_t stream) {
  if (!pair_shape_ok(a, b, na, nb, d, col_chunks) || !r2 || !flag) return TDX_E_BADARG;
  PairArgs p{};
  p.a = a; p.b = b; p.na = na; p.nb = nb; p.d = d; p.r2 = r2; p.k = 1;
  return pair_run<PAIR_MEMBER>(p, col_chunks, flag, scratch, scratch_bytes, true, to_stream(stream));
}

extern "C" int tdx_pair_poly_rowsum(const float* a, const float* b, int na, int nb, int d, float gamma, float coef0,
                                    int exclude_diag, int col_chunks, double* out, void* scratch, size_t scratch_bytes,
                                    tdx_stream_t stream) {
  if (!pair_shape_ok(a, b, na, nb, d, col_chunks) || !out || !std::isfinite(gamma) || !std::isfinite(coef0))
    return TDX_E_BADARG;
  PairArgs p{};
  p.a = a; p.b = b; p.na = na; p.nb = nb; p.d = d; p.k = 1; p.excl = exclude_diag != 0;
  p.gamma = gamma; p.coef0 = coef0;
  return pair_run<PAIR_POLY>(p, col_chunks, out, scratch, scratch_bytes, false, to_stream(stream));
}
