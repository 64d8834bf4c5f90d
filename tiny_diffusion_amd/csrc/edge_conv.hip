// The two boundary convolutions of the UNet - initial_conv (model input, 1 | 4 channels, NCHW ->
// 64 channels-last) and final_conv (64 channels-last -> 1 | 4 channels NCHW) - and their backward
// passes (diffusion.py:28, 98, 116, 160; conditional_diffusion_laion.py:244, 296).  One side of each
// is THIN (K = 9 or 36 taps x channels), the other is a 256-byte-per-pixel activation: all five are
// HBM-bound on the fat tensor (67 MB at B = 256, 32x32) and none is a job for the implicit-GEMM
// kernel (padding 4 channels to 32 would multiply its work by eight).  They are small GEMMs all the
// same, so the three kernels below run them on the fp32 MFMA (exact fp32 products, fp32 accumulate:
// the same arithmetic as the CUDA-core loops they replace, up to summation order) with the thin
// operand gathered straight from the (L2-resident) NCHW tensor:
//   thin_to_fat_conv   out[p][c] = b[c] + sum_k T[p][k] W[k][c]      initial_conv forward; final_conv dgrad (taps mirrored)
//   fat_to_thin_conv   out[n][o][p] = b[o] + sum_{tap,c} F[p+tap][c] W[o][c][tap]      final_conv forward (VALU, weights in LDS)
//   thin_fat_wgrad     dW[k][c] = sum_p T[p][k] F[p][c]              both weight gradients (+ bias gradients)
// T[p][k = (ch, tap)] = thin[n][ch][pixel p shifted by the tap] (0 outside the image).
// Before (B = 256, LAION 4x32x32, us): 107 / 142 / 54 / 408 / 382 of a 10.1 ms step, mostly exposed at its head and tail.
#include "internal.h"
#include "io16.h"

#define IC_CO 64
#define SMALLP_W 2368  // floats per row of the weight-gradient partial buffer (4*64*9 + 64)

namespace {

// k -> (thin channel, dy, dx) for k < K, by multiplications (k < 64)
__device__ __forceinline__ void tap_of(int k, int& c, int& dy, int& dx) {
  c = (k * 57) >> 9;          // k / 9
  const int tap = k - 9 * c;
  const int ty = (tap * 11) >> 5;  // tap / 3
  dy = ty - 1;
  dx = tap - 3 * ty - 1;
}

// ------------------------------------------------------------------ thin -> fat
// 128 pixels x 64 channels per workgroup pass; wave = 32 pixels x 64 channels = two 32x32 MFMA
// tiles, K = CT*9 in steps of 2.  FLIP = false: w is [cor][CT][9] (initial_conv.weight), channels
// >= cor are written as zeros; FLIP = true: w is [CT][64][9] (final_conv.weight), the input
// gradient: g_in[p][c] = sum_{o,tap} g_out[n][o][p - tap] W[o][c][tap].
template <int CT, bool FLIP, typename TF>   // TF: element type of the fat (channels-last, 64-channel) tensor, io16.h
__global__ void __launch_bounds__(256)
thin_to_fat_conv_kernel(const float* __restrict__ thin, const float* __restrict__ w,
                        const float* __restrict__ bias, TF* __restrict__ out, int B, int H, int W,
                        int cor) {
  constexpr int K = CT * 9, KS = (K + 1) / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int HW = H * W;
  const int64_t M = (int64_t)B * HW;

  float bfr[2][KS], bv[2];
  int koff[KS], kdy[KS], kdx[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = 2 * s + half;
    int c, dy, dx;
    tap_of(k, c, dy, dx);
    if (FLIP) { dy = -dy; dx = -dx; }
    kdy[s] = k < K ? dy : 2 * H;  // k >= K (odd K padding): never valid
    kdx[s] = dx;
    koff[s] = c * HW + dy * W + dx;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const int col = cb * 32 + l31;
      float v = 0.f;
      if (k < K) {
        if (!FLIP) {
          if (col < cor) v = w[col * K + k];
        } else {
          const int tap = k - 9 * c;
          v = w[(c * IC_CO + col) * 9 + tap];
        }
      }
      bfr[cb][s] = v;
    }
  }
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) bv[cb] = (!FLIP && bias && cb * 32 + l31 < cor) ? bias[cb * 32 + l31] : 0.f;

  const int64_t tiles = (M + 127) / 128;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t pw0 = tile * 128 + wave * 32;
    const int64_t p = pw0 + l31;
    const bool pv = p < M;
    const int n = pv ? (int)(p / HW) : 0;
    const int r = pv ? (int)(p - (int64_t)n * HW) : 0;
    const int oh = r / W, ow = r - oh * W;
    const float* base = thin + (int64_t)n * CT * HW + r;
    float a[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const bool ok = pv && (unsigned)(oh + kdy[s]) < (unsigned)H && (unsigned)(ow + kdx[s]) < (unsigned)W;
      a[s] = ok ? base[koff[s]] : 0.f;
    }
    f32x16 acc[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[cb][i] = bv[cb];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bfr[0][s], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bfr[1][s], acc[1], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t pp = pw0 + (i & 3) + 8 * (i >> 2) + 4 * half;
      if (pp < M) {
        st1(out + pp * IC_CO + l31, acc[0][i]);
        st1(out + pp * IC_CO + 32 + l31, acc[1][i]);
      }
    }
  }
}

// ------------------------------------------------------------------ fat -> thin
// out[n][o][p] = b[o] + sum_tap sum_c in[p+tap][c] * W[o][c][tap]; 16 lanes per pixel, a float4 of
// channels per lane, weights in LDS, shuffle-reduced over the 16 lanes.  (Weights in registers - CO*9
// float4 per lane - was tried: 210 VGPRs, two waves per SIMD, 152 us instead of 54 at CO = 4.  What is
// left on the table is the LDS weight traffic, one b128 read per four FMAs; the GEMM form
// Z[q][(o,tap)] = in[q][:] . W[o][:][tap] followed by a 9-neighbour gather would read `in` once.)
// DGRAD = true: the input gradient of initial_conv with the same loop.  g_x[n][c][p] =
// sum_{o,tap} g(x0)[p - tap][o] W[o][c][tap] = sum_{tap'} sum_o g(x0)[p + tap'][o] W[o][c][8 - tap'], i.e. this
// kernel on the gradient of x0 with the weight image ws[c][tap'][o] = initial_conv.weight[o][c][8 - tap'] (w is
// [cor][CO][9]; stored channels o >= cor are padding: zero weights) and no bias.
// PS = true (sampling): the reverse-process update ps (PStep, internal.h) in the epilogue - the lane that holds the
// network's output of an element also reads x, draws or loads z / the history / known and mask, and writes x' in place
// (x is not an input of this kernel: the network read it in initial_conv) with pstep_elem, the arithmetic and the
// Philox indexing of pstep_kernel bit for bit; the step's last launch disappears.  The output is still written to
// `out`.  FORM / MK: the update's form and whether it blends (template parameters: an instantiation carries no trace
// of the others).  hist, known, mask and the Philox element are indexed by the element's place in the whole batch
// (idx + ps.elem0); x and z start at this launch's first element.
// GD = true (with PS; classifier-free guidance): B = 2n samples whose first half ran under the caller's condition and
// whose second half under the null condition, both from the same x.  The pixel loop runs over the first half's n H W
// pixels; a lane group accumulates the convolution of its pixel AND of the twin pixel n H W further on against the same
// LDS weight reads, writes both outputs to `out`, combines them (cfg_eps) and writes the one update to both halves of
// x (one launch: elem0 == 0).  Noise as in the unguided chain of n samples.
template <int CO, bool DGRAD, bool PS, typename TF, bool GD = false, int FORM = TDX_STEP_EPS, bool MK = false>
__global__ void __launch_bounds__(256)
fat_to_thin_conv_kernel(const TF* __restrict__ in, const float* __restrict__ w,
                        const float* __restrict__ bias, float* __restrict__ out, int B, int H, int W, int cor,
                        PStep ps) {
  __shared__ __attribute__((aligned(16))) float ws[CO][9][IC_CO];
  if (DGRAD) {
    for (int i = threadIdx.x; i < CO * 9 * IC_CO; i += 256) {
      const int c = i / (9 * IC_CO), r = i % (9 * IC_CO), tap = r / IC_CO, o = r % IC_CO;
      ws[c][tap][o] = o < cor ? w[(o * CO + c) * 9 + (8 - tap)] : 0.f;
    }
  } else {
    for (int i = threadIdx.x; i < CO * 9 * IC_CO; i += 256) {  // w is [co][ci][tap]
      const int co = i / (9 * IC_CO), r = i % (9 * IC_CO);
      ws[co][r % 9][r / 9] = w[i];
    }
  }
  __syncthreads();
  const int ci = (threadIdx.x & 15) * 4, pl = threadIdx.x >> 4;
  const int HW = H * W;
  const int64_t M = (int64_t)(GD ? B / 2 : B) * HW;   // GD: the first half's pixels, the twin of pixel p is p + M
  const int64_t Mpad = (M + 15) / 16 * 16;
  float bv[CO];
#pragma unroll
  for (int co = 0; co < CO; ++co) bv[co] = DGRAD ? 0.f : bias[co];
  int ps_t = 0;
  uint64_t ps_nt = 0;
  PRow ps_r = {};
  if (PS) {
    ps_t = *ps.t_idx;
    ps_nt = ps.tau ? (uint64_t)ps.tau[ps_t] : (uint64_t)ps_t;
    ps_r = pstep_row<FORM>(ps.coef, ps_t);
    // table-mode sampling: the step counter is advanced by the last kernel of the step (see pstep_kernel)
    if (ps.counter_dec && blockIdx.x == 0 && threadIdx.x == 0) *ps.counter_dec = (int64_t)ps_t - 1;
  }
  for (int64_t p = (int64_t)blockIdx.x * 16 + pl; p < Mpad; p += (int64_t)gridDim.x * 16) {
    float s[CO], s2[GD ? CO : 1];
#pragma unroll
    for (int co = 0; co < CO; ++co) s[co] = 0.f;
    if (GD) {
#pragma unroll
      for (int co = 0; co < CO; ++co) s2[co] = 0.f;
    }
    int n = 0, r = 0;
    if (p < M) {
      n = (int)(p / HW);
      r = (int)(p - (int64_t)n * HW);
      const int oh = r / W, ow = r - oh * W;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ih = oh + tap / 3 - 1, iw = ow + tap % 3 - 1;
        if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) {
          const float4 v = ld4(in + (p + (tap / 3 - 1) * W + (tap % 3 - 1)) * IC_CO + ci);
          float4 v2 = v;
          if (GD) v2 = ld4(in + (p + M + (tap / 3 - 1) * W + (tap % 3 - 1)) * IC_CO + ci);
#pragma unroll
          for (int co = 0; co < CO; ++co) {
            const float4 wv = *reinterpret_cast<const float4*>(&ws[co][tap][ci]);
            s[co] = fmaf(v.x, wv.x, s[co]);
            s[co] = fmaf(v.y, wv.y, s[co]);
            s[co] = fmaf(v.z, wv.z, s[co]);
            s[co] = fmaf(v.w, wv.w, s[co]);
            if (GD) {
              s2[co] = fmaf(v2.x, wv.x, s2[co]);
              s2[co] = fmaf(v2.y, wv.y, s2[co]);
              s2[co] = fmaf(v2.z, wv.z, s2[co]);
              s2[co] = fmaf(v2.w, wv.w, s2[co]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int co = 0; co < CO; ++co) {
      s[co] += __shfl_xor(s[co], 8, 64);
      s[co] += __shfl_xor(s[co], 4, 64);
      s[co] += __shfl_xor(s[co], 2, 64);
      s[co] += __shfl_xor(s[co], 1, 64);
    }
    if (GD) {
#pragma unroll
      for (int co = 0; co < CO; ++co) {
        s2[co] += __shfl_xor(s2[co], 8, 64);
        s2[co] += __shfl_xor(s2[co], 4, 64);
        s2[co] += __shfl_xor(s2[co], 2, 64);
        s2[co] += __shfl_xor(s2[co], 1, 64);
      }
    }
    if ((threadIdx.x & 15) == 0 && p < M) {
#pragma unroll
      for (int co = 0; co < CO; ++co) {
        const int64_t idx = ((int64_t)n * CO + co) * HW + r;
        const float e = s[co] + bv[co];
        out[idx] = e;
        if (PS) {
          const int64_t gidx = idx + ps.elem0;
          float eg = e, zh = 0.f, kn = 0.f, mv = 0.f, x0 = 0.f;
          if (GD) {
            const float eu = s2[co] + bv[co];
            out[idx + ps.half] = eu;
            eg = cfg_eps(e, eu, ps.w);
          }
          if (FORM == TDX_STEP_MS) {   // deterministic: the history in the place of the noise
            if (ps_r.e != 0.0f) zh = ps.hist[gidx];
          } else if (ps_t > 0) {   // diffusion.py:267-270: no noise on the last step
            if (ps.philox) {   // element gidx = component gidx % 4 of block gidx / 4 (pstep_kernel)
              const float4 z4 = philox_normal4((uint64_t)(gidx >> 2), ps_nt, ps.seed);
              const int k = (int)(gidx & 3);
              zh = k == 0 ? z4.x : k == 1 ? z4.y : k == 2 ? z4.z : z4.w;
            } else if (ps.z) {
              zh = ps.z[idx];
            }
          }
          if (MK) { kn = ps.known[gidx]; mv = ps.mask[gidx]; }
          const float xn = pstep_elem<FORM, MK>(ps.x[idx], eg, zh, kn, mv, ps_r, ps.lo, ps.hi, &x0);
          ps.x[idx] = xn;
          if (GD) ps.x[idx + ps.half] = xn;
          if (FORM == TDX_STEP_MS) ps.hist[gidx] = x0;
        }
      }
    }
  }
}

// ------------------------------------------------------------------ weight gradients
// MFMA rows = the 64 fat channels (two tiles), columns = k (one tile for K <= 32, two otherwise),
// reduction over pixels two at a time.  A workgroup takes `pix` consecutive pixels, a wave a quarter
// of them; the four waves' accumulators are summed through LDS in wave order (deterministic) and the
// workgroup writes ONE row of the partial buffer, in the parameter's own [o][c][tap] order, that
// reduce_partials sums over workgroups in a fixed order.
//   FLIP = false  initial_conv: thin = x, fat = g(x0); dW[o][c][tap] at o*K + (c*9+tap), o < cor;
//                 an extra all-ones column gives db[o] = sum_p g[p][o] at cor*K + o
//   FLIP = true   final_conv: thin = g_out, fat = the conv's input; dW[o][c][tap] at (o*64 + c)*9 + tap;
//                 db[o] = sum_p g_out[n][o][p] = the column sums of the centre taps, at CT*576 + o
template <int CT, bool FLIP, typename TF>
__global__ void __launch_bounds__(256)
thin_fat_wgrad_kernel(const float* __restrict__ thin, const TF* __restrict__ fat,
                      float* __restrict__ partial, int B, int H, int W, int pix, int cor) {
  constexpr int K = CT * 9, KC = FLIP ? K : K + 1, CB = KC <= 32 ? 1 : 2;
  __shared__ float red[IC_CO][CB * 32 + 1];
  __shared__ float dbl[CB * 32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int HW = H * W;
  const int64_t M = (int64_t)B * HW;
  const int per_wave = pix / 4;
  const int64_t p0 = (int64_t)blockIdx.x * pix + (int64_t)wave * per_wave;
  const int64_t p1 = min(p0 + per_wave, M);

  int kind[CB], koff[CB], kdy[CB], kdx[CB];  // kind: 0 tap, 1 ones, 2 padding, 3 centre tap (FLIP: feeds db)
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    const int k = cb * 32 + l31;
    int c, dy, dx;
    tap_of(k < K ? k : 0, c, dy, dx);
    if (FLIP) { dy = -dy; dx = -dx; }
    kind[cb] = k < K ? ((FLIP && dy == 0 && dx == 0) ? 3 : 0) : (k == K && !FLIP) ? 1 : 2;
    kdy[cb] = dy; kdx[cb] = dx;
    koff[cb] = c * HW + dy * W + dx;
  }
  f32x16 acc[2][CB];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[rb][cb][i] = 0.f;
  float dbacc[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) dbacc[cb] = 0.f;

  // this lane's pixel of the current pair: q = p + half, walked two at a time (W >= 4)
  int64_t q = p0 + half;
  int n = 0, oh = 0, ow = 0;
  if (q < M) {
    n = (int)(q / HW);
    const int r = (int)(q - (int64_t)n * HW);
    oh = r / W;
    ow = r - oh * W;
  }
  // Eight pixel pairs per trip, every load of the trip issued before its first MFMA (branch-free: a refused tap reads
  // the tensor's first element and is zeroed afterwards).  The loop is bound by the round trip of its 4-byte loads, not
  // by its MFMAs: pair by pair (what hipcc makes of the plain loop, the agent-scope loads pinning the order) the
  // initial-convolution launch took 154 us on the tail of the fp32 step for 51 MB of input.
  constexpr int U = 8;
  for (int64_t p = p0; p < p1; p += 2 * U) {
    float a0[U], a1[U], bq[U][CB];
    bool okq[U][CB], qvu[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool qv = q < p1;
      qvu[u] = qv;
      const TF* frow = fat + (qv ? q : p0) * IC_CO + l31;
      a0[u] = ld1(frow);
      a1[u] = ld1(frow + 32);
      const float* tb = thin + (int64_t)n * CT * HW + oh * W + ow;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const bool ok = qv & (kind[cb] == 0 || kind[cb] == 3) & ((unsigned)(oh + kdy[cb]) < (unsigned)H) &
                        ((unsigned)(ow + kdx[cb]) < (unsigned)W);
        okq[u][cb] = ok;
        const float* src = ok ? tb + koff[cb] : thin;
        // initial_conv (FLIP = false): `thin` is the workspace COPY of the model input that the forward made
        // with hipMemcpyAsync, and this kernel may run on a helper stream - the shape of the one hand-off
        // that was seen stale from one XCD: read it at agent scope (L2-served `sc1` loads,
        // 0.8 MB in all: free).  final_conv's thin operand is a kernel's output on the same stream: plain.
        bq[u][cb] = FLIP ? *src : __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      q += 2;
      ow += 2;
      if (ow >= W) { ow -= W; if (++oh == H) { oh = 0; ++n; } }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float x0 = qvu[u] ? a0[u] : 0.f, x1 = qvu[u] ? a1[u] : 0.f;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        float v = okq[u][cb] ? bq[u][cb] : 0.f;
        if (kind[cb] == 1) v = qvu[u] ? 1.f : 0.f;
        if (FLIP && kind[cb] == 3) dbacc[cb] += v;
        acc[0][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0, v, acc[0][cb], 0, 0, 0);
        acc[1][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1, v, acc[1][cb], 0, 0, 0);
      }
    }
  }

  // waves add their tiles in wave order
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int row = rb * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
            float* d = &red[row][cb * 32 + l31];
            *d = wv == 0 ? acc[rb][cb][i] : *d + acc[rb][cb][i];
          }
      if (FLIP) {
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          const float v = dbacc[cb] + __shfl_xor(dbacc[cb], 32, 64);
          if (half == 0) dbl[cb * 32 + l31] = wv == 0 ? v : dbl[cb * 32 + l31] + v;
        }
      }
    }
    __syncthreads();
  }
  float* prow = partial + (size_t)blockIdx.x * SMALLP_W;
  for (int i = threadIdx.x; i < IC_CO * K; i += 256) {
    const int row = i / K, k = i - row * K;
    if (!FLIP) {
      if (row < cor) prow[row * K + k] = red[row][k];
    } else {
      const int o = k / 9, tap = k - 9 * o;
      prow[(o * IC_CO + row) * 9 + tap] = red[row][k];
    }
  }
  if (!FLIP) {
    if (threadIdx.x < cor) prow[cor * K + threadIdx.x] = red[threadIdx.x][K];
  } else if (threadIdx.x < CT) {
    prow[CT * 576 + threadIdx.x] = dbl[threadIdx.x * 9 + 4];
  }
}

// out[i] = sum_b partial[b*stride + i], i < count.  Fixed summation order (deterministic),
// double accumulation; block = 32 columns x 8 interleaved row slices.  Columns >= split go to out2
// (the bias gradient behind the weight gradient in one partial row).
__global__ void __launch_bounds__(256)
reduce_partials_kernel(const float* __restrict__ partial, float* __restrict__ out, float* __restrict__ out2,
                       int split, int nblk, int stride, int count) {
  __shared__ double red[8][32];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + cl;
  double s = 0.0;
  if (i < count) {
#pragma unroll 4
    for (int b = sl; b < nblk; b += 8) s += (double)partial[(size_t)b * stride + i];
  }
  red[sl][cl] = s;
  __syncthreads();
  if (sl == 0 && i < count) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += red[k][cl];
    if (i < split) out[i] = (float)t;
    else out2[i - split] = (float)t;
  }
}

// First level of a long reduction, IN PLACE: block (c, g) sums the rows congruent to g modulo
// gridDim.y over its 32 columns and stores the sum into row g.  No block reads what another one
// writes (rows of another residue class, or other columns), and a block has read all of its rows
// before it writes (barrier), so nblk rows become gridDim.y rows with no second buffer.
__global__ void __launch_bounds__(256)
fold_partials_kernel(float* __restrict__ partial, int nblk, int stride, int count) {
  __shared__ double red[8][32];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + cl, g = blockIdx.y, G = gridDim.y;
  double s = 0.0;
  if (i < count) {
#pragma unroll 4
    for (int b = g + sl * G; b < nblk; b += 8 * G) s += (double)partial[(size_t)b * stride + i];
  }
  red[sl][cl] = s;
  __syncthreads();
  if (sl == 0 && i < count) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += red[k][cl];
    partial[(size_t)g * stride + i] = (float)t;
  }
}

constexpr int FOLD_ROWS = 32;

// out[0..split) and out2[0..count-split) from the columns of `partial` (which is consumed)
int reduce_partials2(float* partial, float* out, float* out2, int split, int nblk, int stride, int count,
                     hipStream_t st) {
  if (nblk > 4 * FOLD_ROWS) {
    fold_partials_kernel<<<dim3(cdiv(count, 32), FOLD_ROWS), 256, 0, st>>>(partial, nblk, stride, count);
    TDX_CHECK_LAUNCH();
    nblk = FOLD_ROWS;
  }
  reduce_partials_kernel<<<cdiv(count, 32), 256, 0, st>>>(partial, out, out2, split, nblk, stride, count);
  TDX_CHECK_LAUNCH();
  return 0;
}

constexpr int WGRAD_PIX = 512;  // pixels per workgroup of thin_fat_wgrad_kernel (a multiple of 8)

int conv_grid(int64_t M) {
  const int64_t tiles = (M + 127) / 128;
  return (int)std::min<int64_t>(tiles, 4096);
}

}  // namespace

int tdx_reduce_partials(const float* partial, float* out, int nblk, int stride, int count,
                        hipStream_t st) {
  reduce_partials_kernel<<<cdiv(count, 32), 256, 0, st>>>(partial, out, nullptr, count, nblk, stride, count);
  TDX_CHECK_LAUNCH();
  return 0;
}

// io16 (all launchers below): the fat, channels-last tensor holds bf16 (io16.h); thin tensors, weights and gradients
// of weights are fp32 always
int tdx_initial_conv_fwd(const float* x, const float* w, const float* bias, void* out, int B, int H,
                         int W, int cin, int cout_real, hipStream_t st, int io16) {
  const int grid = conv_grid((int64_t)B * H * W);
  if (!((cin == 1 && cout_real == 64) || (cin == 4 && cout_real == 32))) return TDX_E_SHAPE;
  TDX_IO_DISPATCH(io16, T,
    if (cin == 1) thin_to_fat_conv_kernel<1, false, T><<<grid, 256, 0, st>>>(x, w, bias, (T*)out, B, H, W, cout_real);
    else thin_to_fat_conv_kernel<4, false, T><<<grid, 256, 0, st>>>(x, w, bias, (T*)out, B, H, W, cout_real));
  TDX_CHECK_LAUNCH();
  return 0;
}

int tdx_final_conv_dgrad(const float* g_out, const float* w, void* g_in, int B, int H, int W,
                         int cout, hipStream_t st, int io16) {
  const int grid = conv_grid((int64_t)B * H * W);
  if (cout != 1 && cout != 4) return TDX_E_SHAPE;
  TDX_IO_DISPATCH(io16, T,
    if (cout == 1) thin_to_fat_conv_kernel<1, true, T><<<grid, 256, 0, st>>>(g_out, w, nullptr, (T*)g_in, B, H, W, IC_CO);
    else thin_to_fat_conv_kernel<4, true, T><<<grid, 256, 0, st>>>(g_out, w, nullptr, (T*)g_in, B, H, W, IC_CO));
  TDX_CHECK_LAUNCH();
  return 0;
}

int tdx_final_conv_fwd(const void* in, const float* w, const float* bias, float* out, int B, int H,
                       int W, int cout, hipStream_t st, int io16) {
  const int64_t M = (int64_t)B * H * W;
  const int grid = (int)std::min<int64_t>((M + 15) / 16, 8192);
  if (cout != 1 && cout != 4) return TDX_E_SHAPE;
  TDX_IO_DISPATCH(io16, T,
    if (cout == 1) fat_to_thin_conv_kernel<1, false, false, T><<<grid, 256, 0, st>>>((const T*)in, w, bias, out, B, H, W, IC_CO, PStep{});
    else fat_to_thin_conv_kernel<4, false, false, T><<<grid, 256, 0, st>>>((const T*)in, w, bias, out, B, H, W, IC_CO, PStep{}));
  TDX_CHECK_LAUNCH();
  return 0;
}

// d loss / d x of the network: the input gradient of initial_conv (the reference's module is differentiable in
// its input like any nn.Module, diffusion.py:116; not needed by train() or sample(), so only on request).
// g_x0: channels-last, 64 stored channels; g_x: NCHW (B, cin, H, W).
int tdx_initial_conv_dgrad(const void* g_x0, const float* w, float* g_x, int B, int H, int W, int cin,
                           int cout_real, hipStream_t st, int io16) {
  const int64_t M = (int64_t)B * H * W;
  const int grid = (int)std::min<int64_t>((M + 15) / 16, 8192);
  if (!((cin == 1 && cout_real == 64) || (cin == 4 && cout_real == 32))) return TDX_E_SHAPE;
  TDX_IO_DISPATCH(io16, T,
    if (cin == 1) fat_to_thin_conv_kernel<1, true, false, T><<<grid, 256, 0, st>>>((const T*)g_x0, w, nullptr, g_x, B, H, W, cout_real, PStep{});
    else fat_to_thin_conv_kernel<4, true, false, T><<<grid, 256, 0, st>>>((const T*)g_x0, w, nullptr, g_x, B, H, W, cout_real, PStep{}));
  TDX_CHECK_LAUNCH();
  return 0;
}

// final_conv forward with the reverse-process update fused in (sampling; PStep): one dispatch over the element type of
// the input, cout, guided, the form and masked
namespace {
template <typename T, bool GD, int FORM, bool MK>
void launch_psample(const void* in, const float* w, const float* bias, float* eps_out, int B, int H, int W, int cout,
                    const PStep& ps, int grid, hipStream_t st) {
  if (cout == 1) fat_to_thin_conv_kernel<1, false, true, T, GD, FORM, MK><<<grid, 256, 0, st>>>((const T*)in, w, bias, eps_out, B, H, W, IC_CO, ps);
  else fat_to_thin_conv_kernel<4, false, true, T, GD, FORM, MK><<<grid, 256, 0, st>>>((const T*)in, w, bias, eps_out, B, H, W, IC_CO, ps);
}
template <typename T, bool GD>
void launch_psample_form(const void* in, const float* w, const float* bias, float* eps_out, int B, int H, int W,
                         int cout, const PStep& ps, int grid, hipStream_t st) {
#define TDX_PS_FORM(FORM_, MK_) launch_psample<T, GD, FORM_, MK_>(in, w, bias, eps_out, B, H, W, cout, ps, grid, st)
  if (ps.form == TDX_STEP_EPS) TDX_PS_FORM(TDX_STEP_EPS, false);
  else if (ps.form == TDX_STEP_X0) { if (ps.known) TDX_PS_FORM(TDX_STEP_X0, true); else TDX_PS_FORM(TDX_STEP_X0, false); }
  else { if (ps.known) TDX_PS_FORM(TDX_STEP_MS, true); else TDX_PS_FORM(TDX_STEP_MS, false); }
#undef TDX_PS_FORM
}
}  // namespace

int tdx_final_conv_fwd_psample(const void* in, const float* w, const float* bias, float* eps_out, int B, int H, int W,
                               int cout, const PStep& s, hipStream_t st, int io16) {
  if (!s.x || (s.guided && (B & 1))) return TDX_E_BADARG;   // guided: two equal halves
  if (s.thr) return TDX_E_BADARG;   // a sample's bound needs the whole output first: never in the epilogue
  const int64_t M = (int64_t)(s.guided ? B / 2 : B) * H * W;
  if (pstep_valid(s, M * cout)) return TDX_E_BADARG;
  if (cout != 1 && cout != 4) return TDX_E_SHAPE;
  const int grid = (int)std::min<int64_t>((M + 15) / 16, 8192);
  PStep ps = s;
  ps.half = s.guided ? M * cout : 0;
  TDX_IO_DISPATCH(io16, T,
    if (s.guided) launch_psample_form<T, true>(in, w, bias, eps_out, B, H, W, cout, ps, grid, st);
    else launch_psample_form<T, false>(in, w, bias, eps_out, B, H, W, cout, ps, grid, st));
  TDX_CHECK_LAUNCH();
  return 0;
}

int tdx_small_conv_wgrad_blocks(int B, int H, int W) {
  return cdiv((int64_t)B * H * W, WGRAD_PIX);
}
int tdx_small_conv_partial_width(void) { return SMALLP_W; }

int tdx_initial_conv_wgrad(const float* x, const void* g, float* partial, float* dw, float* db,
                           int B, int H, int W, int cin, int cout_real, hipStream_t st, int io16) {
  const int nblk = tdx_small_conv_wgrad_blocks(B, H, W);
  if (W < 4) return TDX_E_SHAPE;
  if (!((cin == 1 && cout_real == 64) || (cin == 4 && cout_real == 32))) return TDX_E_SHAPE;
  TDX_IO_DISPATCH(io16, T,
    if (cin == 1) thin_fat_wgrad_kernel<1, false, T><<<nblk, 256, 0, st>>>(x, (const T*)g, partial, B, H, W, WGRAD_PIX, cout_real);
    else thin_fat_wgrad_kernel<4, false, T><<<nblk, 256, 0, st>>>(x, (const T*)g, partial, B, H, W, WGRAD_PIX, cout_real));
  TDX_CHECK_LAUNCH();
  // columns [0, nw) -> dw (contiguous [co][ci][tap]), then cout_real columns -> db
  const int nw = cout_real * cin * 9;
  return reduce_partials2(partial, dw, db, nw, nblk, SMALLP_W, nw + cout_real, st);
}

int tdx_final_conv_wgrad(const void* in, const float* g_out, float* partial, float* dw, float* db,
                         int B, int H, int W, int cout, hipStream_t st, int io16) {
  const int nblk = tdx_small_conv_wgrad_blocks(B, H, W);
  if (W < 4) return TDX_E_SHAPE;
  if (cout != 1 && cout != 4) return TDX_E_SHAPE;
  TDX_IO_DISPATCH(io16, T,
    if (cout == 1) thin_fat_wgrad_kernel<1, true, T><<<nblk, 256, 0, st>>>(g_out, (const T*)in, partial, B, H, W, WGRAD_PIX, IC_CO);
    else thin_fat_wgrad_kernel<4, true, T><<<nblk, 256, 0, st>>>(g_out, (const T*)in, partial, B, H, W, WGRAD_PIX, IC_CO));
  TDX_CHECK_LAUNCH();
  return reduce_partials2(partial, dw, db, cout * 576, nblk, SMALLP_W, cout * 576 + cout, st);
}

// ------------------------------------------------------------------ C ABI (the boundary convolutions on their own)
extern "C" size_t tdx_edge_conv_wgrad_scratch_floats(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)tdx_small_conv_wgrad_blocks(B, H, W) * SMALLP_W;
}
// The _io forms: io16 != 0 -> the fat channels-last tensor (64 stored channels) holds bf16; the thin NCHW tensor, the
// weights and the weight gradients are fp32 either way.  The fp32 entries are the _io forms at io16 == 0.
extern "C" int tdx_initial_conv_forward_io(const float* x, const float* w, const float* bias, void* out, int B, int H,
                                           int W, int cin, int cout, int io16, tdx_stream_t stream) {
  if (!x || !w || !out || B <= 0 || H <= 0 || W <= 0) return TDX_E_BADARG;
  return tdx_initial_conv_fwd(x, w, bias, out, B, H, W, cin, cout, to_stream(stream), io16 ? 1 : 0);
}
extern "C" int tdx_initial_conv_backward_io(const float* x, const void* g_out, float* dw, float* db, float* scratch,
                                            int B, int H, int W, int cin, int cout, int io16, tdx_stream_t stream) {
  if (!x || !g_out || !dw || !db || !scratch || B <= 0 || H <= 0 || W <= 0) return TDX_E_BADARG;
  return tdx_initial_conv_wgrad(x, g_out, scratch, dw, db, B, H, W, cin, cout, to_stream(stream), io16 ? 1 : 0);
}
extern "C" int tdx_initial_conv_input_grad_io(const void* g_out, const float* w, float* g_x, int B, int H, int W,
                                              int cin, int cout, int io16, tdx_stream_t stream) {
  if (!g_out || !w || !g_x || B <= 0 || H <= 0 || W <= 0) return TDX_E_BADARG;
  return tdx_initial_conv_dgrad(g_out, w, g_x, B, H, W, cin, cout, to_stream(stream), io16 ? 1 : 0);
}
extern "C" int tdx_final_conv_forward_io(const void* in, const float* w, const float* bias, float* out, int B, int H,
                                         int W, int cout, int io16, tdx_stream_t stream) {
  if (!in || !w || !bias || !out || B <= 0 || H <= 0 || W <= 0) return TDX_E_BADARG;
  return tdx_final_conv_fwd(in, w, bias, out, B, H, W, cout, to_stream(stream), io16 ? 1 : 0);
}
extern "C" int tdx_final_conv_backward_io(const void* in, const float* g_out, const float* w, void* g_in, float* dw,
                                          float* db, float* scratch, int B, int H, int W, int cout, int io16,
                                          tdx_stream_t stream) {
  if (!in || !g_out || !w || !g_in || !dw || !db || !scratch || B <= 0 || H <= 0 || W <= 0) return TDX_E_BADARG;
  if (W < 4 || (cout != 1 && cout != 4)) return TDX_E_SHAPE;   // (before the input gradient: a refused call writes nothing)
  const int rc = tdx_final_conv_dgrad(g_out, w, g_in, B, H, W, cout, to_stream(stream), io16 ? 1 : 0);
  if (rc) return rc;
  return tdx_final_conv_wgrad(in, g_out, scratch, dw, db, B, H, W, cout, to_stream(stream), io16 ? 1 : 0);
}
extern "C" int tdx_initial_conv_forward(const float* x, const float* w, const float* bias, float* out, int B, int H,
                                        int W, int cin, int cout, tdx_stream_t stream) {
  return tdx_initial_conv_forward_io(x, w, bias, out, B, H, W, cin, cout, 0, stream);
}
extern "C" int tdx_initial_conv_backward(const float* x, const float* g_out, float* dw, float* db, float* scratch,
                                         int B, int H, int W, int cin, int cout, tdx_stream_t stream) {
  return tdx_initial_conv_backward_io(x, g_out, dw, db, scratch, B, H, W, cin, cout, 0, stream);
}
extern "C" int tdx_initial_conv_input_grad(const float* g_out, const float* w, float* g_x, int B, int H, int W,
                                           int cin, int cout, tdx_stream_t stream) {
  return tdx_initial_conv_input_grad_io(g_out, w, g_x, B, H, W, cin, cout, 0, stream);
}
extern "C" int tdx_final_conv_forward(const float* in, const float* w, const float* bias, float* out, int B, int H,
                                      int W, int cout, tdx_stream_t stream) {
  return tdx_final_conv_forward_io(in, w, bias, out, B, H, W, cout, 0, stream);
}
extern "C" int tdx_final_conv_backward(const float* in, const float* g_out, const float* w, float* g_in, float* dw,
                                       float* db, float* scratch, int B, int H, int W, int cout,
                                       tdx_stream_t stream) {
  return tdx_final_conv_backward_io(in, g_out, w, g_in, dw, db, scratch, B, H, W, cout, 0, stream);
}
