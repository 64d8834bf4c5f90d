// Pieces shared by the fp32 (conv3x3.hip) and bf16 (conv3x3_bf16.hip) implicit-GEMM convolutions:
// the argument block and the epilogue (bias, BatchNorm statistics / BN+ReLU, split-K partials).  The C/D
// register map of the 32x32 MFMA does not depend on the operand type, so one epilogue serves both.
#pragma once
#include "internal.h"

enum { EPI_PLAIN = 0, EPI_STATS = 1, EPI_BNRELU = 2, EPI_BNBWD = 3 };

struct ConvArgs {
  const float* in;
  const float* w;  // [Cout][9][Cin]
  const float* bias;
  float* out;
  const float* in_scale;
  const float* in_shift;
  const float* out_scale;
  const float* out_shift;
  float* stats;  // [tilesM][2][Cout]
  int B, H, W, Cin, Cout, M, tilesN;
  int splits, kt_per_split;  // split-K: blockIdx.y = split, raw partials to `out`
  int dbg;                   // timing experiments only (tdx_tune_set "conv_dbg"): 1 no barrier,
                             // 2 no LDS stores, 4 no global loads in the main loop -> WRONG results
  // hybrid launch (training, non-split kernels): block ids >= hyb_full are K-SLICES of the last row tiles -
  // id hyb_full + q is slice q % hyb_sp (kt_per_split K-tiles) of virtual block hyb_full + q / hyb_sp - and write
  // raw partials to hyb_scratch[slice][row - hyb_row0][Cout]; hyb_sp = 0: off (conv3x3.hip, plan_hybrid)
  int hyb_full, hyb_sp, hyb_row0;
  float* hyb_scratch;
  // EPI_BNBWD (input-gradient launches of the backward): the tensor this launch writes is dL/d(activation) of the
  // unit BELOW, whose BatchNorm+ReLU backward comes next and starts with two per-channel reductions over
  // (this gradient, that unit's pre-BN output y).  The accumulators are still in registers here, so the epilogue
  // reads the matching y tile and emits the per-tile partial sums [tilesM][2][Cout] (sum gz, sum gz*xhat; gz = the
  // gradient where relu(bn(y)) is active) - the format bn_bwd_finalize reads - and the separate reduction pass
  // (8 B/element over both tensors + a launch on the backward's dependent chain) is not run.
  const float* bw_y;
  const float* bw_scale; const float* bw_shift; const float* bw_mean; const float* bw_rstd;
  float* bw_partial;
  int compact;    // small grids (fewer than 64 row tiles: inference at small n): workgroup id -> (row tile, column tile) WITHOUT the
                  // padding to groups of 8 row tiles - the XCD-aware order leaves whole XCDs idle when there are fewer than 8 row tiles
                  // (a 4x4 layer at n = 16 is 4 row tiles: ids with (id & 7) >= 4 exit at once, and those ARE XCDs 4-7)
  int out_bf16;   // bf16 storage mode: `out` holds bf16 and the epilogue rounds to nearest-even on store (conv3x3_bf16.hip)
  unsigned long long* stamps;  // diagnostics (tools/gpu_clock_probe.py): per workgroup {shader cycles, 100 MHz ticks}
                               // around the main loop; null in every product launch
};

// ---------------------------------------------------------------------------
// Shared epilogue.  C/D map of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
//   SPLITK      raw partial sums to a.out + split*M*Cout (bias/BN applied by splitk_reduce_kernel)
//   EPI_PLAIN   + bias
//   EPI_BNRELU  relu((acc + bias) * scale + shift)                       (inference)
//   EPI_STATS   + bias, and per-tile per-channel (sum, M2 about the TILE mean) from the accumulators
//               still in registers (two reductions); centred partials are merged with Chan's
//               formula in bn_finalize, so the variance never sees E[y^2]-E[y]^2 cancellation.
template <int BM, int BN, int EPI, bool SPLITK>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, f32x16 (&acc)[BM / 64][BN / 64],
                                              float* smem, int tile_m, int m0, int n0, int wm, int wn,
                                              int l31, int half, int tid) {
  constexpr int WGM = 2;
  constexpr int WTM = BM / 2, WTN = BN / 2, TM = BM / 64, TN = BN / 64;
  if (SPLITK) {
    float* part = a.out + (size_t)blockIdx.y * a.M * a.Cout;
#pragma unroll
    for (int in = 0; in < TN; ++in) {
      const int col = n0 + wn * WTN + in * 32 + l31;
#pragma unroll
      for (int im = 0; im < TM; ++im)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int p = m0 + wm * WTM + im * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          if (p < a.M) part[(size_t)p * a.Cout + col] = acc[im][in][r];
        }
    }
    return;
  }
  if (EPI == EPI_BNBWD) {
    float s1[TN], s2[TN];
#pragma unroll
    for (int in = 0; in < TN; ++in) {
      const int col = n0 + wn * WTN + in * 32 + l31;
      const float bv = a.bias ? a.bias[col] : 0.f;
      const float sc = a.bw_scale[col], sh = a.bw_shift[col], mu = a.bw_mean[col], rs = a.bw_rstd[col];
      float yv[TM][16];
#pragma unroll
      for (int im = 0; im < TM; ++im)   // all of the tile's y loads in flight together
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int p = m0 + wm * WTM + im * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          yv[im][r] = p < a.M ? a.bw_y[(size_t)p * a.Cout + col] : 0.f;
        }
      float a1 = 0.f, a2 = 0.f;
#pragma unroll
      for (int im = 0; im < TM; ++im)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int p = m0 + wm * WTM + im * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          const float v = acc[im][in][r] + bv;
          if (p < a.M) {
            a.out[(size_t)p * a.Cout + col] = v;
            const float gz = fmaf(yv[im][r], sc, sh) > 0.f ? v : 0.f;   // the mask of bn_bwd_reduce / bn_bwd_apply
            a1 += gz;
            a2 += gz * ((yv[im][r] - mu) * rs);
          }
        }
      s1[in] = a1 + __shfl_xor(a1, 32, 64);
      s2[in] = a2 + __shfl_xor(a2, 32, 64);
    }
    float* red = smem;  // [2][WGM][BN], re-uses the tile buffers (K loop is over)
    __syncthreads();    // every wave is done with the tile buffers
#pragma unroll
    for (int in = 0; in < TN; ++in)
      if (half == 0) {
        red[(0 * WGM + wm) * BN + wn * WTN + in * 32 + l31] = s1[in];
        red[(1 * WGM + wm) * BN + wn * WTN + in * 32 + l31] = s2[in];
      }
    __syncthreads();
    for (int c = tid; c < 2 * BN; c += 256) {
      const int q = c / BN, cc = c - q * BN;
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < WGM; ++w) v += red[(q * WGM + w) * BN + cc];   // fixed order: deterministic
      a.bw_partial[((size_t)tile_m * 2 + q) * a.Cout + n0 + cc] = v;
    }
    return;
  }
  // bf16 OUTPUT (bf16 storage mode): in the accumulator layout a wave-instruction covers two rows x 32 columns, i.e.
  // two 64-byte half lines per store when the elements are 2 bytes wide - the input gradient of dec1.0 (134 MB of
  // output from nine K-tiles of work) took 490 us that way.  The tile is rounded into LDS instead (the K loop is
  // over; pitch BN + 8 elements) and written out as whole rows, 16 bytes per lane.
  const bool stage16 = a.out_bf16 != 0;   // workgroup-uniform
  constexpr int CPITCH = BN + 8;
  __bf16* ctile = reinterpret_cast<__bf16*>(smem);
  if (stage16) __syncthreads();           // every wave is done with the tile buffers
  float csum[TN];
#pragma unroll
  for (int in = 0; in < TN; ++in) {
    const int lcol = wn * WTN + in * 32 + l31;
    const int col = n0 + lcol;
    const float bv = a.bias ? a.bias[col] : 0.f;
    float osc = 1.f, osh = 0.f;
    if (EPI == EPI_BNRELU) {
      osc = a.out_scale[col];
      osh = a.out_shift[col];
    }
    float s = 0.f;
#pragma unroll
    for (int im = 0; im < TM; ++im) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * WTM + im * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const int p = m0 + row;
        float v = acc[im][in][r] + bv;
        if (EPI == EPI_BNRELU) v = fmaxf(fmaf(v, osc, osh), 0.f);
        acc[im][in][r] = v;
        if (p < a.M) {
          if (stage16) ctile[row * CPITCH + lcol] = (__bf16)v;
          else a.out[(size_t)p * a.Cout + col] = v;
          s += v;
        }
      }
    }
    csum[in] = s;
  }
  if (stage16) {
    __syncthreads();
    constexpr int CH = BN / 8;   // 16-byte chunks per tile row
    __bf16* out16 = reinterpret_cast<__bf16*>(a.out);
    for (int c = tid; c < BM * CH; c += 256) {
      const int row = c / CH, cc = c - row * CH;
      if (m0 + row < a.M)
        *reinterpret_cast<f32x4*>(out16 + (size_t)(m0 + row) * a.Cout + n0 + cc * 8) =
            *reinterpret_cast<const f32x4*>(ctile + row * CPITCH + cc * 8);
    }
    // (the statistics code below opens with a barrier of its own before it re-uses this LDS)
  }
  if (EPI == EPI_STATS) {
    // Per tile and channel: (sum, M2 about the TILE mean), two passes over the accumulators with the tile mean
    // going through LDS in between (five barriers).  The one-pass alternative below it (round 3, knob
    // "stats_epi" = 1: every lane centres its 16*TM rows about their own mean, (count, sum, M2) triples merged
    // pairwise with Chan's formula - lane halves by shuffle, row waves through LDS - two barriers) gives the same
    // statistics to rounding and was MEASURED no faster (B = 256 step 15.50 vs 15.54 ms): the epilogue's cost is
    // its stores and the drain of the tile, not its barriers.  Kept as the experiment it was.
    if (!(a.dbg & 8)) {
      float* red = smem;  // [WGM][BN] + [BN] means, re-uses the tile buffers (K loop is over)
      const int rows_valid = min(BM, a.M - m0);
      __syncthreads();    // every wave is done with the tile buffers
#pragma unroll
      for (int in = 0; in < TN; ++in) {
        const float s = csum[in] + __shfl_xor(csum[in], 32, 64);
        if (half == 0) red[wm * BN + wn * WTN + in * 32 + l31] = s;
      }
      __syncthreads();
      float* tsum = red + WGM * BN;  // [BN] tile column sums
      for (int c = tid; c < BN; c += 256) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < WGM; ++w) v += red[w * BN + c];
        tsum[c] = v;
        a.stats[((size_t)tile_m * 2 + 0) * a.Cout + n0 + c] = v;
      }
      __syncthreads();
      const float inv_n = 1.0f / (float)rows_valid;
      float cm2[TN];
#pragma unroll
      for (int in = 0; in < TN; ++in) {
        const float mean = tsum[wn * WTN + in * 32 + l31] * inv_n;
        float q = 0.f;
#pragma unroll
        for (int im = 0; im < TM; ++im)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = wm * WTM + im * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (m0 + row < a.M) {
              const float dlt = acc[im][in][r] - mean;
              q = fmaf(dlt, dlt, q);
            }
          }
        cm2[in] = q + __shfl_xor(q, 32, 64);
      }
      __syncthreads();  // everyone has read tsum/red
#pragma unroll
      for (int in = 0; in < TN; ++in)
        if (half == 0) red[wm * BN + wn * WTN + in * 32 + l31] = cm2[in];
      __syncthreads();
      for (int c = tid; c < BN; c += 256) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < WGM; ++w) v += red[w * BN + c];
        a.stats[((size_t)tile_m * 2 + 1) * a.Cout + n0 + c] = v;
      }
      return;
    }
    // rows of this lane that exist (the last row tile may be ragged); the same for every column
    int nl = 0;
#pragma unroll
    for (int im = 0; im < TM; ++im)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        nl += (m0 + wm * WTM + im * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) < a.M ? 1 : 0;
    const float fn = (float)nl;
    const float fn_o = __shfl_xor(fn, 32, 64);
    const float fn2 = fn + fn_o;                       // rows of this wave's 32*TM-row slab
    float* red = smem;  // [3][WGM][BN]: count | sum | M2 of each row wave, re-uses the tile buffers (K loop is over)
    __syncthreads();    // every wave is done with the tile buffers
#pragma unroll
    for (int in = 0; in < TN; ++in) {
      const float s = csum[in];
      const float mean = nl ? s / fn : 0.f;
      float q = 0.f;
#pragma unroll
      for (int im = 0; im < TM; ++im)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wm * WTM + im * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          if (m0 + row < a.M) {
            const float dlt = acc[im][in][r] - mean;
            q = fmaf(dlt, dlt, q);
          }
        }
      // Chan: the other half's (fn_o, s_o, q_o)
      const float s_o = __shfl_xor(s, 32, 64), q_o = __shfl_xor(q, 32, 64);
      const float mean_o = fn_o > 0.f ? s_o / fn_o : 0.f;
      const float d = mean - mean_o;
      const float w = fn2 > 0.f ? fn * fn_o / fn2 : 0.f;
      const float s2 = s + s_o, q2 = q + q_o + d * d * w;
      if (half == 0) {
        const int c = wn * WTN + in * 32 + l31;
        red[(0 * WGM + wm) * BN + c] = fn2;
        red[(1 * WGM + wm) * BN + c] = s2;
        red[(2 * WGM + wm) * BN + c] = q2;
      }
    }
    __syncthreads();
    for (int c = tid; c < BN; c += 256) {
      const float n0f = red[(0 * WGM + 0) * BN + c], n1f = red[(0 * WGM + 1) * BN + c];
      const float s0 = red[(1 * WGM + 0) * BN + c], s1 = red[(1 * WGM + 1) * BN + c];
      const float q0 = red[(2 * WGM + 0) * BN + c], q1 = red[(2 * WGM + 1) * BN + c];
      const float nt = n0f + n1f;
      const float d = (n0f > 0.f ? s0 / n0f : 0.f) - (n1f > 0.f ? s1 / n1f : 0.f);
      const float w = nt > 0.f ? n0f * n1f / nt : 0.f;
      a.stats[((size_t)tile_m * 2 + 0) * a.Cout + n0 + c] = s0 + s1;
      a.stats[((size_t)tile_m * 2 + 1) * a.Cout + n0 + c] = q0 + q1 + d * d * w;
    }
  }
}

// ---------------------------------------------------------------------- wgrad
// GEMM: rows = output channels, cols = input channels of ONE tap, K = pixels, split over pixel chunks
// into deterministic slabs [S][Cout][9][Cin] that tdx_conv3x3_wgrad_reduce sums in a fixed order.
struct WgradArgs {
  const float* in;  // (B,H,W,Cin)
  const float* dy;  // (B,H,W,Cout)
  float* slabs;     // [S][Cout][9][Cin]
  const float* in_scale;
  const float* in_shift;
  int B, H, W, Cin, Cout, M, tilesCi, tilesCo, groups, chunk;
  int adv_q, adv_s;  // 32 pixels = adv_q rows + adv_s columns of a W-wide image
  int dbg;           // ablation bits of the bf16 kernels (tdx_tune_set("conv_dbg")): 16 no MFMA, 32 no LDS staging, 64 no loads
};

void tdx_wgrad_plan(int64_t M, int cin, int cout, int* bm, int* bn, int* splits, int* chunk, bool bf16 = false);
