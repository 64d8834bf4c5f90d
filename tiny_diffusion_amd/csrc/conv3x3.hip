// 3x3 / pad 1 / stride 1 convolution on the fp32 matrix cores of gfx950
// (v_mfma_f32_32x32x2_f32: exact fp32, 64 FLOP/clk/SIMD), channels-last.
//
// Replaces every nn.Conv2d(cin, cout, 3, padding=1) with cin >= 64 of the
// reference UNet (diffusion.py:32-95) - >= 99.9 % of its FLOPs - in three roles:
//   forward   out[p][co]   = sum_{tap,ci} in[p+tap][ci] * W[co][tap][ci]
//   dgrad     same kernel on the flipped/transposed pack of W
//   wgrad     dW[co][tap][ci] = sum_p dy[p][co] * in[p+tap][ci]   (split over p)
//
// Implicit GEMM, no im2col buffer: a K-tile is 32 input channels of ONE tap, so
// an A-tile row is 128 contiguous bytes of the NHWC input (or zeros for padding).
// Tiles are staged global -> registers -> LDS (double-buffered, the loads of tile
// k+1 are issued before the MFMAs of tile k and written after them), rows padded
// to 36 floats so that the ds_read_b128 fragment reads are bank-conflict-free.
//
// MFMA operand trick: lane l supplies A[i=l&31][k=l>>5].  Each lane reads FOUR
// consecutive k of its row with one ds_read_b128 (lanes 0-31 take k..k+3, lanes
// 32-63 take k+4..k+7) and issues four MFMAs from it; A and B use the same
// permutation of k, so the sum over k is unchanged.
#include "internal.h"

#define BK 32   // K-tile: 32 channels of one tap
#define BKP 36  // padded LDS row (floats)

#include "conv_shared.h"

// Register-staging kernel of the BN-on-load launches: relu(in * in_scale + in_shift) is applied between the staging
// registers and LDS (raw inputs run on conv3x3_igemm_dma_kernel).
template <int BM, int BN, int EPI>
__global__ void __launch_bounds__(256)
conv3x3_igemm_kernel(ConvArgs a) {
  constexpr int WGM = 2, WGN = 2;  // 4 waves as 2 x 2
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int AI = BM / 32, BI = BN / 32;  // float4 loads per thread per K-tile
  static_assert(TM >= 1 && TN >= 1, "wave tile must hold a 32x32 MFMA tile");

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                 // [2][BM][BKP]
  float* Bs = smem + 2 * BM * BKP;  // [2][BN][BKP]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int wm = wave / WGN, wn = wave % WGN;
  // Workgroup id -> tile, XCD-aware: ids are dealt round-robin over the 8 XCDs, so the tilesN
  // column tiles of one row tile (which read the same input rows) are given ids that differ by
  // multiples of 8 inside a block of 8*tilesN consecutive ids: same XCD, same L2, close in time.
  const int xb = blockIdx.x / (8 * a.tilesN), xr = blockIdx.x % (8 * a.tilesN);
  const int tile_m = xb * 8 + (xr & 7), tile_n = xr >> 3;
  if (tile_m * BM >= a.M) return;  // grid is padded to a multiple of 8 row tiles
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int HW = a.H * a.W;

  // ---- loaders.  On gfx950 the fp32 "matrix" instruction runs at the vector-ALU rate and every
  // VALU instruction in the loop competes with it, so the per-tile address work is kept off the
  // vector unit: tiles are fetched with BUFFER loads whose address is
  //     descriptor base (SGPRs) + per-thread row offset (one VGPR, fixed) + per-tile offset (one SGPR)
  // and zero padding is the hardware range check: a row outside the image gets an offset beyond
  // num_records and the load returns 0.  Per row and K-tile that leaves one bit test + select.
  const int ld_row = tid >> 3, ld_c4 = (tid & 7) * 4;
  // the descriptor starts (W+1) pixels BEFORE the tensor so that every tap's shift is >= 0
  const int neg = (a.W + 1) * a.Cin;
  const auto rsrc_in = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.in) - neg, 0, (int)(((int64_t)a.M * a.Cin + 2 * neg) * 4), 0x00020000);
  const auto rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0,
                                                        a.Cout * 9 * a.Cin * 4, 0x00020000);
  constexpr unsigned OOB = 0x80000000u;
  unsigned a_off[AI], a_taps[AI];  // byte offset of (pixel, chunk); bit t set <=> tap t is inside the image
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int p = m0 + ld_row + 32 * i;
    unsigned taps = 0;
    if (p < a.M) {
      const int r = p % HW, oh = r / a.W, ow = r % a.W;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int ih = oh + t / 3 - 1, iw = ow + t % 3 - 1;
        if ((unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W) taps |= 1u << t;
      }
    }
    a_taps[i] = taps;
    a_off[i] = (unsigned)(p * a.Cin + ld_c4) * 4u;
  }
  unsigned w_off[BI];
#pragma unroll
  for (int j = 0; j < BI; ++j) w_off[j] = (unsigned)((n0 + ld_row + 32 * j) * 9 * a.Cin + ld_c4) * 4u;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int im = 0; im < TM; ++im)
#pragma unroll
    for (int in = 0; in < TN; ++in)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[im][in][r] = 0.f;

  const int nk = 9 * (a.Cin / BK);
  f32x4 ra[AI], rb[BI];  // ext-vector staging registers: arrays of HIP float4 structs fall back to
                          // scratch once a sched_barrier sits between their definition and use
  float4 sc4 = make_float4(1.f, 1.f, 1.f, 1.f), sh4 = make_float4(0.f, 0.f, 0.f, 0.f);

  // Software pipeline: iteration kt ISSUES the loads of tile kt+1 first (clamped: the last
  // iteration re-loads the last tile and stores it into the idle buffer, which nobody reads),
  // then runs the 64 MFMAs of tile kt from LDS, then writes the staged registers to the other
  // LDS buffer.  kt = -1 is the prologue.  The loads are fenced with sched_barrier: left to
  // itself hipcc sinks them BELOW the MFMA block and then waits with nothing left to overlap.
  int cur = 1;
  for (int kt = -1; kt < nk; ++kt) {
    unsigned okmask = 0;
    {
      const int kn = min(kt + 1, nk - 1);
      const int cblk = kn / 9, tap = kn - cblk * 9;
      const int c0 = cblk * BK + ld_c4;
      // tap shift relative to the descriptor base: ((kh)*W + kw)*Cin, kh,kw in 0..2
      const unsigned soff_in = (unsigned)(((tap / 3) * a.W + (tap % 3)) * a.Cin + cblk * BK) * 4u;
      const unsigned soff_w = (unsigned)(tap * a.Cin + cblk * BK) * 4u;
#pragma unroll
      for (int j = 0; j < BI; ++j)
        rb[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, w_off[j], soff_w, 0));
      sc4 = *reinterpret_cast<const float4*>(a.in_scale + c0);
      sh4 = *reinterpret_cast<const float4*>(a.in_shift + c0);
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        const bool ok = (a_taps[i] >> tap) & 1u;
        okmask |= ok ? (1u << i) : 0u;
        ra[i] = __builtin_bit_cast(
            f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_in, ok ? a_off[i] : OOB, soff_in, 0));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (kt >= 0) {
      const float* Ab = As + cur * BM * BKP + (wm * WTM + l31) * BKP + half * 4;
      const float* Bb = Bs + cur * BN * BKP + (wn * WTN + l31) * BKP + half * 4;
#pragma unroll
      for (int ks = 0; ks < BK / 8; ++ks) {
        f32x4 af[TM], bf[TN];
#pragma unroll
        for (int im = 0; im < TM; ++im)
          af[im] = *reinterpret_cast<const f32x4*>(Ab + im * 32 * BKP + ks * 8);
#pragma unroll
        for (int in = 0; in < TN; ++in)
          bf[in] = *reinterpret_cast<const f32x4*>(Bb + in * 32 * BKP + ks * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int im = 0; im < TM; ++im)
#pragma unroll
            for (int in = 0; in < TN; ++in)
              acc[im][in] =
                  __builtin_amdgcn_mfma_f32_32x32x2f32(af[im][j], bf[in][j], acc[im][in], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    {
      float* Ab = As + (cur ^ 1) * BM * BKP;
      float* Bb = Bs + (cur ^ 1) * BN * BKP;
#pragma unroll
      for (int i = 0; i < AI; ++i) {
        f32x4 v = ra[i];
        // padding must stay 0 AFTER the transform (relu(shift) != 0): only here is the mask needed
        v[0] = fmaxf(fmaf(v[0], sc4.x, sh4.x), 0.f);
        v[1] = fmaxf(fmaf(v[1], sc4.y, sh4.y), 0.f);
        v[2] = fmaxf(fmaf(v[2], sc4.z, sh4.z), 0.f);
        v[3] = fmaxf(fmaf(v[3], sc4.w, sh4.w), 0.f);
        if (!((okmask >> i) & 1u)) v = f32x4{0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(Ab + (ld_row + 32 * i) * BKP + ld_c4) = v;
      }
#pragma unroll
      for (int j = 0; j < BI; ++j)
        *reinterpret_cast<f32x4*>(Bb + (ld_row + 32 * j) * BKP + ld_c4) = rb[j];
    }
    __syncthreads();
    cur ^= 1;
  }

  conv_epilogue<BM, BN, EPI, false>(a, acc, smem, tile_m, m0, n0, wm, wn, l31, half, tid);
}

// ---------------------------------------------------------------------------
// Variant 2, two register stages: today only the split-K launch of a BN-on-load input (launch_splitk; its unsplit
// instantiations lost the in-process A/B against conv3x3_igemm_kernel and are gone).  While the MFMAs of tile k
// run from LDS[k&1], the registers loaded during iteration k-1 (tile k+1) are written to
// LDS[(k+1)&1] in four slices BETWEEN the four MFMA groups, and the global loads of tile
// k+2 are issued into the other register stage.  A load therefore has a whole iteration
// (~4000 cycles) to land and the LDS stores ride in the shadow of the 64-cycle MFMAs, so a
// wave's instruction stream is MFMA-dense even with no co-resident partner wave.
template <int BM, int BN, bool IN_BN, int EPI, bool SPLITK = false>
__global__ void __launch_bounds__(256)
conv3x3_igemm2_kernel(ConvArgs a) {
  constexpr int WGM = 2, WGN = 2;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int AI = BM / 32, BI = BN / 32;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;
  float* Bs = smem + 2 * BM * BKP;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int wm = wave / WGN, wn = wave % WGN;
  // Workgroup id -> tile, XCD-aware: ids are dealt round-robin over the 8 XCDs, so the tilesN
  // column tiles of one row tile (which read the same input rows) are given ids that differ by
  // multiples of 8 inside a block of 8*tilesN consecutive ids: same XCD, same L2, close in time.
  const int xb = blockIdx.x / (8 * a.tilesN), xr = blockIdx.x % (8 * a.tilesN);
  const int tile_m = xb * 8 + (xr & 7), tile_n = xr >> 3;
  if (tile_m * BM >= a.M) return;  // grid is padded to a multiple of 8 row tiles
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int HW = a.H * a.W;

  // buffer-load loaders, exactly as in conv3x3_igemm_kernel
  const int ld_row = tid >> 3, ld_c4 = (tid & 7) * 4;
  const int neg = (a.W + 1) * a.Cin;
  const auto rsrc_in = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.in) - neg, 0, (int)(((int64_t)a.M * a.Cin + 2 * neg) * 4), 0x00020000);
  const auto rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0,
                                                        a.Cout * 9 * a.Cin * 4, 0x00020000);
  constexpr unsigned OOB = 0x80000000u;
  unsigned a_off[AI], a_taps[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int p = m0 + ld_row + 32 * i;
    unsigned taps = 0;
    if (p < a.M) {
      const int r = p % HW, oh = r / a.W, ow = r % a.W;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int ih = oh + t / 3 - 1, iw = ow + t % 3 - 1;
        if ((unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W) taps |= 1u << t;
      }
    }
    a_taps[i] = taps;
    a_off[i] = (unsigned)(p * a.Cin + ld_c4) * 4u;
  }
  unsigned w_off[BI];
#pragma unroll
  for (int j = 0; j < BI; ++j) w_off[j] = (unsigned)((n0 + ld_row + 32 * j) * 9 * a.Cin + ld_c4) * 4u;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int im = 0; im < TM; ++im)
#pragma unroll
    for (int in = 0; in < TN; ++in)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[im][in][r] = 0.f;

  // K-tiles [kt0, kt0 + nk) of the 9*Cin/32 are this workgroup's share (all of them unless
  // split-K spreads a small problem over more workgroups)
  const int nk_total = 9 * (a.Cin / BK);
  const int kt0 = SPLITK ? (int)blockIdx.y * a.kt_per_split : 0;
  const int nk = SPLITK ? min(a.kt_per_split, nk_total - kt0) : nk_total;

  struct Stage {
    f32x4 ra[AI];
    f32x4 rb[BI];
    f32x4 sc, sh;
    unsigned ok;
  };
  Stage S0, S1;

  auto load_tile = [&](int kt, Stage& S) {
    const int kn = kt0 + min(kt, nk - 1);
    const int cblk = kn / 9, tap = kn - cblk * 9;
    const int c0 = cblk * BK + ld_c4;
    const unsigned soff_in = (unsigned)(((tap / 3) * a.W + (tap % 3)) * a.Cin + cblk * BK) * 4u;
    const unsigned soff_w = (unsigned)(tap * a.Cin + cblk * BK) * 4u;
#pragma unroll
    for (int j = 0; j < BI; ++j)
      S.rb[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, w_off[j], soff_w, 0));
    if (IN_BN) {
      S.sc = *reinterpret_cast<const f32x4*>(a.in_scale + c0);
      S.sh = *reinterpret_cast<const f32x4*>(a.in_shift + c0);
    }
    unsigned ok = 0;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const bool v = (a_taps[i] >> tap) & 1u;
      if (IN_BN) ok |= v ? (1u << i) : 0u;
      S.ra[i] = __builtin_bit_cast(
          f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_in, v ? a_off[i] : OOB, soff_in, 0));
    }
    S.ok = ok;
  };
  // slice q (0..3) of the stores of a stage: AI/4 A rows and BI/4 B rows (at least one each
  // when AI, BI >= 4; smaller tiles put everything into the first slices)
  auto store_slice = [&](const Stage& S, int buf, int q) {
    float* Ab = As + buf * BM * BKP;
    float* Bb = Bs + buf * BN * BKP;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      if ((i * 4) / AI != q) continue;
      f32x4 v = S.ra[i];
      if (IN_BN) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(v[e], S.sc[e], S.sh[e]), 0.f);
        if (!((S.ok >> i) & 1u)) v = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      *reinterpret_cast<f32x4*>(Ab + (ld_row + 32 * i) * BKP + ld_c4) = v;
    }
#pragma unroll
    for (int j = 0; j < BI; ++j) {
      if ((j * 4) / BI != q) continue;
      *reinterpret_cast<f32x4*>(Bb + (ld_row + 32 * j) * BKP + ld_c4) = S.rb[j];
    }
  };
  auto mfma_group = [&](int buf, int ks) {
    const float* Ab = As + buf * BM * BKP + (wm * WTM + l31) * BKP + half * 4;
    const float* Bb = Bs + buf * BN * BKP + (wn * WTN + l31) * BKP + half * 4;
    f32x4 af[TM], bf[TN];
#pragma unroll
    for (int im = 0; im < TM; ++im) af[im] = *reinterpret_cast<const f32x4*>(Ab + im * 32 * BKP + ks * 8);
#pragma unroll
    for (int in = 0; in < TN; ++in) bf[in] = *reinterpret_cast<const f32x4*>(Bb + in * 32 * BKP + ks * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int im = 0; im < TM; ++im)
#pragma unroll
        for (int in = 0; in < TN; ++in)
          acc[im][in] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[im][j], bf[in][j], acc[im][in], 0, 0, 0);
  };
  // one iteration: compute tile kt from LDS[cur]; Sst (tile kt+1) -> LDS[cur^1]; load tile kt+2 -> Sld
  auto iteration = [&](int kt, int cur, const Stage& Sst, Stage& Sld) {
    if (!(a.dbg & 4)) load_tile(kt + 2, Sld);
    // keep the loads at the top of the iteration: hipcc would otherwise sink them to the
    // end, a few hundred cycles before the next iteration's first store waits for them
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < BK / 8; ++ks) {
      mfma_group(cur, ks);
      if (!(a.dbg & 2)) store_slice(Sst, cur ^ 1, ks);
    }
    if (!(a.dbg & 1)) __syncthreads();
  };

  // prologue: tile 0 -> LDS[0], tile 1 -> S1 registers
  load_tile(0, S0);
#pragma unroll
  for (int q = 0; q < 4; ++q) store_slice(S0, 0, q);
  load_tile(1, S1);
  __syncthreads();
  int kt = 0;
  for (; kt + 1 < nk; kt += 2) {
    iteration(kt, 0, S1, S0);      // S1 holds tile kt+1; load kt+2 -> S0
    iteration(kt + 1, 1, S0, S1);  // S0 holds tile kt+2; load kt+3 -> S1
  }
  if (kt < nk) iteration(kt, 0, S1, S0);  // odd tail

  conv_epilogue<BM, BN, EPI, SPLITK>(a, acc, smem, tile_m, m0, n0, wm, wn, l31, half, tid);
}

// ---------------------------------------------------------------------------
// Variant 3 (raw inputs only: every dgrad, and the forward of units fed by a materialised
// tensor): the tiles go global -> LDS directly (`buffer_load_dwordx4 ... lds`), no staging
// registers, no ds_write instructions, no address VALU.  An LDS-DMA wave-instruction writes
// 64 x 16 B = 1 KiB contiguously (base in M0 + lane*16), i.e. 8 rows of 128 B, so rows cannot
// be padded; bank conflicts of the ds_read_b128 fragment reads are avoided with an XOR swizzle
// applied on the SOURCE side: the lane that writes chunk position q of row r fetches logical
// chunk q ^ ((r >> 1) & 7), and the fragment read of logical chunk c of row r goes to position
// c ^ ((r >> 1) & 7).  Zero padding (image border, ragged M) is the hardware range check: a lane
// whose tap falls outside the image gets an out-of-range offset and the DMA writes zeros
// (probed on MI355X: tools/micro/lds_dma_probe.hip).
template <int BM, int BN, int EPI, bool SPLITK = false>
__global__ void __launch_bounds__(256)
conv3x3_igemm_dma_kernel(ConvArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass only needs the launch stub (LDS address-space casts do not parse there)
  constexpr int WGN = 2;
  constexpr int WTM = BM / 2, WTN = BN / 2;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int AI = BM / 32, BI = BN / 32;  // DMA instructions per wave per K-tile (A, B)
  typedef __attribute__((address_space(3))) void* lds_ptr_t;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                // [2][BM][32]
  float* Bs = smem + 2 * BM * BK;  // [2][BN][32]
  const unsigned long long t_entry = a.stamps ? __builtin_amdgcn_s_memrealtime() : 0ull;  // diagnostics only

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform (LDS base -> M0)
  const int l31 = lane & 31, half = lane >> 5;
  const int wm = wave / WGN, wn = wave % WGN;
  // Workgroup id -> tile, XCD-aware: ids are dealt round-robin over the 8 XCDs, so the tilesN
  // column tiles of one row tile (which read the same input rows) are given ids that differ by
  // multiples of 8 inside a block of 8*tilesN consecutive ids: same XCD, same L2, close in time.
  int vb = blockIdx.x, hyb_slice = -1;
  if (!SPLITK && a.hyb_sp > 0 && vb >= a.hyb_full) {  // K-slice of one of the last row tiles (hybrid launch)
    const int q = vb - a.hyb_full;
    hyb_slice = q % a.hyb_sp;
    vb = a.hyb_full + q / a.hyb_sp;
  }
  const int xb = vb / (8 * a.tilesN), xr = vb % (8 * a.tilesN);
  const int tile_m = a.compact ? vb / a.tilesN : xb * 8 + (xr & 7);
  const int tile_n = a.compact ? vb - tile_m * a.tilesN : xr >> 3;
  if (tile_m * BM >= a.M) return;  // grid is padded to a multiple of 8 row tiles
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int HW = a.H * a.W;

  // ---- DMA source offsets: lane -> (row 8*wave + lane/8 of each 32-row group, chunk position lane%8)
  const int lrow = wave * 8 + (lane >> 3);
  const int c_log = (lane & 7) ^ ((4 * wave + (lane >> 4)) & 7);  // logical chunk fetched by this lane
  const int neg = (a.W + 1) * a.Cin;
  const auto rsrc_in = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.in) - neg, 0, (int)(((int64_t)a.M * a.Cin + 2 * neg) * 4), 0x00020000);
  const auto rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0,
                                                        a.Cout * 9 * a.Cin * 4, 0x00020000);
  constexpr unsigned OOB = 0x80000000u;
  unsigned a_off[AI], a_taps[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int p = m0 + lrow + 32 * i;
    unsigned taps = 0;
    if (p < a.M) {
      const int r = p % HW, oh = r / a.W, ow = r % a.W;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int ih = oh + t / 3 - 1, iw = ow + t % 3 - 1;
        if ((unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W) taps |= 1u << t;
      }
    }
    a_taps[i] = taps;
    a_off[i] = (unsigned)(p * a.Cin + c_log * 4) * 4u;
  }
  unsigned w_off[BI];
#pragma unroll
  for (int j = 0; j < BI; ++j) w_off[j] = (unsigned)((n0 + lrow + 32 * j) * 9 * a.Cin + c_log * 4) * 4u;

  // ---- fragment-read offsets (floats): row wm*WTM + im*32 + l31, position (2*ks + half) ^ x
  const int x = (l31 >> 1) & 7;
  int frag_pos[BK / 8];
#pragma unroll
  for (int ks = 0; ks < BK / 8; ++ks) frag_pos[ks] = ((2 * ks + half) ^ x) * 4;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int im = 0; im < TM; ++im)
#pragma unroll
    for (int in = 0; in < TN; ++in)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[im][in][r] = 0.f;

  const int nk_total = 9 * (a.Cin / BK);
  const int kt0 = SPLITK ? (int)blockIdx.y * a.kt_per_split : hyb_slice >= 0 ? hyb_slice * a.kt_per_split : 0;
  const int nk = (SPLITK || hyb_slice >= 0) ? min(a.kt_per_split, nk_total - kt0) : nk_total;

  auto dma_tile = [&](int kt, int buf) {
    const int kn = kt0 + min(kt, nk - 1);
    const int cblk = kn / 9, tap = kn - cblk * 9;
    const unsigned soff_in = (unsigned)(((tap / 3) * a.W + (tap % 3)) * a.Cin + cblk * BK) * 4u;
    const unsigned soff_w = (unsigned)(tap * a.Cin + cblk * BK) * 4u;
    float* Ab = As + buf * BM * BK + wave * 8 * BK;
    float* Bb = Bs + buf * BN * BK + wave * 8 * BK;
#pragma unroll
    for (int j = 0; j < BI; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (lds_ptr_t)(Bb + j * 32 * BK), 16, w_off[j], soff_w, 0, 0);
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const bool ok = (a_taps[i] >> tap) & 1u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_in, (lds_ptr_t)(Ab + i * 32 * BK), 16,
                                               ok ? a_off[i] : OOB, soff_in, 0, 0);
    }
  };

  unsigned long long c0 = 0, r0 = 0;
  if (a.stamps) { c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
  dma_tile(0, 0);
  __syncthreads();  // (drains the DMA: hipcc waits vmcnt(0) in front of a barrier)
  int cur = 0;
  // Fragment registers are double-buffered: the four ds_read_b128 of k-step ks+1 are issued BEFORE
  // the 16 MFMAs of k-step ks (hipcc otherwise re-uses the same registers and places the reads
  // after the MFMAs that consume them, exposing the LDS latency once per k-step: ~10 % of the loop).
  f32x4 af[2][TM], bf[2][TN];
  auto read_frags = [&](int buf, int ks, int slot) {
    const float* Ab = As + buf * BM * BK + (wm * WTM + l31) * BK;
    const float* Bb = Bs + buf * BN * BK + (wn * WTN + l31) * BK;
#pragma unroll
    for (int im = 0; im < TM; ++im)
      af[slot][im] = *reinterpret_cast<const f32x4*>(Ab + im * 32 * BK + frag_pos[ks]);
#pragma unroll
    for (int in = 0; in < TN; ++in)
      bf[slot][in] = *reinterpret_cast<const f32x4*>(Bb + in * 32 * BK + frag_pos[ks]);
  };
  // (Tried in round 2: the two workgroups that share a CU alternating s_setprio every K-tile.  It makes the
  // sharing of the matrix pipes fair - main loops of 519..551 us instead of 434..561 on a one-round 128x128
  // launch - and leaves the launch at the same 562 us: the pipe runs at 88 % whoever gets it.)
  for (int kt = 0; kt < nk; ++kt) {
    dma_tile(kt + 1, cur ^ 1);  // clamped at the end: a redundant copy of the last tile, never read
    read_frags(cur, 0, 0);
#pragma unroll
    for (int ks = 0; ks < BK / 8; ++ks) {
      if (ks + 1 < BK / 8) {
        read_frags(cur, ks + 1, (ks + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);  // fence: the reads are issued before this k-step's MFMAs
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int im = 0; im < TM; ++im)
#pragma unroll
          for (int in = 0; in < TN; ++in)
            acc[im][in] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[ks & 1][im][j], bf[ks & 1][in][j], acc[im][in], 0, 0, 0);
    }
    __syncthreads();  // tile kt+1 has landed (vmcnt(0)) and every wave is done reading tile kt
    cur ^= 1;
  }
  unsigned long long c1 = 0, r1 = 0;
  if (a.stamps) { c1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime(); }
  if (!SPLITK && hyb_slice >= 0) {
    // raw partial of this K-slice: the split-K epilogue on a view of the remainder rows
    ConvArgs b = a;
    b.out = a.hyb_scratch + ((ptrdiff_t)hyb_slice * (a.M - a.hyb_row0) - a.hyb_row0) * (ptrdiff_t)a.Cout;
    conv_epilogue<BM, BN, EPI_PLAIN, true>(b, acc, smem, tile_m, m0, n0, wm, wn, l31, half, tid);
    return;
  }
  conv_epilogue<BM, BN, EPI, SPLITK>(a, acc, smem, tile_m, m0, n0, wm, wn, l31, half, tid);
  if (a.stamps && tid == 0) {   // in-kernel clock = d(shader cycles) / d(100 MHz ticks) x 100 MHz (MI355X_MICROARCH.md, DVFS item 6)
    unsigned long long* o = a.stamps + 8 * blockIdx.x;
    o[0] = c1 - c0; o[1] = r1 - r0;                      // main loop: cycles, 10-ns ticks
    o[2] = r0; o[3] = r1; o[4] = __builtin_amdgcn_s_memrealtime();  // absolute: loop start, loop end, epilogue end
    o[5] = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 0xf;  // XCC id
    o[6] = t_entry;                                                       // first instruction of the workgroup
    o[7] = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));          // HW_REG_HW_ID (wave, SIMD, CU, SH, SE ids)
  }
#endif
}

// ---------------------------------------------------------------------------
// Variant 4 (round 4): the INFERENCE convolution of the reverse process (diffusion.py:254-276 calls the UNet 1000
// times at n = 16: M = 256 ... 16384 pixels per layer, latency- not throughput-shaped).  64 x 64 tile, four waves of
// one 32 x 32 MFMA tile each, and what variant 3 lacks for this regime:
//   * an NST-stage LDS-DMA ring with ONE counted-vmcnt barrier per K-tile: the tiles of K-steps kt+1 .. kt+NST-2 are
//     in flight while kt is multiplied.  Variant 3 has one tile of lookahead and drains it at every barrier; at
//     sampling sizes only two workgroups share a CU, and the 7x7 / 4x4 / 8x8 layers, whose operands stream from the
//     Infinity Cache, ran at 1.6-2.4 us per K-tile against 0.86 us of matrix time (tools/gpu_wg_lifetime_sampling.py);
//   * TILE-MAJOR weights (tdx_pack_conv3x3_tiled): [Cout/64][K-tile][64 rows][32 floats] with the XOR swizzle of the
//     LDS image already applied, so the B tile of a K-step is ONE contiguous 8 KB piece copied lane-linearly (the
//     K-contiguous training pack hands a K-tile its 64 rows as 128-byte pieces at a 9*Cin*4-byte stride: 64 DRAM pages).
// Raw inputs only (inference tensors are post-activation).  Epilogues are the shared ones (conv_shared.h).
// MEASURED (tools/gpu_infer_layers.py, tools/gpu_ab.py; profiles/r04_infer_layers.txt) and OFF (knob "infer_ring"): the
// thirteen layers of a reverse step in isolation 472 us against 461 for variant 3 at n = 16, 1436 against 1339 at
// n = 64; inside the step 0.588 against 0.563 ms (n = 16) and 1.68 against 1.59 (n = 64).  The premise was wrong: these
// launches do not wait for memory - with the DMA removed altogether they lose 5-10 % of their time, with the MFMAs
// removed 55-60 % (ablation bits) - they are short of WAVES: a 64 KB ring leaves two workgroups per CU where variant
// 3's 32 KB leave four, and one wave of a 64x64 workgroup has 16 dependent MFMAs per barrier with nothing to hide the
// barrier, the LDS round trip and its own DMA issue behind.  Kept with its kernel-level test as the record of that.
template <int EPI, bool SPLITK, int NST>
__global__ void __launch_bounds__(256)
conv3x3_ring64_kernel(ConvArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int BM = 64, BN = 64;
  constexpr int NV = 4;                    // DMA instructions per wave and K-tile (2 x A, 2 x B; 1 KiB each)
  constexpr int STAGE = (BM + BN) * BK;    // floats per stage: A 64 x 32 | B 64 x 32
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int xb = blockIdx.x / (8 * a.tilesN), xr = blockIdx.x % (8 * a.tilesN);
  const int tile_m = xb * 8 + (xr & 7), tile_n = xr >> 3;
  if (tile_m * BM >= a.M) return;  // grid is padded to a multiple of 8 row tiles
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int HW = a.H * a.W;
  const int nk_total = 9 * (a.Cin / BK);

  // DMA maps, A as in variant 3: lane -> row 8*wave + lane/8 of each 32-row group, stored chunk lane%8 = logical chunk
  // (lane%8) ^ ((row >> 1) & 7).  B: the pack is already the LDS image, so the copy is linear.
  const int lrow = wave * 8 + (lane >> 3);
  const int c_log = (lane & 7) ^ ((4 * wave + (lane >> 4)) & 7);
  const int neg = (a.W + 1) * a.Cin;
  const auto rsrc_in = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.in) - neg, 0, (int)(((int64_t)a.M * a.Cin + 2 * neg) * 4), 0x00020000);
  const auto rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.Cout * 9 * a.Cin * 4, 0x00020000);
  constexpr unsigned OOB = 0x80000000u;
  unsigned a_off[2], a_taps[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = m0 + lrow + 32 * i;
    unsigned taps = 0;
    if (p < a.M) {
      const int r = p % HW, oh = r / a.W, ow = r % a.W;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int ih = oh + t / 3 - 1, iw = ow + t % 3 - 1;
        if ((unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W) taps |= 1u << t;
      }
    }
    a_taps[i] = taps;
    a_off[i] = (unsigned)(p * a.Cin + c_log * 4) * 4u;
  }
  unsigned w_off[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
    w_off[j] = (unsigned)((tile_n * nk_total * 64 + lrow + 32 * j) * BK + (lane & 7) * 4) * 4u;

  const int x = (l31 >> 1) & 7;
  int frag_pos[BK / 8];
#pragma unroll
  for (int ks = 0; ks < BK / 8; ++ks) frag_pos[ks] = ((2 * ks + half) ^ x) * 4;

  f32x16 acc[1][1];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;

  const int kt0 = SPLITK ? (int)blockIdx.y * a.kt_per_split : 0;
  const int nk = SPLITK ? min(a.kt_per_split, nk_total - kt0) : nk_total;

  // every call issues exactly NV DMA instructions per wave (a request past the last tile repeats it into a stage
  // nobody reads any more), so the vmcnt arithmetic below holds in the tail too
  auto issue = [&](int kt, int st) {
    const int kn = kt0 + min(kt, nk - 1);
    const int cblk = kn / 9, tap = kn - cblk * 9;
    const unsigned soff_in = (unsigned)(((tap / 3) * a.W + (tap % 3)) * a.Cin + cblk * BK) * 4u;
    const unsigned soff_w = (unsigned)kn * (unsigned)(BN * BK * 4);
    float* Ab = smem + st * STAGE + wave * 8 * BK;
    float* Bb = Ab + BM * BK;
#pragma unroll
    for (int j = 0; j < 2; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (lds_ptr_t)(Bb + j * 32 * BK), 16, w_off[j], soff_w, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bool ok = (a_taps[i] >> tap) & 1u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_in, (lds_ptr_t)(Ab + i * 32 * BK), 16, ok ? a_off[i] : OOB, soff_in, 0, 0);
    }
  };

#pragma unroll
  for (int s2 = 0; s2 < NST - 1; ++s2) issue(s2, s2);
  int st = 0;   // stage of tile kt
  f32x4 af[2] = {}, bf[2] = {};
  for (int kt = 0; kt < nk; ++kt) {
    // this wave's pieces of tile kt have landed when only the NV * (NST - 2) requests of the younger tiles are
    // outstanding; the barrier says the same of every wave - and that all of them are done reading tile kt - 1,
    // whose stage the request issued next overwrites
    // (a.dbg: ablation bits for tools/gpu_infer_layers.py --ablate, WRONG results: 1 no barrier, 4 no DMA, 16 no MFMA, 32 no LDS reads)
    if (!(a.dbg & 1)) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(NV * (NST - 2)) : "memory");
    int stn = st + NST - 1; stn = stn >= NST ? stn - NST : stn;
    if (!(a.dbg & 4)) issue(kt + NST - 1, stn);
    __builtin_amdgcn_sched_barrier(0);
    const float* Ab = smem + st * STAGE + (wm * 32 + l31) * BK;
    const float* Bb = smem + st * STAGE + BM * BK + (wn * 32 + l31) * BK;
    if (!(a.dbg & 32)) {
      af[0] = *reinterpret_cast<const f32x4*>(Ab + frag_pos[0]);
      bf[0] = *reinterpret_cast<const f32x4*>(Bb + frag_pos[0]);
    }
#pragma unroll
    for (int ks = 0; ks < BK / 8; ++ks) {
      if (ks + 1 < BK / 8) {
        if (!(a.dbg & 32)) {
          af[(ks + 1) & 1] = *reinterpret_cast<const f32x4*>(Ab + frag_pos[ks + 1]);
          bf[(ks + 1) & 1] = *reinterpret_cast<const f32x4*>(Bb + frag_pos[ks + 1]);
        }
        __builtin_amdgcn_sched_barrier(0);  // the reads of k-step ks+1 are issued before this k-step's MFMAs
      }
      if (!(a.dbg & 16)) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[ks & 1][j], bf[ks & 1][j], acc[0][0], 0, 0, 0);
      }
    }
    st = st + 1 == NST ? 0 : st + 1;
  }
  // the tail requests are still in flight towards LDS: drain them before an epilogue re-uses the tile buffers
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  conv_epilogue<BM, BN, EPI, SPLITK>(a, acc, smem, tile_m, m0, n0, wm, wn, l31, half, tid);
#endif
}

// out[p][c] = epi(bias[c] + sum_s partial[s][p][c]); fixed summation order (deterministic)
template <bool BNRELU>
__global__ void splitk_reduce_kernel(const float* __restrict__ partial, int splits, int64_t n4,
                                     int cout, const float* __restrict__ bias,
                                     const float* __restrict__ scale, const float* __restrict__ shift,
                                     float* __restrict__ out) {
  const int c4n = cout / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % c4n) * 4;
    float4 acc = bias ? *reinterpret_cast<const float4*>(bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < splits; ++s) {
      const float4 v = reinterpret_cast<const float4*>(partial)[(int64_t)s * n4 + i];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    if (BNRELU) {
      const float4 sc = *reinterpret_cast<const float4*>(scale + c);
      const float4 sh = *reinterpret_cast<const float4*>(shift + c);
      acc.x = fmaxf(fmaf(acc.x, sc.x, sh.x), 0.f);
      acc.y = fmaxf(fmaf(acc.y, sc.y, sh.y), 0.f);
      acc.z = fmaxf(fmaf(acc.z, sc.z, sh.z), 0.f);
      acc.w = fmaxf(fmaf(acc.w, sc.w, sh.w), 0.f);
    }
    reinterpret_cast<float4*>(out)[i] = acc;
  }
}

// The inference reduction with the 2x2 ceil-mode max-pool that follows the unit folded in (sampling: one launch
// fewer per encoder level): a thread owns one pooled position x 4 channels, reduces the (up to) four pixels of its
// window in the fixed split order, writes each (the skip connection reads the unpooled tensor) and their maximum.
__global__ void splitk_reduce_pool_kernel(const float* __restrict__ partial, int splits, size_t slab, int B, int H,
                                          int W, int cout, const float* __restrict__ bias,
                                          const float* __restrict__ scale, const float* __restrict__ shift,
                                          float* __restrict__ out, float* __restrict__ pooled) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, c4n = cout / 4;
  const int64_t n = (int64_t)B * Ho * Wo * c4n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % c4n) * 4;
    int64_t p = i / c4n;
    const int ow = (int)(p % Wo); p /= Wo;
    const int oh = (int)(p % Ho);
    const int b = (int)(p / Ho);
    const float4 bv = bias ? *reinterpret_cast<const float4*>(bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 sc = *reinterpret_cast<const float4*>(scale + c);
    const float4 sh = *reinterpret_cast<const float4*>(shift + c);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ih = 2 * oh + (k >> 1), iw = 2 * ow + (k & 1);
      if (ih < H && iw < W) {
        const size_t off = (((size_t)b * H + ih) * W + iw) * cout + c;
        float4 acc = bv;
        for (int sp = 0; sp < splits; ++sp) {
          const float4 v = *reinterpret_cast<const float4*>(partial + (size_t)sp * slab + off);
          acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        acc.x = fmaxf(fmaf(acc.x, sc.x, sh.x), 0.f); acc.y = fmaxf(fmaf(acc.y, sc.y, sh.y), 0.f);
        acc.z = fmaxf(fmaf(acc.z, sc.z, sh.z), 0.f); acc.w = fmaxf(fmaf(acc.w, sc.w, sh.w), 0.f);
        *reinterpret_cast<float4*>(out + off) = acc;
        m.x = fmaxf(m.x, acc.x); m.y = fmaxf(m.y, acc.y); m.z = fmaxf(m.z, acc.z); m.w = fmaxf(m.w, acc.w);
      }
    }
    *reinterpret_cast<float4*>(pooled + i * 4) = m;
  }
}

// Training form of the reduction: out = bias + sum_s partial[s] (fixed order) AND the BatchNorm
// statistics partials the convolution epilogue would have written - per tile of TILE_ROWS pixels and per
// channel the sum and the sum of squared deviations from the TILE mean - so that bn_finalize sees the
// same [tiles][2][cout] layout whether K was split or not.  grid (row tiles, cout/64); a thread holds
// TILE_ROWS/16 rows x 4 columns of the tile in registers for the second (centred) pass.
template <int TILE_ROWS>
__global__ void __launch_bounds__(256)
splitk_reduce_stats_kernel(const float* __restrict__ partial, int splits, int M, int cout,
                           const float* __restrict__ bias, float* __restrict__ out, float* __restrict__ stats,
                           int row0) {
  // row0 > 0 (hybrid launch): only rows [row0, M) were split; partial holds [splits][M - row0][cout]
  constexpr int RJ = TILE_ROWS / 16;
  __shared__ float red[16][64];
  __shared__ float tsum[64];
  const int c4 = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int n0 = blockIdx.y * 64, col = n0 + c4 * 4;
  const int m0 = row0 + blockIdx.x * TILE_ROWS;
  const int rows_valid = min(TILE_ROWS, M - m0);
  const size_t slab = (size_t)(M - row0) * cout;
  const int stile = m0 / TILE_ROWS;
  partial -= (size_t)row0 * cout;
  const float4 bv = bias ? *reinterpret_cast<const float4*>(bias + col) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 v[RJ];
  float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int j = 0; j < RJ; ++j) {
    const int p = m0 + rg + 16 * j;
    v[j] = bv;
    if (p < M) {
      const float* src = partial + (size_t)p * cout + col;
      for (int s = 0; s < splits; ++s) {
        const float4 t = *reinterpret_cast<const float4*>(src + s * slab);
        v[j].x += t.x; v[j].y += t.y; v[j].z += t.z; v[j].w += t.w;
      }
      *reinterpret_cast<float4*>(out + (size_t)p * cout + col) = v[j];
      cs.x += v[j].x; cs.y += v[j].y; cs.z += v[j].z; cs.w += v[j].w;
    }
  }
  *reinterpret_cast<float4*>(&red[rg][c4 * 4]) = cs;
  __syncthreads();
  if (threadIdx.x < 64) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][threadIdx.x];
    tsum[threadIdx.x] = t;
    stats[((size_t)stile * 2 + 0) * cout + n0 + threadIdx.x] = t;
  }
  __syncthreads();
  const float inv_n = 1.0f / (float)rows_valid;
  const float4 mean = make_float4(tsum[c4 * 4] * inv_n, tsum[c4 * 4 + 1] * inv_n, tsum[c4 * 4 + 2] * inv_n,
                                  tsum[c4 * 4 + 3] * inv_n);
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int j = 0; j < RJ; ++j)
    if (m0 + rg + 16 * j < M) {
      const float dx = v[j].x - mean.x, dy = v[j].y - mean.y, dz = v[j].z - mean.z, dw = v[j].w - mean.w;
      q.x = fmaf(dx, dx, q.x); q.y = fmaf(dy, dy, q.y); q.z = fmaf(dz, dz, q.z); q.w = fmaf(dw, dw, q.w);
    }
  *reinterpret_cast<float4*>(&red[rg][c4 * 4]) = q;   // everyone read tsum before the barrier below; red is free
  __syncthreads();
  if (threadIdx.x < 64) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][threadIdx.x];
    stats[((size_t)stile * 2 + 1) * cout + n0 + threadIdx.x] = t;
  }
}

// ------------------------------------------------------------------ dispatch
struct TileCfg {
  int bm, bn;
};

// Workgroups of a kernel that one CU holds: LDS is handed out in 1280-byte granules on gfx950 (160 KB / 128), so
// the 32 KB of a 64x64 tile cost 33,280 bytes and FOUR fit, not the five that 160 / 32 (and
// hipOccupancyMaxActiveBlocksPerMultiprocessor) promise - measured with per-workgroup HW_ID stamps: every CU
// peaks at exactly 4 (tools/gpu_wg_lifetime.py).  48 KB -> 3, 64 KB -> 2.
static int lds_slots_per_cu(int lds_bytes) {
  const int alloc = (lds_bytes + 1279) / 1280 * 1280;
  const int n = 163840 / alloc;
  return n < 1 ? 1 : n > 8 ? 8 : n;
}

#define TDX_CONV_OUT_BNBWD 8   /* internal flag: the epilogue emits BatchNorm-backward partial sums (ConvArgs::bw_*) */

// diagnostics: resident workgroups per CU the runtime computes for the LDS-DMA forward kernel of a tile
// (bm*1000 + bn; training epilogue) and for the weight-gradient kernel (negative argument)
extern "C" int tdx_diag_conv_occupancy(int tile) {
  int n = -1;
  hipError_t e = hipErrorInvalidValue;
#define OCC(K, LDS) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(K), 256, LDS)
  if (tile == 64064) OCC((conv3x3_igemm_dma_kernel<64, 64, EPI_STATS>), (size_t)2 * 128 * BK * 4);
  else if (tile == 128064) OCC((conv3x3_igemm_dma_kernel<128, 64, EPI_STATS>), (size_t)2 * 192 * BK * 4);
  else if (tile == 128128) OCC((conv3x3_igemm_dma_kernel<128, 128, EPI_STATS>), (size_t)2 * 256 * BK * 4);
#undef OCC
  return e == hipSuccess ? n : -(int)e;
}

// Tile choice.  A CU retires tiles one after another at a fixed MFMA rate, so what matters
// after per-tile efficiency (bigger is better: 128x128 runs ~8 % faster than 64x64 on a
// perfectly balanced grid) is how evenly the tiles divide over the 256 CUs: 1568 tiles of
// 128x128 leave 224 CUs idle for the last seventh of the kernel.  Take the largest tile whose
// grid is within 3.5 % of an even split; the smallest tile is the fallback.
static TileCfg pick_tile(int64_t M, int cout) {
  const TileCfg cands[3] = {{128, 128}, {128, 64}, {64, 64}};
  if (g_knobs.conv_tile >= 1 && g_knobs.conv_tile <= 3 && cout % cands[g_knobs.conv_tile - 1].bn == 0)
    return cands[g_knobs.conv_tile - 1];
  for (int i = 0; i < 3; ++i) {
    if (cout % cands[i].bn) continue;
    if (i == 2) return cands[i];
    const int64_t tiles = ((M + cands[i].bm - 1) / cands[i].bm) * (cout / cands[i].bn);
    if (tiles < g_knobs.conv_min_tiles) continue;  // would leave CUs idle (or one lone workgroup per CU): try a smaller tile
    const int64_t rounds = (tiles + 255) / 256;
    if ((double)(rounds * 256) <= 1.035 * (double)tiles) return cands[i];
  }
  return cands[2];
}

// Unsplit launch: a raw input runs on the LDS-DMA kernel, BN+ReLU on load on the register-staging kernel
template <int BM, int BN>
static int launch_conv(const ConvArgs& a_in, int flags, hipStream_t st) {
  const bool in_bn = flags & TDX_CONV_IN_BNRELU;
  ConvArgs a = a_in;
  a.compact = !in_bn && cdiv(a.M, BM) < 64;   // (the LDS-DMA kernel knows the compact order)
  const int grid = a.compact ? cdiv(a.M, BM) * a.tilesN : (cdiv(a.M, BM) + 7) / 8 * 8 * a.tilesN;
  const int epi = (flags & TDX_CONV_OUT_BNRELU) ? EPI_BNRELU
                  : (flags & TDX_CONV_OUT_STATS) ? EPI_STATS
                  : (flags & TDX_CONV_OUT_BNBWD) ? EPI_BNBWD
                                                 : EPI_PLAIN;
  if (epi == EPI_BNBWD && in_bn) return TDX_E_BADARG;  // input-gradient launches read a raw tensor
  if (!in_bn) {
    const size_t lds = (size_t)2 * (BM + BN) * BK * sizeof(float);
    if (epi == EPI_BNRELU) conv3x3_igemm_dma_kernel<BM, BN, EPI_BNRELU><<<grid, 256, lds, st>>>(a);
    else if (epi == EPI_STATS) conv3x3_igemm_dma_kernel<BM, BN, EPI_STATS><<<grid, 256, lds, st>>>(a);
    else if (epi == EPI_BNBWD) conv3x3_igemm_dma_kernel<BM, BN, EPI_BNBWD><<<grid, 256, lds, st>>>(a);
    else conv3x3_igemm_dma_kernel<BM, BN, EPI_PLAIN><<<grid, 256, lds, st>>>(a);
    TDX_CHECK_LAUNCH();
    return 0;
  }
  const size_t lds = (size_t)2 * (BM + BN) * BKP * sizeof(float);
#define TDX_LAUNCH(EPI_)                                                                    \
  do {                                                                                      \
    auto kern = conv3x3_igemm_kernel<BM, BN, EPI_>;                                         \
    static bool attr_set = false;                                                           \
    if (lds > 65536 && !attr_set) {                                                         \
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),               \
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
      if (e != hipSuccess) return (int)e;                                                   \
      attr_set = true;                                                                      \
    }                                                                                       \
    kern<<<grid, 256, lds, st>>>(a);                                                        \
  } while (0)
  if (epi == EPI_BNRELU) TDX_LAUNCH(EPI_BNRELU);
  else if (epi == EPI_STATS) TDX_LAUNCH(EPI_STATS);
  else TDX_LAUNCH(EPI_PLAIN);
#undef TDX_LAUNCH
  TDX_CHECK_LAUNCH();
  return 0;
}

// Split-K plan for latency-bound shapes (small-batch inference): when the 64x64 tile grid
// would occupy fewer than 3/4 of the CUs, split K into S contiguous ranges (>= 6 K-tiles each)
// so that about two workgroups land on every CU - two co-resident workgroups also cover each
// other's barrier and LDS-latency bubbles, which a lone workgroup per CU cannot.
static int plan_splitk(int64_t M, int cin, int cout, int* kt_per_split, size_t cap_floats = (size_t)-1) {
  const TileCfg c = pick_tile(M, cout);
  const int64_t tiles = ((M + c.bm - 1) / c.bm) * (cout / c.bn);
  const int nk = 9 * (cin / BK);
  *kt_per_split = nk;
  if (!g_knobs.splitk || c.bm != 64 || tiles >= g_knobs.splitk_tiles) return 1;
  int s = (int)((g_knobs.splitk_target + tiles - 1) / tiles);
  if (s > nk / 6) s = nk / 6;
  const size_t fit = cap_floats / ((size_t)M * cout);  // never ask for more scratch than there is
  if ((size_t)s > fit) s = (int)fit;
  if (s < 2) return 1;
  const int per = (nk + s - 1) / s;
  *kt_per_split = per;
  return (nk + per - 1) / per;
}

extern "C" size_t tdx_conv3x3_splitk_scratch_floats(int B, int H, int W, int cin, int cout) {
  int per;
  const int64_t M = (int64_t)B * H * W;
  const int s = plan_splitk(M, cin, cout, &per);
  return s > 1 ? (size_t)s * M * cout : 0;
}

// Split-K plan of the TRAINING convolutions (forward with statistics, input gradient).  At B = 256 the
// MNIST bottleneck (512 -> 512 at 4x4: 4096 pixels, K = 4608) gets 256 workgroups of 128x64, one per CU,
// each walking 144 K-tiles whose operands (9.4 MB of weights) miss the L2: 422 us for 19.3 GFLOP, 46 TFLOP/s,
// a third of what the other layers reach - a lone workgroup has nobody to cover the latency of its next
// tile.  Such shapes (the picked tile is not 128x128 and the 64x64 grid is under four workgroups per CU) run
// as 64x64 tiles with K split into ~1536 workgroups, reduced (with the BatchNorm partials) by one more launch.
static int plan_splitk_train(int64_t M, int cin, int cout, int* kt_per_split, size_t cap_floats = (size_t)-1) {
  const TileCfg c = pick_tile(M, cout);
  const int nk = 9 * (cin / BK);
  *kt_per_split = nk;
  if (!g_knobs.splitk_train || (c.bm == 128 && c.bn == 128) || nk < 24) return 1;
  const int64_t t64 = ((M + 63) / 64) * (cout / 64);
  if (t64 >= g_knobs.splitk_train_t64) return 1;
  int s = (int)((g_knobs.splitk_train_target + t64 - 1) / t64);
  if (s > nk / 6) s = nk / 6;
  const size_t fit = cap_floats / ((size_t)M * cout);
  if ((size_t)s > fit) s = (int)fit;
  if (s < 2) return 1;
  const int per = (nk + s - 1) / s;
  *kt_per_split = per;
  return (nk + per - 1) / per;
}

static bool plan_hybrid(int64_t M, int cin, int cout, TileCfg c, struct HybridPlan* h);
static size_t hybrid_scratch_floats(int64_t M, int cin, int cout);
extern "C" size_t tdx_conv3x3_train_scratch_floats(int B, int H, int W, int cin, int cout) {
  int per;
  const int64_t M = (int64_t)B * H * W;
  const int s = plan_splitk_train(M, cin, cout, &per);
  return s > 1 ? (size_t)s * M * cout : hybrid_scratch_floats(M, cin, cout);
}

// the plain split-K reduction: out = bias + sum_s partial[s] over n4 float4s in the fixed order 0..splits-1, then
// relu(. * scale + shift) if BNRELU (scale, shift: null otherwise)
template <bool BNRELU>
static int launch_splitk_reduce(const float* partial, int splits, int64_t n4, int cout, const float* bias,
                                const float* scale, const float* shift, float* out, hipStream_t st) {
  int rg = (int)((n4 + 255) / 256);
  if (rg > 2048) rg = 2048;
  splitk_reduce_kernel<BNRELU><<<rg, 256, 0, st>>>(partial, splits, n4, cout, bias, scale, shift, out);
  TDX_CHECK_LAUNCH();
  return 0;
}

// raw-input (LDS-DMA) 64x64 split-K launch, then the training reduction: statistics in tiles of the rows the
// unsplit kernel would have used (tdx_conv3x3_stat_tile_rows), or the plain sum when stats is null
static int launch_splitk_train(ConvArgs a, int splits, int per, float* scratch, int stat_rows, hipStream_t st) {
  float* final_out = a.out;
  a.out = scratch;
  a.splits = splits;
  a.kt_per_split = per;
  a.tilesN = a.Cout / 64;
  dim3 grid((cdiv(a.M, 64) + 7) / 8 * 8 * a.tilesN, splits);
  conv3x3_igemm_dma_kernel<64, 64, EPI_PLAIN, true><<<grid, 256, (size_t)2 * 128 * BK * sizeof(float), st>>>(a);
  TDX_CHECK_LAUNCH();
  if (a.stats) {
    dim3 rg(cdiv(a.M, stat_rows), a.Cout / 64);
    if (stat_rows == 128)
      splitk_reduce_stats_kernel<128><<<rg, 256, 0, st>>>(scratch, splits, a.M, a.Cout, a.bias, final_out, a.stats, 0);
    else
      splitk_reduce_stats_kernel<64><<<rg, 256, 0, st>>>(scratch, splits, a.M, a.Cout, a.bias, final_out, a.stats, 0);
    TDX_CHECK_LAUNCH();
    return 0;
  }
  return launch_splitk_reduce<false>(scratch, splits, (int64_t)a.M * a.Cout / 4, a.Cout, a.bias, nullptr, nullptr,
                                     final_out, st);
}

// Hybrid launch of a TRAINING convolution whose tiles do not fill a whole number of rounds of the chip's workgroup
// slots (256 CUs x lds_slots_per_cu): 6272 tiles of 64x64 are 6.125 rounds of 1024 slots, 3136 are 3.06, 1568 are
// 1.53 - the encoder layers of the UNet at B = 256 ran at 104-124 TFLOP/s against 128-137 for the decoder layers
// whose grids happen to divide, whatever tile was forced.  The tiles of the whole rounds run as usual; the rest
// (the LAST row tiles) are cut along K into `sp` slices per tile - workgroups 1/sp as long, which the dispatcher
// packs into the slots as they free up - in the SAME launch, and one small launch sums their partials (with the
// BatchNorm partials of those rows, or plainly for the input gradient).  Only the remainder rows pay partial traffic.
struct HybridPlan {
  int full_blocks, sp, per, row0;
  size_t scratch_floats;
};
static bool plan_hybrid(int64_t M, int cin, int cout, TileCfg c, HybridPlan* h) {
  // 64x64 tiles only: measured isolated at B = 256, us: 256->256 @14 484 -> 466, 512->512 @7 504 -> 463, 128->256 @14
  // and 256->512 @7 261 -> 254; the 28x28 layers do not move (530: they are held back by their 103 MB inputs coming
  // from HBM - 460 back to back out of the MALL - not by the 0.125 of a round they spill), and the 128x64-tile
  // decoder layers lose 4-10 % (their last round is two thirds full).  Inside the step the total is unchanged.
  if (!g_knobs.conv_hybrid || c.bm != 64 || c.bn != 64) return false;
  const int64_t tilesM = (M + c.bm - 1) / c.bm, tilesN = cout / c.bn, group = 8 * tilesN;
  const int64_t S = 256 * (int64_t)lds_slots_per_cu(2 * (c.bm + c.bn) * BK * 4);
  const int64_t T = tilesM * tilesN;
  if (T <= S) return false;                       // one (partial) round: the dispatcher has nothing to balance
  const int64_t G_full = (T / S) * S / group;     // whole rounds, in groups of 8 row tiles x all column tiles
  const int64_t rem_row_tiles = tilesM - G_full * 8;
  if (rem_row_tiles <= 0) return false;
  const int64_t Trem = rem_row_tiles * tilesN;
  if (4 * Trem > 3 * S) return false;             // the last round is nearly full as it is
  const int nk = 9 * (cin / BK);
  int best_sp = 0;
  double best = 0.85;                             // fraction of a round the remainder may cost; unsplit it costs ~1
  for (int sp = 2; sp <= 16 && sp <= nk / 4; ++sp) {
    const double cost = (double)((Trem * sp + S - 1) / S) / sp + 0.01 * sp;   // + partial traffic
    if (cost < best) { best = cost; best_sp = sp; }
  }
  if (!best_sp) return false;
  h->per = (nk + best_sp - 1) / best_sp;
  h->sp = (nk + h->per - 1) / h->per;
  h->full_blocks = (int)(G_full * group);
  h->row0 = (int)(G_full * 8 * c.bm);
  h->scratch_floats = (size_t)h->sp * (size_t)(M - h->row0) * cout;
  return true;
}

static size_t hybrid_scratch_floats(int64_t M, int cin, int cout) {
  HybridPlan h;
  return plan_hybrid(M, cin, cout, pick_tile(M, cout), &h) ? h.scratch_floats : 0;
}

template <int BM, int BN>
static int launch_hybrid(ConvArgs a, const HybridPlan& h, float* scratch, bool stats, hipStream_t st) {
  a.hyb_full = h.full_blocks; a.hyb_sp = h.sp; a.hyb_row0 = h.row0; a.hyb_scratch = scratch;
  a.kt_per_split = h.per;
  const int vtot = (cdiv(a.M, BM) + 7) / 8 * 8 * a.tilesN;
  const int grid = h.full_blocks + (vtot - h.full_blocks) * h.sp;
  const size_t lds = (size_t)2 * (BM + BN) * BK * sizeof(float);
  if (stats) conv3x3_igemm_dma_kernel<BM, BN, EPI_STATS><<<grid, 256, lds, st>>>(a);
  else conv3x3_igemm_dma_kernel<BM, BN, EPI_PLAIN><<<grid, 256, lds, st>>>(a);
  TDX_CHECK_LAUNCH();
  const int rem = a.M - h.row0;
  if (stats) {
    dim3 rg(cdiv(rem, BM), a.Cout / 64);
    splitk_reduce_stats_kernel<BM><<<rg, 256, 0, st>>>(scratch, h.sp, a.M, a.Cout, a.bias, a.out, a.stats, h.row0);
    TDX_CHECK_LAUNCH();
    return 0;
  }
  return launch_splitk_reduce<false>(scratch, h.sp, (int64_t)rem * a.Cout / 4, a.Cout, a.bias, nullptr, nullptr,
                                     a.out + (size_t)h.row0 * a.Cout, st);
}

// second half of a split-K inference launch: a.out = the partials [splits][M][Cout]; the reduction in the fixed order
// 0..splits-1 with bias / BN+ReLU - deferred to the consumer, fused with the following max-pool, or plain
template <int EPI_>
static int splitk_finish(const ConvArgs& a, float* final_out, float* scratch, int splits, hipStream_t st,
                         TdxSplitDefer* defer, float* pool_out, bool* pooled) {
  if (EPI_ == EPI_BNRELU && defer && splits <= g_knobs.sample_defer_max) {   // the consumer of this tensor reduces on load (spatial.hip, ResizeSrc)
    *defer = TdxSplitDefer{scratch, splits, (size_t)a.M * a.Cout, a.bias, a.out_scale, a.out_shift};
    return 0;
  }
  if (EPI_ == EPI_BNRELU && pool_out) {
    const int64_t np = (int64_t)a.B * ((a.H + 1) / 2) * ((a.W + 1) / 2) * (a.Cout / 4);
    int pg = (int)((np + 255) / 256);
    if (pg > 2048) pg = 2048;
    splitk_reduce_pool_kernel<<<pg, 256, 0, st>>>(scratch, splits, (size_t)a.M * a.Cout, a.B, a.H, a.W, a.Cout, a.bias,
                                                  a.out_scale, a.out_shift, final_out, pool_out);
    TDX_CHECK_LAUNCH();
    if (pooled) *pooled = true;
    return 0;
  }
  constexpr bool bnrelu = EPI_ == EPI_BNRELU;
  return launch_splitk_reduce<bnrelu>(scratch, splits, (int64_t)a.M * a.Cout / 4, a.Cout, a.bias,
                                      bnrelu ? a.out_scale : nullptr, bnrelu ? a.out_shift : nullptr, final_out, st);
}

// extra operands of the EPI_BNBWD epilogue (tdx_conv3x3_dgrad_bnbwd; host-side only)
struct BwOperands { const float *y, *scale, *shift, *mean, *rstd; float* partial; };

// One direct convolution as its entry point asked for it: the entry points below fill this and nothing else;
// conv3x3_fwd_impl checks it, plans and launches.
struct FwdRequest {
  const float *in, *wpk, *bias;
  float* out;
  int B, H, W, cin, cout, flags;
  const float *in_scale, *in_shift, *out_scale, *out_shift;
  float* stats_partial;
  float* scratch;          // split-K / hybrid partials (null: never split)
  size_t scratch_floats;
  bool train;              // plan as a training convolution (plan_splitk_train, plan_hybrid), not as an inference one
  BwOperands bw;           // TDX_CONV_OUT_BNBWD
  // sampling only: defer the split-K reduction to the consumer / fold the following max-pool into it (internal.h);
  // *pooled is set when pool_out was written
  TdxSplitDefer* defer;
  float* pool_out;
  bool* pooled;
};

template <int EPI_>
static int launch_splitk(ConvArgs a, const FwdRequest& r, int splits, int per, hipStream_t st) {
  const bool in_bn = r.flags & TDX_CONV_IN_BNRELU;
  float* final_out = a.out;
  a.out = r.scratch;
  a.splits = splits;
  a.kt_per_split = per;
  a.compact = !in_bn && cdiv(a.M, 64) < 64;
  dim3 grid(a.compact ? cdiv(a.M, 64) * a.tilesN : (cdiv(a.M, 64) + 7) / 8 * 8 * a.tilesN, splits);
  const size_t lds_dma = (size_t)2 * 128 * BK * sizeof(float);
  if (in_bn)
    conv3x3_igemm2_kernel<64, 64, true, EPI_PLAIN, true><<<grid, 256, (size_t)2 * 128 * BKP * sizeof(float), st>>>(a);
  else conv3x3_igemm_dma_kernel<64, 64, EPI_PLAIN, true><<<grid, 256, lds_dma, st>>>(a);
  TDX_CHECK_LAUNCH();
  return splitk_finish<EPI_>(a, final_out, r.scratch, splits, st, r.defer, r.pool_out, r.pooled);
}

extern "C" int tdx_conv3x3_stat_tiles(int B, int H, int W, int cin, int cout) {
  (void)cin;
  int64_t M = (int64_t)B * H * W;
  return cdiv(M, pick_tile(M, cout).bm);
}

extern "C" int tdx_conv3x3_stat_tile_rows(int B, int H, int W, int cin, int cout) {
  (void)cin;
  return pick_tile((int64_t)B * H * W, cout).bm;
}

// Buffer descriptors address the input with 32-bit byte offsets and use offset 0x80000000 as the
// "outside the image" sentinel that the hardware range check turns into zeros: the padded tensor
// ((W+1) pixels of slack on both sides) must therefore stay below 2 GiB, or padding taps would
// read real memory.  rows x ch floats, slack pixels of ch floats on each side.
static bool descriptor_fits(int64_t rows, int ch, int64_t slack_px) {
  return (rows * ch + 2 * slack_px * ch) * 4 < (1ll << 31);
}

extern "C" int tdx_conv3x3_shape_ok(int B, int H, int W, int cin, int cout) {
  if (B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0) return 0;
  const int64_t M = (int64_t)B * H * W;
  // forward reads (M, cin), dgrad reads (M, cout) through the same kernel; wgrad reads both
  return descriptor_fits(M, cin, W + 1) && descriptor_fits(M, cout, W + 1) &&
         (int64_t)cout * 9 * cin * 4 < (1ll << 31);
}

// diagnostics (knob conv_stamp): where the LDS-DMA forward / dgrad kernels of this launch stamp their main loop, or null
static unsigned long long* pick_stamps(const ConvArgs& a, const float* stats_partial) {
  // 1 = every LDS-DMA forward/dgrad launch stamps; M = only training-forward launches of M pixels;
  // -M = only plain-epilogue (dgrad) launches of M pixels
  const bool stamp = g_knobs.conv_stamp == 1 || (g_knobs.conv_stamp > 1 && g_knobs.conv_stamp == a.M && stats_partial) ||
                     (g_knobs.conv_stamp < 0 && -g_knobs.conv_stamp == a.M && !stats_partial);
  // 2 = every training-forward launch, each into its own region of 8192 workgroup records (a per-process
  // slot counter: the tool resets it with conv_stamp = 0)
  static int slot = 0;
  if (g_knobs.conv_stamp == 0) slot = 0;
  // a workgroup writes one 64-byte record at index blockIdx.x; no launch has more workgroups than 64x64 tiles
  const size_t max_wgs = (size_t)cdiv(a.M, 64) * (size_t)(a.Cout / 64), rec = 8 * sizeof(unsigned long long);
  unsigned long long* stamps = stamp && g_tdx_diag_buffer && max_wgs * rec <= g_tdx_diag_bytes
                                   ? reinterpret_cast<unsigned long long*>(g_tdx_diag_buffer) : nullptr;
  if (g_knobs.conv_stamp == 2 && stats_partial && g_tdx_diag_buffer && slot < 16 && max_wgs <= 8192 &&
      (size_t)(slot + 1) * 8192 * rec <= g_tdx_diag_bytes)
    stamps = reinterpret_cast<unsigned long long*>(g_tdx_diag_buffer) + (size_t)(slot++) * 8 * 8192;
  return stamps;
}

static int conv3x3_fwd_impl(const FwdRequest& r, tdx_stream_t stream) {
  const int B = r.B, H = r.H, W = r.W, cin = r.cin, cout = r.cout, flags = r.flags;
  if (!r.in || !r.wpk || !r.out || B <= 0 || H <= 0 || W <= 0) return TDX_E_BADARG;
  if (cin % BK || cout % 64) return TDX_E_SHAPE;
  if ((flags & TDX_CONV_IN_BNRELU) && (!r.in_scale || !r.in_shift)) return TDX_E_BADARG;
  if ((flags & TDX_CONV_OUT_BNRELU) && (!r.out_scale || !r.out_shift)) return TDX_E_BADARG;
  if ((flags & TDX_CONV_OUT_STATS) && !r.stats_partial) return TDX_E_BADARG;
  if ((flags & TDX_CONV_OUT_STATS) && (flags & TDX_CONV_OUT_BNRELU)) return TDX_E_BADARG;
  int64_t M64 = (int64_t)B * H * W;
  if (M64 >= (1ll << 31)) return TDX_E_SHAPE;
  if (!descriptor_fits(M64, cin, W + 1) || (int64_t)cout * 9 * cin * 4 >= (1ll << 31)) return TDX_E_SHAPE;
  ConvArgs a{};
  a.in = r.in; a.w = r.wpk; a.bias = r.bias; a.out = r.out;
  a.in_scale = r.in_scale; a.in_shift = r.in_shift; a.out_scale = r.out_scale; a.out_shift = r.out_shift;
  a.stats = (flags & TDX_CONV_OUT_STATS) ? r.stats_partial : nullptr;
  if (flags & TDX_CONV_OUT_BNBWD) {
    if (!r.bw.y || !r.bw.partial || (flags & (TDX_CONV_OUT_STATS | TDX_CONV_OUT_BNRELU | TDX_CONV_IN_BNRELU))) return TDX_E_BADARG;
    a.bw_y = r.bw.y; a.bw_scale = r.bw.scale; a.bw_shift = r.bw.shift; a.bw_mean = r.bw.mean; a.bw_rstd = r.bw.rstd;
    a.bw_partial = r.bw.partial;
  }
  a.B = B; a.H = H; a.W = W; a.Cin = cin; a.Cout = cout; a.M = (int)M64;
  TileCfg c = pick_tile(M64, cout);
  a.tilesN = cout / c.bn;
  a.splits = 1;
  a.kt_per_split = 9 * (cin / BK);
  a.dbg = g_knobs.conv_dbg;
  a.stamps = pick_stamps(a, r.stats_partial);
  hipStream_t st = to_stream(stream);
  if (r.train && r.scratch && !(flags & (TDX_CONV_IN_BNRELU | TDX_CONV_OUT_BNRELU))) {
    int per;
    const int splits = plan_splitk_train(M64, cin, cout, &per, r.scratch_floats);
    if (splits > 1) return launch_splitk_train(a, splits, per, r.scratch, c.bm, st);
    HybridPlan h;
    if (plan_hybrid(M64, cin, cout, c, &h) && h.scratch_floats <= r.scratch_floats && !a.stamps) {
      const bool stats = flags & TDX_CONV_OUT_STATS;
      if (c.bm == 128 && c.bn == 128) return launch_hybrid<128, 128>(a, h, r.scratch, stats, st);
      if (c.bm == 128 && c.bn == 64) return launch_hybrid<128, 64>(a, h, r.scratch, stats, st);
      return launch_hybrid<64, 64>(a, h, r.scratch, stats, st);
    }
  } else if (r.scratch && !(flags & TDX_CONV_OUT_STATS)) {
    int per;
    const int splits = plan_splitk(M64, cin, cout, &per, r.scratch_floats);
    if (splits > 1) {
      if (flags & TDX_CONV_OUT_BNRELU) return launch_splitk<EPI_BNRELU>(a, r, splits, per, st);
      return launch_splitk<EPI_PLAIN>(a, r, splits, per, st);
    }
  }
  if (c.bm == 128 && c.bn == 128) return launch_conv<128, 128>(a, flags, st);
  if (c.bm == 128 && c.bn == 64) return launch_conv<128, 64>(a, flags, st);
  return launch_conv<64, 64>(a, flags, st);
}

// the fields every entry point has; the rest of the request stays zero until the entry point sets it
static FwdRequest fwd_request(const float* in, const float* wpk, const float* bias, float* out, int B, int H, int W,
                              int cin, int cout, int flags) {
  FwdRequest r{};
  r.in = in; r.wpk = wpk; r.bias = bias; r.out = out;
  r.B = B; r.H = H; r.W = W; r.cin = cin; r.cout = cout; r.flags = flags;
  return r;
}

extern "C" int tdx_conv3x3_fwd(const float* in, const float* wpk, const float* bias, float* out,
                               int B, int H, int W, int cin, int cout, int flags,
                               const float* in_scale, const float* in_shift,
                               const float* out_scale, const float* out_shift,
                               float* stats_partial, tdx_stream_t stream) {
  FwdRequest r = fwd_request(in, wpk, bias, out, B, H, W, cin, cout, flags);
  r.in_scale = in_scale; r.in_shift = in_shift; r.out_scale = out_scale; r.out_shift = out_shift;
  r.stats_partial = stats_partial;
  return conv3x3_fwd_impl(r, stream);
}

extern "C" int tdx_conv3x3_dgrad(const float* dy, const float* w_dgrad, float* dx, int B, int H, int W,
                                 int cin, int cout, tdx_stream_t stream) {
  // the forward kernel on dy with the mirrored, channel-swapped pack: its "cin" is this layer's cout
  return conv3x3_fwd_impl(fwd_request(dy, w_dgrad, nullptr, dx, B, H, W, cout, cin, 0), stream);
}

// tdx_conv3x3_fwd_splitk for the sampler.  defer != null: a split convolution leaves its raw partial slabs in
// `scratch` and describes them in *defer (TdxSplitDefer) for the kernel that reads the result, which sums them
// (splits == 0 on return: not split or not deferrable, `out` was written as usual).  pool != null: the reduction
// also writes the following 2x2 ceil-mode max-pool to pool->pooled (set to null on return when it did not).
int tdx_conv3x3_fwd_splitk_fused(const float* in, const float* wpk, const float* bias, float* out, int B, int H,
                                 int W, int cin, int cout, int flags, const float* out_scale,
                                 const float* out_shift, float* scratch, size_t scratch_floats, tdx_stream_t stream,
                                 TdxSplitDefer* defer, TdxPoolFuse* pool) {
  if (!scratch) return TDX_E_BADARG;
  if (defer) *defer = TdxSplitDefer{};
  bool pooled = false;
  FwdRequest r = fwd_request(in, wpk, bias, out, B, H, W, cin, cout, flags);
  r.out_scale = out_scale; r.out_shift = out_shift;
  r.scratch = scratch; r.scratch_floats = scratch_floats;
  r.defer = defer;
  r.pool_out = pool ? pool->pooled : nullptr;
  r.pooled = &pooled;
  const int rc = conv3x3_fwd_impl(r, stream);
  if (pool && !pooled) pool->pooled = nullptr;   // not split: the caller runs the pooling kernel
  return rc;
}

extern "C" int tdx_conv3x3_fwd_train(const float* in, const float* wpk, const float* bias, float* out, int B,
                                     int H, int W, int cin, int cout, int flags, float* stats_partial,
                                     float* scratch, size_t scratch_floats, tdx_stream_t stream) {
  if (flags & ~TDX_CONV_OUT_STATS) return TDX_E_BADARG;
  FwdRequest r = fwd_request(in, wpk, bias, out, B, H, W, cin, cout, flags);
  r.stats_partial = stats_partial;
  r.scratch = scratch; r.scratch_floats = scratch_floats;
  r.train = true;
  return conv3x3_fwd_impl(r, stream);
}

// The input gradient of a unit (tdx_conv3x3_fwd_train with flags = 0 on the dgrad pack) whose result is
// dL/d(activation) of the unit below: also emits that unit's BatchNorm-backward partial sums from the epilogue
// (ConvArgs::bw_*).  *nblk = number of partial rows written ([nblk][2][cout], rows of `*tile_rows` pixels), or 0
// when this shape runs on a path without the fused epilogue (split-K: the caller then runs the reduction pass).
int tdx_conv3x3_dgrad_bnbwd(const float* in, const float* wpk, float* out, int B, int H, int W, int cin, int cout,
                            const float* y, const float* scale, const float* shift, const float* mean,
                            const float* rstd, float* partial, int* nblk, float* scratch, size_t scratch_floats,
                            tdx_stream_t stream) {
  *nblk = 0;
  const int64_t M = (int64_t)B * H * W;
  int per;
  FwdRequest r = fwd_request(in, wpk, nullptr, out, B, H, W, cin, cout, 0);
  if (!(g_knobs.bnbwd_fused & 1) || !y || !partial || cin % BK || cout % 64 || M >= (1ll << 31) ||
      plan_splitk_train(M, cin, cout, &per, scratch_floats) > 1 || g_knobs.conv_hybrid) {
    r.scratch = scratch; r.scratch_floats = scratch_floats;
    r.train = true;
    return conv3x3_fwd_impl(r, stream);
  }
  r.flags = TDX_CONV_OUT_BNBWD;
  r.bw = {y, scale, shift, mean, rstd, partial};
  const int rc = conv3x3_fwd_impl(r, stream);
  if (rc) return rc;
  *nblk = cdiv(M, pick_tile(M, cout).bm);
  return 0;
}

extern "C" int tdx_conv3x3_fwd_splitk(const float* in, const float* wpk, const float* bias, float* out,
                                      int B, int H, int W, int cin, int cout, int flags,
                                      const float* in_scale, const float* in_shift,
                                      const float* out_scale, const float* out_shift,
                                      float* scratch, size_t scratch_floats, tdx_stream_t stream) {
  if (!scratch) return TDX_E_BADARG;
  FwdRequest r = fwd_request(in, wpk, bias, out, B, H, W, cin, cout, flags);
  r.in_scale = in_scale; r.in_shift = in_shift; r.out_scale = out_scale; r.out_shift = out_shift;
  r.scratch = scratch; r.scratch_floats = scratch_floats;
  return conv3x3_fwd_impl(r, stream);
}

#define RC_(call) do { int rc__ = (call); if (rc__) return rc__; } while (0)
// ------------------------------------------------------------------ inference (variant 4)
// Split plan of the inference convolution.  A CU retires K-tile units (one K-tile of one 64x64 workgroup) at a fixed
// matrix rate however many workgroups share it, so a launch lasts as long as the busiest CU: with W workgroups of
// u = ceil(nk / s) K-tiles each over C compute units that is ceil(W / C) * (u + ovh) units - ovh = the part of a
// workgroup that is not K loop (ring fill: one Infinity-Cache round trip; epilogue: 16 KB of partials) - plus, when
// K is split at all, the dependent reduction launch (red units).  Pick the split count that minimises it; a split
// keeps at least 6 K-tiles.  (Round 3 aimed every layer at ~512 workgroups: enc1.3 at n = 16 is 392 tiles x 36
// K-tiles - unsplit, 136 CUs carry two tiles and 120 one; cut in three, every CU carries 4 or 5 thirds.)
static int plan_infer(int64_t M, int cin, int cout, int* kt_per_split, size_t cap_floats) {
  const int nk = 9 * (cin / BK);
  const int64_t tiles = ((M + 63) / 64) * (cout / 64);
  *kt_per_split = nk;
  int smax = nk / 6;
  const size_t fit = cap_floats / ((size_t)M * cout);
  if ((size_t)smax > fit) smax = (int)fit;
  if (smax < 2) return 1;
  if (g_knobs.infer_splits > 0) {
    const int sf = g_knobs.infer_splits > smax ? smax : g_knobs.infer_splits;
    if (sf < 2) return 1;
    const int per = (nk + sf - 1) / sf;
    *kt_per_split = per;
    return (nk + per - 1) / per;
  }
  const int C = g_knobs.infer_cus;
  int best_s = 1, best_per = nk;
  int64_t best = ((tiles + C - 1) / C) * (int64_t)(nk + g_knobs.infer_ovh);
  for (int sp = 2; sp <= smax; ++sp) {
    const int per = (nk + sp - 1) / sp;
    const int real = (nk + per - 1) / per;
    if (real != sp) continue;   // the same launch as a smaller sp
    const int64_t cost = ((tiles * real + C - 1) / C) * (int64_t)(per + g_knobs.infer_ovh) + g_knobs.infer_red;
    if (cost < best) { best = cost; best_s = real; best_per = per; }
  }
  *kt_per_split = best_per;
  return best_s;
}

template <int NST>
static int launch_infer(ConvArgs a, int splits, int per, float* scratch, hipStream_t st, TdxSplitDefer* defer,
                        float* pool_out, bool* pooled) {
  const size_t lds = (size_t)NST * 128 * BK * sizeof(float);
  const int gx = (cdiv(a.M, 64) + 7) / 8 * 8 * a.tilesN;
  const bool bnrelu = a.out_scale != nullptr;
#define TDX_INFER_KERNEL(EPI_, SPL_)                                                                        \
  do {                                                                                                      \
    auto kern = conv3x3_ring64_kernel<EPI_, SPL_, NST>;                                                     \
    static bool attr_set = false;                                                                           \
    if (lds > 65536 && !attr_set) {                                                                         \
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                               \
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);             \
      if (e != hipSuccess) return (int)e;                                                                   \
      attr_set = true;                                                                                      \
    }                                                                                                       \
    kern<<<grid, 256, lds, st>>>(a);                                                                        \
  } while (0)
  if (splits > 1) {
    float* final_out = a.out;
    a.out = scratch;
    a.splits = splits;
    a.kt_per_split = per;
    dim3 grid(gx, splits);
    TDX_INFER_KERNEL(EPI_PLAIN, true);
    TDX_CHECK_LAUNCH();
    if (bnrelu) return splitk_finish<EPI_BNRELU>(a, final_out, scratch, splits, st, defer, pool_out, pooled);
    return splitk_finish<EPI_PLAIN>(a, final_out, scratch, splits, st, nullptr, nullptr, nullptr);
  }
  dim3 grid(gx, 1);
  if (bnrelu) TDX_INFER_KERNEL(EPI_BNRELU, false);
  else TDX_INFER_KERNEL(EPI_PLAIN, false);
#undef TDX_INFER_KERNEL
  TDX_CHECK_LAUNCH();
  return 0;
}

// out = [relu(] (conv3x3(in, W) + bias) [* out_scale + out_shift)], W in the TILE-MAJOR pack (tdx_pack_conv3x3_tiled);
// scratch: tdx_conv3x3_infer_scratch_floats(...) floats or more (more lets the plan split further; null: never split)
int tdx_conv3x3_fwd_infer_ex(const float* in, const float* w_tiled, const float* bias, float* out, int B, int H, int W,
                             int cin, int cout, const float* out_scale, const float* out_shift, float* scratch,
                             size_t scratch_floats, tdx_stream_t stream, TdxSplitDefer* defer, TdxPoolFuse* pool) {
  if (defer) *defer = TdxSplitDefer{};
  if (!in || !w_tiled || !out || B <= 0 || H <= 0 || W <= 0) return TDX_E_BADARG;
  if (cin % BK || cout % 64) return TDX_E_SHAPE;
  if ((out_scale == nullptr) != (out_shift == nullptr)) return TDX_E_BADARG;
  const int64_t M64 = (int64_t)B * H * W;
  if (M64 >= (1ll << 31)) return TDX_E_SHAPE;
  if (!descriptor_fits(M64, cin, W + 1) || (int64_t)cout * 9 * cin * 4 >= (1ll << 31)) return TDX_E_SHAPE;
  ConvArgs a{};
  a.in = in; a.w = w_tiled; a.bias = bias; a.out = out;
  a.out_scale = out_scale; a.out_shift = out_shift;
  a.B = B; a.H = H; a.W = W; a.Cin = cin; a.Cout = cout; a.M = (int)M64;
  a.tilesN = cout / 64;
  a.splits = 1;
  a.kt_per_split = 9 * (cin / BK);
  a.dbg = g_knobs.conv_dbg;
  int per = a.kt_per_split;
  const int splits = scratch ? plan_infer(M64, cin, cout, &per, scratch_floats) : 1;
  bool pooled = false;
  float* pool_out = pool ? pool->pooled : nullptr;
  const int rc = g_knobs.infer_stages == 3
                     ? launch_infer<3>(a, splits, per, scratch, to_stream(stream), defer, pool_out, &pooled)
                     : launch_infer<4>(a, splits, per, scratch, to_stream(stream), defer, pool_out, &pooled);
  if (pool && !pooled) pool->pooled = nullptr;   // not split: the caller runs the pooling kernel
  return rc;
}

// The inference convolution on the Winograd kernel (conv3x3_wino.hip): one workgroup = 64 tiles (256 pixels) x 64
// channels and ONE workgroup per CU (it owns the register file), so a reverse step's launches - 8 .. 98 workgroups at
// n = 16 - are cut along the input channels into `splits` ranges until the busiest CU's queue is shortest (same cost
// model as plan_infer, in stages of 8 channels), partials reduced by the shared split-K reduction.
static int plan_wino_infer(int64_t wgs, int ns, int64_t M, int cout, int* per, size_t cap_floats) {
  *per = ns;
  int smax = ns / 2;   // at least two stages per workgroup
  const size_t fit = cap_floats / ((size_t)M * cout);
  if ((size_t)smax > fit) smax = (int)fit;
  const int C = g_knobs.infer_cus;
  int best_s = 1;
  int64_t best = ((wgs + C - 1) / C) * (int64_t)(ns + g_knobs.wino_infer_ovh);
  for (int sp = 2; sp <= smax; ++sp) {
    const int p2 = (ns + sp - 1) / sp, real = (ns + p2 - 1) / p2;
    if (real != sp) continue;
    const int64_t cost = ((wgs * real + C - 1) / C) * (int64_t)(p2 + g_knobs.wino_infer_ovh) + g_knobs.wino_infer_red;
    if (cost < best) { best = cost; best_s = real; *per = p2; }
  }
  return best_s;
}

int tdx_conv3x3_fwd_wino_infer_ex(const float* in, const float* u, const float* bias, float* out, int B, int H, int W,
                                  int cin, int cout, const float* out_scale, const float* out_shift, float* scratch,
                                  size_t scratch_floats, tdx_stream_t stream, TdxSplitDefer* defer, TdxPoolFuse* pool) {
  if (defer) *defer = TdxSplitDefer{};
  if (!out_scale || !out_shift) return TDX_E_BADARG;
  const int64_t M = (int64_t)B * H * W;
  const int64_t wgs = (int64_t)tdx_conv3x3_wino_stat_tiles(B, H, W) * (cout / 64);
  int per = cin / 8;
  const int splits = scratch ? plan_wino_infer(wgs, cin / 8, M, cout, &per, scratch_floats) : 1;
  if (splits <= 1) {
    if (pool) pool->pooled = nullptr;   // not split: the caller runs the pooling kernel
    return tdx_conv3x3_wino_launch(in, u, bias, out, B, H, W, cin, cout, TDX_CONV_OUT_BNRELU, out_scale, out_shift, nullptr,
                                   1, 0, stream);
  }
  RC_(tdx_conv3x3_wino_launch(in, u, nullptr, scratch, B, H, W, cin, cout, 0, nullptr, nullptr, nullptr, splits, per, stream));
  ConvArgs a{};
  a.bias = bias; a.out = scratch; a.out_scale = out_scale; a.out_shift = out_shift;
  a.B = B; a.H = H; a.W = W; a.Cin = cin; a.Cout = cout; a.M = (int)M;
  bool pooled = false;
  const int rc = splitk_finish<EPI_BNRELU>(a, out, scratch, splits, to_stream(stream), defer, pool ? pool->pooled : nullptr, &pooled);
  if (pool && !pooled) pool->pooled = nullptr;
  return rc;
}

extern "C" int tdx_conv3x3_fwd_wino_infer(const float* in, const float* u, const float* bias, float* out, int B, int H,
                                         int W, int cin, int cout, const float* out_scale, const float* out_shift,
                                         float* scratch, size_t scratch_floats, tdx_stream_t stream) {
  return tdx_conv3x3_fwd_wino_infer_ex(in, u, bias, out, B, H, W, cin, cout, out_scale, out_shift, scratch, scratch_floats,
                                       stream, nullptr, nullptr);
}

extern "C" int tdx_conv3x3_fwd_infer(const float* in, const float* w_tiled, const float* bias, float* out, int B, int H,
                                     int W, int cin, int cout, const float* out_scale, const float* out_shift,
                                     float* scratch, size_t scratch_floats, tdx_stream_t stream) {
  return tdx_conv3x3_fwd_infer_ex(in, w_tiled, bias, out, B, H, W, cin, cout, out_scale, out_shift, scratch,
                                  scratch_floats, stream, nullptr, nullptr);
}

extern "C" size_t tdx_conv3x3_infer_scratch_floats(int B, int H, int W, int cin, int cout) {
  int per;
  const int64_t M = (int64_t)B * H * W;
  if (B <= 0 || H <= 0 || W <= 0 || cin % BK || cout % 64) return 0;
  const int s = plan_infer(M, cin, cout, &per, (size_t)-1);
  return s > 1 ? (size_t)s * M * cout : 0;
}

// ---------------------------------------------------------------------- wgrad
// GEMM: rows = output channels, cols = input channels of ONE tap, K = pixels.
// Both operands are k-major in memory ([pixel][channel]), so LDS tiles are
// [32 pixels][channels] and a lane reads TM (TN) adjacent channels of its pixel
// row: MFMA tile `im` then holds channels  base + TM*i + im  (i = MFMA row), a
// permutation that the epilogue undoes.

template <int BM, int BN>
__global__ void __launch_bounds__(256)
conv3x3_wgrad_kernel(WgradArgs a) {
  constexpr int WGM = 2, WGN = 2;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int ACH = BM / 4, BCH = BN / 4;          // float4 chunks per pixel row
  constexpr int AROWS = 256 / ACH, BROWS = 256 / BCH;  // pixel rows per pass
  constexpr int AI = 32 / AROWS, BI = 32 / BROWS;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                // [2][32][BM]
  float* Bs = smem + 2 * 32 * BM;  // [2][32][BN]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int wm = wave / WGN, wn = wave % WGN;

  // Workgroup id -> (group g = (pixel chunk, co tile, ci tile), tap).  The nine taps of a group
  // read the SAME dy chunk and (shifted) input chunk; ids are laid out so that they differ by
  // multiples of 8 inside a block of 72 consecutive ids: the dispatcher deals consecutive ids
  // round-robin over the 8 XCDs, so the nine land on one XCD at about the same time and share
  // its L2 instead of fetching the chunk nine times from HBM (speed only, never correctness).
  const int L = blockIdx.x;
  const int g = (L / 72) * 8 + (L % 8);
  const int tap = (L % 72) / 8;
  if (g >= a.groups) return;
  const int tiles = a.tilesCo * a.tilesCi;
  const int split = g / tiles, tl = g % tiles;
  const int tile_co = tl / a.tilesCi, tile_ci = tl % a.tilesCi;
  const int co0 = tile_co * BM, ci0 = tile_ci * BN;
  const int dh = tap / 3 - 1, dw = tap % 3 - 1;
  const int HW = a.H * a.W;
  const int p_lo = split * a.chunk;
  const int p_hi = min(p_lo + a.chunk, a.M);

  const int a_c4 = (tid % ACH) * 4, a_r0 = tid / ACH;
  const int b_c4 = (tid % BCH) * 4, b_r0 = tid / BCH;
  float4 sc4 = make_float4(1.f, 1.f, 1.f, 1.f), sh4 = make_float4(0.f, 0.f, 0.f, 0.f);
  sc4 = *reinterpret_cast<const float4*>(a.in_scale + ci0 + b_c4);
  sh4 = *reinterpret_cast<const float4*>(a.in_shift + ci0 + b_c4);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int im = 0; im < TM; ++im)
#pragma unroll
    for (int in = 0; in < TN; ++in)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[im][in][r] = 0.f;

  const int nk = (p_hi - p_lo + 31) / 32;

  // Two register stages, like conv3x3_igemm2_kernel: while the 64 MFMAs of pixel-tile k run
  // from LDS[k&1], the registers holding tile k+1 are written to LDS[(k+1)&1] in four slices
  // between the MFMA groups and the loads of tile k+2 are issued into the other stage.
  struct Stage {
    f32x4 ra[AI];
    f32x4 rb[BI];
    unsigned okB;
  };
  Stage S0, S1;
  // Buffer loads (see conv3x3_igemm_kernel): descriptor base in SGPRs + fixed per-thread row
  // offset + per-tile scalar offset.  The dy descriptor ENDS at this workgroup's last pixel, so
  // the ragged end of the pixel range is zero-filled by the hardware range check with no
  // instruction at all; the input descriptor starts (W+1) pixels before the tensor so that the
  // tap shift is a non-negative scalar, and a row whose tap falls outside the image gets an
  // out-of-range offset.
  constexpr unsigned OOB = 0x80000000u;
  const int neg = (a.W + 1) * a.Cin;
  const auto rsrc_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), 0,
                                                         (int)((int64_t)p_hi * a.Cout * 4), 0x00020000);
  // (... and ENDS with the tensor: a valid tap of a pixel < M reads a pixel < M, so nothing legitimate lies behind it, and
  // the rows past M of a ragged last tile - whose taps are judged on (oh, ow) alone - are refused by the range check
  // instead of being read from whatever follows the tensor)
  const auto rsrc_in = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.in) - neg, 0, (int)(((int64_t)a.M * a.Cin + neg) * 4), 0x00020000);
  unsigned a_off[AI], b_off[BI];
#pragma unroll
  for (int i = 0; i < AI; ++i) a_off[i] = (unsigned)((a_r0 + AROWS * i) * a.Cout + co0 + a_c4) * 4u;
#pragma unroll
  for (int i = 0; i < BI; ++i) b_off[i] = (unsigned)((b_r0 + BROWS * i) * a.Cin + ci0 + b_c4) * 4u;
  const unsigned tap_shift = (unsigned)(((tap / 3) * a.W + (tap % 3)) * a.Cin) * 4u;
  // (oh, ow) of each B row this thread stages, advanced by 32 pixels per K-tile with adds and
  // conditional subtracts (load_tile is called for tiles 0, 1, 2, ... in order): on the fp32
  // "matrix" path every VALU instruction competes with the MFMAs for the same SIMD, and two
  // integer divisions per row and tile used to cost ~20 % of the kernel.
  int b_oh[BI], b_ow[BI];
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const int r = (p_lo + b_r0 + BROWS * i) % HW;
    b_oh[i] = r / a.W;
    b_ow[i] = r % a.W;
  }
  int tiles_issued = 0;
  auto load_tile = [&](int kt, Stage& S) {
    const int pbase = p_lo + min(kt, nk - 1) * 32;
    const bool advance = kt > 0 && kt < nk && kt == tiles_issued;  // clamped tail calls re-load the last tile
    if (kt == tiles_issued) ++tiles_issued;
    const unsigned soff_a = (unsigned)pbase * (unsigned)a.Cout * 4u;
    const unsigned soff_b = (unsigned)pbase * (unsigned)a.Cin * 4u + tap_shift;
    unsigned okB = 0;
#pragma unroll
    for (int i = 0; i < AI; ++i)
      S.ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_dy, a_off[i], soff_a, 0));
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      if (advance) {
        int ow = b_ow[i] + a.adv_s, oh = b_oh[i] + a.adv_q;  // 32 = adv_q * W + adv_s
        if (ow >= a.W) { ow -= a.W; oh += 1; }
        if (oh >= 2 * a.H) oh -= 2 * a.H;
        if (oh >= a.H) oh -= a.H;
        b_ow[i] = ow;
        b_oh[i] = oh;
      }
      const int ih = b_oh[i] + dh, iw = b_ow[i] + dw;
      const bool ok = (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
      okB |= ok ? (1u << i) : 0u;
      S.rb[i] = __builtin_bit_cast(
          f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_in, ok ? b_off[i] : OOB, soff_b, 0));
    }
    S.okB = okB;
  };
  auto store_slice = [&](const Stage& S, int buf, int q) {
    float* Ab = As + buf * 32 * BM;
    float* Bb = Bs + buf * 32 * BN;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      if ((i * 4) / AI != q) continue;
      *reinterpret_cast<f32x4*>(Ab + (a_r0 + AROWS * i) * BM + a_c4) = S.ra[i];
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      if ((i * 4) / BI != q) continue;
      f32x4 v = S.rb[i];
      v[0] = fmaxf(fmaf(v[0], sc4.x, sh4.x), 0.f);
      v[1] = fmaxf(fmaf(v[1], sc4.y, sh4.y), 0.f);
      v[2] = fmaxf(fmaf(v[2], sc4.z, sh4.z), 0.f);
      v[3] = fmaxf(fmaf(v[3], sc4.w, sh4.w), 0.f);
      if (!((S.okB >> i) & 1u)) v = f32x4{0.f, 0.f, 0.f, 0.f};  // padding stays 0 after the transform
      *reinterpret_cast<f32x4*>(Bb + (b_r0 + BROWS * i) * BN + b_c4) = v;
    }
  };
  auto mfma_steps = [&](int buf, int ks0) {  // four of the sixteen 2-pixel k-steps
    const float* Ab = As + buf * 32 * BM + half * BM + wm * WTM + TM * l31;
    const float* Bb = Bs + buf * 32 * BN + half * BN + wn * WTN + TN * l31;
#pragma unroll
    for (int ks = ks0; ks < ks0 + 4; ++ks) {
      float af[TM], bf[TN];
      if (TM == 2) {
        float2 v = *reinterpret_cast<const float2*>(Ab + ks * 2 * BM);
        af[0] = v.x; af[TM - 1] = v.y;
      } else {
        af[0] = Ab[ks * 2 * BM];
      }
      if (TN == 2) {
        float2 v = *reinterpret_cast<const float2*>(Bb + ks * 2 * BN);
        bf[0] = v.x; bf[TN - 1] = v.y;
      } else {
        bf[0] = Bb[ks * 2 * BN];
      }
#pragma unroll
      for (int im = 0; im < TM; ++im)
#pragma unroll
        for (int in = 0; in < TN; ++in)
          acc[im][in] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[im], bf[in], acc[im][in], 0, 0, 0);
    }
  };
  auto iteration = [&](int kt, int cur, const Stage& Sst, Stage& Sld) {
    load_tile(kt + 2, Sld);
    __builtin_amdgcn_sched_barrier(0);  // keep the loads at the top (see conv3x3_igemm2_kernel)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      mfma_steps(cur, q * 4);
      store_slice(Sst, cur ^ 1, q);
    }
    __syncthreads();
  };

  if (nk > 0) {
    load_tile(0, S0);
#pragma unroll
    for (int q = 0; q < 4; ++q) store_slice(S0, 0, q);
    load_tile(1, S1);
  }
  __syncthreads();
  int kt = 0;
  for (; kt + 1 < nk; kt += 2) {
    iteration(kt, 0, S1, S0);
    iteration(kt + 1, 1, S0, S1);
  }
  if (kt < nk) iteration(kt, 0, S1, S0);

  float* slab = a.slabs + (size_t)split * a.Cout * 9 * a.Cin;
#pragma unroll
  for (int im = 0; im < TM; ++im)
#pragma unroll
    for (int in = 0; in < TN; ++in)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * half;
        const int co = co0 + wm * WTM + TM * i + im;
        const int ci = ci0 + wn * WTN + TN * l31 + in;
        slab[((size_t)co * 9 + tap) * a.Cin + ci] = acc[im][in][r];
      }
}

// wgrad with both operands fetched by LDS-DMA (raw input only).  The [32 pixels][channels]
// tiles are already linear in LDS (a pixel row is 256 or 512 contiguous bytes and the fragment
// reads are lane-contiguous ds_read_b64/b32), so no swizzle is needed: one DMA wave-instruction
// lands 1 KiB = 2 (or 4) whole pixel rows.  Ragged pixel ranges and image borders are zero
// filled by the buffer range check as in conv3x3_wgrad_kernel.
template <int BM, int BN>
__global__ void __launch_bounds__(256)
conv3x3_wgrad_dma_kernel(WgradArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int WGN = 2;
  constexpr int WTM = BM / 2, WTN = BN / 2;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int ACH = BM / 4, BCH = BN / 4;
  constexpr int AROWS = 256 / ACH, BROWS = 256 / BCH;  // pixel rows per pass of the 256 threads
  constexpr int AI = 32 / AROWS, BI = 32 / BROWS;
  typedef __attribute__((address_space(3))) void* lds_ptr_t;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                // [2][32][BM]
  float* Bs = smem + 2 * 32 * BM;  // [2][32][BN]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int wm = wave / WGN, wn = wave % WGN;

  const int L = blockIdx.x;
  const int g = (L / 72) * 8 + (L % 8);
  const int tap = (L % 72) / 8;
  if (g >= a.groups) return;
  const int tiles = a.tilesCo * a.tilesCi;
  const int split = g / tiles, tl = g % tiles;
  const int tile_co = tl / a.tilesCi, tile_ci = tl % a.tilesCi;
  const int co0 = tile_co * BM, ci0 = tile_ci * BN;
  const int dh = tap / 3 - 1, dw = tap % 3 - 1;
  const int HW = a.H * a.W;
  const int p_lo = split * a.chunk;
  const int p_hi = min(p_lo + a.chunk, a.M);
  const int nk = (p_hi - p_lo + 31) / 32;

  const int a_c4 = (tid % ACH) * 4, a_r0 = tid / ACH;
  const int b_c4 = (tid % BCH) * 4, b_r0 = tid / BCH;
  constexpr unsigned OOB = 0x80000000u;
  const int neg = (a.W + 1) * a.Cin;
  const auto rsrc_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), 0,
                                                         (int)((int64_t)p_hi * a.Cout * 4), 0x00020000);
  // (... and ENDS with the tensor: a valid tap of a pixel < M reads a pixel < M, so nothing legitimate lies behind it, and
  // the rows past M of a ragged last tile - whose taps are judged on (oh, ow) alone - are refused by the range check
  // instead of being read from whatever follows the tensor)
  const auto rsrc_in = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.in) - neg, 0, (int)(((int64_t)a.M * a.Cin + neg) * 4), 0x00020000);
  unsigned a_off[AI], b_off[BI];
#pragma unroll
  for (int i = 0; i < AI; ++i) a_off[i] = (unsigned)((a_r0 + AROWS * i) * a.Cout + co0 + a_c4) * 4u;
#pragma unroll
  for (int i = 0; i < BI; ++i) b_off[i] = (unsigned)((b_r0 + BROWS * i) * a.Cin + ci0 + b_c4) * 4u;
  const unsigned tap_shift = (unsigned)(((tap / 3) * a.W + (tap % 3)) * a.Cin) * 4u;
  int b_oh[BI], b_ow[BI];
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const int r = (p_lo + b_r0 + BROWS * i) % HW;
    b_oh[i] = r / a.W;
    b_ow[i] = r % a.W;
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int im = 0; im < TM; ++im)
#pragma unroll
    for (int in = 0; in < TN; ++in)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[im][in][r] = 0.f;

  // tiles are requested strictly in order 0, 1, 2, ...; `first` skips the coordinate advance
  auto dma_tile = [&](int kt, int buf, bool advance) {
    const int pbase = p_lo + kt * 32;
    const unsigned soff_a = (unsigned)pbase * (unsigned)a.Cout * 4u;
    const unsigned soff_b = (unsigned)pbase * (unsigned)a.Cin * 4u + tap_shift;
    // LDS destination of this wave's instruction i: rows (wave*64/ACH + AROWS*i) .. , lane-linear
    float* Ab = As + buf * 32 * BM + wave * 256;
    float* Bb = Bs + buf * 32 * BN + wave * 256;
#pragma unroll
    for (int i = 0; i < AI; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_dy, (lds_ptr_t)(Ab + i * AROWS * BM), 16, a_off[i], soff_a, 0, 0);
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      if (advance) {
        int ow = b_ow[i] + a.adv_s, oh = b_oh[i] + a.adv_q;
        if (ow >= a.W) { ow -= a.W; oh += 1; }
        if (oh >= 2 * a.H) oh -= 2 * a.H;
        if (oh >= a.H) oh -= a.H;
        b_ow[i] = ow;
        b_oh[i] = oh;
      }
      const int ih = b_oh[i] + dh, iw = b_ow[i] + dw;
      const bool ok = (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_in, (lds_ptr_t)(Bb + i * BROWS * BN), 16,
                                               ok ? b_off[i] : OOB, soff_b, 0, 0);
    }
  };

  // (Round 4: spreading the DMA pieces of tile kt+1 between the k-steps of tile kt, pinned with fences - the issue order
  // that gained 10 % in conv3x3_wino.hip - was measured here and in conv3x3_igemm_dma_kernel and dropped: the step went
  // from 13.10 to 13.66 ms with it in this kernel and did not move with it in the forward kernel.  These kernels run
  // two workgroups per CU; the partner's MFMAs already cover a clump of DMA issue, and the fences cost hipcc its own
  // interleaving of the fragment reads.)
  if (nk > 0) dma_tile(0, 0, false);
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) dma_tile(kt + 1, cur ^ 1, true);
    const float* Ab = As + cur * 32 * BM + half * BM + wm * WTM + TM * l31;
    const float* Bb = Bs + cur * 32 * BN + half * BN + wn * WTN + TN * l31;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      float af[TM], bf[TN];
      if (TM == 2) {
        float2 v = *reinterpret_cast<const float2*>(Ab + ks * 2 * BM);
        af[0] = v.x; af[TM - 1] = v.y;
      } else {
        af[0] = Ab[ks * 2 * BM];
      }
      if (TN == 2) {
        float2 v = *reinterpret_cast<const float2*>(Bb + ks * 2 * BN);
        bf[0] = v.x; bf[TN - 1] = v.y;
      } else {
        bf[0] = Bb[ks * 2 * BN];
      }
#pragma unroll
      for (int im = 0; im < TM; ++im)
#pragma unroll
        for (int in = 0; in < TN; ++in)
          acc[im][in] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[im], bf[in], acc[im][in], 0, 0, 0);
    }
    __syncthreads();
    cur ^= 1;
  }

  float* slab = a.slabs + (size_t)split * a.Cout * 9 * a.Cin;
#pragma unroll
  for (int im = 0; im < TM; ++im)
#pragma unroll
    for (int in = 0; in < TN; ++in)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * half;
        const int co = co0 + wm * WTM + TM * i + im;
        const int ci = ci0 + wn * WTN + TN * l31 + in;
        slab[((size_t)co * 9 + tap) * a.Cin + ci] = acc[im][in][r];
      }
#endif
}

struct WgradCfg {
  int bm, bn, splits, chunk;
};

// Tile and pixel split of the weight gradient (shared with the bf16 kernels: tdx_wgrad_plan)
static WgradCfg pick_wgrad(int64_t M, int cin, int cout, bool bf16 = false) {
  WgradCfg c;
  c.bm = (cout % 128 == 0) ? 128 : 64;
  c.bn = (cin % 128 == 0) ? 128 : 64;
  // Deep layers have many weight tiles but few pixels: 128x128 tiles would need ~15 pixel splits
  // to fill the chip, i.e. 15 partial copies of a 9.4 MB gradient written and re-read by the
  // reduce (140 MB per layer).  64x64 tiles give 4x the workgroups from the weights alone.
  // Not in bf16 mode: there a 64x64 tile (16 FLOP per operand byte from L2) is L2-bound at ~175 TFLOP/s -
  // the four deep layers of the MNIST UNet ran at exactly that - and the bigger tile wins despite the slabs.
  if (!bf16 && g_knobs.wgrad_small && (int64_t)cout * cin >= (1 << 17) && M <= 16384) { c.bm = 64; c.bn = 64; }
  int64_t tiles = (int64_t)(cout / c.bm) * (cin / c.bn) * 9;
  const int target = (c.bm == 128 && c.bn == 128 && g_knobs.wgrad_target_big > 0) ? g_knobs.wgrad_target_big : g_knobs.wgrad_target;
  int64_t s = (target + tiles - 1) / tiles;
  if (!bf16 && c.bm == c.bn) {
    // Both targets are two rounds of the chip's workgroup slots (64x64: 4 per CU, 128x128: 2; lds_slots_per_cu),
    // but rounding the split count UP put most layers a few workgroups ABOVE two rounds (2052 on 1024 slots,
    // 1044 on 512), i.e. into a third round for 4 of them: isolated, 554 -> 463 us (256 -> 256 at 14x14),
    // 744 -> 608 (512 -> 128 at 16x16), 201 -> 165 (128 -> 128 at 16x16).  Round DOWN where the split is fine
    // enough for that to matter.  (Inside the step, where this kernel shares the CUs with the input-gradient
    // GEMM, it is neutral; ONE round - fewest slabs, what a per-layer cost model picks - is 5 % slower there,
    // 16.3 vs 15.6 ms: nothing left to rebalance with.)  Square tiles only.
    const int64_t two_rounds = 2 * 256 * (int64_t)lds_slots_per_cu(2 * 32 * (c.bm + c.bn) * 4);
    if (two_rounds / tiles >= 8) s = two_rounds / tiles;
  }
  // bf16 mode with the nine-tap kernel (64 x 64 tiles, all taps in one workgroup): aim at g_knobs.wgrad9_wgs workgroups
  if (bf16 && g_knobs.wgrad9_wgs > 0) s = g_knobs.wgrad9_wgs / ((int64_t)(cout / 64) * (cin / 64));
  int64_t smax = (M + 255) / 256;
  if (s > smax) s = smax;
  if (s < 1) s = 1;
  int64_t chunk = (M + s - 1) / s;
  chunk = (chunk + 31) / 32 * 32;
  s = (M + chunk - 1) / chunk;
  c.splits = (int)s;
  c.chunk = (int)chunk;
  return c;
}

// which tile a shape resolves to (tests assert that every template is exercised):
// role 0 = forward / dgrad-as-forward (channels as passed to tdx_conv3x3_fwd), 1 = wgrad; bm*1000 + bn
extern "C" int tdx_conv3x3_tile_shape(int B, int H, int W, int cin, int cout, int role) {
  const int64_t M = (int64_t)B * H * W;
  if (role == 1) {
    const WgradCfg c = pick_wgrad(M, cin, cout);
    return c.bm * 1000 + c.bn;
  }
  const TileCfg c = pick_tile(M, cout);
  return c.bm * 1000 + c.bn;
}

// the split plan is shared with the bf16 kernels (same slab layout, same reduce)
void tdx_wgrad_plan(int64_t M, int cin, int cout, int* bm, int* bn, int* splits, int* chunk, bool bf16) {
  const WgradCfg c = pick_wgrad(M, cin, cout, bf16);
  *bm = c.bm; *bn = c.bn; *splits = c.splits; *chunk = c.chunk;
}

extern "C" int tdx_conv3x3_wgrad_splits(int B, int H, int W, int cin, int cout) {
  return pick_wgrad((int64_t)B * H * W, cin, cout).splits;
}
extern "C" int tdx_conv3x3_wgrad_splits_bf16(int B, int H, int W, int cin, int cout) {
  return pick_wgrad((int64_t)B * H * W, cin, cout, true).splits;
}

template <int BM, int BN>
static int launch_wgrad(const WgradArgs& a, int splits, bool in_bn, hipStream_t st) {
  const size_t lds = (size_t)2 * 32 * (BM + BN) * sizeof(float);
  dim3 grid((unsigned)(((int64_t)a.groups + 7) / 8 * 72));
  if (in_bn) conv3x3_wgrad_kernel<BM, BN><<<grid, 256, lds, st>>>(a);
  else conv3x3_wgrad_dma_kernel<BM, BN><<<grid, 256, lds, st>>>(a);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_conv3x3_wgrad(const float* in, const float* dy, float* dw_slabs, int B, int H,
                                 int W, int cin, int cout, int flags, const float* in_scale,
                                 const float* in_shift, tdx_stream_t stream) {
  if (!in || !dy || !dw_slabs || B <= 0 || H <= 0 || W <= 0) return TDX_E_BADARG;
  if (cin % 64 || cout % 64) return TDX_E_SHAPE;
  const bool in_bn = flags & TDX_CONV_IN_BNRELU;
  if (in_bn && (!in_scale || !in_shift)) return TDX_E_BADARG;
  int64_t M64 = (int64_t)B * H * W;
  if (M64 >= (1ll << 31) - 64) return TDX_E_SHAPE;
  if (!descriptor_fits(M64, cin, W + 1) || !descriptor_fits(M64, cout, 0)) return TDX_E_SHAPE;
  WgradCfg c = pick_wgrad(M64, cin, cout);
  WgradArgs a;
  a.in = in; a.dy = dy; a.slabs = dw_slabs; a.in_scale = in_scale; a.in_shift = in_shift;
  a.B = B; a.H = H; a.W = W; a.Cin = cin; a.Cout = cout; a.M = (int)M64;
  a.tilesCi = cin / c.bn; a.tilesCo = cout / c.bm; a.chunk = c.chunk;
  a.groups = a.tilesCi * a.tilesCo * c.splits;
  // 32 pixels further = 32 / W rows and 32 % W columns; only the row modulo H matters (the kernels test the tap's
  // row against the image, nothing else), so the rows are reduced here: oh + adv_q + carry <= 2 H - 1 and the kernels'
  // conditional subtracts suffice for every H x W.  (Unreduced, 32 / W >= 3 H - narrow, short maps such as 4 x 2 or
  // 8 x 1 - left oh >= H and dropped valid taps; maps with H < 4 and W < 32 / (2 H - 1) were refused.)
  a.adv_q = (32 / W) % H; a.adv_s = 32 % W; a.dbg = 0;
  hipStream_t st = to_stream(stream);
  if (c.bm == 128 && c.bn == 128) return launch_wgrad<128, 128>(a, c.splits, in_bn, st);
  if (c.bm == 128 && c.bn == 64) return launch_wgrad<128, 64>(a, c.splits, in_bn, st);
  if (c.bm == 64 && c.bn == 128) return launch_wgrad<64, 128>(a, c.splits, in_bn, st);
  return launch_wgrad<64, 64>(a, c.splits, in_bn, st);
}

// Sum the split-K slabs in a fixed order and write the OIHW gradient
// (cin = channels as stored in the slabs; only the first cin_real of them exist in dw).
// A workgroup owns one output channel and 64 input channels: per slab that is 9 runs of 256 B
// (one per tap), read as float4 by 144 threads; the slabs are dealt round-robin to 4 such thread
// groups (576 threads), so every thread keeps splits/4 independent 16-byte loads in flight and the
// whole chip streams (the first version - one thread per element looping over all slabs, 4-byte
// stores 36 B apart - ran at 1 TB/s: 143 us per call, 1.85 ms per B=256 step).  The four partial
// sums are added in a fixed order in LDS, transposed [tap][ci] -> [ci][tap] there, and written as one
// contiguous 2304-byte run.  Deterministic: no atomics, fixed order.
__global__ void __launch_bounds__(576)
wgrad_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ dw,
                    int splits, int cout, int cin, int cin_real) {
  __shared__ __attribute__((aligned(16))) float red[4][576];
  __shared__ float tr[576];
  const int co = blockIdx.x, ci0 = blockIdx.y * 64;
  const int q = threadIdx.x / 144, j = threadIdx.x % 144;  // slab group, float4 column
  const int tap = j / 16, c4 = (j % 16) * 4;
  const size_t n = (size_t)cout * 9 * cin;
  const float* src = slabs + ((size_t)co * 9 + tap) * cin + ci0 + c4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
  for (int k = q; k < splits; k += 4) {
    const float4 v = *reinterpret_cast<const float4*>(src + (size_t)k * n);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  *reinterpret_cast<float4*>(&red[q][tap * 64 + c4]) = acc;
  __syncthreads();
  {
    const int e = threadIdx.x;  // element (tap, ci) = (e / 64, e % 64)
    const float v = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    tr[(e % 64) * 9 + e / 64] = v;
  }
  __syncthreads();
  const int nci = min(64, cin_real - ci0);  // channels of this block that exist in dw (<= 0: padding only)
  if ((int)threadIdx.x < nci * 9) dw[((size_t)co * cin_real + ci0) * 9 + threadIdx.x] = tr[threadIdx.x];
}

int tdx_conv3x3_wgrad_reduce_pad(const float* dw_slabs, float* dw_oihw, int splits, int cout, int cin,
                                 int cin_real, tdx_stream_t stream) {
  if (!dw_slabs || !dw_oihw || splits <= 0 || cout <= 0 || cin <= 0 || cin_real <= 0 || cin_real > cin)
    return TDX_E_BADARG;
  if (cin % 64) return TDX_E_SHAPE;
  wgrad_reduce_kernel<<<dim3(cout, cin / 64), 576, 0, to_stream(stream)>>>(dw_slabs, dw_oihw, splits, cout, cin,
                                                                           cin_real);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_conv3x3_wgrad_reduce(const float* dw_slabs, float* dw_oihw, int splits, int cout,
                                        int cin, tdx_stream_t stream) {
  return tdx_conv3x3_wgrad_reduce_pad(dw_slabs, dw_oihw, splits, cout, cin, cin, stream);
}

// ----------------------------------------------------------------- packing
// (the packs hold cin channels; channels >= cin_real are zero - a zero-padded input tensor)
__global__ void pack_conv3x3_kernel(const float* __restrict__ w, float* __restrict__ wf,
                                    float* __restrict__ wd, int cout, int cin, int cin_real) {
  const int64_t n = (int64_t)cout * cin * 9;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    // i indexes the forward pack [co][tap][ci] (coalesced writes)
    const int ci = (int)(i % cin);
    const int tap = (int)((i / cin) % 9);
    const int co = (int)(i / ((int64_t)9 * cin));
    const float v = ci < cin_real ? w[((size_t)co * cin_real + ci) * 9 + tap] : 0.f;
    if (wf) wf[i] = v;
    // dgrad pack [ci][8-tap][co]: dIn[p][ci] = sum dy[p + tap'][co] * W[co][ci][flip(tap')]
    if (wd) wd[((size_t)ci * 9 + (8 - tap)) * cout + co] = v;
  }
}

// all 13 units of a network in ONE launch (the weights change every training step, and
// 13 separate 10 us launches were 0.14 ms of a 17.8 ms step); blocks are assigned to units by
// a prefix table of 1024-element chunks
__global__ void pack_conv3x3_batch_kernel(TdxPackBatch b) {
  int u = 0;
  while (u + 1 < b.count && (int)blockIdx.x >= b.chunk_start[u + 1]) ++u;
  const int64_t n = (int64_t)b.cout[u] * b.cin[u] * 9;
  const int cin = b.cin[u], cin_real = b.cin_real[u], cout = b.cout[u];
  const float* __restrict__ w = b.w[u];
  float* __restrict__ wf = b.wf[u];
  float* __restrict__ wd = b.wd[u];
  const int64_t base = (int64_t)(blockIdx.x - b.chunk_start[u]) * 1024;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    if (i >= n) break;
    const int ci = (int)(i % cin);
    const int tap = (int)((i / cin) % 9);
    const int co = (int)(i / ((int64_t)9 * cin));
    const float v = ci < cin_real ? w[((size_t)co * cin_real + ci) * 9 + tap] : 0.f;
    if (wf) wf[i] = v;
    if (wd) wd[((size_t)ci * 9 + (8 - tap)) * cout + co] = v;
  }
}

// Tile-major pack of the inference convolution (conv3x3_ring64_kernel): [cout/64][kn = (ci/32)*9 + tap][64 rows][32 floats],
// and inside a row the eight 16-byte chunks already in their LDS position (position q holds logical chunk
// q ^ ((row >> 1) & 7)): a K-tile's B operand is one contiguous 8 KB piece that the DMA copies lane-linearly.
__device__ __forceinline__ float tiled_pack_value(const float* __restrict__ w, int64_t i, int cin, int cin_real) {
  const int nk = 9 * (cin / 32);
  const int e = (int)(i & 3), q = (int)((i >> 2) & 7), row = (int)((i >> 5) & 63);
  const int64_t t = i >> 11;
  const int kn = (int)(t % nk), blk = (int)(t / nk);
  const int c = q ^ ((row >> 1) & 7);
  const int ci = (kn / 9) * 32 + c * 4 + e, tap = kn % 9, co = blk * 64 + row;
  return ci < cin_real ? w[((size_t)co * cin_real + ci) * 9 + tap] : 0.f;
}

__global__ void pack_conv3x3_tiled_kernel(const float* __restrict__ w, float* __restrict__ wt, int cout, int cin,
                                          int cin_real) {
  const int64_t n = (int64_t)cout * cin * 9;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    wt[i] = tiled_pack_value(w, i, cin, cin_real);
}

__global__ void pack_conv3x3_tiled_batch_kernel(TdxPackBatch b) {
  int u = 0;
  while (u + 1 < b.count && (int)blockIdx.x >= b.chunk_start[u + 1]) ++u;
  const int64_t n = (int64_t)b.cout[u] * b.cin[u] * 9;
  const int64_t base = (int64_t)(blockIdx.x - b.chunk_start[u]) * 1024;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    if (i >= n) break;
    b.wf[u][i] = tiled_pack_value(b.w[u], i, b.cin[u], b.cin_real[u]);
  }
}

// every unit's tile-major pack into wf[] in one launch (wd[] unused)
int tdx_pack_conv3x3_tiled_batch(TdxPackBatch* b, tdx_stream_t stream) {
  if (!b || b->count <= 0 || b->count > TDX_PACK_MAX) return TDX_E_BADARG;
  int chunks = 0;
  for (int u = 0; u < b->count; ++u) {
    if (!b->w[u] || !b->wf[u] || b->cin_real[u] <= 0 || b->cin_real[u] > b->cin[u] || b->cin[u] % 32 || b->cout[u] % 64)
      return TDX_E_BADARG;
    b->chunk_start[u] = chunks;
    chunks += cdiv((int64_t)b->cout[u] * b->cin[u] * 9, 1024);
  }
  pack_conv3x3_tiled_batch_kernel<<<chunks, 256, 0, to_stream(stream)>>>(*b);
  TDX_CHECK_LAUNCH();
  return 0;
}

int tdx_pack_conv3x3_tiled_pad(const float* w_oihw, float* w_tiled, int cout, int cin_real, int cin, tdx_stream_t stream) {
  if (!w_oihw || !w_tiled || cout <= 0 || cin <= 0 || cin_real <= 0 || cin_real > cin) return TDX_E_BADARG;
  if (cin % 32 || cout % 64) return TDX_E_SHAPE;
  const int64_t n = (int64_t)cout * cin * 9;
  int grid = (int)((n + 255) / 256);
  if (grid > 4096) grid = 4096;
  pack_conv3x3_tiled_kernel<<<grid, 256, 0, to_stream(stream)>>>(w_oihw, w_tiled, cout, cin, cin_real);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_pack_conv3x3_tiled(const float* w_oihw, float* w_tiled, int cout, int cin, tdx_stream_t stream) {
  return tdx_pack_conv3x3_tiled_pad(w_oihw, w_tiled, cout, cin, cin, stream);
}

int tdx_pack_conv3x3_batch(TdxPackBatch* b, tdx_stream_t stream) {
  if (!b || b->count <= 0 || b->count > TDX_PACK_MAX) return TDX_E_BADARG;
  int chunks = 0;
  for (int u = 0; u < b->count; ++u) {
    if (!b->w[u] || b->cin_real[u] <= 0 || b->cin_real[u] > b->cin[u]) return TDX_E_BADARG;
    b->chunk_start[u] = chunks;
    chunks += (b->wf[u] || b->wd[u]) ? cdiv((int64_t)b->cout[u] * b->cin[u] * 9, 1024) : 0;
  }
  pack_conv3x3_batch_kernel<<<chunks, 256, 0, to_stream(stream)>>>(*b);
  TDX_CHECK_LAUNCH();
  return 0;
}

int tdx_pack_conv3x3_pad(const float* w_oihw, float* w_fwd, float* w_dgrad, int cout, int cin_real,
                         int cin, tdx_stream_t stream) {
  if (!w_oihw || cout <= 0 || cin <= 0 || cin_real <= 0 || cin_real > cin) return TDX_E_BADARG;
  int64_t n = (int64_t)cout * cin * 9;
  int grid = (int)((n + 255) / 256);
  if (grid > 4096) grid = 4096;
  pack_conv3x3_kernel<<<grid, 256, 0, to_stream(stream)>>>(w_oihw, w_fwd, w_dgrad, cout, cin, cin_real);
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_pack_conv3x3(const float* w_oihw, float* w_fwd, float* w_dgrad, int cout,
                                int cin, tdx_stream_t stream) {
  return tdx_pack_conv3x3_pad(w_oihw, w_fwd, w_dgrad, cout, cin, cin, stream);
}
