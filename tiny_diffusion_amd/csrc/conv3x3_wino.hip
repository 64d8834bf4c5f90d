// 3x3 / pad 1 / stride 1 convolution by Winograd's minimal filtering F(2x2, 3x3) on the fp32 matrix cores of gfx950.
//
// Why (round 4).  On gfx950 the fp32 MFMA (v_mfma_f32_32x32x2_f32) runs at the vector rate - 157 TFLOP/s - and the
// direct implicit GEMM of conv3x3.hip has sat at 0.76 of it for three rounds: the convolutions of the reference's UNet
// (diffusion.py:32-95; >= 99.9 % of its FLOPs) are bound by the matrix pipe itself.  F(2x2, 3x3) computes a 2x2 output
// tile from a 4x4 input patch with 16 multiplications per (input channel, output channel) instead of 36: 2.25x fewer
// matrix cycles for the same result up to fp32 rounding (the transforms are additions and halvings):
//
//     Y = A^T [ (G g G^T) .* (B^T d B) ] A        d: 4x4 input patch, g: 3x3 filter, Y: 2x2 outputs
//     B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]   G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]   A^T = [1 1 1 0; 0 1 -1 -1]
//
// i.e. SIXTEEN independent GEMMs, one per position (xi, nu) of the transformed 4x4: O_p[tile][co] = sum_ci V_p[tile][ci] U_p[co][ci].
//
// Everything is fused into one kernel - a transformed-input tensor in HBM would be 4x the input, and this path is
// worth nothing if it becomes HBM-bound:
//   * a workgroup owns 64 consecutive tiles (256 output pixels) x 64 output channels; four waves, each 32 tiles x 32
//     channels x ALL 16 positions (the inference launches; the training launches split the waves by transform row
//     instead, see the kernel) = sixteen 32x32 accumulators = 256 accumulator registers per lane (one wave per SIMD);
//   * per stage of 8 input channels the raw 4x4 patches of the 64 tiles and the 16 x 64 x 8 transformed weights go
//     global -> LDS by DMA (32 KB + 32 KB, double-buffered), in exactly the order the fragment reads want them
//     ([pixel | position][tile | channel][k-half][4 floats]: every ds_read_b128 of a wave is one contiguous KiB);
//   * each lane transforms the patch of ITS tile in registers (B^T d B on four channels at a time: 128 scalar adds per
//     64 MFMAs, 64 in the row split) - the transformed input never exists in memory;
//   * the weights are transformed once per step by the pack kernel (U = G g G^T, tile-major so that a stage is one
//     contiguous 32 KB piece), for the forward and - flipped and transposed - for the input gradient;
//   * the epilogue applies A^T . A to the sixteen accumulators of a (tile, channel) - lane-local - then bias and the
//     shared epilogues' arithmetic: BatchNorm statistics partials (sum, M2 about the workgroup mean) for training,
//     relu(y * scale + shift) for inference, plain for the input gradient.
// Zero padding and the ragged last workgroup are the buffer range check, as in conv3x3.hip.
#include "internal.h"
#include "conv_shared.h"


constexpr int WT = 64;    // tiles per workgroup
constexpr int WN = 64;    // output channels per workgroup
constexpr int WK = 8;     // input channels per stage
constexpr int A_ST = 16 * WT * WK;   // floats per A stage  [16 px][64 tiles][2][4]
constexpr int B_ST = 16 * WN * WK;   // floats per B stage  [16 pos][64 co][2][4]
constexpr int STAGE = A_ST + B_ST;   // 16384 floats = 64 KB

struct WinoArgs {
  const float* in;
  const float* u;        // [Cout/64][Cin/8][16][64][2][4]
  const float* bias;
  float* out;
  const float* out_scale;
  const float* out_shift;
  float* stats;          // [workgroups along tiles][2][Cout]
  int B, H, W, Cin, Cout, th, tw, NT, tilesN, M;
  float rcp_tpi, rcp_tw; // 1 / (th * tw), 1 / tw: the kernel divides tile indices (< 2^24) by multiplication + one fix-up
  int per;               // SPLITK: stages per split
  int compact;           // workgroup id -> (tile block, channel block) without the XCD grouping (launches of fewer than 64 tile blocks)
  unsigned long long* stamps;  // diagnostics (tools/gpu_wino_phases.py): per workgroup 8 x u64, null in every product launch
};

constexpr int OLD = 68;            // floats per pixel of the epilogue's output image in LDS (64 channels + 4: rows stay 16-byte aligned)
constexpr int TAB_OFF = 2 * STAGE; // floats: behind the two stages, the workgroup's tile table - per tile {byte offset of its first
                                   // output pixel in the NHWC output, validity bits of its four pixels} (built once at kernel start)
constexpr int XREG = 2 * STAGE / 4; // floats of one wave's region of the row split's epilogue exchange (32 KB)
constexpr int XQ = XREG / 4;        // floats of one register quad's part of it: 8 accumulators x 64 lanes x 4
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Shared epilogue: A^T . A on the sixteen accumulators of every (tile, channel) this lane holds, bias, the epilogue's
// arithmetic, the stores, and (EPI_STATS) the BatchNorm partials of the workgroup.
// C/D map of the 32x32 MFMA: column (channel) = l31, row (tile) = (r & 3) + 8 (r >> 2) + 4 half.
// The 256 x 64 outputs go through LDS (the stages are free by now) so that a lane stores 16 bytes of one pixel's channels
// and a wave instruction four whole 256-byte rows: 16 buffer stores per lane instead of 64 scalar ones, and no integer
// division per accumulator row - measured with the workgroup stamps (tools/gpu_wino_phases.py), the scalar form cost
// 8-9 us of a 31-50 us workgroup.
// XH >= 0 (the row split): this wave holds channel half wn = XH of positions 8 XH .. 8 XH + 7 in acc; the other eight
// positions' registers 4 j .. 4 j + 3 are at xin[(j * 8 + p) * 64] (p = position - 8 (1 - XH)) in LDS - quarter j of
// the wave's own region of the exchange.  They are read four registers at a time (held all at once, they spill), one
// row group ahead: the eight reads of rows 4 j + 4 .. 4 j + 7 fly while rows 4 j .. 4 j + 3 are transformed.  The output
// image does not overlap anybody else's quads: a wave writes its 128 pixels x 32 channels into ITS OWN region -
// rows 4 j .. 4 j + 3 (32 pixels x 32 floats, 4 KB) into the first half of quarter j, which only this wave reads and has
// read by then - so no barrier stands between the row loop and the image; the one barrier in front of the stores
// also publishes the statistics' sums (in the second half of quarter 0).  A store instruction's source - 16 lanes x
// 16 bytes of one pixel - is 128 bytes in each of the two channel halves' regions, an odd and an even pixel row
// together covering the 64 banks once.
// Statistics: sums and counts before the stores' barrier, one barrier behind the means, one behind the M2 partials
// (which have a slot of their own) - two barriers, where the first form had four.
// FULL (statistics only): every tile of the workgroup lies inside the tensor with all four outputs valid (even H and
// W, not the ragged last block).  The validity tests, selections and the count then select the value itself and
// multiply by 1.0f: this copy of the epilogue leaves them out - the same bits from a third fewer instructions, and with
// one wave per SIMD every instruction costs its issue slot.  The kernel picks the copy per workgroup.
template <int EPI, int XH = -1, bool FULL = false>
__device__ __forceinline__ void wino_epilogue(const WinoArgs& a, float* out, const float* bias, f32x16 (&acc)[16], float* smem,
                                              int tblk, int n0, int wm, int wn, int l31, int half, int tid,
                                              const f32x4* xin = nullptr) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned* tab = reinterpret_cast<const unsigned*>(smem + TAB_OFF);
  const int cl = wn * 32 + l31, col = n0 + cl;
  const float bv = bias ? bias[col] : 0.f;
  float osc = 1.f, osh = 0.f;
  if (EPI == EPI_BNRELU) { osc = a.out_scale[col]; osh = a.out_shift[col]; }
  float csum = 0.f, cnt = 0.f;
  constexpr bool RX = XH >= 0;
  float* ot = smem;   // channel split: [256 pixels = 64 tiles x 4][OLD]
  float* own = smem + (RX ? (2 * XH + wm) * XREG : 0);   // row split: this wave's region of the exchange
  // the statistics' scratch, per (tile group, channel): slot 0 the sums, 1 the counts, 2 the M2 - and the 64 means
  auto red = [&](int slot, int g, int c) -> float* {
    return RX ? smem + (2 * (c >> 5) + g) * XREG + XQ / 2 + slot * 32 + (c & 31) : smem + 256 * OLD + (2 * slot + g) * 64 + c;
  };
  float* means = RX ? smem + XQ / 2 + 128 : smem + 256 * OLD + 384;
  // the transformed outputs replace the accumulators of positions 0, 1, 4, 5 (Y00, Y01, Y10, Y11), so that the centred
  // second pass of the statistics can read them again
  f32x4 pv[2][8];
  if (RX) {
#pragma unroll
    for (int p = 0; p < 8; ++p) pv[0][p] = xin[p * 64];
  }
  // Two rows (registers r, r + 1 = tiles tl, tl + 1) at a time, as float pairs: with one wave per SIMD every vector
  // instruction costs its issue slot whatever it computes, and no MFMA runs beside these, so the 24 additions of
  // A^T . A and the bias are packed (v_pk_add_f32: the same IEEE additions in the same order, half the instructions).
  // (The inference epilogue keeps one row at a time, as it was.)
  constexpr int RW = EPI == EPI_BNRELU ? 1 : 2;
  typedef float rowv __attribute__((ext_vector_type(RW)));
#pragma unroll
  for (int r = 0; r < 16; r += RW) {
    if (RX && (r & 3) == 0 && r < 12) {   // the quads of the next four rows fly while these four are transformed
#pragma unroll
      for (int p = 0; p < 8; ++p) pv[((r >> 2) + 1) & 1][p] = xin[(((r >> 2) + 1) * 8 + p) * 64];
    }
    auto M = [&](int p) {
      rowv v;
#pragma unroll
      for (int e = 0; e < RW; ++e) v[e] = RX && (p >> 3) != XH ? pv[(r >> 2) & 1][p & 7][(r & 3) + e] : acc[p][r + e];
      return v;
    };
    rowv s0[4], s1[4], bv2;
#pragma unroll
    for (int e = 0; e < RW; ++e) bv2[e] = bv;
#pragma unroll
    for (int nu = 0; nu < 4; ++nu) {
      s0[nu] = M(0 + nu) + M(4 + nu) + M(8 + nu);
      s1[nu] = M(4 + nu) - M(8 + nu) - M(12 + nu);
    }
    const rowv y2[4] = {s0[0] + s0[1] + s0[2] + bv2, s0[1] - s0[2] - s0[3] + bv2, s1[0] + s1[1] + s1[2] + bv2,
                         s1[1] - s1[2] - s1[3] + bv2};
#pragma unroll
    for (int e = 0; e < RW; ++e) {
      const int re = r + e;
      const int tl = wm * 32 + (re & 3) + 8 * (re >> 2) + 4 * half;
      const unsigned m = FULL ? 15u : tab[2 * tl + 1];
      float y[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float val = y2[q][e];
        if (EPI == EPI_BNRELU) val = fmaxf(fmaf(val, osc, osh), 0.f);
        const bool ok = (m >> q) & 1u;
        // the image serves the stores only, and a pixel that is not valid is never stored: no masking for it
        if (RX) own[(re >> 2) * XQ + (((re & 3) + 4 * half) * 4 + q) * 32 + l31] = val;
        else ot[(tl * 4 + q) * OLD + cl] = val;
        csum += ok ? val : 0.f;
        cnt += ok ? 1.f : 0.f;
        y[q] = ok ? val : 0.f;
      }
      acc[0][re] = y[0]; acc[1][re] = y[1]; acc[4][re] = y[2]; acc[5][re] = y[3];
      if (!FULL) {
        acc[2][re] = (m & 1u) ? 1.f : 0.f;          // validity of the four outputs, for pass two
        acc[3][re] = (m & 2u) ? 1.f : 0.f;
        acc[6][re] = (m & 4u) ? 1.f : 0.f;
        acc[7][re] = (m & 8u) ? 1.f : 0.f;
      }
    }
  }
  if (EPI == EPI_STATS) {   // the wave's sums and counts ride on the barrier the image needs anyway
    const float s = csum + __shfl_xor(csum, 32, 64);
    const float n = cnt + __shfl_xor(cnt, 32, 64);
    if (half == 0) { *red(0, wm, cl) = s; *red(1, wm, cl) = n; }
  }
  __syncthreads();
  {
    const auto rsrc_out = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)((int64_t)a.M * a.Cout * 4), 0x00020000);
    const int c4 = (tid & 15) * 4, q = (tid >> 4) & 3;   // a wave instruction = the four pixels of one tile: tile 4 i + wave, pixel q
    const unsigned qoff = (unsigned)((((q >> 1) * a.W + (q & 1)) * a.Cout + n0 + c4) * 4);
    const uint2* tab2 = reinterpret_cast<const uint2*>(tab);
    // pixel P = (tid >> 4) + 16 i.  Row split: region 2 (c4 >> 5) + (P >> 7), chunk (P & 127) >> 5, row P & 31
    const float* src = RX ? smem + 2 * (c4 >> 5) * XREG + (tid >> 4) * 32 + (c4 & 31) : ot + (tid >> 4) * OLD + c4;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint2 e = tab2[4 * i + (tid >> 6)];
      const unsigned off = ((e.y >> q) & 1u) ? e.x + qoff : 0x80000000u;
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + (RX ? (i >> 3) * XREG + ((i & 7) >> 1) * XQ + (i & 1) * 512 : i * 16 * OLD));
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrc_out, off, 0, 0);
    }
  }
  if (EPI == EPI_STATS) {
    // per workgroup and channel: (sum, M2 about the workgroup mean) - the partials bn_finalize merges with Chan's formula
    if (tid < 64) {
      const float ts = *red(0, 0, tid) + *red(0, 1, tid);
      const float tn = *red(1, 0, tid) + *red(1, 1, tid);
      means[tid] = tn > 0.f ? ts / tn : 0.f;
      a.stats[((size_t)tblk * 2 + 0) * a.Cout + n0 + tid] = ts;
    }
    __syncthreads();
    const float mean = means[cl];
    float q = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float d0 = acc[0][r] - mean, d1 = acc[1][r] - mean, d2 = acc[4][r] - mean, d3 = acc[5][r] - mean;
      if (FULL) {   // (d * 1.0f is d)
        q = fmaf(d0, d0, q); q = fmaf(d1, d1, q); q = fmaf(d2, d2, q); q = fmaf(d3, d3, q);
      } else {
        q = fmaf(d0 * acc[2][r], d0, q); q = fmaf(d1 * acc[3][r], d1, q);
        q = fmaf(d2 * acc[6][r], d2, q); q = fmaf(d3 * acc[7][r], d3, q);
      }
    }
    q += __shfl_xor(q, 32, 64);
    if (half == 0) *red(2, wm, cl) = q;   // (a slot of its own: no barrier between the means' readers and this)
    __syncthreads();
    if (tid < 64) a.stats[((size_t)tblk * 2 + 1) * a.Cout + n0 + tid] = *red(2, 0, tid) + *red(2, 1, tid);
  }
#endif
}

#if defined(__HIP_DEVICE_COMPILE__)
// scalar fp32 adds the compiler can neither pack (v_pk_add_f32 costs more beside MFMAs) nor move across the fences
__device__ __forceinline__ float s_add(float x, float y) { float r; asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y)); return r; }
__device__ __forceinline__ float s_sub(float x, float y) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y)); return r; }
__device__ __forceinline__ f32x4 add4(f32x4 x, f32x4 y) { return f32x4{s_add(x[0], y[0]), s_add(x[1], y[1]), s_add(x[2], y[2]), s_add(x[3], y[3])}; }
__device__ __forceinline__ f32x4 sub4(f32x4 x, f32x4 y) { return f32x4{s_sub(x[0], y[0]), s_sub(x[1], y[1]), s_sub(x[2], y[2]), s_sub(x[3], y[3])}; }
#endif

// The kernel.  Three earlier main loops were measured and removed (profiles/r04_wino_layers_{first,v2,v3}.txt,
// profiles/r04_wino_phases_v3.txt; 13 layers at B = 256, forward / input gradient us): the same stages with the issue
// order left to hipcc - sixteen DMA pieces, the fragment reads and the transform in front of the first MFMA of every
// stage - 3473 / 3597; four-channel stages on a four-deep ring with the next stage's transform under the MFMAs but PACKED
// adds (v_pk_add_f32: +13 cycles each beside MFMAs, MI355X_MICROARCH.md) 3873 / 4023; a hand-pinned order with the stage
// boundary at the barrier and scalar per-lane output stores 3115 / 3249; this one 2647 / 2734 (direct implicit GEMM:
// 4559 / 4634).  The fillers are pinned by sched_barrier fences: every one rides behind a 64-cycle MFMA, scalar adds by
// inline asm (the fp32 MFMA shares the vector pipe: each add still costs ~7 cycles - ablation in DESIGN.md 3.1).
// SPLITK: blockIdx.y takes `per` consecutive stages of the input channels and writes raw partial outputs (the output
// transform is linear) to out + blockIdx.y * M * Cout; bias and epilogue are applied by the split-K reduction of
// conv3x3.hip.  Used by the inference path, whose launches would not fill the chip otherwise.
// n / d for 0 <= n < 2^24 and d > 0 with r = 1.0f / d: the product is within one of the quotient, one fix-up step
__device__ __forceinline__ int div_rcp(int n, int d, float r, int* rem) {
  int q = (int)((float)n * r);
  int m = n - q * d;
  if (m < 0) { --q; m += d; }
  else if (m >= d) { ++q; m -= d; }
  *rem = m;
  return q;
}

// ROWS (training launches, knob wino_rows): the waves split the TRANSFORM ROWS instead of the output channels - see the
// main loop below.
template <int EPI, bool SPLITK, bool ROWS>
__global__ void __launch_bounds__(256)
conv3x3_wino_kernel(WinoArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  static_assert(!ROWS || (!SPLITK && EPI != EPI_BNRELU), "the row split serves the training launches only");
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const unsigned long long t_entry = a.stamps ? __builtin_amdgcn_s_memrealtime() : 0ull;   // diagnostics only
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  // tile group wm (tiles 32 wm .. 32 wm + 31); channel half wn (channel split) or transform rows 2 wn, 2 wn + 1 (ROWS)
  const int wm = ROWS ? wave & 1 : wave >> 1, wn = ROWS ? wave >> 1 : wave & 1;
  // workgroup id -> (tile block, channel block): the channel blocks of one tile block (same input patches) get ids that
  // differ by multiples of 8 inside a group of 8 * tilesN consecutive ids: same XCD, same L2 (as conv3x3.hip)
  const int xb = blockIdx.x / (8 * a.tilesN), xr = blockIdx.x % (8 * a.tilesN);
  // (compact: small launches are NOT padded to groups of 8 tile blocks - ids beyond the last block exit at once, and with
  // fewer than 8 blocks those are whole XCDs: conv_shared.h)
  const int tblk = a.compact ? (int)blockIdx.x / a.tilesN : xb * 8 + (xr & 7);
  const int nblk = a.compact ? (int)blockIdx.x - tblk * a.tilesN : xr >> 3;
  const int T0 = tblk * WT;
  if (T0 >= a.NT) return;
  const int n0 = nblk * WN;
  const int tpi = a.th * a.tw;   // tiles per image

  // ---- Prologue order: the weight pieces of stage 0 depend on nothing but the workgroup's ids, so they are requested
  // first and fly while the tile table and the patch offsets (four divisions and the border tests per lane) are
  // computed; then the patches of stage 0, then the weights of stage 1.  Everything of stage 0 is still requested
  // before anything of stage 1: the counted wait in front of the first barrier keeps its meaning.
  // DMA maps.  B: a stage is 32 contiguous KiB of the pack; this wave copies KiB 8*wave .. 8*wave+7
  const auto rsrc_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, (int)((int64_t)a.M * a.Cin * 4), 0x00020000);
  const auto rsrc_u = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.u), 0, a.Cout * 16 * a.Cin * 4, 0x00020000);
  constexpr unsigned OOB = 0x80000000u;
  const unsigned u_base = (unsigned)(nblk * (a.Cin / WK)) * (unsigned)(B_ST * 4) + (unsigned)(wave * 8 * 1024 + lane * 16);
  unsigned a_off[4][2];

  const int s0 = SPLITK ? (int)blockIdx.y * a.per : 0;                        // first stage of this workgroup
  const int ns = SPLITK ? min(a.per, a.Cin / WK - s0) : a.Cin / WK;             // and how many
  // one DMA piece (1 KiB) of stage k (a request past the end repeats the last stage into the idle buffer) into buffer
  // buf: pieces 0-7 the weights, 8-15 the patches
  auto piece = [&](int i, int buf, int k) {
    const int sc = s0 + (k < ns ? k : ns - 1);
    float* Ab = smem + buf * STAGE;
    float* Bb = Ab + A_ST;
    if (i < 8)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_u, (lds_ptr_t)(Bb + (wave * 8 + i) * 256), 16, u_base + i * 1024,
                                               (unsigned)sc * (unsigned)(B_ST * 4), 0, 0);
    else
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_in, (lds_ptr_t)(Ab + (4 * wave + ((i - 8) >> 1)) * 512 + ((i - 8) & 1) * 256), 16,
                                               a_off[(i - 8) >> 1][(i - 8) & 1], (unsigned)(sc * WK * 4), 0, 0);
  };
  // (Training instantiations only, like the peeled first stage below: the inference instantiations keep the requests
  // behind the arithmetic, as they were.)
  constexpr bool PEEL = !SPLITK && EPI != EPI_BNRELU;
  if (PEEL) {
#pragma unroll
    for (int i = 0; i < 8; ++i) piece(i, 0, 0);
    __builtin_amdgcn_sched_barrier(0);   // (the requests stay in front of the arithmetic below)
  }

  // ---- the tile table of the epilogue (visible after the first barrier below)
  if (tid < WT) {
    const int T = T0 + tid;
    const bool tv = T < a.NT;
    int rem, tx;
    const int b = div_rcp(T, tpi, a.rcp_tpi, &rem);
    const int ty = div_rcp(rem, a.tw, a.rcp_tw, &tx);
    const bool r1 = 2 * ty + 1 < a.H, c1 = 2 * tx + 1 < a.W;
    unsigned* tab = reinterpret_cast<unsigned*>(smem + TAB_OFF);
    tab[2 * tid] = tv ? (unsigned)(((b * a.H + 2 * ty) * a.W + 2 * tx) * a.Cout * 4) : 0u;
    tab[2 * tid + 1] = tv ? (1u | (c1 ? 2u : 0u) | (r1 ? 4u : 0u) | (r1 && c1 ? 8u : 0u)) : 0u;
  }

  // ---- A: instruction (px, g) covers pixel px of the 32 tiles of group g: lane L -> tile g*32 + (L >> 1), k-half L & 1
  // (4 channels); this wave issues px = 4*wave .. 4*wave+3 for both groups - one patch row (px >> 2 == wave): the row
  // test and the row's offset are common to the four.
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int T = T0 + g * 32 + (lane >> 1);
    const bool tv = T < a.NT;
    int rem, tx;
    const int b = div_rcp(T, tpi, a.rcp_tpi, &rem);
    const int ty = div_rcp(rem, a.tw, a.rcp_tw, &tx);
    const int ih = 2 * ty - 1 + wave;
    const bool rok = tv && (unsigned)ih < (unsigned)a.H;
    const int rowpx = (b * a.H + ih) * a.W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int iw = 2 * tx - 1 + j;
      const bool ok = rok && (unsigned)iw < (unsigned)a.W;
      a_off[j][g] = ok ? (unsigned)(((rowpx + iw) * a.Cin + (lane & 1) * 4) * 4) : OOB;
    }
  }

  // Training launches (statistics epilogue, plain input gradient) never zero the 256 accumulator registers: their first
  // stage is a second copy of the stage's code whose first MFMA of every position takes the constant 0 as C (0.43 us
  // of a 23-40 us workgroup: step 9.98 -> 9.87 ms).  The inference launches keep the zeroing: their workgroups run 4-16
  // stages from a cold instruction cache, and the second copy cost a reverse step 8 us at n = 16 and 17 us at n = 64.
  f32x16 acc[16];
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (!PEEL) {
#pragma unroll
    for (int p = 0; p < 16; ++p)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[p][r] = 0.f;
  }

#pragma unroll
  for (int i = PEEL ? 8 : 0; i < 16; ++i) piece(i, 0, 0);   // (PEEL: the weights of stage 0 went out at the top)
  unsigned long long t_issued = 0, t_landed = 0, t_loop = 0, c_loop = 0;
  if constexpr (ROWS) {
    // ---- the row split.  Wave (h, wm) = wave 2 h + wm owns tiles 32 wm .. 32 wm + 31, the positions xi = 2h, 2h+1 (all
    // four nu) and ALL 64 output channels as two 32-wide column blocks: still sixteen 32x32 accumulators, acc[2 pp + c]
    // for local position pp = 4 (xi - 2h) + nu and channel half c.  A lane builds only rows 2h, 2h+1 of B^T d from its
    // patch rows h .. h+2 (12 of the 16 pixel reads) and their columns: 64 scalar adds per 64 MFMAs where the channel
    // split builds all four rows in both waves of a tile group (128).  Every V value feeds two MFMAs (one per channel
    // half), and a stage still reads 16 weight fragments: group g = 2 pp + c of the wave's 16 MFMA groups takes the one
    // at position 8h + pp, channel half c - 256 floats after group g-1's, so the wave's fragments are one contiguous 8 KB.
    // Same operand expressions, lane -> (tile, k) map and k order as the channel split: every accumulator sums the
    // same products in the same order, and the result is bit-identical to it.  The stage keeps that loop's shape - one
    // barrier, at group 12, between MFMAs (12,0) and (12,1); behind it the next stage's patch rows are read and its row
    // 2h transformed in the shadow of groups 12-15 - with the fillers re-placed for the new counts: row 2h+1 of the
    // stage (8 f32x4 operations) in groups 0-3, two per gap, ready for its first use in group 8.
    // Epilogue: A^T . A mixes all four xi rows.  Wave (h, wm) keeps channel half h and hands its 8 accumulators of half
    // 1-h to wave (1-h, wm) through the free ring (32 KB per wave, 128 KB = the two stages: the tile table stays); the
    // shared epilogue then does what wave (wm, wn = h) of the channel split did, with the same arithmetic, reading the
    // received rows from LDS one row group ahead and writing its part of the output image into its own region of the
    // exchange as the quarters empty (XH; the layout and the barriers: above wino_epilogue).  A forward workgroup whose
    // 256 outputs are all valid takes the epilogue's copy without the validity masks (FULL).
    static_assert(4 * 8 * 16 * 64 == 2 * STAGE, "the exchange fills the ring");
#pragma unroll
    for (int i = 0; i < 8; ++i) piece(i, 1, 1);
    if (a.stamps) t_issued = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // stage 0 has landed (loads return in order)
    if (a.stamps) { t_landed = __builtin_amdgcn_s_memrealtime(); c_loop = __builtin_amdgcn_s_memtime(); }
    auto body = [&](auto Hc) {
      constexpr int H = decltype(Hc)::value;
      // d: patch rows H .. H+2 (local rows 0-2) x 4 pixels; v: V rows 2H (0-3) and 2H+1 (4-7); t: one row of B^T d
      f32x4 d[12], v[8], t[4], bq[5], nbq[2];
      const int lofs = wm * 256 + l31 * 8 + half * 4;
      // column c of row 2H + x of B^T d, by the channel split's expressions: d0 - d2, d1 + d2 | d2 - d1, d1 - d3
      auto trow = [&](int x, int c) {
        if (H == 0) t[c] = x == 0 ? sub4(d[c], d[8 + c]) : add4(d[4 + c], d[8 + c]);
        else t[c] = x == 0 ? sub4(d[4 + c], d[c]) : sub4(d[c], d[8 + c]);
      };
      auto vcol = [&](int x, int c) {   // V[2H + x][c] = ((B^T d) B)[.][c]
        f32x4& o = v[4 * x + c];
        if (c == 0) o = sub4(t[0], t[2]);
        else if (c == 1) o = add4(t[1], t[2]);
        else if (c == 2) o = sub4(t[2], t[1]);
        else o = sub4(t[1], t[3]);
      };
      // the local rows that row 2H reads first (0 and 2 | 0 and 1), then the remaining one
      constexpr int RA = 0, RB = H == 0 ? 2 : 1, RC = H == 0 ? 1 : 2;
      {
        const float* Ab = smem + 4 * H * 512 + lofs;
        const float* Bb = smem + A_ST + 8 * H * 512 + l31 * 8 + half * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          d[4 * RA + c] = *reinterpret_cast<const f32x4*>(Ab + (4 * RA + c) * 512);
          d[4 * RB + c] = *reinterpret_cast<const f32x4*>(Ab + (4 * RB + c) * 512);
        }
        nbq[0] = *reinterpret_cast<const f32x4*>(Bb);
        nbq[1] = *reinterpret_cast<const f32x4*>(Bb + 256);
#pragma unroll
        for (int c = 0; c < 4; ++c) d[4 * RC + c] = *reinterpret_cast<const f32x4*>(Ab + (4 * RC + c) * 512);
#pragma unroll
        for (int c = 0; c < 4; ++c) trow(0, c);
#pragma unroll
        for (int c = 0; c < 4; ++c) vcol(0, c);
      }
      auto stage = [&](auto first_c, int s) {
        constexpr bool FIRST = decltype(first_c)::value;
        const int cb = s & 1;
        const float* Bb = smem + cb * STAGE + A_ST + 8 * H * 512 + l31 * 8 + half * 4;   // fragment of group g: Bb + 256 g
        const float* An = smem + (cb ^ 1) * STAGE + 4 * H * 512 + lofs;                 // the next stage's
        const float* Bn = smem + (cb ^ 1) * STAGE + A_ST + 8 * H * 512 + l31 * 8 + half * 4;
        bq[0] = nbq[0]; bq[1] = nbq[1];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int cur = g % 5, pp = g >> 1, ai = 8 * (g & 1) + pp;
          if (FIRST) acc[ai] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[pp][0], bq[cur][0], zero16, 0, 0, 0);
          else acc[ai] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[pp][0], bq[cur][0], acc[ai], 0, 0, 0);
          if (g < 8) piece(8 + g, cb ^ 1, s + 1);
          if (g == 10) bq[4] = *reinterpret_cast<const f32x4*>(Bb + 14 * 256);
          if (g == 11) bq[0] = *reinterpret_cast<const f32x4*>(Bb + 15 * 256);
          if (g == 12) {
            // stage s+1 has landed and every wave is done reading the buffer of stage s
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              d[4 * RA + c] = *reinterpret_cast<const f32x4*>(An + (4 * RA + c) * 512);
              d[4 * RB + c] = *reinterpret_cast<const f32x4*>(An + (4 * RB + c) * 512);
            }
          }
          if (g == 13) {
#pragma unroll
            for (int c = 0; c < 4; ++c) d[4 * RC + c] = *reinterpret_cast<const f32x4*>(An + (4 * RC + c) * 512);
          }
          if (g == 14) {
#pragma unroll
            for (int c = 0; c < 4; ++c) trow(0, c);    // row 2H of the next stage (t is free: row 2H+1 is done)
          }
          if (g == 15) { vcol(0, 2); vcol(0, 3); }
          __builtin_amdgcn_sched_barrier(0);
          acc[ai] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[pp][1], bq[cur][1], acc[ai], 0, 0, 0);
          if (g < 2) { trow(1, 2 * g); trow(1, 2 * g + 1); }          // row 2H+1 of this stage
          else if (g < 4) { vcol(1, 2 * g - 4); vcol(1, 2 * g - 3); }
          else if (g >= 12) piece(2 * (g - 12), cb, s + 2);
          __builtin_amdgcn_sched_barrier(0);
          acc[ai] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[pp][2], bq[cur][2], acc[ai], 0, 0, 0);
          if (g < 12) bq[(g + 2) % 5] = *reinterpret_cast<const f32x4*>(Bb + (g + 2) * 256);
          if (g == 12) { nbq[0] = *reinterpret_cast<const f32x4*>(Bn); nbq[1] = *reinterpret_cast<const f32x4*>(Bn + 256); }
          if (g == 14) { vcol(0, 0); vcol(0, 1); }
          if (g == 15) piece(7, cb, s + 2);
          __builtin_amdgcn_sched_barrier(0);
          acc[ai] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[pp][3], bq[cur][3], acc[ai], 0, 0, 0);
          if (g >= 12 && g < 15) piece(2 * (g - 12) + 1, cb, s + 2);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      stage(std::true_type{}, 0);
      for (int s = 1; s < ns; ++s) stage(std::false_type{}, s);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the requests past the end; the ring is free
      if (a.stamps) { t_loop = __builtin_amdgcn_s_memrealtime(); c_loop = __builtin_amdgcn_s_memtime() - c_loop; }
      // exchange: [receiving wave][register quad][accumulator][lane][4] (16-byte lane runs: conflict-free).  Quad-major:
      // the eight reads of one row group empty one quarter (XQ floats) of the receiver's region, which then takes that
      // group's rows of the output image (see wino_epilogue)
      {
        f32x4* xo = reinterpret_cast<f32x4*>(smem + (2 * (1 - H) + wm) * XREG) + lane;
#pragma unroll
        for (int pp = 0; pp < 8; ++pp)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const f32x16& x = acc[8 * (1 - H) + pp];
            xo[(r4 * 8 + pp) * 64] = f32x4{x[4 * r4], x[4 * r4 + 1], x[4 * r4 + 2], x[4 * r4 + 3]};
          }
      }
      __syncthreads();
      if (EPI == EPI_STATS && !((a.H | a.W) & 1) && T0 + WT <= a.NT)   // all 256 outputs valid: the FULL copy
        wino_epilogue<EPI, H, true>(a, a.out, a.bias, acc, smem, tblk, n0, wm, H, l31, half, tid,
                                    reinterpret_cast<const f32x4*>(smem + wave * XREG) + lane);
      else
        wino_epilogue<EPI, H>(a, a.out, a.bias, acc, smem, tblk, n0, wm, H, l31, half, tid,
                              reinterpret_cast<const f32x4*>(smem + wave * XREG) + lane);
    };
    if (wn) body(std::integral_constant<int, 1>{});
    else body(std::integral_constant<int, 0>{});
  } else {
    f32x4 d[16], v[16], t1[4], t2[4], t3[4];
    // f32x4 operation q (0..23) of the transform behind its first row: rows 1, 2, 3 of t (q % 8 < 4) and of V (q % 8 >= 4)
    auto xop = [&](int q) {
      const int r = q >> 3, k = q & 7, c = k & 3;
      if (k < 4) {
        if (r == 0) t1[c] = add4(d[4 + c], d[8 + c]);
        else if (r == 1) t2[c] = sub4(d[8 + c], d[4 + c]);
        else t3[c] = sub4(d[4 + c], d[12 + c]);
      } else {
        f32x4(&t)[4] = r == 0 ? t1 : r == 1 ? t2 : t3;
        f32x4& o = v[4 * (r + 1) + c];
        if (c == 0) o = sub4(t[0], t[2]);
        else if (c == 1) o = add4(t[1], t[2]);
        else if (c == 2) o = sub4(t[2], t[1]);
        else o = sub4(t[1], t[3]);
      }
    };
    {
      // ---- the stage boundary of the LDS ring sits at position 12 of the MFMA stage.  With the boundary at the barrier
      // the workgroup stamps (tools/gpu_wino_phases.py) put a stage at 2.35-2.7 us against 1.73 us of MFMA issue: after the
      // barrier every wave - alone on its SIMD - read eighteen fragments and transformed a row before its first MFMA, and the
      // last DMA piece of the next stage was requested 256 cycles before the barrier that waited for it.  Here the weight fragments of
      // positions 12-15 are in registers by position 11, so the ONE barrier per stage stands between MFMAs (12,0) and
      // (12,1): behind it the next stage's patch rows and first two weight fragments are read and its first transform row
      // computed in the shadow of positions 12-15, and the buffer just released takes the weights (pieces 0-7) of stage
      // s+2 at once; its patches (pieces 8-15) follow at positions 0-7 of stage s+1 - four positions before the barrier
      // that needs them.
#pragma unroll
      for (int i = 0; i < 8; ++i) piece(i, 1, 1);
      if (a.stamps) t_issued = __builtin_amdgcn_s_memrealtime();
      asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // stage 0 has landed (loads return in order)
      if (a.stamps) { t_landed = __builtin_amdgcn_s_memrealtime(); c_loop = __builtin_amdgcn_s_memtime(); }
      f32x4 bq[5], nbq[2];
      {
        const float* Ab = smem + wm * 256 + l31 * 8 + half * 4;
        const float* Bb = smem + A_ST + wn * 256 + l31 * 8 + half * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) { d[c] = *reinterpret_cast<const f32x4*>(Ab + c * 512); d[8 + c] = *reinterpret_cast<const f32x4*>(Ab + (8 + c) * 512); }
        nbq[0] = *reinterpret_cast<const f32x4*>(Bb);
        nbq[1] = *reinterpret_cast<const f32x4*>(Bb + 512);
#pragma unroll
        for (int c = 0; c < 4; ++c) { d[4 + c] = *reinterpret_cast<const f32x4*>(Ab + (4 + c) * 512); d[12 + c] = *reinterpret_cast<const f32x4*>(Ab + (12 + c) * 512); }
        f32x4 t0[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) t0[c] = sub4(d[c], d[8 + c]);
        v[0] = sub4(t0[0], t0[2]); v[1] = add4(t0[1], t0[2]); v[2] = sub4(t0[2], t0[1]); v[3] = sub4(t0[1], t0[3]);
      }
      auto stage = [&](auto first_c, int s) {
        constexpr bool FIRST = decltype(first_c)::value;
        const int cb = s & 1;
        const float* Bb = smem + cb * STAGE + A_ST + wn * 256 + l31 * 8 + half * 4;
        const float* An = smem + (cb ^ 1) * STAGE + wm * 256 + l31 * 8 + half * 4;     // the next stage's
        const float* Bn = smem + (cb ^ 1) * STAGE + A_ST + wn * 256 + l31 * 8 + half * 4;
        bq[0] = nbq[0]; bq[1] = nbq[1];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < 16; ++p) {
          const int cur = p % 5;
          if (FIRST) acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[p][0], bq[cur][0], zero16, 0, 0, 0);
          else acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[p][0], bq[cur][0], acc[p], 0, 0, 0);
          if (p < 8) piece(8 + p, cb ^ 1, s + 1);
          if (p == 10) bq[4] = *reinterpret_cast<const f32x4*>(Bb + 14 * 512);
          if (p == 11) bq[0] = *reinterpret_cast<const f32x4*>(Bb + 15 * 512);
          if (p == 12) {
            // stage s+1 has landed and every wave is done reading the buffer of stage s
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
            for (int c = 0; c < 4; ++c) { d[c] = *reinterpret_cast<const f32x4*>(An + c * 512); d[8 + c] = *reinterpret_cast<const f32x4*>(An + (8 + c) * 512); }
          }
          if (p == 13) {
#pragma unroll
            for (int c = 0; c < 4; ++c) d[4 + c] = *reinterpret_cast<const f32x4*>(An + (4 + c) * 512);
          }
          if (p == 14) {
#pragma unroll
            for (int c = 0; c < 4; ++c) t1[c] = sub4(d[c], d[8 + c]);    // (t1 is free: the row-0 temporaries of the next stage)
          }
          if (p == 15) { v[2] = sub4(t1[2], t1[1]); v[3] = sub4(t1[1], t1[3]); }
          __builtin_amdgcn_sched_barrier(0);
          acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[p][1], bq[cur][1], acc[p], 0, 0, 0);
          if (p < 12) { xop(2 * p); xop(2 * p + 1); }   // (both in one gap: 2.5 % faster than one per gap)
          else piece(2 * (p - 12), cb, s + 2);
          __builtin_amdgcn_sched_barrier(0);
          acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[p][2], bq[cur][2], acc[p], 0, 0, 0);
          if (p < 12) bq[(p + 2) % 5] = *reinterpret_cast<const f32x4*>(Bb + (p + 2) * 512);
          if (p == 12) { nbq[0] = *reinterpret_cast<const f32x4*>(Bn); nbq[1] = *reinterpret_cast<const f32x4*>(Bn + 512); }
          if (p == 13) {
#pragma unroll
            for (int c = 0; c < 4; ++c) d[12 + c] = *reinterpret_cast<const f32x4*>(An + (12 + c) * 512);
          }
          if (p == 14) { v[0] = sub4(t1[0], t1[2]); v[1] = add4(t1[1], t1[2]); }
          if (p == 15) piece(7, cb, s + 2);
          __builtin_amdgcn_sched_barrier(0);
          acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[p][3], bq[cur][3], acc[p], 0, 0, 0);
          if (p >= 12 && p < 15) piece(2 * (p - 12) + 1, cb, s + 2);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      if (PEEL) stage(std::true_type{}, 0);
      for (int s = PEEL ? 1 : 0; s < ns; ++s) stage(std::false_type{}, s);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the requests past the end; every wave out of the loop
    }
    if (a.stamps) { t_loop = __builtin_amdgcn_s_memrealtime(); c_loop = __builtin_amdgcn_s_memtime() - c_loop; }
    if (SPLITK)   // raw partials: bias and epilogue are the split-K reduction's
      wino_epilogue<EPI_PLAIN>(a, a.out + (size_t)blockIdx.y * (size_t)a.M * a.Cout, nullptr, acc, smem, tblk, n0, wm, wn, l31, half, tid);
    else   // (no FULL copy here: with all sixteen positions in its registers this instantiation spills around the choice)
      wino_epilogue<EPI>(a, a.out, a.bias, acc, smem, tblk, n0, wm, wn, l31, half, tid);
  }
  if (a.stamps && tid == 0) {   // 10-ns ticks: entry, first stage requested, landed, loop end, epilogue end; loop cycles; ids
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the epilogue's stores have left the wave
    unsigned long long* o = a.stamps + 8 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
    o[0] = t_entry; o[1] = t_issued; o[2] = t_landed; o[3] = t_loop; o[4] = __builtin_amdgcn_s_memrealtime();
    o[5] = c_loop;
    o[6] = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));          // HW_REG_HW_ID
    o[7] = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 0xf;    // XCC id
  }
#endif
}

// All units of a network in one launch, forward and input-gradient packs from the same nine loads: a block of 512
// threads owns 64 output channels x 8 input channels, thread (cl, k8).  Flipping the filter swaps rows / columns 0 and 3
// of G g G^T and leaves 1 and 2 in place, so the input-gradient pack is the forward one with positions permuted and
// the channel roles exchanged; both are written as 256-byte runs.
__global__ void __launch_bounds__(512) pack_wino_batch_kernel(TdxWinoPackBatch b) {
  int u = 0;
  while (u + 1 < b.count && (int)blockIdx.x >= b.start[u + 1]) ++u;
  const int cin = b.cin[u], cout = b.cout[u], cin_real = b.cin_real[u];
  const int blk = blockIdx.x - b.start[u];
  const int nkb = cin / 8;
  const int cb = blk / nkb, kb = blk - cb * nkb;
  const int cl = threadIdx.x >> 3, k8 = threadIdx.x & 7;
  const int co = cb * 64 + cl, ci = kb * 8 + k8;
  float g[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) g[tap] = ci < cin_real ? b.w[u][((size_t)co * cin_real + ci) * 9 + tap] : 0.f;
  float gg[4][3], U[16];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    gg[0][c] = g[c];
    gg[1][c] = 0.5f * (g[c] + g[3 + c] + g[6 + c]);
    gg[2][c] = 0.5f * (g[c] - g[3 + c] + g[6 + c]);
    gg[3][c] = g[6 + c];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    U[r * 4 + 0] = gg[r][0];
    U[r * 4 + 1] = 0.5f * (gg[r][0] + gg[r][1] + gg[r][2]);
    U[r * 4 + 2] = 0.5f * (gg[r][0] - gg[r][1] + gg[r][2]);
    U[r * 4 + 3] = gg[r][2];
  }
  if (b.uf[u]) {
    float* dst = b.uf[u] + (((size_t)cb * nkb + kb) * 16) * 512 + cl * 8 + k8;
#pragma unroll
    for (int p = 0; p < 16; ++p) dst[p * 512] = U[p];
  }
  if (b.ud[u]) {   // output channel ci, input channel co; position (xi, nu) <- (sigma xi, sigma nu), sigma = (3, 1, 2, 0)
    float* dst = b.ud[u] + (((size_t)(ci >> 6) * (cout / 8) + (co >> 3)) * 16) * 512 + (ci & 63) * 8 + (co & 7);
    constexpr int ps = 512;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int xi = p >> 2, nu = p & 3;
      const int sx = xi == 0 ? 3 : xi == 3 ? 0 : xi, sn = nu == 0 ? 3 : nu == 3 ? 0 : nu;
      dst[p * ps] = U[sx * 4 + sn];
    }
  }
}

static int wino_tile_rows(int H, int W) {   // output pixels per workgroup (uniform over workgroups), or 0: unsupported geometry
  const int th = (H + 1) / 2, tw = (W + 1) / 2;
  if (!(H & 1) && !(W & 1)) return 4 * WT;
  if (WT % (th * tw) == 0) return (WT / (th * tw)) * H * W;   // whole images per workgroup
  return 0;
}

// 1 when the Winograd kernel serves this shape (else the caller uses the direct kernels of conv3x3.hip)
extern "C" int tdx_conv3x3_wino_ok(int B, int H, int W, int cin, int cout) {
  if (B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || cin % WK || cout % WN) return 0;
  if (!wino_tile_rows(H, W)) return 0;
  const int64_t M = (int64_t)B * H * W;
  // (tile indices < 2^24: the kernel divides them in fp32, div_rcp)
  return M * cin * 4 < (1ll << 31) && M * cout * 4 < (1ll << 31) && (int64_t)cout * 16 * cin * 4 < (1ll << 31) &&
         (int64_t)B * ((H + 1) / 2) * ((W + 1) / 2) + 64 < (1ll << 24);
}

extern "C" int tdx_conv3x3_wino_stat_tile_rows(int B, int H, int W) { (void)B; return wino_tile_rows(H, W); }
extern "C" int tdx_conv3x3_wino_stat_tiles(int B, int H, int W) {
  const int th = (H + 1) / 2, tw = (W + 1) / 2;
  return cdiv((int64_t)B * th * tw, WT);
}

// OIHW (cout, cin_real, 3, 3) -> transformed packs of cout x cin channels (channels >= cin_real are zero): u_fwd for the
// forward, u_dgrad (cin x cout roles swapped, taps mirrored) for the input gradient; either may be null.
// Each holds cout * cin * 16 floats.
int tdx_pack_conv3x3_wino_pad(const float* w_oihw, float* u_fwd, float* u_dgrad, int cout, int cin_real, int cin,
                              tdx_stream_t stream);

int tdx_pack_conv3x3_wino_batch(TdxWinoPackBatch* b, tdx_stream_t stream) {
  if (!b || b->count <= 0 || b->count > TDX_PACK_MAX) return TDX_E_BADARG;
  int blocks = 0;
  for (int u = 0; u < b->count; ++u) {
    if (!b->w[u] || b->cin_real[u] <= 0 || b->cin_real[u] > b->cin[u] || b->cin[u] % 64 || b->cout[u] % 64) return TDX_E_BADARG;
    b->start[u] = blocks;
    blocks += (b->cin[u] / 8) * (b->cout[u] / 64);
  }
  pack_wino_batch_kernel<<<blocks, 512, 0, to_stream(stream)>>>(*b);
  TDX_CHECK_LAUNCH();
  return 0;
}

int tdx_pack_conv3x3_wino_pad(const float* w_oihw, float* u_fwd, float* u_dgrad, int cout, int cin_real, int cin,
                              tdx_stream_t stream) {
  if (!w_oihw || cout <= 0 || cin <= 0 || cin_real <= 0 || cin_real > cin) return TDX_E_BADARG;
  if (cin % 64 || cout % 64) return TDX_E_SHAPE;
  if (!u_fwd && !u_dgrad) return 0;
  TdxWinoPackBatch b{};
  b.count = 1;
  b.w[0] = w_oihw; b.uf[0] = u_fwd; b.ud[0] = u_dgrad; b.cout[0] = cout; b.cin[0] = cin; b.cin_real[0] = cin_real;
  return tdx_pack_conv3x3_wino_batch(&b, stream);
}

extern "C" int tdx_pack_conv3x3_wino(const float* w_oihw, float* u_fwd, float* u_dgrad, int cout, int cin,
                                     tdx_stream_t stream) {
  return tdx_pack_conv3x3_wino_pad(w_oihw, u_fwd, u_dgrad, cout, cin, cin, stream);
}

// splits > 1: K (input channels) cut into `splits` ranges of `per` stages, raw partials to out[split][M][cout]
// (flags, bias, scale / shift then belong to the caller's reduction)
int tdx_conv3x3_wino_launch(const float* in, const float* u, const float* bias, float* out, int B, int H, int W,
                            int cin, int cout, int flags, const float* out_scale, const float* out_shift,
                            float* stats_partial, int splits, int per, tdx_stream_t stream) {
  if (!in || !u || !out) return TDX_E_BADARG;
  if (!tdx_conv3x3_wino_ok(B, H, W, cin, cout)) return TDX_E_SHAPE;
  if (flags & ~(TDX_CONV_OUT_BNRELU | TDX_CONV_OUT_STATS)) return TDX_E_BADARG;
  if ((flags & TDX_CONV_OUT_BNRELU) && (!out_scale || !out_shift)) return TDX_E_BADARG;
  if ((flags & TDX_CONV_OUT_STATS) && (!stats_partial || (flags & TDX_CONV_OUT_BNRELU))) return TDX_E_BADARG;
  if (splits < 1 || (splits > 1 && (per < 1 || (int64_t)per * (splits - 1) >= cin / WK))) return TDX_E_BADARG;
  WinoArgs a{};
  a.in = in; a.u = u; a.bias = bias; a.out = out; a.out_scale = out_scale; a.out_shift = out_shift;
  a.stats = stats_partial;
  a.B = B; a.H = H; a.W = W; a.Cin = cin; a.Cout = cout;
  a.th = (H + 1) / 2; a.tw = (W + 1) / 2;
  a.NT = B * a.th * a.tw;
  a.rcp_tpi = 1.0f / (float)(a.th * a.tw); a.rcp_tw = 1.0f / (float)a.tw;
  a.tilesN = cout / WN;
  a.M = B * H * W;
  a.per = per;
  a.compact = cdiv(a.NT, WT) < 64;
  const dim3 grid(a.compact ? cdiv(a.NT, WT) * a.tilesN : (cdiv(a.NT, WT) + 7) / 8 * 8 * a.tilesN, splits);
  a.stamps = g_knobs.conv_stamp == 3 && g_tdx_diag_buffer && (size_t)grid.x * grid.y * 64 <= g_tdx_diag_bytes
                 ? reinterpret_cast<unsigned long long*>(g_tdx_diag_buffer) : nullptr;   // diagnostic knob conv_stamp = 3
  const size_t lds = (size_t)2 * STAGE * sizeof(float) + WT * 2 * sizeof(unsigned);   // two stages + the tile table
  hipStream_t st = to_stream(stream);
#define TDX_WINO_LAUNCH(EPI_, SPL_, ROWS_)                                                                       \
  do {                                                                                                           \
    auto kern = conv3x3_wino_kernel<EPI_, SPL_, ROWS_>;                                                          \
    static bool attr_set = false;                                                                                \
    if (!attr_set) {                                                                                             \
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                                    \
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                  \
      if (e != hipSuccess) return (int)e;                                                                        \
      attr_set = true;                                                                                           \
    }                                                                                                            \
    kern<<<grid, 256, lds, st>>>(a);                                                                             \
  } while (0)
  const bool rows = g_knobs.wino_rows && cin / WK >= g_knobs.wino_rows_min_stages;   // the training launches' loop
  if (splits > 1) TDX_WINO_LAUNCH(EPI_PLAIN, true, false);
  else if (flags & TDX_CONV_OUT_BNRELU) TDX_WINO_LAUNCH(EPI_BNRELU, false, false);
  else if (flags & TDX_CONV_OUT_STATS) {
    if (rows) TDX_WINO_LAUNCH(EPI_STATS, false, true);
    else TDX_WINO_LAUNCH(EPI_STATS, false, false);
  } else if (rows) TDX_WINO_LAUNCH(EPI_PLAIN, false, true);
  else TDX_WINO_LAUNCH(EPI_PLAIN, false, false);
#undef TDX_WINO_LAUNCH
  TDX_CHECK_LAUNCH();
  return 0;
}

extern "C" int tdx_conv3x3_fwd_wino(const float* in, const float* u, const float* bias, float* out, int B, int H, int W,
                                    int cin, int cout, int flags, const float* out_scale, const float* out_shift,
                                    float* stats_partial, tdx_stream_t stream) {
  return tdx_conv3x3_wino_launch(in, u, bias, out, B, H, W, cin, cout, flags, out_scale, out_shift, stats_partial, 1, 0,
                                 stream);
}

// =====================================================================================================================
// Weight gradient by F(3x3, 2x2) (round 4).  dW[co][ci][kh][kw] = sum over 2x2 output tiles of sum_{i,j} dy[i][j] d[i+kh][j+kw],
// d the 4x4 input patch of the tile: a correlation with a 2x2 "filter" and a 3x3 result, the transposition of the
// forward's identity -
//
//     dW = G^T [ (A e A^T) .* (B^T d B) ] G        e: the tile's 2x2 of dy,  A = (A^T of the forward)^T,  B^T, G as above
//
// 16 multiplications per (tile, co, ci) instead of 36, summed over the tiles: sixteen GEMMs M_p[co][ci] = sum_tiles E_p[tile][co]
// V_p[tile][ci] whose K dimension is the TILES.  Both operands are transformed on the fly, per lane for its channels
// (lane l31 gives the A operand of output channel 2 l31 + c and the B operand of one input channel) and four tiles per
// K-stage of eight: the lane reads its channels of the tile's raw 4 dy pixels and input pixels from [tile][pixel][channel]
// LDS images (conflict-free: consecutive lanes = consecutive channels), computes E' = A' e A'^T (A' is A with the sign
// of its last row dropped - the signs s_xi s_nu come back in the output transform) and V = B^T d B, and issues one MFMA
// per (position, output-channel parity c) with them - the operand trick along the tiles: MFMA j of a stage contracts
// tile j (lanes 0-31) and tile 4+j (lanes 32-63).  The waves split the TRANSFORM ROWS: wave (h, wn) owns the positions
// xi = 2h, 2h+1 (all four nu) of all 64 output channels (the even and the odd 32) and input-channel half wn, so that no
// two waves compute the same transform: per tile a lane builds two rows of B^T d (from patch rows h..h+2: 8 adds) and
// their columns (8), and two rows of E' for output channels 2 l31 and 2 l31 + 1 (6 adds each) - 28 scalar adds for 16
// MFMAs where a split by output channel (every wave all 16 positions) needs 44: the fp32 MFMA shares the vector pipe,
// and each add beside it costs ~7 cycles.  Every accumulator sums the same products in the same order
// as in that split, from operands built by the same expressions: the result is bit-identical to it.  A stage is 4
// tile-iterations of 16 MFMAs; the operands of the NEXT tile are read and transformed in the shadow of the current
// tile's MFMAs, so only the very first tile of a workgroup has nothing to hide behind.  Three LDS stages of 40 KB (8
// tiles x (16 + 4) pixels x 64 channels); the pieces of stage s+2 are requested in tile-iterations 2 and 3 of stage s,
// behind the single barrier per stage that makes stage s+1 visible.  The DMA addressing is scalar: a wave's two tiles
// of a stage are wave-uniform, so their base offsets ride in soffset and the validity of a piece's pixels in a 64-bit
// lane mask built by the scalar unit; one v_cndmask per piece puts the out-of-range voffset on the lanes of invalid
// pixels (zero padding: image borders, odd maps, the ragged end of the chunk; soffset is outside the range check, so
// this v_cndmask is the bounds protection).  The table the workgroup builds once in LDS holds one word per tile: its
// first output pixel and the validity of its patch rows and columns.  The accumulators are never zeroed: a
// workgroup's first stage is a second copy of the stage's code whose first tile-iteration takes the constant 0 as C.  Epilogue:
// G^T . G mixes all four xi rows, held by two waves - each wave hands the rows of the OTHER channel parity to its
// partner through LDS (the ring is free by then) and finalises its own.  Output: the direct kernel's slabs
// [split][Cout][9][Cin], summed by the shared fixed-order reduction.
constexpr int GT8 = 8;                    // tiles per K-stage
constexpr int XS_F = GT8 * 16 * 64;       // floats of a stage's input patches  [tile][16 px][64 ci]
constexpr int ES_F = GT8 * 4 * 64;        // floats of a stage's dy tiles       [tile][4 px][64 co]
constexpr int WST_F = XS_F + ES_F;        // 10240 floats = 40 KB
constexpr int WNST = 3;
constexpr int WG_MAX_CHUNK = 1024;        // tiles per workgroup at most (table: 4 B per tile)
constexpr int WG_XCH_F = 4 * 8 * 16 * 64; // floats of the epilogue exchange: per wave 8 accumulators x 64 lanes (32 KB)
constexpr size_t WG_LDS = 131072;         // bytes: the ring + the largest table, or the exchange
static_assert((size_t)WNST * WST_F * 4 + (size_t)WG_MAX_CHUNK * 4 <= WG_LDS && (size_t)WG_XCH_F * 4 <= WG_LDS, "LDS");

struct WinoWgArgs {
  const float* in;
  const float* dy;
  float* slabs;
  int B, H, W, Cin, Cout, th, tw, NT, M;
  int tilesCo, tilesCi, chunk;
  unsigned long long* stamps;  // diagnostics (tools/gpu_wino_phases.py --wgrad), null in every product launch
};

#if defined(__HIP_DEVICE_COMPILE__)
// bit q of m (wave-uniform) -> lanes 16q .. 16q+15: the DMA lanes of pixel column q (patch) or output pixel q (dy)
// (m < 16; s_bitreplicate doubles every bit of its 32-bit source: four of them widen a bit to sixteen lanes)
__device__ __forceinline__ unsigned long long wg_lanes16(unsigned m) {
  unsigned long long r;
  asm("s_bitreplicate_b64_b32 %0, %1" : "=s"(r) : "s"(m));
  asm("s_bitreplicate_b64_b32 %0, %1" : "=s"(r) : "s"((unsigned)r));
  asm("s_bitreplicate_b64_b32 %0, %1" : "=s"(r) : "s"((unsigned)r));
  asm("s_bitreplicate_b64_b32 %0, %1" : "=s"(r) : "s"((unsigned)r));
  return r;
}
// per lane: mask bit of the lane ? x : y - one VALU, the mask read from an SGPR pair
__device__ __forceinline__ unsigned wg_sel(unsigned long long mask, unsigned x, unsigned y) {
  unsigned r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(y), "v"(x), "s"(mask));
  return r;
}
#endif

__global__ void __launch_bounds__(256)
conv3x3_wgrad_wino_kernel(WinoWgArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  unsigned* tab = reinterpret_cast<unsigned*>(smem + WNST * WST_F);
  const unsigned long long t_entry = a.stamps ? __builtin_amdgcn_s_memrealtime() : 0ull;   // diagnostics only
  unsigned long long t_table = 0, t_first = 0, t_loop = 0, c_loop = 0;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int wn = wave & 1;
  const int ntile = a.tilesCo * a.tilesCi;
  const int split = blockIdx.x / ntile, tl = blockIdx.x - split * ntile;
  const int tile_co = tl / a.tilesCi, tile_ci = tl - tile_co * a.tilesCi;
  const int co0 = tile_co * 64, ci0 = tile_ci * 64;
  const int T_lo = split * a.chunk;
  const int T_hi = min(T_lo + a.chunk, a.NT);
  const int ns = (T_hi - T_lo + GT8 - 1) / GT8;
  const int tpi = a.th * a.tw;
  const int neg = (a.W + 1) * a.Cin;   // the input descriptor starts (W+1) pixels before the tensor: patch row / column -1

  // ---- the tile table: per tile {index of its output pixel (0,0) (< 2^23) | validity of the 4 patch columns (bits 4-7)
  // and rows (bits 0-3)}; the output pixels are patch rows / columns 1 and 2, a tile past the chunk's end is all invalid
  for (int i = tid; i < ns * GT8; i += 256) {
    const int T = T_lo + i;
    unsigned e = 0;
    if (T < T_hi) {
      const int b = T / tpi, rem = T - b * tpi;
      const int ty = rem / a.tw, tx = rem - ty * a.tw;
      unsigned rows = 0, cols = 0;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if ((unsigned)(2 * ty - 1 + p) < (unsigned)a.H) rows |= 1u << p;
        if ((unsigned)(2 * tx - 1 + p) < (unsigned)a.W) cols |= 1u << p;
      }
      e = (unsigned)((b * a.H + 2 * ty) * a.W + 2 * tx) << 8 | cols << 4 | rows;
    }
    tab[i] = e;
  }
  __syncthreads();
  if (a.stamps) t_table = __builtin_amdgcn_s_memrealtime();

  const auto rsrc_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in) - neg, 0,
                                                         (int)(((int64_t)a.M * a.Cin + 2 * neg) * 4), 0x00020000);
  const auto rsrc_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), 0, (int)((int64_t)a.M * a.Cout * 4), 0x00020000);
  // DMA lane: pixel column q = lane / 16 of the piece (patch column / output pixel), channels 4 (lane % 16) .. +3;
  // the patch row and the tile are in soffset
  const int q = lane >> 4, c16 = lane & 15;
  const unsigned x_lane = (unsigned)((q * a.Cin + ci0 + c16 * 4) * 4);
  const unsigned dy_lane = (unsigned)((((q >> 1) * a.W + (q & 1)) * a.Cout + co0 + c16 * 4) * 4);
  const unsigned row_bytes = (unsigned)(a.W * a.Cin * 4), cin4 = (unsigned)a.Cin * 4u, cout4 = (unsigned)a.Cout * 4u;
  unsigned oob = 0x80000000u;   // the out-of-range voffset, in a VGPR of its own (the v_cndmask operand)
  asm volatile("" : "+v"(oob));

  // the wave-uniform DMA state of this wave's two tiles 2*wave, 2*wave+1 of a stage, from their table entries
  struct Pair { unsigned xb[2], rows[2], db[2]; unsigned long long cm[2], dm[2]; };
  // (patch pixel (0,0) of the tile is (W+1) pixels before its output pixel (0,0): the input descriptor's base)
  // of table entry w (in an SGPR): the patch half (tile t's base offset, row validity, lane mask of its columns) ...
  auto pair_x = [&](Pair& P, int t, unsigned w) {
    P.xb[t] = (w >> 8) * cin4;
    P.rows[t] = w & 15u;
    P.cm[t] = wg_lanes16((w >> 4) & 15u);
  };
  // ... and the dy half
  auto pair_dy = [&](Pair& P, int t, unsigned w) {
    const unsigned r12 = (w >> 1) & 3u, c12 = (w >> 5) & 3u;   // output rows / columns 0, 1
    P.db[t] = (w >> 8) * cout4;
    P.dm[t] = wg_lanes16(((r12 & 1u) ? c12 : 0u) | ((r12 & 2u) ? c12 << 2 : 0u));   // output pixel q = 2 row + column
  };
  auto pair_of = [&](uint2 e) {
    Pair P;
    const unsigned w[2] = {(unsigned)__builtin_amdgcn_readfirstlane(e.x), (unsigned)__builtin_amdgcn_readfirstlane(e.y)};
#pragma unroll
    for (int t = 0; t < 2; ++t) { pair_x(P, t, w[t]); pair_dy(P, t, w[t]); }
    return P;
  };
  auto entries = [&](int s) {   // (past the end: a redundant copy of the last stage, never read)
    const int sc = s < ns ? s : ns - 1;
    return *reinterpret_cast<const uint2*>(tab + sc * GT8 + 2 * wave);
  };
  // piece k (0..9) of a stage into buffer buf: tile 2*wave + (k >> 2), patch row k & 3 (k < 8), then the two dy tiles
  auto issue_piece = [&](int k, const Pair& P, int buf) {
    float* Xb = smem + buf * WST_F;
    float* Eb = Xb + XS_F;
    if (k < 8) {
      const int t = k >> 2, r = k & 3;
      const unsigned long long m = (P.rows[t] >> r) & 1u ? P.cm[t] : 0ull;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_in, (lds_ptr_t)(Xb + ((2 * wave + t) * 16 + r * 4) * 64), 16,
                                               wg_sel(m, x_lane, oob), P.xb[t] + r * row_bytes, 0, 0);
    } else {
      const int t = k - 8;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_dy, (lds_ptr_t)(Eb + (2 * wave + t) * 4 * 64), 16,
                                               wg_sel(P.dm[t], dy_lane, oob), P.db[t], 0, 0);
    }
  };

  const int x_rd = wn * 32 + l31;
  // The body for wave row pair H (wave = 2 H + wn): the transforms differ between the two (rows 0/1 of B^T d are
  // d0 - d2, d1 + d2; rows 2/3 are d2 - d1, d1 - d3), so each has its own copy of the loop.
  auto body = [&](auto Hc) {
    constexpr int H = decltype(Hc)::value;
    // [c][xi - 2H][nu]: output channels 2 m + c (m the accumulator row).  Never zeroed: the first tile-iteration of the
    // workgroup's first stage takes the constant 0 as C (the first stage is a second copy of the stage's code)
    f32x16 acc[16];
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    // operands of one tile for this lane: E'[c][xi - 2H][nu] (output channels 2 l31, 2 l31 + 1), V[xi - 2H][nu] (its
    // input channel)
    float Ec[16], Vc[8], En[16], Vn[8];
    float dr[12], er[8], ern[8];   // raw values of the tile being prepared: patch rows H .. H+2, dy of both channels
    // LDS byte addresses of this lane's raw values of tile half*4 in buffer 0 (patch row H, channel x_rd; dy channels
    // 2 l31, +1): a buffer is one add away, a tile and a pixel are immediate offsets of the ds_read
    typedef __attribute__((address_space(3))) const float lds_f;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const unsigned lds0 = (unsigned)(size_t)(lds_f*)smem;
    const unsigned rx_lane = lds0 + (unsigned)((half * 4 * 16 * 64 + 4 * H * 64 + x_rd) * 4);
    const unsigned re_lane = lds0 + (unsigned)((XS_F + half * 4 * 4 * 64) * 4 + l31 * 8);
    auto read_raw = [&](unsigned rx, unsigned re, int j, float (&E)[8]) {   // tile half*4 + j
#pragma unroll
      for (int p = 0; p < 12; ++p) dr[p] = *(lds_f*)(size_t)(rx + j * 16 * 64 * 4 + p * 256);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const f32x2 v = *(const __attribute__((address_space(3))) f32x2*)(size_t)(re + j * 4 * 64 * 4 + p * 256);
        E[p] = v[0]; E[4 + p] = v[1];
      }
    };
    float tt[8], aa[4];
    auto xop = [&](int k, float (&V)[8], float (&E)[16]) {   // k-th of the 28 scalar adds that turn (dr, er) into (V, E')
      if (k < 8) {          // the two rows of B^T d
        const int c = k & 3, w = k >> 2;
        if (H == 0) {
          if (w == 0) tt[c] = s_sub(dr[c], dr[8 + c]);               // d0 - d2
          else tt[4 + c] = s_add(dr[4 + c], dr[8 + c]);              // d1 + d2
        } else {
          if (w == 0) tt[c] = s_sub(dr[4 + c], dr[c]);               // d2 - d1
          else tt[4 + c] = s_sub(dr[c], dr[8 + c]);                  // d1 - d3
        }
      } else if (k < 16) {  // columns: V = (B^T d) B
        const int r = (k - 8) >> 2, w = (k - 8) & 3;
        if (w == 0) V[4 * r] = s_sub(tt[4 * r], tt[4 * r + 2]);
        else if (w == 1) V[4 * r + 1] = s_add(tt[4 * r + 1], tt[4 * r + 2]);
        else if (w == 2) V[4 * r + 2] = s_sub(tt[4 * r + 2], tt[4 * r + 1]);
        else V[4 * r + 3] = s_sub(tt[4 * r + 1], tt[4 * r + 3]);
      } else {              // E' of output channel c2: er = (e00, e01, e10, e11); rows of A' e (e0j, e0j + e1j, e0j - e1j, e1j)
        const int c2 = (k - 16) / 6, w = (k - 16) % 6;
        const float* e = er + 4 * c2;
        float* a2 = aa + 2 * c2;
        if (w < 2) a2[w] = H == 0 ? s_add(e[w], e[2 + w]) : s_sub(e[w], e[2 + w]);   // row 1 / row 2
        else {             // columns: E'[xi] = (a_xi0, a_xi0 + a_xi1, a_xi0 - a_xi1, a_xi1)
          const int x = (w - 2) >> 1;   // xi - 2H
          const float a0 = (H == 0) == (x == 0) ? e[2 * H] : a2[0];
          const float a1 = (H == 0) == (x == 0) ? e[2 * H + 1] : a2[1];
          float* o = E + 8 * c2 + 4 * x;
          if ((w & 1) == 0) { o[0] = a0; o[3] = a1; o[1] = s_add(a0, a1); }
          else o[2] = s_sub(a0, a1);
        }
      }
    };

    // ---- main loop.  The raw values of tile j+2 are read at position 8 of tile-iteration j (the patch registers are free
    // by then), nine MFMAs before their first use: the 28 adds that prepare the next tile stand together behind MFMA 1
    // (per stage, profiles/r11_wino_phases_wgrad_ablation.txt: 2.20 us with four behind every second MFMA, 2.16 with
    // eight behind every fourth, 2.14 with 16 + 12, 2.13 with all 28 in one gap; over MFMAs 0-7 with the raw reads at
    // position 11: 2.23).  The one barrier per stage sits at the top of tile-iteration 2 (the reads of that iteration
    // are the first into stage s+1), and stage s+2 is requested behind it, in tile-iterations 2 and 3.  Its two table
    // entries are read with the raw values of tile-iteration 0 (the table never changes) and turned into the scalar DMA
    // state in the even gaps of tile-iteration 1, a part per gap: a wave is alone on its SIMD, so a run of scalar
    // instructions that outlasts one MFMA leaves the matrix pipe idle - built in one piece behind the barrier, the
    // ~80 instructions of the state cost 0.17 us per stage.
    {
      const Pair P0 = pair_of(entries(0));
#pragma unroll
      for (int k = 0; k < 10; ++k) issue_piece(k, P0, 0);
      const Pair P1 = pair_of(entries(1));
#pragma unroll
      for (int k = 0; k < 10; ++k) issue_piece(k, P1, 1);
    }
    asm volatile("s_waitcnt vmcnt(10)\n\ts_barrier" ::: "memory");
    read_raw(rx_lane, re_lane, 0, er);
#pragma unroll
    for (int k = 0; k < 28; ++k) xop(k, Vc, Ec);
    read_raw(rx_lane, re_lane, 1, er);
    if (a.stamps) { t_first = __builtin_amdgcn_s_memrealtime(); c_loop = __builtin_amdgcn_s_memtime(); }
    unsigned rx0 = rx_lane, re0 = re_lane;   // the addresses in the buffers of stages s and s+1 (rx1, re1)
    int b0 = 0;   // buffer of stage s
    auto stage = [&](auto first_c, int s) {
      constexpr bool FIRST = decltype(first_c)::value;
      int b1 = b0 + 1; b1 = b1 == WNST ? 0 : b1;
      int b2 = b1 + 1; b2 = b2 == WNST ? 0 : b2;
      unsigned rx1 = rx_lane + (unsigned)(b1 * WST_F * 4), re1 = re_lane + (unsigned)(b1 * WST_F * 4);
      asm volatile("" : "+v"(rx1), "+v"(re1));
      uint2 e2 = {0u, 0u};
      unsigned w0 = 0, w1 = 0;
      Pair P;
      auto tile_iter = [&](auto Jc) {
        constexpr int J = decltype(Jc)::value;
        if (J == 2) {
          // stage s+1 has landed (requested a stage ago) and every wave has finished reading stage s-1, whose buffer the
          // requests of stage s+2 overwrite
          asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < 16; ++p) {   // MFMA p: output channels 2 m + (p >> 3), position 2H + (p >> 2 & 1), nu = p & 3
          if (FIRST && J == 0) acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ec[p], Vc[p & 7], zero16, 0, 0, 0);
          else acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ec[p], Vc[p & 7], acc[p], 0, 0, 0);
          if (p == 1) {   // all 28 adds in ONE gap: every group of adds between two MFMAs costs the matrix pipe a restart
#pragma unroll
            for (int k = 0; k < 28; ++k) xop(k, Vn, En);
          }
          if (p == 8) {
            read_raw(J < 2 ? rx0 : rx1, J < 2 ? re0 : re1, (J + 2) & 3, ern);   // raw values of tile J + 2
            if (J == 0) e2 = entries(s + 2);
          }
          if (J == 1) {
            if (p == 0) { w0 = (unsigned)__builtin_amdgcn_readfirstlane(e2.x); w1 = (unsigned)__builtin_amdgcn_readfirstlane(e2.y); }
            if (p == 2) pair_x(P, 0, w0);
            if (p == 4) pair_x(P, 1, w1);
            if (p == 6) pair_dy(P, 0, w0);
            if (p == 10) pair_dy(P, 1, w1);
          }
          if ((J == 2 || J == 3) && p % 3 == 1 && p / 3 < 5) issue_piece(J == 2 ? p / 3 : 5 + p / 3, P, b2);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int p = 0; p < 16; ++p) Ec[p] = En[p];
#pragma unroll
        for (int p = 0; p < 8; ++p) { Vc[p] = Vn[p]; er[p] = ern[p]; }
      };
      tile_iter(std::integral_constant<int, 0>{});
      tile_iter(std::integral_constant<int, 1>{});
      tile_iter(std::integral_constant<int, 2>{});
      tile_iter(std::integral_constant<int, 3>{});
      b0 = b1; rx0 = rx1; re0 = re1;
    };
    stage(std::true_type{}, 0);
    for (int s = 1; s < ns; ++s) stage(std::false_type{}, s);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the ring is free

    if (a.stamps) { t_loop = __builtin_amdgcn_s_memrealtime(); c_loop = __builtin_amdgcn_s_memtime() - c_loop; }

    // ---- epilogue: this wave finalises output channels 2 m + H; the partner (1 - H, wn) holds its rows xi = 2 (1-H), +1.
    // Exchange: [receiving wave][accumulator][register quad][lane][4] (16-byte lane runs: conflict-free)
    {
      f32x4* xo = reinterpret_cast<f32x4*>(smem) + ((1 - H) * 2 + wn) * 2048 + lane;
#pragma unroll
      for (int p = 0; p < 8; ++p)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const f32x16& v = acc[8 * (1 - H) + p];
          xo[(p * 4 + r4) * 64] = f32x4{v[4 * r4], v[4 * r4 + 1], v[4 * r4 + 2], v[4 * r4 + 3]};
        }
    }
    __syncthreads();
    // dW = G^T (s_xi s_nu M') G per (co, ci), to this split's slab [Cout][9][Cin]
    float* slab = a.slabs + (size_t)split * a.Cout * 9 * a.Cin;
    const int ci = ci0 + wn * 32 + l31;
    const f32x4* xin = reinterpret_cast<const f32x4*>(smem) + wave * 2048 + lane;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      f32x4 pv[8];
#pragma unroll
      for (int p = 0; p < 8; ++p) pv[p] = xin[(p * 4 + r4) * 64];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int r = 4 * r4 + rr;
        const int co = co0 + 2 * ((r & 3) + 8 * (r >> 2) + 4 * half) + H;
        auto M = [&](int x, int nu) {   // accumulator of position (x, nu), output channel co
          return (x >> 1) == H ? acc[8 * H + 4 * (x & 1) + nu][r] : pv[4 * (x & 1) + nu][rr];
        };
        float R[3][4];
#pragma unroll
        for (int nu = 0; nu < 4; ++nu) {
          const float sg = nu == 3 ? -1.f : 1.f;
          const float m0 = sg * M(0, nu), m1 = sg * M(1, nu), m2 = sg * M(2, nu), m3 = -sg * M(3, nu);
          R[0][nu] = m0 + 0.5f * (m1 + m2);
          R[1][nu] = 0.5f * (m1 - m2);
          R[2][nu] = 0.5f * (m1 + m2) + m3;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          float* dst = slab + ((size_t)co * 9 + 3 * k) * a.Cin + ci;
          dst[0] = R[k][0] + 0.5f * (R[k][1] + R[k][2]);
          dst[a.Cin] = 0.5f * (R[k][1] - R[k][2]);
          dst[2 * a.Cin] = 0.5f * (R[k][1] + R[k][2]) + R[k][3];
        }
      }
    }
  };
  if (wave >> 1) body(std::integral_constant<int, 1>{});
  else body(std::integral_constant<int, 0>{});

  if (a.stamps && tid == 0) {   // 10-ns ticks: entry, table built, first tile prepared, loop end, epilogue end; loop cycles; ids
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned long long* o = a.stamps + 8 * (size_t)blockIdx.x;
    o[0] = t_entry; o[1] = t_table; o[2] = t_first; o[3] = t_loop; o[4] = __builtin_amdgcn_s_memrealtime();
    o[5] = c_loop;
    o[6] = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));          // HW_REG_HW_ID
    o[7] = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 0xf;    // XCC id
  }
#endif
}

// pixel chunks (in tiles, a multiple of 8) of the Winograd weight gradient: about `target` workgroups of 64 x 64 channels
static int wino_wgrad_plan(int NT, int cin, int cout, int* chunk) {
  const int ntile = (cout / 64) * (cin / 64);
  const int target = g_knobs.wino_wgrad_target;
  int splits = (target + ntile - 1) / ntile;
  int ch = (NT + splits - 1) / splits;
  ch = (ch + GT8 - 1) / GT8 * GT8;
  if (ch < 4 * GT8) ch = 4 * GT8;               // at least four stages per workgroup
  if (ch > WG_MAX_CHUNK) ch = WG_MAX_CHUNK;
  *chunk = ch;
  return (NT + ch - 1) / ch;
}

extern "C" int tdx_conv3x3_wgrad_wino_splits(int B, int H, int W, int cin, int cout) {
  if (B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || cin % 64 || cout % 64) return 0;
  int chunk;
  return wino_wgrad_plan(B * ((H + 1) / 2) * ((W + 1) / 2), cin, cout, &chunk);
}

// dw_slabs: [tdx_conv3x3_wgrad_wino_splits][cout][9][cin] (the format of tdx_conv3x3_wgrad: same reduction); raw input
extern "C" int tdx_conv3x3_wgrad_wino(const float* in, const float* dy, float* dw_slabs, int B, int H, int W, int cin,
                                      int cout, tdx_stream_t stream) {
  if (!in || !dy || !dw_slabs) return TDX_E_BADARG;
  if (B <= 0 || H <= 0 || W <= 0 || cin % 64 || cout % 64 || cin <= 0 || cout <= 0) return TDX_E_SHAPE;
  const int64_t M = (int64_t)B * H * W;
  if ((M * cin + 2 * (int64_t)(W + 1) * cin) * 4 >= (1ll << 31) || M * cout * 4 >= (1ll << 31)) return TDX_E_SHAPE;
  WinoWgArgs a{};
  a.in = in; a.dy = dy; a.slabs = dw_slabs;
  a.B = B; a.H = H; a.W = W; a.Cin = cin; a.Cout = cout;
  a.th = (H + 1) / 2; a.tw = (W + 1) / 2;
  a.NT = B * a.th * a.tw;
  a.M = (int)M;
  a.tilesCo = cout / 64; a.tilesCi = cin / 64;
  const int splits = wino_wgrad_plan(a.NT, cin, cout, &a.chunk);
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_wgrad_wino_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)WG_LDS);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  a.stamps = g_knobs.conv_stamp == 3 && g_tdx_diag_buffer && (size_t)splits * a.tilesCo * a.tilesCi * 64 <= g_tdx_diag_bytes
                 ? reinterpret_cast<unsigned long long*>(g_tdx_diag_buffer) : nullptr;   // diagnostic knob conv_stamp = 3
  const dim3 grid(splits * a.tilesCo * a.tilesCi);
  conv3x3_wgrad_wino_kernel<<<grid, 256, WG_LDS, to_stream(stream)>>>(a);
  TDX_CHECK_LAUNCH();
  return 0;
}
