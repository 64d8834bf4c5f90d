// Whole-network orchestration of the reference's UNet noise predictors and their autograd
// backward, as a fixed sequence of kernel launches on HIP streams.  No allocation, no host
// sync: the sequence can be captured into a hipGraph by the caller.
//
//   kind 0  NoiseModel of diffusion.py:11-162 / conditional_diffusion.py:14-172
//           (1x28x28 input, widths 64..512, raw-t time MLP, optional class embedding,
//            ceil-mode pooling 28->14->7->4 and resize-to-match skips 7->8, 14->16, 28->32, 32->28)
//   kind 1  NoiseModel of conditional_diffusion_laion.py:234-332
//           (4x32x32 latents, widths 32..256, sinusoidal embedding + 768-d MLP + additive text
//            conditioning, pooling 32->16->8->4, skips at equal resolution)
//
// Data flow (channels-last, fp32).  Only PRE-BatchNorm convolution outputs Y[u] are stored;
// every consumer applies relu(y*scale+shift) on load:
//
//   x -> initial_conv -> x0 -> U0 -> U1 -+-> pool -> U2 -> U3 -+-> pool -> U4 -> U5 -+-> pool -> U6
//                                        |                     |                     |           |
//        cat1 = [up(U10) | rs(U1 + t1)] <+  cat2 = [up(U8) | rs(U3 + t2)]  cat3 = [up(U6) | rs(U5 + t3)]
//   cat3 -> U7 -> U8 ; cat2 -> U9 -> U10 ; cat1 -> U11 -> U12 -> resize -> final_conv -> eps
//
// The channel concatenations (diffusion.py:140,147,154) cost nothing: the two resize kernels
// write straight into the two channel halves of one buffer.
#include "internal.h"
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <new>
#include <string>
#include <vector>

namespace {

struct UnitDef {
  int cin, cout, hw;  // square maps; cin as STORED (the LAION x0 is zero-padded 32 -> 64 channels)
  int in_bn;          // 1: input is Y[u-1] (BN+ReLU on load); 0: raw tensor
  int cin_real;       // channels of the reference weight tensor
};

struct NetSpec {
  int in_ch, hw0, out_hw;  // model input channels / resolution, output resolution
  int x0_ch, x0_real;      // initial_conv output channels as stored / in the reference
  int overlap;             // 1: training runs on three streams (see tdx_unet_backward); 0: one stream
  int time_dim;
  int enc_hw[4];           // resolutions of enc1, enc2, enc3, bottleneck
  int dec_hw[3];           // resolutions of dec3, dec2, dec1
  int skip_ch[3];          // channels of e1, e2, e3 (= time_proj widths)
  UnitDef units[13];       // enc1.0 enc1.3 enc2.0 enc2.3 enc3.0 enc3.3 bottleneck dec3.0 dec3.3 dec2.0 dec2.3 dec1.0 dec1.3
};

const NetSpec SPECS[2] = {
    {1, 28, 28, 64, 64, 1, 256, {28, 14, 7, 4}, {8, 16, 32}, {128, 256, 512},
     {{64, 128, 28, 0, 64},  {128, 128, 28, 1, 128}, {128, 256, 14, 0, 128}, {256, 256, 14, 1, 256},
      {256, 512, 7, 0, 256}, {512, 512, 7, 1, 512},  {512, 512, 4, 0, 512},  {1024, 256, 8, 0, 1024},
      {256, 256, 8, 1, 256}, {512, 128, 16, 0, 512}, {128, 128, 16, 1, 128}, {256, 64, 32, 0, 256},
      {64, 64, 32, 1, 64}}},
    // overlap: in round 1 this network ran 22 % SLOWER on three streams (11.7 -> 14.4 ms at B=256: two GEMMs
    // thrashing the L2s under its thin 64-channel layers) and was kept on one.  With round 2's weight-gradient
    // split (half the slab traffic), slab reduction and loss kernels the sign flipped - B=256, one / three
    // streams: 10.88 / 10.20 ms at 32x32, 39.6 / 37.8 at 64x64, bf16 mode 5.66 / 5.04 and 18.4 / 17.6 - so it
    // overlaps like the MNIST network (mode 2, helpers only on the third stream: 10.85, no gain).
    {4, 32, 32, 64, 32, 1, 768, {32, 16, 8, 4}, {8, 16, 32}, {64, 128, 256},
     {{64, 64, 32, 0, 32},   {64, 64, 32, 1, 64},    {64, 128, 16, 0, 64},   {128, 128, 16, 1, 128},
      {128, 256, 8, 0, 128}, {256, 256, 8, 1, 256},  {256, 256, 4, 0, 256},  {512, 256, 8, 0, 512},
      {256, 256, 8, 1, 256}, {384, 128, 16, 0, 384}, {128, 128, 16, 1, 128}, {192, 64, 32, 0, 192},
      {64, 64, 32, 1, 64}}}};

constexpr int N_STAGES = 15;

// The table rows are the reference resolutions.  The LAION network is fully convolutional
// (floor-mode pooling, exact 2x up-sampling, skips at equal resolution:
// conditional_diffusion_laion.py:304-332), so any input side hw = 32 * k / 4 (a multiple of 8, >= 32)
// runs through the same code: every resolution of the table scales by hw / 32.  The MNIST network
// resizes to fixed sizes (7->8, 14->16, 28->32, 32->28: diffusion.py:135-159): 28 only.
bool make_spec(int kind, int hw, int time_dim, NetSpec* out) {
  NetSpec S = SPECS[kind];
  // time_dim is a constructor argument of the reference's NoiseModel (diffusion.py:16,
  // conditional_diffusion_laion.py:236): any width (multiples of 256 up to 1024 run on the row kernels of
  // time_embed.hip, everything else on its generic ones; the sinusoidal embedding needs 4 columns)
  if (time_dim > 0) {
    if (time_dim > 4096 || (kind == 1 && time_dim < 4)) return false;
    S.time_dim = time_dim;
  }
  if (hw <= 0 || hw == S.hw0) { *out = S; return true; }
  if (kind != 1 || hw % 8 || hw < 32 || hw > 512) return false;
  auto sc = [&](int v) { return (int)((int64_t)v * hw / 32); };
  S.hw0 = S.out_hw = hw;
  for (int i = 0; i < 4; ++i) S.enc_hw[i] = sc(S.enc_hw[i]);
  for (int i = 0; i < 3; ++i) S.dec_hw[i] = sc(S.dec_hw[i]);
  for (int i = 0; i < 13; ++i) S.units[i].hw = sc(S.units[i].hw);
  *out = S;
  return true;
}


inline size_t align64(size_t n) { return (n + 63) / 64 * 64; }

// Workspace layout in floats, a pure function of (spec, batch).
struct Layout {
  size_t x, t, y;               // copies of the inputs (t is int64 -> 2 floats each; y: labels or embeddings)
  size_t sin, pre, emb, tp[3];  // time path: sinusoid (kind 1), first-layer pre-activation, embedding, projections
  size_t x0, Y[13], ss[13];     // ss: scale | shift | mean | rstd (4*cout)
  size_t A[13];                 // relu(bn(Y[u])) for the units whose successor is a 3x3 conv on it (else unused)
  size_t ep[3], cat[3], d1a;    // pooled encoder outputs, decoder inputs (cat[0] = level 3), resized d1
  size_t stats;                 // conv epilogue partials (largest unit)
  size_t ksplit, ksplit_floats; // split-K partials of the training convolutions (forward and dgrad share it: main stream)
  // backward
  size_t G1, G2, G3, G4, GS[3], gtp[3], slabs, slabs2, bnscr, smallp, smallp2, timescr;
  size_t gbuf;                  // floats in EACH of G1..G4
  size_t total;
};

Layout make_layout(const NetSpec& S, int B) {
  Layout L;
  size_t o = 0;
  auto take = [&](size_t n) { size_t r = o; o += align64(n); return r; };
  const size_t b = (size_t)B;
  const size_t px0 = (size_t)S.hw0 * S.hw0;
  L.x = take(b * px0 * S.in_ch); L.t = take(2 * b); L.y = take(std::max<size_t>(2 * b, b * S.time_dim));
  L.sin = take(b * S.time_dim); L.pre = take(b * S.time_dim); L.emb = take(b * S.time_dim);
  for (int k = 0; k < 3; ++k) L.tp[k] = take(b * S.skip_ch[k]);
  L.x0 = take(b * px0 * S.x0_ch);
  size_t stats = 0, slabs = 0, bnscr = 0, gbuf = 0, ksplit = 0;
  for (int u = 0; u < 13; ++u) {
    const UnitDef& d = S.units[u];
    L.Y[u] = take(b * d.hw * d.hw * d.cout);
    L.ss[u] = take(4 * (size_t)d.cout);
    L.A[u] = (u + 1 < 13 && S.units[u + 1].in_bn) ? take(b * d.hw * d.hw * d.cout) : 0;
    stats = std::max(stats, (size_t)tdx_conv3x3_stat_tiles(B, d.hw, d.hw, d.cin, d.cout) * 2 * d.cout);
    slabs = std::max(slabs, (size_t)std::max(std::max(tdx_conv3x3_wgrad_splits(B, d.hw, d.hw, d.cin, d.cout),
                                                      tdx_conv3x3_wgrad_splits_bf16(B, d.hw, d.hw, d.cin, d.cout)),
                                             tdx_conv3x3_wgrad_wino_splits(B, d.hw, d.hw, d.cin, d.cout)) *
                                9 * (size_t)d.cin * d.cout);
    ksplit = std::max(ksplit, std::max(tdx_conv3x3_train_scratch_floats(B, d.hw, d.hw, d.cin, d.cout),
                                       tdx_conv3x3_train_scratch_floats(B, d.hw, d.hw, d.cout, d.cin)));
    bnscr = std::max(bnscr, tdx_bn_relu_bwd_scratch_floats((int64_t)b * d.hw * d.hw, d.cout));
    gbuf = std::max(gbuf, b * d.hw * d.hw * (size_t)std::max(d.cin, d.cout));
  }
  for (int k = 0; k < 3; ++k) {
    const int hp = S.enc_hw[k + 1];
    L.ep[k] = take(b * hp * hp * S.skip_ch[k]);
  }
  for (int k = 0; k < 3; ++k) {  // cat[0]: dec3 input ... cat[2]: dec1 input
    const UnitDef& d = S.units[7 + 2 * k];
    L.cat[k] = take(b * d.hw * d.hw * d.cin);
  }
  L.d1a = take(b * S.out_hw * S.out_hw * 64);
  gbuf = std::max(gbuf, b * (size_t)S.out_hw * S.out_hw * 64);
  L.stats = take(stats);
  L.ksplit_floats = ksplit;
  L.ksplit = take(ksplit);
  L.gbuf = gbuf;
  L.G1 = take(gbuf); L.G2 = take(gbuf); L.G3 = take(gbuf); L.G4 = take(gbuf);
  for (int k = 0; k < 3; ++k) {
    L.GS[k] = take(b * S.enc_hw[k] * S.enc_hw[k] * S.skip_ch[k]);
    L.gtp[k] = take(b * S.skip_ch[k]);
  }
  L.slabs = take(slabs);
  L.slabs2 = take(slabs);
  L.bnscr = take(bnscr);
  L.smallp = take((size_t)tdx_small_conv_wgrad_blocks(B, S.hw0, S.hw0) * tdx_small_conv_partial_width());
  L.smallp2 = take((size_t)tdx_small_conv_wgrad_blocks(B, S.hw0, S.hw0) * tdx_small_conv_partial_width());
  L.timescr = take(3 * b * S.time_dim);
  L.total = o;
  return L;
}

}  // namespace

struct PlanHandles {
  hipStream_t side, side2, half;
  hipEvent_t ev[81];
};

struct tdx_unet {
  int max_batch, num_classes, kind;
  NetSpec spec_own;        // the table row scaled to this plan's resolution
  const NetSpec* spec;
  float* wpack;            // device: per unit fwd pack then dgrad pack
  size_t wf_off[13], wd_off[13];
  float* upack;            // device: Winograd packs (transformed weights), per unit forward then input gradient
  size_t uf_off[13], ud_off[13];
  bool wino_f[13], wino_d[13], wino_w[13];   // this step's forward / input gradient / weight gradient of unit i runs on the Winograd kernels (decided per forward)
  float* infer_ss;         // device: per unit scale|shift from running stats (INFER mode)
  size_t iss_off[13];
  bool packed;
  bool wf_tiled;           // INFER pack of the fp32 mode: wf holds the tile-major pack of the inference convolution (conv3x3.hip, variant 4)
  // sampling tables (tdx_unet_prepare_sampling; time_embed.hip): tab = [T][w1] | [T][w2] | [T][w3] | cond part
  // [tab_batch][w1|w2|w3] | scratch.  Valid for the INFER pack generation they were built at and for the
  // (batch, cond pointer) they were built with; tdx_unet_eval_step falls back to the direct path otherwise.
  float* tab;
  size_t tab_floats;
  int tab_T, tab_batch, tab_gen, pack_gen;
  const void* tab_cond;
  const int64_t* tab_tau;   // timestep schedule the T rows were built at (tdx_unet_prepare_sampling_sched); null: t = 0..T-1
  bool skip_time_path;   // set by tdx_unet_eval_step around its forward: the projections are already in the workspace
  // set by tdx_unet_eval_step around its forward: final_conv applies the reverse-process update in its epilogue
  PStep ps;   // ps.x != null: armed
  bool whole_batch;      // set by a guided eval step around its forward: the two halves of a guided batch are not the halves of "sample_halves"
  // half-batch inference (tdx_unet_forward, INFER mode): the second half runs on this stream, forked from / joined to the caller's
  hipStream_t half_own;
  hipEvent_t ev_h_fork, ev_h_join;
  PlanHandles handles;   // what the fields above were filled from (returned to the pool by tdx_unet_destroy)
  int precision, saved_precision;  // TDX_PREC_*: of the next forward / of the saved forward
  int io16, saved_io16;            // bf16 mode: activation tensors in the workspace hold bf16 (io16.h); of the next / saved forward
  tdx_allreduce_fn bn_sync;        // synchronised BatchNorm: all-reduce callback (null: rank-local statistics)
  void* bn_sync_user;
  double* bn_sync_buf;
  int saved_batch, saved_mode;  // state of the last forward (for backward)
  // backward state that survives between tdx_unet_backward calls that split the stages:
  float* g_next;                // where the gradient w.r.t. the next unit's activation lives
  int bw_unit, bw_nblk;         // unit whose BatchNorm-backward partial sums a producer kernel has left in bnscr (-1: none)
  float* g_x;                   // one-shot request: d loss / d x written by the last backward stage (null: not asked)
  struct GBuf { float* p; int w_unit; int s2; int age; } gb[4];  // rotating gradient buffers + last readers
  int clock;
  bool red_pending[13];         // slab reduction of unit i enqueued (third stream) and not yet waited for
  // backward runs the weight-gradient GEMMs on a second (low-priority) HIP stream so that
  // they fill the tail of the input-gradient GEMM and overlap the HBM-bound BN/pool/resize
  // kernels of the next unit; fork/join with events, so the caller still sees ONE stream
  bool materialize;             // train: write relu(bn(Y)) of the first conv of every stage (see Layout::A)
  int use_streams;              // 0: `side` / `side2` alias the caller's stream; 1: three streams; 2: the weight-
                                // gradient GEMMs stay on the caller's stream, only the HBM-bound helpers (slab
                                // reductions, boundary-conv weight gradients' reductions, skip-branch resizes,
                                // time path) use the third stream
  hipStream_t side_own, side2_own;
  hipStream_t side;
  hipEvent_t ev_dy[13], ev_w[13], ev_join, ev_fork, ev_pack;
  // third stream: the HBM-bound skip-branch resizes (forward and backward) run beside the
  // convolutions instead of between them
  hipStream_t side2;
  hipEvent_t ev_s2_fork[3], ev_s2_done[3], ev_join2, ev_red[13];
  hipEvent_t ev_mark[N_STAGES][2];   // tdx_unet_backward_mark: where side / side2 were when slot i was marked
  // Waits the caller's stream does not need (helper_record / caller_wait below): the events the caller's stream waits
  // for (ev_w, ev_pack on `side`; ev_s2_done on `side2`) are numbered per helper stream as they are recorded, and
  // `seen` is the highest number of each helper the caller's stream `st` has waited for since caller_begin.
  struct Joined { hipStream_t st; bool capturing; uint64_t rec[2], seen[2]; } jn;
  uint64_t seq_w[13], seq_s2[3], seq_pack;
};

// An event wait costs the waiting stream 4-6 us on MI355X whether or not the event has completed long ago
// (tools/micro/event_boundary_probe.hip, profiles/r12_event_boundary_probe.txt): the barrier packet is processed in
// queue order in front of the next kernel.  A helper stream completes its events in the order it records them, so a
// wait for event n of helper h (0: side, 1: side2) orders the caller's stream behind every earlier event of h too, and
// a later wait for one of those is not enqueued.  The same holds inside a stream capture (a helper's captured nodes
// form a chain).  The bookkeeping starts afresh with every training forward, and whenever the caller's stream or its
// capture status is another one than at the last wait.
static void caller_begin(tdx_unet* u, hipStream_t st, bool fresh) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cs);
  const bool capturing = cs == hipStreamCaptureStatusActive;
  if (fresh || st != u->jn.st || capturing != u->jn.capturing) u->jn.seen[0] = u->jn.seen[1] = 0;
  u->jn.st = st;
  u->jn.capturing = capturing;
}

static hipError_t helper_record(tdx_unet* u, int h, hipEvent_t ev, uint64_t* seq) {
  *seq = ++u->jn.rec[h];
  return hipEventRecord(ev, h ? u->side2 : u->side);
}

static hipError_t caller_wait(tdx_unet* u, hipStream_t st, int h, hipEvent_t ev, uint64_t seq) {
  if ((h ? u->side2 : u->side) == st) return hipSuccess;   // the helper is the caller's stream itself
  if (seq <= u->jn.seen[h]) return hipSuccess;              // an earlier wait covers it
  u->jn.seen[h] = seq;
  return hipStreamWaitEvent(st, ev, 0);
}

// Streams and events of destroyed plans are RECYCLED, never destroyed (round 4).  A module keeps its six most recently
// used plans and destroys the rest, so a long process creates and destroys plans by the hundred; with a captured
// training graph alive, a replay right after such a destruction died inside hipGraphLaunch (segmentation fault in the
// runtime, ROCm 7.2 - only in processes that had already been through ~200 tests' worth of plans, never in a short one:
// tests/test_gpu_unet.py::test_captured_step_keeps_its_plan_alive_across_lru_eviction after test_gpu_ops.py).  The
// graph refers to none of the destroyed plan's objects; what the two have in common is the runtime's stream / event
// bookkeeping.  Handing the handles to the next plan instead takes hipStreamDestroy / hipEventDestroy out of the
// picture, and makes a plan's creation ~50 runtime calls cheaper.
static std::mutex g_handles_mu;
static std::vector<PlanHandles> g_handles_pool;

static bool make_handles(PlanHandles* h) {
  {
    std::lock_guard<std::mutex> lk(g_handles_mu);
    if (!g_handles_pool.empty()) { *h = g_handles_pool.back(); g_handles_pool.pop_back(); return true; }
  }
  int lo = 0, hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // lo = least urgent
  // side / side2: LOW priority, and not only for scheduling: ROCm multiplexes all streams of one priority level onto a
  // few hardware queues (GPU_MAX_HW_QUEUES, 4 by default).  A normal-priority helper can land on the caller's queue,
  // and its waits on the wgrad stream then block the main chain (measured with a communication stream + RCCL's stream
  // also alive: the step went from 16.3 to 18.1 ms, convolutions fully serialised; low priority: 16.7 ms).
  // half: the second half-batch of an inference forward: NORMAL priority like the caller's stream (the halves are peers).
  h->side = h->side2 = h->half = nullptr;
  if (hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, lo) != hipSuccess) return false;
  if (hipStreamCreateWithPriority(&h->side2, hipStreamNonBlocking, lo) != hipSuccess) return false;
  if (hipStreamCreateWithFlags(&h->half, hipStreamNonBlocking) != hipSuccess) return false;
  // ev[0..50] order work among the plan's own streams and the caller's on ONE device, inside a step: no system-scope
  // release (a record costs its stream 3-4 us instead of 5.6, profiles/r12_event_boundary_probe.txt; what the host or
  // another device reads is released by the caller's stream, whose kernels follow the join).  ev[51..80] are ev_mark:
  // the host synchronises on them and a communication stream consumes behind them, so they keep the system fence.
  // The flags go with the position in `ev`, so every pooled PlanHandles has the same ones.
  for (int i = 0; i < 81; ++i) {
    const unsigned flags = hipEventDisableTiming | (i < 51 ? hipEventDisableSystemFence : 0);
    if (hipEventCreateWithFlags(&h->ev[i], flags) != hipSuccess) return false;
  }
  return true;
}

static void recycle_handles(const PlanHandles& h) {
  (void)hipStreamSynchronize(h.side);
  (void)hipStreamSynchronize(h.side2);
  (void)hipStreamSynchronize(h.half);
  std::lock_guard<std::mutex> lk(g_handles_mu);
  g_handles_pool.push_back(h);
}

extern "C" int tdx_unet_create_ex(tdx_unet** out, int max_batch, int kind, int num_classes) {
  return tdx_unet_create_hw(out, max_batch, kind, num_classes, 0);
}

extern "C" int tdx_unet_create_hw(tdx_unet** out, int max_batch, int kind, int num_classes, int hw) {
  return tdx_unet_create_full(out, max_batch, kind, num_classes, hw, 0);
}

extern "C" int tdx_unet_create_full(tdx_unet** out, int max_batch, int kind, int num_classes, int hw,
                                    int time_dim) {
  if (!out || max_batch <= 0 || num_classes < 0 || kind < 0 || kind > 2 || hw < 0 || time_dim < 0) return TDX_E_BADARG;
  if (kind == TDX_UNET_LATENT_MLP && time_dim != 0 && time_dim != 256) return TDX_E_SHAPE;
  if (kind == TDX_UNET_LAION && num_classes != 0) return TDX_E_BADARG;
  if (kind == TDX_UNET_LATENT_MLP && num_classes <= 0) return TDX_E_BADARG;
  NetSpec spec_hw;
  if (kind != TDX_UNET_LATENT_MLP) {
    if (!make_spec(kind, hw, time_dim, &spec_hw)) return TDX_E_SHAPE;
    // every unit must be addressable at max_batch (32-bit buffer offsets: tdx_conv3x3_shape_ok)
    const NetSpec& S = spec_hw;
    for (int i = 0; i < 13; ++i)
      if (!tdx_conv3x3_shape_ok(max_batch, S.units[i].hw, S.units[i].hw, S.units[i].cin, S.units[i].cout))
        return TDX_E_SHAPE;
  }
  tdx_unet* u = new (std::nothrow) tdx_unet();
  if (!u) return TDX_E_BADARG;
  u->max_batch = max_batch;
  u->num_classes = num_classes;
  u->kind = kind;
  if (kind != TDX_UNET_LATENT_MLP) u->spec_own = spec_hw;
  u->spec = kind == TDX_UNET_LATENT_MLP ? nullptr : &u->spec_own;
  size_t o = 64, so = 0;
  if (u->spec) {
    for (int i = 0; i < 13; ++i) {
      const UnitDef& d = u->spec->units[i];
      const size_t n = (size_t)d.cin * d.cout * 9;
      u->wf_off[i] = o; o += align64(n);
      u->wd_off[i] = o; o += align64(n);
      u->iss_off[i] = so; so += align64(2 * (size_t)d.cout);
    }
  } else {
    so = tdx_latent_infer_ss_floats();  // the MLP needs no weight packs
  }
  hipError_t e = hipMalloc(&u->wpack, o * sizeof(float));
  if (e != hipSuccess) { delete u; return (int)e; }
  u->upack = nullptr;
  for (int i = 0; i < 13; ++i) u->wino_f[i] = u->wino_d[i] = u->wino_w[i] = false;
  if (u->spec) {
    size_t uo = 64;
    for (int i = 0; i < 13; ++i) {
      const size_t n = (size_t)u->spec->units[i].cin * u->spec->units[i].cout * 16;
      u->uf_off[i] = uo; uo += align64(n);
      u->ud_off[i] = uo; uo += align64(n);
    }
    e = hipMalloc(&u->upack, uo * sizeof(float));
    if (e != hipSuccess) { (void)hipFree(u->wpack); delete u; return (int)e; }
  }
  e = hipMalloc(&u->infer_ss, so * sizeof(float));
  if (e != hipSuccess) { (void)hipFree(u->wpack); if (u->upack) (void)hipFree(u->upack); delete u; return (int)e; }
  u->packed = false;
  u->wf_tiled = false;
  u->tab = nullptr;
  u->tab_floats = 0;
  u->tab_T = u->tab_batch = 0;
  u->tab_gen = -1;
  u->pack_gen = 0;
  u->tab_cond = nullptr;
  u->tab_tau = nullptr;
  u->skip_time_path = false;
  u->whole_batch = false;
  u->ps = {};
  u->precision = TDX_PREC_F32;
  u->saved_precision = TDX_PREC_F32;
  u->io16 = u->saved_io16 = 0;
  u->bn_sync = nullptr;
  u->bn_sync_user = nullptr;
  u->bn_sync_buf = nullptr;
  u->saved_batch = 0;
  u->saved_mode = -1;
  u->g_next = nullptr;
  u->g_x = nullptr;
  u->bw_unit = -1;
  u->bw_nblk = 0;
  u->materialize = g_knobs.materialize != 0;
  u->use_streams = g_knobs.streams < 0 ? (u->spec ? u->spec->overlap : 0) : g_knobs.streams;
  if (!make_handles(&u->handles)) {
    (void)hipFree(u->wpack); if (u->upack) (void)hipFree(u->upack); (void)hipFree(u->infer_ss);
    delete u;
    return TDX_E_STATE;
  }
  {
    const PlanHandles& h = u->handles;
    int k = 0;
    u->side_own = h.side; u->side2_own = h.side2; u->half_own = h.half;
    for (int i = 0; i < 13; ++i) { u->ev_dy[i] = h.ev[k++]; u->ev_w[i] = h.ev[k++]; u->ev_red[i] = h.ev[k++]; }
    for (int i = 0; i < 3; ++i) { u->ev_s2_fork[i] = h.ev[k++]; u->ev_s2_done[i] = h.ev[k++]; }
    u->ev_join = h.ev[k++]; u->ev_fork = h.ev[k++]; u->ev_pack = h.ev[k++]; u->ev_join2 = h.ev[k++];
    u->ev_h_fork = h.ev[k++]; u->ev_h_join = h.ev[k++];   // k == 51
    for (int i = 0; i < N_STAGES; ++i) { u->ev_mark[i][0] = h.ev[k++]; u->ev_mark[i][1] = h.ev[k++]; }   // k == 81
  }
  u->side = u->side_own;
  u->side2 = u->side2_own;
  u->jn = {};
  *out = u;
  return 0;
}

extern "C" int tdx_unet_create(tdx_unet** out, int max_batch, int num_classes) {
  return tdx_unet_create_ex(out, max_batch, 0, num_classes);
}

extern "C" int tdx_unet_set_bn_sync(tdx_unet* u, tdx_allreduce_fn fn, void* user, double* buffer) {
  if (!u || (fn && !buffer)) return TDX_E_BADARG;
  if (!u->spec) return fn ? TDX_E_SHAPE : 0;   // the latent MLP's BatchNorm1d kernels keep local statistics
  u->bn_sync = fn;
  u->bn_sync_user = user;
  u->bn_sync_buf = buffer;
  return 0;
}

extern "C" int tdx_unet_set_streams(tdx_unet* u, int mode) {
  if (!u || mode < -1 || mode > 2) return TDX_E_BADARG;
  u->use_streams = mode < 0 ? (u->spec ? u->spec->overlap : 0) : mode;
  return 0;
}

extern "C" int tdx_unet_set_precision(tdx_unet* u, int precision) {
  if (!u || (precision != TDX_PREC_F32 && precision != TDX_PREC_BF16)) return TDX_E_BADARG;
  if (!u->spec) { u->precision = precision; return 0; }   // latent MLP: bf16 operands in its Linear layers (mlp.hip); nothing is packed per precision
  if (precision != u->precision) u->packed = false;                 // INFER packs are per precision
  u->precision = precision;
  // bf16 mode = bf16 MFMA operands AND bf16 activation tensors in HBM (round 3; knob "bf16_storage" = 0 keeps fp32 tensors)
  u->io16 = precision == TDX_PREC_BF16 && g_knobs.bf16_storage ? 1 : 0;
  return 0;
}

extern "C" int tdx_unet_destroy(tdx_unet* u) {
  if (!u) return TDX_E_BADARG;
  recycle_handles(u->handles);   // (synchronises the plan's streams; nothing is destroyed: see PlanHandles)
  (void)hipFree(u->wpack);
  if (u->upack) (void)hipFree(u->upack);
  (void)hipFree(u->infer_ss);
  if (u->tab) (void)hipFree(u->tab);
  delete u;
  return 0;
}

extern "C" size_t tdx_unet_workspace_bytes(const tdx_unet* u, int batch, int mode) {
  (void)mode;
  if (!u || batch <= 0 || batch > u->max_batch) return 0;
  if (!u->spec) return tdx_latent_workspace_floats(batch) * sizeof(float);
  // (an inference forward may run as two half-batches, each in a layout of its own inside the same workspace)
  const size_t whole = make_layout(*u->spec, batch).total;
  const int b0 = (batch + 1) / 2;
  const size_t halves = batch >= 2 ? make_layout(*u->spec, b0).total + make_layout(*u->spec, batch - b0).total : 0;
  return std::max(whole, halves) * sizeof(float);
}

extern "C" int tdx_unet_backward_stages(void) { return N_STAGES; }

// Where a named intermediate lives inside the workspace (testing / debugging aid):
// "x0", "Y0".."Y12" (pre-BN conv outputs; post-activation in INFER mode), "ss0".."ss12"
// (scale|shift|mean|rstd), "e1p" "e2p" "e3p" "cat3" "cat2" "cat1" "d1a" "emb" "t1" "t2" "t3",
// "G1" "G2" "GS1" "GS2" "GS3".
extern "C" int tdx_unet_tensor(const tdx_unet* u, int batch, const char* name, size_t* offset_floats,
                               size_t* numel) {
  if (!u || !name || !offset_floats || !numel || batch <= 0 || batch > u->max_batch) return TDX_E_BADARG;
  if (!u->spec) return tdx_latent_tensor(batch, name, offset_floats, numel);
  const NetSpec& S = *u->spec;
  const Layout L = make_layout(S, batch);
  const size_t b = (size_t)batch;
  std::string n(name);
  auto unit_index = [&](const std::string& s, size_t prefix) -> int {
    if (s.size() <= prefix) return -1;
    int v = atoi(s.c_str() + prefix);
    return (v >= 0 && v < 13) ? v : -1;
  };
  auto sq = [](int v) { return (size_t)v * v; };
  struct { const char* nm; size_t off, cnt; } fixed[] = {
      {"x0", L.x0, b * sq(S.hw0) * S.x0_ch},
      {"e1p", L.ep[0], b * sq(S.enc_hw[1]) * S.skip_ch[0]},
      {"e2p", L.ep[1], b * sq(S.enc_hw[2]) * S.skip_ch[1]},
      {"e3p", L.ep[2], b * sq(S.enc_hw[3]) * S.skip_ch[2]},
      {"cat3", L.cat[0], b * sq(S.units[7].hw) * S.units[7].cin},
      {"cat2", L.cat[1], b * sq(S.units[9].hw) * S.units[9].cin},
      {"cat1", L.cat[2], b * sq(S.units[11].hw) * S.units[11].cin},
      {"d1a", L.d1a, b * sq(S.out_hw) * 64}, {"emb", L.emb, b * S.time_dim},
      {"t_copy", L.t, 2 * b}, {"tf", L.sin, b}, {"pre", L.pre, b * S.time_dim},
      {"time_g_h", L.timescr + 2 * b * S.time_dim, b * S.time_dim},
      {"t1", L.tp[0], b * S.skip_ch[0]}, {"t2", L.tp[1], b * S.skip_ch[1]}, {"t3", L.tp[2], b * S.skip_ch[2]},
      {"G1", L.G1, L.gbuf}, {"G2", L.G2, L.gbuf}, {"G3", L.G3, L.gbuf}, {"G4", L.G4, L.gbuf},
      {"GS1", L.GS[0], b * sq(S.enc_hw[0]) * S.skip_ch[0]},
      {"GS2", L.GS[1], b * sq(S.enc_hw[1]) * S.skip_ch[1]},
      {"GS3", L.GS[2], b * sq(S.enc_hw[2]) * S.skip_ch[2]}};
  for (auto& f : fixed)
    if (n == f.nm) { *offset_floats = f.off; *numel = f.cnt; return 0; }
  if (n.rfind("ss", 0) == 0) {
    int i = unit_index(n, 2);
    if (i < 0) return TDX_E_BADARG;
    *offset_floats = L.ss[i]; *numel = 4 * (size_t)S.units[i].cout; return 0;
  }
  if (n[0] == 'Y') {
    int i = unit_index(n, 1);
    if (i < 0) return TDX_E_BADARG;
    *offset_floats = L.Y[i]; *numel = b * sq(S.units[i].hw) * S.units[i].cout; return 0;
  }
  return TDX_E_BADARG;
}

// weights always; the INFER-mode scale/shift (from the running statistics) only when
// `buffers` is given
// `overlap`: the packs of units 2..12 (98 % of the weights) are written on the side stream while
// the main stream runs the time path, initial_conv and the first two units; the caller makes the
// main stream wait for ev_pack before unit 2.
// which units of a training step at batch B run on the Winograd kernel (fp32 only; the unit's input must be a raw tensor:
// x0, a pooled map, a concat buffer or a materialised relu(bn(.)))
// 1 when the training step at batch B runs this layer's forward (role 0) / input gradient (role 1) on the Winograd kernel:
// the geometry must be served in both directions and the launch must fill the chip (one workgroup per CU)
extern "C" int tdx_conv3x3_train_algo(int B, int H, int W, int cin, int cout, int role) {
  if (!g_knobs.wino || B <= 0 || role < 0 || role > 2) return 0;
  if (role == 2)   // weight gradient, F(3x3,2x2): any geometry; enough tiles that its workgroups (>= 4 stages of 8 tiles) fill the chip
    return g_knobs.wino_wgrad && cin % 64 == 0 && cout % 64 == 0 &&
           (int64_t)B * ((H + 1) / 2) * ((W + 1) / 2) >= g_knobs.wino_wgrad_min_tiles ? 1 : 0;
  if (!tdx_conv3x3_wino_ok(B, H, W, cin, cout) || !tdx_conv3x3_wino_ok(B, H, W, cout, cin)) return 0;
  const int blocks = tdx_conv3x3_wino_stat_tiles(B, H, W);
  return blocks * ((role == 0 ? cout : cin) / 64) >= g_knobs.wino_min_wgs ? 1 : 0;
}

// 1 when an INFER-mode (sampling) forward of n = B samples runs this layer on the Winograd kernel with split K
// (tdx_conv3x3_fwd_wino_infer), 0: on the direct kernels.  Winograd where the launch is big enough to pay for its fixed
// costs (one workgroup per CU, ring fill, output transform, partials): measured per layer at n = 16 / 32 / 64
// (profiles/r04_infer_layers_wino.txt) it wins wherever workgroups x stages >= ~800 and loses up to 6 us per layer
// below (the 64-channel and 4x4 layers at n = 16).  The plan must also hold the Winograd pack (decide_wino).
extern "C" int tdx_conv3x3_infer_algo(int B, int H, int W, int cin, int cout) {
  if (!g_knobs.wino_infer || g_knobs.infer_ring || !tdx_conv3x3_wino_ok(B, H, W, cin, cout)) return 0;
  return (int64_t)tdx_conv3x3_wino_stat_tiles(B, H, W) * (cout / 64) * (cin / 8) >= g_knobs.wino_infer_min_units ? 1 : 0;
}

static void decide_wino(tdx_unet* u, int B, bool training_modes) {
  for (int i = 0; i < 13; ++i) {
    u->wino_f[i] = u->wino_d[i] = u->wino_w[i] = false;
    const UnitDef& d = u->spec->units[i];
    if (!training_modes) {
      // INFER pack (fp32): every unit whose geometry the kernel serves (at any batch: the map size decides) gets a Winograd
      // pack; whether a forward uses it is decided from its batch (run_unit).  Post-activation tensors are raw inputs.
      u->wino_f[i] = g_knobs.wino_infer && u->precision != TDX_PREC_BF16 && !g_knobs.infer_ring &&
                     tdx_conv3x3_wino_ok(1, d.hw, d.hw, d.cin, d.cout);
      continue;
    }
    if (u->precision == TDX_PREC_BF16 || (d.in_bn && !u->materialize)) continue;   // (a BN+ReLU-on-load input is not raw)
    u->wino_f[i] = tdx_conv3x3_train_algo(B, d.hw, d.hw, d.cin, d.cout, 0) != 0;
    u->wino_d[i] = tdx_conv3x3_train_algo(B, d.hw, d.hw, d.cin, d.cout, 1) != 0;
    u->wino_w[i] = tdx_conv3x3_train_algo(B, d.hw, d.hw, d.cin, d.cout, 2) != 0;
  }
}

// the packs of units [lo, hi): direct packs where a direct kernel reads them, Winograd packs where that kernel runs
static int pack_units(tdx_unet* u, const float* const* P, int lo, int hi, tdx_stream_t stream, bool tiled, bool infer) {
  TdxPackBatch pb{};
  TdxWinoPackBatch wb{};
  for (int i = lo; i < hi; ++i) {
    const UnitDef& d = u->spec->units[i];
    // (INFER: both forward packs - which kernel a unit runs on is decided per forward from its batch - and no input-gradient pack)
    const bool need_f = infer || !u->wino_f[i], need_d = !infer && !u->wino_d[i];
    if (need_f || need_d) {
      const int k = pb.count++;
      pb.w[k] = P[TDX_P_UNIT0 + 4 * i];
      pb.wf[k] = need_f ? u->wpack + u->wf_off[i] : nullptr;
      pb.wd[k] = need_d && !tiled ? u->wpack + u->wd_off[i] : nullptr;
      pb.cout[k] = d.cout; pb.cin[k] = d.cin; pb.cin_real[k] = d.cin_real;
    }
    if (u->wino_f[i] || u->wino_d[i]) {
      const int k = wb.count++;
      wb.w[k] = P[TDX_P_UNIT0 + 4 * i];
      wb.uf[k] = u->wino_f[i] ? u->upack + u->uf_off[i] : nullptr;
      wb.ud[k] = u->wino_d[i] ? u->upack + u->ud_off[i] : nullptr;
      wb.cout[k] = d.cout; wb.cin[k] = d.cin; wb.cin_real[k] = d.cin_real;
    }
  }
  if (pb.count) {
    auto pack = u->precision == TDX_PREC_BF16 ? tdx_pack_conv3x3_batch_bf16 : tiled ? tdx_pack_conv3x3_tiled_batch : tdx_pack_conv3x3_batch;
    int rc = pack(&pb, stream);
    if (rc) return rc;
  }
  if (wb.count) return tdx_pack_conv3x3_wino_batch(&wb, stream);
  return 0;
}

static int pack_impl(tdx_unet* u, const void* const* params, void* const* buffers,
                     tdx_stream_t stream, bool overlap = false, int train_batch = 0) {
  const float* const* P = reinterpret_cast<const float* const*>(params);
  if (!u->spec) {
    if (buffers) {
      int rc = tdx_latent_pack(P, buffers, u->infer_ss, to_stream(stream));
      if (rc) return rc;
    }
    u->packed = buffers != nullptr;
    ++u->pack_gen;
    return 0;
  }
  // INFER pack of the fp32 mode: tile-major, forward only (knob "infer_ring")
  const bool tiled = buffers && !overlap && u->precision != TDX_PREC_BF16 && g_knobs.infer_ring;
  u->wf_tiled = tiled;
  decide_wino(u, train_batch, train_batch > 0);
  // overlap: head now; the tail is launched by pack_tail() once the main stream has MFMA work in flight
  // (beside the tiny kernels at the start of a step it only slowed them down)
  {
    int rc = pack_units(u, P, 0, overlap ? 2 : 13, stream, tiled, buffers != nullptr && !overlap);
    if (rc) return rc;
  }
  for (int i = 0; i < 13; ++i) {
    const UnitDef& d = u->spec->units[i];
    int rc = 0;
    if (buffers) {
      float* ss = u->infer_ss + u->iss_off[i];
      rc = tdx_bn_finalize(nullptr, 0, 0, 0, d.cout, P[TDX_P_UNIT0 + 4 * i + 2],
                           P[TDX_P_UNIT0 + 4 * i + 3], (float*)buffers[3 * i],
                           (float*)buffers[3 * i + 1], nullptr, ss, ss + d.cout, nullptr,
                           nullptr, 0, stream);
      if (rc) return rc;
    }
  }
  u->packed = buffers != nullptr;
  ++u->pack_gen;   // sampling tables built for an earlier pack are stale
  return 0;
}

extern "C" int tdx_unet_pack(tdx_unet* u, const void* const* params, void* const* buffers,
                             tdx_stream_t stream) {
  if (!u || !params || !buffers) return TDX_E_BADARG;
  return pack_impl(u, params, buffers, stream);
}

// packs of units 2..12 on the side stream, ordered after what the main stream has enqueued so far.  (Forking the side
// stream with the head's record instead - the packs read nothing of the forward - saves this record and was measured:
// 9.308 against the parent's 9.295 ms per B = 256 step, profiles/r12_event_chain_ab.txt: the packs then start beside
// the step's small head kernels and unit 0.  Not kept.)
static int pack_tail(tdx_unet* u, const void* const* params, tdx_stream_t stream) {
  const float* const* P = reinterpret_cast<const float* const*>(params);
  TDX_HIP(hipEventRecord(u->ev_fork, to_stream(stream)));
  TDX_HIP(hipStreamWaitEvent(u->side, u->ev_fork, 0));
  int rc = pack_units(u, P, 2, 13, reinterpret_cast<tdx_stream_t>(u->side), false, false);
  if (rc) return rc;
  TDX_HIP(helper_record(u, 0, u->ev_pack, &u->seq_pack));
  return 0;
}

#define RC(call)            \
  do {                      \
    int rc__ = (call);      \
    if (rc__) return rc__;  \
  } while (0)

// Half-batch inference (round 4).  A reverse step at n = 16 is ~35 dependent launches: every kernel boundary is a
// ~5 us bubble, every convolution ends in a tail in which a few workgroups hold the chip, and the small kernels
// between the convolutions (split-K reductions, resizes, pools) occupy a handful of CUs.  Samples are independent in
// eval mode (BatchNorm uses running statistics), so the batch is cut in two and the two halves run the same launch
// sequence side by side - the first on the caller's stream, the second on a stream of the plan forked from it and
// joined at the end (legal inside a stream capture: tools/micro/capture_fork_probe.hip, cases 0-11) - each in a
// workspace layout of its own: one half's bubbles, tails and small kernels are covered by the other half's
// convolutions.  Results equal the whole-batch forward up to the summation order of the split-K plans (which
// depend on M); in-kernel noise keeps the whole batch's Philox indexing (PStep::elem0).
static bool infer_halves(const tdx_unet* u, int batch, size_t workspace_bytes, int* b0) {
  if (!u->spec || !u->half_own || u->whole_batch || !g_knobs.sample_halves || batch < 2 || batch < g_knobs.sample_halves_min) return false;
  const int h0 = (batch + 1) / 2;
  if (workspace_bytes < (make_layout(*u->spec, h0).total + make_layout(*u->spec, batch - h0).total) * sizeof(float)) return false;
  *b0 = h0;
  return true;
}

static int unet_forward_impl(tdx_unet* u, const void* const* params, void* const* buffers, const float* x,
                             const int64_t* t, const void* cond, float* out, void* workspace, size_t workspace_bytes,
                             int batch, int mode, tdx_stream_t stream, const PStep& ps);

extern "C" int tdx_unet_forward(tdx_unet* u, const void* const* params, void* const* buffers,
                                const float* x, const int64_t* t, const void* cond, float* out,
                                void* workspace, size_t workspace_bytes, int batch, int mode,
                                tdx_stream_t stream) {
  if (!u || !params || !buffers || !x || !t || !out || !workspace) return TDX_E_BADARG;
  if (batch <= 0 || batch > u->max_batch) return TDX_E_BADARG;
  if (mode < TDX_MODE_TRAIN || mode > TDX_MODE_INFER) return TDX_E_BADARG;
  const bool needs_cond = u->kind == 1 || u->num_classes > 0;
  if (needs_cond != (cond != nullptr)) return TDX_E_BADARG;
  int b0 = 0;
  if (mode == TDX_MODE_INFER && infer_halves(u, batch, workspace_bytes, &b0)) {
    const NetSpec& S = *u->spec;
    if (!u->packed) RC(pack_impl(u, params, buffers, stream));
    hipStream_t st = to_stream(stream);
    const size_t per = (size_t)S.in_ch * S.hw0 * S.hw0;
    const size_t w0 = make_layout(S, b0).total;
    const void* cond1 = !cond ? nullptr
                        : u->kind == 1 ? static_cast<const void*>(static_cast<const float*>(cond) + (size_t)b0 * S.time_dim)
                                       : static_cast<const void*>(static_cast<const int64_t*>(cond) + b0);
    PStep ps0 = u->ps, ps1 = u->ps;
    if (ps1.x) {
      ps1.x += b0 * per;
      if (ps1.z) ps1.z += b0 * per;
      ps1.elem0 = (int64_t)(b0 * per);
      ps1.counter_dec = nullptr;   // the step counter is advanced once, by the first half's last kernel: the step's head
                                   // kernel read it before the fork, the next step's reads it after the join
    }
    TDX_HIP(hipEventRecord(u->ev_h_fork, st));
    TDX_HIP(hipStreamWaitEvent(u->half_own, u->ev_h_fork, 0));
    RC(unet_forward_impl(u, params, buffers, x, t, cond, out, workspace, w0 * sizeof(float), b0, mode, stream, ps0));
    RC(unet_forward_impl(u, params, buffers, x + b0 * per, t + b0, cond1, out + b0 * per,
                         reinterpret_cast<float*>(workspace) + w0, workspace_bytes - w0 * sizeof(float), batch - b0, mode,
                         reinterpret_cast<tdx_stream_t>(u->half_own), ps1));
    TDX_HIP(hipEventRecord(u->ev_h_join, u->half_own));
    TDX_HIP(hipStreamWaitEvent(st, u->ev_h_join, 0));
    return 0;
  }
  return unet_forward_impl(u, params, buffers, x, t, cond, out, workspace, workspace_bytes, batch, mode, stream, u->ps);
}

static int unet_forward_impl(tdx_unet* u, const void* const* params, void* const* buffers, const float* x,
                             const int64_t* t, const void* cond, float* out, void* workspace, size_t workspace_bytes,
                             int batch, int mode, tdx_stream_t stream, const PStep& ps) {
  if (!u->spec) {  // latent MLP
    if (workspace_bytes < tdx_latent_workspace_floats(batch) * sizeof(float)) return TDX_E_WORKSPACE;
    if (mode == TDX_MODE_INFER && !u->packed) {
      int rc = pack_impl(u, params, buffers, stream);
      if (rc) return rc;
    }
    int rc = tdx_latent_forward(reinterpret_cast<const float* const*>(params), buffers, x, t,
                                static_cast<const int64_t*>(cond), out, reinterpret_cast<float*>(workspace), batch,
                                mode, u->infer_ss, to_stream(stream), u->precision == TDX_PREC_BF16);
    if (rc) return rc;
    u->saved_batch = mode == TDX_MODE_INFER ? 0 : batch;
    u->saved_mode = mode;
    u->saved_precision = u->precision;
    return 0;
  }
  const NetSpec& S = *u->spec;
  const Layout L = make_layout(S, batch);
  if (workspace_bytes < L.total * sizeof(float)) return TDX_E_WORKSPACE;
  const float* const* P = reinterpret_cast<const float* const*>(params);
  float* ws = reinterpret_cast<float*>(workspace);
  hipStream_t st = to_stream(stream);
  u->side = u->use_streams == 1 ? u->side_own : st;
  u->side2 = u->use_streams ? u->side2_own : st;
  const int B = batch;
  const bool infer = mode == TDX_MODE_INFER;
  const bool training = mode == TDX_MODE_TRAIN;
  const int64_t* labels = u->kind == 0 ? static_cast<const int64_t*>(cond) : nullptr;
  const float* cond_emb = u->kind == 1 ? static_cast<const float*>(cond) : nullptr;

  const bool bf16 = u->precision == TDX_PREC_BF16;
  const int io16 = bf16 ? u->io16 : 0;
  if (!infer) RC(pack_impl(u, params, nullptr, stream, true, B));  // weights change every step
  else if (!u->packed) RC(pack_impl(u, params, buffers, stream));
  if (!infer) {
    // keep the inputs for backward (caller tensors may be gone by then): ONE copy kernel on the compute stream for
    // x, t and the labels.  A kernel's writes are released at its end and acquired by the next kernel like every
    // other tensor of the step; the agent-scope loads of the readers stay as a second line of defence.
    const size_t nx = (size_t)B * S.hw0 * S.hw0 * S.in_ch;
    const float* src[3] = {x, reinterpret_cast<const float*>(t), reinterpret_cast<const float*>(labels)};
    float* dst[3] = {ws + L.x, ws + L.t, ws + L.y};
    const size_t cnt[3] = {nx, 2 * (size_t)B, labels ? 2 * (size_t)B : 0};
    RC(tdx_copy_segments(src, dst, cnt, 3, st));
  }

  // The time / class MLP feeds only the skip branches (t_k is added where e_k is resized into the decoder's
  // concat buffer) and the backward: in the training modes all of that lives on the third stream, so the MLP
  // runs there too, beside initial_conv and the first encoder level (LAION, 768 wide: 90 us off the head
  // of the step).  Sampling is one stream.
  hipStream_t tst = st;
  if (!infer) caller_begin(u, st, true);
  if (!infer && u->side2 != st) {
    TDX_HIP(hipEventRecord(u->ev_fork, st));   // t / labels / cond are in place
    TDX_HIP(hipStreamWaitEvent(u->side2, u->ev_fork, 0));
    tst = u->side2;
  }
  if (!(infer && u->skip_time_path))   // table-mode sampling: the step's head kernel has written tp[0..2] already
    RC(tdx_time_embed_fwd(u->kind, t, labels, cond_emb, P, ws + L.sin, ws + L.pre, ws + L.emb, ws + L.tp[0],
                          ws + L.tp[1], ws + L.tp[2], B, tst, S.time_dim));
  RC(tdx_initial_conv_fwd(x, P[TDX_P_INIT_W], P[TDX_P_INIT_B], ws + L.x0, B, S.hw0, S.hw0, S.in_ch,
                          S.x0_real, st, io16));

  // scale/shift of unit i as seen by its consumers (null in INFER mode: already applied)
  auto sc = [&](int i) -> const float* { return infer ? nullptr : ws + L.ss[i]; };
  auto sh = [&](int i) -> const float* { return infer ? nullptr : ws + L.ss[i] + S.units[i].cout; };

  // tile partials of unit i -> scale / shift / saved mean, rstd / running statistics; with a SyncBN callback
  // installed (train mode) the per-channel moments go through the caller's all-reduce first
  auto finalize_bn = [&](int i, int tiles, int tile_rows, int64_t count) -> int {
    const UnitDef& d = S.units[i];
    float* ss = ws + L.ss[i];
    if (training && u->bn_sync) {
      RC(tdx_bn_moments(ws + L.stats, tiles, tile_rows, count, d.cout, u->bn_sync_buf, st));
      RC(u->bn_sync(u->bn_sync_user, u->bn_sync_buf, 2 * d.cout + 1, stream));
      return tdx_bn_finalize_moments(u->bn_sync_buf, d.cout, P[TDX_P_UNIT0 + 4 * i + 2], P[TDX_P_UNIT0 + 4 * i + 3],
                                     (float*)buffers[3 * i], (float*)buffers[3 * i + 1], (int64_t*)buffers[3 * i + 2],
                                     ss, ss + d.cout, ss + 2 * d.cout, ss + 3 * d.cout, st);
    }
    return tdx_bn_finalize(ws + L.stats, tiles, tile_rows, count, d.cout, P[TDX_P_UNIT0 + 4 * i + 2],
                           P[TDX_P_UNIT0 + 4 * i + 3], (float*)buffers[3 * i], (float*)buffers[3 * i + 1],
                           (int64_t*)buffers[3 * i + 2], ss, ss + d.cout, ss + 2 * d.cout, ss + 3 * d.cout,
                           training ? 1 : 0, stream);
  };

  // INFER (sampling) extras of a unit: `defer` = leave a split-K result unreduced for the resize kernel that reads it
  // (units 6, 8, 10, 12: nothing else reads their output), `pool` = let the reduction do the max-pool that follows
  // (units 3, 5 at small batches) - one launch less each, ~5 us of a ~550 us step (TdxSplitDefer / TdxPoolFuse)
  auto run_unit = [&](int i, const float* in, TdxSplitDefer* defer = nullptr, TdxPoolFuse* pool = nullptr) -> int {
    const UnitDef& d = S.units[i];
    const float* wf = u->wpack + u->wf_off[i];
    const float* bias = P[TDX_P_UNIT0 + 4 * i + 1];
    float* Y = ws + L.Y[i];
    float* ss = ws + L.ss[i];
    if (bf16) {
      // bf16 operands, fp32 accumulate.  bf16 storage (round 3): relu(bn(Y)) of a unit that feeds another convolution
      // directly is written out once (25 us of HBM time on the largest layer) instead of being recomputed by the
      // consumer's staging path - at the bf16 matrix rate the transform's ~128 VALU instructions per K-tile were as long
      // as the K-tile's MFMAs (forward launches with BN on load: +50 % over the same shapes with a raw input)
      const int64_t M = (int64_t)B * d.hw * d.hw;
      const bool mat16 = io16 && u->materialize && g_knobs.bf16_materialize;
      if (infer) {
        const float* iss = u->infer_ss + u->iss_off[i];
        return tdx_conv3x3_fwd_bf16_io(in, wf, bias, Y, B, d.hw, d.hw, d.cin, d.cout, TDX_CONV_OUT_BNRELU, nullptr,
                                       nullptr, iss, iss + d.cout, nullptr, io16, stream);
      }
      const bool on_load = d.in_bn && !mat16;
      if (d.in_bn && mat16) in = ws + L.A[i - 1];
      const int fl = (on_load ? TDX_CONV_IN_BNRELU : 0) | (training ? TDX_CONV_OUT_STATS : 0);
      RC(tdx_conv3x3_fwd_bf16_io(in, wf, bias, Y, B, d.hw, d.hw, d.cin, d.cout, fl, on_load ? sc(i - 1) : nullptr,
                                 on_load ? sh(i - 1) : nullptr, nullptr, nullptr, ws + L.stats, io16, stream));
      const int rows = tdx_conv3x3_bf16_stat_tile_rows();
      RC(finalize_bn(i, cdiv(M, rows), rows, M));
      if (mat16 && i + 1 < 13 && S.units[i + 1].in_bn)
        RC(tdx_bn_relu_apply(Y, ws + L.A[i], M, d.cout, ss, ss + d.cout, st, 1));
      return 0;
    }
    if (infer) {
      const float* iss = u->infer_ss + u->iss_off[i];
      // small-batch sampling is latency-bound: split K over more workgroups where the tile
      // grid would not fill the chip; the (unused in INFER mode) gradient buffers are the scratch.
      // Winograd where the launch is big enough to pay for its fixed costs (tdx_conv3x3_infer_algo)
      if (u->wino_f[i] && tdx_conv3x3_infer_algo(B, d.hw, d.hw, d.cin, d.cout))
        return tdx_conv3x3_fwd_wino_infer_ex(in, u->upack + u->uf_off[i], bias, Y, B, d.hw, d.hw, d.cin, d.cout, iss,
                                             iss + d.cout, ws + L.G1, 2 * L.gbuf, stream, defer, pool);
      if (u->wf_tiled)
        return tdx_conv3x3_fwd_infer_ex(in, wf, bias, Y, B, d.hw, d.hw, d.cin, d.cout, iss, iss + d.cout, ws + L.G1,
                                        2 * L.gbuf, stream, defer, pool);
      return tdx_conv3x3_fwd_splitk_fused(in, wf, bias, Y, B, d.hw, d.hw, d.cin, d.cout, TDX_CONV_OUT_BNRELU, iss,
                                          iss + d.cout, ws + L.G1, 2 * L.gbuf, stream, defer, pool);
    }
    const bool bn_on_load = d.in_bn && !u->materialize;
    if (d.in_bn && u->materialize) in = ws + L.A[i - 1];
    int flags = (bn_on_load ? TDX_CONV_IN_BNRELU : 0) | (training ? TDX_CONV_OUT_STATS : 0);
    if (u->wino_f[i] && !bn_on_load) {   // Winograd F(2x2,3x3): its own statistics tiling (256 output pixels per workgroup)
      RC(tdx_conv3x3_fwd_wino(in, u->upack + u->uf_off[i], bias, Y, B, d.hw, d.hw, d.cin, d.cout,
                              training ? TDX_CONV_OUT_STATS : 0, nullptr, nullptr, ws + L.stats, stream));
      RC(finalize_bn(i, tdx_conv3x3_wino_stat_tiles(B, d.hw, d.hw), tdx_conv3x3_wino_stat_tile_rows(B, d.hw, d.hw),
                     (int64_t)B * d.hw * d.hw));
      if (u->materialize && i + 1 < 13 && S.units[i + 1].in_bn)
        RC(tdx_bn_relu_apply(Y, ws + L.A[i], (int64_t)B * d.hw * d.hw, d.cout, ss, ss + d.cout, st));
      return 0;
    }
    if (bn_on_load)
      RC(tdx_conv3x3_fwd(in, wf, bias, Y, B, d.hw, d.hw, d.cin, d.cout, flags, sc(i - 1), sh(i - 1), nullptr, nullptr,
                         ws + L.stats, stream));
    else  // raw input: shapes that would put one lone workgroup on a CU split K (tdx_conv3x3_fwd_train)
      RC(tdx_conv3x3_fwd_train(in, wf, bias, Y, B, d.hw, d.hw, d.cin, d.cout, flags, ws + L.stats, ws + L.ksplit,
                               L.ksplit_floats, stream));
    const int tiles = tdx_conv3x3_stat_tiles(B, d.hw, d.hw, d.cin, d.cout);
    RC(finalize_bn(i, tiles, tdx_conv3x3_stat_tile_rows(B, d.hw, d.hw, d.cin, d.cout), (int64_t)B * d.hw * d.hw));
    if (u->materialize && i + 1 < 13 && S.units[i + 1].in_bn)
      RC(tdx_bn_relu_apply(Y, ws + L.A[i], (int64_t)B * d.hw * d.hw, d.cout, ss, ss + d.cout, st));
    return 0;
  };

  // encoder: two units per level, then 2x2 max-pool of relu(bn(.))
  RC(run_unit(0, ws + L.x0));
  if (!infer) RC(pack_tail(u, params, stream));  // beside unit 1's convolution
  for (int k = 0; k < 3; ++k) {
    const int ua = 2 * k, ub = 2 * k + 1;
    if (k == 1 && !infer) TDX_HIP(caller_wait(u, st, 0, u->ev_pack, u->seq_pack));  // packs of units 2..12
    if (k > 0) RC(run_unit(ua, ws + L.ep[k - 1]));
    TdxPoolFuse pf{infer && !bf16 && (g_knobs.sample_fuse & 2) ? ws + L.ep[k] : nullptr};
    RC(run_unit(ub, ws + L.Y[ua], nullptr, pf.pooled ? &pf : nullptr));
    if (!infer) {
      // the skip branch resize(e_k + t_k) -> second half of the decoder's concat buffer only needs
      // this unit: do it now on the third stream, beside the rest of the encoder
      const int kd = 2 - k, ud = 7 + 2 * kd;  // decoder level / its first unit
      const UnitDef& dd = S.units[ud];
      const int c_up = S.units[kd == 0 ? 6 : 6 + 2 * kd].cout;
      TDX_HIP(hipEventRecord(u->ev_s2_fork[k], st));
      TDX_HIP(hipStreamWaitEvent(u->side2, u->ev_s2_fork[k], 0));
      RC(tdx_bilinear_ac_fwd_t(ws + L.Y[ub], sc(ub), sh(ub), ws + L.tp[k], ws + L.cat[kd], B, S.enc_hw[k],
                               S.enc_hw[k], dd.hw, dd.hw, S.skip_ch[k], dd.cin, c_up, io16,
                               reinterpret_cast<tdx_stream_t>(u->side2)));
      TDX_HIP(helper_record(u, 1, u->ev_s2_done[k], &u->seq_s2[k]));
    }
    if (!pf.pooled)   // (null also when the convolution was not split: its reduction could not do the pooling)
      RC(tdx_maxpool2_ceil_fwd_t(ws + L.Y[ub], sc(ub), sh(ub), ws + L.ep[k], B, S.enc_hw[k], S.enc_hw[k],
                                 S.skip_ch[k], io16, stream));
  }
  const bool defer_ok = infer && !bf16 && (g_knobs.sample_fuse & 1);
  TdxSplitDefer dfr{};   // the deferred result of the unit about to be resized (6, 8, 10, then 12)
  RC(run_unit(6, ws + L.ep[2], defer_ok ? &dfr : nullptr));
  // decoder level k (0: dec3 .. 2: dec1): cat = [up(previous) | resize(e + t)], diffusion.py:135-154
  for (int k = 0; k < 3; ++k) {
    const int ua = 7 + 2 * k, ub = 8 + 2 * k;   // dec units of this level
    const int prev = k == 0 ? 6 : 6 + 2 * k;    // unit whose activation is up-sampled (6, 8, 10)
    const int skip_u = 5 - 2 * k;               // encoder unit feeding the skip (5, 3, 1)
    const int skip_k = 2 - k;                   // index into skip_ch / tp
    const UnitDef& da = S.units[ua];
    const UnitDef& dp = S.units[prev];
    const int hw = da.hw, c_up = dp.cout, c_skip = S.skip_ch[skip_k];
    if (infer) {  // both halves in one launch (post-activation tensors: nothing to apply on load)
      RC(tdx_bilinear_pair_fwd_ex(ws + L.Y[prev], &dfr, dp.hw, dp.hw, c_up, ws + L.Y[skip_u], ws + L.tp[skip_k],
                                  S.enc_hw[skip_k], S.enc_hw[skip_k], c_skip, ws + L.cat[k], B, hw, hw, st, io16));
      dfr = TdxSplitDefer{};
    } else {
      RC(tdx_bilinear_ac_fwd_t(ws + L.Y[prev], sc(prev), sh(prev), nullptr, ws + L.cat[k], B, dp.hw, dp.hw, hw, hw,
                               c_up, da.cin, 0, io16, stream));
      // skip half: written during the encoder (the first level's wait, for the last resize, covers the other two)
      TDX_HIP(caller_wait(u, st, 1, u->ev_s2_done[skip_k], u->seq_s2[skip_k]));
    }
    RC(run_unit(ua, ws + L.cat[k]));
    RC(run_unit(ub, ws + L.Y[ua], defer_ok ? &dfr : nullptr));
  }
  // resize to the output resolution (identity copy when equal) and the output convolution
  if (dfr.splits > 0)   // sampling: the last unit's split-K partials are reduced by the resize itself
    RC(tdx_bilinear_pair_fwd_ex(nullptr, &dfr, S.dec_hw[2], S.dec_hw[2], 64, nullptr, nullptr, 0, 0, 0, ws + L.d1a, B,
                                S.out_hw, S.out_hw, st));
  else
    RC(tdx_bilinear_ac_fwd_t(ws + L.Y[12], sc(12), sh(12), nullptr, ws + L.d1a, B, S.dec_hw[2], S.dec_hw[2],
                             S.out_hw, S.out_hw, 64, 64, 0, io16, stream));
  if (infer && ps.x)
    RC(tdx_final_conv_fwd_psample(ws + L.d1a, P[TDX_P_FINAL_W], P[TDX_P_FINAL_B], out, B, S.out_hw, S.out_hw, S.in_ch,
                                  ps, st, io16));
  else
    RC(tdx_final_conv_fwd(ws + L.d1a, P[TDX_P_FINAL_W], P[TDX_P_FINAL_B], out, B, S.out_hw, S.out_hw, S.in_ch, st, io16));

  u->saved_batch = infer ? 0 : B;
  if (!infer) u->g_x = nullptr;   // a request belongs to the backward of the forward it was made after
  u->saved_mode = mode;
  u->saved_precision = u->precision;
  u->saved_io16 = io16;
  return 0;
}

static int unet_backward_impl(tdx_unet* u, const void* const* params, void* const* grads, const float* d_out,
                              void* workspace, size_t workspace_bytes, int batch, int stage_lo, int stage_hi,
                              tdx_stream_t stream);

extern "C" int tdx_unet_backward(tdx_unet* u, const void* const* params, void* const* grads,
                                 const float* d_out, void* workspace, size_t workspace_bytes,
                                 int batch, int stage_lo, int stage_hi, tdx_stream_t stream) {
  if (!u || !params || !grads || !d_out || !workspace) return TDX_E_BADARG;
  const int rc = unet_backward_impl(u, params, grads, d_out, workspace, workspace_bytes, batch, stage_lo, stage_hi, stream);
  // a one-shot d loss / d x request (tdx_unet_request_input_grad) dies with the call that fails: the caller's
  // buffer may be gone by the time another backward reaches the last stage
  if (rc) u->g_x = nullptr;
  return rc;
}

static int unet_backward_impl(tdx_unet* u, const void* const* params, void* const* grads, const float* d_out,
                              void* workspace, size_t workspace_bytes, int batch, int stage_lo, int stage_hi,
                              tdx_stream_t stream) {
  if (batch != u->saved_batch || u->saved_mode == TDX_MODE_INFER || u->saved_mode < 0) return TDX_E_STATE;
  if (stage_lo < 0 || stage_hi > N_STAGES || stage_lo >= stage_hi) return TDX_E_BADARG;
  if (!u->spec) {
    if (workspace_bytes < tdx_latent_workspace_floats(batch) * sizeof(float)) return TDX_E_WORKSPACE;
    return tdx_latent_backward(reinterpret_cast<const float* const*>(params), reinterpret_cast<float* const*>(grads),
                               d_out, reinterpret_cast<float*>(workspace), batch,
                               u->saved_mode == TDX_MODE_TRAIN ? 1 : 0, stage_lo, stage_hi, u->num_classes,
                               to_stream(stream), u->saved_precision == TDX_PREC_BF16);
  }
  const NetSpec& S = *u->spec;
  const Layout L = make_layout(S, batch);
  if (workspace_bytes < L.total * sizeof(float)) return TDX_E_WORKSPACE;
  const float* const* P = reinterpret_cast<const float* const*>(params);
  float* const* G = reinterpret_cast<float* const*>(grads);
  float* ws = reinterpret_cast<float*>(workspace);
  hipStream_t st = to_stream(stream);
  u->side = u->use_streams == 1 ? u->side_own : st;
  u->side2 = u->use_streams ? u->side2_own : st;
  const int B = batch;
  const int training = u->saved_mode == TDX_MODE_TRAIN ? 1 : 0;
  if (u->precision != u->saved_precision) return TDX_E_STATE;  // backward in the precision of its forward
  const bool bf16 = u->saved_precision == TDX_PREC_BF16;
  const int io16 = u->saved_io16;
  // Activation gradients rotate through FOUR buffers, handed out least-recently-used: the weight
  // gradient of unit u (side stream) keeps reading dy(u) while the main stream is already two
  // units further down, so the two streams are coupled loosely - the side stream works through
  // its queue of wgrad GEMMs back to back and fills the gaps the main stream's HBM-bound
  // BN / pool / resize kernels would otherwise leave on the matrix cores.  (With two ping-pong
  // buffers every dgrad had to wait for the previous unit's wgrad: lockstep.)
  typedef tdx_unet::GBuf GBuf;
  GBuf* gb = u->gb;
  int& clock = u->clock;
  if (stage_lo == 0) {
    float* base[4] = {ws + L.G1, ws + L.G2, ws + L.G3, ws + L.G4};
    for (int i = 0; i < 4; ++i) gb[i] = GBuf{base[i], -1, -1, 0};
    clock = 0;
    for (int i = 0; i < 13; ++i) u->red_pending[i] = false;
    u->bw_unit = -1;
  } else if (gb[0].p != ws + L.G1) {
    return TDX_E_STATE;  // another workspace than the one stage 0 ran on
  }
  auto find = [&](const float* p) -> GBuf* {
    for (int i = 0; i < 4; ++i)
      if (gb[i].p == p) return &gb[i];
    return nullptr;
  };
  auto touch = [&](const float* p) { if (GBuf* b = find(p)) b->age = ++clock; };
  // a buffer to overwrite: not `a`, not `b`; waits (on the main stream) for its last readers
  auto acquire = [&](const float* a, const float* b, float** out) -> int {
    GBuf* best = nullptr;
    for (int i = 0; i < 4; ++i) {
      GBuf& c = gb[i];
      if (c.p != a && c.p != b && (!best || c.age < best->age)) best = &c;
    }
    if (best->w_unit >= 0) TDX_HIP(caller_wait(u, st, 0, u->ev_w[best->w_unit], u->seq_w[best->w_unit]));
    if (best->s2 >= 0) TDX_HIP(caller_wait(u, st, 1, u->ev_s2_done[best->s2], u->seq_s2[best->s2]));
    best->w_unit = -1;
    best->s2 = -1;
    best->age = ++clock;
    *out = best->p;
    return 0;
  };
  if (stage_lo > 0 && !find(u->g_next)) return TDX_E_STATE;  // stages must be run in order after a forward
  float* g_next = u->g_next;

  tdx_stream_t side = reinterpret_cast<tdx_stream_t>(u->side);
  // Stream capture (TrainStep(use_graph=True)).  The eager schedule makes the two helper streams wait for
  // EACH OTHER (slab reduction on the third stream behind the weight-gradient GEMM of the second; the GEMM
  // two units later behind that reduction, whose slab buffer it overwrites) while both are also forked from
  // the caller's stream.  That is legal under the rules of capture - every event waited for is recorded
  // inside the capture, both helpers are joined before EndCapture - but hipStreamEndCapture of ROCm 7.2
  // dies on it with a segmentation fault.  tools/micro/capture_fork_probe.hip reproduces it without libtdx
  // (case 12: this function's event sequence with one-line kernels) and bisects it: any ONE of the two
  // cross-helper waits removed, or the third stream's forks from the caller's stream removed, and the
  // capture ends and replays correctly; origin <-> helper forks and joins alone are fine in every
  // combination tried (cases 0-11).  So inside a capture the reduction runs on the GEMM's own stream:
  // no helper ever waits for the other, everything else (three streams, the same kernels, the same
  // summation orders, bit-identical results) stays.
  hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cap_status);
  const bool capturing = cap_status == hipStreamCaptureStatusActive;
  caller_begin(u, st, false);
  // The slab reduction of unit i's weight gradient: third stream - or, while the step is being CAPTURED, right
  // behind the GEMM on its own stream (see above), which needs neither of the two cross-helper waits.
  auto slab_reduce = [&](int i) -> int {
    const UnitDef& d = S.units[i];
    const bool mat = u->materialize && (!bf16 || (io16 && g_knobs.bf16_materialize));
    const bool wino = u->wino_w[i] && !(d.in_bn && !mat);
    float* slab = ws + ((i & 1) ? L.slabs2 : L.slabs);
    hipStream_t wst = u->side;
    hipStream_t red_st = capturing ? wst : u->side2;
    if (red_st != wst) TDX_HIP(hipStreamWaitEvent(red_st, u->ev_w[i], 0));
    RC(tdx_conv3x3_wgrad_reduce_pad(slab, G[TDX_P_UNIT0 + 4 * i],
                                    bf16 ? tdx_conv3x3_wgrad_splits_bf16(B, d.hw, d.hw, d.cin, d.cout)
                                    : wino ? tdx_conv3x3_wgrad_wino_splits(B, d.hw, d.hw, d.cin, d.cout)
                                           : tdx_conv3x3_wgrad_splits(B, d.hw, d.hw, d.cin, d.cout),
                                    d.cout, d.cin, d.cin_real, reinterpret_cast<tdx_stream_t>(red_st)));
    if (red_st != wst) {
      TDX_HIP(hipEventRecord(u->ev_red[i], red_st));
      u->red_pending[i] = true;
    }
    return 0;
  };
  // unit_bwd: g_next holds dL/d(activation of unit i); afterwards that buffer holds
  // dL/d(conv output) (read by the wgrad on the side stream) and *g_in_out the input gradient.
  // reduce_later: the caller enqueues slab_reduce(i) itself, behind work the third stream must not keep waiting
  // for this unit's weight gradient (dec_level_bwd)
  auto unit_bwd = [&](int i, const float* in, float** g_in_out, bool reduce_later = false) -> int {
    const UnitDef& d = S.units[i];
    float* g = g_next;
    const float* ss = ws + L.ss[i];
    const int64_t rows = (int64_t)B * d.hw * d.hw;
    if (u->bw_unit == i && u->bw_nblk > 0) {
      // the kernel that wrote g (the input-gradient convolution of the unit above, a resize adjoint or a max-pool
      // backward) left this unit's partial sums in bnscr: no reduction pass over (g, y)
      RC(tdx_bn_relu_bwd_tail(g, ws + L.Y[i], rows, d.cout, ss, ss + d.cout, ss + 2 * d.cout, ss + 3 * d.cout,
                              P[TDX_P_UNIT0 + 4 * i + 2], G[TDX_P_UNIT0 + 4 * i + 2], G[TDX_P_UNIT0 + 4 * i + 3],
                              G[TDX_P_UNIT0 + 4 * i + 1], ws + L.bnscr, u->bw_nblk,
                              ws + L.bnscr + (size_t)u->bw_nblk * 2 * d.cout, training,
                              training ? u->bn_sync : nullptr, u->bn_sync_user, u->bn_sync_buf, stream, io16));
    } else {
      RC(tdx_bn_relu_bwd_sync(g, ws + L.Y[i], rows, d.cout, ss, ss + d.cout, ss + 2 * d.cout,
                              ss + 3 * d.cout, P[TDX_P_UNIT0 + 4 * i + 2], G[TDX_P_UNIT0 + 4 * i + 2],
                              G[TDX_P_UNIT0 + 4 * i + 3], G[TDX_P_UNIT0 + 4 * i + 1], ws + L.bnscr, training,
                              training ? u->bn_sync : nullptr, u->bn_sync_user, u->bn_sync_buf, stream, io16));
    }
    u->bw_unit = -1;
    // Weight gradient: forked to the side stream (which IS the main stream for networks whose
    // NetSpec says overlap = 0).
    const bool mat = u->materialize && (!bf16 || (io16 && g_knobs.bf16_materialize));
    const bool bn_on_load = d.in_bn && !mat;
    if (d.in_bn && mat) in = ws + L.A[i - 1];  // materialised relu(bn(Y[i-1]))
    const float* isc = bn_on_load ? ws + L.ss[i - 1] : nullptr;
    const float* ish = bn_on_load ? ws + L.ss[i - 1] + S.units[i - 1].cout : nullptr;
    const bool fork = true;
    float* slab = ws + ((i & 1) ? L.slabs2 : L.slabs);
    // The split-K slabs alternate between two buffers; the (HBM-bound) slab reduction runs on the
    // third stream.  Unit i's slab buffer was last read by the reduction of unit i+2.
    hipStream_t wst = fork ? u->side : st;
    if (fork) {
      TDX_HIP(hipEventRecord(u->ev_dy[i], st));
      TDX_HIP(hipStreamWaitEvent(u->side, u->ev_dy[i], 0));
    }
    if (i + 2 < 13 && u->red_pending[i + 2]) {
      TDX_HIP(hipStreamWaitEvent(wst, u->ev_red[i + 2], 0));
      u->red_pending[i + 2] = false;
    }
    if (bf16)
      RC(tdx_conv3x3_wgrad_bf16_io(in, g, slab, B, d.hw, d.hw, d.cin, d.cout, bn_on_load ? TDX_CONV_IN_BNRELU : 0, isc,
                                   ish, io16, reinterpret_cast<tdx_stream_t>(wst)));
    else if (u->wino_w[i] && !bn_on_load)
      RC(tdx_conv3x3_wgrad_wino(in, g, slab, B, d.hw, d.hw, d.cin, d.cout, reinterpret_cast<tdx_stream_t>(wst)));
    else
      RC(tdx_conv3x3_wgrad(in, g, slab, B, d.hw, d.hw, d.cin, d.cout, bn_on_load ? TDX_CONV_IN_BNRELU : 0, isc, ish,
                           reinterpret_cast<tdx_stream_t>(wst)));
    // dy is free again once the wgrad GEMM has read it
    TDX_HIP(helper_record(u, 0, u->ev_w[i], &u->seq_w[i]));
    if (!reduce_later) RC(slab_reduce(i));
    GBuf* gbuf = find(g);
    gbuf->w_unit = i;
    gbuf->age = ++clock;
    // main: input gradient = the forward kernel on the flipped pack, channels swapped
    float* g_in;
    RC(acquire(g, nullptr, &g_in));
    if (bf16)
      RC(tdx_conv3x3_fwd_bf16_io(g, u->wpack + u->wd_off[i], nullptr, g_in, B, d.hw, d.hw, d.cout, d.cin, 0, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, io16, stream));
    else if (u->wino_d[i])   // Winograd on the mirrored, channel-swapped pack
      RC(tdx_conv3x3_fwd_wino(g, u->upack + u->ud_off[i], nullptr, g_in, B, d.hw, d.hw, d.cout, d.cin, 0, nullptr, nullptr,
                              nullptr, stream));
    else if (d.in_bn) {
      // g_in is dL/d(activation) of unit i-1 (same resolution, no pool / resize in between): its BatchNorm backward
      // comes next, and this launch's epilogue leaves that unit's partial sums behind (nblk = 0: not on this path)
      const float* pss = ws + L.ss[i - 1];
      int nblk = 0;
      RC(tdx_conv3x3_dgrad_bnbwd(g, u->wpack + u->wd_off[i], g_in, B, d.hw, d.hw, d.cout, d.cin, ws + L.Y[i - 1], pss,
                                 pss + d.cin, pss + 2 * d.cin, pss + 3 * d.cin, ws + L.bnscr, &nblk, ws + L.ksplit,
                                 L.ksplit_floats, stream));
      if (nblk > 0) { u->bw_unit = i - 1; u->bw_nblk = nblk; }
    } else
      RC(tdx_conv3x3_fwd_train(g, u->wpack + u->wd_off[i], nullptr, g_in, B, d.hw, d.hw, d.cout, d.cin, 0, nullptr,
                               ws + L.ksplit, L.ksplit_floats, stream));
    *g_in_out = g_in;
    return 0;
  };
  // the BatchNorm operands of unit i for a producer of its activation gradient (tdx_*_bwd_bn)
  auto bw_y = [&](int i) -> const float* { return ws + L.Y[i]; };
  auto plain_unit_bwd = [&](int i, const float* in) -> int {
    float* g_in;
    RC(unit_bwd(i, in, &g_in));
    g_next = g_in;
    return 0;
  };
  auto ssc = [&](int i) { return ws + L.ss[i]; };
  auto ssh = [&](int i) { return ws + L.ss[i] + S.units[i].cout; };
  // the time / class path's backward on the third stream, in `parts` (internal.h)
  auto time_path_parts = [&](int parts) -> int {
    return tdx_time_embed_bwd(u->kind, u->num_classes > 0 ? reinterpret_cast<const int64_t*>(ws + L.y) : nullptr,
                              P, G, ws + L.sin, ws + L.pre, ws + L.emb, ws + L.gtp[0], ws + L.gtp[1],
                              ws + L.gtp[2], ws + L.timescr, B, u->num_classes, u->side2, S.time_dim, parts);
  };
  // first unit of a decoder level (stages 2, 4, 6 = units 11, 9, 7): after its dgrad the
  // gradient of the concatenated input is split into the up-sampled branch and the skip branch
  auto dec_level_bwd = [&](int k) -> int {  // k = 2 (dec1), 1 (dec2), 0 (dec3)
    const int ua = 7 + 2 * k;
    const int prev = k == 0 ? 6 : 6 + 2 * k;
    const int skip_k = 2 - k;
    const UnitDef& da = S.units[ua];
    const UnitDef& dp = S.units[prev];
    const int c_up = dp.cout, c_skip = S.skip_ch[skip_k];
    // The skip branch's adjoint goes to the third stream BEFORE this unit's slab reduction.  Behind it, it waited for
    // this unit's weight gradient, which the side stream reaches late: at the innermost level the very next stage
    // needs GS (max-pool backward), and the main stream stood idle for ~100 us of a B = 256 MNIST step
    // (profiles/r12_step_timeline_before.txt, 6193.7 .. 6296.0; afterwards 11.6 us).  Not inside a capture, where
    // the reduction is not on the third stream.
    const bool reduce_later = !capturing;
    float* gcat;
    RC(unit_bwd(ua, ws + L.cat[k], &gcat, reduce_later));
    // skip branch (needed only when the encoder is reached): third stream
    TDX_HIP(hipEventRecord(u->ev_s2_fork[k], st));
    TDX_HIP(hipStreamWaitEvent(u->side2, u->ev_s2_fork[k], 0));
    {
      int unused = 0;   // (no BatchNorm follows the skip branch: the plain adjoint, in the storage type)
      RC(tdx_bilinear_ac_bwd_bn(gcat, ws + L.GS[skip_k], B, S.enc_hw[skip_k], S.enc_hw[skip_k], da.hw, da.hw, c_skip,
                                da.cin, c_up, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &unused,
                                reinterpret_cast<tdx_stream_t>(u->side2), io16));
    }
    RC(tdx_pixel_sum(ws + L.GS[skip_k], ws + L.gtp[skip_k], B, S.enc_hw[skip_k] * S.enc_hw[skip_k], c_skip,
                     u->side2, io16));
    TDX_HIP(helper_record(u, 1, u->ev_s2_done[k], &u->seq_s2[k]));
    if (reduce_later) RC(slab_reduce(ua));
    // this projection's weight gradient and its share of g(emb) as soon as its pixel sum exists (levels
    // arrive in the order time_proj1, 2, 3 = the summation order of tdx_time_embed_bwd): six of the
    // time path's small kernels leave the tail of the step.  The REST of that path stays after the last
    // stage (see time_path_bwd).
    RC(tdx_time_proj_bwd(u->kind, skip_k, P, G, ws + L.emb, ws + L.gtp[skip_k], ws + L.timescr, B, u->side2,
                         S.time_dim));
    // after the third projection g(emb) is complete: the middle of the time path follows at once (for kind 1
    // that is all of it); only kind 0's first-layer kernel waits for the last stage (see time_path_bwd)
    if (skip_k == 2) RC(time_path_parts(TDX_TIME_MID));
    find(gcat)->s2 = k;
    float* gup;
    RC(acquire(gcat, nullptr, &gup));
    {
      const float* pss = ws + L.ss[prev];
      int nblk = 0;
      RC(tdx_bilinear_ac_bwd_bn(gcat, gup, B, dp.hw, dp.hw, da.hw, da.hw, c_up, da.cin, 0, bw_y(prev), pss, pss + c_up,
                                pss + 2 * c_up, pss + 3 * c_up, ws + L.bnscr, &nblk, stream, io16));
      if (nblk > 0) { u->bw_unit = prev; u->bw_nblk = nblk; }
    }
    touch(gcat);
    g_next = gup;
    return 0;
  };
  // what dec_level_bwd has not issued: kind 0's first-layer kernel, after the last stage, ordered on the third
  // stream behind `st` (kind 1 has no separate first-layer part, its time path is complete after TDX_TIME_MID)
  auto time_path_bwd = [&](hipStream_t st) -> int {
    TDX_HIP(hipEventRecord(u->ev_fork, st));
    TDX_HIP(hipStreamWaitEvent(u->side2, u->ev_fork, 0));
    if (u->kind == 1) return 0;
    return time_path_parts(TDX_TIME_L1);
  };
  // first unit of an encoder level below the top, or the bottleneck (units 6, 4, 2): its input is a
  // pooled tensor; route the gradient through the max-pool and add the skip-path gradient
  auto pooled_unit_bwd = [&](int ui, int k) -> int {  // k: encoder level whose output was pooled (2, 1, 0)
    float* gpool;
    RC(unit_bwd(ui, ws + L.ep[k], &gpool));
    const int ub = 2 * k + 1;  // unit producing the pooled activation (5, 3, 1)
    float* gnew;
    RC(acquire(gpool, nullptr, &gnew));
    // GS[k] was written on the third stream during the decoder
    TDX_HIP(caller_wait(u, st, 1, u->ev_s2_done[2 - k], u->seq_s2[2 - k]));
    {
      const int cu = S.skip_ch[k];
      int nblk = 0;
      RC(tdx_maxpool2_ceil_bwd_bn(ws + L.Y[ub], ssc(ub), ssh(ub), gpool, ws + L.GS[k], gnew, B, S.enc_hw[k],
                                  S.enc_hw[k], cu, ws + L.ss[ub] + 2 * cu, ws + L.ss[ub] + 3 * cu,
                                  ws + L.bnscr, &nblk, stream, io16));
      if (nblk > 0) { u->bw_unit = ub; u->bw_nblk = nblk; }
    }
    touch(gpool);
    g_next = gnew;
    return 0;
  };

  for (int s = stage_lo; s < stage_hi; ++s) {
    switch (s) {
      case 0:  // final_conv + the output resize; its weight gradient is off the critical path
        TDX_HIP(hipEventRecord(u->ev_fork, st));  // d_out is ready on the main stream
        TDX_HIP(hipStreamWaitEvent(u->side, u->ev_fork, 0));
        RC(tdx_final_conv_wgrad(ws + L.d1a, d_out, ws + L.smallp2, G[TDX_P_FINAL_W], G[TDX_P_FINAL_B], B,
                                S.out_hw, S.out_hw, S.in_ch, u->side, io16));
        {
          float *gd1a, *g12;
          RC(acquire(nullptr, nullptr, &gd1a));
          RC(tdx_final_conv_dgrad(d_out, P[TDX_P_FINAL_W], gd1a, B, S.out_hw, S.out_hw, S.in_ch, st, io16));
          if (S.dec_hw[2] == S.out_hw) {  // the output resize is the identity (LAION network): so is its adjoint
            g_next = gd1a;
          } else {
            RC(acquire(gd1a, nullptr, &g12));
            const float* pss = ws + L.ss[12];
            int nblk = 0;
            RC(tdx_bilinear_ac_bwd_bn(gd1a, g12, B, S.dec_hw[2], S.dec_hw[2], S.out_hw, S.out_hw, 64, 64, 0, bw_y(12), pss,
                                      pss + 64, pss + 128, pss + 192, ws + L.bnscr, &nblk, stream, io16));
            if (nblk > 0) { u->bw_unit = 12; u->bw_nblk = nblk; }
            g_next = g12;
          }
        }
        break;
      case 1: RC(plain_unit_bwd(12, ws + L.Y[11])); break;
      case 2: RC(dec_level_bwd(2)); break;
      case 3: RC(plain_unit_bwd(10, ws + L.Y[9])); break;
      case 4: RC(dec_level_bwd(1)); break;
      case 5: RC(plain_unit_bwd(8, ws + L.Y[7])); break;
      case 6: RC(dec_level_bwd(0)); break;
      case 7: RC(pooled_unit_bwd(6, 2)); break;
      case 8: RC(plain_unit_bwd(5, ws + L.Y[4])); break;
      case 9: RC(pooled_unit_bwd(4, 1)); break;
      case 10: RC(plain_unit_bwd(3, ws + L.Y[2])); break;
      case 11: RC(pooled_unit_bwd(2, 0)); break;
      case 12: RC(plain_unit_bwd(1, ws + L.Y[0])); break;
      case 13: RC(plain_unit_bwd(0, ws + L.x0)); break;  // g(x0)
      case 14:
        RC(time_path_bwd(st));
        RC(tdx_initial_conv_wgrad(ws + L.x, g_next, ws + L.smallp, G[TDX_P_INIT_W], G[TDX_P_INIT_B], B, S.hw0,
                                  S.hw0, S.in_ch, S.x0_real, st, io16));
        if (u->g_x) {   // d loss / d x, on request only (tdx_unet_request_input_grad)
          RC(tdx_initial_conv_dgrad(g_next, P[TDX_P_INIT_W], u->g_x, B, S.hw0, S.hw0, S.in_ch, S.x0_real, st, io16));
          u->g_x = nullptr;
        }
        break;
    }
  }
  u->g_next = g_next;
  // After the LAST stage everything the side streams did is ordered before whatever follows on
  // `stream`.  A partial range does not join (the main stream would stall on weight-gradient
  // GEMMs it does not depend on): tdx_unet_backward_join() orders a stream of the caller's
  // choice - the one its gradient all-reduce runs on - after the work enqueued so far.
  if (stage_hi == N_STAGES) return tdx_unet_backward_join(u, stream);
  return 0;
}

// One reverse step: the head (step counter, timestep vector), the forward and the update ps (PStep, internal.h; its
// counter_dec and fused-only fields are set here).  ps.tau == null: the step counter is the timestep t; otherwise a
// schedule of n_steps steps - the counter is the step index k, the coefficient row, and the network runs at tau[k].
// ps.guided: batch = 2n rows of x, the second half under the null condition, n_elems the first half's.  The head, the
// counter and the half-batch logic do not know the update's form; a half-batch launch indexes the one history, known
// and mask by the element's place in the whole batch (PStep::elem0).  ps.thr (dynamic thresholding, dyn_rank / dyn_frac
// the quantile): the bound of a sample needs the whole output, so the epilogue is never armed - after the forward (whose
// half-batch streams have joined) come the threshold launch and the update kernel, which advances the table-mode counter.
static int eval_step_impl(tdx_unet* u, const void* const* params, void* const* buffers, float* x, const void* cond,
                          PStep ps, int n_steps, int64_t* counter, int32_t* t_idx, int64_t* t_vec, float* eps,
                          int64_t n_elems, void* workspace, size_t workspace_bytes, int batch, tdx_stream_t stream,
                          int dyn_rank = 0, float dyn_frac = 0.f) {
  const int64_t* tau = ps.tau;
  const bool guided = ps.guided;
  if (!u || !params || !buffers || !x || !counter || !t_vec || !eps || !workspace || batch <= 0 || ps.t_idx != t_idx)
    return TDX_E_BADARG;   // (params, buffers, workspace: before the head kernel writes anything, not after)
  if (const int rc = pstep_valid(ps, n_elems)) return rc;
  if (guided) {
    if (!u->spec) return TDX_E_SHAPE;   // the UNets only
    if ((batch & 1) || 2 * n_elems != (int64_t)batch * u->spec->in_ch * u->spec->out_hw * u->spec->out_hw) return TDX_E_BADARG;
  }
  // Table mode (tdx_unet_prepare_sampling was called for this pack, batch and cond): ONE head kernel sets t and
  // adds two table rows per sample into the workspace's projection slots - in place of step_begin, the time MLP and
  // the three projections - and the update kernel advances the counter.
  // (an identity table never serves a scheduled step nor the other way round: the schedule pointer and length match)
  const bool tab = u->spec && u->tab && u->packed && u->tab_gen == u->pack_gen && u->tab_batch == batch &&
                   u->tab_cond == cond && u->tab_tau == tau && (!tau || u->tab_T == n_steps) && workspace &&
                   workspace_bytes >= make_layout(*u->spec, batch).total * sizeof(float);
  if (tab) {
    const NetSpec& S = *u->spec;
    const Layout L = make_layout(S, batch);
    float* ws = reinterpret_cast<float*>(workspace);
    const size_t T = (size_t)u->tab_T, w1 = S.skip_ch[0], w2 = S.skip_ch[1], w3 = S.skip_ch[2];
    const float* t1 = u->tab;
    const float* t2 = t1 + T * w1;
    const float* t3 = t2 + T * w2;
    const float* c1 = cond ? t3 + T * w3 : nullptr;
    const float* c2 = cond ? c1 + (size_t)batch * w1 : nullptr;
    const float* c3 = cond ? c2 + (size_t)batch * w2 : nullptr;
    int b0 = 0;
    if (!guided && infer_halves(u, batch, workspace_bytes, &b0)) {   // the forward below runs as two half-batches: each half's projection slots
      const Layout L0 = make_layout(S, b0), L1 = make_layout(S, batch - b0);
      float* ws1 = ws + L0.total;
      RC(tdx_sample_head(counter, t_idx, t_vec, batch, u->tab_T, u->kind, t1, t2, t3, c1, c2, c3, ws + L0.tp[0],
                         ws + L0.tp[1], ws + L0.tp[2], to_stream(stream), b0, ws1 + L1.tp[0], ws1 + L1.tp[1],
                         ws1 + L1.tp[2], tau));
    } else {
      RC(tdx_sample_head(counter, t_idx, t_vec, batch, u->tab_T, u->kind, t1, t2, t3, c1, c2, c3, ws + L.tp[0],
                         ws + L.tp[1], ws + L.tp[2], to_stream(stream), 0, nullptr, nullptr, nullptr, tau));
    }
  } else if (tau) {
    RC(tdx_step_begin_sched(counter, tau, t_idx, t_vec, batch, stream));
  } else {
    RC(tdx_step_begin(counter, t_idx, t_vec, batch, stream));
  }
  u->skip_time_path = tab;
  u->whole_batch = guided;   // (set here, cleared below: no early return in between)
  // the UNets apply the update in final_conv's epilogue (one launch less); the latent MLP keeps the separate kernel
  const bool fuse_ps = u->spec && (g_knobs.sample_fuse & 4) && !ps.thr &&
                       (guided ? 2 : 1) * n_elems == (int64_t)batch * u->spec->in_ch * u->spec->out_hw * u->spec->out_hw;
  ps.counter_dec = tab ? counter : nullptr;
  if (fuse_ps) { u->ps = ps; u->ps.x = x; }
  const int rc = tdx_unet_forward(u, params, buffers, x, t_vec, cond, eps, workspace, workspace_bytes, batch,
                                  TDX_MODE_INFER, stream);
  u->skip_time_path = false;
  u->whole_batch = false;
  u->ps = {};
  if (rc || fuse_ps) return rc;
  if (ps.thr) RC(tdx_x0_threshold_launch(ps, x, eps, (int)(n_elems / ps.per), dyn_rank, dyn_frac, to_stream(stream)));
  // elementwise, so x is updated in place
  return tdx_pstep_launch(ps, x, x, eps, n_elems, to_stream(stream));
}

static PStep eval_pstep(int form, const float* coef, const int32_t* t_idx, const int64_t* tau, const float* z,
                        uint64_t philox_seed, int guided, float w, float lo, float hi, float* hist, const float* known,
                        const float* mask) {
  PStep s{};
  s.form = form; s.coef = coef; s.t_idx = t_idx; s.tau = tau;
  s.z = z; s.philox = !z && form != TDX_STEP_MS; s.seed = philox_seed;   // z == null: in-kernel Philox noise
  s.guided = guided != 0; s.w = w;
  s.lo = lo; s.hi = hi;
  s.hist = hist; s.known = known; s.mask = mask;
  return s;
}

extern "C" int tdx_unet_eval_step(tdx_unet* u, const void* const* params, void* const* buffers, float* x,
                                  const void* cond, const float* z, const float* coef, int64_t* counter,
                                  int32_t* t_idx, int64_t* t_vec, float* eps, int64_t n_elems,
                                  void* workspace, size_t workspace_bytes, int batch, uint64_t philox_seed,
                                  tdx_stream_t stream) {
  return eval_step_impl(u, params, buffers, x, cond,
                        eval_pstep(TDX_STEP_EPS, coef, t_idx, nullptr, z, philox_seed, 0, 0.f, 0.f, 0.f, nullptr, nullptr, nullptr),
                        0, counter, t_idx, t_vec, eps, n_elems, workspace, workspace_bytes, batch, stream);
}

// Every other step (include/tdx.h): a schedule, guidance, the x0 and the multistep form, a known region.  The update
// runs in final_conv's epilogue, or in pstep_kernel when the epilogue is switched off (knob "sample_fuse") and for the
// latent MLP (u->spec == nullptr; the transformer has no plan: its host loop calls tdx_p_sample_update itself).
extern "C" int tdx_unet_eval_step_update(tdx_unet* u, const void* const* params, void* const* buffers, float* x,
                                         const void* cond, const float* z, const float* coef, const int64_t* tau, int S,
                                         int64_t* counter, int32_t* t_idx, int64_t* t_vec, float* eps, int64_t n_elems,
                                         void* workspace, size_t workspace_bytes, int batch, uint64_t philox_seed,
                                         int form, int guided, float w, float lo, float hi, float* hist,
                                         const float* known, const float* mask, tdx_stream_t stream) {
  const PStep ps = eval_pstep(form, coef, t_idx, tau, z, philox_seed, guided, w, lo, hi, hist, known, mask);
  if ((tau && S <= 0) || pstep_valid(ps, n_elems)) return TDX_E_BADARG;
  return eval_step_impl(u, params, buffers, x, cond, ps, tau ? S : 0, counter, t_idx, t_vec, eps, n_elems, workspace,
                        workspace_bytes, batch, stream);
}

extern "C" int tdx_unet_eval_step_update_dyn(tdx_unet* u, const void* const* params, void* const* buffers, float* x,
                                             const void* cond, const float* z, const float* coef, const int64_t* tau,
                                             int S, int64_t* counter, int32_t* t_idx, int64_t* t_vec, float* eps,
                                             int64_t n_elems, void* workspace, size_t workspace_bytes, int batch,
                                             uint64_t philox_seed, int form, int guided, float w, float lo, float hi,
                                             float* hist, const float* known, const float* mask, int rank, float frac,
                                             float* thr, tdx_stream_t stream) {
  PStep ps = eval_pstep(form, coef, t_idx, tau, z, philox_seed, guided, w, lo, hi, hist, known, mask);
  const int n = guided ? batch / 2 : batch;   // samples: the threshold buffer's rows
  if (!thr || batch <= 0 || (guided && (batch & 1)) || n_elems <= 0 || n_elems % n || n_elems / n > INT32_MAX) return TDX_E_BADARG;
  ps.thr = thr; ps.per = (int)(n_elems / n); ps.c = dyn_centre(lo, hi);
  if ((tau && S <= 0) || pstep_valid(ps, n_elems)) return TDX_E_BADARG;
  if (!(lo < hi) || rank < 0 || rank >= ps.per || !(frac >= 0.0f && frac <= 1.0f)) return TDX_E_BADARG;   // before the head kernel writes
  return eval_step_impl(u, params, buffers, x, cond, ps, tau ? S : 0, counter, t_idx, t_vec, eps, n_elems, workspace,
                        workspace_bytes, batch, stream, rank, frac);
}

// Build the sampling tables for the CURRENT INFER pack (call after tdx_unet_pack / the first INFER forward, once
// per sample() call, outside any stream capture: it may allocate).  T = number of diffusion steps (the counter
// handed to tdx_unet_eval_step must stay below it); cond = the labels / text embeddings the eval steps will be
// given (the same pointer: the cond part is computed from its contents NOW).
static int prepare_sampling_impl(tdx_unet* u, const void* const* params, const void* cond, int batch, int T,
                                 const int64_t* tau, tdx_stream_t stream) {
  if (!u || !params || batch <= 0 || batch > u->max_batch || T <= 0) return TDX_E_BADARG;
  if (!u->spec) return TDX_E_SHAPE;   // the latent MLP runs its own fused time path
  const bool needs_cond = u->kind == 1 || u->num_classes > 0;
  if (needs_cond != (cond != nullptr)) return TDX_E_BADARG;
  if (!u->packed) return TDX_E_STATE;
  if (!g_knobs.sample_tables) { u->tab_gen = -1; return 0; }   // knob "sample_tables" = 0: A/B against the direct path
  const NetSpec& S = *u->spec;
  const size_t wsum = (size_t)S.skip_ch[0] + S.skip_ch[1] + S.skip_ch[2], td = S.time_dim;
  // scratch = int64 step indices [T] | sin, pre, emb [T][td] (read as float4 rows: the index block is rounded up to
  // 16 bytes so that an odd T does not leave them 8-byte aligned; time_embed.hip places them the same way)
  const size_t scratch = std::max<size_t>(tdx_time_tables_index_floats(T) + 3 * (size_t)T * td, (size_t)batch * td);
  const size_t need = (size_t)T * wsum + (size_t)batch * wsum + scratch + 64;
  if (need > u->tab_floats) {
    if (u->tab) (void)hipFree(u->tab);
    u->tab = nullptr;
    u->tab_floats = 0;
    hipError_t e = hipMalloc(&u->tab, need * sizeof(float));
    if (e != hipSuccess) return (int)e;
    u->tab_floats = need;
    u->tab_gen = -1;
  }
  const float* const* P = reinterpret_cast<const float* const*>(params);
  hipStream_t st = to_stream(stream);
  float* t1 = u->tab;
  float* t2 = t1 + (size_t)T * S.skip_ch[0];
  float* t3 = t2 + (size_t)T * S.skip_ch[1];
  float* c1 = t3 + (size_t)T * S.skip_ch[2];
  float* c2 = c1 + (size_t)batch * S.skip_ch[0];
  float* c3 = c2 + (size_t)batch * S.skip_ch[1];
  float* scr = c3 + (size_t)batch * S.skip_ch[2];
  // (the cond block moves with T and batch; a schedule is rebuilt on every call: its contents may change under the
  // same pointer, and S rows cost little)
  if (u->tab_gen != u->pack_gen || u->tab_T != T || u->tab_batch != batch || tau || u->tab_tau)
    RC(tdx_time_tables_build(u->kind, P, T, S.time_dim, t1, t2, t3, scr, st, tau));
  if (cond) RC(tdx_time_tables_cond(u->kind, P, cond, batch, S.time_dim, c1, c2, c3, scr, st));
  u->tab_T = T;
  u->tab_batch = batch;
  u->tab_cond = cond;
  u->tab_tau = tau;
  u->tab_gen = u->pack_gen;
  return 0;
}

extern "C" int tdx_unet_prepare_sampling(tdx_unet* u, const void* const* params, const void* cond, int batch, int T,
                                         tdx_stream_t stream) {
  return prepare_sampling_impl(u, params, cond, batch, T, nullptr, stream);
}

extern "C" int tdx_unet_prepare_sampling_sched(tdx_unet* u, const void* const* params, const void* cond, int batch,
                                               const int64_t* tau, int S, tdx_stream_t stream) {
  if (!tau) return TDX_E_BADARG;
  return prepare_sampling_impl(u, params, cond, batch, S, tau, stream);
}

// Forget the sampling tables: the eval steps that follow take the direct time path (step counter, time MLP and
// projections as launches of their own), whose results are the eager forward's bit for bit - the table look-up
// reassociates one sum of a conditional network.  The next tdx_unet_prepare_sampling builds them again.
extern "C" int tdx_unet_drop_sampling_tables(tdx_unet* u) {
  if (!u) return TDX_E_BADARG;
  u->tab_gen = -1;
  return 0;
}

extern "C" int tdx_unet_request_input_grad(tdx_unet* u, float* g_x) {
  if (!u) return TDX_E_BADARG;
  if (!u->spec) return g_x ? TDX_E_SHAPE : 0;
  u->g_x = g_x;
  return 0;
}

extern "C" int tdx_unet_backward_mark(tdx_unet* u, int slot) {
  if (!u || slot < 0 || slot >= N_STAGES) return TDX_E_BADARG;
  if (!u->spec || !u->use_streams) return 0;  // everything ran on the caller's stream
  TDX_HIP(hipEventRecord(u->ev_mark[slot][0], u->side));
  TDX_HIP(hipEventRecord(u->ev_mark[slot][1], u->side2));
  return 0;
}

extern "C" int tdx_unet_backward_wait_mark(tdx_unet* u, int slot, tdx_stream_t stream) {
  if (!u || slot < 0 || slot >= N_STAGES) return TDX_E_BADARG;
  if (!u->spec || !u->use_streams) return 0;
  hipStream_t st = to_stream(stream);
  TDX_HIP(hipStreamWaitEvent(st, u->ev_mark[slot][0], 0));
  TDX_HIP(hipStreamWaitEvent(st, u->ev_mark[slot][1], 0));
  return 0;
}

extern "C" int tdx_unet_backward_sync_mark(tdx_unet* u, int slot) {
  if (!u || slot < 0 || slot >= N_STAGES) return TDX_E_BADARG;
  if (!u->spec || !u->use_streams) return 0;
  TDX_HIP(hipEventSynchronize(u->ev_mark[slot][0]));
  TDX_HIP(hipEventSynchronize(u->ev_mark[slot][1]));
  return 0;
}

extern "C" int tdx_unet_backward_join(tdx_unet* u, tdx_stream_t stream) {
  if (!u) return TDX_E_BADARG;
  if (!u->spec || !u->use_streams) return 0;  // everything already ran on the caller's stream
  hipStream_t st = to_stream(stream);
  u->side = u->side_own;
  u->side2 = u->side2_own;
  TDX_HIP(hipEventRecord(u->ev_join, u->side));
  TDX_HIP(hipStreamWaitEvent(st, u->ev_join, 0));
  TDX_HIP(hipEventRecord(u->ev_join2, u->side2));
  TDX_HIP(hipStreamWaitEvent(st, u->ev_join2, 0));
  return 0;
}
