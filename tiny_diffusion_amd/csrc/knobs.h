// The tuning knobs (tdx_tune_set / tdx_tune_get, TDX_TUNE= at import): one field per key, named like the key, with
// its default.  knobs.hip holds the key table and the rule each key normalises a value by.  Readers take g_knobs.field
// at the point where the knob acts (plan creation, pack time or launch), never a copy.
#pragma once

struct TdxKnobs {
  // ---- fp32 direct convolution (conv3x3.hip); 0 = heuristic
  int conv_tile = 0;                // 1: 128x128, 2: 128x64, 3: 64x64
  int conv_min_tiles = 256;         // smallest grid a 128-row tile may have
  int conv_dbg = 0;                 // ConvArgs::dbg bits; bit 3 (key "stats_epi"): one-pass (Chan) statistics epilogue
  int conv_stamp = 0;               // diagnostics: LDS-DMA forward (1 | 2 | +-M) and Winograd (3) kernels stamp their main loop into the diag buffer
  int splitk = 1;                   // 0: never split K; 1: split K when the grid would not fill the chip
  int splitk_tiles = 260;           // split K when the 64x64 grid has fewer tiles than this (sweep on
                                    // MI355X: 192 -> 260 is neutral at n=16 and 4 % faster at n=64)
  int splitk_target = 512;          // ... into about this many workgroups
  int wgrad_target = 2048;          // workgroups aimed at by the wgrad pixel split
  int wgrad_target_big = 1024;      // the same for 128x128 tiles (0: wgrad_target): at most two of them fit a
                                    // CU (64 KiB of LDS each), so fewer, longer workgroups halve the slab traffic
  int conv_hybrid = 0;              // 1: training convolutions K-slice the tiles beyond the last whole round (plan_hybrid).
                                    // OFF: isolated it gains 1 % on the roofline leg (120.9 -> 121.7 TFLOP/s), inside the step
                                    // nothing (the reduction launch it adds sits in the forward's dependent chain: 15.53 vs
                                    // 15.56 ms), and it adds 16 % HBM traffic per launch (221.9 -> 257.7 MB, PMC)
  int splitk_train = 1;             // training convolutions of latency-bound shapes split K (plan_splitk_train)
  int splitk_train_t64 = 1024;      // ... when the 64x64 grid has fewer tiles than this
  int splitk_train_target = 1536;   // ... into about this many workgroups
  int wgrad9_wgs = 0;               // bf16 mode: workgroups of the nine-tap kernel aimed at by the split (0: the per-tap plan's splits)
  int wgrad_small = 1;              // 64x64 wgrad tiles for big-weight / few-pixel layers
  // inference (sampling) convolution, variant 4 (conv3x3_ring64_kernel): "infer_ring" (0: variant 3 on the K-contiguous
  // pack; 1: INFER-mode plans pack tile-major and run variant 4), "infer_stages" (3 | 4 LDS stages), "infer_splits" (> 0:
  // force that split count where K allows), "infer_ovh" / "infer_red" (plan_infer's per-workgroup and per-reduction costs,
  // in K-tile units), "infer_cus" (compute units one launch may count on: 256, or 128 when two half-batches run side by side)
  int infer_ring = 0;               // OFF: measured slower than variant 3 (comment at conv3x3_ring64_kernel)
  int infer_stages = 4;
  int infer_splits = 0;
  int infer_ovh = 4;
  int infer_red = 12;
  int infer_cus = 256;
  int wino_infer = 1;               // INFER-mode plans run Winograd with split-K (tdx_conv3x3_fwd_wino_infer_ex); INFER packs written afterwards follow
  int wino_infer_ovh = 2;           // plan of the Winograd inference launch: a workgroup's non-loop time in stages (ring fill + epilogue ~ 4 us of 2.3)
  int wino_infer_red = 3;           // ... and the dependent reduction launch
  int wino_infer_min_units = 700;   // (n = 16: 784 for the first 64->128 layer, 512 for the 4x4 / 64-channel ones)
  // ---- Winograd training kernels (conv3x3_wino.hip); plans created / steps run afterwards follow
  // "wino": fp32 training forwards / input gradients of raw-input units run on Winograd F(2x2,3x3) where the launch
  // fills the chip (>= "wino_min_wgs" workgroups of 64 tiles x 64 channels) and the map geometry allows
  int wino = 1;
  int wino_min_wgs = 100;
  int wino_wgrad = 1;               // weight gradients by F(3x3,2x2) (conv3x3_wgrad_wino_kernel)
  int wino_wgrad_min_tiles = 1024;
  int wino_wgrad_target = 512;      // workgroups the pixel split of the Winograd weight gradient aims at
  int wino_rows = 1;                // training launches on the row-split main loop (0: the channel split)
  int wino_rows_min_stages = 16;    // ... of at least this many K-stages (the 8-stage input gradients lost
                                    // more to the exchange than their loop saved: profiles/r06_wino_phases.txt)
  // ---- bf16 mode (conv3x3_bf16.hip, unet.hip)
  int bf16_storage = 1;             // plans switched to bf16 afterwards keep their activation tensors in bf16 too
  int bf16_materialize = 1;         // "materialize" in bf16 storage mode (0: BN + ReLU while the consuming GEMMs stage their tiles)
  // conv3x3_bf16_ring_kernel.  Off by default: isolated, the ring kernel is 6-9 % faster over the MNIST launches
  // (forward 1109 -> 1043 us, input gradient 955 -> 865), but one 155 KB workgroup per CU shares a CU with nothing, and
  // inside the three-stream step it measured SLOWER (MNIST bf16 4.50 vs 4.40 ms, LAION 64x64 10.29 vs 10.12).
  int bf16_ring = 0;                // 0: 128-row register-staging bf16 GEMM everywhere
  // conv3x3_bf16_thin_kernel: 0 off | 1 layers with 64 output channels | 2 also layers with 64 input channels |
  // 3 (default) every raw-input launch whose rows are a multiple of 256 (wider layers run one workgroup per 64 output
  // channels, each with its own copy of the window).  Measured, B = 256: isolated (LAION 64x64) 64 -> 64 forward
  // 201 -> 129 us, its input gradient 151-193 -> 104-144, 192 -> 64 forward 428 -> 273, its input gradient (64 -> 192)
  // 473 -> 335; steps in ms, knob 0 / 1 / 2 / 3: LAION 64x64 9.34 / 8.84 / 8.65 / 8.49, LAION 32x32 3.24 / 3.11 / 3.08 /
  // 2.96, MNIST 4.27 / 4.16 / 4.13 / 3.98.  Still 3-4x the thin layers' HBM time: a workgroup's 72 MFMAs per wave (1 us)
  // wait for nine weight tiles one L2 round trip each - keeping the 72 KB of weights resident across tiles is the next step.
  int bf16_thin = 3;
  int bf16_wgrad_swz = 1;           // bf16-storage weight gradient (conv3x3_wgrad_bf16s_kernel); 0: the round-2 staging (8-way LDS store conflicts)
  int bf16_wgrad9 = 1;              // conv3x3_wgrad9_bf16_kernel; 0: one workgroup per tap (conv3x3_wgrad_bf16s_kernel)
  // ---- plans and the training step (unet.hip)
  int streams = -1;                 // -1 = per-network default (NetSpec::overlap), 0 / 1 = plans created afterwards train on one / three streams
  int materialize = 1;              // 1 = the activation feeding the second convolution of a stage is written out (post
                                    // BN+ReLU) so that convolution and its wgrad run on the LDS-DMA kernels
  // "bnbwd_fused": the kernel that PRODUCES dL/d(activation) of a unit also emits the partial sums of that unit's
  // BatchNorm backward, and the separate reduction pass is skipped (tdx_unet_backward): bit 0 input-gradient
  // convolutions, bit 1 resize adjoints, bit 2 max-pool backward.  Measured at B = 256 (tools/gpu_ab.py, ms/step):
  // 0: 15.54, 1: 15.73, 2: 15.52, 4: 15.55, 6: 15.53, 7: 15.66 - the heavier convolution epilogue costs the GEMMs more
  // than the reduction pass it saves (that pass is HBM-bound and runs beside the weight-gradient GEMMs of the other
  // stream for nothing); the two spatial producers are neutral in time and save 8 B/element of HBM traffic and a launch
  // on seven layers: on.  The convolution form stays an experiment.
  int bnbwd_fused = 6;
  // ---- sampling (unet.hip)
  // Sampling (INFER forward) launch fusions, "sample_fuse": bit 0 a split-K result consumed only by a resize is left
  // unreduced and summed by that resize on load (splits <= "sample_defer_max"), bit 1 the reduction of units 3 / 5 also
  // does the max-pool that follows, bit 2 final_conv applies the reverse-process update in its epilogue.  Measured at
  // n = 16 (tools/gpu_ab.py, ms per reverse step, tables on): none 0.565, pool 0.564, update 0.561, both 0.562, + deferral
  // of 2-way splits 0.561, of <= 4-way 0.571, of <= 8-way 0.575.  A launch removed this way gives back 1-4 us, not the
  // 5-6 us the trace shows per small kernel: that time is the dependent pass itself (partials written behind eight L2s
  // are read back through the fabric), which the fused kernel still makes - and the deferred form re-reads every
  // partial ~4 times.  Pool and update fusion stay on (neutral to -4 us, two launches fewer); deferral is off.
  int sample_defer_max = 2;
  int sample_fuse = 6;
  // "sample_halves": INFER forwards of >= "sample_halves_min" samples run as two half-batches side by side (tdx_unet_forward).
  // Built, parity-tested, measured, OFF: whether the two branches of the captured step overlap at all depends on which
  // hardware queues the runtime gives them (tools/micro/graph_branch_probe.py: the same two-branch graph replays in 0.50x
  // or in 0.74x the one-chain time from process to process; tools/micro/halves_matrix.sh: reverse step at n = 16 / 64,
  // ms: whole batch 0.61 / 1.75, halves 1.65 / 2.12 with the default 4 hardware queues, 0.62 / 1.61 with
  // GPU_MAX_HW_QUEUES=8) - at best -8 % at n = 64 and nothing at n = 16, at worst 2.7x slower.
  int sample_halves = 0;
  int sample_halves_min = 4;
  int sample_tables = 1;            // tdx_unet_prepare_sampling builds the tables (0: leaves eval steps on the direct path)
};
extern TdxKnobs g_knobs;   // knobs.hip
