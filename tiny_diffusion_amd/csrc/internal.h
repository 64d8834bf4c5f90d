// Library-internal entry points (not part of the C ABI).
#pragma once
#include <cmath>
#include "common.h"
#include "knobs.h"

// the diagnostic buffer (tdx_diag_set_buffer, time_embed.hip): every path that stamps checks its records against the size
extern unsigned* g_tdx_diag_buffer;
extern size_t g_tdx_diag_bytes;

int tdx_copy_segments(const float* const* src, float* const* dst, const size_t* n, int count, hipStream_t st);
int tdx_pixel_sum(const void* g, float* out, int B, int HW, int C, hipStream_t st, int io16 = 0);
int tdx_reduce_partials(const float* partial, float* out, int nblk, int stride, int count,
                        hipStream_t st);
// initial_conv: NCHW model input (cin = 1 | 4) -> channels-last, 64 channels stored of which the
// first cout_real (64 | 32) are real; final_conv: channels-last 64 -> NCHW cout (1 | 4)
int tdx_initial_conv_fwd(const float* x, const float* w, const float* bias, void* out, int B, int H,
                         int W, int cin, int cout_real, hipStream_t st, int io16 = 0);
int tdx_small_conv_wgrad_blocks(int B, int H, int W);
int tdx_small_conv_partial_width(void);
int tdx_initial_conv_wgrad(const float* x, const void* g, float* partial, float* dw, float* db,
                           int B, int H, int W, int cin, int cout_real, hipStream_t st, int io16 = 0);
int tdx_initial_conv_dgrad(const void* g_x0, const float* w, float* g_x, int B, int H, int W, int cin,
                           int cout_real, hipStream_t st, int io16 = 0);
int tdx_final_conv_fwd(const void* in, const float* w, const float* bias, float* out, int B, int H,
                       int W, int cout, hipStream_t st, int io16 = 0);
// One reverse-process update x <- step(x, out, noise | history), as the elementwise kernel (tdx_pstep_launch,
// elementwise.hip) and the epilogue of final_conv (tdx_final_conv_fwd_psample, edge_conv.hip) run it.  form says what
// the rows of coef are and which update of common.h (pstep_elem) they drive:
//   TDX_STEP_EPS  (S,3) rows (c1, c2, sigma)         x' = c1*(x - c2*out) + sigma*z
//   TDX_STEP_X0   (S,5) rows (p, q, A, Bx, sigma)    x' = (A*x0 + Bx*x) + sigma*z,  x0 = clamp(p*x + q*out, lo, hi)
//   TDX_STEP_MS   (S,5) rows (p, q, A, Bx, H)        x' = (A*x0 + Bx*x) + H*hist;  hist <- x0   (deterministic)
// Row t = *t_idx.  Noise at t > 0 only: Philox block (element / 4), stream tau[t] (t when tau == null), or z, or none.
// guided: x and out hold two halves - the caller's condition, the null condition - that cfg_eps combines under w; the
// one update is written to both halves of x, and z / hist / known / mask / Philox are those of the first half.
// known / mask (X0, MS): x0 <- x0_blend(x0, known, mask) before the step (inpainting).
// thr (X0, MS): dynamic thresholding - (s, r) per sample of `per` elements, written by tdx_x0_threshold_launch, drive
// x0_thresholded in place of x0_clamped; [lo, hi] is then the finite data range and c its centre.
struct PStep {
  int form; const float* coef; const int32_t* t_idx; const int64_t* tau;
  const float* z; int philox; uint64_t seed;   // philox: in-kernel noise, z ignored
  int guided; float w;
  float lo, hi;
  float* hist;
  const float* known; const float* mask;
  int64_t* counter_dec;   // non-null: *counter_dec = *t_idx - 1 (the table-mode step counter, advanced by a step's last kernel)
  // the fused epilogue only: the state it updates in place (x and z start at this launch's first element), that
  // element's index in the whole batch (a half-batch launch keeps the batch's Philox stream; hist, known and mask are
  // indexed by it) and the elements of one guided half
  float* x; int64_t elem0, half;
  float* thr; int per; float c;   // dynamic thresholding (never in the fused epilogue)
};
// 0, or the error of an update over n elements (guided: per half): TDX_E_SHAPE for an eps-form n % 4 != 0 with
// nothing else wrong, as the eps-form entries have always answered; TDX_E_BADARG for every other broken rule
static inline int pstep_valid(const PStep& s, int64_t n) {
  if (!s.coef || !s.t_idx || n <= 0 || (s.elem0 & 3) || (s.guided && s.elem0)) return TDX_E_BADARG;
  if (s.form != TDX_STEP_EPS && s.form != TDX_STEP_X0 && s.form != TDX_STEP_MS) return TDX_E_BADARG;
  if (s.form != TDX_STEP_EPS && !(s.lo < s.hi)) return TDX_E_BADARG;   // rejects a NaN bound
  if (s.form == TDX_STEP_MS && (!s.hist || s.z)) return TDX_E_BADARG;
  if ((s.known != nullptr) != (s.mask != nullptr) || (s.known && s.form == TDX_STEP_EPS)) return TDX_E_BADARG;
  if (n % 4) return s.form == TDX_STEP_EPS ? TDX_E_SHAPE : TDX_E_BADARG;
  if (s.thr && (s.form == TDX_STEP_EPS || s.per <= 0 || s.per % 4 || n % s.per || !std::isfinite(s.lo) ||
                !std::isfinite(s.hi) || !std::isfinite(s.hi - s.lo))) return TDX_E_BADARG;
  return 0;
}
// The centre and the half width of the data range, (lo + hi) / 2 and (hi - lo) / 2 in fp32
static inline float dyn_centre(float lo, float hi) { return (lo + hi) / 2.0f; }
static inline float dyn_half(float lo, float hi) { return (hi - lo) / 2.0f; }
// (s_b, r_b) of s.thr for the n_samples samples of s.per elements of x / out (guided: out holds 2 n_samples rows), from
// s.coef, s.t_idx, s.guided, s.w, s.lo, s.hi (x0_threshold_kernel, elementwise.hip); rank in [0, per), frac in [0, 1]
int tdx_x0_threshold_launch(const PStep& s, const float* x, const float* out, int n_samples, int rank, float frac,
                            hipStream_t st);
// x_out may alias x (guided: it must); the fused-only fields of s are ignored
int tdx_pstep_launch(const PStep& s, float* x_out, const float* x, const float* out, int64_t n, hipStream_t st);
// final_conv forward with the update in its epilogue (sampling): s.x in place, the network's output still goes to eps_out
int tdx_final_conv_fwd_psample(const void* in, const float* w, const float* bias, float* eps_out, int B, int H, int W,
                               int cout, const PStep& s, hipStream_t st, int io16 = 0);
int tdx_final_conv_dgrad(const float* g_out, const float* w, void* g_in, int B, int H, int W,
                         int cout, hipStream_t st, int io16 = 0);
int tdx_final_conv_wgrad(const void* in, const float* g_out, float* partial, float* dw, float* db,
                         int B, int H, int W, int cout, hipStream_t st, int io16 = 0);
// kind 0: raw-t MLP (+ class embedding y); kind 1: sinusoid + 768-d MLP + additive `cond`
int tdx_time_embed_fwd(int kind, const int64_t* t, const int64_t* y, const float* cond,
                       const float* const* P, float* sin, float* pre, float* emb, float* t1, float* t2,
                       float* t3, int B, hipStream_t st, int td = 0);  // td: time_dim (0 = the kind's default)
int tdx_time_embed_bwd(int kind, const int64_t* y, const float* const* P, float* const* G,
                       const float* sin, const float* pre, const float* emb, const float* g_t1,
                       const float* g_t2, const float* g_t3, float* scratch, int B, int ncls,
                       hipStream_t st, int td = 0, int parts = 7);
// `parts` of the time path's backward, in dependency order: the three projections (dW, db, their sum into
// g(emb)); the middle (class embedding, second linear layer, and for kind 1 the first one too); kind 0's
// first layer (time_l1_bwd_kernel).  A caller may issue them at different times (unet.hip).
enum { TDX_TIME_PROJ = 1, TDX_TIME_MID = 2, TDX_TIME_L1 = 4 };
// one projection's share of TDX_TIME_PROJ (time_embed.hip)
int tdx_time_proj_bwd(int kind, int k, const float* const* P, float* const* G, const float* emb,
                      const float* g_tk, float* scratch, int B, hipStream_t st, int td = 0);
struct TdxSplitDefer;
struct TdxPoolFuse;
int tdx_conv3x3_fwd_splitk_fused(const float* in, const float* wpk, const float* bias, float* out, int B, int H,
                                 int W, int cin, int cout, int flags, const float* out_scale,
                                 const float* out_shift, float* scratch, size_t scratch_floats, tdx_stream_t stream,
                                 TdxSplitDefer* defer = nullptr, TdxPoolFuse* pool = nullptr);
// the inference convolution (conv3x3.hip, variant 4) on the tile-major pack, with the sampling-only extras of
// tdx_conv3x3_fwd_splitk_fused (defer the split-K reduction to the consumer / fold the following max-pool into it)
int tdx_conv3x3_fwd_infer_ex(const float* in, const float* w_tiled, const float* bias, float* out, int B, int H, int W,
                             int cin, int cout, const float* out_scale, const float* out_shift, float* scratch,
                             size_t scratch_floats, tdx_stream_t stream, TdxSplitDefer* defer, TdxPoolFuse* pool);
#define TDX_PACK_MAX 13
struct TdxPackBatch {
  const float* w[TDX_PACK_MAX];
  float* wf[TDX_PACK_MAX];
  float* wd[TDX_PACK_MAX];
  int cout[TDX_PACK_MAX], cin[TDX_PACK_MAX], cin_real[TDX_PACK_MAX], chunk_start[TDX_PACK_MAX];
  int count;
};
int tdx_pack_conv3x3_batch(TdxPackBatch* b, tdx_stream_t stream);   // (wf[u] / wd[u] may be null: that pack is skipped)
// Winograd packs (conv3x3_wino.hip): uf / ud = transformed weights of the forward / the input gradient, cout*cin*16 floats each; either may be null
struct TdxWinoPackBatch {
  const float* w[TDX_PACK_MAX];
  float* uf[TDX_PACK_MAX];
  float* ud[TDX_PACK_MAX];
  int cout[TDX_PACK_MAX], cin[TDX_PACK_MAX], cin_real[TDX_PACK_MAX], start[TDX_PACK_MAX];
  int count;
};
int tdx_pack_conv3x3_wino_batch(TdxWinoPackBatch* b, tdx_stream_t stream);
extern "C" int tdx_conv3x3_wino_ok(int B, int H, int W, int cin, int cout);
extern "C" int tdx_conv3x3_wino_stat_tiles(int B, int H, int W);
extern "C" int tdx_conv3x3_wino_stat_tile_rows(int B, int H, int W);
extern "C" int tdx_conv3x3_wgrad_wino_splits(int B, int H, int W, int cin, int cout);
extern "C" int tdx_conv3x3_wgrad_wino(const float* in, const float* dy, float* dw_slabs, int B, int H, int W, int cin, int cout,
                                      tdx_stream_t stream);
int tdx_conv3x3_wino_launch(const float* in, const float* u, const float* bias, float* out, int B, int H, int W,
                            int cin, int cout, int flags, const float* out_scale, const float* out_shift,
                            float* stats_partial, int splits, int per, tdx_stream_t stream);
int tdx_conv3x3_fwd_wino_infer_ex(const float* in, const float* u, const float* bias, float* out, int B, int H, int W,
                                  int cin, int cout, const float* out_scale, const float* out_shift, float* scratch,
                                  size_t scratch_floats, tdx_stream_t stream, TdxSplitDefer* defer, TdxPoolFuse* pool);
int tdx_pack_conv3x3_tiled_batch(TdxPackBatch* b, tdx_stream_t stream);  // wf: tile-major fp32 pack (wd unused)
int tdx_pack_conv3x3_tiled_pad(const float* w_oihw, float* w_tiled, int cout, int cin_real, int cin, tdx_stream_t stream);
int tdx_pack_conv3x3_batch_bf16(TdxPackBatch* b, tdx_stream_t stream);  // wf / wd hold bf16 (either may be null)
// conv3x3 weight packs / gradient for an input tensor zero-padded from cin_real to cin channels
int tdx_pack_conv3x3_pad(const float* w_oihw, float* w_fwd, float* w_dgrad, int cout, int cin_real,
                         int cin, tdx_stream_t stream);
int tdx_conv3x3_wgrad_reduce_pad(const float* dw_slabs, float* dw_oihw, int splits, int cout, int cin,
                                 int cin_real, tdx_stream_t stream);
// tf: float(t) per sample, as stored by the forward (tdx_time_embed_fwd kind 0 -> sin, tdx_time_embed_only)
int tdx_time_embed_bwd_ex(const float* tf, const int64_t* y, const float* const* P, float* const* G,
                          const float* pre, const float* emb, const float* const* gk, const int* ldg,
                          const int* widths, float* scratch, int B, int ncls, hipStream_t st, int td = 0,
                          int parts = 7);
// synchronised BatchNorm pieces (bn.hip); tdx_allreduce_fn: include/tdx.h
int tdx_bn_moments(const float* stats_partial, int tiles, int tile_rows, int64_t count, int C, double* mom,
                   hipStream_t st);
int tdx_bn_finalize_moments(const double* mom, int C, const float* gamma, const float* beta, float* running_mean,
                            float* running_var, int64_t* nbt, float* scale, float* shift, float* save_mean,
                            float* save_rstd, hipStream_t st);
int tdx_bn_relu_bwd_sync(float* g, const float* y, int64_t rows, int C, const float* scale, const float* shift,
                         const float* save_mean, const float* save_rstd, const float* gamma, float* dgamma,
                         float* dbeta, float* dbias, float* scratch, int training, tdx_allreduce_fn sync,
                         void* sync_user, double* mom, tdx_stream_t stream, int io16 = 0);
int tdx_time_embed_only(const int64_t* t, const int64_t* y, const float* const* P, float* pre, float* emb,
                        float* tf_out, int B, hipStream_t st);
// sampling tables (time_embed.hip) and the pieces of a table-mode reverse step
size_t tdx_time_tables_index_floats(int T);
// tau != null: the T rows are built at the timesteps tau[0..T) (a DDIM schedule) instead of 0..T-1
int tdx_time_tables_build(int kind, const float* const* P, int T, int td, float* tab1, float* tab2, float* tab3,
                          float* scratch, hipStream_t st, const int64_t* tau = nullptr);
int tdx_time_tables_cond(int kind, const float* const* P, const void* cond, int B, int td, float* tabc1, float* tabc2,
                         float* tabc3, float* scratch, hipStream_t st);
// B0 < B: samples >= B0 go to the second set of destinations (o1b ...), indexed from 0 (half-batch sampling: unet.hip)
int tdx_sample_head(const int64_t* counter, int32_t* t_idx, int64_t* t_vec, int B, int T, int kind, const float* tab1,
                    const float* tab2, const float* tab3, const float* tc1, const float* tc2, const float* tc3,
                    float* o1, float* o2, float* o3, hipStream_t st, int B0 = 0, float* o1b = nullptr, float* o2b = nullptr,
                    float* o3b = nullptr, const int64_t* tau = nullptr);
// latent MLP noise model (latent_diffusion.py:16-128), kind TDX_UNET_LATENT_MLP of tdx_unet_*
size_t tdx_latent_workspace_floats(int B);
size_t tdx_latent_infer_ss_floats(void);
int tdx_latent_pack(const float* const* P, void* const* buffers, float* infer_ss, hipStream_t st);
int tdx_latent_forward(const float* const* P, void* const* buffers, const float* z, const int64_t* t,
                       const int64_t* y, float* out, float* ws, int B, int mode, const float* infer_ss,
                       hipStream_t st, int bf16 = 0);
int tdx_latent_backward(const float* const* P, float* const* G, const float* d_out, float* ws, int B,
                        int training, int stage_lo, int stage_hi, int ncls, hipStream_t st, int bf16 = 0);
int tdx_latent_tensor(int B, const char* name, size_t* off, size_t* numel);
int tdx_bn_relu_apply(const float* y, float* out, int64_t rows, int C, const float* scale, const float* shift,
                      hipStream_t st, int io16 = 0);
int tdx_conv3x3_dgrad_bnbwd(const float* in, const float* wpk, float* out, int B, int H, int W, int cin, int cout,
                            const float* y, const float* scale, const float* shift, const float* mean,
                            const float* rstd, float* partial, int* nblk, float* scratch, size_t scratch_floats,
                            tdx_stream_t stream);
// BatchNorm+ReLU backward from partial sums a producer kernel has already written ([nblk][2][C] at `partial`;
// coef: 3*C floats of scratch): finalize + apply, the tail of tdx_bn_relu_bwd_sync
int tdx_bn_relu_bwd_tail(float* g, const float* y, int64_t rows, int C, const float* scale, const float* shift,
                         const float* save_mean, const float* save_rstd, const float* gamma, float* dgamma,
                         float* dbeta, float* dbias, const float* partial, int nblk, float* coef, int training,
                         tdx_allreduce_fn sync, void* sync_user, double* mom, tdx_stream_t stream, int io16 = 0);
// the resize adjoint / max-pool backward that also emit those partial sums for the tensor they write
// (bn_y .. bn_rstd of the unit whose activation gradient g_in is; partial [*nblk][2][C])
int tdx_bilinear_ac_bwd_bn(const void* g_out, void* g_in, int B, int Hi, int Wi, int Ho, int Wo, int C,
                           int g_cstride, int g_coff, const void* bn_y, const float* bn_scale,
                           const float* bn_shift, const float* bn_mean, const float* bn_rstd, float* partial,
                           int* nblk, tdx_stream_t stream, int io16 = 0);
int tdx_maxpool2_ceil_bwd_bn(const void* y, const float* scale, const float* shift, const void* g_out,
                             const void* skip_grad, void* g_in, int B, int H, int W, int C, const float* bn_mean,
                             const float* bn_rstd, float* partial, int* nblk, tdx_stream_t stream, int io16 = 0);
// the fp32 | bf16 forms of the spatial kernels (io16: activation tensors hold bf16, io16.h)
int tdx_maxpool2_ceil_fwd_t(const void* y, const float* scale, const float* shift, void* out, int B, int H, int W,
                            int C, int io16, tdx_stream_t stream);
int tdx_bilinear_ac_fwd_t(const void* in, const float* scale, const float* shift, const float* addend, void* out, int B,
                          int Hi, int Wi, int Ho, int Wo, int C, int out_cstride, int out_coff, int io16,
                          tdx_stream_t stream);
#define TDX_BNBWD_MAX_PRODUCER_BLOCKS 2048   // workgroups of the two spatial producers above
// inference: both halves of a decoder's concatenated input (resize(a) | resize(b + b_addend)) in one launch
// A split-K convolution of the sampling path whose reduction is DEFERRED to the kernel that reads its result
// (tdx_conv3x3_fwd_splitk_fused with a non-null `defer`): `splits` raw partial slabs of `slab` floats at `partial`,
// to be summed in the order 0..splits-1, + bias, then relu(. * scale + shift).  splits == 0: the convolution was not
// split (or not deferrable) and wrote its output tensor as usual.
// the 2x2 ceil-mode max-pool that follows a sampling convolution, done by its split-K reduction (pooled = null on
// return when the convolution was not split: the caller then runs the pooling kernel)
struct TdxPoolFuse { float* pooled; };
struct TdxSplitDefer {
  const float* partial; int splits; size_t slab; const float* bias; const float* scale; const float* shift;
};
int tdx_bilinear_pair_fwd_ex(const void* a, const TdxSplitDefer* a_defer, int Ha, int Wa, int Ca, const void* b,
                             const float* b_addend, int Hb, int Wb, int Cb, void* out, int B, int Ho, int Wo,
                             hipStream_t st, int io16 = 0);
int tdx_bilinear_pair_fwd(const float* a, int Ha, int Wa, int Ca, const float* b, const float* b_addend, int Hb,
                          int Wb, int Cb, float* out, int B, int Ho, int Wo, hipStream_t st);
