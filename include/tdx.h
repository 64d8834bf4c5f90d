/*
 * tdx.h - C ABI of libtdx.so: the MI355X (gfx950) implementation of the
 * tiny-diffusion DDPM hot path.
 *
 * The reference (david-wb/tiny-diffusion) is pure Python and defines no FFI;
 * its boundary for this path is the Python call surface
 *     NoiseModel.forward(x, t[, y])      diffusion.py:109 / conditional_diffusion.py:115
 *     ForwardProcess.q_sample(...)       diffusion.py:177
 *     sample(...) reverse loop           diffusion.py:254-276
 * Each entry point below names the reference lines it replaces.  The host side
 * (the tiny_diffusion_amd python package) mirrors that Python surface and calls these
 * through ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every function returns int: 0 = ok, >0 = hipError_t, <0 = TDX_E_*.
 *     Nothing throws.
 *   - all data pointers are caller-owned DEVICE pointers; the library never
 *     allocates on the hot path (scratch comes from a caller workspace sized
 *     by tdx_unet_workspace_bytes).
 *   - every launch takes an explicit hipStream_t (as void*).
 *   - activations are fp32, channels-last (N,H,W,C); (N,1,H,W) model inputs
 *     and outputs are bit-identical in both layouts.
 *   - parameters are passed in the REFERENCE layout (OIHW conv weights, the
 *     state_dict order of diffusion.py:16-107); packing is done on device.
 */
#ifndef TDX_H
#define TDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDX_VERSION 400 /* 0.4.0: additions: tdx_step_begin_sched, tdx_p_sample_step_sched{,_philox}, tdx_unet_prepare_sampling_sched, tdx_unet_eval_step_update (timestep schedules: DDIM sampling); tdx_pack_conv3x3_tiled, tdx_conv3x3_fwd_infer, tdx_conv3x3_infer_scratch_floats (the inference convolution of the reverse process), tdx_linear_{fwd,bwd}_prec; tdx_unet_set_precision accepts TDX_PREC_BF16 for the latent MLP.  0.3.0: tdx_diag_set_buffer takes the buffer size (incompatible); additions: tdx_timestep_embedding_f32, tdx_initial_conv_input_grad, tdx_unet_request_input_grad; time_dim of any width */

#define TDX_E_BADARG (-1)   /* null pointer, size <= 0, batch > plan capacity ... */
#define TDX_E_SHAPE (-2)    /* shape the kernel family does not cover */
#define TDX_E_WORKSPACE (-3) /* workspace too small */
#define TDX_E_STATE (-4)    /* backward without a saved forward, etc. */

typedef void* tdx_stream_t; /* hipStream_t */

int tdx_version(void);
const char* tdx_error_string(int code);

/* ---- forward process / reverse step (HBM-bound elementwise) ------------- */

/* q_sample, diffusion.py:177-190: x_t = sqrt_ac[t]*x0 + sqrt_1mac[t]*noise.
 * sqrt_ac / sqrt_1mac: device tables (T,) = sqrt(alphas_cumprod), sqrt(1-alphas_cumprod)
 * computed by the host with the reference's fp32 expressions.
 * 12 B/element algorithmic traffic (read x0, noise; write x_t). */
int tdx_q_sample(const float* x0, const float* noise, const int64_t* t,
                 const float* sqrt_ac, const float* sqrt_1mac, float* x_t,
                 int batch, int per_sample, tdx_stream_t stream);

/* q_sample with in-kernel Philox4x32-10 + Box-Muller noise (throughput mode;
 * statistically equivalent to, not bit-identical with, torch.randn).
 * Writes both x_t and the noise (the training target, diffusion.py:225/231). */
int tdx_q_sample_philox(const float* x0, const int64_t* t, const float* sqrt_ac,
                        const float* sqrt_1mac, float* x_t, float* noise_out,
                        int batch, int per_sample, uint64_t seed, uint64_t offset,
                        tdx_stream_t stream);

/* q_sample that also writes the training target of a parameterisation (an addition: the reference trains on
 * eps only).  x_t as tdx_q_sample, bit for bit.  kind 0 (eps): target = noise.  kind 1 (v, Salimans & Ho 2022):
 * target = sqrt_ac[t]*noise - sqrt_1mac[t]*x0, both products and the subtraction rounded separately.  target may be
 * the noise buffer.  Another kind: TDX_E_BADARG; per_sample % 4: TDX_E_SHAPE. */
int tdx_q_sample_target(const float* x0, const float* noise, const int64_t* t, const float* sqrt_ac,
                        const float* sqrt_1mac, float* x_t, float* target, int batch, int per_sample, int kind,
                        tdx_stream_t stream);
/* ... with the in-kernel noise of tdx_q_sample_philox (same stream and indexing: x_t equals that entry's for the
 * same seed and offset).  Writes x_t and target only: 12 B/element. */
int tdx_q_sample_target_philox(const float* x0, const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac,
                               float* x_t, float* target, int batch, int per_sample, int kind, uint64_t seed,
                               uint64_t offset, tdx_stream_t stream);

/* One reverse step, diffusion.py:272-274:
 *   x_out = c1*(x - c2*eps) + sigma*z        (z == NULL or t == 0: z = 0, diffusion.py:267-270)
 * coef: device table (T,3) of (c1,c2,sigma) = (1/sqrt(alpha), (1-alpha)/sqrt(1-acp), sqrt(beta));
 * t_idx: device pointer to the current step index (int32) so that a captured
 * graph can be replayed for every t.  16 B/element (read x, eps, z; write x). */
int tdx_p_sample_step(float* x_out, const float* x, const float* eps, const float* z,
                      const float* coef, const int32_t* t_idx, int64_t n,
                      tdx_stream_t stream);

/* Same, with in-kernel Philox noise (z generated, never stored): 12 B/element. */
int tdx_p_sample_step_philox(float* x_out, const float* x, const float* eps,
                             const float* coef, const int32_t* t_idx, int64_t n,
                             uint64_t seed, tdx_stream_t stream);
/* Device-side step counter for graph-captured sampling loops: t = *counter; *t_idx = t;
 * t_vec[0..n) = t; *counter = t - 1.  (diffusion.py:259-260 rebuilds t on the host per step.) */
int tdx_step_begin(int64_t* counter, int32_t* t_idx, int64_t* t_vec, int n, tdx_stream_t stream);

/* Timestep schedules (DDIM, schedule.py ddim_schedule): a reverse chain of S steps k = S-1 .. 0 that runs the
 * network at the timesteps tau[k] (device int64, strictly ascending, < T).  The step index k takes the place of t:
 * it is the row of the (S,3) coefficient table coef = (c1, c2, sigma) of x' = c1 (x - c2 eps) + sigma z, the noise
 * term is skipped at k == 0, and in-kernel Philox noise is keyed by (element, tau[k], seed) - so the identity
 * schedule tau = 0..T-1 with the table of tdx_p_sample_step reproduces that update bit for bit.
 * tdx_step_begin_sched: k = *counter; *t_idx = k; t_vec[0..n) = tau[k]; *counter = k - 1. */
int tdx_step_begin_sched(int64_t* counter, const int64_t* tau, int32_t* t_idx, int64_t* t_vec, int n,
                         tdx_stream_t stream);
/* The update at step k = *k_idx (z == NULL: no noise term). */
int tdx_p_sample_step_sched(float* x_out, const float* x, const float* eps, const float* z, const float* coef,
                            const int64_t* tau, const int32_t* k_idx, int64_t n, tdx_stream_t stream);
int tdx_p_sample_step_sched_philox(float* x_out, const float* x, const float* eps, const float* coef,
                                   const int64_t* tau, const int32_t* k_idx, int64_t n, uint64_t seed,
                                   tdx_stream_t stream);

/* Classifier-free guidance (Ho & Salimans 2021).  The null condition is label -1 (any negative label: emb = t_emb, no
 * read of class_embedding) or an all-zero text-embedding row.  A guided chain of n samples keeps 2n rows: x and eps hold
 * two halves of n_half_elems floats, the first evaluated under the caller's condition, the second under the null
 * condition, and the halves of x are equal.  For j < n_half_elems:
 *   e = eps[j + n_half_elems] + w (eps[j] - eps[j + n_half_elems]);   x' = c1 (x[j] - c2 e) + sigma z[j]
 * written to x[j] and x[j + n_half_elems] (in place).  z: n_half_elems floats or NULL; use_philox: in-kernel noise
 * indexed by j (the stream of the unguided chain of n samples); no noise at step 0.  tau: the schedule's timesteps
 * (t_idx holds the step index k) or NULL for the identity chain.  counter_dec != NULL: *counter_dec = *t_idx - 1
 * (the table-mode step counter, advanced by the last kernel of a step). */
int tdx_p_sample_step_guided(float* x, const float* eps, const float* z, const float* coef, const int64_t* tau,
                             const int32_t* t_idx, int64_t n_half_elems, float w, int use_philox, uint64_t philox_seed,
                             int64_t* counter_dec, tdx_stream_t stream);

/* Clipped-x0 sampling ("clip_denoised", Ho et al. 2020; Imagen's static thresholding): the update in x0 form with the
 * implied x0 clamped to [lo, hi].  coef5: device table (S,5) of rows (p, q, A, Bx, sigma) (schedule.py
 * TimestepSchedule.x0_form), row t = *t_idx:
 *   x0 = p*x + q*out;   x0c = min(max(x0, lo), hi);   x_out = (A*x0c + Bx*x) + sigma*z
 * every product and sum rounded separately, in this order.  out is the network's output (eps or v: the row's p, q say
 * which).  Noise: z (n floats) or NULL, or in-kernel Philox when use_philox != 0 (z ignored) - block j/4, component j%4,
 * stream tau[t] (t when tau == NULL), as tdx_p_sample_step{,_sched}_philox; none at t == 0.  tau, counter_dec as in
 * tdx_p_sample_step_guided.  x_out may be x.  Infinite bounds never bind.  TDX_E_BADARG: a null pointer, n <= 0,
 * n % 4, or not lo < hi (a NaN bound included). */
int tdx_p_sample_step_x0(float* x_out, const float* x, const float* out, const float* z, const float* coef5,
                         const int64_t* tau, const int32_t* t_idx, int64_t n, float lo, float hi, int use_philox,
                         uint64_t philox_seed, int64_t* counter_dec, tdx_stream_t stream);
/* ... guided: the layout, the combination e = out_u + w (out_c - out_u) and the noise of tdx_p_sample_step_guided, then
 * the x0 form above on e; written to both halves of x (in place). */
int tdx_p_sample_step_x0_guided(float* x, const float* out, const float* z, const float* coef5, const int64_t* tau,
                                const int32_t* t_idx, int64_t n_half_elems, float w, float lo, float hi,
                                int use_philox, uint64_t philox_seed, int64_t* counter_dec, tdx_stream_t stream);

/* The multistep sampler (DPM-Solver++(2M), Lu et al. 2022): the x0-form update plus one term in the clamped x0 of the
 * step before.  coef5: device table (S,5) of rows (p, q, A, Bx, H) (schedule.py TimestepSchedule.multistep_form),
 * row t = *t_idx:
 *   x0 = p*x + q*out;   x0c = min(max(x0, lo), hi);   x_out = (A*x0c + Bx*x) + H*hist;   hist = x0c
 * every product and sum rounded separately, in this order; deterministic (no noise).  hist: n floats that the caller
 * keeps from step to step; when the row's H == 0 (the first and the last step, order 1) it is not read and the term is
 * not added, so it never has to be initialised; it is always written.  x_out may be x; counter_dec as in
 * tdx_p_sample_step_x0.  Infinite bounds never bind (no clipping).  TDX_E_BADARG: a null pointer, n <= 0, n % 4, or
 * not lo < hi (a NaN bound included). */
int tdx_p_sample_step_ms(float* x_out, const float* x, const float* out, float* hist, const float* coef5,
                         const int32_t* t_idx, int64_t n, float lo, float hi, int64_t* counter_dec,
                         tdx_stream_t stream);
/* ... guided: the layout and the combination e = out_u + w (out_c - out_u) of tdx_p_sample_step_guided, then the
 * update above on e against one history of n_half_elems floats; written to both halves of x (in place). */
int tdx_p_sample_step_ms_guided(float* x, const float* out, float* hist, const float* coef5, const int32_t* t_idx,
                                int64_t n_half_elems, float w, float lo, float hi, int64_t* counter_dec,
                                tdx_stream_t stream);

/* Inpainting (masked sampling with a known region; Song et al. 2021 I.2, Lugmayr et al. 2022): the two updates above
 * with the clamped prediction blended with the caller's data before the step,
 *   x0m = (1 - mask)*x0c + mask*known          mask = 1 keeps the known value, 0 generates, a fraction is a soft edge
 *   x_out = (A*x0m + Bx*x) + sigma*z           (x0 form; tdx_p_sample_step_x0's arguments)
 *   x_out = (A*x0m + Bx*x) + H*hist; hist = x0m   (multistep form; tdx_p_sample_step_ms's arguments)
 * every operation rounded separately, in this order; known is not clamped.  known, mask: n floats each (guided:
 * n_half_elems, indexed like hist), finite, mask in [0, 1] (the caller checks).  The noise, the Philox indexing, tau,
 * counter_dec, in-place use and the H == 0 rule are the unmasked entries'.  On row 0 (A = 1, Bx = 0, no noise) the result
 * is known wherever mask == 1, bit for bit.  TDX_E_BADARG: the cases of the unmasked entry, or a null known / mask. */
int tdx_p_sample_step_x0_masked(float* x_out, const float* x, const float* out, const float* z, const float* known,
                                const float* mask, const float* coef5, const int64_t* tau, const int32_t* t_idx,
                                int64_t n, float lo, float hi, int use_philox, uint64_t philox_seed,
                                int64_t* counter_dec, tdx_stream_t stream);
int tdx_p_sample_step_x0_guided_masked(float* x, const float* out, const float* z, const float* known,
                                       const float* mask, const float* coef5, const int64_t* tau, const int32_t* t_idx,
                                       int64_t n_half_elems, float w, float lo, float hi, int use_philox,
                                       uint64_t philox_seed, int64_t* counter_dec, tdx_stream_t stream);
int tdx_p_sample_step_ms_masked(float* x_out, const float* x, const float* out, float* hist, const float* known,
                                const float* mask, const float* coef5, const int32_t* t_idx, int64_t n, float lo,
                                float hi, int64_t* counter_dec, tdx_stream_t stream);
int tdx_p_sample_step_ms_guided_masked(float* x, const float* out, float* hist, const float* known, const float* mask,
                                       const float* coef5, const int32_t* t_idx, int64_t n_half_elems, float w,
                                       float lo, float hi, int64_t* counter_dec, tdx_stream_t stream);

/* Every update above behind one entry.  form: the table's rows and the update - TDX_STEP_EPS (S,3) rows (c1, c2, sigma),
 * TDX_STEP_X0 (S,5) rows (p, q, A, Bx, sigma), TDX_STEP_MS (S,5) rows (p, q, A, Bx, H).  n: the elements of x_out / z /
 * hist / known / mask; guided != 0: x and out hold 2n (x_out == x).  Nullable: tau (identity chain), z (no noise; ignored
 * when use_philox), hist (required by MS, which takes no z), known / mask (both or neither, X0 / MS only), counter_dec.
 * lo < hi is required by X0 / MS.  Anything else - a null pointer, n <= 0, n % 4 - is TDX_E_BADARG; nothing is written. */
#define TDX_STEP_EPS 0
#define TDX_STEP_X0 1
#define TDX_STEP_MS 2
int tdx_p_sample_update(float* x_out, const float* x, const float* out, int64_t n, int form, const float* coef,
                        const int32_t* t_idx, const int64_t* tau, const float* z, int use_philox, uint64_t philox_seed,
                        int guided, float w, float lo, float hi, float* hist, const float* known, const float* mask,
                        int64_t* counter_dec, tdx_stream_t stream);

/* Dynamic thresholding (Saharia et al. 2022, Imagen, 2.3): the clamp of the x0 / multistep form with a bound per sample,
 * a quantile of |x0 - c| over the sample, in place of the fixed one.  The data range is [lo, hi], finite, lo < hi;
 * c = (lo + hi) / 2, h = (hi - lo) / 2.  Row t = *t_idx of coef5 gives p and q.  For sample b of n_samples, per elements
 * each, every operation fp32, rounded separately, in the order written:
 *   u_j   = p*x_j + q*o_j - c            o_j: the network's output; guided: out_u + w (out_c - out_u)
 *   a     = sort(|u_j|), ascending
 *   s_q   = a[rank] + frac * (a[min(rank+1, per-1)] - a[rank])
 *   s_b   = max(s_q, h);   r_b = h / s_b
 *   x0c_j = min(max(c + min(max(u_j, -s_b), s_b) * r_b, lo), hi)
 * From x0c on the step is the x0-form / multistep step above: the blend with known / mask, (A*x0 + Bx*x) + sigma*z or
 * + H*hist, and the history stores the thresholded (and blended) value.  Where s_q <= h this is the static clamp
 * (s_b = h, r_b = 1), and the outer clamp keeps x0c in [lo, hi] exactly.  rank, frac: linear interpolation as in
 * torch.quantile(|u|, q, dim=1), computed by the host in fp64: pos = q*(per-1), rank = floor(pos),
 * frac = float32(pos - rank).  |u| is ordered by its bit pattern as an unsigned integer (exact for non-negative floats;
 * a NaN sorts last, and a NaN s_q is written as it is).
 *
 * tdx_x0_dyn_threshold writes (s_b, r_b) of every sample to thr, (n_samples, 2) floats: one workgroup per sample, exact
 * selection by radix over the 32-bit keys with integer LDS histograms (no global atomics; bit-reproducible).  x:
 * n_samples*per floats (guided != 0: the first half of the 2n-row state); out: as many (guided: twice as many, the
 * caller's condition then the null condition).  TDX_E_BADARG, nothing written: a null pointer, n_samples <= 0,
 * per <= 0, per % 4, bounds that are not finite with lo < hi, rank outside [0, per), frac outside [0, 1]. */
int tdx_x0_dyn_threshold(const float* x, const float* out, int n_samples, int per, const float* coef5,
                         const int32_t* t_idx, int guided, float w, float lo, float hi, int rank, float frac, float* thr,
                         tdx_stream_t stream);
/* tdx_p_sample_update with the thresholded x0c: its arguments, then thr (what tdx_x0_dyn_threshold wrote for this x,
 * out and row) and per (element j belongs to sample j / per).  TDX_STEP_X0 and TDX_STEP_MS only.  TDX_E_BADARG, nothing
 * written: the cases of tdx_p_sample_update, TDX_STEP_EPS, a null thr, per <= 0, per % 4, n % per, a bound that is not
 * finite. */
int tdx_p_sample_update_dyn(float* x_out, const float* x, const float* out, int64_t n, int form, const float* coef,
                            const int32_t* t_idx, const int64_t* tau, const float* z, int use_philox,
                            uint64_t philox_seed, int guided, float w, float lo, float hi, float* hist,
                            const float* known, const float* mask, int64_t* counter_dec, float* thr, int per,
                            tdx_stream_t stream);

/* The per-sample sums of the variational bound on the negative log-likelihood (Ho et al. 2020 eq. 5; Nichol & Dhariwal
 * 2021, calc_bpd_loop): what tiny_diffusion_amd.likelihood turns into bits per dimension.
 * rows: device table (T,5) fp32 of (p, q, ex, eo, dec).  Sample b uses row t[b].  Per element, fp32, every
 * operation rounded separately, in this order (x = x_t, o = out):
 *   u = p*x + q*o;  x0c = min(max(u, clip_lo), clip_hi);  d = x0 - x0c;  e = noise - (ex*x + eo*o)
 * terms[b*sample_stride + 0] = sum_j e^2      (0 when noise == NULL)
 * terms[b*sample_stride + 1] = sum_j d^2
 * terms[b*sample_stride + 2] = dec > 0 && bins ? sum_j -log P_j : 0
 * P_j, with s = dec (1/sigma of the decoder), half = (data_hi - data_lo) / (2 (bins - 1)), a = (d + half) s,
 * b = (d - half) s, Phi the standard normal CDF:
 *   x0 < data_lo + half: Phi(a)      x0 > data_hi - half: 1 - Phi(b)      else: Phi(a) - Phi(b)
 * floored at 1e-12 before the log.  Every CDF is evaluated as a tail, Phi(z) = erfc(-z / sqrt 2) / 2, the interior
 * difference on the side where both tails are small (d > 0: Phi(-b) - Phi(-a)), subtracted before the floor; half and
 * the two edges are fp32 expressions of the host.
 * One workgroup per sample, 16-byte loads, one pass over the four inputs (16 B/element); the three sums are reduced
 * inside the wave, then across the waves through LDS in a fixed order (no global atomics): a sample's three numbers are
 * bit-reproducible and do not depend on batch or on the other samples.  sample_stride (floats, >= 3) lets a caller
 * write column t of a (B, T, 3) buffer directly.  t is not range-checked, as in tdx_q_sample.  A row (0, 0, 0, 0, 0) with
 * infinite clip bounds gives d = x0: slot 1 is then sum_j x0^2 (the prior term).
 * TDX_E_BADARG, before any GPU call and with nothing written: a null pointer other than noise, batch <= 0,
 * per_sample <= 0, per_sample % 4, sample_stride < 3, not clip_lo < clip_hi (infinite bounds are allowed, NaN is not),
 * bins == 1 or bins < 0, and with bins >= 2 a data range that is not finite with data_lo < data_hi. */
int tdx_vlb_terms(const float* x0, const float* x_t, const float* out, const float* noise, const int64_t* t,
                  const float* rows, int batch, int per_sample, float clip_lo, float clip_hi, float data_lo,
                  float data_hi, int bins, float* terms, int64_t sample_stride, tdx_stream_t stream);

/* The per-sample squared norm of the model's noise prediction (csrc/analytic.hip): the statistic of the KL-optimal
 * reverse variance (Bao et al. 2022, Analytic-DPM; tiny_diffusion_amd/analytic.py).  With (ex, eo) = rows[t[b]] of the
 * fp32 (T, 2) table - (0, 1) for an eps-model, (sqrt(1 - abar), sqrt(abar)) for a v-model -
 *   sums[b * sample_stride] = sum_i (ex x_t[b,i] + eo out[b,i])^2,
 * each product and sum rounded separately.  One workgroup of 256 per sample, 16-byte loads, one pass over the two
 * inputs (8 B/element); the sum is reduced inside the wave, then across the four waves through LDS in wave order (no
 * global atomics): a sample's number is bit-reproducible and does not depend on batch or on the other samples.
 * sample_stride (floats, >= 1) lets a caller write column k of an (N, S) buffer directly.  t is not range-checked, as
 * in tdx_q_sample.
 * TDX_E_BADARG, before any GPU call and with nothing written: a null pointer, batch <= 0, per_sample <= 0,
 * per_sample % 4, sample_stride < 1. */
int tdx_eps_sqnorm(const float* x_t, const float* out, const int64_t* t, const float* rows, int batch, int per_sample,
                   float* sums, int64_t sample_stride, tdx_stream_t stream);

/* Condition dropout for training the unconditional branch: sample b is dropped iff a Philox uniform in [0,1) keyed by
 * (seed, offset, b) is < p (p == 0: exact copy, p == 1: every sample).  A dropped sample gets label -1 / a zeroed row.
 * The two entries draw the same mask for the same key.  In place (y_out == y, c_out == c) is allowed. */
int tdx_cond_drop_labels(const int64_t* y, int64_t* y_out, int B, float p, uint64_t seed, uint64_t offset,
                         tdx_stream_t stream);
int tdx_cond_drop_rows(const float* c, float* c_out, int B, int dim, float p, uint64_t seed, uint64_t offset,
                       tdx_stream_t stream);

/* Caller side of the path: minibatch gather from a device-resident uint8
 * dataset fused with ToTensor + Normalize((mean,),(std,)) of diffusion.py:202-204:
 *   out[b] = ((u8[idx[b]] / 255) - mean) / std      (idx == NULL: rows 0..batch-1)
 * Bit-exact with the reference's two transforms.  5 B/element. */
int tdx_u8_gather_normalize(const uint8_t* data, const int64_t* idx, float* out, int batch,
                            int per_sample, float mean, float stdv, tdx_stream_t stream);

/* mean((a-b)^2) -> out[0] (F.mse_loss, diffusion.py:231) and its gradient
 * d_a = 2*(a-b)/n * gscale.  Either output may be NULL. */
int tdx_mse_loss(const float* a, const float* b, float* loss_out, float* d_a,
                 float gscale, int64_t n, tdx_stream_t stream);

/* The same loss and gradient in one multi-block pass + a one-block finish (what the fused training step
 * uses: the single-block reduction of tdx_mse_loss is latency-bound and sits between forward and backward).
 * scratch: tdx_mse_scratch_bytes() bytes of device memory, 8-byte aligned.  d_a may be NULL. */
size_t tdx_mse_scratch_bytes(void);
int tdx_mse_loss_grad(const float* a, const float* b, float* loss_out, float* d_a, float gscale,
                      int64_t n, void* scratch, tdx_stream_t stream);
/* ... with a loss weight per timestep (min-SNR weighting, Hang et al. 2023), n = batch*per_sample, sample s of
 * the batch at timestep t[s]:  loss = sum_s w_table[t[s]] sum_j (a-b)^2 / n,  d_a = (a-b) * k_s with
 * k_s = fl(fl(2*gscale/n) * w_table[t[s]]).  Same passes, scratch and summation order as tdx_mse_loss_grad: a table of
 * ones reproduces its loss and gradient bit for bit.  d_a may be NULL.  t is not range-checked (as in tdx_q_sample):
 * w_table, like sqrt_ac / sqrt_1mac, must hold at least max(t) + 1 entries and every t[s] must be >= 0. */
int tdx_mse_loss_grad_weighted(const float* a, const float* b, const int64_t* t, const float* w_table,
                               float* loss_out, float* d_a, float gscale, int batch, int per_sample, void* scratch,
                               tdx_stream_t stream);

/* Training timestep sampling (additions within ABI 400; csrc/timestep.hip): which timestep each sample
 * of a training step sees, from a fixed (T,) probability table or from the loss-second-moment resampler of Nichol &
 * Dhariwal 2021 (3.3).  Every entry: one stream, no allocation, no atomics on global memory, no host synchronisation
 * (capturable), bit-reproducible.  TDX_E_BADARG, nothing launched: a null pointer that is not marked optional, a size
 * <= 0, H < 1, a uniform_prob outside [0, 1].
 *
 * tdx_timestep_cdf: probs (T,) >= 0 and not all zero (negative and NaN entries count as 0; an all-zero table gives the
 * uniform one), one workgroup.  p = probs / sum(probs) and its inclusive prefix sum in double, in a fixed order,
 * rounded once: cdf[k] = fl(sum_{j<=k} p_j) - non-decreasing - and EXACTLY 1.0f from the last k with p_k > 0 on, so that
 * a trailing zero-probability timestep cannot be drawn when the running sum rounds below 1 (leading and interior zeros
 * are skipped by the strict comparison of the draw).  w_eff[k] = fl(w_obj[k] / (T p_k)) with importance != 0 (the
 * weight that keeps E_p[w_eff L] = mean_t w_obj L_t), else w_obj[k]; 0 where p_k == 0.  w_obj == NULL: ones. */
int tdx_timestep_cdf(const float* probs, const float* w_obj, int importance, float* cdf, float* w_eff, int T,
                     tdx_stream_t stream);
/* t_out[b] = #{k : cdf[k] <= u_b} (np.searchsorted(cdf, u, side="right"), by binary search; clamped to T - 1) with
 * u_b = (v[1] >> 8) * 2^-24 in [0, 1), v the Philox4x32-10 block of counter (b, offset) under key seed - word 1, while
 * tdx_cond_drop_* compares word 0 of the same block with its p.  u_out (B,): NULL, or receives u (tests).  rng_dev: NULL,
 * or two device uint64 {seed, offset} read INSTEAD of the by-value pair, as in tdx_transformer_loss_grads (a captured
 * step draws fresh timesteps at every replay). */
int tdx_timestep_draw(const float* cdf, int T, int64_t* t_out, float* u_out, int B, uint64_t seed, uint64_t offset,
                      const uint64_t* rng_dev, tdx_stream_t stream);
/* loss_b[s] = fl(w_obj[t[s]] * sum_j (a[s,j] - b[s,j])^2 / per_sample): the loss of every sample on its own, a pass
 * beside tdx_mse_loss_grad* (whose element -> block mapping stays as it is).  One workgroup of 256 per sample, 16-byte
 * loads when a and b are 16-byte aligned and per_sample % 4 == 0, differences, squares and sums in double in a fixed
 * order, one rounding.  w_obj == NULL: weight 1, and t may then be NULL too.  t is not range-checked. */
int tdx_mse_per_sample(const float* a, const float* b, const int64_t* t, const float* w_obj, float* loss_b, int batch,
                       int per_sample, tdx_stream_t stream);
/* The resampler's state and table, one workgroup.  history (T,H) holds the last H losses of every timestep, oldest
 * first, counts (T,) int32 how many are valid (both zero at the start).  1. The state after the call is that of
 * applying samples b = 0 .. B-1 IN BATCH ORDER - counts[t_b] < H appends, a full row drops its oldest entry and appends:
 * improved-DDPM's sequential update, duplicates of a timestep inside the batch included (each sample's place follows
 * from how many samples of its timestep come before it; no atomics); a t_b outside [0, T) is skipped.  T <= 4096
 * (TDX_E_SHAPE otherwise: the per-timestep moments of phase 3 live in LDS).  2. Warmed up iff every counts[k] == H.  3. Not warmed up: cdf[k] = fl((k + 1) / T), w_eff =
 * w_obj, exactly.  Warmed up: w_k = sqrt(mean_h history[k,h]^2), p = w / sum(w), p = p (1 - uniform_prob) +
 * uniform_prob / T in double, then cdf and w_eff as tdx_timestep_cdf writes them with importance = 1 (all-zero
 * losses: the uniform p).  B == 0 (t and loss_b may be NULL) only rebuilds cdf / w_eff from the state: after loading
 * one, or when w_obj changed. */
int tdx_timestep_history_update(const int64_t* t, const float* loss_b, int B, float* history, int32_t* counts, int H,
                                float uniform_prob, const float* w_obj, float* cdf, float* w_eff, int T,
                                tdx_stream_t stream);

/* Progressive distillation (additions within ABI 400; csrc/distill.hip; Salimans & Ho 2022, Algorithm
 * 2): two deterministic DDIM steps of a frozen teacher at PER-SAMPLE timesteps and the target with which ONE DDIM step
 * of the student lands where they did.  Sample b reads row t[b] of rows, a (T, 12) fp32 table
 *   (p1, q1, A1, B1,  p2, q2, A2, B2,  W2, W1, G, H)          (schedule.distill_tables; 16-byte aligned)
 * - two rows (p, q, A, Bx) of the x0 form (TDX_STEP_X0) of the teacher's grid, the convex weights of the student's
 * x0 and the map from it to the student's target - and with clamp(v) = min(max(v, lo), hi):
 *   tdx_distill_teacher_step:  x1c = clamp(p1 z_t + q1 out1),   z_mid = A1 x1c + B1 z_t,   t_mid[b] = t_mid_table[t[b]]
 *   tdx_distill_target:        x2c = clamp(p2 z_mid + q2 out2), x~ = W2 x2c + W1 x1c,      target = G x~ + H z_t
 * out1 = teacher(z_t, t), out2 = teacher(z_mid, t_mid).  Every product and sum is rounded separately in the order
 * written: the arithmetic of tdx_p_sample_update(form = TDX_STEP_X0) without its noise term, so z_mid is that entry's
 * result bit for bit when every sample sits on one row.  Infinite bounds never bind.  x_tilde may be NULL (not
 * written; target is the same bits).  t is not range-checked, as in tdx_q_sample: rows and t_mid_table must hold
 * max(t) + 1 entries.  Elementwise, float4 accesses, grid-strided, no LDS, no atomics, one stream, capturable: 16 B per
 * element and 20 B (24 B with x_tilde).  TDX_E_BADARG, before any GPU call and with nothing written: a null pointer
 * other than x_tilde, batch <= 0, per_sample <= 0, per_sample % 4 (a float4 must not straddle two samples), not lo < hi
 * (a NaN bound included). */
int tdx_distill_teacher_step(const float* z_t, const float* out1, const int64_t* t, const float* rows,
                             const int64_t* t_mid_table, float* z_mid, float* x1c, int64_t* t_mid, int batch,
                             int per_sample, float lo, float hi, tdx_stream_t stream);
int tdx_distill_target(const float* z_t, const float* z_mid, const float* out2, const float* x1c, const int64_t* t,
                       const float* rows, float* target, float* x_tilde, int batch, int per_sample, float lo, float hi,
                       tdx_stream_t stream);

/* Guided distillation (additions within ABI 400; csrc/distill.hip; Meng et al. 2023): the teacher is
 * sampled under classifier-free guidance and the student's ONE conditional evaluation learns the combination.  Guided
 * layout as in tdx_p_sample_step_guided: with n = batch * per_sample, out1 / out2 hold 2n floats - the rows under the
 * caller's condition, then the rows under the null condition - and for j < n
 *   e[j] = out[j + n] + w (out[j] - out[j + n])                 (each operation rounded separately: common.h cfg_eps)
 * takes the place of the teacher's output; out[j] == out[j + n] gives out[j + n] bit for bit, whatever w.  The
 * arithmetic that follows is the unguided entries', operation for operation:
 *   tdx_distill_teacher_step_guided:  x1c = clamp(p1 z_t + q1 e1),   z_mid = A1 x1c + B1 z_t
 *       z_mid (2n floats) is written to both halves and t_mid (2 batch entries) to both halves: with them and the
 *       doubled condition the teacher's second forward runs as is.  z_t, x1c: n floats (z_t may be the first half of
 *       the 2n-float input of the first forward).
 *   tdx_distill_target_guided:        x2c = clamp(p2 z_mid + q2 e2), x~ = W2 x2c + W1 x1c,   target = G x~ + H z_t
 *       z_mid: its first n floats are read; target, x_tilde (nullable): n floats.
 *   tdx_distill_guidance_target:      x0c = clamp(p z_t + q e),      target = G x0c + H z_t
 *       the same-timestep step (stage one of Meng et al.): sample b reads row t[b] of rows, a (T, 4) fp32 table
 *       (p, q, G, H) (schedule.guidance_distill_table; 16-byte aligned) - (p, q) of the x0 form at timestep t, (G, H) the
 *       map from x0 to the student's target.  guided != 0: out holds 2n floats and e is the combination; guided == 0:
 *       out holds n floats, e = out and w is not read - a change of parameterisation (an eps teacher, a v student).
 *       x0c may be NULL (not written; target is the same bits).
 * t is not range-checked.  Elementwise, float4 accesses, grid-strided, no LDS, no atomics, one stream, capturable.  Per
 * element of the n: 24 B (reads z_t and two of out1, writes two of z_mid and x1c); 24 B (28 B with x_tilde); 12 B
 * unguided and 16 B guided (4 B more with x0c).  TDX_E_BADARG, before any GPU call and with nothing written: a null
 * pointer other than x_tilde / x0c, batch <= 0, per_sample <= 0, per_sample % 4, not lo < hi (a NaN bound included), a w
 * that is not finite (tdx_distill_guidance_target: when guided != 0). */
int tdx_distill_teacher_step_guided(const float* z_t, const float* out1, const int64_t* t, const float* rows,
                                    const int64_t* t_mid_table, float* z_mid, float* x1c, int64_t* t_mid, int batch,
                                    int per_sample, float w, float lo, float hi, tdx_stream_t stream);
int tdx_distill_target_guided(const float* z_t, const float* z_mid, const float* out2, const float* x1c,
                              const int64_t* t, const float* rows, float* target, float* x_tilde, int batch,
                              int per_sample, float w, float lo, float hi, tdx_stream_t stream);
int tdx_distill_guidance_target(const float* z_t, const float* out, const int64_t* t, const float* rows, float* target,
                                float* x0c, int batch, int per_sample, int guided, float w, float lo, float hi,
                                tdx_stream_t stream);

/* Adam, torch defaults (diffusion.py:211/236): one fused pass over a flat
 * parameter buffer, 28 B/param.  step is the 1-based step count. */
int tdx_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  int64_t n, float lr, float beta1, float beta2, float eps, int step,
                  float grad_scale, tdx_stream_t stream);

/* The same update with the step-dependent scalars in device memory, for a training step captured
 * in a HIP graph: hyper[0] = lr / (1 - beta1^step), hyper[1] = 1 / sqrt(1 - beta2^step),
 * hyper[2] = grad_scale (the host refreshes the three floats before each replay). */
int tdx_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                      int64_t n, const float* hyper, float beta1, float beta2, float eps,
                      tdx_stream_t stream);

/* torch.nn.utils.clip_grad_norm_(params, max_norm) + Adam (conditional_diffusion_laion.py:469-472) fused:
 * a fixed-order sum of squares of the flat gradient, then the Adam pass applies
 *   g * grad_scale * min(1, max_norm / (sqrt(sum g^2) * |grad_scale| + 1e-6))
 * on the fly (the clipped gradient is never written back).  hyper_dev: NULL, or the three device
 * floats of tdx_adam_step_dev (then lr / step / grad_scale are ignored): graph-capturable.
 * scratch: tdx_adam_clip_scratch_bytes() bytes of device memory, 8-byte aligned. */
size_t tdx_adam_clip_scratch_bytes(void);
int tdx_adam_step_clip(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                       int64_t n, float lr, float beta1, float beta2, float eps, int step,
                       float grad_scale, float max_norm, const float* hyper_dev, void* scratch,
                       tdx_stream_t stream);

/* Adam with an exponential moving average of the parameters fused into the same pass (36 B/param): the
 * three updates above, bit-identical in param / exp_avg / exp_avg_sq, and for the same element
 *   ema = ema + ema_one_minus_decay * (param_new - ema)
 * as three separately rounded fp32 operations (torch's e + a * (p - e)).  ema_one_minus_decay = 1 - decay in
 * [0, 1]; in the device-scalar forms it is hyper4[3], after the three floats of tdx_adam_step_dev (the clip
 * form with hyper4_dev then ignores lr / step / grad_scale / ema_one_minus_decay).  ema must not overlap
 * param.  No alignment requirement beyond fp32's; no allocation, no synchronisation, graph-capturable. */
int tdx_adam_ema_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                      int64_t n, float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                      float ema_one_minus_decay, tdx_stream_t stream);
int tdx_adam_ema_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                          int64_t n, const float* hyper4, float beta1, float beta2, float eps, tdx_stream_t stream);
int tdx_adam_ema_step_clip(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                           int64_t n, float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                           float max_norm, float ema_one_minus_decay, const float* hyper4_dev, void* scratch,
                           tdx_stream_t stream);

/* Exchange the contents of two fp32 buffers of n elements in place (16 B/element; the ranges must not
 * overlap): how TrainStep.ema_weights() puts the averaged weights where every plan and captured graph
 * already points. */
int tdx_swap_f32(float* a, float* b, int64_t n, tdx_stream_t stream);

/* ---- building blocks (exported for unit tests and re-use) --------------- */

/* OIHW (Cout,Cin,3,3) -> forward pack [Cout][9][Cin] and dgrad pack
 * [Cin][9 flipped][Cout].  Either destination may be NULL. */
int tdx_pack_conv3x3(const float* w_oihw, float* w_fwd, float* w_dgrad, int cout, int cin,
                     tdx_stream_t stream);

/* Flags for tdx_conv3x3_fwd */
#define TDX_CONV_IN_BNRELU 1   /* input is a pre-BN tensor: apply relu(x*in_scale+in_shift) on load */
#define TDX_CONV_OUT_BNRELU 2  /* epilogue: out = relu((acc+bias)*out_scale+out_shift)  (inference) */
#define TDX_CONV_OUT_STATS 4   /* epilogue: also emit per-tile per-channel (sum, sumsq) partials */

/* The two boundary convolutions (diffusion.py:28 initial_conv / :98 final_conv, applied at :116 and :160;
 * conditional_diffusion_laion.py:244, 296), on the fp32 MFMA with the thin side gathered from NCHW:
 *   initial_conv  x (B,cin,H,W) NCHW, w (cout,cin,3,3), bias (cout) -> out (B,H,W,64) channels-last; channels
 *                 >= cout are written as zeros.  (cin, cout) = (1, 64) MNIST | (4, 32) LAION latents.
 *   final_conv    in (B,H,W,64) channels-last, w (cout,64,3,3), bias (cout) -> out (B,cout,H,W) NCHW; cout = 1 | 4.
 * backward: g_out in the forward output's layout; dw / db in the parameter's layout; the input gradient of
 * final_conv (g_in, channels-last) - initial_conv's input is the data, it has none.  scratch:
 * tdx_edge_conv_wgrad_scratch_floats(B,H,W) floats (consumed).  H and W are independent (any H >= 1).  The two backward
 * entries need W >= 4 (their kernel walks the pixels in pairs) and return TDX_E_SHAPE for a narrower map before anything
 * is written, g_in included; the forwards and tdx_initial_conv_input_grad take any W >= 1.  Other channel counts:
 * TDX_E_SHAPE. */
size_t tdx_edge_conv_wgrad_scratch_floats(int B, int H, int W);
int tdx_initial_conv_forward(const float* x, const float* w, const float* bias, float* out, int B, int H, int W,
                             int cin, int cout, tdx_stream_t stream);
int tdx_initial_conv_backward(const float* x, const float* g_out, float* dw, float* db, float* scratch, int B,
                              int H, int W, int cin, int cout, tdx_stream_t stream);
/* d loss / d x: the input gradient of initial_conv (NCHW (B,cin,H,W)) from the gradient of its output
 * (channels-last, 64 stored channels).  The reference's module is differentiable in x like any nn.Module
 * (diffusion.py:116); train() and sample() never ask for it. */
int tdx_initial_conv_input_grad(const float* g_out, const float* w, float* g_x, int B, int H, int W, int cin,
                                int cout, tdx_stream_t stream);
int tdx_final_conv_forward(const float* in, const float* w, const float* bias, float* out, int B, int H, int W,
                           int cout, tdx_stream_t stream);
int tdx_final_conv_backward(const float* in, const float* g_out, const float* w, float* g_in, float* dw, float* db,
                            float* scratch, int B, int H, int W, int cout, tdx_stream_t stream);
/* The same five with the storage flag of the bf16 mode: io16 != 0 -> the FAT channels-last tensor of 64 stored channels
 * (`out` of initial_conv; `g_out` of its two backward entries; `in` and `g_in` of final_conv) holds bf16, widened on load
 * and rounded to nearest-even once on store; the thin NCHW tensor, the weights, bias, dw, db and scratch stay fp32.
 * io16 == 0: exactly the entries above, refusals (W < 4, channel counts) included. */
int tdx_initial_conv_forward_io(const float* x, const float* w, const float* bias, void* out, int B, int H, int W,
                                int cin, int cout, int io16, tdx_stream_t stream);
int tdx_initial_conv_backward_io(const float* x, const void* g_out, float* dw, float* db, float* scratch, int B,
                                 int H, int W, int cin, int cout, int io16, tdx_stream_t stream);
int tdx_initial_conv_input_grad_io(const void* g_out, const float* w, float* g_x, int B, int H, int W, int cin,
                                   int cout, int io16, tdx_stream_t stream);
int tdx_final_conv_forward_io(const void* in, const float* w, const float* bias, float* out, int B, int H, int W,
                              int cout, int io16, tdx_stream_t stream);
int tdx_final_conv_backward_io(const void* in, const float* g_out, const float* w, void* g_in, float* dw, float* db,
                               float* scratch, int B, int H, int W, int cout, int io16, tdx_stream_t stream);

/* 3x3, pad 1, stride 1 convolution as an implicit GEMM on fp32 MFMA
 * (nn.Conv2d(cin,cout,3,padding=1), diffusion.py:28-98), NHWC.
 *   in  (B,H,W,cin)  wpk [cout][9][cin]  bias (cout) or NULL  out (B,H,W,cout)
 * With the dgrad pack and the roles of cin/cout swapped the same entry point
 * computes the input gradient.  cin % 32 == 0, cout % 64 == 0; any H, W >= 1, independent of each other (so for
 * every direct forward below: _splitk, _train, _infer, tdx_conv3x3_dgrad).
 * stats_partial (when TDX_CONV_OUT_STATS): [tdx_conv3x3_stat_tiles(...)][2][cout] holding,
 * per tile of tdx_conv3x3_stat_tile_rows(...) output pixels and per channel, the sum
 * and the sum of squared deviations from the TILE mean (merged by tdx_bn_finalize). */
int tdx_conv3x3_fwd(const float* in, const float* wpk, const float* bias, float* out,
                    int B, int H, int W, int cin, int cout, int flags,
                    const float* in_scale, const float* in_shift,
                    const float* out_scale, const float* out_shift,
                    float* stats_partial, tdx_stream_t stream);
/* Same convolution for latency-bound (small batch) shapes: when the tile grid would leave
 * most of the 256 CUs idle, K = 9*cin is split over more workgroups, partial sums go to
 * `scratch` (tdx_conv3x3_splitk_scratch_floats; 0 = no split for this shape) and a second
 * launch reduces them in a fixed order and applies bias / the BN+ReLU epilogue.
 * TDX_CONV_OUT_STATS is not available on this path. */
int tdx_conv3x3_fwd_splitk(const float* in, const float* wpk, const float* bias, float* out,
                           int B, int H, int W, int cin, int cout, int flags,
                           const float* in_scale, const float* in_shift,
                           const float* out_scale, const float* out_shift,
                           float* scratch, size_t scratch_floats, tdx_stream_t stream);
size_t tdx_conv3x3_splitk_scratch_floats(int B, int H, int W, int cin, int cout);
/* The same convolution by Winograd's F(2x2, 3x3) on the fp32 MFMA (csrc/conv3x3_wino.hip): 16 multiplications per
 * (input channel, output channel, 2x2 output tile) instead of 36, input and output transforms fused into the kernel;
 * equal to tdx_conv3x3_fwd up to fp32 rounding (the transforms add and halve).  Raw NHWC input; cin % 64 == 0,
 * cout % 64 == 0; H and W even, or (H+1)/2 * (W+1)/2 dividing 64 (tdx_conv3x3_wino_ok).  Weights: tdx_pack_conv3x3_wino
 * (u_fwd for the forward; u_dgrad, channel roles swapped and taps mirrored, makes the same entry the input gradient:
 * in = dy, cin/cout swapped).  flags: 0, TDX_CONV_OUT_BNRELU or TDX_CONV_OUT_STATS; the statistics partials are
 * [tdx_conv3x3_wino_stat_tiles][2][cout] over tiles of tdx_conv3x3_wino_stat_tile_rows output pixels (same format as
 * tdx_conv3x3_fwd's, other tiling). */
int tdx_conv3x3_wino_ok(int B, int H, int W, int cin, int cout);
int tdx_pack_conv3x3_wino(const float* w_oihw, float* u_fwd, float* u_dgrad, int cout, int cin, tdx_stream_t stream);
int tdx_conv3x3_fwd_wino(const float* in, const float* u, const float* bias, float* out, int B, int H, int W,
                         int cin, int cout, int flags, const float* out_scale, const float* out_shift,
                         float* stats_partial, tdx_stream_t stream);
/* Inference form (reverse process, diffusion.py:254-276): relu((conv + bias) * out_scale + out_shift) with the input
 * channels split over more workgroups where the launch would not fill the chip (one Winograd workgroup per CU); partials
 * in `scratch` (any size: the plan splits as far as it reaches; NULL: never split), summed in a fixed order. */
int tdx_conv3x3_fwd_wino_infer(const float* in, const float* u, const float* bias, float* out, int B, int H, int W,
                               int cin, int cout, const float* out_scale, const float* out_shift, float* scratch,
                               size_t scratch_floats, tdx_stream_t stream);
/* 1 when a training step of the UNets at batch B runs this layer's forward (role 0) / input gradient (role 1) on the
 * Winograd kernel (tuning knobs "wino", "wino_min_wgs"), 0: on the direct kernels - what bench.py's roofline leg times.
 * Those launches run the main loop whose waves split the transform rows (knob "wino_rows", default 1; 0: the loop whose
 * waves split the output channels; "wino_rows_min_stages": only launches of at least that many 8-channel K-stages take
 * the row split) - bit-identical results either way. */
int tdx_conv3x3_train_algo(int B, int H, int W, int cin, int cout, int role);
/* 1 when a sampling (INFER-mode) forward of B samples runs this layer on tdx_conv3x3_fwd_wino_infer (tuning knobs
 * "wino_infer", "wino_infer_min_units", "infer_ring"), 0: on the direct kernels (split-K tdx_conv3x3_fwd_splitk). */
int tdx_conv3x3_infer_algo(int B, int H, int W, int cin, int cout);
/* Weight gradient by F(3x3, 2x2) (the transposition of the forward's identity; both operands transformed on the fly):
 * dw_slabs = [tdx_conv3x3_wgrad_wino_splits(...)][cout][9][cin], the slab format of tdx_conv3x3_wgrad - sum with
 * tdx_conv3x3_wgrad_reduce.  Raw NHWC input and dy; cin % 64 == 0, cout % 64 == 0; any H, W. */
int tdx_conv3x3_wgrad_wino_splits(int B, int H, int W, int cin, int cout);
int tdx_conv3x3_wgrad_wino(const float* in, const float* dy, float* dw_slabs, int B, int H, int W, int cin, int cout,
                           tdx_stream_t stream);
int tdx_conv3x3_wino_stat_tiles(int B, int H, int W);
int tdx_conv3x3_wino_stat_tile_rows(int B, int H, int W);
/* The INFERENCE convolution of the reverse process (diffusion.py:254-276: one eval-mode UNet forward per step, n = 16
 * samples by default - M = 256 .. 16384 pixels per layer): out = [relu(] (conv3x3(in, W) + bias) [* out_scale +
 * out_shift)] (scale / shift both NULL: bias only).  Weights in the TILE-MAJOR pack written by tdx_pack_conv3x3_tiled
 * ([cout/64][(ci/32)*9 + tap][64][32], rows pre-swizzled: conv3x3.hip); cin % 32 == 0, cout % 64 == 0; raw NHWC input.
 * 64x64 tiles on a 4-stage LDS-DMA ring; K is split where that shortens the busiest CU's queue (plan inside), partials
 * go to `scratch` and a second launch sums them in a fixed order.  scratch: at least
 * tdx_conv3x3_infer_scratch_floats(...) floats (0: this shape never splits, scratch may be NULL). */
int tdx_pack_conv3x3_tiled(const float* w_oihw, float* w_tiled, int cout, int cin, tdx_stream_t stream);
int tdx_conv3x3_fwd_infer(const float* in, const float* w_tiled, const float* bias, float* out, int B, int H, int W,
                          int cin, int cout, const float* out_scale, const float* out_shift, float* scratch,
                          size_t scratch_floats, tdx_stream_t stream);
size_t tdx_conv3x3_infer_scratch_floats(int B, int H, int W, int cin, int cout);
/* The TRAINING form (flags: 0 or TDX_CONV_OUT_STATS; raw input): tdx_conv3x3_fwd, except that shapes whose
 * tile grid would put one lone workgroup on a CU (few pixels, long K: the bottleneck of the UNet at B = 256)
 * run as 64x64 tiles with K split, and a second launch reduces the partials in a fixed order, adds the bias
 * and writes the same [stat_tiles][2][cout] statistics partials.  `scratch`: at least
 * tdx_conv3x3_train_scratch_floats(...) floats (0 = this shape never splits; scratch may then be NULL).
 * With the dgrad pack and cin/cout swapped it is the input gradient, as tdx_conv3x3_dgrad. */
int tdx_conv3x3_fwd_train(const float* in, const float* wpk, const float* bias, float* out, int B, int H, int W,
                          int cin, int cout, int flags, float* stats_partial, float* scratch,
                          size_t scratch_floats, tdx_stream_t stream);
size_t tdx_conv3x3_train_scratch_floats(int B, int H, int W, int cin, int cout);
int tdx_conv3x3_stat_tiles(int B, int H, int W, int cin, int cout);
int tdx_conv3x3_stat_tile_rows(int B, int H, int W, int cin, int cout);
/* 1 when (B,H,W,cin,cout) is addressable by the convolution kernels: they use 32-bit buffer
 * offsets with 0x80000000 as the zero-padding sentinel, so every activation tensor of the layer
 * (plus (W+1) pixels of slack on both sides) must stay below 2 GiB; the entry points return
 * TDX_E_SHAPE otherwise (MNIST UNet: per-GPU batch <= 2047). */
int tdx_conv3x3_shape_ok(int B, int H, int W, int cin, int cout);
/* Launch geometry a shape resolves to, bm*1000 + bn (introspection for tests: every tile
 * template must be covered by a direct oracle check).  role 0: forward (and dgrad, called with
 * the channel roles swapped), role 1: weight gradient. */
int tdx_conv3x3_tile_shape(int B, int H, int W, int cin, int cout, int role);

/* dx = d(conv3x3)/d(input) (autograd of diffusion.py:32-95 convolutions): the same implicit GEMM
 * with the roles of the channels swapped and the taps mirrored.
 *   dy (B,H,W,cout) NHWC; w_dgrad: the second output of tdx_pack_conv3x3; dx (B,H,W,cin) NHWC. */
int tdx_conv3x3_dgrad(const float* dy, const float* w_dgrad, float* dx, int B, int H, int W,
                      int cin, int cout, tdx_stream_t stream);

/* Weight gradient of the same convolution:
 *   dw_slabs[s][cout][9][cin] partial sums over pixel chunk s (split-K, deterministic)
 * followed by tdx_conv3x3_wgrad_reduce -> OIHW gradient.  `in` may be a pre-BN
 * tensor (TDX_CONV_IN_BNRELU with in_scale/in_shift).  cin % 64 == 0, cout % 64 == 0; any H, W >= 1, independent of
 * each other (narrow and one-row maps included). */
int tdx_conv3x3_wgrad_splits(int B, int H, int W, int cin, int cout);
int tdx_conv3x3_wgrad(const float* in, const float* dy, float* dw_slabs,
                      int B, int H, int W, int cin, int cout, int flags,
                      const float* in_scale, const float* in_shift, tdx_stream_t stream);
int tdx_conv3x3_wgrad_reduce(const float* dw_slabs, float* dw_oihw, int splits, int cout, int cin,
                             tdx_stream_t stream);

/* ---- bf16 compute mode (opt-in; BASELINE.json configs[3]/[4]; the reference is fp32-only) --------
 * The same three GEMMs on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16) with fp32 accumulation.
 * Tensors stay fp32 in memory; the MFMA operands are rounded to bf16 (nearest even) while a tile is
 * staged, weights are packed to bf16 by tdx_pack_conv3x3_bf16 ([cout][9][cin] / [cin][9][cout], 2 bytes
 * per element).  Arguments as tdx_conv3x3_fwd / _wgrad; cin % 64 == 0, cout % 64 == 0; statistics
 * tiles are always tdx_conv3x3_bf16_stat_tile_rows() = 128 pixels; the weight gradient writes the fp32
 * path's slab layout (same reduce) in tdx_conv3x3_wgrad_splits_bf16(...) slabs - its own split plan: the
 * bf16 kernel is bound by L2 bandwidth, not MFMA rate, and wants bigger tiles.  Tolerance: tests/test_gpu_bf16.py. */
int tdx_conv3x3_wgrad_splits_bf16(int B, int H, int W, int cin, int cout);
/* The bf16 STORAGE forms (round 3): io16 != 0 -> `in`, `out` / `dy` hold bf16 elements (the activation tensors of
 * a plan in bf16 mode); io16 == 0 -> exactly tdx_conv3x3_fwd_bf16 / tdx_conv3x3_wgrad_bf16.  bias, scale / shift,
 * statistics partials and the weight-gradient slabs are fp32 either way. */
int tdx_conv3x3_fwd_bf16_io(const void* in, const void* wpk_bf16, const float* bias, void* out, int B, int H, int W,
                            int cin, int cout, int flags, const float* in_scale, const float* in_shift,
                            const float* out_scale, const float* out_shift, float* stats_partial, int io16,
                            tdx_stream_t stream);
int tdx_conv3x3_wgrad_bf16_io(const void* in, const void* dy, float* dw_slabs, int B, int H, int W, int cin, int cout,
                              int flags, const float* in_scale, const float* in_shift, int io16, tdx_stream_t stream);
int tdx_pack_conv3x3_bf16(const float* w_oihw, void* w_fwd_bf16, void* w_dgrad_bf16, int cout, int cin,
                          tdx_stream_t stream);
int tdx_conv3x3_bf16_stat_tile_rows(void);
int tdx_conv3x3_fwd_bf16(const float* in, const void* wpk_bf16, const float* bias, float* out,
                         int B, int H, int W, int cin, int cout, int flags,
                         const float* in_scale, const float* in_shift,
                         const float* out_scale, const float* out_shift,
                         float* stats_partial, tdx_stream_t stream);
int tdx_conv3x3_wgrad_bf16(const float* in, const float* dy, float* dw_slabs,
                           int B, int H, int W, int cin, int cout, int flags,
                           const float* in_scale, const float* in_shift, tdx_stream_t stream);

/* BatchNorm2d (diffusion.py:34 ...): turn the conv epilogue's partials into
 * per-channel scale/shift (+ saved mean/rstd) and update the running buffers.
 * Tile t covers rows [t*tile_rows, min((t+1)*tile_rows, count)); partials are merged
 * with Chan's parallel-variance formula in double precision.
 *   training != 0: batch statistics (biased var to normalise, unbiased into
 *                  running_var, momentum 0.1, num_batches_tracked += 1)
 *   training == 0: scale/shift from the running statistics.
 * C % 4 == 0 (the kernel reads four channels of a tile at once); TDX_E_SHAPE otherwise, nothing is written. */
int tdx_bn_finalize(const float* stats_partial, int tiles, int tile_rows, int64_t count, int C,
                    const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked,
                    float* scale, float* shift, float* save_mean, float* save_rstd,
                    int training, tdx_stream_t stream);

/* a = relu(y*scale + shift): the normalised activation written out (BatchNorm2d + ReLU,
 * diffusion.py:34-35) for consumers that want it materialised; scale/shift from tdx_bn_finalize.
 *   y, out (rows, C) NHWC rows; C % 4 == 0. */
int tdx_bn_apply_relu_fwd(const float* y, float* out, int64_t rows, int C, const float* scale,
                          const float* shift, tdx_stream_t stream);

/* BN+ReLU backward, in place on g (B*H*W, C):
 *   gz = g * [y*scale+shift > 0];  dgamma = sum gz*xhat;  dbeta = sum gz
 *   training: g <- gamma*rstd*(gz - dbeta/N - xhat*dgamma/N)   else g <- gz*scale
 * Also returns dbias = column sums of the result (gradient of the conv bias).
 * Widths: C in {4, 8, 16, 32, 64, 128, 256, 512, 1024} (C % 4 == 0, C <= 1024, 256 % (C / 4) == 0: a workgroup of 256
 * threads holds whole rows).  Any other C: TDX_E_SHAPE, and tdx_bn_relu_bwd_scratch_floats returns 0.
 * scratch: tdx_bn_relu_bwd_scratch_floats(rows, C) floats. */
int tdx_bn_relu_bwd(float* g, const float* y, int64_t rows, int C,
                    const float* scale, const float* shift, const float* save_mean,
                    const float* save_rstd, const float* gamma,
                    float* dgamma, float* dbeta, float* dbias, float* scratch,
                    int training, tdx_stream_t stream);
size_t tdx_bn_relu_bwd_scratch_floats(int64_t rows, int C);

/* MaxPool2d(2, ceil_mode=True) (diffusion.py:101) over relu(y*scale+shift)
 * (scale == NULL: raw input).  (B,H,W,C) -> (B,ceil(H/2),ceil(W/2),C). */
int tdx_maxpool2_ceil_fwd(const float* y, const float* scale, const float* shift, float* out,
                          int B, int H, int W, int C, tdx_stream_t stream);
/* g_in = (skip_grad or 0) + route(g_out to the first arg-max of each window). */
int tdx_maxpool2_ceil_bwd(const float* y, const float* scale, const float* shift,
                          const float* g_out, const float* skip_grad, float* g_in,
                          int B, int H, int W, int C, tdx_stream_t stream);

/* Bilinear resize, align_corners=True (nn.Upsample / F.interpolate,
 * diffusion.py:102, 135-159) of relu(y*scale+shift) + addend[n][c]
 * (scale == NULL: raw input; addend == NULL: none).  The destination may be a
 * channel slice of a wider tensor: out[(pixel)*out_cstride + out_coff + c]. */
int tdx_bilinear_ac_fwd(const float* in, const float* scale, const float* shift,
                        const float* addend, float* out,
                        int B, int Hi, int Wi, int Ho, int Wo, int C,
                        int out_cstride, int out_coff, tdx_stream_t stream);
/* Transposed resize: g_in (B,Hi,Wi,C) from g_out slice (B,Ho,Wo,[coff:coff+C]).
 * Contributor limit: an input index may receive from at most 8 contributing outputs per axis.  It is decided per axis on
 * the candidate window of every input index i, [floor((i-1)/s) - 1, ceil((i+1)/s) + 1] clipped to the output, with
 * s = (n_in-1)/(n_out-1) in fp32 (s == 0, i.e. n_in == 1 or n_out == 1: the whole output): more than 8 candidates for any
 * i returns TDX_E_SHAPE and leaves g_in untouched.  n_out <= 2 n_in always passes (every resize of the networks);
 * 2 -> 9, 1 -> 9, 3 -> 9 and 4 -> 14 are among the smallest that do not.  tdx_bilinear_ac_fwd has no such limit.
 * Both entries: C, cstride and coff multiples of 4, coff + C <= cstride; TDX_E_SHAPE otherwise. */
int tdx_bilinear_ac_bwd(const float* g_out, float* g_in,
                        int B, int Hi, int Wi, int Ho, int Wo, int C,
                        int g_cstride, int g_coff, tdx_stream_t stream);

/* ---- the storage-flag (_io) forms of the HBM-bound kernels, and the sum-emitting producers -----------------
 * What a plan in bf16 mode (tdx_unet_set_precision(TDX_PREC_BF16)) and the default training step launch, one kernel
 * at a time, so each can be held against a reference on its own (tests/test_gpu_io16_dispatch.py).  io16 != 0: every
 * `void*` ACTIVATION tensor (channels-last activations and activation gradients) holds bf16 - widened exactly on load,
 * arithmetic in fp32, ONE round-to-nearest-even on store; io16 == 0: they hold fp32 and the call is exactly the fp32
 * entry of the same name without the suffix.  Per-channel operands (scale, shift, mean, rstd, gamma, addend, bias),
 * partial sums, dgamma / dbeta / dbias and every thin (NCHW) tensor, weight and weight gradient are fp32 either way.
 * Layouts, channel rules and refusals are those of the fp32 entry unless stated.  Every refusal (TDX_E_BADARG: a NULL
 * or non-positive argument; TDX_E_SHAPE: a width the kernel does not have) comes before the first launch and writes
 * nothing.  No new kernel, no new arithmetic: additions within ABI 400. */

/* tdx_bn_apply_relu_fwd.  io16 != 0 needs C % 8 == 0 (the bf16 kernel handles eight channels per thread):
 * TDX_E_SHAPE otherwise, like every other width refusal of this header.  io16 == 0 answers C % 4 != 0 as
 * tdx_bn_apply_relu_fwd always has (TDX_E_BADARG); C = 12 is therefore computed in fp32 and refused in bf16. */
int tdx_bn_apply_relu_fwd_io(const void* y, void* out, int64_t rows, int C, const float* scale, const float* shift,
                             int io16, tdx_stream_t stream);
/* tdx_bn_relu_bwd: reduction pass over (g, y), finalize, in-place apply pass; g and y (rows, C) in the storage type.
 * In bf16 the reduction reads the STORED (rounded) gradient.  scratch: tdx_bn_relu_bwd_scratch_floats(rows, C). */
int tdx_bn_relu_bwd_io(void* g, const void* y, int64_t rows, int C, const float* scale, const float* shift,
                       const float* save_mean, const float* save_rstd, const float* gamma, float* dgamma,
                       float* dbeta, float* dbias, float* scratch, int training, int io16, tdx_stream_t stream);
/* The same WITHOUT the reduction pass: partial [nblk][2][C] (per block and channel: sum gz, then sum gz * xhat) is
 * already in memory - written by a producer below, or by the caller.  The blocks are added in double in a fixed order;
 * dgamma / dbeta / dbias (each may be NULL), then g <- the input gradient in place.  coef: 3 * C floats of scratch.
 * nblk >= 1; C % 4 == 0 and C <= 1024 (TDX_E_SHAPE otherwise).  A buffer of tdx_bn_relu_bwd_scratch_floats(rows, C)
 * floats holds the largest `partial` any producer writes (2048 blocks) plus coef. */
int tdx_bn_relu_bwd_from_partials(void* g, const void* y, int64_t rows, int C, const float* scale, const float* shift,
                                  const float* save_mean, const float* save_rstd, const float* gamma, float* dgamma,
                                  float* dbeta, float* dbias, const float* partial, int nblk, float* coef,
                                  int training, int io16, tdx_stream_t stream);

/* tdx_maxpool2_ceil_fwd / _bwd.  The maximum of bf16 values is a bf16 value and skip + g is rounded once.
 * Backward, partial == NULL: the plain kernel (bn_mean, bn_rstd ignored; *nblk = 0 when nblk is given).
 * partial != NULL: the PRODUCER form - besides g_in it writes, per workgroup, the BatchNorm-backward sums of the unit
 * whose pre-BN output is y (scale / shift its BN, bn_mean / bn_rstd its saved statistics) over the elements the
 * workgroup wrote: partial [*nblk][2][C], *nblk <= 2048 workgroups, formed from the fp32 gradient BEFORE it is rounded
 * for the store.  nblk, bn_mean, bn_rstd must then be given (TDX_E_BADARG).  It falls back to the plain kernel, and
 * says so with *nblk == 0 (partial untouched), when scale == NULL, when C is not a width of tdx_bn_relu_bwd, or when
 * bit 2 of the knob bnbwd_fused is off.  nblk points to HOST memory. */
int tdx_maxpool2_ceil_fwd_io(const void* y, const float* scale, const float* shift, void* out, int B, int H, int W,
                             int C, int io16, tdx_stream_t stream);
int tdx_maxpool2_ceil_bwd_io(const void* y, const float* scale, const float* shift, const void* g_out,
                             const void* skip_grad, void* g_in, int B, int H, int W, int C, const float* bn_mean,
                             const float* bn_rstd, float* partial, int* nblk, int io16, tdx_stream_t stream);

/* tdx_bilinear_ac_fwd / _bwd (addend stays fp32 (B, C)).  Backward, partial == NULL: the plain adjoint.
 * partial != NULL: the PRODUCER form of the row kernel: bn_y (B, Hi, Wi, C, storage type) is the pre-BN output of the
 * unit whose activation gradient g_in is, bn_scale .. bn_rstd its BN; partial [*nblk][2][C], *nblk = min(B Hi, 2048);
 * all of nblk, bn_y, bn_scale, bn_shift, bn_mean, bn_rstd must be given (TDX_E_BADARG).  Falls back to the plain
 * adjoint with *nblk == 0 when Hi or Wi > 64, when C is not a width of tdx_bn_relu_bwd, or when bit 1 of bnbwd_fused
 * is off.  The contributor limit and the slice rules of tdx_bilinear_ac_bwd hold in every form. */
int tdx_bilinear_ac_fwd_io(const void* in, const float* scale, const float* shift, const float* addend, void* out,
                           int B, int Hi, int Wi, int Ho, int Wo, int C, int out_cstride, int out_coff, int io16,
                           tdx_stream_t stream);
int tdx_bilinear_ac_bwd_io(const void* g_out, void* g_in, int B, int Hi, int Wi, int Ho, int Wo, int C, int g_cstride,
                           int g_coff, const void* bn_y, const float* bn_scale, const float* bn_shift,
                           const float* bn_mean, const float* bn_rstd, float* partial, int* nblk, int io16,
                           tdx_stream_t stream);
/* Both halves of a decoder input in one launch (inference): out (B, Ho, Wo, Ca + Cb) = resize(A) | resize(b + b_addend).
 * a (B, Ha, Wa, Ca), b (B, Hb, Wb, Cb) and out in the storage type; b_addend (B, Cb) fp32 or NULL; Cb == 0: no second
 * source (b ignored).  a_splits > 0: source A is a DEFERRED split-K convolution - a is ignored and every element of A is
 * relu((a_bias + partial_0 + ... + partial_{a_splits-1}) * a_scale + a_shift), summed in that order, from a_splits
 * fp32 slabs (B, Ha, Wa, Ca) that lie a_slab >= B Ha Wa Ca floats apart at a_partial (fp32 in both storage types);
 * a_bias may be NULL, a_scale and a_shift may not.  Ca % 4, Cb % 4: TDX_E_SHAPE. */
int tdx_bilinear_pair_fwd_io(const void* a, const float* a_partial, int a_splits, size_t a_slab, const float* a_bias,
                             const float* a_scale, const float* a_shift, int Ha, int Wa, int Ca, const void* b,
                             const float* b_addend, int Hb, int Wb, int Cb, void* out, int B, int Ho, int Wo, int io16,
                             tdx_stream_t stream);
/* out[b][c] = sum over the HW pixels of g (B, HW, C), fp32 (B, C): the gradient of a broadcast per-sample addend.
 * Widths as tdx_bn_relu_bwd (TDX_E_SHAPE otherwise); NULL or non-positive arguments: TDX_E_BADARG. */
int tdx_pixel_sum_io(const void* g, float* out, int B, int HW, int C, int io16, tdx_stream_t stream);

/* ---- whole network ------------------------------------------------------ */

/* Parameter slots, in reference state_dict order (diffusion.py:16-107).
 * Conv/BN units: U0..U12 = enc1.0 enc1.3 enc2.0 enc2.3 enc3.0 enc3.3 bottleneck
 *                          dec3.0 dec3.3 dec2.0 dec2.3 dec1.0 dec1.3 */
enum {
  TDX_P_TE0_W = 0, TDX_P_TE0_B, TDX_P_TE2_W, TDX_P_TE2_B,
  TDX_P_CLASS_EMB,            /* NULL for the unconditional model */
  TDX_P_INIT_W, TDX_P_INIT_B,
  TDX_P_UNIT0,                /* 13 units x (conv_w, conv_b, bn_w, bn_b) */
  TDX_P_FINAL_W = TDX_P_UNIT0 + 13 * 4, TDX_P_FINAL_B,
  TDX_P_TP1_W, TDX_P_TP1_B, TDX_P_TP2_W, TDX_P_TP2_B, TDX_P_TP3_W, TDX_P_TP3_B,
  TDX_P_COUNT
};
/* Buffer slots: 13 units x (running_mean, running_var, num_batches_tracked) */
#define TDX_B_COUNT (13 * 3)

#define TDX_MODE_TRAIN 0      /* batch statistics, activations saved for backward */
#define TDX_MODE_EVAL_GRAD 1  /* running statistics, activations saved for backward */
#define TDX_MODE_INFER 2      /* running statistics, fused conv+BN+ReLU, nothing saved */

/* ---- Linear layers and the MLP VAE (latent_diffusion.py / vae.py) -------
 * out[M,N] (row stride ldo) = act(x[M,K] (row stride ldx) . w[N,K]^T + bias);  nn.Linear layout.
 * act: 0 none, 1 ReLU, 2 sigmoid. */
int tdx_linear_fwd(const float* x, int ldx, const float* w, const float* bias, float* out, int ldo,
                   int M, int N, int K, int act, tdx_stream_t stream);
/* Backward of y = x w^T + b given gy[M,N]: dw[N,K] = gy^T x, db[N] = column sums of gy,
 * gx[M,K] = gy w.  Any of dw / db / gx may be NULL (skipped). */
int tdx_linear_bwd(const float* gy, int ldgy, const float* x, int ldx, const float* w, float* gx,
                   int ldgx, float* dw, float* db, int M, int N, int K, tdx_stream_t stream);
/* The same two with the arithmetic of the bf16 mode (precision = TDX_PREC_BF16: operands rounded to bf16, products on
 * v_mfma_f32_32x32x16_bf16, fp32 accumulation and epilogue; TDX_PREC_F32 = the entries above): the Linear layers of
 * the latent noise model (latent_diffusion.py:16-128) in BASELINE.json configs[3]. */
int tdx_linear_fwd_prec(const float* x, int ldx, const float* w, const float* bias, float* out, int ldo,
                        int M, int N, int K, int act, int precision, tdx_stream_t stream);
int tdx_linear_bwd_prec(const float* gy, int ldgy, const float* x, int ldx, const float* w, float* gx,
                        int ldgx, float* dw, float* db, int M, int N, int K, int precision, tdx_stream_t stream);
/* VAE.encode (vae.py:51-53): params = {fc1.w, fc1.b, fc21.w, fc21.b, fc22.w, fc22.b};
 * x (B,input_dim) -> mu, logvar (B,latent_dim).  workspace: tdx_vae_workspace_floats() floats. */
size_t tdx_vae_workspace_floats(int batch, int hidden_dim);
int tdx_vae_encode(const float* x, const void* const* params, float* mu, float* logvar,
                   float* workspace, int batch, int input_dim, int hidden_dim, int latent_dim,
                   tdx_stream_t stream);
/* VAE.reparameterize (vae.py:55-58) with caller-supplied eps: z = mu + eps * exp(0.5 logvar). */
int tdx_vae_reparameterize(const float* mu, const float* logvar, const float* eps, float* z,
                           int64_t n, tdx_stream_t stream);
/* VAE.decode (vae.py:60-62): params = {fc3.w, fc3.b, fc4.w, fc4.b}; z (B,latent_dim) ->
 * sigmoid output (B,input_dim). */
int tdx_vae_decode(const float* z, const void* const* params, float* out, float* workspace,
                   int batch, int input_dim, int hidden_dim, int latent_dim, tdx_stream_t stream);
/* VAE training (vae.py:70-76, 104-115).  Both loss sums are deterministic: a fixed element -> block map, double
 * partials, one finish launch (scratch: tdx_vae_loss_scratch_bytes() bytes, 8-byte aligned).
 * BCE from the decoder's LOGITS (fc4 without its sigmoid) against target = (x + 1) / 2, x in [-1, 1], sum-reduced:
 *   BCE_i = max(a, 0) - a target + log1p(exp(-|a|));  d_logits_i = gscale (sigmoid(a) - target);  recon_i = sigmoid(a)
 * d_logits and recon may be null.  Equals F.binary_cross_entropy(sigmoid(a), target, reduction="sum") wherever
 * torch's clamp log >= -100 does not bind, and stays exact where the fp32 sigmoid saturates. */
size_t tdx_vae_loss_scratch_bytes(void);
int tdx_vae_bce_logits_grad(const float* logits, const float* x, float* loss_out, float* d_logits, float* recon,
                            float gscale, int64_t n, void* scratch, tdx_stream_t stream);
/* kld_out = -0.5 sum (1 + logvar - mu^2 - exp(logvar)) (unweighted) and, when g_z (the decoder's gradient w.r.t. z =
 * mu + eps exp(0.5 logvar)) is given:  g_mu = g_z + kld_weight mu,
 * g_logvar = 0.5 g_z eps exp(0.5 logvar) + 0.5 kld_weight (exp(logvar) - 1).  g_z == NULL: the sum only. */
int tdx_vae_kld_reparam_bwd(const float* mu, const float* logvar, const float* eps, const float* g_z, float* kld_out,
                            float* g_mu, float* g_logvar, float kld_weight, int64_t n, void* scratch,
                            tdx_stream_t stream);
/* tdx_vae_reparameterize with eps drawn in the kernel: element i takes lane i % 4 of the Philox block
 * (counter i / 4, stream `offset`, key `seed`); the drawn eps is written to eps_out. */
int tdx_vae_reparameterize_philox(const float* mu, const float* logvar, float* z, float* eps_out, int64_t n,
                                  uint64_t seed, uint64_t offset, tdx_stream_t stream);
/* One call = VAE.forward + loss_function + loss.backward() (vae.py:111-113).  params / grads: {fc1.w, fc1.b, fc21.w,
 * fc21.b, fc22.w, fc22.b, fc3.w, fc3.b, fc4.w, fc4.b}; every gradient is written, not accumulated; grads == NULL:
 * forward and losses only.  eps (B,latent_dim), or NULL: drawn from Philox (seed, offset).  out3 (device) =
 * {BCE + kld_weight KLD, BCE, KLD}; the gradients are those of gscale * out3[0].  workspace:
 * tdx_vae_train_workspace_floats() floats, at least 8-byte aligned (it holds the loss scratch: double partials at an
 * offset that is a multiple of 256 bytes; TDX_E_BADARG otherwise - 16-byte alignment lets every kernel use its
 * vector loads).  No allocation, no host sync: capturable. */
size_t tdx_vae_train_workspace_floats(int batch, int input_dim, int hidden_dim, int latent_dim);
int tdx_vae_loss_grads(const float* x, const void* const* params, void* const* grads, const float* eps, uint64_t seed,
                       uint64_t offset, float kld_weight, float gscale, float* out3, float* workspace, int batch,
                       int input_dim, int hidden_dim, int latent_dim, tdx_stream_t stream);

/* ---- row / elementwise blocks of the "transformer" noise model (diffusion_transformer.py:16-107;
 * its attention runs on a length-1 sequence, i.e. it is out_proj(v_proj(x))) -------------------
 * LayerNorm over the last dimension N (N % 64 == 0, N <= 1024), eps as nn.LayerNorm (1e-5);
 * mean / rstd (M,) are saved for the backward. */
int tdx_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* out,
                      float* mean, float* rstd, int M, int N, float eps, tdx_stream_t stream);
/* gx (M,N), dgamma, dbeta (N,); gx or the pair dgamma/dbeta may be NULL. */
int tdx_layernorm_bwd(const float* gy, const float* x, const float* gamma, const float* mean,
                      const float* rstd, float* gx, float* dgamma, float* dbeta, int M, int N,
                      tdx_stream_t stream);
/* kind 0: SiLU, 1: GELU (erf form, the nn.GELU default). */
int tdx_act_fwd(const float* x, float* out, int64_t n, int kind, tdx_stream_t stream);
int tdx_act_bwd(const float* gy, const float* x, float* gx, int64_t n, int kind, tdx_stream_t stream);
/* out = x * keep / (1-p), one Philox Bernoulli draw per `group` consecutive elements (group 1 =
 * nn.Dropout; group = head_dim = dropout of a head's single attention weight).  The backward is
 * the same call on the gradient with the same (seed, offset). */
int tdx_dropout(const float* x, float* out, int64_t n, int group, float p, uint64_t seed,
                uint64_t offset, tdx_stream_t stream);
/* out[i] = a[i] + b[i % b_period] (b_period 0: same shape). */
int tdx_add(const float* a, const float* b, float* out, int64_t n, int64_t b_period, tdx_stream_t stream);
/* nn.Embedding forward (gather of rows) and backward (deterministic scatter-sum). */
int tdx_embedding_fwd(const float* weight, const int64_t* idx, float* out, int M, int N,
                      tdx_stream_t stream);
int tdx_embedding_bwd(const float* g, const int64_t* idx, float* dweight, int M, int N, int num,
                      tdx_stream_t stream);

/* ---- training of the "transformer" noise model: forward, loss and backward of
 * diffusion_transformer.py:82-107 + F.mse_loss in one call (transformer.hip).
 * Limits (those of the row kernels above): dim % 64 == 0, dim <= 1024, dim % num_heads == 0; anything else, or a
 * size <= 0, a dropout_p outside [0, 1) or an ln_eps <= 0: TDX_E_SHAPE, and the workspace size is 0. */
typedef struct tdx_transformer_shape {
  int batch, latent_dim, dim, num_heads, num_layers, num_classes;
  float dropout_p, ln_eps;
} tdx_transformer_shape;
size_t tdx_transformer_train_workspace_floats(const tdx_transformer_shape* shape);
/* params / grads: 12 + 12 * num_layers device pointers in the module's state_dict() order:
 *    0 pos_encoding (dim)                 1 time_embedding.0.weight (dim,1)    2 time_embedding.0.bias
 *    3 time_embedding.2.weight (dim,dim)  4 time_embedding.2.bias              5 class_embedding.weight (classes,dim)
 *    6 input_proj.weight (dim,latent)     7 input_proj.bias
 *    8 + 12 l + {0 attention.in_proj_weight (3 dim,dim), 1 attention.in_proj_bias (3 dim), 2 attention.out_proj.weight,
 *                3 attention.out_proj.bias, 4 norm1.weight, 5 norm1.bias, 6 ff.0.weight (4 dim,dim), 7 ff.0.bias,
 *                8 ff.2.weight (dim,4 dim), 9 ff.2.bias, 10 norm2.weight, 11 norm2.bias}     for block l
 *    8 + 12 L + {0 final_layer.0.weight, 1 final_layer.0.bias, 2 final_layer.1.weight (latent,dim), 3 final_layer.1.bias}
 * Every gradient is WRITTEN, not accumulated: the Q and K thirds of in_proj_weight / in_proj_bias (the softmax over
 * the single key of a length-1 sequence is constant) and the class_embedding rows of labels absent from y are exact
 * zeros.  grads == NULL: forward and loss only.
 * z_t (B,latent), t, y (B,) int64 (neither is range-checked: 0 <= y < num_classes is the caller's contract, as for
 * tdx_embedding_fwd), target (B,latent).  loss_out[0] = mean((eps_hat - target)^2), or with w_table (T,) the weighted
 * loss of tdx_mse_loss_grad_weighted (same passes, same fixed summation order); the gradients are those of
 * gscale * loss_out[0].  eps_hat_out (B,latent) may be NULL.
 * Dropout: train != 0 and dropout_p > 0 turn on the four sites of every block - the head weight (one draw per
 * (row, head)), the attention output, ff's own dropout, the block's dropout.  Site k = 1 .. 4 L in forward order draws
 * from Philox stream offset + k under key seed with tdx_dropout's element -> draw map (group = dim / num_heads at the
 * head site, 1 elsewhere), so offset = 0 gives the masks of the module's own train-mode forward under that seed.  The
 * backward regenerates the masks; none is stored.  rng_dev: NULL, or two device uint64 {seed, offset} that the kernels
 * read INSTEAD of the two by-value arguments (a captured step then draws fresh masks at every replay).
 * workspace: tdx_transformer_train_workspace_floats() floats, 16-byte aligned (TDX_E_BADARG otherwise).  One stream,
 * no allocation, no host synchronisation: capturable. */
int tdx_transformer_loss_grads(const tdx_transformer_shape* shape, const void* const* params, void* const* grads,
                               const float* z_t, const int64_t* t, const int64_t* y, const float* target,
                               const float* w_table, int train, uint64_t seed, uint64_t offset,
                               const uint64_t* rng_dev, float gscale, float* loss_out, float* eps_hat_out,
                               float* workspace, tdx_stream_t stream);

typedef struct tdx_unet tdx_unet;

/* num_classes == 0: unconditional (diffusion.py); > 0: class-conditional. */
int tdx_unet_create(tdx_unet** out, int max_batch, int num_classes);
/* kind TDX_UNET_MNIST: the 1x28x28 NoiseModel above (tdx_unet_create == kind 0);
 * kind TDX_UNET_LAION: NoiseModel of conditional_diffusion_laion.py:234-332 - 4x32x32 latents,
 *   widths 32..256, sinusoidal timestep embedding + Linear(768,768) MLP, additive 768-d text
 *   conditioning (num_classes must be 0).  Same parameter/buffer slot numbering; slot
 *   TDX_P_CLASS_EMB is unused, TDX_P_TE0_W is (768,768).
 * kind TDX_UNET_LATENT_MLP: NoiseModel of latent_diffusion.py:16-128 - MLP on (B,20) VAE latents,
 *   13 Linear+BatchNorm1d+ReLU units 512..64..512, class-conditional (num_classes > 0); the same
 *   slot numbering with Linear weights (out,in) in the conv-weight slots, initial_fc / final_fc in
 *   TDX_P_INIT_* / TDX_P_FINAL_*; x and out are (B,20). */
enum { TDX_UNET_MNIST = 0, TDX_UNET_LAION = 1, TDX_UNET_LATENT_MLP = 2 };
int tdx_unet_create_ex(tdx_unet** out, int max_batch, int kind, int num_classes);
/* The same with an explicit input resolution hw x hw (0 = the reference's: 28 for kind 0, 32 for
 * kind 1).  The LAION network is fully convolutional (conditional_diffusion_laion.py:304-332): any
 * multiple of 8 from 32 to 512 is accepted (64 = BASELINE.json configs[4]); the MNIST network resizes
 * to fixed sizes and takes 28 only.  TDX_E_SHAPE otherwise. */
int tdx_unet_create_hw(tdx_unet** out, int max_batch, int kind, int num_classes, int hw);
/* ... and an explicit width of the time embedding (the reference's NoiseModel(time_dim=...) constructor
 * argument: diffusion.py:16, conditional_diffusion.py:19, conditional_diffusion_laion.py:236): 0 = the
 * kind's default (256 / 768), else a multiple of 256 up to 1024 (the text embeddings of kind 1 have that
 * width too).  TDX_E_SHAPE otherwise. */
int tdx_unet_create_full(tdx_unet** out, int max_batch, int kind, int num_classes, int hw, int time_dim);
/* Synchronised BatchNorm for data-parallel training (an addition: the reference has no
 * distributed code).  With a callback installed, every train-mode BatchNorm of the plan takes its
 * statistics over the GLOBAL batch: the forward hands `buffer` = [sum x (C) | sum x^2 (C) | count]
 * (doubles, device memory owned by the caller, >= 2*1024 + 1 of them) to `fn`, which must all-reduce
 * (SUM) its first n elements across ranks on `stream` (ordered like a kernel: no host wait needed) and
 * return 0; the backward does the same with [sum gz | sum gz*xhat | rows].  dgamma / dbeta keep local
 * sums (the gradient all-reduce averages them).  An N-rank step then equals the single-process step on
 * the concatenated batch.  fn == NULL restores rank-local statistics (the default, DistributedDataParallel
 * semantics).  Not capturable in a graph. */
typedef int (*tdx_allreduce_fn)(void* user, double* device_buffer, int n, tdx_stream_t stream);
int tdx_unet_set_bn_sync(tdx_unet* u, tdx_allreduce_fn fn, void* user, double* buffer);

/* Stream schedule of the plan's training calls: -1 the network's default, 0 everything on the caller's
 * stream, 1 three streams (weight-gradient GEMMs and HBM-bound helpers beside the main chain, joined by
 * events before the call's last stage returns), 2 helpers only.  Capture of a whole training step into a
 * HIP graph must use 0: hipStreamEndCapture of a capture that forked into the library's low-priority
 * streams crashed inside the runtime on ROCm 7.2 (segmentation fault, no error code). */
int tdx_unet_set_streams(tdx_unet* u, int mode);

/* Arithmetic of the plan's 3x3 convolutions: TDX_PREC_F32 (default: exact fp32 MFMA) or TDX_PREC_BF16
 * (bf16 operands, fp32 accumulation and storage; see the bf16 section above).  Call before a forward;
 * a backward must run in the precision of its forward (TDX_E_STATE otherwise).  Not for kind 2. */
#define TDX_PREC_F32 0
#define TDX_PREC_BF16 1
int tdx_unet_set_precision(tdx_unet* u, int precision);
int tdx_unet_destroy(tdx_unet* u);
size_t tdx_unet_workspace_bytes(const tdx_unet* u, int batch, int mode);

/* eps_hat = NoiseModel.forward(x, t[, cond]) (diffusion.py:109-162,
 * conditional_diffusion.py:115-172, conditional_diffusion_laion.py:304-332).
 *   params: TDX_P_COUNT device pointers (reference layout); buffers: TDX_B_COUNT.
 *   kind MNIST: x (B,1,28,28) fp32; t (B,) int64; cond = y (B,) int64 labels or NULL; out (B,1,28,28).
 *   kind LAION: x (B,4,32,32) fp32; t (B,) int64; cond = text_embeds (B,768) fp32; out (B,4,32,32).
 *   kind LATENT_MLP: x (B,20) fp32; t (B,) int64; cond = y (B,) int64 labels; out (B,20).
 * In TRAIN mode the BN running buffers are updated in place. */
int tdx_unet_forward(tdx_unet* u, const void* const* params, void* const* buffers,
                     const float* x, const int64_t* t, const void* cond, float* out,
                     void* workspace, size_t workspace_bytes, int batch, int mode,
                     tdx_stream_t stream);

/* Gradients of every parameter for the most recent TRAIN/EVAL_GRAD forward on
 * this plan+workspace (autograd of diffusion.py:235 through the UNet).
 *   d_out (B,1,28,28); grads: TDX_P_COUNT device pointers, reference layout,
 *   each fully overwritten (not accumulated).  stage_lo/stage_hi select a
 *   contiguous range of backward stages [0, tdx_unet_backward_stages()) so the
 *   host can all-reduce finished buckets while later stages run. */
int tdx_unet_backward_stages(void);
int tdx_unet_backward(tdx_unet* u, const void* const* params, void* const* grads,
                      const float* d_out, void* workspace, size_t workspace_bytes,
                      int batch, int stage_lo, int stage_hi, tdx_stream_t stream);
/* A call that ends before the last stage does not make `stream` wait for the library's internal
 * streams (weight-gradient GEMMs, skip-branch resizes).  This orders `stream` - typically the
 * stream of the gradient all-reduce - after everything enqueued so far by tdx_unet_backward,
 * so that the gradients of the finished stages are final there.  (The caller orders `stream`
 * after its own compute stream as well.) */
int tdx_unet_backward_join(tdx_unet* u, tdx_stream_t stream);
/* The same in two halves, for a host that enqueues the collective of a bucket LATER than the bucket's stages (a wait
 * that sits unsatisfied in an otherwise idle hardware queue slows the dispatch of every other queue on gfx950: the step
 * measured 11.3 ms with the all-reduce waits enqueued at once, 10.0 ms without any): _mark records where the internal
 * streams are NOW (slot 0 .. tdx_unet_backward_stages()-1; a slot may be re-used by the next step), _wait_mark orders
 * `stream` after that point whenever it is called.  Replaces nothing in the reference (single-process training,
 * diffusion.py:228-236); this is the seam SURVEY.md 8(e)'s data-parallel step hangs its all-reduce on. */
int tdx_unet_backward_mark(tdx_unet* u, int slot);
int tdx_unet_backward_wait_mark(tdx_unet* u, int slot, tdx_stream_t stream);
/* Blocks the calling HOST thread until the internal streams have passed the mark (so that a wait enqueued afterwards
 * is satisfied on arrival). */
int tdx_unet_backward_sync_mark(tdx_unet* u, int slot);

/* d loss / d x on request: the NEXT tdx_unet_backward call that runs the last stage also writes the gradient
 * w.r.t. the network input x into g_x ((B, in_ch, H, W) fp32, the shape of x), on `stream`.  One-shot: the
 * request is cleared by that call (and by NULL).  The UNets only (the latent MLP: TDX_E_SHAPE). */
int tdx_unet_request_input_grad(tdx_unet* u, float* g_x);

/* get_timestep_embedding(timesteps, embedding_dim), conditional_diffusion_laion.py:222-232:
 * out[n][j] = sin(t_n f_j) for j < dim/2, cos(t_n f_{j-dim/2}) after, f_j = exp(-ln(1e4) j/(dim/2-1)),
 * one trailing zero column when dim is odd.  out (B, dim) fp32. */
int tdx_timestep_embedding(const int64_t* t, float* out, int B, int dim, tdx_stream_t stream);
/* floating-point timesteps (the reference converts with .float(): a fractional t keeps its fraction) */
int tdx_timestep_embedding_f32(const float* t, float* out, int B, int dim, tdx_stream_t stream);

/* The time / class path on its own (diffusion.py:21-25, 105-113, 130-132;
 * conditional_diffusion.py:31, 121-125): emb = W2 silu(W1 float(t) + b1) + b2 [+ E[y]], then the
 * three 1x1 projections.  params/grads: TDX_P_COUNT tables (only the TE, CLASS_EMB, TP slots are read /
 * written).  pre, emb (B,256); t1 (B,128), t2 (B,256), t3 (B,512); y NULL = unconditional.
 * bwd: g_t1..3 are d(loss)/d(t1..3) (already summed over pixels); scratch (3*256 + 1)*B floats. */
int tdx_time_mlp_fwd(const int64_t* t, const int64_t* y, const void* const* params, float* pre,
                     float* emb, float* t1, float* t2, float* t3, int batch, tdx_stream_t stream);
int tdx_time_mlp_bwd(const int64_t* t, const int64_t* y, const void* const* params,
                     void* const* grads, const float* pre, const float* emb, const float* g_t1,
                     const float* g_t2, const float* g_t3, float* scratch, int batch,
                     int num_classes, tdx_stream_t stream);

/* Additions within ABI 400: the same path at either kind and any time_dim (a constructor argument of every reference
 * model), as the networks run it.  kind 0 is the formula above at width time_dim; kind 1 is the LAION model's
 * (conditional_diffusion_laion.py:222-243, 297-308): emb = W2 silu(W1 sinusoid(t) + b1) + b2 + cond, projections of
 * 64 | 128 | 256 outputs.  time_dim: 1 ... 4096 for kind 0, 4 ... 4096 for kind 1 (the sinusoid divides by
 * time_dim / 2 - 1); TDX_E_SHAPE otherwise, nothing is written.  TDX_E_BADARG, nothing written: another kind, a null
 * pointer that is not marked optional, batch <= 0, parts that is 0 or holds a bit other than 1 | 2 | 4, k outside
 * 0 ... 2, labels with num_classes <= 0, or - at the widths 256, 512, 768, 1024, whose kernels read rows as float4 -
 * a weight matrix, pre, emb, the sinusoid or the text rows off a 16-byte boundary.
 *   fwd:  cond  kind 0: int64 labels (a negative label is the null condition) or NULL; kind 1: (B, time_dim) text rows.
 *         aux   written: kind 0 float(t), B floats; kind 1 the sinusoid, (B, time_dim).
 *         pre, emb (B, time_dim); t1, t2, t3 (B, 128 | 256 | 512) for kind 0, (B, 64 | 128 | 256) for kind 1.
 *   bwd:  parts 1 = the three projections (dW_k, db_k and g_emb), 2 = the middle (dE, dW2, db2, g_h; for kind 1 dW1 and
 *         db1 too), 4 = kind 0's first layer (dW1, db1); in one call or, in this order, in several.  y: kind 0's labels
 *         or NULL (optional; ignored for kind 1), aux / pre / emb as the forward left them.  g_t1..3 are read by part 1
 *         only.  scratch: 3 * B * time_dim floats, g_emb | h | g_h, which the caller may read afterwards: g_emb is
 *         d(loss)/d(emb), h = silu(pre), g_h = d(loss)/d(h) (kind 1: already multiplied by silu'(pre)).
 *   proj_bwd: part 1 of projection k alone: dW_k, db_k, and g_emb = (k > 0 ? g_emb : 0) + g_tk W_k in scratch[0 : B *
 *         time_dim].  Calling k = 0, 1, 2 and then bwd with parts 2 (| 4) equals bwd with all parts bit for bit. */
int tdx_time_path_fwd(int kind, int time_dim, const int64_t* t, const void* cond, const void* const* params,
                      float* aux, float* pre, float* emb, float* t1, float* t2, float* t3, int batch,
                      tdx_stream_t stream);
int tdx_time_path_bwd(int kind, int time_dim, int parts, const int64_t* y, const void* const* params,
                      void* const* grads, const float* aux, const float* pre, const float* emb, const float* g_t1,
                      const float* g_t2, const float* g_t3, float* scratch, int batch, int num_classes,
                      tdx_stream_t stream);
int tdx_time_path_proj_bwd(int kind, int time_dim, int k, const void* const* params, void* const* grads,
                           const float* emb, const float* g_tk, float* scratch, int batch, tdx_stream_t stream);

/* One reverse step x_t -> x_{t-1} of sample() (diffusion.py:259-274), capturable in a HIP graph:
 *   t = *counter; *counter = t - 1;  eps = eps_theta(x, t[, cond]) in TDX_MODE_INFER;
 *   x = c1[t] (x - c2[t] eps) + sigma[t] z   in place (z = 0 at t == 0).
 * z: recorded / host-drawn noise of x's shape, or NULL for in-kernel Philox noise keyed by
 * (philox_seed, t).  coef: (T,3) table as for tdx_p_sample_step.  t_idx (1 int32), t_vec (batch
 * int64) and eps (x's shape) are caller scratch.  x has n_elems = batch * per-sample elements. */
int tdx_unet_eval_step(tdx_unet* u, const void* const* params, void* const* buffers, float* x,
                       const void* cond, const float* z, const float* coef, int64_t* counter,
                       int32_t* t_idx, int64_t* t_vec, float* eps, int64_t n_elems,
                       void* workspace, size_t workspace_bytes, int batch, uint64_t philox_seed,
                       tdx_stream_t stream);

/* Sampling tables (optional, a speed-up only).  The time / class signal enters the network through projections
 * that are linear in the embedding, so inside one sample() call W_k MLP(t) + b_k is a table over t < T and
 * W_k c_b a table over the samples: built here once (for the plan's current INFER pack - call after
 * tdx_unet_pack - and for exactly this batch and this cond pointer, whose contents are read now), after which
 * tdx_unet_eval_step with the same batch / cond replaces its step counter, time MLP and projection launches by one
 * table look-up kernel (results equal up to fp32 reassociation of one sum).  May allocate: not inside a capture.
 * Any later tdx_unet_pack invalidates the tables (eval steps then take the direct path). */
int tdx_unet_prepare_sampling(tdx_unet* u, const void* const* params, const void* cond, int batch, int T,
                              tdx_stream_t stream);

/* Invalidate the tables of tdx_unet_prepare_sampling{,_sched}: later eval steps take the direct path, which computes
 * what an eager forward computes bit for bit, until tables are prepared again.  No launch, no allocation. */
int tdx_unet_drop_sampling_tables(tdx_unet* u);

/* The tables of a timestep schedule of S steps (tau: device int64 [S], see tdx_step_begin_sched): S table rows at
 * the timesteps tau[0..S) (rebuilt on every call); a scheduled eval step (tdx_unet_eval_step_update with tau) runs
 * eps_theta(x, tau[k]) and the update of coefficient row k; the counter holds k.  A table built
 * for one schedule (or for none) serves only eval steps with the same tau pointer and S: otherwise the step takes
 * the direct path. */
int tdx_unet_prepare_sampling_sched(tdx_unet* u, const void* const* params, const void* cond, int batch,
                                    const int64_t* tau, int S, tdx_stream_t stream);
/* The reverse step with any update of tdx_p_sample_update: tdx_unet_eval_step's arguments plus
 *   tau, S    the schedule (tau == NULL: the identity chain, S ignored; tau != NULL needs S > 0),
 *   form      TDX_STEP_EPS | TDX_STEP_X0 | TDX_STEP_MS, the kind of table coef is,
 *   guided, w classifier-free guidance: batch = 2n rows of x / cond / eps whose second half carries the null condition,
 *             n_elems = the FIRST half's elements, z = n rows or NULL (Philox); tables are prepared at batch 2n with
 *             the 2n-row cond; the UNets only (the latent MLP returns TDX_E_SHAPE), no half-batch forward,
 *   lo, hi    the clamp of X0 / MS,
 *   hist      MS: the history, n_elems floats kept by the caller from step to step (MS takes no z),
 *   known, mask   X0 / MS, both or neither: inpainting, n_elems floats each (a half-batch forward indexes them, like
 *             the history, by the element's place in the whole batch).
 * Sampling tables, the counter and the half-batch forward as in tdx_unet_eval_step.  The update runs in final_conv's
 * epilogue, or as tdx_p_sample_update when the epilogue is switched off (knob "sample_fuse") and for the latent MLP. */
int tdx_unet_eval_step_update(tdx_unet* u, const void* const* params, void* const* buffers, float* x,
                              const void* cond, const float* z, const float* coef, const int64_t* tau, int S,
                              int64_t* counter, int32_t* t_idx, int64_t* t_vec, float* eps, int64_t n_elems,
                              void* workspace, size_t workspace_bytes, int batch, uint64_t philox_seed, int form,
                              int guided, float w, float lo, float hi, float* hist, const float* known,
                              const float* mask, tdx_stream_t stream);
/* The reverse step with dynamic thresholding (tdx_x0_dyn_threshold): tdx_unet_eval_step_update's arguments plus rank,
 * frac and thr, (n, 2) floats kept by the caller (n = batch, guided: batch / 2; per = n_elems / n).  TDX_STEP_X0 and
 * TDX_STEP_MS only.  The bound of a sample is known only after the whole forward, so the update never runs in
 * final_conv's epilogue: the step is the head, the forward with the plain final_conv, the threshold launch and the
 * update as tdx_p_sample_update_dyn.  Sampling tables (the update advances the counter), the half-batch forward and
 * the latent MLP as in tdx_unet_eval_step_update.  TDX_E_BADARG: the cases of the three entries it is made of. */
int tdx_unet_eval_step_update_dyn(tdx_unet* u, const void* const* params, void* const* buffers, float* x,
                                  const void* cond, const float* z, const float* coef, const int64_t* tau, int S,
                                  int64_t* counter, int32_t* t_idx, int64_t* t_vec, float* eps, int64_t n_elems,
                                  void* workspace, size_t workspace_bytes, int batch, uint64_t philox_seed, int form,
                                  int guided, float w, float lo, float hi, float* hist, const float* known,
                                  const float* mask, int rank, float frac, float* thr, tdx_stream_t stream);

/* Testing aid: offset (in floats) and element count of a named intermediate inside the
 * workspace after a forward: "x0", "Y0".."Y12", "ss0".."ss12", "e1p", "cat1", "d1a", ... */
int tdx_unet_tensor(const tdx_unet* u, int batch, const char* name, size_t* offset_floats,
                    size_t* numel);

/* Pack conv weights + fold nothing: refreshes the plan's device-side packed
 * copies from `params`.  Called by forward automatically in TRAIN/EVAL_GRAD;
 * INFER reuses the packed copy until this is called again. */
int tdx_unet_pack(tdx_unet* u, const void* const* params, void* const* buffers,
                  tdx_stream_t stream);

/* Tuning knobs for experiments (process-global; the defaults are the product): "conv_tile" 0 auto |
 * 1 128x128 | 2 128x64 | 3 64x64; "wgrad_target" workgroups aimed at by the wgrad pixel split;
 * "splitk" 0 | 1; the rest are listed in INTEGRATION.md.  An unknown key returns TDX_E_BADARG. */
int tdx_tune_set(const char* key, int value);
/* Additions within ABI 400: the value a key holds now (as tdx_tune_set normalised it; TDX_E_BADARG for a null or
 * unknown key or a null `value`), and the index-th key of the table, NULL past its end. */
int tdx_tune_get(const char* key, int* value);
const char* tdx_tune_name(int index);

/* Diagnostics (tools/gpu_clock_probe.py, ...): device buffer of `bytes` bytes that the instrumented
 * kernels (knob "conv_stamp") record into; NULL disables it.
 * A path whose records would not fit in `bytes` does not stamp (never writes past the end). */
int tdx_diag_set_buffer(void* device_buffer, size_t bytes);
int tdx_diag_conv_occupancy(int tile);  /* resident workgroups per CU of the forward kernel of tile bm*1000+bn */

/* Additions within ABI 400: the pairwise kernels of the sample-quality metrics (metrics.hip; metrics.py builds the
 * Frechet distance, KID and precision / recall on them).  a (na, d) and b (nb, d) are row-major fp32 feature matrices,
 * every na, nb, d >= 1.  One kernel body computes
 *     g_ij = fma(a_i[d-1], b_j[d-1], ... fma(a_i[1], b_j[1], fma(a_i[0], b_j[0], 0)))
 * - the k-ordered fp32 fmaf chain of v_mfma_f32_32x32x2_f32, the same bits for every tiling and chunking - and four
 * epilogues take what a metric needs from it; only tdx_pair_gram writes the pair matrix.  The three reductions:
 *   - squared row norms, by the library from the same matrices: n_i = fma(x[d-1], x[d-1], ... fma(x[0], x[0], 0)), so
 *     the norm of a row equals its g with a bit-identical row;
 *   - d2_ij = max(0, (|a_i|^2 + |b_j|^2) - 2 g_ij): one fp32 add, the exact doubling, one fp32 subtraction, the floor;
 *   - the candidates b are cut into col_chunks chunks of whole 128-row tiles (0: the library chooses; more chunks than
 *     tiles are clipped), grid = ceil(na / 128) x chunks; each chunk writes a partial result per query to `scratch`
 *     and a second launch folds the chunks in ascending order.  No atomics: every output is bit-reproducible from
 *     launch to launch, and those of tdx_pair_kth_dist2 and tdx_pair_member are the same bits for every col_chunks
 *     (d2 does not depend on the chunking, and a k-smallest multiset or an OR does not depend on the order);
 *   - scratch: tdx_pair_scratch_bytes(na, nb, k, col_chunks) bytes (k: that of tdx_pair_kth_dist2, 0 for the other
 *     two; 0 is returned for na, nb <= 0, col_chunks < 0 or k > 8), 16-byte aligned.  TDX_E_WORKSPACE when smaller.
 * TDX_E_BADARG, before any launch and with nothing written: a null pointer, na, nb or d <= 0, col_chunks < 0, and the
 * cases named at each entry.  All launches go to `stream`; capturable. */
size_t tdx_pair_scratch_bytes(int na, int nb, int k, int col_chunks);
/* out (na, nb): out[i * nb + j] = g_ij. */
int tdx_pair_gram(const float* a, const float* b, int na, int nb, int d, float* out, tdx_stream_t stream);
/* out (na,): the k-th smallest d2_ij over j (ties count: the k-th element of the sorted row).  exclude_diag != 0
 * leaves out j == i by INDEX - an exact duplicate of row i elsewhere in b still counts, at distance 0.
 * 1 <= k <= 8 and nb >= k (nb >= k + 1 with exclude_diag); TDX_E_BADARG otherwise. */
int tdx_pair_kth_dist2(const float* a, const float* b, int na, int nb, int d, int k, int exclude_diag, int col_chunks,
                       float* out, void* scratch, size_t scratch_bytes, tdx_stream_t stream);
/* flag (na,) int32: flag[i] = 1 if d2_ij <= r2[j] for some j, else 0.  r2 (nb,) belongs to the CANDIDATES b: query a_i
 * is a member when it lies inside the ball of some b_j. */
int tdx_pair_member(const float* a, const float* b, const float* r2, int na, int nb, int d, int col_chunks,
                    int32_t* flag, void* scratch, size_t scratch_bytes, tdx_stream_t stream);
/* out (na,) fp64: out[i] = sum_j v_ij^3 with v_ij = fma((double)gamma, (double)g_ij, (double)coef0) and the cube
 * (v * v) * v, all in fp64 (exclude_diag != 0: j != i, by index).  Each lane half adds its candidates in ascending j
 * (of a 128-tile at offset 32 t: rows (r & 3) + 8 (r >> 2) + 4 h, h = 0 | 1 the half), the chunk's value is
 * half 0 + half 1, and the chunks are added in ascending order: reproducible, but a function of col_chunks in the
 * last fp64 bits.  gamma and coef0 finite (TDX_E_BADARG otherwise). */
int tdx_pair_poly_rowsum(const float* a, const float* b, int na, int nb, int d, float gamma, float coef0,
                         int exclude_diag, int col_chunks, double* out, void* scratch, size_t scratch_bytes,
                         tdx_stream_t stream);

/* Peak probes used by bench.py for measured roofline denominators. */
int tdx_probe_mfma_f32(float* out, int iters, int blocks, tdx_stream_t stream);
int tdx_probe_stream_copy(const float* src, float* dst, int64_t n, tdx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TDX_H */
