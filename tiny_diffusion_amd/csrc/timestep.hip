// Training timestep sampling on the device: which timestep each sample of a training step sees.
// Four tiny launches on the step's own stream, no atomics, no host synchronisation, capturable, bit-reproducible:
//   tdx_timestep_cdf             a (T,) probability table -> its CDF and the per-timestep loss weights
//   tdx_timestep_draw            one Philox uniform per sample, inverted through the CDF by binary search
//   tdx_mse_per_sample           the loss of every sample on its own (what the adaptive sampler learns from)
//   tdx_timestep_history_update  the loss-second-moment resampler of Nichol & Dhariwal 2021 (3.3): the last H losses
//                                of every timestep, p_t ~ sqrt(E[L_t^2]) mixed with a little uniform
#include "internal.h"

#define TS_BLOCK 256

// ---------------------------------------------------------------- block helpers
// Exclusive prefix of one double per thread over the workgroup, in thread order, and the total: thread 0 adds the
// TS_BLOCK partials one after the other, so excl[i + 1] == fl(excl[i] + v[i]) exactly - the CDF below is monotone
// because of it.  Ends with a barrier; `red` may be reused after the call.
__device__ static inline double block_excl_scan(double v, double* red, double* total) {
  __syncthreads();   // the previous use of red is over
  red[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double run = 0.0;
    for (int i = 0; i < TS_BLOCK; ++i) {
      const double x = red[i];
      red[i] = run;
      run += x;
    }
    red[TS_BLOCK] = run;
  }
  __syncthreads();
  const double e = red[threadIdx.x];
  *total = red[TS_BLOCK];
  return e;
}

// What both table builders end with.  raw(k) >= 0: the unnormalised weight of timestep k in double (evaluated three
// times per k: T is small and the alternative is a (T,) double scratch).  Thread i owns the contiguous timesteps
// [i * chunk, (i + 1) * chunk).
//   p_k   = raw_k / sum(raw),  then with mix > 0:  p_k (1 - mix) + mix / T            (double)
//   cdf_k = fl(sum_{j <= k} p_j), and exactly 1.0f from the last k with p_k > 0 on: a trailing zero-probability
//           timestep must not be drawn when the running sum rounds below 1 (the draw counts cdf_k <= u, u < 1)
//   w_eff_k = importance ? fl(w_obj_k / (T p_k)) : w_obj_k, 0 where p_k == 0          (w_obj == NULL: ones)
// A sum(raw) that is not > 0 (all-zero losses) gives the uniform table.
template <typename RAW>
__device__ static inline void write_cdf(RAW raw, double mix, const float* __restrict__ w_obj, int importance,
                                        float* __restrict__ cdf, float* __restrict__ w_eff, int T, double* red,
                                        int* last_sh) {
  const int chunk = (T + TS_BLOCK - 1) / TS_BLOCK;
  const int lo = min((int)threadIdx.x * chunk, T), hi = min(lo + chunk, T);
  double s = 0.0, raw_sum, p_sum;
  for (int k = lo; k < hi; ++k) s += raw(k);
  block_excl_scan(s, red, &raw_sum);
  const double total = raw_sum;
  const bool flat = !(total > 0.0) || !(total < INFINITY);
  const double inv_T = 1.0 / (double)T;
  auto prob = [&](int k) {
    const double p = flat ? inv_T : raw(k) / total;
    return mix > 0.0 ? p * (1.0 - mix) + mix * inv_T : p;
  };
  if (threadIdx.x == 0) *last_sh = 0;
  s = 0.0;
  int last = -1;
  for (int k = lo; k < hi; ++k) {
    const double p = prob(k);
    s += p;
    if (p > 0.0) last = k;
  }
  const double excl = block_excl_scan(s, red, &p_sum);   // (its first barrier orders the store to *last_sh)
  if (last >= 0) atomicMax(last_sh, last);               // LDS, integer: order-independent
  __syncthreads();
  last = *last_sh;
  double run = 0.0;
  for (int k = lo; k < hi; ++k) {
    const double p = prob(k);
    run += p;
    cdf[k] = k >= last ? 1.0f : (float)(excl + run);
    const float wo = w_obj ? w_obj[k] : 1.0f;
    w_eff[k] = !(p > 0.0) ? 0.0f : importance ? (float)((double)wo / ((double)T * p)) : wo;
  }
}

// ------------------------------------------------------------------ fixed table
__global__ void __launch_bounds__(TS_BLOCK)
timestep_cdf_kernel(const float* __restrict__ probs, const float* __restrict__ w_obj, int importance,
                    float* __restrict__ cdf, float* __restrict__ w_eff, int T) {
  __shared__ double red[TS_BLOCK + 1];
  __shared__ int last_sh;
  write_cdf([&](int k) { return (double)fmaxf(probs[k], 0.0f); }, 0.0, w_obj, importance, cdf, w_eff, T, red, &last_sh);
}

extern "C" int tdx_timestep_cdf(const float* probs, const float* w_obj, int importance, float* cdf, float* w_eff, int T,
                                tdx_stream_t stream) {
  if (!probs || !cdf || !w_eff || T <= 0) return TDX_E_BADARG;
  timestep_cdf_kernel<<<1, TS_BLOCK, 0, to_stream(stream)>>>(probs, w_obj, importance != 0, cdf, w_eff, T);
  TDX_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------- draw
// Sample b: u = 24 bits of word 1 of the Philox block (b, offset, seed) - word 0 is what tdx_cond_drop_* compares with
// p, and a step whose two seeds are equal must not drop exactly its low-u samples - and t = #{k : cdf[k] <= u}
// (np.searchsorted(cdf, u, side="right")).  cdf[T - 1] == 1 > u keeps t < T.
__global__ void __launch_bounds__(TS_BLOCK)
timestep_draw_kernel(const float* __restrict__ cdf, int T, int64_t* __restrict__ t_out, float* __restrict__ u_out, int B,
                     uint64_t seed, uint64_t offset, const uint64_t* __restrict__ rng_dev) {
  const int b = blockIdx.x * TS_BLOCK + threadIdx.x;
  if (b >= B) return;
  if (rng_dev) {
    seed = rng_dev[0];
    offset = rng_dev[1];
  }
  const Philox4 r = philox4x32_10((uint64_t)b, offset, seed);
  const float u = (float)(r.v[1] >> 8) * 5.9604644775390625e-8f;   // 24 bits: exact in fp32, never 1
  int lo = 0, hi = T;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] <= u) lo = mid + 1;
    else hi = mid;
  }
  t_out[b] = lo < T ? lo : T - 1;   // (a cdf that does not end in 1 is the caller's error: stay inside the tables)
  if (u_out) u_out[b] = u;
}

extern "C" int tdx_timestep_draw(const float* cdf, int T, int64_t* t_out, float* u_out, int B, uint64_t seed,
                                 uint64_t offset, const uint64_t* rng_dev, tdx_stream_t stream) {
  if (!cdf || !t_out || T <= 0 || B <= 0) return TDX_E_BADARG;
  timestep_draw_kernel<<<cdiv(B, TS_BLOCK), TS_BLOCK, 0, to_stream(stream)>>>(cdf, T, t_out, u_out, B, seed, offset,
                                                                               rng_dev);
  TDX_CHECK_LAUNCH();
  return 0;
}

// -------------------------------------------------------------- per-sample loss
// One workgroup per sample; the differences and their squares in double (exact products of fp32 differences), the
// wave reduction of the MSE kernels (elementwise.hip), the four wave partials in a fixed order, one rounding at the end.
template <bool VEC>
__global__ void __launch_bounds__(TS_BLOCK)
mse_per_sample_kernel(const float* __restrict__ a, const float* __restrict__ b, const int64_t* __restrict__ t,
                      const float* __restrict__ w_obj, float* __restrict__ loss_b, int per_sample) {
  __shared__ double red[TS_BLOCK / 64];
  const int s_idx = blockIdx.x;
  const float* ra = a + (int64_t)s_idx * per_sample;
  const float* rb = b + (int64_t)s_idx * per_sample;
  double s = 0.0;
  if (VEC) {
    const float4* a4 = reinterpret_cast<const float4*>(ra);
    const float4* b4 = reinterpret_cast<const float4*>(rb);
    for (int i = threadIdx.x; i < per_sample / 4; i += TS_BLOCK) {
      const float4 x = a4[i], y = b4[i];
      const double d0 = (double)x.x - (double)y.x, d1 = (double)x.y - (double)y.y;
      const double d2 = (double)x.z - (double)y.z, d3 = (double)x.w - (double)y.w;
      s += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
    }
  } else {
    for (int i = threadIdx.x; i < per_sample; i += TS_BLOCK) {
      const double d = (double)ra[i] - (double)rb[i];
      s += d * d;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    long long v = __double_as_longlong(s);
    int lo = __shfl_xor((int)(v & 0xffffffffll), o, 64);
    int hi = __shfl_xor((int)(v >> 32), o, 64);
    s += __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sum = ((red[0] + red[1]) + red[2]) + red[3];
    const double w = w_obj ? (double)w_obj[t[s_idx]] : 1.0;
    loss_b[s_idx] = (float)(w * sum / (double)per_sample);
  }
}

extern "C" int tdx_mse_per_sample(const float* a, const float* b, const int64_t* t, const float* w_obj, float* loss_b,
                                  int batch, int per_sample, tdx_stream_t stream) {
  if (!a || !b || !loss_b || (w_obj && !t) || batch <= 0 || per_sample <= 0) return TDX_E_BADARG;
  const bool vec = per_sample % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
  if (vec) mse_per_sample_kernel<true><<<batch, TS_BLOCK, 0, to_stream(stream)>>>(a, b, t, w_obj, loss_b, per_sample);
  else mse_per_sample_kernel<false><<<batch, TS_BLOCK, 0, to_stream(stream)>>>(a, b, t, w_obj, loss_b, per_sample);
  TDX_CHECK_LAUNCH();
  return 0;
}

// --------------------------------------------------------------- loss history
// One workgroup.  Phase 1 gives every row of `history` (oldest first) exactly what improved-DDPM's sequential loop
// over the batch gives it - a row below H appends, a full row drops its oldest entry and appends - duplicates of a
// timestep inside one batch included, without walking the batch serially: a row is a queue, so after the n samples of
// a batch that hit timestep k its content is the last H entries of (its c old entries, then the n losses IN BATCH
// ORDER).  Thread j takes sample j of a piece of TS_BLOCK samples and counts, over the piece's timesteps in LDS, the
// samples at its timestep (n) and those of them before it (r: its place in batch order).  With shift = max(0, c + n -
// H): the old entry h + shift moves to h (the first sample of each timestep does that, eight loads in flight), then -
// after a barrier - sample j's loss lands at c + r - shift, or is dropped when that is negative (more than H samples
// of one timestep in a batch).  No atomics: the places are distinct by construction.  Pieces run one after the other.
// A t outside [0, T) is skipped.  Phase 2: warmed up iff every counts[k] == H.  Phase 3: sqrt(mean_h history[k,h]^2)
// of every timestep once, into LDS (TS_MAX_T doubles), and the table (write_cdf) from there - or the uniform table
// exactly.
#define TS_MAX_T 4096
__global__ void __launch_bounds__(TS_BLOCK)
timestep_history_kernel(const int64_t* __restrict__ t, const float* __restrict__ loss_b, int B, float* history,
                        int32_t* counts, int H, float uniform_prob, const float* __restrict__ w_obj,
                        float* __restrict__ cdf, float* __restrict__ w_eff, int T) {
  __shared__ double red[TS_BLOCK + 1];
  __shared__ double wk[TS_MAX_T];
  __shared__ int last_sh;
  __shared__ int t_sh[TS_BLOCK];
  const int tid = threadIdx.x;
  for (int b0 = 0; b0 < B; b0 += TS_BLOCK) {
    const int nb = min(TS_BLOCK, B - b0);
    int k = -1;
    float loss = 0.f;
    if (tid < nb) {
      const int64_t tb = t[b0 + tid];
      if (tb >= 0 && tb < T) k = (int)tb;
      loss = loss_b[b0 + tid];
    }
    __syncthreads();   // the piece before this one is done with t_sh, and its rows and counts are written
    t_sh[tid] = k;
    __syncthreads();
    int n = 0, r = 0, c = 0, shift = 0;
    float* row = history;
    if (k >= 0) {
      for (int i = 0; i < nb; ++i) {
        const int same = t_sh[i] == k;
        n += same;
        r += same & (i < tid);
      }
      c = min(max(counts[k], 0), H);
      shift = max(0, c + n - H);
      row += (int64_t)k * H;
    }
    __syncthreads();   // every sample has read its row's count
    if (k >= 0 && r == 0) {
      const int keep = c - shift;   // old entries that survive (<= 0: none)
      for (int h0 = 0; shift > 0 && h0 < keep; h0 += 8) {   // moving down: a chunk's loads lie above every store so far
        float tmp[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) tmp[j] = h0 + j < keep ? row[h0 + j + shift] : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (h0 + j < keep) row[h0 + j] = tmp[j];
      }
      counts[k] = min(c + n, H);
    }
    __syncthreads();   // the old entries have moved
    const int at = c + r - shift;
    if (k >= 0 && at >= 0) row[at] = loss;
  }
  __syncthreads();   // rows and counts written above are read by other threads below
  int full = 1;
  for (int k = tid; k < T; k += TS_BLOCK) full &= counts[k] == H;
  if (!__syncthreads_and(full)) {
    for (int k = tid; k < T; k += TS_BLOCK) {
      cdf[k] = k == T - 1 ? 1.0f : (float)((double)(k + 1) / (double)T);
      w_eff[k] = w_obj ? w_obj[k] : 1.0f;
    }
    return;
  }
  for (int k = tid; k < T; k += TS_BLOCK) {
    const float* row = history + (int64_t)k * H;
    double m = 0.0;
    for (int h = 0; h < H; ++h) m += (double)row[h] * (double)row[h];
    wk[k] = sqrt(m / (double)H);
  }
  __syncthreads();
  write_cdf([&](int k) { return wk[k]; }, (double)uniform_prob, w_obj, 1, cdf, w_eff, T, red, &last_sh);
}

extern "C" int tdx_timestep_history_update(const int64_t* t, const float* loss_b, int B, float* history, int32_t* counts,
                                           int H, float uniform_prob, const float* w_obj, float* cdf, float* w_eff, int T,
                                           tdx_stream_t stream) {
  if (!history || !counts || !cdf || !w_eff || T <= 0 || H < 1 || B < 0 || (B > 0 && (!t || !loss_b)) ||
      !(uniform_prob >= 0.f && uniform_prob <= 1.f))
    return TDX_E_BADARG;
  if (T > TS_MAX_T) return TDX_E_SHAPE;
  timestep_history_kernel<<<1, TS_BLOCK, 0, to_stream(stream)>>>(t, loss_b, B, history, counts, H, uniform_prob, w_obj,
                                                                 cdf, w_eff, T);
  TDX_CHECK_LAUNCH();
  return 0;
}
