"""Integer / fp64 numpy restatements for the training timestep sampler (csrc/timestep.hip): the Philox
block and the uniform the draw takes from it, the CDF of a probability table with its trailing-ones rule, the draw, and
improved-DDPM's ``LossSecondMomentResampler`` with its sequential update."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _u64(v):
    if isinstance(v, (int, np.integer)):
        return np.array(int(v) % (1 << 64), dtype=np.uint64)
    return np.asarray(v).astype(np.uint64)


def philox4x32_10(ctr_lo, ctr_hi, key):
    """``philox4x32_10`` of csrc/common.h: ten rounds over the 128-bit counter (ctr_lo, ctr_hi) under the 64-bit key,
    in uint64 arithmetic masked to 32 bits.  Arguments broadcast; returns (..., 4) uint32."""
    ctr_lo, ctr_hi, key = np.broadcast_arrays(_u64(ctr_lo), _u64(ctr_hi), _u64(key))
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    c0, c1, c2, c3 = ctr_lo & _M32, ctr_lo >> _S32, ctr_hi & _M32, ctr_hi >> _S32
    k0, k1 = key & _M32, key >> _S32
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2            # 32 x 32 bits: no overflow of the uint64
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> _S32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + W0) & _M32, (k1 + W1) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniform_of(seed, offset, b):
    """The draw's uniform of sample(s) ``b``: 24 bits of word 1 of the block (b, offset) under ``seed``, fp32, < 1."""
    v = philox4x32_10(b, offset, seed)[..., 1]
    return (v >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def cdf_of(probs, normalise=True):
    """fp32 CDF of a table of probabilities >= 0: the sequential fp64 prefix sum rounded once, and exactly 1 from the
    last positive entry on."""
    p = np.asarray(probs, dtype=np.float64)
    if normalise:
        p = p / p.sum()
    cdf = np.cumsum(p).astype(np.float32)
    cdf[np.flatnonzero(p > 0)[-1]:] = np.float32(1.0)
    return cdf


def draw(cdf, u):
    """t = #{k : cdf[k] <= u}."""
    return np.searchsorted(np.asarray(cdf, dtype=np.float32), np.asarray(u, dtype=np.float32), side="right").astype(np.int64)


def w_eff_of(probs, w_obj=None, importance=True):
    """fp32 loss weights of a normalised fp64 table: w_obj / (T p) under importance weights, 0 where p == 0."""
    p = np.asarray(probs, dtype=np.float64)
    T = p.shape[0]
    w = np.ones(T, dtype=np.float32) if w_obj is None else np.asarray(w_obj, dtype=np.float32)
    if not importance:
        return np.where(p > 0, w, np.float32(0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p > 0, w.astype(np.float64) / (T * p), 0.0).astype(np.float32)


def ulp_diff(a, b):
    """Largest distance in fp32 units in the last place between two arrays of finite non-negative floats."""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max())


class LossSecondMoment:
    """``LossSecondMomentResampler`` of improved-DDPM (Nichol & Dhariwal 2021, 3.3): the last H losses of every
    timestep, updated sample by sample in batch order; once every timestep has H, p_t ~ sqrt(mean_h L_t,h^2) mixed with
    ``uniform_prob`` of the uniform distribution; before, uniform."""

    def __init__(self, T, H=10, uniform_prob=0.001):
        self.T, self.H, self.uniform_prob = T, H, uniform_prob
        self.history = np.zeros((T, H), dtype=np.float32)
        self.counts = np.zeros(T, dtype=np.int32)

    def update(self, ts, losses):
        for t, loss in zip(np.asarray(ts).tolist(), np.asarray(losses, dtype=np.float32).tolist()):
            if self.counts[t] == self.H:        # shift out the oldest loss term
                self.history[t, :-1] = self.history[t, 1:]
                self.history[t, -1] = loss
            else:
                self.history[t, self.counts[t]] = loss
                self.counts[t] += 1

    def warmed_up(self):
        return bool((self.counts == self.H).all())

    def weights(self):
        """The fp64 probabilities (they sum to 1 up to rounding)."""
        if not self.warmed_up():
            return np.full(self.T, 1.0 / self.T)
        w = np.sqrt(np.mean(self.history.astype(np.float64) ** 2, axis=-1))
        w = w / w.sum()
        return w * (1.0 - self.uniform_prob) + self.uniform_prob / self.T

    def tables(self, w_obj=None):
        """(cdf, w_eff) in fp32 as the device writes them: before the warm-up ends fl((k + 1) / T) and w_obj exactly."""
        wo = np.ones(self.T, dtype=np.float32) if w_obj is None else np.asarray(w_obj, dtype=np.float32)
        if not self.warmed_up():
            return ((np.arange(1, self.T + 1, dtype=np.float64) / self.T).astype(np.float32)), wo
        p = self.weights()
        return cdf_of(p, normalise=False), w_eff_of(p, wo, True)

    def state(self):
        """(history oldest first, counts)."""
        return self.history.copy(), self.counts.copy()
