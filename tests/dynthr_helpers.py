"""Helpers of the dynamic-thresholding tests (tests/test_dynthr_host.py, tests/test_gpu_dynthr.py): the fp32 restatement
of the per-sample bound and of the thresholded updates (include/tdx.h: sort, then every product and sum a separate
torch op in the kernels' order), and the fp64 chains with the threshold (``torch.quantile`` in double).  Restated here,
not imported from the package."""
import math

import torch

from inpaint_helpers import _out64, blend32, cfg32, x0_rows64

F32 = torch.float32


def quantile_rank(q, per):
    """(rank, frac): pos = q (per - 1) in fp64, rank = floor(pos), frac = float32(pos - rank)."""
    pos = float(q) * (per - 1)
    rank = int(math.floor(pos))
    return rank, torch.tensor(pos - rank, dtype=torch.float64).to(F32).item()


def centre_half32(lo, hi):
    lo, hi = torch.tensor(lo, dtype=F32), torch.tensor(hi, dtype=F32)
    return (lo + hi) / 2, (hi - lo) / 2


def u32(x, out, row, lo, hi, w=None):
    """u = p*x + q*o - c per element, fp32; ``out`` holds both halves when ``w`` is given."""
    p, q = row[0], row[1]
    if w is not None:
        n = x.shape[0]
        out = cfg32(out[:n], out[n:], w)
    c, _ = centre_half32(lo, hi)
    return (p * x + q * out) - c


def threshold32(u, lo, hi, rank, frac):
    """(s, r, s_q), each of shape (n,): the sorted |u| of every sample, a[rank] + frac (a[min(rank+1, per-1)] - a[rank]),
    s = max(s_q, h), r = h / s."""
    _, h = centre_half32(lo, hi)
    a = u.abs().flatten(1).sort(dim=1).values
    per = a.shape[1]
    a0, a1 = a[:, rank], a[:, min(rank + 1, per - 1)]
    sq = a0 + torch.tensor(frac, dtype=F32) * (a1 - a0)
    s = torch.maximum(sq, h)
    return s, h / s, sq


def x0_thresholded32(u, s, r, lo, hi):
    """min(max(c + min(max(u, -s), s) * r, lo), hi) with the sample's (s, r) broadcast over its elements."""
    c, _ = centre_half32(lo, hi)
    shape = (-1,) + (1,) * (u.dim() - 1)
    s, r = s.reshape(shape), r.reshape(shape)
    v = torch.minimum(torch.maximum(u, -s), s)
    return torch.minimum(torch.maximum(c + v * r, torch.tensor(lo, dtype=F32)), torch.tensor(hi, dtype=F32))


def cpu_dyn_step(form, x, out, zh, row, lo, hi, k, rank, frac, w=None, known=None, mask=None):
    """The thresholded update of ``form`` "x0" (zh: the noise or None) or "ms" (zh: the history): returns
    (x', the value a multistep chain stores as history, (s, r))."""
    A, Bx, e = row[2], row[3], row[4]
    u = u32(x, out, row, lo, hi, w)
    s, r, _ = threshold32(u, lo, hi, rank, frac)
    x0 = x0_thresholded32(u, s, r, lo, hi)
    if known is not None:
        x0 = blend32(x0, known, mask)
    res = A * x0 + Bx * x
    if form == "x0":
        zz = zh if (zh is not None and k > 0) else torch.zeros_like(x)
        res = res + e * zz
    elif e.item() != 0.0:
        res = res + e * zh
    return res, x0, (s, r)


# ---------------------------------------------------------------- fp64
def threshold64(x0, lo, hi, q):
    """The thresholded x0 in double, and per sample the quantile s_q, the clamped and the unclamped element count."""
    c, h = (lo + hi) / 2, (hi - lo) / 2
    u = x0 - c
    sq = torch.quantile(u.abs().flatten(1), q, dim=1)
    s = torch.clamp(sq, min=h).reshape((-1,) + (1,) * (u.dim() - 1))
    x0c = torch.clamp(c + torch.clamp(u, -s, s) * (h / s), lo, hi)
    over = (u.abs() > s).flatten(1).sum(1)
    return x0c, sq, over, u[0].numel() - over


class Stats:
    """What the fp64 chain saw: (sample, step) pairs whose bound exceeded h / did not, and on the former the clamped
    and the unclamped elements."""

    def __init__(self, h):
        self.h, self.binding, self.static, self.clamped, self.free = h, 0, 0, 0, 0

    def add(self, sq, over, under):
        b = sq > self.h
        self.binding += int(b.sum())
        self.static += int((~b).sum())
        self.clamped += int(over[b].sum())
        self.free += int(under[b].sum())

    def ok(self):
        return self.binding > 0 and self.static > 0 and self.clamped > 0 and self.free > 0

    def __repr__(self):
        return (f"s > h on {self.binding} (sample, step) pairs, s == h on {self.static}; on the former {self.clamped} "
                f"elements clamped, {self.free} not")


@torch.no_grad()
def dyn_chain64(fwd, kind, fp, sched, x_T, y, lo, hi, q, prediction="eps", w=None, zs=None, known=None, mask=None):
    """The x0-form chain with the dynamic threshold (and the blend after it), fp64 state.  Returns (x, Stats)."""
    x = x_T.double()
    n = x.shape[0]
    taus = sched.timesteps.tolist()
    st = Stats((hi - lo) / 2)
    for k, (a, b, A, Bx, sg) in reversed(list(enumerate(x0_rows64(fp, sched)))):
        t = torch.full((n,), taus[k], dtype=torch.long)
        out = _out64(fwd, kind, x, t, y, w)
        x0 = (x - b * out) / a if prediction == "eps" else a * x - b * out
        x0c, sq, over, under = threshold64(x0, lo, hi, q)
        st.add(sq, over, under)
        if known is not None:
            x0c = (1 - mask.double()) * x0c + mask.double() * known.double()
        x = A * x0c + Bx * x
        if k > 0 and sg > 0:
            x = x + sg * zs[taus[k]].double()
    return x, st


@torch.no_grad()
def dyn_dpm_chain64(fwd, kind, fp, taus, x_T, y, lo, hi, q, prediction="eps", w=None, known=None, mask=None, order=2):
    """DPM-Solver++(2M) from its closed forms in Python doubles with the dynamic threshold (and the blend after it): D
    is built from the thresholded, blended predictions of this step and the step before.  Returns (x, Stats)."""
    acp = fp.alphas_cumprod.double()
    ab = [(math.sqrt(acp[t].item()), math.sqrt(1 - acp[t].item())) for t in taus]
    lam = [math.log(a / b) for a, b in ab]
    x = x_T.double()
    n, S = x.shape[0], len(taus)
    st = Stats((hi - lo) / 2)
    prev = None
    for k in range(S - 1, -1, -1):
        a, b = ab[k]
        t = torch.full((n,), taus[k], dtype=torch.long)
        out = _out64(fwd, kind, x, t, y, w)
        x0 = (x - b * out) / a if prediction == "eps" else a * x - b * out
        x0m, sq, over, under = threshold64(x0, lo, hi, q)
        st.add(sq, over, under)
        if known is not None:
            x0m = (1 - mask.double()) * x0m + mask.double() * known.double()
        if k == 0:
            return x0m, st
        a1, b1 = ab[k - 1]
        h = lam[k - 1] - lam[k]
        D = x0m
        if order == 2 and k < S - 1:
            r = (lam[k] - lam[k + 1]) / h
            D = (1 + 1 / (2 * r)) * x0m - (1 / (2 * r)) * prev
        x = (b1 / b) * x + a1 * -math.expm1(-h) * D
        prev = x0m
