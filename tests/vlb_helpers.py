"""The fp64 restatement of the variational bound (tests/test_vlb_host.py, tests/test_gpu_vlb.py): the element chain of
``tdx_vlb_terms`` in fp32 torch ops in the kernel's order, the decoder term in its tail form (fp64, and the fp32 CPU
restatement of the same form) and in the textbook form, the table formulas, the assembly of the result, and the input
generator the GPU tests and the host tests share.  Restated here from the formulas, not imported from the package.

Bounds.  SUM_TOL: a sum of non-negative fp32 terms in which one lane adds at most per / 64 terms serially is off by at
most (per / 64) 2^-24 relative, 256 * 2^-24 = 1.5e-5 at per <= 16384, rounded up to 2e-5.  The decoder sum may differ
from fp64 by DEC_K times the distance of the fp32 CPU restatement of the tail form from fp64 on the same inputs - taken
per element, sum_j |nll32_j - nll64_j|, so that errors which cancel in the restatement's own sum do not shrink the bound -
plus the summation bound, and never by more than DEC_CAP relative (the textbook form misses that by over 100x)."""
import math

import numpy as np
import torch

LN2 = math.log(2.0)
FLOOR = 1e-12
SUM_TOL = 2e-5
DEC_CAP = 1e-4
# Twice the ratio measured on an MI355X - 3.39, the worst of the 80 launches of test_kernel_against_the_restatement
# (DESIGN.md 3.18): the device erfc and log are a few ulp off the CPU's and the summation order differs.  A measured
# ratio above 8 would mean the form is wrong, not the bound.
DEC_K = 6.8
FLOOR_CAP = 0.05      # at most this share of a sample's elements may sit at the 1e-12 floor in the fp64 reference
INF = float("inf")


# ---------------------------------------------------------------- tables
def tables64(fp, prediction="eps", variance="beta"):
    """Python-side tables in fp64 from the fp32 ``betas`` / ``alphas_cumprod``: dict of (T,) tensors p, q, ex, eo, c0,
    bt (beta tilde), s2 (sigma^2), kc, g (both 0 in row 0) and the floats inv_sigma0, acp_last."""
    beta, acp = fp.betas.double(), fp.alphas_cumprod.double()
    T = beta.shape[0]
    prev = torch.cat([torch.ones(1, dtype=torch.float64), acp[:-1]])
    a, b = acp.sqrt(), (1 - acp).sqrt()
    p, q = (1 / a, -b / a) if prediction == "eps" else (a, -b)
    ex, eo = (torch.zeros_like(a), torch.ones_like(a)) if prediction == "eps" else (b, a)
    c0 = beta * prev.sqrt() / (1 - acp)
    c0[0] = 1.0
    bt = beta * (1 - prev) / (1 - acp)
    if variance == "beta":
        s2 = beta.clone()
    else:
        s2 = bt.clone()
        s2[0] = bt[1]
    kc, g = torch.zeros(T, dtype=torch.float64), torch.zeros(T, dtype=torch.float64)
    kc[1:] = 0.5 * (s2[1:].log() - bt[1:].log() + bt[1:] / s2[1:] - 1)
    g[1:] = c0[1:] ** 2 / (2 * s2[1:])
    return dict(p=p, q=q, ex=ex, eo=eo, c0=c0, bt=bt, s2=s2, kc=kc, g=g, inv_sigma0=1 / math.sqrt(s2[0].item()),
                acp_last=acp[-1].item())


def rows32(tab, bins=True):
    """The (T,5) fp32 rows (p, q, ex, eo, dec): dec = 1 / sigma_0 in row 0 under ``bins``, 0 elsewhere."""
    dec = torch.zeros_like(tab["p"])
    if bins:
        dec[0] = tab["inv_sigma0"]
    return torch.stack([tab["p"], tab["q"], tab["ex"], tab["eo"], dec], dim=1).float().contiguous()


# ---------------------------------------------------------------- the element chain, fp32 in the kernel's order
def chain32(x0, x_t, out, noise, rows, t, clip=(-INF, INF)):
    """(d, e) of ``tdx_vlb_terms``: every product and sum a separate fp32 torch op.  Inputs (B, per) fp32 on the CPU;
    ``rows`` (T,5) fp32; ``t`` (B,) int64.  e is None without noise."""
    r = rows[t]
    p, q, ex, eo = (r[:, i:i + 1] for i in range(4))
    u = p * x_t + q * out
    x0c = torch.minimum(torch.maximum(u, torch.tensor(clip[0])), torch.tensor(clip[1]))
    d = x0 - x0c
    e = None if noise is None else noise - (ex * x_t + eo * out)
    return d, e


# ---------------------------------------------------------------- the decoder term
def edges32(data_range, bins):
    """(half, lo_edge, hi_edge) as the C entry forms them in fp32."""
    lo, hi = np.float32(data_range[0]), np.float32(data_range[1])
    half = (hi - lo) / (np.float32(2.0) * np.float32(bins - 1))
    return float(half), float(lo + half), float(hi - half)


def dec_prob(x0, d, s, data_range=(-1.0, 1.0), bins=256, dtype=torch.float64, form="tail"):
    """The probability the decoder N(x0 - d, 1 / s^2) gives to the bin of x0, per element, before the floor.  ``x0`` and
    ``d`` are the fp32 values; ``s`` (B,1) or a float is the fp32 row's dec.  ``form="tail"``: every CDF a tail
    (erfc), the interior difference on the side where both tails are small, each operation rounded in ``dtype`` in the
    kernel's order.  ``form="textbook"``: (1 + erf) / 2."""
    half, lo_edge, hi_edge = edges32(data_range, bins)
    dd = d.to(dtype)
    s = torch.as_tensor(s, dtype=torch.float32).to(dtype)
    rs2 = torch.tensor(0.70710678118654752, dtype=dtype)
    h = torch.tensor(half, dtype=dtype)
    a = ((dd + h) * s) * rs2
    b = ((dd - h) * s) * rs2
    low, high = x0 < lo_edge, x0 > hi_edge
    if form == "tail":
        inner = torch.where(dd > 0, torch.erfc(b) - torch.erfc(a), torch.erfc(-a) - torch.erfc(-b))
        P = torch.where(low, torch.erfc(-a), torch.where(high, torch.erfc(b), inner))
        return torch.tensor(0.5, dtype=dtype) * P
    Pa, Pb = 0.5 * (1 + torch.erf(a)), 0.5 * (1 + torch.erf(b))
    return torch.where(low, Pa, torch.where(high, 1 - Pb, Pa - Pb))


def dec_nll(x0, d, s, data_range=(-1.0, 1.0), bins=256, dtype=torch.float64, form="tail"):
    """-log max(P, 1e-12) per element in ``dtype``, and the mask of the elements at the floor."""
    P = dec_prob(x0, d, s, data_range, bins, dtype, form)
    floor = torch.tensor(FLOOR, dtype=dtype)
    return -torch.log(torch.maximum(P, floor)), P <= floor


# ---------------------------------------------------------------- the three sums of one launch
def sums64(x0, x_t, out, noise, rows, t, clip=(-INF, INF), data_range=(-1.0, 1.0), bins=256):
    """What ``tdx_vlb_terms`` writes, from the fp32 (d, e) summed in fp64: ``(sums (B,3) fp64, info)``; info holds the
    per-sample distance of the fp32 CPU restatement of the decoder term from fp64 (``dist``, summed per element) and
    the share of the elements at the floor (``floored``)."""
    B = x0.shape[0]
    d, e = chain32(x0, x_t, out, noise, rows, t, clip)
    s = torch.zeros(B, 3, dtype=torch.float64)
    if e is not None:
        s[:, 0] = (e.double() ** 2).sum(1)
    s[:, 1] = (d.double() ** 2).sum(1)
    dec = rows[t][:, 4:5]
    dist, floored = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    if bins:
        on = dec[:, 0] > 0
        safe = torch.where(dec > 0, dec, torch.ones_like(dec))
        n64, fl = dec_nll(x0, d, safe, data_range, bins, torch.float64)
        n32, _ = dec_nll(x0, d, safe, data_range, bins, torch.float32)
        s[:, 2] = torch.where(on, n64.sum(1), torch.zeros(B, dtype=torch.float64))
        dist = torch.where(on, (n32.double() - n64).abs().sum(1), dist)
        floored = torch.where(on, fl.double().mean(1), floored)
    return s, dict(dist=dist, floored=floored, d=d, e=e)


# ---------------------------------------------------------------- the host formulas
def assemble64(tab, sums, t, D, bins):
    """(vb, mse, xstart_mse) from sums[..., 3] at the timesteps ``t`` (the shape of sums[..., 0])."""
    e2, d2, nll = sums[..., 0].double(), sums[..., 1].double(), sums[..., 2].double()
    kl = (D * tab["kc"][t] + tab["g"][t] * d2) / (D * LN2)
    if bins:
        first = nll / (D * LN2)
    else:
        s0 = tab["s2"][0].item()
        first = (0.5 * D * math.log(2 * math.pi * s0) + d2 / (2 * s0)) / (D * LN2)
    return torch.where(t == 0, first, kl), e2 / D, d2 / D


def prior64(tab, x0):
    """KL(N(sqrt(abar) x0, (1 - abar) I) || N(0, I)) per sample in bits per dimension, abar = abar_{T-1}."""
    D = x0[0].numel()
    v = 1 - tab["acp_last"]
    sq = (x0.double().reshape(x0.shape[0], -1) ** 2).sum(1)
    return 0.5 * (D * (-math.log(v) - 1 + v) + tab["acp_last"] * sq) / (D * LN2)


def loop64(fp, x0, noises, outs, prediction="eps", variance="beta", clip=(-INF, INF), bins=None,
           data_range=(-1.0, 1.0)):
    """The whole bound from recorded noise and the network outputs ``outs[t]`` the caller evaluated at
    ``x_t = q_sample(x0, t, noises[t])`` (fp32, the reference's expression): (total, prior, vb, mse, xstart_mse, info)
    with info the (B, T) distance / floor figures of the decoder column."""
    tab = tables64(fp, prediction, variance)
    rows = rows32(tab, bool(bins))
    B, T = x0.shape[0], fp.num_timesteps
    D = x0[0].numel()
    f0 = x0.reshape(B, D).float()
    sums = torch.zeros(B, T, 3, dtype=torch.float64)
    dist = torch.zeros(B, T, dtype=torch.float64)
    for t in range(T):
        tt = torch.full((B,), t, dtype=torch.int64)
        s, info = sums64(f0, x_t_of(fp, x0, t, noises[t]).reshape(B, D), outs[t].reshape(B, D).float(),
                         noises[t].reshape(B, D).float(), rows, tt, clip, data_range, bins)
        sums[:, t], dist[:, t] = s, info["dist"]
    steps = torch.arange(T).expand(B, T)
    vb, mse, xs = assemble64(tab, sums, steps, D, bins)
    prior = prior64(tab, x0)
    return prior + vb.sum(1), prior, vb, mse, xs, dict(dist=dist, sums=sums, tab=tab)


def x_t_of(fp, x0, t, noise):
    """q_sample in the reference's fp32 expression: sqrt(acp[t]) x0 + sqrt(1 - acp[t]) noise."""
    a = torch.sqrt(fp.alphas_cumprod)[t]
    b = torch.sqrt(1.0 - fp.alphas_cumprod)[t]
    return a * x0.float() + b * noise.float()


# ---------------------------------------------------------------- the inputs of the kernel tests
def gen_inputs(fp, per, t, rows, seed=0, floored=True):
    """Pixel-like inputs for samples at the timesteps ``t`` (a list): x0 on the 256-level grid of [-1, 1], the first
    eighth at -1 and the next eighth at +1; x_t = a x0 + b eps; model outputs such that x0c - x0 ~ N(0, (2 sigma_0)^2)
    with sigma_0 = 0.01, and - for per >= 20 with ``floored`` - six times that error on the last max(1, per // 50)
    elements, so that some elements sit at the 1e-12 floor.  Returns fp32 CPU tensors (x0, x_t, out, noise), (B, per)."""
    B = len(t)
    g = torch.Generator().manual_seed(1000 * per + 10 * B + seed)
    x0 = torch.randint(0, 256, (B, per), generator=g).float() * (2.0 / 255.0) - 1.0
    n8 = per // 8
    x0[:, :n8] = -1.0
    x0[:, n8:2 * n8] = 1.0
    eps = torch.randn(B, per, generator=g)
    err = 0.02 * torch.randn(B, per, generator=g)
    if floored and per >= 20:
        err[:, per - max(1, per // 50):] *= 6.0
    tt = torch.tensor(t)
    x_t = torch.stack([x_t_of(fp, x0[i], tt[i], eps[i]) for i in range(B)])
    return x0.contiguous(), x_t.contiguous(), solve_out(x0, err, x_t, rows, tt), eps.contiguous()


def solve_out(x0, err, x_t, rows, t):
    """The network output whose x0 prediction p x_t + q out is x0 + err (up to fp32 rounding), row t[b] for sample b."""
    r = rows[t].double()
    return ((x0.double() + err.double() - r[:, 0:1] * x_t.double()) / r[:, 1:2]).float().contiguous()
