"""fp64 references, error bounds, input builders and a host model of the dispatch of csrc/bn.hip and csrc/spatial.hip
(DESIGN.md 3.14).  Plain module, no fixtures: tests/test_spatial_refs_host.py checks it against torch on the CPU,
tests/test_gpu_spatial_bn_dispatch.py holds the kernels against it.  Every reference is computed in fp64 from the
kernel's OWN fp32 operands (scale, shift, save_mean, save_rstd, gamma, the statistics partials, the addend), on
whichever device the operands live, in the kernels' channels-last layout.

Bounds.  u = 2^-24; an fp32 result that went through K roundings, each relative to a partial result no larger than the
magnitude-sum `mag` (the same reference evaluated on absolute values), is within LAM u sqrt(K) mag of the exact one
(the probabilistic model behind ELEM_DIRECT = 9 of tests/test_gpu_conv_launches.py).  K is read off the kernel and
stated where the bound is formed; nothing here was fitted to a kernel's output."""
import math

import numpy as np
import torch

from oracle import ref_cpu as R

U = 2.0 ** -24
LAM = 9.0
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
TDX_E_SHAPE = -2

# constants of csrc/spatial.hip and csrc/bn.hip that decide a branch (test_spatial_refs_host.py pins what follows
# from them, so a change there shows up as a failed expectation)
BIL_MAXC = 8          # candidate outputs per input index and axis in the resize adjoint
BIL_BATCH = 5         # the row kernel batches the loads of a column with at most this many contributors
BIL_ROW_MAXW = 64     # row kernel while Hi, Wi <= 64, generic kernel beyond
BIL_ROW_GRID = 16384  # rows per launch of the row kernel before its stride loop takes a second trip
EW_GRID_CAP = 4096    # workgroups of 256 threads: max-pool and resize
BN_APPLY_CAP = 8192   # bn_relu_apply_kernel
BN_BWD_APPLY_CAP = 4096
BN_BWD_WIDTHS = (4, 8, 16, 32, 64, 128, 256, 512, 1024)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def elem_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound; where the bound is 0 the element must be exact.  NaN counts as inf."""
    err = (got.double() - ref).abs()
    zero = bound == 0
    if bool((err[zero] > 0).any()) or bool(torch.isnan(err).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / bound[~zero]).max())


# ------------------------------------------------------------------------------------------------ BatchNorm2d
def bn_bwd_width_ok(C):
    return C > 0 and C % 4 == 0 and C <= 1024 and 256 % (C // 4) == 0


def bn_bwd_plan(rows, C):
    """Host model of bwd_rows_per_block (csrc/bn.hip): rows per block of the reduction pass, its regime, the number
    of blocks, and K = rpb / rgroups + rgroups, the fp32 additions behind one per-channel sum (a thread adds every
    rgroups-th row of its block, the block adds its rgroups threads; the blocks meet in double)."""
    assert bn_bwd_width_ok(C)
    rgroups = 256 // (C // 4)
    want = -(-rows // 2048)
    if want < 2 * rgroups:
        regime, rpb = "floor", 2 * rgroups
    elif want > 512:
        regime, rpb = "cap", 512
    else:
        regime, rpb = "rows/2048", want
    rpb = -(-rpb // rgroups) * rgroups
    return {"rgroups": rgroups, "rpb": rpb, "nblk": -(-rows // rpb), "regime": regime, "K": rpb // rgroups + rgroups,
            "apply_grid": -(-(rows * C // 4) // 256)}


def bn_finalize_operands(tiles, tile_rows, count, C, seed, device, big_mean):
    """Partials [tiles][2][C] as a convolution epilogue would leave them (tile sums n_t m_t with tile means scattered
    about the channel mean by std / sqrt(n_t), squared deviations (n_t - 1) std^2 (1 +- 10 %), 0 for a one-row tile),
    and gamma | beta | running_mean | running_var.  big_mean: |mean| / std ~ 100."""
    gen = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=gen).double()   # noqa: E731
    n_t = torch.full((tiles, 1), float(tile_rows), dtype=torch.float64, device=device)
    n_t[-1] = float(count - (tiles - 1) * tile_rows)
    mu = (30.0 if big_mean else 0.5) * rn(C)
    sd = 0.3 + torch.rand(C, device=device, generator=gen).double()
    m_t = mu + sd * rn(tiles, C) / n_t.sqrt()
    q_t = (n_t - 1) * sd.pow(2) * (1 + 0.1 * rn(tiles, C)).clamp_(min=0)
    stats = torch.stack([n_t * m_t, q_t], 1).float().contiguous()
    return {"stats": stats, "gamma": (1 + 0.1 * rn(C)).float(), "beta": (0.1 * rn(C)).float(),
            "running_mean": (0.1 * rn(C)).float(), "running_var": (1 + torch.rand(C, device=device, generator=gen))}


def bn_finalize_ref(stats, tile_rows, count, gamma, beta, rmean, rvar, training):
    """tdx_bn_finalize in fp64 from its fp32 operands -> {name: (reference, bound)} per channel.

    Train mode merges the tile partials (Chan et al.) about the global mean, m2 = sum Q_t + sum n_t (S_t/n_t - mean)^2:
    the same quantity as the kernel's sum Q_t + (sum S_t^2/n_t - S^2/N) without its cancellation.  The kernel merges in
    double, so what it adds to the bounds is the fp64 noise of that cancellation, 2^-50 (tiles + 2) sum S_t^2/n_t on m2
    (`noise`), and the float value of eps (relative u).  fp32 roundings K per output:
      save_mean 1 (the cast)            save_rstd 1 (the cast)           scale = gamma rstd: 2
      shift = beta - float(mean) scale: 5 (two casts, scale, product, difference), mag |beta| + |mean scale|
      running' = 0.9f old + 0.1f new: 6 (two constants, cast, two products, sum), mag 0.9 |old| + 0.1 |new|
    Eval mode is fp32 throughout: rstd = 1 / sqrtf(rvar + eps) 4 (eps, sum, root, quotient), scale 5, shift 7;
    save_mean is a copy."""
    g, b = gamma.double(), beta.double()
    out = {}
    if training:
        st = stats.double()
        tiles = st.shape[0]
        assert (tiles - 1) * tile_rows < count <= tiles * tile_rows
        n_t = torch.full((tiles, 1), float(tile_rows), dtype=torch.float64, device=st.device)
        n_t[-1] = float(count - (tiles - 1) * tile_rows)
        S_t, Q_t = st[:, 0], st[:, 1]
        mean = S_t.sum(0) / count
        m2 = Q_t.sum(0) + (n_t * (S_t / n_t - mean).pow(2)).sum(0)
        noise = 2.0 ** -50 * (tiles + 2) * (S_t.pow(2) / n_t).sum(0)
        var = m2 / count
        unbiased = m2 / (count - 1) if count > 1 else var
        rstd = 1.0 / torch.sqrt(var + BN_EPS)
        d_rstd = 0.5 * rstd * (noise / count + BN_EPS * U) / (var + BN_EPS)
        scale = g * rstd
        out["save_mean"] = (mean, LAM * U * mean.abs())
        out["save_rstd"] = (rstd, LAM * U * rstd + d_rstd)
        out["scale"] = (scale, LAM * U * math.sqrt(2) * scale.abs() + g.abs() * d_rstd)
        out["shift"] = (b - mean * scale, LAM * U * math.sqrt(5) * (b.abs() + (mean * scale).abs())
                        + (mean * g).abs() * d_rstd)
        if rmean is not None:
            rm, rv = rmean.double(), rvar.double()
            out["running_mean"] = ((1 - BN_MOMENTUM) * rm + BN_MOMENTUM * mean,
                                   LAM * U * math.sqrt(6) * ((1 - BN_MOMENTUM) * rm.abs() + BN_MOMENTUM * mean.abs()))
            out["running_var"] = ((1 - BN_MOMENTUM) * rv + BN_MOMENTUM * unbiased,
                                  LAM * U * math.sqrt(6) * ((1 - BN_MOMENTUM) * rv.abs() + BN_MOMENTUM * unbiased)
                                  + BN_MOMENTUM * noise / max(count - 1, 1))
    else:
        mean, rv = rmean.double(), rvar.double()
        rstd = 1.0 / torch.sqrt(rv + BN_EPS)
        scale = g * rstd
        out["save_mean"] = (mean, torch.zeros_like(mean))
        out["save_rstd"] = (rstd, LAM * U * math.sqrt(4) * rstd)
        out["scale"] = (scale, LAM * U * math.sqrt(5) * scale.abs())
        out["shift"] = (b - mean * scale, LAM * U * math.sqrt(7) * (b.abs() + (mean * scale).abs()))
    return out


def relu_margin(y, scale, shift):
    """fp64 pre-activation y scale + shift (channels last) and the threshold 8 u (|y scale| + |shift|) below which its
    sign is not decided by the operands: the kernels' single fma is within u |pre| of it."""
    ys = y.double() * scale.double()
    return ys + shift.double(), 8.0 * U * (ys.abs() + shift.double().abs())


def nudge_relu(y, scale, shift, bf16=False):
    """y with every element whose pre-activation is inside the threshold moved away from it (by 64 u of the
    magnitude, in the direction it already points): afterwards every element is decidable, none is left out.
    bf16: y is rounded to bf16 first and an offender moves to ANOTHER bf16 value - by the step above or by `trip`
    spacings of bf16 at |y| (2^-7 relative, 2^-133 at zero), whichever is larger - and is checked again after the
    rounding; the result is bf16-representable (returned as fp32)."""
    y = y.clone()
    if bf16:
        y = y.bfloat16().float()
    for trip in range(16 if bf16 else 4):
        pre, thr = relu_margin(y, scale, shift)
        bad = ~(pre.abs() > thr)
        if not bool(bad.any()):
            break
        sc = scale.double().expand_as(pre)
        step = (8.0 * thr + 1e-20) / sc.abs() * torch.where(pre >= 0, 1.0, -1.0) * torch.sign(sc)
        if bf16:
            spacing = torch.exp2(torch.floor(torch.log2(y.double().abs().clamp_min(2.0 ** -126))) - 7.0)
            step = torch.sign(step) * torch.maximum(step.abs(), (trip + 1) * spacing)
            y = torch.where(bad, (y.double() + step).float().bfloat16().float(), y)
        else:
            y = torch.where(bad, (y.double() + step).float(), y)
    assert relu_decidable(y, scale, shift)
    return y


def relu_decidable(y, scale, shift):
    pre, thr = relu_margin(y, scale, shift)
    return bool((pre.abs() > thr).all())


def bn_relu_fwd_ref(y, scale, shift):
    """relu(y scale + shift) and its bound 2 u (|y scale| + |shift|): one fma, one rounding."""
    pre, thr = relu_margin(y, scale, shift)
    return torch.relu(pre), thr / 4.0


def bn_operands(rows, C, seed, device, big_mean=False):
    """y, g (rows, C) and consistent per-channel scale | shift | mean | rstd | gamma | beta in fp32, the ReLU decidable
    everywhere.  big_mean: |mean| / std ~ 100, the data of test_bn_finalize_and_backward."""
    gen = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=gen)   # noqa: E731
    std = 0.3 + torch.rand(C, device=device, generator=gen)
    mean = (30.0 if big_mean else 0.5) * rn(C)
    gamma = 1 + 0.1 * rn(C)
    gamma = torch.where(gamma.abs() < 0.05, torch.full_like(gamma, 0.05), gamma)
    beta = 0.1 * rn(C)
    rstd = (1.0 / torch.sqrt(std.double() ** 2 + BN_EPS)).float()
    scale = gamma * rstd
    shift = beta - mean * scale
    y = rn(rows, C) * std + mean
    y = nudge_relu(y, scale, shift)
    return {"y": y, "g": rn(rows, C), "scale": scale, "shift": shift, "mean": mean, "rstd": rstd, "gamma": gamma,
            "beta": beta}


def bn_relu_bwd_ref(g, y, scale, shift, mean, rstd, gamma, training, K):
    """tdx_bn_relu_bwd in fp64 from its fp32 operands -> {name: (reference, bound)}; K = bn_bwd_plan(...)["K"].

      gz = g [y scale + shift > 0]    xhat = (y - mean) rstd    dbeta = sum gz    dgamma = sum gz xhat
      train: g' = gamma rstd (gz - dbeta / N - xhat dgamma / N), dbias = 0      eval: g' = gz scale, dbias = dbeta scale
    Roundings: dbeta K additions + the cast = K + 1, mag sum |gz|; dgamma K + 4 (xhat two, the product, the cast), mag
    sum |gz xhat|.  g' in train mode carries both sums' errors and nine roundings of its own (gamma rstd, the two casts
    of the means, xhat two, xhat m2, two differences, the product): K + 13 against
    mag = |gamma rstd| (|gz| + sum |gz| / N + |xhat| sum |gz xhat| / N).  Eval: one product; dbias K + 2."""
    g, y = g.double(), y.double()
    N = g.shape[0]
    pre = y * scale.double() + shift.double()
    gz = torch.where(pre > 0, g, torch.zeros_like(g))
    xh = (y - mean.double()) * rstd.double()
    s1, s2 = gz.sum(0), (gz * xh).sum(0)
    a1, a2 = gz.abs().sum(0), (gz * xh).abs().sum(0)
    out = {"dbeta": (s1, LAM * U * math.sqrt(K + 1) * a1), "dgamma": (s2, LAM * U * math.sqrt(K + 4) * a2)}
    if training:
        k1 = gamma.double() * rstd.double()
        out["g"] = (k1 * (gz - s1 / N - xh * s2 / N),
                    LAM * U * math.sqrt(K + 13) * k1.abs() * (gz.abs() + a1 / N + xh.abs() * a2 / N))
        out["dbias"] = (torch.zeros_like(s1), torch.zeros_like(s1))
    else:
        out["g"] = (gz * scale.double(), LAM * U * (gz * scale.double()).abs())
        out["dbias"] = (s1 * scale.double(), LAM * U * math.sqrt(K + 2) * a1 * scale.double().abs())
    return out


# ------------------------------------------------------------------------------------------------ max-pool
POOL_SCALES = (1.0, -1.0, 2.0, 0.5)
POOL_SHIFTS = (0.0, -0.125, 0.0, 0.125)


def first_max_index(win):
    """Index of the FIRST maximum of every window (..., 4) in scan order, without relying on argmax's tie rule."""
    eq = win == win.max(-1, keepdim=True).values
    first = eq & (eq.cumsum(-1) == 1)
    return first.to(torch.int64).argmax(-1, keepdim=True)


def maxpool_refs(y, scale, shift, g_out, skip):
    """tdx_maxpool2_ceil_fwd / _bwd in fp64, channels last: R.maxpool2_ceil over relu(y scale + shift) (scale None: the
    raw input), the gradient routed to the first maximum of each window by autograd, plus skip (None: nothing)."""
    a = nchw(y.double())
    if scale is not None:
        a = torch.relu(a * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    a.requires_grad_(True)
    idx = first_max_index(R.pool_windows(a.detach()))
    out = R.maxpool2_ceil(a, idx)
    (ga,) = torch.autograd.grad(out, a, nchw(g_out.double()))
    if skip is not None:
        ga = ga + nchw(skip.double())
    return nhwc(out.detach()), nhwc(ga)


def maxpool_window_stats(y, scale, shift):
    """Fractions that make first-maximum routing observable: windows of two or more valid positions whose maximum
    is positive and attained twice (`tie`), windows that are all zero after the ReLU (`zero`), windows whose maximum
    is negative (`neg`, raw input only); `multi` = number of windows with two or more valid positions."""
    a = nchw(y.double())
    if scale is not None:
        a = torch.relu(a * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    win = R.pool_windows(a)
    m = win.max(-1, keepdim=True).values
    multi = (win > float("-inf")).sum(-1) >= 2
    tie = ((win == m).sum(-1) >= 2) & (m.squeeze(-1) > 0)
    return {"multi": int(multi.sum()), "tie": float(tie[multi].double().mean()) if bool(multi.any()) else None,
            "zero": float((m == 0).double().mean()), "neg": float((m < 0).double().mean())}


def maxpool_inputs(B, H, W, C, seed, device, bn):
    """Dyadic operands: y in {-2 .. 2} / 8, g_out and skip in {-8 .. 8} / 8, scale in {1, -1, 2, 1/2} and shift in
    {0, -1/8, 0, 1/8} by channel, so y scale + shift, the ReLU, the maximum and skip + g are exact in fp32 and fp64
    alike and the comparison is bit for bit.  Ties and dead windows are planted on top of the random draw, and it is
    asserted that at least 5 % of the windows with two or more valid positions hold a tie between two positive values
    ((1, 1) has no such window) and, after BN+ReLU, at least 5 % of all windows are all zero."""
    gen = torch.Generator(device=device).manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, device=device, generator=gen).float() / 8.0   # noqa: E731
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    y, g_out, skip = ri(-2, 3, B, H, W, C), ri(-8, 9, B, Ho, Wo, C), ri(-8, 9, B, H, W, C)
    ch = torch.arange(C, device=device)
    scale = torch.tensor(POOL_SCALES, device=device)[ch % 4] if bn else None
    shift = torch.tensor(POOL_SHIFTS, device=device)[ch % 4] if bn else None
    # every fifth window gets the largest value there is (1/4 after BN: positive with every scale | shift pair) at
    # its first two positions, the next one the smallest at all four: <= 0 after BN (dead), -1/4 without (a negative tie)
    widx = torch.arange(B * Ho * Wo * C, device=device).view(B, Ho, Wo, C) % 5
    top = 0.25 * (torch.sign(scale) if bn else torch.ones(C, device=device))

    def put(dh, dw, mask, val):
        v = y[:, dh::2, dw::2, :]
        v.copy_(torch.where(mask[:, :v.shape[1], :v.shape[2], :], val.expand_as(v), v))

    put(0, 0, widx == 0, top)
    put(*((0, 1) if W > 1 else (1, 0)), widx == 0, top)
    for dh in (0, 1):
        for dw in (0, 1):
            put(dh, dw, widx == 1, -top)
    st =maxpool_window_stats(y[:4096], scale, shift)   # (of the first 4096 samples: enough to count)
    if st["multi"]:
        assert st["tie"] >= 0.05, st
    if bn:
        assert st["zero"] >= 0.05, st
    else:
        assert st["neg"] > 0, st
    return y, scale, shift, g_out, skip


# ------------------------------------------------------------------------------------------------ bilinear resize
def ac_src(n_in, n_out, device=None):
    """Exact align_corners source coordinate of every output index, fp64."""
    dst = torch.arange(n_out, dtype=torch.float64, device=device)
    return dst * (n_in - 1) / (n_out - 1) if n_out > 1 else dst * 0.0


def ac_matrix(n_in, n_out, device=None):
    """(n_out, n_in) weights of one axis of the align_corners resize from the exact coordinate."""
    src = ac_src(n_in, n_out, device)
    i0 = src.floor().to(torch.int64).clamp_(max=n_in - 1)
    i1 = (i0 + 1).clamp_(max=n_in - 1)
    l1 = src - i0.to(torch.float64)
    Wm = torch.zeros(n_out, n_in, dtype=torch.float64, device=device)
    rows = torch.arange(n_out, device=device)
    Wm.index_put_((rows, i0), 1.0 - l1, accumulate=True)
    Wm.index_put_((rows, i1), l1, accumulate=True)
    return Wm


def ac_coord_delta(n_in, n_out):
    """|fp32 coordinate - exact coordinate| <= (2 u + u^2) (n_in - 1): the scale is one rounded quotient, the
    coordinate one rounded product, and no coordinate exceeds n_in - 1.  Exactly 0 on a degenerate axis (scale 0)."""
    return (2 * U + U * U) * (n_in - 1) if n_in > 1 and n_out > 1 else 0.0


def ac_coord_matrix(n_in, n_out, device=None):
    """(n_out, n_in) bound on what the fp32 coordinate moves each weight by: delta wherever the input index lies
    within 1 + delta of the exact coordinate (the two taps, and the neighbour a coordinate on a grid point may flip to),
    0 elsewhere."""
    d = ac_coord_delta(n_in, n_out)
    src = ac_src(n_in, n_out, device).view(-1, 1)
    idx = torch.arange(n_in, dtype=torch.float64, device=device).view(1, -1)
    return ((src - idx).abs() < 1 + d).to(torch.float64) * d


def resize_apply(Mh, Mw, a):
    """out[b, o, p, c] = sum_{h, w} Mh[o, h] Mw[p, w] a[b, h, w, c]."""
    return torch.einsum("oh,bhwc,pw->bopc", Mh, a, Mw)


def resize_apply_t(Mh, Mw, g):
    """g_in = Mh^T g Mw per (b, c): the transpose of resize_apply."""
    return torch.einsum("oh,bopc,pw->bhwc", Mh, g, Mw)


def resize_fwd_exact(a, Ho, Wo):
    """The fp64 forward operator from exact coordinates (the reference pair of the adjoint identity)."""
    a = a.double()
    return resize_apply(ac_matrix(a.shape[1], Ho, a.device), ac_matrix(a.shape[2], Wo, a.device), a)


def resize_coord_term_fwd(a_abs, Ho, Wo):
    """Bound on |resize with fp32 coordinates - resize with exact ones| of an input of magnitude a_abs."""
    Hi, Wi, dev = a_abs.shape[1], a_abs.shape[2], a_abs.device
    Mh, Mw, Dh, Dw = ac_matrix(Hi, Ho, dev), ac_matrix(Wi, Wo, dev), ac_coord_matrix(Hi, Ho, dev), ac_coord_matrix(Wi, Wo, dev)
    return resize_apply(Dh, Mw, a_abs) + resize_apply(Mh, Dw, a_abs) + resize_apply(Dh, Dw, a_abs)


def resize_input_ref(y, scale, shift, addend):
    """What the resize interpolates, relu(y scale + shift) + addend[b][c] in fp64, and its magnitude with the loader's
    roundings: |y scale| + |shift| where the ReLU is open (one fma) plus |addend| (one sum)."""
    a = y.double()
    mag = a.abs()
    if scale is not None:
        pre, thr = relu_margin(y, scale, shift)
        a = torch.relu(pre)
        mag = torch.where(pre > 0, thr / (8.0 * U), torch.zeros_like(pre))
    if addend is not None:
        ad = addend.double().view(addend.shape[0], 1, 1, -1)
        a, mag = a + ad, mag + ad.abs()
    return a, mag


def resize_fwd_ref(y, scale, shift, addend, Ho, Wo):
    """tdx_bilinear_ac_fwd in fp64, channels last -> (reference, bound).  The reference is R.bilinear_ac, whose fp32
    coordinates are the kernel's (ATen's), over resize_input_ref; K = 4 fp32 roundings on the longest path of an output
    (product, sum along W; product, sum along H; the oracle's weights, 1 - lambda included, are the kernel's bit for bit)
    + 1 with BN on load + 1 with an addend."""
    a, mag = resize_input_ref(y, scale, shift, addend)
    K = 4 + (scale is not None) + (addend is not None)
    with torch.device(a.device):
        ref = nhwc(R.bilinear_ac(nchw(a), (Ho, Wo)))
        m = nhwc(R.bilinear_ac(nchw(mag), (Ho, Wo)))
    return ref, LAM * U * math.sqrt(K) * m


def resize_adj_ref(g, Hi, Wi, with_coord=True):
    """tdx_bilinear_ac_bwd in fp64 -> (reference, bound, rounding part of the bound): g_in = Wh^T g Ww with the exact
    operator.  An input element sums hn wn products (its contributors per axis) by fma: K = hn wn + 3 (1 - lambda, a
    clamped tap's lambda0 + lambda1, the product of the two axis weights), mag = Wh^T |g| Ww.  The fp32 coordinate
    adds Dh^T |g| Ww + Wh^T |g| Dw + Dh^T |g| Dw (ac_coord_matrix)."""
    g = g.double()
    Ho, Wo, dev = g.shape[1], g.shape[2], g.device
    Mh, Mw = ac_matrix(Hi, Ho, dev), ac_matrix(Wi, Wo, dev)
    ref = resize_apply_t(Mh, Mw, g)
    hn = (Mh != 0).sum(0).clamp_(min=1).double()
    wn = (Mw != 0).sum(0).clamp_(min=1).double()
    K = (hn.view(-1, 1) * wn.view(1, -1) + 3.0).view(1, Hi, Wi, 1)
    rounding = LAM * U * torch.sqrt(K) * resize_apply_t(Mh, Mw, g.abs())
    bound = rounding
    if with_coord:
        Dh, Dw = ac_coord_matrix(Hi, Ho, dev), ac_coord_matrix(Wi, Wo, dev)
        ga = g.abs()
        bound = rounding + resize_apply_t(Dh, Mw, ga) + resize_apply_t(Mh, Dw, ga) + resize_apply_t(Dh, Dw, ga)
    return ref, bound, rounding


def resize_inputs(B, Hi, Wi, Ho, Wo, C, seed, device):
    """y, scale (|scale| >= 1/2), shift, addend, g_out in fp32; the ReLU of y scale + shift decidable everywhere."""
    gen = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=gen)   # noqa: E731
    scale = (0.5 + torch.rand(C, device=device, generator=gen)) * torch.where(rn(C) < 0, -1.0, 1.0)
    shift = 0.2 * rn(C)
    y = nudge_relu(rn(B, Hi, Wi, C), scale, shift)
    return {"y": y, "scale": scale, "shift": shift, "addend": rn(B, C), "g": rn(B, Ho, Wo, C)}


# ---- host model of the adjoint's dispatch, fp32 like the device code
_f32 = np.float32


def ac_scale32(n_in, n_out):
    return _f32(n_in - 1) / _f32(n_out - 1) if n_out > 1 else _f32(0)


def axis_taps32(n_in, n_out):
    """(i0, i1, l0, l1) of every output index with ATen's fp32 arithmetic (axis_tap in csrc/spatial.hip)."""
    s = ac_scale32(n_in, n_out)
    taps = []
    for o in range(n_out):
        src = _f32(s * _f32(o))
        i0 = min(int(src), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = _f32(src - _f32(i0))
        taps.append((i0, i1, _f32(_f32(1) - l1), l1))
    return taps


def axis_spans32(n_in, n_out):
    """Per input index: the span (last - first + 1) of the outputs that reach it with a non-zero weight, 0 if none -
    the `wn` / `hn` of the row kernel."""
    taps = axis_taps32(n_in, n_out)
    spans = []
    for i in range(n_in):
        nz = [o for o, (i0, i1, l0, l1) in enumerate(taps)
              if _f32((l0 if i0 == i else _f32(0)) + (l1 if i1 == i else _f32(0))) != 0]
        spans.append(nz[-1] - nz[0] + 1 if nz else 0)
    return spans


def adjoint_axis_ok(n_in, n_out):
    """include/tdx.h: tdx_bilinear_ac_bwd covers an axis when, for every input index i, the candidate outputs
    [floor((i - 1) / s) - 1, ceil((i + 1) / s) + 1] (s = (n_in - 1) / (n_out - 1) in fp32, clipped to the output) are at
    most 8; with s = 0 (n_in = 1 or n_out = 1), when n_out <= 8.  So no input has more than 8 contributing outputs."""
    s = ac_scale32(n_in, n_out)
    if not s > 0:
        return n_out <= BIL_MAXC
    for i in range(n_in):
        lo = max(0, int(math.floor(_f32(_f32(i - 1) / s))) - 1)
        hi = min(n_out - 1, int(math.ceil(_f32(_f32(i + 1) / s))) + 1)
        if hi - lo + 1 > BIL_MAXC:
            return False
    return True


def adjoint_branch(Hi, Wi, Ho, Wo):
    """Which path tdx_bilinear_ac_bwd takes: "rejected" (TDX_E_SHAPE), "generic" (Hi or Wi > 64), or the row kernel's
    "rows-batched" (every column has wn <= BIL_BATCH) / "rows-loop" (some column has more)."""
    if not (adjoint_axis_ok(Hi, Ho) and adjoint_axis_ok(Wi, Wo)):
        return "rejected"
    if Hi > BIL_ROW_MAXW or Wi > BIL_ROW_MAXW:
        return "generic"
    return "rows-loop" if max(axis_spans32(Wi, Wo)) > BIL_BATCH else "rows-batched"


# ------------------------------------------------------------------------------------------------ the cases of part 3
def case_seed(*xs):
    """One seed per case, the same in the host test of the builders and in the GPU test."""
    s = 17
    for x in xs:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return s


def bn_floor_rows(C):
    """rows = 1, rpb - 1, rpb, rpb + 1 at the floor rpb = 2 rgroups of width C: ragged and full last blocks."""
    rpb = 2 * (256 // (C // 4))
    return sorted({1, rpb - 1, rpb, rpb + 1})


# (tiles, tile_rows, count, C, big_mean)
FINALIZE_CASES = [
    (1, 2, 2, 4, False),                       # count = 2, one tile, one block
    (2, 1, 2, 4, False),                       # count = 2 as two one-row tiles
    (2, 500, 501, 1024, False),                # ragged last tile of one row
    (3, 500, 1176, 128, True),                 # the data of test_bn_finalize_and_backward (|mean| / std ~ 100)
    (256, 64, 256 * 64, 128, False),           # exactly one trip of the tile loop
    (257, 64, 256 * 64 + 1, 128, True),        # a second trip of one thread, ragged last tile of one row
    (600, 49, 600 * 49 - 20, 1024, False),     # up to three trips
    (257, 1 << 20, (256 << 20) + 12345, 4, True),   # a count beyond 2^24
]
BN_BWD_OTHER = [   # (C, rows, regime, what it is there for)
    (1024, 4100, "rows/2048", "rpb 3, rgroups 1"),
    (128, 40000, "rows/2048", "rpb 20 -> 24"),
    (4, 1048577 + 5, "cap", "rpb 512 at the cap"),
    (128, 4800, "floor", "300 blocks: the finalize loop's second trip"),
    (8, 524289, "rows/2048", "rpb 257 -> 384; 4097 apply workgroups"),
]
APPLY_CASES = [(1, 4), (1048580, 8)]   # (rows, C); the second has rows C / 4 = 2 097 160 > 8192 x 256
POOL_SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (5, 4), (7, 7), (28, 14), (13, 32)]
POOL_BIG = (262200, 3, 3, 4)           # B, H, W, C: 1 048 800 window quads > 4096 x 256
# (Hi, Wi, Ho, Wo) -> the adjoint's branch (test_spatial_refs_host.py checks each against adjoint_branch)
RESIZE_CASES = {
    (4, 7, 8, 8): "rows-batched",
    (7, 4, 8, 16): "rejected",        # 4 -> 16 has nine contributors per inner column
    (14, 28, 16, 32): "rows-batched",
    (32, 16, 28, 28): "rows-batched",
    (5, 5, 5, 5): "rows-batched",
    (3, 2, 7, 6): "rows-batched",     # wn = 5 = BIL_BATCH exactly, hn = 5
    (2, 3, 7, 8): "rows-loop",        # hn = 6, wn = 6
    (2, 3, 7, 5): "rows-batched",     # hn = 6 alone (added: the list above has no pair with only the H axis past 5)
    (1, 2, 8, 7): "rows-loop",        # wn = 6, hn = 8
    (1, 1, 1, 1): "rows-batched",
    (5, 8, 1, 1): "rows-batched",     # n_out = 1: every input but the first has no contributor
    (64, 2, 2, 8): "rows-loop",       # 64 -> 2: 62 empty rows; wn = 7
    (65, 3, 66, 6): "generic",
    (3, 66, 6, 67): "generic",
    # added: the two above never put a weight on the generic kernel's last candidates (a, d = 6, 7 of BIL_MAXC = 8)
    (1, 66, 8, 67): "generic",        # hn = 8: all eight candidates of the H axis contribute
    (66, 2, 67, 8): "generic",        # wn = 7: candidates 1 ... 7 of the W axis contribute to the second column
}
RESIZE_REJECTED_AXES = [(2, 9), (1, 9), (3, 9), (4, 14)]
RESIZE_FWD_BIG = (19500, 3, 5, 6, 9, 4)    # B, Hi, Wi, Ho, Wo, C: 1 053 000 output quads > 4096 x 256
RESIZE_BWD_BIG = (5500, 3, 2, 6, 5, 4)     # B Hi = 16500 rows > 16384
