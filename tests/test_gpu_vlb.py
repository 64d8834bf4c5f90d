"""Variational-bound evaluation on the device: ``tdx_vlb_terms`` per sample against the fp64 restatement
(tests/vlb_helpers.py) fed the bit-identical fp32 (d, e), its bit reproducibility, the edge classes of the decoder, the
prior row, and the loop of all five models against the restatement fed the same noise and the network outputs the test
evaluates itself - t order, column placement, tables, prior and units; the network is not under test.

Bounds (vlb_helpers): the two sums of squares SUM_TOL = 2e-5 relative (derived); the decoder sum DEC_K times the
per-element distance of the fp32 CPU restatement from fp64 plus SUM_TOL, and under DEC_CAP = 1e-4 relative in any
case.  Every figure is printed before it is asserted."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import vlb_helpers as H  # noqa: E402
from inpaint_helpers import NUM_CLASSES, SHAPES, model  # noqa: E402

from tiny_diffusion_amd import _lib  # noqa: E402
from tiny_diffusion_amd._lib import check, lib  # noqa: E402
from tiny_diffusion_amd.likelihood import bits_per_dim_loop, bits_per_dim_terms  # noqa: E402
from tiny_diffusion_amd.schedule import ForwardProcess  # noqa: E402

INF = H.INF
SENTINEL = -7.0


def _launch(x0, x_t, out, noise, t, rows, clip=(-INF, INF), data_range=(-1.0, 1.0), bins=256, stride=3, into=None):
    """One ``tdx_vlb_terms`` launch on device copies of the CPU tensors.  Returns the (B, 3) buffer it wrote,
    sentinel-filled before; ``into=(buffer, first float)``: writes there instead, ``stride`` floats between samples."""
    B, per = x0.shape
    dev = [None if v is None else v.cuda().contiguous() for v in (x0, x_t, out, noise, t, rows)]
    terms = torch.full((B, 3), SENTINEL, device="cuda") if into is None else into[0]
    ptr = terms.data_ptr() + (0 if into is None else 4 * into[1])
    check(lib.tdx_vlb_terms(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), _lib.ptr(dev[3]), dev[4].data_ptr(),
                            dev[5].data_ptr(), B, per, clip[0], clip[1], data_range[0], data_range[1], bins, ptr, stride,
                            torch.cuda.current_stream().cuda_stream), "tdx_vlb_terms")
    torch.cuda.synchronize()
    return terms.cpu()


@functools.lru_cache(maxsize=None)
def _fp1000():
    return ForwardProcess()


@functools.lru_cache(maxsize=None)
def _rows(prediction):
    return H.rows32(H.tables64(_fp1000(), prediction, "beta"), True)


def _check_sums(got, want, info, tag):
    """The three slots of every sample against the fp64 sums: returns the worst decoder ratio (error / distance)."""
    worst = 0.0
    for b in range(got.shape[0]):
        for slot, name in ((0, "sum e^2"), (1, "sum d^2")):
            g, w = got[b, slot].item(), want[b, slot].item()
            print(f"{tag} sample {b} {name}: got {g:.9g} want {w:.9g} rel {abs(g - w) / max(w, 1e-300):.2e}")
            assert abs(g - w) <= H.SUM_TOL * w, (tag, b, name, g, w)
        g, w, dist = got[b, 2].item(), want[b, 2].item(), info["dist"][b].item()
        if w == 0.0:
            assert g == 0.0, (tag, b, g)       # no decoder on this row: exactly 0
            continue
        err = abs(g - w)
        worst = max(worst, err / dist)
        print(f"{tag} sample {b} decoder: got {g:.9g} want {w:.9g} rel {err / w:.2e} restatement distance {dist / w:.2e} "
              f"ratio {err / dist:.2f} floored {info['floored'][b].item():.4f}")
        assert info["floored"][b].item() <= H.FLOOR_CAP, (tag, b)
        assert err <= H.DEC_K * dist + H.SUM_TOL * w, (tag, b, g, w, dist)
        assert err <= H.DEC_CAP * w, (tag, b, g, w)
    return worst


# ---------------------------------------------------------------- 1. the kernel against the helper, per sample
@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("per", [4, 20, 784, 4096, 16384])
def test_kernel_against_the_restatement(per, B, prediction):
    """4: fewer elements than lanes; 20: the latent width; 784: a ragged last trip; 4096, 16384: several trips."""
    fp, rows = _fp1000(), _rows(prediction)
    t = [0] if B == 1 else [500, 0, 999]
    x0, x_t, out, eps = H.gen_inputs(fp, per, t, rows)
    tt = torch.tensor(t)
    worst = 0.0
    for clip in ((-INF, INF), (-1.0, 1.0)):
        for noise in (eps, None):
            want, info = H.sums64(x0, x_t, out, noise, rows, tt, clip)
            got = _launch(x0, x_t, out, noise, tt, rows, clip).double()
            if noise is None:
                assert (got[:, 0] == 0).all()
            tag = f"per={per} B={B} {prediction} clip={clip[1]} noise={'given' if noise is not None else 'NULL'}"
            worst = max(worst, _check_sums(got, want, info, tag))
    print(f"per={per} B={B} {prediction}: worst decoder ratio {worst:.2f} (DEC_K = {H.DEC_K})")
    assert worst <= 8.0     # above that the form would be wrong, not the bound


def test_stride_places_the_columns():
    """sample_stride > 3: slots 0..2 of every sample's row are written, nothing else is touched."""
    fp, rows = _fp1000(), _rows("eps")
    t = torch.tensor([0, 7, 999])
    x0, x_t, out, eps = H.gen_inputs(fp, 784, t.tolist(), rows)
    want = _launch(x0, x_t, out, eps, t, rows)
    buf = _launch(x0, x_t, out, eps, t, rows, stride=12, into=(torch.full((3, 4, 3), SENTINEL, device="cuda"), 6))
    assert torch.equal(buf[:, 2], want)                              # column 2 of a (B, T = 4, 3) buffer
    assert (buf[:, [0, 1, 3]] == SENTINEL).all()


# ---------------------------------------------------------------- 2. bit reproducibility
@pytest.mark.parametrize("per", [20, 784, 16384])
def test_bit_reproducible_and_independent_of_the_batch(per):
    fp, rows = _fp1000(), _rows("v")
    t = torch.tensor([0, 500, 0])
    x0, x_t, out, eps = H.gen_inputs(fp, per, t.tolist(), rows)
    first = _launch(x0, x_t, out, eps, t, rows, (-1.0, 1.0))
    assert torch.equal(first, _launch(x0, x_t, out, eps, t, rows, (-1.0, 1.0)))
    for b in range(3):
        one = _launch(x0[b:b + 1], x_t[b:b + 1], out[b:b + 1], eps[b:b + 1], t[b:b + 1], rows, (-1.0, 1.0))
        assert torch.equal(one[0], first[b]), b
    assert not torch.equal(first[0], first[2])      # two samples on the same row differ: the sums are per sample


# ---------------------------------------------------------------- 3. the edge classes of the decoder
def test_edge_classes():
    """All of a sample in the first bin, all in the last, all interior - and all at data_lo + half exactly, which the
    strict < makes interior."""
    fp, rows = _fp1000(), _rows("eps")
    per = 784
    half, lo_edge, hi_edge = H.edges32((-1.0, 1.0), 256)
    t = torch.zeros(4, dtype=torch.int64)
    g = torch.Generator().manual_seed(4)
    x0 = torch.randint(13, 243, (4, per), generator=g).float() * (2.0 / 255.0) - 1.0     # row 2: interior levels
    x0[0], x0[1], x0[3] = -1.0, 1.0, lo_edge
    eps = torch.randn(4, per, generator=g)
    x_t = H.x_t_of(fp, x0, 0, eps)
    out = H.solve_out(x0, 0.02 * torch.randn(4, per, generator=g), x_t, rows, t)
    assert (x0[2] >= lo_edge).all() and (x0[2] <= hi_edge).all()
    want, info = H.sums64(x0, x_t, out, eps, rows, t)
    got = _launch(x0, x_t, out, eps, t, rows).double()
    _check_sums(got, want, info, "edge classes")
    d = info["d"]
    as_first_bin = -torch.log(torch.maximum(0.5 * torch.erfc(-((d[3].double() + half) * rows[0, 4].double())
                                                             * 0.70710678118654752), torch.tensor(H.FLOOR).double())).sum()
    assert abs(as_first_bin.item() - want[3, 2].item()) > 100 * H.DEC_CAP * want[3, 2].item()   # the classes differ
    assert torch.tensor(lo_edge) == torch.tensor(-1.0) + torch.tensor(half)


# ---------------------------------------------------------------- 4. the prior row
@pytest.mark.parametrize("per", [20, 784, 4096])
def test_prior_row_gives_the_sum_of_squares(per):
    g = torch.Generator().manual_seed(per)
    x0 = (2 * torch.rand(3, per, generator=g) - 1).contiguous()
    zero_row = torch.zeros(1, 5)
    t = torch.zeros(3, dtype=torch.int64)
    got = _launch(x0, x0, x0, None, t, zero_row, bins=0).double()
    want = (x0.double() ** 2).sum(1)
    print(f"per={per}: prior sums {got[:, 1].tolist()} want {want.tolist()}")
    assert ((got[:, 1] - want).abs() <= H.SUM_TOL * want).all()
    assert (got[:, 0] == 0).all() and (got[:, 2] == 0).all()


# ---------------------------------------------------------------- 5. the loop, all five models
T_LOOP = 6
KINDS = ["uncond", "cond", "laion", "latent", "transformer"]
PIXELS = ("uncond", "cond")


def _module(kind):
    from tiny_diffusion_amd import (conditional_diffusion, conditional_diffusion_laion, diffusion, diffusion_transformer,
                                    latent_diffusion)
    return {"uncond": diffusion, "cond": conditional_diffusion, "laion": conditional_diffusion_laion,
            "latent": latent_diffusion, "transformer": diffusion_transformer}[kind]


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(model, fp, x_0, condition, T recorded noises) of one kind, built once and never changed."""
    B = 4 if kind == "latent" else 2
    g = torch.Generator().manual_seed(11 + len(kind))
    shape = SHAPES[kind]
    if kind in PIXELS:
        x0 = torch.randint(0, 256, (B, *shape), generator=g).float() * (2.0 / 255.0) - 1.0
    else:
        x0 = torch.randn(B, *shape, generator=g)
    zs = torch.randn(T_LOOP, B, *shape, generator=g)
    if kind == "uncond":
        y = None
    elif kind == "laion":
        y = torch.randn(B, 768, generator=g).cuda()
    else:
        y = torch.randint(0, NUM_CLASSES, (B,), generator=g).cuda()
    return model(kind).eval(), ForwardProcess(num_timesteps=T_LOOP), x0.contiguous(), y, zs


@functools.lru_cache(maxsize=None)
@torch.no_grad()
def _outs(kind):
    """The network evaluated by the test, in eval mode, at the x_t of the reference's fp32 q_sample expression."""
    m, fp, x0, y, zs = _case(kind)
    outs = []
    for t in range(T_LOOP):
        x_t = H.x_t_of(fp, x0, t, zs[t]).cuda()
        tv = torch.full((x0.shape[0],), t, dtype=torch.int64, device="cuda")
        outs.append((m(x_t, tv) if y is None else m(x_t, tv, y)).cpu())
    return outs


def _compare(got, want, x0, bins, D, tag):
    """Every field against the restatement, the bounds of test 1 carried through the host formulas: an error of
    SUM_TOL in sum d^2 moves a KL term by g_t SUM_TOL sum d^2 / (D L), the continuous decoder by SUM_TOL sum d^2 /
    (2 sigma2_0 D L), the prior by abar SUM_TOL sum x0^2 / (2 D L); the discretised decoder has its own bound."""
    total, prior, vb, mse, xs, info = want
    tab, sums = info["tab"], info["sums"]
    DL = D * H.LN2
    tol_vb = tab["g"][None, :] * H.SUM_TOL * sums[..., 1] / DL
    if bins:
        tol_vb[:, 0] = (H.DEC_K * info["dist"][:, 0] + H.SUM_TOL * sums[:, 0, 2]) / DL
    else:
        tol_vb[:, 0] = H.SUM_TOL * sums[:, 0, 1] / (2 * tab["s2"][0].item()) / DL
    tol_vb = tol_vb + 1e-12 * vb.abs()
    sq = (x0.double().reshape(x0.shape[0], -1) ** 2).sum(1)
    tol_prior = H.SUM_TOL * tab["acp_last"] * sq / (2 * DL) + 1e-12 * prior.abs()
    for name, g, w, tol in (("vb", got.vb, vb, tol_vb), ("mse", got.mse, mse, H.SUM_TOL * mse),
                            ("xstart_mse", got.xstart_mse, xs, H.SUM_TOL * xs), ("prior_bpd", got.prior_bpd, prior, tol_prior),
                            ("total_bpd", got.total_bpd, total, tol_vb.sum(1) + tol_prior)):
        assert g.dtype == torch.float64 and g.shape == w.shape and not g.is_cuda, (tag, name)
        err = (g - w).abs()
        print(f"{tag} {name}: worst |got - want| / tol = {(err / tol.clamp(min=1e-300)).max().item():.3f}; "
              f"want {w.flatten()[:6].tolist()}")
        assert torch.isfinite(g).all() and (err <= tol).all(), (tag, name, g.tolist(), w.tolist(), tol.tolist())
    assert torch.equal(got.total_bpd, got.prior_bpd + got.vb.sum(dim=1))


@pytest.mark.parametrize("kind", KINDS)
def test_loop_of_every_model(kind, monkeypatch):
    """The module's ``bits_per_dim`` with its defaults (pixels: 256 bins and the clamp; latents: neither), under the
    recorded noise, against the restatement - and the launches it makes: T + 1 calls of the entry, step t writing
    column t of one (B, T, 3) buffer through terms / sample_stride, the prior last."""
    m, fp, x0, y, zs = _case(kind)
    pixels = kind in PIXELS
    bins, clip = (256, (-1.0, 1.0)) if pixels else (None, (-INF, INF))
    D = x0[0].numel()
    want = H.loop64(fp, x0, zs, _outs(kind), "eps", "beta", clip, bins)
    calls = []
    real = lib.tdx_vlb_terms
    monkeypatch.setattr(lib, "tdx_vlb_terms", lambda *a: calls.append(a) or real(*a))
    mod = _module(kind)
    noises = {t: zs[t] for t in range(T_LOOP)}
    m.train()
    if kind == "uncond":
        got = mod.bits_per_dim(m, fp, x0.cuda(), noises=noises)
    elif kind == "laion":
        got = mod.bits_per_dim(m, fp, x0.cuda(), text_embeds=y, noises=noises)
    else:
        got = mod.bits_per_dim(m, fp, x0.cuda(), y=y, noises=noises)
    assert not m.training                       # left in eval mode, as sample_loop does
    assert len(calls) == T_LOOP + 1
    base = calls[0][13] - 12 * (T_LOOP - 1)
    for i, a in enumerate(calls[:-1]):
        t = T_LOOP - 1 - i
        assert a[13] == base + 12 * t and a[14] == 3 * T_LOOP and a[6:8] == (x0.shape[0], D), (i, a)
        assert a[12] == (bins or 0) and a[3] is not None
    last = calls[-1]
    assert last[3] is None and last[12] == 0 and last[14] == 3 and last[8:10] == (-INF, INF)
    _compare(got, want, x0, bins, D, kind)


@pytest.mark.parametrize("kind,prediction,variance,bins,clip", [("latent", "v", "posterior", None, None),
                                                               ("uncond", "v", "posterior", 256, True),
                                                               ("latent", "eps", "posterior", 16, (-3.0, 3.0))])
def test_loop_other_settings(kind, prediction, variance, bins, clip):
    """The v rows, the posterior variance, and bins / clamp on a latent with its own data range."""
    m, fp, x0, y, zs = _case(kind)
    D = x0[0].numel()
    data_range = (-3.0, 3.0) if kind == "latent" else (-1.0, 1.0)
    cl = (-INF, INF) if clip is None else (-1.0, 1.0) if clip is True else clip
    want = H.loop64(fp, x0, zs, _outs(kind), prediction, variance, cl, bins, data_range)
    got = bits_per_dim_loop(m, fp, x0.cuda(), y, noises=list(zs), prediction=prediction, variance=variance,
                            clip_denoised=clip, bins=bins, data_range=data_range)
    _compare(got, want, x0, bins, D, f"{kind} {prediction} {variance} bins={bins}")


# ---------------------------------------------------------------- 6. the terms against the loop
@pytest.mark.parametrize("kind", ["uncond", "latent"])
def test_terms_equal_the_loop_bit_for_bit(kind):
    m, fp, x0, y, zs = _case(kind)
    bins, clip = (256, True) if kind in PIXELS else (None, None)
    loop = bits_per_dim_loop(m, fp, x0.cuda(), y, noises=list(zs), bins=bins, clip_denoised=clip)
    B = x0.shape[0]
    t = torch.tensor([0, 3] + [5] * (B - 2))
    noise = torch.stack([zs[int(t[b])][b] for b in range(B)])
    terms = bits_per_dim_terms(m, fp, x0.cuda(), t, y, noise=noise, bins=bins, clip_denoised=clip)
    for name in ("vb", "mse", "xstart_mse"):
        got, want = getattr(terms, name), getattr(loop, name)
        assert got.shape == (B,) and got.dtype == torch.float64
        for b in range(B):
            assert got[b].item() == want[b, int(t[b])].item(), (name, b, got[b].item(), want[b, int(t[b])].item())
    # t on the device, noise drawn by the call: the same shapes, finite numbers
    drawn = bits_per_dim_terms(m, fp, x0.cuda(), t.cuda(), y, bins=bins, clip_denoised=clip)
    assert all(torch.isfinite(v).all() and v.shape == (B,) for v in drawn)


# ---------------------------------------------------------------- 7. Philox
def test_philox_seed_reproduces_the_loop():
    m, fp, x0, y, _ = _case("latent")
    a = bits_per_dim_loop(m, fp, x0.cuda(), y, philox_seed=5)
    b = bits_per_dim_loop(m, fp, x0.cuda(), y, philox_seed=5)
    c = bits_per_dim_loop(m, fp, x0.cuda(), y, philox_seed=6)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert not torch.equal(a.vb, c.vb) and not torch.equal(a.mse, c.mse)
    assert torch.equal(a.prior_bpd, c.prior_bpd)            # the prior does not see the noise
    ta = bits_per_dim_terms(m, fp, x0.cuda(), torch.tensor([0, 1, 2, 5]), y, philox_seed=5)
    tb = bits_per_dim_terms(m, fp, x0.cuda(), torch.tensor([0, 1, 2, 5]), y, philox_seed=5)
    assert all(torch.equal(u, v) and torch.isfinite(u).all() for u, v in zip(ta, tb))


# ---------------------------------------------------------------- 8. under the averaged weights
def test_under_ema_weights():
    """``with step.ema_weights():`` puts the average under the loop's forward, stale inference packs included: the bound
    equals that of a second model loaded with the average bit for bit, differs from the live weights', and the live
    weights are back afterwards."""
    from oracle.weights import make_state_dict
    from tiny_diffusion_amd import diffusion as D
    from tiny_diffusion_amd.train import TrainStep

    fp = ForwardProcess(num_timesteps=T_LOOP)
    m = D.NoiseModel()
    m.load_state_dict(make_state_dict(1, False), strict=True)
    m = m.cuda().train()
    step = TrainStep(m, fp, lr=1e-3, ema_decay=0.5)
    g = torch.Generator().manual_seed(21)
    x0 = (torch.randint(0, 256, (8, 1, 28, 28), generator=g).float() * (2.0 / 255.0) - 1.0).cuda()
    zs = list(torch.randn(T_LOOP, 2, 1, 28, 28, generator=g))
    for _ in range(3):
        step.step(x0)
    live = D.bits_per_dim(m, fp, x0[:2], noises=zs)      # also warms the inference packs of the live weights
    with step.ema_weights():
        ema = D.bits_per_dim(m, fp, x0[:2], noises=zs)
    again = D.bits_per_dim(m, fp, x0[:2], noises=zs)
    m2 = D.NoiseModel()
    m2.load_state_dict(step.ema_state_dict(), strict=True)
    want = D.bits_per_dim(m2.cuda(), fp, x0[:2], noises=zs)
    for a, b, c, d in zip(ema, want, live, again):
        assert torch.equal(a, b) and torch.equal(c, d)
    assert not torch.equal(ema.vb, live.vb) and torch.isfinite(ema.total_bpd).all()
