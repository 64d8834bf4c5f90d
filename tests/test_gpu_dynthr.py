"""Dynamic thresholding on the device (``dynamic_threshold``): the selection kernel and the thresholded update bit for
bit against the CPU fp32 restatement (tests/dynthr_helpers.py), a threshold that never binds against the static clamp,
the rejections, whole chains in the three modes against a fp64 chain, the modes against each other, and the sequence of
C entries with and without the keyword.

Chain tolerance: the thresholded map x0 -> x0c has Lipschitz constant 2 in the sup norm (an unclamped element moves by
at most (h/s)(1 + |u|/s) eps <= 2 eps, a clamped one not at all), so the bound is the clipped chains' relative MSE
times 2^2."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from dynthr_helpers import (cpu_dyn_step, dyn_chain64, dyn_dpm_chain64, quantile_rank, threshold32,  # noqa: E402
                            u32)
from inpaint_helpers import (INF, SHAPES, amp as _amp, block_mask, fp64_forward, inputs, known_data,  # noqa: E402
                             model, spy_entries)
from parity_helpers import rel_mse  # noqa: E402

from tiny_diffusion_amd import _lib  # noqa: E402
from tiny_diffusion_amd._lib import check, lib, tuned  # noqa: E402
from tiny_diffusion_amd.schedule import (GRAPH_STEPS, ForwardProcess, ddim_schedule, dpm_sample_loop,  # noqa: E402
                                         dpm_solver_schedule, sample_loop)

TDX_E_BADARG = -1
CHAIN_TOL = 1e-8    # the project's chain tolerance (test_gpu_clip.py: relative MSE against fp64)
LIP2 = 4            # the square of the thresholded map's Lipschitz constant
X0, MS = _lib.STEP_X0, _lib.STEP_MS
MODES = {"eager": dict(use_graph=False), "graph": dict(use_graph=True), "philox": dict(use_graph=True, philox_seed=7)}
S_K = 10


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _tables():
    fp = ForwardProcess()
    sched = ddim_schedule(fp, steps=S_K, eta=0.5)
    ms = dpm_solver_schedule(fp, steps=S_K, spacing="uniform")
    assert ms.steps == S_K
    return {"x0": (sched.x0_form(fp, "eps"), sched.device_tables("cuda")[0]), "ms": (ms.multistep_form(fp, "eps"), None)}


def _draw(shape, row, w, seed, scale=1.5):
    """x ~ N(0, 1) and an output such that the implied x0 is about N(0, scale^2) (the guided pair combines to it)."""
    g = torch.Generator().manual_seed(seed)
    p, q = row[0].item(), row[1].item()
    x = torch.randn(shape, generator=g)
    x0 = scale * torch.randn(shape, generator=g)
    out = (x0 - p * x) / q
    z = torch.randn(shape, generator=g)
    if w is not None:
        d = torch.randn(shape, generator=g)
        out = torch.cat([out + (1 - w) * d, out - w * d])
    return x.contiguous(), out.contiguous(), z.contiguous()


def _threshold(x, out, per, coef, t_idx, w, lo, hi, rank, frac, thr, n=None):
    return lib.tdx_x0_dyn_threshold(_p(x), _p(out), x.shape[0] if n is None else n, per, _p(coef), _p(t_idx),
                                    int(w is not None), w or 0.0, lo, hi, rank, frac, _p(thr), _stream())


def _update_dyn(xo, x, out, n, form, coef, t_idx, tau, z, philox, seed, w, lo, hi, hist, known, mask, cdec, thr, per):
    return lib.tdx_p_sample_update_dyn(_p(xo), _p(x), _p(out), n, form, _p(coef), _p(t_idx), _p(tau), _p(z), philox,
                                       seed, int(w is not None), w or 0.0, lo, hi, _p(hist), _p(known), _p(mask),
                                       _p(cdec), _p(thr), per, _stream())


def _update(xo, x, out, n, form, coef, t_idx, tau, z, w, lo, hi, hist):
    return lib.tdx_p_sample_update(_p(xo), _p(x), _p(out), n, form, _p(coef), _p(t_idx), _p(tau), _p(z), 0, 0,
                                   int(w is not None), w or 0.0, lo, hi, _p(hist), None, None, None, _stream())


# ---------------------------------------------------------------- 1. the selection kernel, bit for bit
# 1024 and 1028: with 256 threads of one float4 each, exactly one trip of the kernel's loops, and one trip plus one float4
PERS = [4, 20, 784, 1024, 1028, 4096, 16384]
KINDS = ["random", "tied", "constant", "zeros", "guided", "asym"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("per", PERS)
def test_threshold_kernel_bitwise(per, kind):
    n, k = 3, 4
    tab = _tables()["x0"][0]
    lo, hi = (-0.75, 0.5) if kind == "asym" else (-1.0, 1.0)
    w = 2.5 if kind == "guided" else None
    g = torch.Generator().manual_seed(per + len(kind))
    if kind == "tied":        # u = x - out in multiples of 0.25: many equal keys, a[rank + 1] == a[rank]
        tab = torch.tensor([[1.0, -1.0, 0.5, 0.5, 0.1]] * S_K)
        x = torch.round(4 * torch.randn(n, per, generator=g)) / 4
        out = torch.round(4 * torch.randn(n, per, generator=g)) / 4
    elif kind == "constant":
        x = torch.ones(n, per) * torch.tensor([[0.5], [-1.75], [3.0]])
        out = torch.ones(n, per) * torch.tensor([[-0.25], [0.5], [1.0]])
    elif kind == "zeros":
        x, out = torch.zeros(n, per), torch.zeros(n, per)
    else:
        x, out, _ = _draw((n, per), tab[k], w, seed=per)
    coef = tab.cuda().contiguous()
    t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
    xd, od = x.cuda().contiguous(), out.cuda().contiguous()
    u = u32(x, out, tab[k], lo, hi, w)
    a = u.abs().sort(dim=1).values
    ties = 0
    for q in (0.5 / per, 0.5, 0.995, 1.0):
        rank, frac = quantile_rank(q, per)
        if q < 0.5:
            assert rank == 0 and frac > 0
        s, r, _ = threshold32(u, lo, hi, rank, frac)
        ties += int((a[:, rank] == a[:, min(rank + 1, per - 1)]).sum())
        thr = torch.full((n, 2), -7.0, device="cuda")
        keep = [t.clone() for t in (xd, od, coef, t_idx)]
        check(_threshold(xd, od, per, coef, t_idx, w, lo, hi, rank, frac, thr))
        want = torch.stack([s, r], dim=1)
        assert torch.equal(thr.cpu(), want), (q, rank, frac, thr.cpu().tolist(), want.tolist())
        for t, saved in zip((xd, od, coef, t_idx), keep):    # inputs untouched
            assert torch.equal(t, saved)
    if kind in ("tied", "constant", "zeros"):
        assert ties > 0
    if kind == "zeros" and lo == -1.0:
        assert torch.equal(thr.cpu(), torch.tensor([[1.0, 1.0]] * n))      # s = h, r = 1: the static clamp


def test_threshold_kernel_many_samples_more_than_one_row():
    """More workgroups than one wave of them, each on its own sample and its own row of the buffer."""
    n, per, k = 300, 20, 2
    tab = _tables()["x0"][0]
    x, out, _ = _draw((n, per), tab[k], None, seed=3)
    rank, frac = quantile_rank(0.9, per)
    s, r, _ = threshold32(u32(x, out, tab[k], -1.0, 1.0), -1.0, 1.0, rank, frac)
    thr = torch.zeros(n, 2, device="cuda")
    t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
    check(_threshold(x.cuda(), out.cuda(), per, tab.cuda(), t_idx, None, -1.0, 1.0, rank, frac, thr))
    assert torch.equal(thr.cpu(), torch.stack([s, r], dim=1))


# ---------------------------------------------------------------- 2. the thresholded update, bit for bit
def _philox_noise(shape, k, tau, seed):
    """The noise the existing Philox update draws at step k: that update on x = 0, eps = 0 with the row (1, 0, 1)."""
    zero = torch.zeros(shape, device="cuda")
    got = torch.empty(shape, device="cuda")
    coef3 = torch.tensor([[1.0, 0.0, 1.0]] * S_K, device="cuda")
    t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
    if tau is None:
        check(lib.tdx_p_sample_step_philox(got.data_ptr(), zero.data_ptr(), zero.data_ptr(), coef3.data_ptr(),
                                           t_idx.data_ptr(), zero.numel(), seed, _stream()))
    else:
        check(lib.tdx_p_sample_step_sched_philox(got.data_ptr(), zero.data_ptr(), zero.data_ptr(), coef3.data_ptr(),
                                                 tau.data_ptr(), t_idx.data_ptr(), zero.numel(), seed, _stream()))
    return got


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("form", ["x0", "ms"])
def test_update_dyn_bitwise(form, guided, masked):
    shape, per = (2, 1, 28, 28), 784
    n = shape[0]
    tab, tau_dev = _tables()[form]
    coef = tab.cuda().contiguous()
    w = 2.5 if guided else None
    lo, hi = -1.0, 1.0
    rank, frac = quantile_rank(0.9, per)
    known = known_data(n, shape[1:], seed=2) if masked else None
    mask = block_mask(shape[1:]).expand(shape).contiguous() if masked else None
    kd, md = (None, None) if not masked else (known.cuda(), mask.cuda())
    FORM = X0 if form == "x0" else MS
    for k in (0, 1, S_K - 2, S_K - 1):
        x, out, z = _draw(shape, tab[k], w, seed=7 * k + guided + 2 * masked)
        zh = z if form == "x0" else 0.5 * z          # the noise, or the history of the step before
        want, h_want, (s, r) = cpu_dyn_step(form, x, out, zh, tab[k], lo, hi, k, rank, frac, w, known, mask)
        u = u32(x, out, tab[k], lo, hi, w)
        sb = s.reshape(-1, 1, 1, 1)
        assert (s > 1).all() and (u.abs() > sb).any() and (u.abs() < sb).any()    # binds: clamped and unclamped elements
        if form == "ms":
            assert (tab[k, 4].item() != 0) == (0 < k < S_K - 1)
        thr = torch.stack([s, r], dim=1).cuda().contiguous()
        t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
        for tau in ((None, tau_dev) if form == "x0" else (None,)):
            xd = (torch.cat([x, x]) if guided else x).cuda().contiguous()
            od, zd = out.cuda(), zh.cuda().contiguous()
            hist = zd.clone() if form == "ms" else None
            cdec = torch.tensor([99], dtype=torch.int64, device="cuda")
            keep = [t.clone() for t in (od, coef, t_idx, thr)]
            xo = xd if guided else torch.empty_like(xd)      # guided: in place by definition, both halves of x
            check(_update_dyn(xo, xd, od, x.numel(), FORM, coef, t_idx, tau, None if form == "ms" else zd, 0, 0, w, lo, hi,
                              hist, kd, md, cdec, thr, per))
            assert torch.equal(xo[:n].cpu(), want), (k, (xo[:n].cpu() - want).abs().max().item())
            assert cdec.item() == k - 1
            if guided:
                assert torch.equal(xo[n:], xo[:n])
            else:      # the input untouched, and in place gives the same
                assert torch.equal(xd.cpu(), x)
                h2 = zd.clone() if form == "ms" else None
                check(_update_dyn(xd, xd, od, x.numel(), FORM, coef, t_idx, tau, None if form == "ms" else zd, 0, 0, w,
                                  lo, hi, h2, kd, md, None, thr, per))
                assert torch.equal(xd.cpu(), want)
            if form == "ms":
                assert torch.equal(hist.cpu(), h_want)      # the history is the thresholded (and blended) value
            for t, saved in zip((od, coef, t_idx, thr), keep):
                assert torch.equal(t, saved)
            if form == "x0":
                # in-kernel noise = the tensor form fed the noise the existing Philox update draws under this seed
                zp = _philox_noise(shape, k, tau, seed=11)
                assert (zp.abs().max() > 0) == (k > 0)
                xa = (torch.cat([x, x]) if guided else x).cuda().contiguous()
                xb = xa.clone()
                check(_update_dyn(xa, xa, od, x.numel(), FORM, coef, t_idx, tau, None, 1, 11, w, lo, hi, None, kd, md,
                                  None, thr, per))
                check(_update_dyn(xb, xb, od, x.numel(), FORM, coef, t_idx, tau, zp, 0, 0, w, lo, hi, None, kd, md,
                                  None, thr, per))
                assert torch.equal(xa, xb) and torch.isfinite(xa).all()
        if k == 0 and not masked:
            assert want.min() >= lo and want.max() <= hi      # the last step returns the thresholded prediction


# ---------------------------------------------------------------- 3. a threshold that never binds
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("form", ["x0", "ms"])
def test_a_threshold_that_never_binds_is_the_static_clamp(form, guided):
    shape, per, k = (2, 1, 28, 28), 784, 3
    n = shape[0]
    tab, tau = _tables()[form]
    coef = tab.cuda().contiguous()
    w = 2.5 if guided else None
    rank, frac = quantile_rank(0.5, per)
    x, out, z = _draw(shape, tab[k], w, seed=5, scale=1.0)
    u = u32(x, out, tab[k], -1.0, 1.0, w)
    _, _, sq = threshold32(u, -1.0, 1.0, rank, frac)
    assert (sq <= 1).all() and (u.abs() > 1).any() and (u.abs() < 1).any()      # s = h; the static clamp does bind
    t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
    xd = (torch.cat([x, x]) if guided else x).cuda().contiguous()
    od, zd = out.cuda(), z.cuda()
    thr = torch.zeros(n, 2, device="cuda")
    check(_threshold(xd, od, per, coef, t_idx, w, -1.0, 1.0, rank, frac, thr, n=n))
    assert torch.equal(thr.cpu(), torch.ones(n, 2))
    FORM = X0 if form == "x0" else MS
    xa, xb = xd.clone(), xd.clone()
    ha, hb = (zd.clone(), zd.clone()) if form == "ms" else (None, None)
    zz = None if form == "ms" else zd
    check(_update_dyn(xa, xa, od, x.numel(), FORM, coef, t_idx, tau, zz, 0, 0, w, -1.0, 1.0, ha, None, None, None, thr, per))
    check(_update(xb, xb, od, x.numel(), FORM, coef, t_idx, tau, zz, w, -1.0, 1.0, hb))
    assert torch.equal(xa, xb) and not torch.equal(xa, xd)
    if form == "ms":
        assert torch.equal(ha, hb)


# ---------------------------------------------------------------- 4. rejections
def test_rejections_write_nothing():
    per, n = 8, 2
    tab, _ = _tables()["x0"]
    coef = tab.cuda().contiguous()
    x = torch.full((n * per,), 3.0, device="cuda")
    xo = torch.full((n * per,), -5.0, device="cuda")
    out = torch.zeros(2 * n * per, device="cuda")
    hist = torch.full((n * per,), 2.0, device="cuda")
    thr = torch.tensor([[1.0, 1.0]] * n, device="cuda")
    t_idx = torch.ones(1, dtype=torch.int32, device="cuda")
    nan = float("nan")

    def upd(form=X0, n_el=n * per, lo=-1.0, hi=1.0, thr_=thr, per_=per, hist_=None, x_out=xo, w=None):
        return _update_dyn(x_out, x, out, n_el, form, coef, t_idx, None, None, 0, 0, w, lo, hi, hist_, None, None, None,
                           thr_, per_)

    bad = [dict(form=_lib.STEP_EPS), dict(thr_=None), dict(per_=0), dict(per_=-8), dict(per_=6), dict(per_=12),
           dict(n_el=12, per_=8), dict(lo=-INF), dict(hi=INF), dict(lo=-INF, hi=INF), dict(lo=nan), dict(hi=nan),
           dict(lo=1.0, hi=-1.0), dict(n_el=0), dict(form=MS), dict(form=7)]
    for kw in bad:
        assert upd(**kw) == TDX_E_BADARG, kw
        if "form" not in kw:
            assert upd(form=MS, hist_=hist, **kw) == TDX_E_BADARG, kw
    torch.cuda.synchronize()
    assert (xo == -5.0).all() and (x == 3.0).all() and (hist == 2.0).all()
    # the selection kernel
    tb = torch.full((n, 2), -7.0, device="cuda")

    def sel(x_=x, out_=out, n_=n, per_=per, coef_=coef, t_=t_idx, lo=-1.0, hi=1.0, rank=3, frac=0.5, thr_=tb):
        return lib.tdx_x0_dyn_threshold(_p(x_), _p(out_), n_, per_, _p(coef_), _p(t_), 0, 0.0, lo, hi, rank, frac,
                                        _p(thr_), _stream())

    for kw in (dict(x_=None), dict(out_=None), dict(coef_=None), dict(t_=None), dict(thr_=None), dict(n_=0), dict(n_=-1),
               dict(per_=0), dict(per_=6), dict(lo=-INF), dict(hi=INF), dict(lo=nan), dict(lo=1.0, hi=1.0),
               dict(rank=-1), dict(rank=per), dict(frac=-0.5), dict(frac=1.5), dict(frac=nan)):
        assert sel(**kw) == TDX_E_BADARG, kw
    torch.cuda.synchronize()
    assert (tb == -7.0).all()
    # and the good calls do write
    assert sel() == 0 and upd() == 0 and upd(form=MS, hist_=hist) == 0
    torch.cuda.synchronize()
    assert not (tb == -7.0).any() and not (xo == -5.0).any() and not (hist == 2.0).any()


def test_eval_step_dyn_rejections_write_nothing():
    n, S = 2, 2
    fp = ForwardProcess()
    m = model("uncond", 3).eval()
    sched = ddim_schedule(fp, timesteps=[200, 700], eta=1.0)
    tau = sched.device_tables("cuda")[0]
    coef = sched.x0_form(fp, "eps", device="cuda")
    x_T, _, _ = inputs("uncond", n, 1, seed=2)
    x = x_T.cuda().contiguous()
    counter = torch.tensor([1], dtype=torch.int64, device="cuda")
    t_idx = torch.full((1,), -3, dtype=torch.int32, device="cuda")
    t_vec = torch.full((n,), -3, dtype=torch.int64, device="cuda")
    out = torch.zeros_like(x)
    thr = torch.full((n, 2), -7.0, device="cuda")
    for clip, dyn in (((-INF, INF), (700, 0.5, thr)), ((-1.0, INF), (700, 0.5, thr)), ((-1.0, 1.0), (784, 0.0, thr)),
                      ((-1.0, 1.0), (-1, 0.0, thr)), ((-1.0, 1.0), (700, 1.5, thr))):
        with torch.no_grad(), pytest.raises(_lib.TdxError, match="tdx_unet_eval_step_update_dyn"):
            m._run_eval_step(x, None, coef, counter, t_idx, t_vec, out, philox_seed=9, tau=tau, S=S, clip=clip, dyn=dyn)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), x_T) and counter.item() == 1 and t_idx.item() == -3 and (thr == -7.0).all()
    with torch.no_grad():
        m._run_eval_step(x, None, coef, counter, t_idx, t_vec, out, philox_seed=9, tau=tau, S=S, clip=(-1.0, 1.0),
                         dyn=(700, 0.5, thr))
    assert counter.item() == 0 and t_idx.item() == 1 and int(t_vec[-1]) == 700 and (thr[:, 0] >= 1).all()
    assert not torch.equal(x.cpu(), x_T) and torch.isfinite(x).all()


# ---------------------------------------------------------------- 5. chains against fp64
# (kind, w, prediction, n, q): q chosen per model on the CPU so that the fp64 chain alone has s > h on some (sample, step)
# pairs and s == h on others (every step rescales a sample's q-quantile to h, so the next step's lies close to h on
# either side), with clamped and unclamped elements on the former - asserted below
CHAINS = [("uncond", None, "eps", 4, 0.1), ("cond", 3.0, "eps", 5, 0.9), ("uncond", None, "v", 4, 0.1),
          ("laion", None, "eps", 4, 0.5), ("latent", None, "eps", 4, 0.9), ("transformer", None, "eps", 4, 0.995)]


def _chain_inputs(kind, n):
    g = torch.Generator().manual_seed(11 + n)
    x_T = torch.randn(n, *SHAPES[kind], generator=g)
    if kind == "uncond":
        y = None
    elif kind == "laion":
        y = torch.randn(n, 768, generator=g).cuda()
    else:
        y = torch.randint(0, 10, (n,), generator=g).cuda()
    return x_T, y


@pytest.mark.parametrize("kind,w,prediction,n,q", CHAINS)
def test_thresholded_ddim_chain_against_fp64(kind, w, prediction, n, q):
    S = 10
    fp = ForwardProcess()
    m = model(kind, 1)
    x_T, y = _chain_inputs(kind, n)
    sched = ddim_schedule(fp, steps=S)
    want, stats = dyn_chain64(fp64_forward(kind, 1), kind, fp, sched, x_T, y, -1.0, 1.0, q, prediction, w)
    print(f"thresholded DDIM eta=0 S={S} {kind} w={w} {prediction} q={q}: fp64 chain {stats}")
    assert stats.ok(), stats
    assert want.min() >= -1 and want.max() <= 1
    bound = LIP2 * CHAIN_TOL * _amp(w)
    for mode, kw in MODES.items():   # eta = 0 draws no noise: the Philox mode is comparable too
        got = sample_loop(m, fp, "cuda", n, y, x_T=x_T, schedule=sched, guidance_scale=w, prediction=prediction,
                          dynamic_threshold=q, **kw)
        r = rel_mse(got, want)
        print(f"thresholded DDIM eta=0 S={S} {kind} w={w} {prediction} q={q} {mode}: relative MSE vs fp64 {r:.3e} "
              f"(bound {bound:.1e})")
        assert got.shape == x_T.shape and r < bound, (mode, r)
        assert got.min() >= -1 and got.max() <= 1


def test_thresholded_dpm_chain_with_inpainting_against_fp64():
    kind, w, n, q = "uncond", None, 4, 0.3
    fp = ForwardProcess()
    m = model(kind, 1)
    x_T, _, y = inputs(kind, n, 1, seed=21)
    known = known_data(n, SHAPES[kind], seed=3).clamp(-1, 1)
    mask = block_mask(SHAPES[kind])
    taus = dpm_solver_schedule(fp, steps=10).timesteps.tolist()
    want, stats = dyn_dpm_chain64(fp64_forward(kind, 1), kind, fp, taus, x_T, y, -1.0, 1.0, q, "eps", w, known, mask)
    print(f"thresholded masked DPM-Solver++(2M) S={len(taus)} {kind} q={q}: fp64 chain {stats}")
    assert stats.ok(), stats
    bound = LIP2 * CHAIN_TOL * _amp(w)
    mf = mask.expand(n, *SHAPES[kind])
    for mode, kw in MODES.items():
        got = dpm_sample_loop(m, fp, "cuda", n, y, steps=10, x_T=x_T, known=known, mask=mask, dynamic_threshold=q, **kw)
        r = rel_mse(got, want)
        print(f"thresholded masked DPM-Solver++(2M) {kind} q={q} {mode}: relative MSE vs fp64 {r:.3e} (bound {bound:.1e})")
        assert r < bound, (mode, r)
        assert got.min() >= -1 and got.max() <= 1
        assert torch.equal(got.cpu()[mf == 1], known.expand_as(got)[mf == 1])      # the known region, bit for bit


# ---------------------------------------------------------------- 6. the modes against each other
@pytest.mark.parametrize("kind,w,prediction", [("uncond", None, "eps"), ("cond", 2.0, "v"), ("laion", 2.0, "eps"),
                                               ("latent", None, "eps")])
def test_thresholded_philox_graph_equals_eager(kind, w, prediction):
    """In-kernel noise: the graph mode (device counter, the one-call thresholded step, a tail graph) equals the eager
    chain bit for bit with the sampling tables off, and within the pairing tolerance of
    test_gpu_clip.py::test_clipped_philox_graph_equals_eager (the table mode reassociates one projection sum) times the
    factor 4 with them on."""
    n, S, q = 4, 13, 0.9
    assert S % GRAPH_STEPS
    fp = ForwardProcess()
    m = model(kind, 4)
    x_T, _, y = inputs(kind, n, 1, seed=S)
    sched = ddim_schedule(fp, steps=S, eta=0.5)
    assert float(sched.coef[1:, 2].min()) > 0
    kw = dict(x_T=x_T, schedule=sched, guidance_scale=w, prediction=prediction, dynamic_threshold=q, philox_seed=4)
    pe = sample_loop(m, fp, "cuda", n, y, **kw)
    pt = sample_loop(m, fp, "cuda", n, y, use_graph=True, **kw)
    with tuned(sample_tables=0):
        pg = sample_loop(m, fp, "cuda", n, y, use_graph=True, **kw)
    assert torch.isfinite(pe).all() and pe.min() >= -1 and pe.max() <= 1
    assert torch.equal(pg, pe), rel_mse(pg, pe)
    r = rel_mse(pt, pe)
    print(f"thresholded graph + Philox vs eager + Philox {kind} w={w} {prediction} S={S}: relative MSE {r:.3e} "
          f"(bound {LIP2 * 1e-10:.1e})")
    assert r < LIP2 * 1e-10
    other = sample_loop(m, fp, "cuda", n, y, use_graph=True, **{**kw, "philox_seed": 5})
    assert rel_mse(other, pe) > 1e-4      # the comparison can tell one noise stream from another
    clipped = sample_loop(m, fp, "cuda", n, y, use_graph=True, **{**kw, "dynamic_threshold": None, "clip_denoised": True})
    assert rel_mse(clipped, pe) > 1e-4    # ... and a thresholded chain from a clipped one


# ---------------------------------------------------------------- 7. call sequences
NEW = ("tdx_x0_dyn_threshold", "tdx_p_sample_update_dyn", "tdx_unet_eval_step_update_dyn")


def test_call_sequences(monkeypatch):
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import diffusion as D

    calls = []
    watched = [nm for nm in _lib.EXPORTS if "p_sample_step" in nm or "p_sample_update" in nm or "eval_step" in nm
               or "dyn_threshold" in nm]
    assert set(NEW) <= set(watched)
    spy_entries(monkeypatch, lib, watched, calls)
    n, T, S = 3, 20, 6
    fp = ForwardProcess(num_timesteps=T)
    Sd = dpm_solver_schedule(fp, steps=S).steps
    for kind, mod, w in (("uncond", D, None), ("cond", C, 2.0)):
        g = ",guided" if w is not None else ""
        up, ev = "tdx_p_sample_update[", "tdx_unet_eval_step_update["
        m = model(kind, 2)
        x_T, zs, y = inputs(kind, n, T, seed=4)
        cond = dict(n_samples=n) if kind == "uncond" else dict(n_samples=n, y=y, guidance_scale=w)
        rec, phx = dict(x_T=x_T, noises=zs), dict(x_T=x_T, use_graph=True, philox_seed=3)
        # dynamic_threshold=None: today's call strings, none of the new entries
        expect = [
            ("sample", {}, rec, [up + "eps" + g + "]"] * T),
            ("sample", {}, phx, [ev + "eps" + g + "]" if g else "tdx_unet_eval_step"] * (1 + GRAPH_STEPS)),
            ("ddim_sample", dict(steps=S, eta=0.4, clip_denoised=True), rec, [up + "x0,sched" + g + "]"] * S),
            ("ddim_sample", dict(steps=S, eta=0.4, clip_denoised=True), phx, [ev + "x0,sched" + g + "]"] * (1 + S)),
            ("dpm_sample", dict(steps=S), dict(x_T=x_T), [up + "ms,sched" + g + "]"] * Sd),
            ("dpm_sample", dict(steps=S), phx, [ev + "ms,sched" + g + "]"] * (1 + Sd)),
        ]
        for sampler, extra, kw, want in expect:
            outs = []
            for none in ({}, dict(dynamic_threshold=None)):
                calls.clear()
                outs.append(getattr(mod, sampler)(m, fp, "cuda", **cond, **extra, **kw, **none))
                assert calls == want, (kind, sampler, list(kw), calls)
            assert torch.equal(outs[0], outs[1]), (kind, sampler, list(kw))
        # dynamic_threshold set: eager - the selection then the update, once per step; one-call mode - only the new step
        pair = ["tdx_x0_dyn_threshold", "tdx_p_sample_update_dyn"]
        for sampler, extra, steps in (("sample", {}, T), ("ddim_sample", dict(steps=S, eta=0.4), S),
                                      ("dpm_sample", dict(steps=S), Sd)):
            rk = dict(x_T=x_T) if sampler == "dpm_sample" else rec
            calls.clear()
            eager = getattr(mod, sampler)(m, fp, "cuda", **cond, **extra, **rk, dynamic_threshold=0.9)
            assert calls == pair * steps, (kind, sampler, calls)
            calls.clear()
            getattr(mod, sampler)(m, fp, "cuda", **cond, **extra, **phx, dynamic_threshold=0.9)
            warm = 1 + min(steps, GRAPH_STEPS) + (steps % GRAPH_STEPS if steps > GRAPH_STEPS else 0)
            assert calls == ["tdx_unet_eval_step_update_dyn"] * warm, (kind, sampler, calls)
            assert eager.min() >= -1 and eager.max() <= 1
