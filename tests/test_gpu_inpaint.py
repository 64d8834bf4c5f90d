"""Inpainting on the device (``known`` / ``mask``): the masked update kernels bit for bit against a CPU fp32 restatement,
an all-zero mask against the unmasked entries, bad arguments, the fused epilogue of final_conv against the separate
kernels, whole chains against fp64 chains with the blend (the oracle's network in double), graph + Philox against eager
Philox, the known region returned exactly, ``known=None`` is the path as it was, nothing stale between masked and
unmasked calls.

The blend x0m = (1 - m) x0c + m known is a convex combination, 1-Lipschitz in x0c like the clamp before it, so the chain
tolerances are the unmasked chains' (``CHAIN_TOL``)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from inpaint_helpers import (INF, SHAPES, amp, block_mask, cpu_ms_masked_step, cpu_x0_masked_step,  # noqa: E402
                             fp64_forward, inpaint_chain64, inpaint_dpm_chain64, inputs, known_data, model, null_cond,
                             spy_entries)
from parity_helpers import rel_mse  # noqa: E402

from tiny_diffusion_amd._lib import check, lib, tuned  # noqa: E402
from tiny_diffusion_amd.schedule import (GRAPH_STEPS, ForwardProcess, ddim_sample_loop, ddim_schedule,  # noqa: E402
                                         dpm_sample_loop, dpm_solver_schedule, sample_loop)

NAN = float("nan")
TDX_E_BADARG = -1
CHAIN_TOL = 1e-8    # the project's chain tolerance (test_gpu_clip.py / test_gpu_ddim.py: relative MSE against fp64)
MODES = {"eager": dict(use_graph=False), "graph": dict(use_graph=True), "philox": dict(use_graph=True, philox_seed=7)}
MASKED = ("tdx_p_sample_step_x0_masked", "tdx_p_sample_step_x0_guided_masked", "tdx_p_sample_step_ms_masked",
          "tdx_p_sample_step_ms_guided_masked")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t):
    return t.cuda().contiguous()


def _km(kind, n, seed=0, binary=False, known_rows=None):
    """known (n or 1 rows) and a block mask that broadcasts over samples and channels, and the two expanded."""
    shape = SHAPES[kind]
    known = known_data(n if known_rows is None else known_rows, shape, seed)
    mask = block_mask(shape, binary)
    full = (n,) + tuple(shape)
    return known, mask, known.expand(full).contiguous(), mask.expand(full).contiguous()


# ---------------------------------------------------------------- 1. the kernels, bit for bit
def _tables(form):
    fp = ForwardProcess()
    if form == "x0":
        sched = ddim_schedule(fp, steps=10, eta=0.5)
        tab = sched.x0_form(fp, "eps")
        dev = sched.x0_form(fp, "eps", device="cuda")
    else:
        sched = dpm_solver_schedule(fp, steps=10)
        tab = sched.multistep_form(fp, "eps")
        dev = sched.multistep_form(fp, "eps", device="cuda")
        assert tab[0, 4] == 0 and tab[-1, 4] == 0 and (tab[1:-1, 4] != 0).all()
    assert tab.shape == (10, 5)
    return sched, tab, dev


def _draw(shape, row, w, seed):
    """x ~ N(0, 1), an output whose implied x0 is about N(0, 1.5^2) (a guided pair combines to it), noise, a history,
    known data (partly outside the clamp) and a mask of exact 0, exact 1 and fractions."""
    g = torch.Generator().manual_seed(seed)
    p, q = row[0].item(), row[1].item()
    x = torch.randn(shape, generator=g)
    x0 = 1.5 * torch.randn(shape, generator=g)
    out = (x0 - p * x) / q
    z = torch.randn(shape, generator=g)
    hist = 0.5 * torch.randn(shape, generator=g)
    known = 1.5 * torch.randn(shape, generator=g)
    u = torch.rand(shape, generator=g)
    mask = torch.where(u < 0.3, torch.zeros(()), torch.where(u < 0.6, torch.ones(()), torch.rand(shape, generator=g)))
    if w is not None:
        d = torch.randn(shape, generator=g)
        out = torch.cat([out + (1 - w) * d, out - w * d])
    return [t.contiguous() for t in (x, out, z, hist, known, mask)]


def _call_x0m(x, out, z, known, mask, coef, tau, t_idx, lo, hi, philox=0, seed=0, w=None, n=None, xo=None):
    zp = None if z is None else z.data_ptr()
    tp = None if tau is None else tau.data_ptr()
    if w is None:
        return lib.tdx_p_sample_step_x0_masked((x if xo is None else xo).data_ptr(), x.data_ptr(), out.data_ptr(), zp,
                                               known.data_ptr(), mask.data_ptr(), coef.data_ptr(), tp, t_idx.data_ptr(),
                                               x.numel() if n is None else n, lo, hi, philox, seed, None, _stream())
    return lib.tdx_p_sample_step_x0_guided_masked(x.data_ptr(), out.data_ptr(), zp, known.data_ptr(), mask.data_ptr(),
                                                  coef.data_ptr(), tp, t_idx.data_ptr(),
                                                  x.numel() // 2 if n is None else n, w, lo, hi, philox, seed, None,
                                                  _stream())


def _call_msm(x, out, hist, known, mask, coef, t_idx, lo, hi, w=None, n=None, xo=None):
    if w is None:
        return lib.tdx_p_sample_step_ms_masked((x if xo is None else xo).data_ptr(), x.data_ptr(), out.data_ptr(),
                                               hist.data_ptr(), known.data_ptr(), mask.data_ptr(), coef.data_ptr(),
                                               t_idx.data_ptr(), x.numel() if n is None else n, lo, hi, None, _stream())
    return lib.tdx_p_sample_step_ms_guided_masked(x.data_ptr(), out.data_ptr(), hist.data_ptr(), known.data_ptr(),
                                                  mask.data_ptr(), coef.data_ptr(), t_idx.data_ptr(),
                                                  x.numel() // 2 if n is None else n, w, lo, hi, None, _stream())


def _philox_noise(shape, k, tau, seed):
    """The noise the existing scheduled Philox update draws at step k: that update on x = 0, eps = 0, row (1, 0, 1)."""
    zero = torch.zeros(shape, device="cuda")
    got = torch.empty(shape, device="cuda")
    coef3 = torch.tensor([[1.0, 0.0, 1.0]] * 10, device="cuda")
    t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
    check(lib.tdx_p_sample_step_sched_philox(got.data_ptr(), zero.data_ptr(), zero.data_ptr(), coef3.data_ptr(),
                                             tau.data_ptr(), t_idx.data_ptr(), zero.numel(), seed, _stream()))
    return got


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("shape", [(3, 1, 28, 28), (5, 4, 8, 8)], ids=["3x1x28x28", "5x4x8x8"])
def test_x0_masked_kernels_bitwise(shape, guided):
    sched, tab, coef = _tables("x0")
    tau = sched.device_tables("cuda")[0]
    lo, hi, w = -1.0, 1.0, (2.5 if guided else None)
    n = shape[0]
    for k in range(10):      # every row of the table, in place
        x, out, z, _, known, mask = _draw(shape, tab[k], w, seed=10 * k + n)
        want, x0, x0m = cpu_x0_masked_step(x, out, z, known, mask, tab[k], lo, hi, k, w)
        assert (x0 < lo).any() and (x0 > hi).any() and ((x0 > lo) & (x0 < hi)).any()   # the clamp binds on part
        assert (mask == 0).any() and (mask == 1).any() and ((mask > 0) & (mask < 1)).any()
        if k == 0:      # the last step returns the blend: known at m = 1, the clamped prediction at m = 0
            assert torch.equal(want, x0m) and torch.equal(want[mask == 1], known[mask == 1])
            assert want[mask == 0].abs().max() <= 1 and known[mask == 1].abs().max() > 1
        t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
        od, zd, kd, md = _dev(out), _dev(z), _dev(known), _dev(mask)
        keep = [t.clone() for t in (od, zd, kd, md, coef, tau, t_idx)]
        xd = _dev(torch.cat([x, x]) if guided else x)
        check(_call_x0m(xd, od, zd, kd, md, coef, tau, t_idx, lo, hi, w=w))
        assert torch.equal(xd[:n].cpu(), want), (k, (xd[:n].cpu() - want).abs().max().item())
        if guided:
            assert torch.equal(xd[n:], xd[:n])
        else:       # and out of place, x untouched
            xs = _dev(x)
            xo = torch.empty_like(xs)
            check(_call_x0m(xs, od, zd, kd, md, coef, tau, t_idx, lo, hi, xo=xo))
            assert torch.equal(xo.cpu(), want) and torch.equal(xs.cpu(), x)
        for t, saved in zip((od, zd, kd, md, coef, tau, t_idx), keep):    # inputs untouched
            assert torch.equal(t, saved)
        # in-kernel noise = the tensor form fed the noise the existing Philox update draws under this seed
        zp = _philox_noise(shape, k, tau, seed=11)
        assert zp.abs().max() > 0 if k > 0 else not zp.any()
        xa = _dev(torch.cat([x, x]) if guided else x)
        xb = xa.clone()
        check(_call_x0m(xa, od, None, kd, md, coef, tau, t_idx, lo, hi, philox=1, seed=11, w=w))
        check(_call_x0m(xb, od, zp, kd, md, coef, tau, t_idx, lo, hi, w=w))
        assert torch.equal(xa, xb) and torch.isfinite(xa).all()
        if k > 0:
            assert not torch.equal(xa, xd)


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("shape", [(3, 1, 28, 28), (5, 4, 8, 8)], ids=["3x1x28x28", "5x4x8x8"])
def test_ms_masked_kernels_bitwise(shape, guided):
    _, tab, coef = _tables("ms")
    lo, hi, w = -1.0, 1.0, (2.5 if guided else None)
    n = shape[0]
    for k in range(10):
        x, out, _, hist, known, mask = _draw(shape, tab[k], w, seed=20 * k + n)
        h0 = tab[k, 4].item() == 0.0
        if h0:      # H == 0: the history is not read - NaN in it must not reach the result
            hist = torch.full(shape, NAN)
        want, x0, x0m = cpu_ms_masked_step(x, out, hist, known, mask, tab[k], lo, hi, w)
        assert torch.isfinite(want).all() and torch.isfinite(x0m).all()
        assert (x0 < lo).any() and (x0 > hi).any() and ((x0 > lo) & (x0 < hi)).any()
        if k == 0:
            assert torch.equal(want, x0m) and torch.equal(want[mask == 1], known[mask == 1])
        t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
        od, kd, md, hd = _dev(out), _dev(known), _dev(mask), _dev(hist)
        keep = [t.clone() for t in (od, kd, md, coef, t_idx)]
        xd = _dev(torch.cat([x, x]) if guided else x)
        check(_call_msm(xd, od, hd, kd, md, coef, t_idx, lo, hi, w=w))
        assert torch.equal(xd[:n].cpu(), want), (k, (xd[:n].cpu() - want).abs().max().item())
        assert torch.equal(hd.cpu(), x0m)           # the history is overwritten with the blend x0m, not with x0c
        if guided:
            assert torch.equal(xd[n:], xd[:n])
        else:
            xs, h2 = _dev(x), _dev(hist)
            xo = torch.empty_like(xs)
            check(_call_msm(xs, od, h2, kd, md, coef, t_idx, lo, hi, xo=xo))
            assert torch.equal(xo.cpu(), want) and torch.equal(xs.cpu(), x) and torch.equal(h2.cpu(), x0m)
        for t, saved in zip((od, kd, md, coef, t_idx), keep):
            assert torch.equal(t, saved)


# ---------------------------------------------------------------- 2. an all-zero mask is the unmasked entry
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
def test_all_zero_mask_is_the_unmasked_entry(guided):
    shape = (3, 1, 28, 28)
    n, lo, hi, w = shape[0], -1.0, 1.0, (2.5 if guided else None)
    sched, tab, coef = _tables("x0")
    tau = sched.device_tables("cuda")[0]
    _, tabm, coefm = _tables("ms")
    for k in (0, 1, 5, 9):
        t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
        x, out, z, hist, known, _ = _draw(shape, tab[k], w, seed=k + 3)
        zero = torch.zeros(shape, device="cuda")
        x2 = _dev(torch.cat([x, x]) if guided else x)
        od, zd, kd = _dev(out), _dev(z), _dev(known)
        for philox, zz in ((0, zd), (1, None)):
            a, b = x2.clone(), x2.clone()
            check(_call_x0m(a, od, zz, kd, zero, coef, tau, t_idx, lo, hi, philox=philox, seed=5, w=w))
            zp, tp = None if zz is None else zz.data_ptr(), tau.data_ptr()
            if guided:
                check(lib.tdx_p_sample_step_x0_guided(b.data_ptr(), od.data_ptr(), zp, coef.data_ptr(), tp,
                                                      t_idx.data_ptr(), b.numel() // 2, w, lo, hi, philox, 5, None,
                                                      _stream()))
            else:
                check(lib.tdx_p_sample_step_x0(b.data_ptr(), b.data_ptr(), od.data_ptr(), zp, coef.data_ptr(), tp,
                                               t_idx.data_ptr(), b.numel(), lo, hi, philox, 5, None, _stream()))
            assert torch.equal(a, b), (k, philox)
        x, out, _, hist, known, _ = _draw(shape, tabm[k], w, seed=k + 4)
        x2 = _dev(torch.cat([x, x]) if guided else x)
        od, kd = _dev(out), _dev(known)
        a, b, ha, hb = x2.clone(), x2.clone(), _dev(hist), _dev(hist)
        check(_call_msm(a, od, ha, kd, zero, coefm, t_idx, lo, hi, w=w))
        if guided:
            check(lib.tdx_p_sample_step_ms_guided(b.data_ptr(), od.data_ptr(), hb.data_ptr(), coefm.data_ptr(),
                                                  t_idx.data_ptr(), b.numel() // 2, w, lo, hi, None, _stream()))
        else:
            check(lib.tdx_p_sample_step_ms(b.data_ptr(), b.data_ptr(), od.data_ptr(), hb.data_ptr(), coefm.data_ptr(),
                                           t_idx.data_ptr(), b.numel(), lo, hi, None, _stream()))
        assert torch.equal(a, b) and torch.equal(ha, hb), k


# ---------------------------------------------------------------- 3. bad arguments
def test_masked_kernels_bad_arguments():
    _, _, coef = _tables("x0")
    x = torch.zeros(8, device="cuda")
    out = torch.zeros(16, device="cuda")
    hist = torch.zeros(8, device="cuda")
    known = torch.full((8,), 0.5, device="cuda")
    mask = torch.ones(8, device="cuda")
    t_idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = _stream()
    xp, op, hp, knp, mp, cp, kp = (t.data_ptr() for t in (x, out, hist, known, mask, coef, t_idx))
    bounds = ((1.0, -1.0), (0.0, 0.0), (NAN, 1.0), (-1.0, NAN), (INF, INF))
    cases = [   # (entry, good arguments, pointers that must not be null, index of n, index of lo)
        (lib.tdx_p_sample_step_x0_masked, (xp, xp, op, None, knp, mp, cp, None, kp, 8, -1.0, 1.0, 0, 0, None, st),
         (0, 1, 2, 4, 5, 6, 8), 9, 10),
        (lib.tdx_p_sample_step_x0_guided_masked, (xp, op, None, knp, mp, cp, None, kp, 4, 2.0, -1.0, 1.0, 0, 0, None, st),
         (0, 1, 3, 4, 5, 7), 8, 10),
        (lib.tdx_p_sample_step_ms_masked, (xp, xp, op, hp, knp, mp, cp, kp, 8, -1.0, 1.0, None, st),
         (0, 1, 2, 3, 4, 5, 6, 7), 8, 9),
        (lib.tdx_p_sample_step_ms_guided_masked, (xp, op, hp, knp, mp, cp, kp, 4, 2.0, -1.0, 1.0, None, st),
         (0, 1, 2, 3, 4, 5, 6), 7, 9),
    ]
    for fn, ok, ptrs, i_n, i_lo in cases:
        for i in ptrs:      # known and mask among them
            bad = list(ok)
            bad[i] = None
            assert fn(*bad) == TDX_E_BADARG, (fn.__name__, i)
        for n in (0, -4, 6, 7):
            assert fn(*ok[:i_n], n, *ok[i_n + 1:]) == TDX_E_BADARG, (fn.__name__, n)
        for lo, hi in bounds:
            assert fn(*ok[:i_lo], lo, hi, *ok[i_lo + 2:]) == TDX_E_BADARG, (fn.__name__, lo, hi)
    torch.cuda.synchronize()
    assert not x.any() and not hist.any()       # nothing was written
    for fn, ok, _, _, _ in cases:               # and the good arguments are good: mask = 1 on row 0 returns known
        x.zero_(), hist.zero_()
        assert fn(*ok) == 0
        torch.cuda.synchronize()
        filled = x if "guided" not in fn.__name__ else x[:4]
        assert torch.equal(filled, torch.full_like(filled, 0.5)), fn.__name__


# ---------------------------------------------------------------- 4. fused = separate
@pytest.mark.parametrize("form", ["x0", "ms"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,w,n,halves", [("uncond", None, 4, 0), ("cond", 2.0, 4, 0), ("laion", 2.0, 2, 0),
                                             ("uncond", None, 5, 1)],
                         ids=["uncond", "cond-guided", "laion-guided", "uncond-halves"])
def test_masked_fused_update_equals_separate_kernel(kind, w, n, halves, bf16, form):
    """One masked step at a middle row through tdx_unet_eval_step_{x0,ms}_masked with the update in final_conv's epilogue,
    and one with the knob sample_fuse without bit 2 (the plain convolution, then the separate masked kernel): x, the
    history and the network's output bit-identical, and both equal to the CPU restatement on the network's output.
    The launches exercised: the unguided epilogue at C = 1 (uncond), the guided epilogue at C = 1 (cond) and C = 4
    (laion), fp32 and bf16 fat tensors; "uncond-halves" turns the knob sample_halves on, so the n = 5 step runs as two
    half-batch launches of 3 and 2 samples, the second with elem0 = 3 * 784: its epilogue must index known, mask, the
    history and the Philox stream by the element's place in the whole batch (guided steps never run as halves)."""
    S, lo, hi = 3, -1.0, 1.0
    fp = ForwardProcess()
    m = model(kind, 8).eval()
    if bf16:
        m.set_compute_dtype(torch.bfloat16)
    x_T, _, y = inputs(kind, n, 1, seed=2)
    if form == "x0":
        sched = ddim_schedule(fp, timesteps=[100, 400, 800], eta=1.0)
        coef = sched.x0_form(fp, "eps", device="cuda")
        assert coef[1, 4] > 0
    else:
        sched = dpm_solver_schedule(fp, timesteps=[100, 400, 800])
        coef = sched.multistep_form(fp, "eps", device="cuda")
        assert coef[1, 4] < 0
    tau = sched.device_tables("cuda")[0]
    _, _, known, mask = _km(kind, n, seed=3)
    rows = 2 * n if w is not None else n
    y2 = y if w is None else torch.cat([y, null_cond(kind, y)]).contiguous()
    h0 = 0.5 * torch.randn(x_T.shape, generator=torch.Generator().manual_seed(3))
    res = {}
    for fused in (True, False):
        with tuned(sample_halves=halves, sample_fuse=6 if fused else 2):
            x = _dev(torch.cat([x_T, x_T]) if w is not None else x_T)
            hist = _dev(h0) if form == "ms" else None
            kd, md = _dev(known), _dev(mask)
            counter = torch.tensor([1], dtype=torch.int64, device="cuda")
            t_idx = torch.empty(1, dtype=torch.int32, device="cuda")
            t_vec = torch.empty(rows, dtype=torch.int64, device="cuda")
            out = torch.empty_like(x)
            with torch.no_grad():
                m._run_eval_step(x, y2, coef, counter, t_idx, t_vec, out, philox_seed=9, tau=tau, S=S, guidance_scale=w,
                                 clip=(lo, hi), hist=hist, known=kd, mask=md)
            torch.cuda.synchronize()
            assert counter.item() == 0 and t_idx.item() == 1 and int(t_vec[-1]) == 400
            res[fused] = (x.clone(), None if hist is None else hist.clone(), out.clone())
    (xf, hf, of), (xs, hs, os_) = res[True], res[False]
    assert torch.isfinite(xf).all()
    assert torch.equal(of, os_) and torch.equal(xf, xs), rel_mse(xf, xs)
    if w is not None:
        assert torch.equal(xf[:n], xf[n:])
    o = of.cpu()
    if form == "ms":
        assert torch.equal(hf, hs)
        want, x0, x0m = cpu_ms_masked_step(x_T, o, h0, known, mask, coef[1].cpu(), lo, hi, w)
        assert torch.equal(xf[:n].cpu(), want) and torch.equal(hf.cpu(), x0m)
    else:
        zp = _philox_noise(x_T.shape, 1, tau, seed=9).cpu()
        want, x0, x0m = cpu_x0_masked_step(x_T, o, zp, known, mask, coef[1].cpu(), lo, hi, 1, w)
        assert torch.equal(xf[:n].cpu(), want)
    assert (x0.abs() > 1).any() and (x0.abs() < 1).any()       # the step did clamp, and not everywhere


# ---------------------------------------------------------------- 5. chains against fp64
def _check_chain(name, got, want, x_T, w, mode):
    r = rel_mse(got, want)
    print(f"masked {name} {mode}: relative MSE vs fp64 {r:.3e} (bound {CHAIN_TOL * amp(w):.1e})")
    assert got.shape == x_T.shape and torch.isfinite(got).all()
    assert r < CHAIN_TOL * amp(w), (name, mode, r)


DDIM_CHAINS = [("uncond", None, "eps", 4), ("uncond", None, "v", 5), ("cond", 3.0, "eps", 5), ("laion", None, "eps", 4),
               ("latent", None, "eps", 4), ("transformer", None, "v", 4)]
DDPM_CHAINS = [("uncond", None, "eps", 4), ("cond", 3.0, "v", 5), ("laion", None, "eps", 4), ("latent", None, "v", 4),
               ("transformer", None, "eps", 4)]
DPM_CHAINS = [("uncond", None, "eps", 4), ("uncond", None, "v", 5), ("cond", 3.0, "eps", 5), ("laion", None, "v", 4),
              ("latent", None, "eps", 4), ("transformer", None, "eps", 4)]


@pytest.mark.parametrize("kind,w,prediction,n", DDIM_CHAINS)
def test_masked_ddim_chain_against_fp64(kind, w, prediction, n):
    S = 10
    fp = ForwardProcess()
    m = model(kind, 1)
    x_T, _, y = inputs(kind, n, 1, seed=11 + n)
    known, mask, kf, mf = _km(kind, n, seed=n)
    sched = ddim_schedule(fp, steps=S)
    clip = True if prediction == "eps" else None        # with the clamp and without it (infinite bounds)
    lo, hi = (-1.0, 1.0) if clip else (-INF, INF)
    want = inpaint_chain64(fp64_forward(kind, 1), kind, fp, sched, x_T, y, kf, mf, lo, hi, prediction, w)
    for mode, kw in MODES.items():   # eta = 0 draws no noise: the Philox mode is comparable too
        got = sample_loop(m, fp, "cuda", n, y, x_T=x_T, schedule=sched, guidance_scale=w, prediction=prediction,
                          clip_denoised=clip, known=known, mask=mask, **kw)
        _check_chain(f"DDIM eta=0 S={S} {kind} w={w} {prediction} clip={clip}", got, want, x_T, w, mode)


@pytest.mark.parametrize("kind,w,prediction,n", DDPM_CHAINS)
def test_masked_ddpm_chain_against_fp64(kind, w, prediction, n):
    from tiny_diffusion_amd.schedule import ddpm_schedule

    T = 20
    fp = ForwardProcess(num_timesteps=T)
    m = model(kind, 1)
    x_T, zs, y = inputs(kind, n, T, seed=5 + n)
    known, mask, kf, mf = _km(kind, n, seed=n, known_rows=1)      # known broadcasts over the samples too
    clip = None if prediction == "eps" else (-0.75, 0.5)
    lo, hi = clip if clip else (-INF, INF)
    want = inpaint_chain64(fp64_forward(kind, 1), kind, fp, ddpm_schedule(fp), x_T, y, kf, mf, lo, hi, prediction, w,
                           zs)
    for mode in ("eager", "graph"):      # recorded noise (the Philox stream has no fp64 counterpart)
        got = sample_loop(m, fp, "cuda", n, y, x_T=x_T, noises=zs, guidance_scale=w, prediction=prediction,
                          clip_denoised=clip, known=known, mask=mask, **MODES[mode])
        _check_chain(f"DDPM T={T} {kind} w={w} {prediction} clip={clip}", got, want, x_T, w, mode)


@pytest.mark.parametrize("kind,w,prediction,n", DPM_CHAINS)
def test_masked_dpm_chain_against_fp64(kind, w, prediction, n):
    fp = ForwardProcess()
    m = model(kind, 1)
    x_T, _, y = inputs(kind, n, 1, seed=21 + n)
    known, mask, kf, mf = _km(kind, n, seed=n)
    taus = dpm_solver_schedule(fp, steps=10).timesteps.tolist()
    clip = True if prediction == "eps" else None
    lo, hi = (-1.0, 1.0) if clip else (-INF, INF)
    want = inpaint_dpm_chain64(fp64_forward(kind, 1), kind, fp, taus, x_T, y, kf, mf, lo, hi, prediction, w)
    for mode, kw in MODES.items():
        got = dpm_sample_loop(m, fp, "cuda", n, y, steps=10, x_T=x_T, guidance_scale=w, prediction=prediction,
                              clip_denoised=clip, known=known, mask=mask, **kw)
        _check_chain(f"DPM-Solver++(2M) S={len(taus)} {kind} w={w} {prediction} clip={clip}", got, want, x_T, w, mode)


# ---------------------------------------------------------------- 6. graph + Philox = eager Philox
@pytest.mark.parametrize("tables", [0, 1], ids=["tables-off", "tables-on"])
@pytest.mark.parametrize("form", ["x0", "ms"])
@pytest.mark.parametrize("kind,w", [("uncond", None), ("cond", 2.0)], ids=["unguided", "guided"])
def test_masked_philox_graph_equals_eager(kind, w, form, tables):
    """In-kernel noise: the device-counter graphs (one-call masked step, fused epilogue, a tail graph: S = 13) against
    the eager chain (the separate masked kernels), bit for bit, with the sampling tables off and on.

    The table look-up of a conditional UNet adds the time and the class projection in another order than the forward
    does: the UNMASKED guided chain, printed beside the masked one, differs from its eager twin by 5.2e-12 (x0) and
    3.3e-12 (ms) relative MSE with the tables on (the pairing tests/test_gpu_clip.py and tests/test_gpu_dpm.py hold to
    1e-10), and a masked chain that used the tables differed by 3.3e-12 / 2.7e-12.  A masked chain under a condition
    therefore stays on the direct time path (sample_loop: _drop_sampling_tables), whatever the knob says, and the
    equality holds in all eight cases."""
    n, S = 4, 13
    assert S > GRAPH_STEPS and S % GRAPH_STEPS
    fp = ForwardProcess()
    m = model(kind, 4)
    x_T, _, y = inputs(kind, n, 1, seed=S)
    known, mask, _, _ = _km(kind, n, seed=6)
    kw = dict(x_T=x_T, guidance_scale=w, clip_denoised=True, philox_seed=4, known=known, mask=mask)
    if form == "x0":
        sched = ddim_schedule(fp, steps=S, eta=0.5)
        assert float(sched.coef[1:, 2].min()) > 0
    else:
        sched = dpm_solver_schedule(fp, steps=S, spacing="uniform")
        assert sched.steps == S
    pe = sample_loop(m, fp, "cuda", n, y, schedule=sched, **kw)
    with tuned(sample_tables=tables):
        pg = sample_loop(m, fp, "cuda", n, y, schedule=sched, use_graph=True, **kw)
    r = rel_mse(pg, pe)
    print(f"masked graph + Philox vs eager + Philox {kind} w={w} {form} tables={tables} S={S}: relative MSE {r:.3e}")
    if tables:      # the same pairing without known / mask, for the record: what the table mode itself costs
        uk = {k: v for k, v in kw.items() if k not in ("known", "mask")}
        ue = sample_loop(m, fp, "cuda", n, y, schedule=sched, **uk)
        ug = sample_loop(m, fp, "cuda", n, y, schedule=sched, use_graph=True, **uk)
        print(f"unmasked graph + Philox vs eager + Philox {kind} w={w} {form} tables=1 S={S}: relative MSE "
              f"{rel_mse(ug, ue):.3e}")
    assert torch.isfinite(pe).all()
    assert torch.equal(pg, pe), r
    if form == "x0":
        other = sample_loop(m, fp, "cuda", n, y, schedule=sched, use_graph=True, **{**kw, "philox_seed": 5})
        assert rel_mse(other, pe) > 1e-4      # the comparison can tell one noise stream from another


# ---------------------------------------------------------------- 7. the known region is returned exactly
@pytest.mark.parametrize("clip", [None, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("sampler", ["sample", "ddim_sample", "dpm_sample"])
def test_known_region_is_returned_exactly(sampler, clip):
    from tiny_diffusion_amd import diffusion as D

    n = 4
    fp = ForwardProcess(num_timesteps=20) if sampler == "sample" else ForwardProcess()
    m = model("uncond", 3)
    x_T, zs, _ = inputs("uncond", n, 1000, seed=17)
    known, mask, kf, mf = _km("uncond", n, seed=9, binary=True)
    assert set(mask.unique().tolist()) == {0.0, 1.0} and kf[mf == 1].abs().max() > 1
    extra = {"sample": {}, "ddim_sample": dict(steps=7, eta=0.7), "dpm_sample": dict(steps=6)}[sampler]
    free = getattr(D, sampler)(m, fp, "cuda", n_samples=n, x_T=x_T, philox_seed=7, **extra)
    assert free.abs().max() > 1          # the free chain leaves the range
    for mode, kw in MODES.items():
        noise = dict(noises=zs) if ("philox_seed" not in kw and sampler != "dpm_sample") else {}
        got = getattr(D, sampler)(m, fp, "cuda", n_samples=n, x_T=x_T, clip_denoised=clip, known=known, mask=mask,
                                  **extra, **noise, **kw).cpu()
        assert got.shape == x_T.shape and torch.isfinite(got).all()
        assert torch.equal(got[mf == 1], kf[mf == 1]), (sampler, mode)
        assert not torch.equal(got[mf == 0], kf[mf == 0])
        if clip:
            assert got[mf == 0].min() >= -1 and got[mf == 0].max() <= 1, (sampler, mode)


# ---------------------------------------------------------------- 8. known=None is the path as it was
def test_defaults_are_the_path_as_it_was(monkeypatch):
    """The sequence of sampling entries each sampler calls without ``known`` / ``mask``, and the update each call asks
    for (``spy_entries``) - the unmasked one, in every mode, guided or not; ``known=None, mask=None`` is the same call."""
    from tiny_diffusion_amd import _lib
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import diffusion as D

    calls = []
    watched = [nm for nm in _lib.EXPORTS if "p_sample_step" in nm or "p_sample_update" in nm or "eval_step" in nm
               or "step_begin" in nm or "prepare_sampling" in nm or "sampling_tables" in nm]
    assert set(MASKED) | {"tdx_p_sample_update", "tdx_unet_eval_step_update"} <= set(watched)
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
        rec, gph, phx = dict(x_T=x_T, noises=zs), dict(x_T=x_T, noises=zs, use_graph=True), \
            dict(x_T=x_T, use_graph=True, philox_seed=3)
        det, dgph = dict(x_T=x_T), dict(x_T=x_T, use_graph=True)
        expect = [
            # the reference's chain: the eps-form update, one per step; one warm-up + one captured step; tables + the
            # one-call step (one warm-up + GRAPH_STEPS captured, replayed twice)
            ("sample", {}, rec, [up + "eps" + g + "]"] * T),
            ("sample", {}, gph, [up + "eps" + g + "]"] * 2),
            ("sample", {}, phx, ["tdx_unet_prepare_sampling"]
             + [ev + "eps" + g + "]" if g else "tdx_unet_eval_step"] * (1 + GRAPH_STEPS)),
            ("ddim_sample", dict(steps=S, eta=0.4), rec, [up + "eps,sched" + g + "]"] * S),
            ("ddim_sample", dict(steps=S, eta=0.4), gph, [up + "eps,sched" + g + "]"] * 2),
            ("ddim_sample", dict(steps=S, eta=0.4), phx, ["tdx_unet_prepare_sampling_sched"]
             + [ev + "eps,sched" + g + "]"] * (1 + S)),
            ("ddim_sample", dict(steps=S, eta=0.4, clip_denoised=True), rec, [up + "x0,sched" + g + "]"] * S),
            ("ddim_sample", dict(steps=S, eta=0.4, clip_denoised=True), phx, ["tdx_unet_prepare_sampling_sched"]
             + [ev + "x0,sched" + g + "]"] * (1 + S)),
            ("dpm_sample", dict(steps=S), det, [up + "ms,sched" + g + "]"] * Sd),
            ("dpm_sample", dict(steps=S), dgph, [up + "ms,sched" + g + "]"] * 2),
            ("dpm_sample", dict(steps=S), phx, ["tdx_unet_prepare_sampling_sched"]
             + [ev + "ms,sched" + g + "]"] * (1 + Sd)),
        ]
        for sampler, extra, kw, want in expect:
            outs = []
            for none in ({}, dict(known=None, mask=None)):
                calls.clear()
                outs.append(getattr(mod, sampler)(m, fp, "cuda", **cond, **extra, **kw, **none))
                assert calls == want, (kind, sampler, list(kw), calls)
            assert torch.equal(outs[0], outs[1]), (kind, sampler, list(kw))
        # and the spies do see a masked call: the one-call step in graph + Philox mode, the separate kernel otherwise
        known, mask, _, _ = _km(kind, n, seed=1)
        calls.clear()
        mod.ddim_sample(m, fp, "cuda", **cond, steps=3, x_T=x_T, use_graph=True, philox_seed=3, known=known, mask=mask)
        # (under a condition the masked chain leaves the tables aside: the direct time path, the eager chain's bits)
        head = "tdx_unet_prepare_sampling_sched" if kind == "uncond" else "tdx_unet_drop_sampling_tables"
        assert calls == [head] + [ev + "x0,sched" + g + ",masked]"] * 4, calls
        calls.clear()
        mod.dpm_sample(m, fp, "cuda", **cond, steps=S, x_T=x_T, known=known, mask=mask)
        assert calls == [up + "ms,sched" + g + ",masked]"] * Sd, calls
        calls.clear()
        mod.sample(m, fp, "cuda", **cond, x_T=x_T, noises=zs, known=known, mask=mask)
        assert calls == [up + "x0,sched" + g + ",masked]"] * T, calls
        calls.clear()


# ---------------------------------------------------------------- 9. no stale state
@pytest.mark.parametrize("mode", ["philox", "eager"])
@pytest.mark.parametrize("kind,w", [("uncond", None), ("cond", 2.0)])
def test_no_stale_state_between_masked_and_unmasked_calls(kind, w, mode):
    n = 4
    fp = ForwardProcess()
    m = model(kind, 6)
    x_T, _, y = inputs(kind, n, 1, seed=8)
    known, mask, kf, mf = _km(kind, n, seed=2, binary=True)
    kw = dict(x_T=x_T, steps=12, guidance_scale=w, clip_denoised=True, **MODES[mode])   # sampling tables are on
    mk = dict(known=known, mask=mask)
    for loop in (ddim_sample_loop, dpm_sample_loop):
        first = loop(m, fp, "cuda", n, y, **kw, **mk)
        second = loop(m, fp, "cuda", n, y, **kw)
        third = loop(m, fp, "cuda", n, y, **kw, **mk)
        assert torch.equal(third, first)
        assert torch.equal(second, loop(model(kind, 6), fp, "cuda", n, y, **kw))       # what it gives alone
        assert torch.equal(first, loop(model(kind, 6), fp, "cuda", n, y, **kw, **mk))
        assert torch.equal(first.cpu()[mf == 1], kf[mf == 1])
        assert not torch.equal(second.cpu()[mf == 1], kf[mf == 1])
