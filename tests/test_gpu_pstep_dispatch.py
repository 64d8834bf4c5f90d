"""The one reverse-step update behind ``tdx_p_sample_update`` / ``tdx_unet_eval_step_update``:

1. every instantiation of the elementwise kernel on its grid-stride path (more float4 than one pass of the 2048 x 256
   grid covers, plus a tail), in place, bit for bit against the CPU fp32 restatements of the step;
2. every ``tdx_p_sample_step*`` entry against ``tdx_p_sample_update`` with the corresponding fields, bit for bit, at
   the smallest length with a tail, the counter decrement included;
3. the argument rules of the two entries: TDX_E_BADARG and nothing written."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from inpaint_helpers import (cfg32, cpu_ms_masked_step, cpu_ms_step, cpu_x0_masked_step, cpu_x0_step,  # noqa: E402
                             model)

from tiny_diffusion_amd._lib import STEP_EPS, STEP_MS, STEP_X0, check, lib  # noqa: E402
from tiny_diffusion_amd.schedule import ForwardProcess, ddim_schedule, dpm_solver_schedule  # noqa: E402

INF, NAN = float("inf"), float("nan")
TDX_E_BADARG = -1
N_BIG = 4 * (2048 * 256 + 3)    # floats per half: one pass of the 2048 x 256 grid and a second, ragged one
N_TAIL = 4 * (256 + 1)          # one full workgroup and one thread of a second
LO, HI, W, SEED = -1.0, 1.0, 2.5, 11
K = {STEP_EPS: 500, STEP_X0: 5, STEP_MS: 5}    # a row with k > 0; for MS one with H != 0
CASES = [(STEP_EPS, g, False) for g in (False, True)] + \
        [(f, g, m) for f in (STEP_X0, STEP_MS) for g in (False, True) for m in (False, True)]
IDS = [f"{'eps x0 ms'.split()[f]}{'-guided' if g else ''}{'-masked' if m else ''}" for f, g, m in CASES]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def _tables(form):
    """(CPU table, device table, device tau): the identity chain's (T,3) table, a DDIM (eta = 0.5) x0 form, a
    DPM-Solver++(2M) multistep form."""
    fp = ForwardProcess()
    if form == STEP_EPS:
        return fp.tables("cpu")[2], fp.tables("cuda")[2], torch.arange(fp.num_timesteps, device="cuda")
    if form == STEP_X0:
        sched = ddim_schedule(fp, steps=10, eta=0.5)
        return sched.x0_form(fp, "eps"), sched.x0_form(fp, "eps", device="cuda"), sched.device_tables("cuda")[0]
    sched = dpm_solver_schedule(fp, steps=10)
    tab = sched.multistep_form(fp, "eps")
    assert tab[K[STEP_MS], 4] != 0
    return tab, sched.multistep_form(fp, "eps", device="cuda"), None


def _draw(n, row, w, seed):
    """As test_gpu_inpaint.py draws: x ~ N(0, 1), an output whose implied x0 is about N(0, 1.5^2) (a guided pair
    combines to it; no row: an eps-form output ~ N(0, 1)), noise, a history, known data (partly outside the clamp) and a
    mask of exact 0, exact 1 and fractions."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    x0 = 1.5 * torch.randn(n, generator=g)
    out = x0 if row is None else (x0 - row[0].item() * x) / row[1].item()
    z = torch.randn(n, generator=g)
    hist = 0.5 * torch.randn(n, generator=g)
    known = 1.5 * torch.randn(n, generator=g)
    u = torch.rand(n, generator=g)
    mask = torch.where(u < 0.3, torch.zeros(()), torch.where(u < 0.6, torch.ones(()), torch.rand(n, generator=g)))
    if w is not None:
        d = torch.randn(n, generator=g)
        out = torch.cat([out + (1 - w) * d, out - w * d])
    return [t.contiguous() for t in (x, out, z, hist, known, mask)]


def _cpu_step(form, guided, masked, x, out, zh, known, mask, row, k):
    """(x', the value the kernel stores as history or None) from the suite's fp32 restatements."""
    w = W if guided else None
    if form == STEP_EPS:
        e = cfg32(out[:x.shape[0]], out[x.shape[0]:], W) if guided else out
        return R.p_sample_step(R.Schedule(), x, e, k, zh), None
    if form == STEP_X0:
        if masked:
            want, x0, _ = cpu_x0_masked_step(x, out, zh, known, mask, row, LO, HI, k, w)
        else:
            want, x0 = cpu_x0_step(x, out, zh, row, LO, HI, k, w)
        stored = None
    else:
        e = cfg32(out[:x.shape[0]], out[x.shape[0]:], W) if guided else out
        if masked:
            want, x0, stored = cpu_ms_masked_step(x, e, zh, known, mask, row, LO, HI)
        else:
            want, stored, x0 = cpu_ms_step(x, e, zh, row, LO, HI)
    assert (x0 < LO).any() and (x0 > HI).any() and ((x0 > LO) & (x0 < HI)).any()   # the clamp binds on part of the data
    return want, stored


def _update(x, out, n, form, coef, t_idx, tau=None, z=None, philox=0, seed=0, guided=False, w=0.0, lo=0.0, hi=0.0,
            hist=None, known=None, mask=None, counter=None, xo=None):
    return lib.tdx_p_sample_update(_ptr(x if xo is None else xo), _ptr(x), _ptr(out), n, form, _ptr(coef), _ptr(t_idx),
                                   _ptr(tau), _ptr(z), philox, seed, int(guided), w, lo, hi, _ptr(hist), _ptr(known),
                                   _ptr(mask), _ptr(counter), _stream())


@functools.lru_cache(maxsize=None)
def _philox_noise(n, k, form, seed):
    """The noise the scheduled Philox update draws at step k: that update on x = 0, eps = 0, row (1, 0, 1)."""
    tau = _tables(form)[2]
    zero = torch.zeros(n, device="cuda")
    got = torch.empty(n, device="cuda")
    coef3 = torch.tensor([[1.0, 0.0, 1.0]] * tau.numel(), device="cuda")
    t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
    check(lib.tdx_p_sample_step_sched_philox(got.data_ptr(), zero.data_ptr(), zero.data_ptr(), coef3.data_ptr(),
                                             tau.data_ptr(), t_idx.data_ptr(), n, seed, _stream()))
    assert got.abs().max() > 0
    return got


# ---------------------------------------------------------------- 1. the grid-stride path of every instantiation
@pytest.mark.parametrize("form,guided,masked", CASES, ids=IDS)
def test_grid_stride_path_bitwise(form, guided, masked):
    tab, coef, tau = _tables(form)
    k, n = K[form], N_BIG
    x, out, z, hist, known, mask = _draw(n, None if form == STEP_EPS else tab[k], W if guided else None, seed=form)
    if masked:
        assert (mask == 0).any() and (mask == 1).any() and ((mask > 0) & (mask < 1)).any()
    want, stored = _cpu_step(form, guided, masked, x, out, hist if form == STEP_MS else z, known, mask, tab[k], k)
    t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
    od = out.cuda()
    kd, md = (known.cuda(), mask.cuda()) if masked else (None, None)
    kw = dict(guided=guided, w=W, lo=LO, hi=HI, known=kd, mask=md)
    xd = (torch.cat([x, x]) if guided else x).cuda()
    if form == STEP_MS:     # one value of PHILOX only
        hd = hist.cuda()
        check(_update(xd, od, n, form, coef, t_idx, hist=hd, **kw))
        assert torch.equal(hd.cpu(), stored)
    else:
        check(_update(xd, od, n, form, coef, t_idx, tau=tau, z=z.cuda(), **kw))
    assert torch.equal(xd[:n].cpu(), want), (xd[:n].cpu() - want).abs().max().item()
    if guided:
        assert torch.equal(xd[n:], xd[:n])
    if form != STEP_MS:     # the PHILOX instantiation = the z instantiation fed the noise Philox draws under this seed
        xa = (torch.cat([x, x]) if guided else x).cuda()
        xb = xa.clone()
        check(_update(xa, od, n, form, coef, t_idx, tau=tau, philox=1, seed=SEED, **kw))
        check(_update(xb, od, n, form, coef, t_idx, tau=tau, z=_philox_noise(n, k, form, SEED), **kw))
        assert torch.equal(xa, xb) and torch.isfinite(xa).all() and not torch.equal(xa, xd)
        if guided:
            assert torch.equal(xa[n:], xa[:n])


# ---------------------------------------------------------------- 2. the entries of each form = the one entry
def _legacy_cases():
    """(entry, form, guided, masked, takes z, takes Philox arguments, takes tau, takes counter_dec, call)."""
    L = lib
    return [
        ("tdx_p_sample_step", STEP_EPS, 0, 0, 1, 0, 0, 0,
         lambda b: L.tdx_p_sample_step(b.x, b.x, b.o, b.z, b.c, b.k, b.n, b.st)),
        ("tdx_p_sample_step_philox", STEP_EPS, 0, 0, 0, 1, 0, 0,
         lambda b: L.tdx_p_sample_step_philox(b.x, b.x, b.o, b.c, b.k, b.n, SEED, b.st)),
        ("tdx_p_sample_step_sched", STEP_EPS, 0, 0, 1, 0, 1, 0,
         lambda b: L.tdx_p_sample_step_sched(b.x, b.x, b.o, b.z, b.c, b.tau, b.k, b.n, b.st)),
        ("tdx_p_sample_step_sched_philox", STEP_EPS, 0, 0, 0, 1, 1, 0,
         lambda b: L.tdx_p_sample_step_sched_philox(b.x, b.x, b.o, b.c, b.tau, b.k, b.n, SEED, b.st)),
        ("tdx_p_sample_step_guided", STEP_EPS, 1, 0, 1, 1, 1, 1,
         lambda b: L.tdx_p_sample_step_guided(b.x, b.o, b.z, b.c, b.tau, b.k, b.n, W, b.ph, SEED, b.cd, b.st)),
        ("tdx_p_sample_step_x0", STEP_X0, 0, 0, 1, 1, 1, 1,
         lambda b: L.tdx_p_sample_step_x0(b.x, b.x, b.o, b.z, b.c, b.tau, b.k, b.n, LO, HI, b.ph, SEED, b.cd, b.st)),
        ("tdx_p_sample_step_x0_guided", STEP_X0, 1, 0, 1, 1, 1, 1,
         lambda b: L.tdx_p_sample_step_x0_guided(b.x, b.o, b.z, b.c, b.tau, b.k, b.n, W, LO, HI, b.ph, SEED, b.cd, b.st)),
        ("tdx_p_sample_step_ms", STEP_MS, 0, 0, 0, 0, 0, 1,
         lambda b: L.tdx_p_sample_step_ms(b.x, b.x, b.o, b.h, b.c, b.k, b.n, LO, HI, b.cd, b.st)),
        ("tdx_p_sample_step_ms_guided", STEP_MS, 1, 0, 0, 0, 0, 1,
         lambda b: L.tdx_p_sample_step_ms_guided(b.x, b.o, b.h, b.c, b.k, b.n, W, LO, HI, b.cd, b.st)),
        ("tdx_p_sample_step_x0_masked", STEP_X0, 0, 1, 1, 1, 1, 1,
         lambda b: L.tdx_p_sample_step_x0_masked(b.x, b.x, b.o, b.z, b.kn, b.m, b.c, b.tau, b.k, b.n, LO, HI, b.ph,
                                                 SEED, b.cd, b.st)),
        ("tdx_p_sample_step_x0_guided_masked", STEP_X0, 1, 1, 1, 1, 1, 1,
         lambda b: L.tdx_p_sample_step_x0_guided_masked(b.x, b.o, b.z, b.kn, b.m, b.c, b.tau, b.k, b.n, W, LO, HI,
                                                        b.ph, SEED, b.cd, b.st)),
        ("tdx_p_sample_step_ms_masked", STEP_MS, 0, 1, 0, 0, 0, 1,
         lambda b: L.tdx_p_sample_step_ms_masked(b.x, b.x, b.o, b.h, b.kn, b.m, b.c, b.k, b.n, LO, HI, b.cd, b.st)),
        ("tdx_p_sample_step_ms_guided_masked", STEP_MS, 1, 1, 0, 0, 0, 1,
         lambda b: L.tdx_p_sample_step_ms_guided_masked(b.x, b.o, b.h, b.kn, b.m, b.c, b.k, b.n, W, LO, HI, b.cd,
                                                        b.st)),
    ]


class _Args:
    pass


@pytest.mark.parametrize("case", _legacy_cases(), ids=lambda c: c[0])
def test_every_entry_equals_the_one_entry(case):
    name, form, guided, masked, has_z, has_philox, has_tau, has_cd, call = case
    tab, coef, tau = _tables(form)
    k, n = K[form], N_TAIL
    x, out, z, hist, known, mask = _draw(n, None if form == STEP_EPS else tab[k], W if guided else None, seed=7 + form)
    t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
    x2, od, zd, kd, md = ((torch.cat([x, x]) if guided else x).cuda(), out.cuda(), z.cuda(), known.cuda(), mask.cuda())
    philox_runs = (1,) if not has_z else (0, 1) if has_philox else (0,)
    for philox in philox_runs if form != STEP_MS else (0,):
        for with_counter in (False, True) if has_cd else (False,):
            xa, xb, ha, hb = x2.clone(), x2.clone(), hist.cuda(), hist.cuda()
            ca, cb = (torch.full((1,), 99, dtype=torch.int64, device="cuda") for _ in range(2))
            b = _Args()
            b.x, b.o, b.c, b.k, b.n, b.st = xa.data_ptr(), od.data_ptr(), coef.data_ptr(), t_idx.data_ptr(), n, _stream()
            b.z = zd.data_ptr() if has_z and not philox else None
            b.tau = tau.data_ptr() if has_tau else None
            b.h, b.kn, b.m, b.ph = ha.data_ptr(), kd.data_ptr(), md.data_ptr(), philox
            b.cd = ca.data_ptr() if with_counter else None
            check(call(b), name)
            check(_update(xb, od, n, form, coef, t_idx, tau=tau if has_tau else None,
                          z=zd if has_z and not philox else None, philox=philox, seed=SEED, guided=bool(guided), w=W,
                          lo=LO, hi=HI, hist=hb if form == STEP_MS else None, known=kd if masked else None,
                          mask=md if masked else None, counter=cb if with_counter else None), "tdx_p_sample_update")
            assert torch.equal(xa, xb) and not torch.equal(xa, x2), (name, philox, with_counter)
            assert torch.equal(ha, hb) and (form == STEP_MS) != torch.equal(ha.cpu(), hist)
            want_counter = k - 1 if with_counter else 99
            assert ca.item() == want_counter and cb.item() == want_counter, (name, ca.item(), cb.item())


# ---------------------------------------------------------------- 3. argument rules of the two new entries
BOUNDS = ((1.0, -1.0), (0.0, 0.0), (NAN, 1.0), (-1.0, NAN), (INF, INF))    # test_masked_kernels_bad_arguments' pairs


def _bad_cases(base, required):
    """(why, arguments) for every rule; ``base[form]`` are good keyword arguments of that form."""
    eps, x0, ms = base[STEP_EPS], base[STEP_X0], base[STEP_MS]
    cases = [(f"form {f}", dict(x0, form=f)) for f in (-1, 3, 7)]
    cases += [("ms with z", dict(ms, z=x0["z"])), ("ms without hist", dict(ms, hist=None))]
    cases += [("known without mask", dict(f, mask=None)) for f in (x0, ms)]
    cases += [("mask without known", dict(f, known=None)) for f in (x0, ms)]
    cases += [("known / mask with eps", dict(eps, known=x0["known"], mask=x0["mask"]))]
    cases += [(f"bounds {b} form {f['form']}", dict(f, lo=b[0], hi=b[1])) for b in BOUNDS for f in (x0, ms)]
    cases += [(f"n {n} form {f['form']}", dict(f, n=n)) for n in (0, -4, 6, 7) for f in (eps, x0, ms)]
    cases += [(f"null {name} form {f['form']}", dict(f, **{name: None})) for name in required for f in (eps, x0, ms)]
    return cases


def _base(n):
    known = torch.full((n,), 0.5, device="cuda")
    mask = torch.ones(n, device="cuda")
    z = torch.ones(n, device="cuda")
    hist = torch.zeros(n, device="cuda")
    base = {}
    for form in (STEP_EPS, STEP_X0, STEP_MS):
        _, coef, tau = _tables(form)
        base[form] = dict(form=form, coef=coef, tau=tau, z=None if form == STEP_MS else z, lo=LO, hi=HI,
                          hist=hist if form == STEP_MS else None, known=None if form == STEP_EPS else known,
                          mask=None if form == STEP_EPS else mask, n=n)
    return base, hist


def test_update_entry_bad_arguments():
    n = 8
    x = torch.zeros(n, device="cuda")
    out = torch.zeros(n, device="cuda")
    t_idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    base, hist = _base(n)
    for f in base.values():
        f.update(x=x, out=out, t_idx=t_idx, xo=x)

    def call(a):
        return lib.tdx_p_sample_update(_ptr(a["xo"]), _ptr(a["x"]), _ptr(a["out"]), a["n"], a["form"], _ptr(a["coef"]),
                                       _ptr(a["t_idx"]), _ptr(a["tau"]), _ptr(a["z"]), 0, 0, 0, 0.0, a["lo"], a["hi"],
                                       _ptr(a["hist"]), _ptr(a["known"]), _ptr(a["mask"]), None, _stream())

    for why, a in _bad_cases(base, ("xo", "x", "out", "coef", "t_idx")):
        assert call(a) == TDX_E_BADARG, why
    torch.cuda.synchronize()
    assert not x.any() and not hist.any()       # nothing was written
    for form, a in base.items():                # and the good arguments are good: on row 0 mask = 1 returns known
        x.zero_()
        assert call(a) == 0, form
        if form != STEP_EPS:
            assert torch.equal(x, torch.full_like(x, 0.5)), form


def test_eval_step_update_entry_bad_arguments():
    m = model("uncond").eval()
    x = torch.zeros(2, 1, 28, 28, device="cuda")
    n = x.numel()
    eps = torch.zeros_like(x)
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    t_idx = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    t_vec = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    plan, pptr, bptr, st = m._plan_ptrs(x)
    base, hist = _base(n)
    for f in base.values():
        f.update(u=plan.handle, x=x, counter=counter, t_idx=t_idx, t_vec=t_vec, eps=eps, S=0 if f["tau"] is None else f["tau"].numel())

    def call(a):
        u = a["u"]
        return lib.tdx_unet_eval_step_update(u, pptr, bptr, _ptr(a["x"]), None, _ptr(a["z"]), _ptr(a["coef"]),
                                             _ptr(a["tau"]), a["S"], _ptr(a["counter"]), _ptr(a["t_idx"]),
                                             _ptr(a["t_vec"]), _ptr(a["eps"]), a["n"], plan.workspace.data_ptr(),
                                             plan.ws_bytes, 2, 0, a["form"], 0, 0.0, a["lo"], a["hi"], _ptr(a["hist"]),
                                             _ptr(a["known"]), _ptr(a["mask"]), st)

    for why, a in _bad_cases(base, ("u", "x", "coef", "counter", "t_idx", "t_vec", "eps")):
        assert call(a) == TDX_E_BADARG, why
    assert call(dict(base[STEP_X0], S=0)) == TDX_E_BADARG       # a schedule needs its length
    torch.cuda.synchronize()
    assert not x.any() and not eps.any() and not hist.any()     # nothing was written, the head did not run
    assert counter.item() == 0 and t_idx.item() == 77 and (t_vec == 77).all()
    for form, a in base.items():                # and the good arguments are good: on row 0 mask = 1 returns known
        x.zero_(), counter.zero_()
        assert call(a) == 0, form
        assert counter.item() == -1 and t_idx.item() == 0
        if form != STEP_EPS:
            assert torch.equal(x, torch.full_like(x, 0.5)), form
