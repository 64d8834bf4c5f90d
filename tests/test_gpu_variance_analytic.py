"""The analytic (KL-optimal) reverse variance on the device: ``tdx_eps_sqnorm`` per sample against fp64 under its derived
bound (tests/analytic_helpers.py) and against the restatement of its summation order, its independence of the batch,
``estimate_eps_moments`` of every model against its own composition (Philox ``q_sample``, the model's forward, fp64 on
the host), the samplers under ``variance=`` against their explicit schedules, and the bound under an ``EpsMoments`` and
on a sub-trajectory against the fp64 assembly from the kernel's own sums.  Every figure is printed before it is asserted.

The LAION UNet runs at (4, 32, 32): the model refuses a side below 32, so (4, 8, 8) cannot be launched.

The file's name sorts after tests/test_gpu_bench*.py on purpose.  Those tests start ``bench.py`` as child processes and
judge figures of two ranks that share the one GPU (``roofline.frac < 1``); they used to be the first GPU tests of a
session, run while the pytest process itself had not opened the GPU.  With this file in front of them the pytest
process holds a live GPU context, models and workspaces during the children's run, and the two-rank figure came out at
1.16 - 1.22 in three sessions out of three; run on their own the same children give 0.53 - 0.85."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import analytic_helpers as A  # noqa: E402
import vlb_helpers as H  # noqa: E402
from inpaint_helpers import NUM_CLASSES, SHAPES, block_mask, known_data, model  # noqa: E402

from tiny_diffusion_amd._lib import check, lib, tuned  # noqa: E402
from tiny_diffusion_amd.analytic import EpsMoments, estimate_eps_moments, optimal_sigma2  # noqa: E402
from tiny_diffusion_amd.schedule import ForwardProcess, ddim_schedule, ddpm_schedule, sample_loop  # noqa: E402

SENTINEL = -7.0
TDX_E_BADARG = -1
T_SMALL = 6


@functools.lru_cache(maxsize=None)
def _fp(T=1000):
    return ForwardProcess(num_timesteps=T)


@functools.lru_cache(maxsize=None)
def _model(kind):
    return model(kind).eval()


def _module(kind):
    from tiny_diffusion_amd import (conditional_diffusion, conditional_diffusion_laion, diffusion, diffusion_transformer,
                                    latent_diffusion)
    return {"uncond": diffusion, "cond": conditional_diffusion, "laion": conditional_diffusion_laion,
            "latent": latent_diffusion, "transformer": diffusion_transformer}[kind]


def _launch(x_t, out, t, rows, stride=1, into=None):
    """One ``tdx_eps_sqnorm`` launch on device copies of the CPU tensors.  Returns the (B,) buffer it wrote,
    sentinel-filled before; ``into=(buffer, first float)``: writes there instead, ``stride`` floats between samples."""
    B, per = x_t.shape
    dev = [v.cuda().contiguous() for v in (x_t, out, t, rows)]
    sums = torch.full((B,), SENTINEL, device="cuda") if into is None else into[0]
    ptr = sums.data_ptr() + (0 if into is None else 4 * into[1])
    check(lib.tdx_eps_sqnorm(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), B, per, ptr,
                             stride, torch.cuda.current_stream().cuda_stream), "tdx_eps_sqnorm")
    torch.cuda.synchronize()
    return sums.cpu()


# ---------------------------------------------------------------- 1. the kernel, per sample
@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("per", A.SQNORM_PERS)
def test_kernel_against_fp64(per, B, prediction):
    """Distinct per-sample t with 0 and T - 1 among them; eps rows (0, 1) and v rows; stride 1 and 5 with sentinel
    neighbours.  The bound is derived (analytic_helpers); the restatement of the summation order gives the same bits."""
    fp = _fp()
    rows = A.eps_rows32(fp, prediction)
    t = torch.tensor([999] if B == 1 else [500, 0, 999])
    x_t, out = A.sqnorm_inputs(fp, per, t.tolist())
    want, bound = A.sqnorm64(x_t, out, rows, t)
    got = _launch(x_t, out, t, rows)
    err = (got.double() - want).abs()
    print(f"per={per} B={B} {prediction}: got {got.tolist()} want {want.tolist()} |err| / bound {(err / bound).tolist()}")
    assert (err <= bound).all()
    assert torch.equal(got, A.sqnorm32(x_t, out, rows, t))          # the documented order, bit for bit
    buf = _launch(x_t, out, t, rows, stride=5, into=(torch.full((B, 5), SENTINEL, device="cuda"), 2))
    assert torch.equal(buf[:, 2], got) and (buf[:, [0, 1, 3, 4]] == SENTINEL).all()


@pytest.mark.parametrize("per", [20, 784, 4096])
def test_a_sample_has_the_same_bits_alone_and_at_any_row(per):
    fp = _fp()
    rows = A.eps_rows32(fp, "v")
    t = torch.tensor([0, 500, 0])
    x_t, out = A.sqnorm_inputs(fp, per, t.tolist())
    first = _launch(x_t, out, t, rows)
    assert torch.equal(first, _launch(x_t, out, t, rows))
    for b in range(3):
        one = _launch(x_t[b:b + 1], out[b:b + 1], t[b:b + 1], rows)
        assert torch.equal(one[0], first[b]), b
    back = _launch(x_t.flip(0).contiguous(), out.flip(0).contiguous(), t.flip(0).contiguous(), rows)
    assert torch.equal(back.flip(0), first)
    assert not torch.equal(first[0], first[2])      # two samples on the same row differ: the sums are per sample


@pytest.mark.parametrize("bad", A.SQNORM_BAD_ARGS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_entry_rejects_bad_arguments_without_a_launch(bad):
    assert A.sqnorm_call(**bad) == TDX_E_BADARG, bad


# ---------------------------------------------------------------- 2. the estimator against its own composition
def _data(kind, B, seed=0):
    g = torch.Generator().manual_seed(31 + len(kind) + seed)
    shape = SHAPES[kind]
    if kind in ("uncond", "cond"):
        x0 = torch.randint(0, 256, (B, *shape), generator=g).float() * (2.0 / 255.0) - 1.0
    else:
        x0 = torch.randn(B, *shape, generator=g)
    if kind == "uncond":
        y = None
    elif kind == "laion":
        y = torch.randn(B, 768, generator=g).cuda()
    else:
        y = torch.randint(0, NUM_CLASSES, (B,), generator=g).cuda()
    return x0.contiguous(), y


@torch.no_grad()
def _composition(m, fp, x0, y, taus, prediction, seed, repeats=1, chunk=None):
    """(want, bound), fp64 (N repeats, S), per element: the launches of the estimator made by the test - Philox
    q_sample on stream t + r T, the model's forward - and the squared norm in fp64 on the host from the device tensors."""
    rows = A.eps_rows32(fp, prediction)
    N, T, S = x0.shape[0], fp.num_timesteps, len(taus)
    D = x0[0].numel()
    chunk = chunk or N
    want, bound = torch.zeros(N * repeats, S, dtype=torch.float64), torch.zeros(N * repeats, S, dtype=torch.float64)
    for r in range(repeats):
        for start in range(0, N, chunk):
            x = x0[start:start + chunk].cuda()
            n = x.shape[0]
            yc = None if y is None else y[start:start + n]
            for k, t in enumerate(taus):
                tv = torch.full((n,), t, dtype=torch.int64, device="cuda")
                x_t, _ = fp.q_sample_philox(x, tv, seed, t + r * T)
                out = m(x_t, tv) if y is None else m(x_t, tv, yc)
                w, b = A.sqnorm64(x_t.cpu().reshape(n, D), out.cpu().reshape(n, D), rows, tv.cpu())
                want[r * N + start:r * N + start + n, k], bound[r * N + start:r * N + start + n, k] = w, b
    return want / D, bound / D


def _check_moments(mo, want, bound, taus, T, prediction, tag):
    """The mean within the mean of the per-sample bounds; the standard error within ||bound||_2 / sqrt(n (n - 1)) (the
    centred norm is a seminorm: |std(a) - std(b)| <= ||a - b||_2 / sqrt(n - 1))."""
    n = want.shape[0]
    assert isinstance(mo, EpsMoments) and mo.num_timesteps == T and mo.timesteps.tolist() == list(taus)
    assert mo.count == n and mo.prediction == prediction
    assert mo.g.dtype == torch.float64 and mo.g.shape == (len(taus),) and not mo.g.is_cuda
    err, tol = (mo.g - want.mean(0)).abs(), bound.mean(0) + 1e-15 * want.mean(0)
    se = want.std(0, unbiased=True) / math.sqrt(n)
    se_err, se_tol = (mo.stderr - se).abs(), bound.norm(dim=0) / math.sqrt(n * (n - 1)) + 1e-15 * se
    print(f"{tag}: g {mo.g.tolist()} |err| / tol {(err / tol).tolist()} stderr {mo.stderr.tolist()} "
          f"|err| / tol {(se_err / se_tol).tolist()}")
    assert torch.isfinite(mo.g).all() and (mo.g > 0).all() and (err <= tol).all()
    assert (se_err <= se_tol).all()


CASES = [("latent", 8, None, "eps"), ("transformer", 8, None, "eps"), ("uncond", 4, [0, 3, 5], "eps"),
         ("cond", 4, [0, 3, 5], "v"), ("laion", 2, [0, 3, 5], "eps")]


@pytest.mark.parametrize("kind,B,taus,prediction", CASES, ids=[c[0] for c in CASES])
def test_estimate_against_its_own_composition(kind, B, taus, prediction):
    fp, m = _fp(T_SMALL), _model(kind)
    x0, y = _data(kind, B)
    chain = list(range(T_SMALL)) if taus is None else taus
    m.train()
    mo = estimate_eps_moments(m, fp, x0.cuda(), y, timesteps=taus, prediction=prediction, philox_seed=5)
    assert not m.training                       # left in eval mode, as bits_per_dim_loop does
    want, bound = _composition(m, fp, x0, y, chain, prediction, 5)
    _check_moments(mo, want, bound, chain, T_SMALL, prediction, kind)
    again = estimate_eps_moments(m, fp, x0.cuda(), y, timesteps=taus, prediction=prediction, philox_seed=5)
    assert torch.equal(again.g, mo.g) and torch.equal(again.stderr, mo.stderr)
    other = estimate_eps_moments(m, fp, x0.cuda(), y, timesteps=taus, prediction=prediction, philox_seed=6)
    assert not torch.equal(other.g, mo.g)


def test_estimate_repeats_and_chunks():
    """``repeats=2`` draws the second pass from the streams t + T; chunks of ``batch_size`` (8 = 3 + 3 + 2) change
    neither the count nor the timestep columns, and every chunk is the composition of its own launches."""
    fp, m = _fp(T_SMALL), _model("latent")
    x0, y = _data("latent", 8)
    taus = [0, 2, 5]
    one = estimate_eps_moments(m, fp, x0.cuda(), y, timesteps=taus, philox_seed=5)
    two = estimate_eps_moments(m, fp, x0.cuda(), y, timesteps=taus, philox_seed=5, repeats=2)
    want, bound = _composition(m, fp, x0, y, taus, "eps", 5, repeats=2)
    _check_moments(two, want, bound, taus, T_SMALL, "eps", "repeats=2")
    assert two.count == 16 and not torch.equal(two.g, one.g)
    assert not torch.allclose(want[:8], want[8:])                 # the second stream is another noise
    chunked = estimate_eps_moments(m, fp, x0.cuda(), y, timesteps=taus, philox_seed=5, batch_size=3, repeats=2)
    want, bound = _composition(m, fp, x0, y, taus, "eps", 5, repeats=2, chunk=3)
    _check_moments(chunked, want, bound, taus, T_SMALL, "eps", "batch_size=3")
    assert chunked.count == two.count and torch.equal(chunked.timesteps, two.timesteps)
    whole = estimate_eps_moments(m, fp, x0.cuda(), y, timesteps=taus, philox_seed=5, batch_size=64, repeats=2)
    assert torch.equal(whole.g, two.g) and torch.equal(whole.stderr, two.stderr)


# ---------------------------------------------------------------- 3. the samplers
@functools.lru_cache(maxsize=None)
def _estimated(kind):
    """The estimate of the model itself on T = 6, all timesteps."""
    x0, y = _data(kind, 4, seed=1)
    return estimate_eps_moments(_model(kind), _fp(T_SMALL), x0.cuda(), y, philox_seed=2)


def _given():
    """Moments strictly between the two limits at every timestep, so that the chain differs from both fixed choices
    whatever the weights of the test's model give (an estimate g >= 1 is the posterior variance itself)."""
    return EpsMoments(T_SMALL, torch.linspace(0.3, 0.9, T_SMALL, dtype=torch.float64))


def _x_T(kind, n=2):
    return torch.randn(n, *SHAPES[kind], generator=torch.Generator().manual_seed(9))


def test_sample_runs_on_its_explicit_schedule():
    fp, m, mo = _fp(T_SMALL), _model("uncond"), _given()
    D = _module("uncond")
    x_T = _x_T("uncond")
    zs = torch.randn(T_SMALL, 2, 1, 28, 28, generator=torch.Generator().manual_seed(3))
    sched = ddpm_schedule(fp).with_sigma(torch.sqrt(optimal_sigma2(fp, mo, None, 1.0, None)))
    assert torch.equal(sched.coef[:, :2], fp.tables("cpu")[2][:, :2]) and not torch.equal(sched.coef[:, 2], fp.tables("cpu")[2][:, 2])
    got = D.sample(m, fp, "cuda", 2, x_T=x_T, noises=zs, variance=mo)
    assert torch.isfinite(got).all()
    assert torch.equal(got, sample_loop(m, fp, "cuda", 2, None, x_T=x_T, noises=zs, schedule=sched))
    plain = D.sample(m, fp, "cuda", 2, x_T=x_T, noises=zs)
    assert not torch.equal(got, plain)
    assert torch.equal(plain, D.sample(m, fp, "cuda", 2, x_T=x_T, noises=zs, variance=None))
    # the three modes: recorded noise eager = per-step graph; in-kernel noise eager = device counter (on the direct
    # time path, as test_gpu_ddim.py pairs them)
    assert torch.equal(D.sample(m, fp, "cuda", 2, x_T=x_T, noises=zs, variance=mo, use_graph=True), got)
    pe = D.sample(m, fp, "cuda", 2, x_T=x_T, philox_seed=4, variance=mo)
    with tuned(sample_tables=0):
        pg = D.sample(m, fp, "cuda", 2, x_T=x_T, philox_seed=4, variance=mo, use_graph=True)
    assert torch.isfinite(pe).all() and torch.equal(pg, pe) and not torch.equal(pe, got)
    assert torch.equal(pe, sample_loop(m, fp, "cuda", 2, None, x_T=x_T, philox_seed=4, schedule=sched))
    assert not torch.equal(pe, D.sample(m, fp, "cuda", 2, x_T=x_T, philox_seed=4))
    # end to end: the model's own estimate
    est = _estimated("uncond")
    own = ddpm_schedule(fp).with_sigma(torch.sqrt(optimal_sigma2(fp, est, None, 1.0, None)))
    assert torch.equal(D.sample(m, fp, "cuda", 2, x_T=x_T, philox_seed=4, variance=est),
                       sample_loop(m, fp, "cuda", 2, None, x_T=x_T, philox_seed=4, schedule=own))


def test_ddim_sample_runs_on_its_explicit_schedule():
    fp, m, mo = _fp(T_SMALL), _model("uncond"), _given()
    D = _module("uncond")
    x_T = _x_T("uncond")
    base = ddim_schedule(fp, steps=3, eta=1.0)
    assert base.timesteps.tolist() == [0, 2, 4]
    sched = base.with_sigma(torch.sqrt(optimal_sigma2(fp, mo, base.timesteps, 1.0, None)))
    assert (sched.coef[1:, 2] > base.coef[1:, 2]).all()           # above the posterior variance: g < 1
    pe = D.ddim_sample(m, fp, "cuda", 2, steps=3, eta=1.0, x_T=x_T, philox_seed=4, variance=mo)
    assert torch.isfinite(pe).all()
    assert torch.equal(pe, sample_loop(m, fp, "cuda", 2, None, x_T=x_T, philox_seed=4, schedule=sched))
    assert not torch.equal(pe, D.ddim_sample(m, fp, "cuda", 2, steps=3, eta=1.0, x_T=x_T, philox_seed=4))
    with tuned(sample_tables=0):
        pg = D.ddim_sample(m, fp, "cuda", 2, steps=3, eta=1.0, x_T=x_T, philox_seed=4, variance=mo, use_graph=True)
    assert torch.equal(pg, pe)
    zs = torch.randn(T_SMALL, 2, 1, 28, 28, generator=torch.Generator().manual_seed(3))
    eager = D.ddim_sample(m, fp, "cuda", 2, steps=3, eta=1.0, x_T=x_T, noises=zs, variance=mo)
    assert torch.equal(eager, D.ddim_sample(m, fp, "cuda", 2, steps=3, eta=1.0, x_T=x_T, noises=zs, variance=mo, use_graph=True))
    assert torch.equal(eager, sample_loop(m, fp, "cuda", 2, None, x_T=x_T, noises=zs, schedule=sched))
    # clipped: the x0 form carries the table (capped for data in the clamp's range), the samples lie inside the range
    capped = base.with_sigma(torch.sqrt(optimal_sigma2(fp, mo, base.timesteps, 1.0, (-1.0, 1.0))))
    clipped = D.ddim_sample(m, fp, "cuda", 2, steps=3, eta=1.0, x_T=x_T, philox_seed=4, variance=mo, clip_denoised=True)
    assert clipped.min().item() >= -1.0 and clipped.max().item() <= 1.0
    assert torch.equal(clipped, sample_loop(m, fp, "cuda", 2, None, x_T=x_T, philox_seed=4, schedule=capped, clip_denoised=True))
    # masked: runs, and returns the known region exactly
    known, mask = known_data(2, SHAPES["uncond"]), block_mask(SHAPES["uncond"], binary=True)
    masked = D.ddim_sample(m, fp, "cuda", 2, steps=3, eta=1.0, x_T=x_T, philox_seed=4, variance=mo, known=known, mask=mask)
    keep = mask.expand_as(known) == 1
    assert torch.isfinite(masked).all() and torch.equal(masked.cpu()[keep], known[keep])


def test_guided_and_v_chains_run():
    fp, m = _fp(T_SMALL), _model("cond")
    C = _module("cond")
    x0, y = _data("cond", 2, seed=2)
    mo = estimate_eps_moments(m, fp, x0.cuda(), y, philox_seed=2)
    x_T = _x_T("cond")
    guided = C.sample(m, fp, "cuda", 2, y=y, guidance_scale=2.0, x_T=x_T, philox_seed=4, variance=mo)
    assert guided.shape == (2, 1, 28, 28) and torch.isfinite(guided).all()
    assert not torch.equal(guided, C.sample(m, fp, "cuda", 2, y=y, guidance_scale=2.0, x_T=x_T, philox_seed=4))
    mv = EpsMoments(T_SMALL, mo.g, prediction="v")
    sched = ddpm_schedule(fp).with_sigma(torch.sqrt(optimal_sigma2(fp, mv, None, 1.0, None)))
    v = C.sample(m, fp, "cuda", 2, y=y, x_T=x_T, philox_seed=4, variance=mv, prediction="v")
    assert torch.isfinite(v).all()
    assert torch.equal(v, sample_loop(m, fp, "cuda", 2, y, x_T=x_T, philox_seed=4, schedule=sched, prediction="v"))


# ---------------------------------------------------------------- 4. the likelihood
def _bound_tol(vb):
    """The kernel's own sums go in, so what test_gpu_vlb.py allows for the sums (SUM_TOL, the decoder's distance) is
    zero here and its 1e-12 relative of the fp64 host formulas is left - taken of the largest term of the sample too,
    since the continuous decoder row is a difference of two terms."""
    return 1e-12 * vb.abs() + 1e-12 * vb.abs().max(dim=1, keepdim=True).values


@pytest.mark.parametrize("kind", ["latent", "uncond"])
def test_bound_under_the_analytic_variance_and_on_a_sub_trajectory(kind):
    fp, m, mod = _fp(T_SMALL), _model(kind), _module(kind)
    x0, y = _data(kind, 2, seed=3)
    mo = _estimated(kind)
    bins = 256 if kind == "uncond" else None
    cap = (-1.0, 1.0) if bins else None          # the data-range cap applies where the data is declared discretised
    cond = {} if y is None else {"y": y}
    D = x0[0].numel()
    sq = (x0.double().reshape(2, -1) ** 2).sum(1)
    plain = mod.bits_per_dim(m, fp, x0.cuda(), philox_seed=3, **cond)
    sub = [0, 2, 5]
    for name, variance in (("beta", "beta"), ("posterior", "posterior"), ("analytic", mo)):
        for taus in (list(range(T_SMALL)), sub):
            kw = {} if len(taus) == T_SMALL else {"timesteps": taus}
            got = mod.bits_per_dim(m, fp, x0.cuda(), philox_seed=3, variance=variance, **cond, **kw)
            S = len(taus)
            g = None if name != "analytic" else mo.at(taus)
            tab = A.sub_tables64(fp, taus, "eps", name, g, cap)
            total, prior, vb = A.assemble_bound(fp, tab, got, x0, bins)
            for f in (got.vb, got.mse, got.xstart_mse):
                assert f.shape == (2, S) and f.dtype == torch.float64 and not f.is_cuda
            err, tol = (got.vb - vb).abs(), _bound_tol(vb)
            tol_prior = H.SUM_TOL * tab["acp_last"] * sq / (2 * D * H.LN2) + 1e-12 * prior.abs()
            print(f"{kind} {name} {taus}: total {got.total_bpd.tolist()} vb |err| / tol {(err / tol).max().item():.3f} "
                  f"prior |err| / tol {((got.prior_bpd - prior).abs() / tol_prior).max().item():.3f}")
            assert torch.isfinite(got.total_bpd).all() and (err <= tol).all()
            assert ((got.prior_bpd - prior).abs() <= tol_prior).all()
            assert ((got.total_bpd - total).abs() <= tol.sum(1) + tol_prior).all()
            assert torch.equal(got.total_bpd, got.prior_bpd + got.vb.sum(dim=1))
            # the chain ran at its own timesteps on their own noise: the columns of the full grid's sums, bit for bit
            idx = torch.tensor(taus)
            assert torch.equal(got.mse, plain.mse[:, idx]) and torch.equal(got.xstart_mse, plain.xstart_mse[:, idx])
            if name == "analytic":
                assert (tab["kc"] >= -1e-15).all() and not torch.equal(got.vb[:, 1:], plain.vb[:, idx][:, 1:])
    for variance in ("beta", mo):
        a = mod.bits_per_dim(m, fp, x0.cuda(), philox_seed=3, variance=variance, **cond)
        b = mod.bits_per_dim(m, fp, x0.cuda(), philox_seed=3, variance=variance, timesteps=range(T_SMALL), **cond)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    for u, v in zip(plain, mod.bits_per_dim(m, fp, x0.cuda(), philox_seed=3, variance="beta", **cond)):
        assert torch.equal(u, v)
