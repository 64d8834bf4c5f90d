"""The analytic (KL-optimal) reverse variance, host side (no GPU): ``optimal_sigma2`` against the closed forms for
Gaussian data (tests/analytic_helpers.py), its two limits and bounds, the tables of the bound under an ``EpsMoments`` and
on a sub-trajectory against first principles, ``TimestepSchedule.with_sigma``, the new C entry, the fp32 restatement of
the kernel against its derived bound, and every argument error before any GPU call, in every module.

Row 0 of a chain adds no noise in any sampler; its variance is a convention: the floor is the posterior variance of
row 1 (as under ``variance="posterior"``) and the model's excess r_0^2 (1 - g_0) is added to it.  The closed forms for
Gaussian data are therefore asserted for the rows k >= 1 and, for row 0, with that floor added."""
import math
import os
import re

import pytest
import torch

import analytic_helpers as A
import vlb_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDX_E_BADARG = -1
RTOL = 1e-10       # two orders over the cancellation measured in fp64 (6e-13)
SPARSE = [0, 99, 499, 999]


def _fp(T=1000):
    from tiny_diffusion_amd.schedule import ForwardProcess

    return ForwardProcess(num_timesteps=T)


def _moments(T, g, taus=None, prediction="eps"):
    from tiny_diffusion_amd.analytic import EpsMoments

    return EpsMoments(T, g, timesteps=taus, prediction=prediction)


def _close(got, want, rtol=RTOL):
    assert got.dtype == torch.float64 and got.shape == want.shape
    if want.numel() == 0:
        return 0.0
    rel = ((got - want).abs() / want.abs()).max().item()
    assert rel <= rtol, rel
    return rel


GRIDS = [(6, None), (6, [0, 2, 5]), (1000, None), (1000, SPARSE)]


# ------------------------------------------------------------------ 1. Gaussian data: the closed forms
@pytest.mark.parametrize("s2", [0.09, 0.25, 1.0])
@pytest.mark.parametrize("T,taus", GRIDS, ids=lambda v: "full" if v is None else str(v))
def test_gaussian_data_gives_the_true_conditional_variance(T, taus, s2):
    """eta = 1: sigma*2_k is Var(x_{tau_{k-1}} | x_{tau_k}) of the Gaussian model; at s2 = 1 that is beta_k."""
    from tiny_diffusion_amd.analytic import optimal_sigma2

    fp = _fp(T)
    chain = A.full(fp) if taus is None else taus
    m = _moments(T, A.gaussian_g(fp, chain, s2), chain)
    for data_range in ((-1, 1), None):       # the cap of [-1, 1] does not bind for s2 <= 1
        got = optimal_sigma2(fp, m, taus, 1.0, data_range)
        rel = _close(got[1:], A.gaussian_true_var(fp, chain, s2)[1:])
    print(f"T={T} {taus} s2={s2}: worst relative difference {rel:.1e}")
    ab, abp = A.ab_columns(fp, chain)
    row0 = A.floor0(fp, chain) + s2 * (1 - ab[0]) / (ab[0] * s2 + 1 - ab[0])      # floor + Var(x_0 | x_tau_0)
    assert abs(got[0].item() - row0.item()) <= RTOL * row0.item()
    if s2 == 1.0:
        _close(got[1:], (1 - ab / abp)[1:])


@pytest.mark.parametrize("eta", [1.0, 0.3])
@pytest.mark.parametrize("s2", [0.09, 0.25, 1.0])
@pytest.mark.parametrize("T,taus", GRIDS, ids=lambda v: "full" if v is None else str(v))
def test_gaussian_data_any_eta(T, taus, s2, eta):
    """sigma*2_k = lam2_k + u_k^2 s2 (1 - ab) / v, and the estimate itself is g = (1 - ab) / v."""
    from tiny_diffusion_amd.analytic import optimal_sigma2

    fp = _fp(T)
    chain = A.full(fp) if taus is None else taus
    g = A.gaussian_g(fp, chain, s2)
    ab, _ = A.ab_columns(fp, chain)
    got = optimal_sigma2(fp, _moments(T, g, chain), taus, eta)
    want = A.gaussian_any_eta(fp, chain, s2, eta)
    _close(got[1:], want[1:])
    lam2, _, u = A.lam2_r_u(fp, chain, eta)
    row0 = A.floor0(fp, chain) + (want[0] - lam2[0]).item()
    assert abs(got[0].item() - row0) <= RTOL * row0
    _close(got, A.sigma2_star(fp, chain, g, eta))          # the row-by-row restatement, row 0 included


# ------------------------------------------------------------------ 2. the two limits
@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("T", [6, 1000])
def test_g_one_reproduces_the_posterior_tables(T, prediction):
    from tiny_diffusion_amd.likelihood import vlb_tables

    fp = _fp(T)
    m = _moments(T, torch.ones(T), prediction=prediction)
    got, want = vlb_tables(fp, prediction, m), vlb_tables(fp, prediction, "posterior")
    for name in ("sigma2", "kc", "g"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.shape == (T,) and torch.allclose(a, b, rtol=1e-14, atol=0), name
    assert (got.kc == 0).all()
    assert got.inv_sigma0 == pytest.approx(want.inv_sigma0, rel=1e-14)
    assert got.variance is m and vlb_tables(fp, prediction, m) is not got      # not cached on the diffusion
    # and in the samplers: the sigma of ddim_schedule(eta) at every row k >= 1
    from tiny_diffusion_amd.analytic import optimal_sigma2
    from tiny_diffusion_amd.schedule import ddim_schedule

    for eta in (1.0, 0.3):
        s2 = optimal_sigma2(fp, m, None, eta)
        assert torch.allclose(s2[1:], ddim_schedule(fp, steps=T, eta=eta).coef64[1:, 2] ** 2, rtol=1e-13, atol=0)


@pytest.mark.parametrize("T", [6, 1000])
def test_g_zero_gives_the_upper_bound(T):
    """The full grid at eta = 1: beta_t / alpha_t (row 0: the floor plus beta_0 / alpha_0)."""
    from tiny_diffusion_amd.analytic import optimal_sigma2

    fp = _fp(T)
    got = optimal_sigma2(fp, _moments(T, torch.zeros(T)), None, 1.0, None)
    ab, abp = A.ab_columns(fp, A.full(fp))
    want = (1 - ab / abp) / (ab / abp)
    _close(got[1:], want[1:])
    assert abs(got[0].item() - (A.floor0(fp, A.full(fp)) + want[0].item())) <= RTOL * got[0].item()


# ------------------------------------------------------------------ 3. bounds and the data-range cap
@pytest.mark.parametrize("eta", [1.0, 0.5])
@pytest.mark.parametrize("T,taus", GRIDS, ids=lambda v: "full" if v is None else str(v))
def test_bounds_hold_for_any_estimate(T, taus, eta):
    from tiny_diffusion_amd.analytic import optimal_excess, optimal_sigma2

    fp = _fp(T)
    chain = A.full(fp) if taus is None else taus
    gen = torch.Generator().manual_seed(T + len(chain))
    g = torch.rand(len(chain), generator=gen, dtype=torch.float64) * 2 - 0.5          # [-0.5, 1.5]
    m = _moments(T, g, chain)
    lam2, r, u = A.lam2_r_u(fp, chain, eta)
    lam2[0] = A.floor0(fp, chain)
    free = optimal_sigma2(fp, m, taus, eta, None)
    assert (free >= lam2 * (1 - 1e-15)).all() and (free <= (lam2 + r * r) * (1 + 1e-15)).all()
    assert torch.equal(free[g >= 1], optimal_excess(fp, m, taus, eta, None)[0][g >= 1])     # exactly the floor
    _close(free[g <= 0], (lam2 + r * r)[g <= 0], 1e-14)
    _close(free, A.sigma2_star(fp, chain, g, eta, None), 1e-13)
    for rng in ((-1.0, 1.0), (-0.1, 0.1), (0.0, 3.0)):
        h2 = (0.5 * (rng[1] - rng[0])) ** 2
        capped = optimal_sigma2(fp, m, taus, eta, rng)
        assert (capped <= free).all() and (capped <= (lam2 + u * u * h2) * (1 + 1e-15)).all()
        _close(capped, A.sigma2_star(fp, chain, g, eta, rng), 1e-13)


def test_the_cap_binds_where_it_should():
    """g = 0 and data in [-0.1, 0.1]: u^2 h^2 < r^2 = u^2 (1 - ab) / ab exactly where (1 - ab) / ab > h^2 = 0.01."""
    from tiny_diffusion_amd.analytic import optimal_sigma2

    fp = _fp(1000)
    ab, _ = A.ab_columns(fp, A.full(fp))
    lam2, r, u = A.lam2_r_u(fp, A.full(fp), 1.0)
    lam2[0] = A.floor0(fp, A.full(fp))
    got = optimal_sigma2(fp, _moments(1000, torch.zeros(1000)), None, 1.0, (-0.1, 0.1))
    binds = (1 - ab) / ab > 0.01
    assert binds.any() and (~binds).any()
    _close(got[binds], (lam2 + u * u * 0.01)[binds], 1e-14)
    _close(got[~binds], (lam2 + r * r)[~binds], 1e-14)
    assert (got[binds] < (lam2 + r * r)[binds]).all()


# ------------------------------------------------------------------ 4. the tables of a sub-trajectory
def _variances(T, taus):
    gen = torch.Generator().manual_seed(5)
    g = torch.rand(len(taus), generator=gen, dtype=torch.float64)
    return [("beta", "beta", None), ("posterior", "posterior", None), ("analytic", _moments(T, g, taus), g)]


@pytest.mark.parametrize("T,taus", [(1000, SPARSE), (1000, list(range(0, 1000, 100))), (6, [0, 2, 5]), (6, [1, 4])], ids=str)
def test_sub_trajectory_rows_are_the_kl_of_the_two_normals(T, taus):
    """Row k >= 1 from first principles: the forward step tau_{k-1} -> tau_k is N(sqrt(alpha_k) x, beta_k) with alpha_k
    = ab/abp, so q(x_{tau_{k-1}} | x_{tau_k}, x_0) has the variance 1 / (alpha_k / beta_k + 1 / (1 - abp)) and the
    weight var sqrt(abp) / (1 - abp) on x_0; kc_k + g_k d^2 is the KL to the model's normal, whose mean differs by
    c0_k d - by the method and the tolerances of test_vlb_host.py::test_kl_term_is_the_kl_of_the_two_normals."""
    from torch.distributions import Normal, kl_divergence

    from tiny_diffusion_amd.likelihood import vlb_tables

    fp = _fp(T)
    ab, abp = A.ab_columns(fp, taus)
    S = len(taus)
    for name, variance, g in _variances(T, taus):
        tb = vlb_tables(fp, "eps", variance, timesteps=taus)
        want = A.sub_tables64(fp, taus, "eps", name, g)
        for mine, key in ((tb.c0, "c0"), (tb.beta_tilde, "bt"), (tb.sigma2, "s2"), (tb.kc, "kc"), (tb.g, "g")):
            assert mine.shape == (S,) and torch.allclose(mine, want[key], rtol=1e-13, atol=1e-300), (name, key)
        assert tb.p.shape == (T,) and torch.equal(tb.p, vlb_tables(fp, "eps", "beta").p)
        assert tb.timesteps.tolist() == taus and tb.acp_last == ab[-1].item() and tb.c0[0].item() == 1.0
        assert tb.inv_sigma0 == pytest.approx(want["inv_sigma0"], rel=1e-14)
        rows = tb.rows(bins=True)
        assert rows.shape == (T, 5) and rows[taus[0], 4].item() > 0 and int((rows[:, 4] != 0).sum()) == 1
        for k in sorted({1, S // 2, S - 1}):
            alpha, beta = (ab[k] / abp[k]).item(), (1 - ab[k] / abp[k]).item()
            var = 1.0 / (alpha / beta + 1.0 / (1 - abp[k].item()))
            w0 = var * math.sqrt(abp[k].item()) / (1 - abp[k].item())
            assert tb.beta_tilde[k].item() == pytest.approx(var, rel=1e-10)
            assert tb.c0[k].item() == pytest.approx(w0, rel=1e-10)
            c0, bt, s2 = tb.c0[k], tb.beta_tilde[k], tb.sigma2[k]
            d = torch.tensor([0.5, -1.0, 3.0], dtype=torch.float64) * s2.sqrt() / c0
            mu_q = torch.full_like(d, 0.25)
            kl = kl_divergence(Normal(mu_q, bt.sqrt()), Normal(mu_q - c0 * d, s2.sqrt()))
            got = tb.kc[k] + tb.g[k] * d ** 2
            assert ((got - kl).abs() <= 1e-12 * kl).all(), (name, k, got.tolist(), kl.tolist())
            kl0 = kl_divergence(Normal(mu_q[:1], bt.sqrt()), Normal(mu_q[:1], s2.sqrt())).item()
            assert abs(tb.kc[k].item() - kl0) <= 1e-12 * kl0 + 4 * 2.0 ** -53, (name, k, kl0)
            if name == "beta":
                assert s2.item() == beta
            if name != "beta":
                assert tb.kc[k].item() >= 0.0
        if name == "posterior":
            assert (tb.kc == 0).all() and tb.sigma2[0] == tb.beta_tilde[1]
        assert vlb_tables(fp, "eps", variance, timesteps=taus) is tb or name == "analytic"     # the named ones are cached


@pytest.mark.parametrize("T", [6, 1000])
def test_the_list_of_all_timesteps_is_the_full_grid_bit_for_bit(T):
    from tiny_diffusion_amd.likelihood import vlb_tables

    fp = _fp(T)
    m = _moments(T, torch.linspace(0.2, 1.1, T, dtype=torch.float64), prediction="v")
    for prediction, variance in (("eps", "beta"), ("v", "posterior"), ("v", m)):
        a = vlb_tables(fp, prediction, variance)
        for taus in (range(T), list(range(T)), torch.arange(T)):
            b = vlb_tables(fp, prediction, variance, timesteps=taus)
            for name in ("p", "q", "ex", "eo", "c0", "beta_tilde", "sigma2", "kc", "g", "timesteps"):
                assert torch.equal(getattr(a, name), getattr(b, name)), name
            assert a.inv_sigma0 == b.inv_sigma0 and a.acp_last == b.acp_last
            assert torch.equal(a.rows(), b.rows())
    want = H.tables64(fp, "eps", "beta")             # and today's values: the restatement of test_vlb_host.py
    tb = vlb_tables(fp, "eps", "beta", timesteps=range(T))
    assert torch.equal(tb.rows(bins=True), H.rows32(want, True)) and torch.equal(tb.sigma2, fp.betas.double())


# ------------------------------------------------------------------ 5. with_sigma
def test_with_sigma_keeps_the_mean_and_rounds_sigma_once():
    from tiny_diffusion_amd.schedule import ddim_schedule, ddpm_schedule, dpm_solver_schedule

    fp = _fp(1000)
    for sched in (ddpm_schedule(fp), ddim_schedule(fp, steps=50, eta=0.7), ddim_schedule(fp, timesteps=SPARSE, eta=1.0)):
        S = sched.steps
        sigma = torch.linspace(0.0, 0.3, S, dtype=torch.float64) + 1e-9 / 3
        before = (sched.coef.clone(), sched.coef64.clone())
        new = sched.with_sigma(sigma)
        assert new is not sched and torch.equal(sched.coef, before[0]) and torch.equal(sched.coef64, before[1])
        assert new.coef.dtype == torch.float32 and new.coef.is_contiguous() and new.coef.shape == (S, 3)
        assert torch.equal(new.coef[:, :2], sched.coef[:, :2])             # bit for bit: the reference's own rows
        assert torch.equal(new.coef[:, 2], sigma.to(torch.float32))        # one rounding
        assert torch.equal(new.coef64[:, :2], sched.coef64[:, :2]) and torch.equal(new.coef64[:, 2], sigma)
        assert torch.equal(new.timesteps, sched.timesteps) and new.eta == sched.eta
        assert new.num_timesteps == sched.num_timesteps
        # the x0 form and the v form carry the new sigma and nothing else new
        for prediction in ("eps", "v"):
            f64, old = new.x0_form(fp, prediction, dtype=torch.float64), sched.x0_form(fp, prediction, dtype=torch.float64)
            assert torch.equal(f64[:, :4], old[:, :4]) and torch.equal(f64[:, 4], sigma)
            f32 = new.x0_form(fp, prediction)
            assert torch.equal(f32[:, :4], sched.x0_form(fp, prediction)[:, :4])
            assert torch.equal(f32[:, 4], sigma.to(torch.float32))
        v, vold = new.for_prediction(fp, "v"), sched.for_prediction(fp, "v")
        assert torch.equal(v.coef[:, :2], vold.coef[:, :2]) and torch.equal(v.coef[:, 2], sigma.to(torch.float32))
        assert torch.equal(v.coef64[:, 2], sigma) and new.for_prediction(fp, "eps") is new
    ref = ddpm_schedule(fp)
    assert torch.equal(ref.with_sigma(ref.coef64[:, 2]).coef, fp.tables("cpu")[2])     # its own sigma: nothing changes
    for bad in (torch.zeros(999), torch.zeros(1000, 1), -torch.ones(1000), torch.full((1000,), float("nan")),
                torch.full((1000,), float("inf")), torch.zeros(1000, dtype=torch.bool)):
        with pytest.raises(ValueError, match="sigma"):
            ref.with_sigma(bad)
    with pytest.raises(ValueError, match="deterministic"):
        dpm_solver_schedule(fp, steps=10).with_sigma(torch.zeros(10))


# ------------------------------------------------------------------ 6. EpsMoments
def test_eps_moments_object():
    from tiny_diffusion_amd.analytic import EpsMoments

    m = EpsMoments(10, [0.5, 0.75, 1.0], timesteps=[1, 4, 9], stderr=[0.01, 0.0, 0.02], count=64, prediction="v")
    assert m.num_timesteps == 10 and m.timesteps.dtype == torch.int64 and m.timesteps.tolist() == [1, 4, 9]
    assert m.g.dtype == torch.float64 and m.stderr.dtype == torch.float64 and m.count == 64 and m.prediction == "v"
    for name in ("g", "count", "other"):
        with pytest.raises(AttributeError):
            setattr(m, name, 0)
    with pytest.raises(AttributeError):
        del m.g
    sd = m.state_dict()
    assert all(isinstance(v, (torch.Tensor, str)) for v in sd.values()) and isinstance(sd["prediction"], str)
    back = EpsMoments.from_state_dict(sd)
    assert back.num_timesteps == 10 and back.count == 64 and back.prediction == "v"
    for name in ("timesteps", "g", "stderr"):
        assert torch.equal(getattr(back, name), getattr(m, name))
    sd["g"][0] = 7.0
    assert m.g[0].item() == 0.5                                   # the state dict holds copies
    full = EpsMoments(4, torch.ones(4))
    assert full.timesteps.tolist() == [0, 1, 2, 3] and (full.stderr == 0).all() and full.count == 0
    assert full.prediction == "eps" and torch.equal(m.at([9, 1]), torch.tensor([1.0, 0.5], dtype=torch.float64))
    for kw in (dict(g=[1.0, 1.0]), dict(g=[1.0, float("nan"), 1.0]), dict(timesteps=[4, 1, 9]), dict(timesteps=[1, 4, 10]),
               dict(timesteps=[1, 4, 4]), dict(stderr=[-1.0, 0.0, 0.0]), dict(stderr=[0.0]), dict(count=-1),
               dict(count=1.5), dict(prediction="x0"), dict(num_timesteps=0), dict(num_timesteps=True)):
        args = dict(num_timesteps=10, g=[0.5, 0.75, 1.0], timesteps=[1, 4, 9])
        args.update(kw)
        with pytest.raises(ValueError):
            EpsMoments(**args)


def test_optimal_sigma2_errors():
    from tiny_diffusion_amd.analytic import optimal_sigma2

    fp = _fp(10)
    m = _moments(10, [0.5, 0.75, 1.0], [1, 4, 9])
    assert optimal_sigma2(fp, m, [1, 9]).shape == (2,) and optimal_sigma2(fp, m, [1, 4, 9], 0.5, None).dtype == torch.float64
    with pytest.raises(ValueError, match="no estimate"):
        optimal_sigma2(fp, m)                                     # the full grid: most timesteps are missing
    with pytest.raises(ValueError, match="no estimate"):
        optimal_sigma2(fp, m, [1, 5, 9])
    with pytest.raises(ValueError, match="T = 10"):
        optimal_sigma2(_fp(12), m, [1, 4, 9])
    for eta in (0.0, -1.0, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="eta"):
            optimal_sigma2(fp, m, [1, 4, 9], eta)
    with pytest.raises(ValueError, match="too large"):
        optimal_sigma2(fp, m, [1, 4, 9], 30.0)
    with pytest.raises(ValueError, match="at least 2"):
        optimal_sigma2(fp, m, [4])
    for bad in ([4, 1], [1, 10], [], [1.5, 4]):
        with pytest.raises(ValueError, match="timesteps"):
            optimal_sigma2(fp, m, bad)
    for rng in ((1, 1), (1, -1), (0, float("inf")), (0, 1, 2), "ab"):
        with pytest.raises(ValueError, match="data_range"):
            optimal_sigma2(fp, m, [1, 4, 9], 1.0, rng)
    with pytest.raises(ValueError, match="EpsMoments"):
        optimal_sigma2(fp, "posterior", [1, 4, 9])


# ------------------------------------------------------------------ 7. the C entry
def test_entry_declared_listed_and_bound():
    import tiny_diffusion_amd._lib as L

    hdr = open(os.path.join(ROOT, "include", "tdx.h")).read()
    assert re.search(r"\btdx_eps_sqnorm\s*\(", hdr)
    assert "tdx_eps_sqnorm" in L.EXPORTS
    assert len(L.lib.tdx_eps_sqnorm.argtypes) == 9
    assert L.lib.tdx_version() == 400   # the ABI only grows
    assert os.path.exists(os.path.join(ROOT, "tiny_diffusion_amd", "csrc", "analytic.hip"))


@pytest.mark.parametrize("bad", A.SQNORM_BAD_ARGS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_entry_rejects_bad_arguments_before_any_gpu_call(bad):
    assert A.sqnorm_call(**bad) == TDX_E_BADARG, bad


# ------------------------------------------------------------------ 8. the kernel's bound, without a GPU
@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("per", A.SQNORM_PERS)
def test_fp32_restatement_stays_within_the_derived_bound(per, prediction):
    fp = _fp(1000)
    rows = A.eps_rows32(fp, prediction)
    t = torch.tensor([500, 0, 999])
    x_t, out = A.sqnorm_inputs(fp, per, t.tolist())
    want, bound = A.sqnorm64(x_t, out, rows, t)
    got = A.sqnorm32(x_t, out, rows, t).double()
    err = (got - want).abs()
    print(f"per={per} {prediction}: |restatement - fp64| / bound = {(err / bound).tolist()}, bound / want = {(bound / want).tolist()}")
    assert (want > 0).all() and (err <= bound).all()
    assert (bound <= 1e-3 * want).all()              # a bound, not a licence: 4096 elements, (per + 1) 2^-24 = 2.4e-4
    if prediction == "eps":                          # rows (0, 1): the sum of out^2
        assert ((want - (out.double() ** 2).sum(1)).abs() <= 1e-15 * want).all()
    # a plain fp32 sum in another order obeys the same bound
    r = rows[t]
    e = r[:, 0:1] * x_t + r[:, 1:2] * out
    assert (((e * e).sum(1).double() - want).abs() <= bound).all()


# ------------------------------------------------------------------ 9. argument errors, before the model or the GPU
class _NoModel:
    def eval(self):
        raise AssertionError("the argument errors come before the model is touched")


class _CondModel(_NoModel):
    num_classes = 10


class _Vae:
    def eval(self):
        return self


def _samplers(fp, which="sample", device="cpu", **kw):
    """Every public way into a sampling chain, on a model that must not be touched."""
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import conditional_diffusion_laion as LA
    from tiny_diffusion_amd import diffusion as D
    from tiny_diffusion_amd import diffusion_transformer as DT
    from tiny_diffusion_amd import latent_diffusion as LD
    from tiny_diffusion_amd import schedule as SC

    y, te = torch.arange(2), torch.zeros(2, 768)
    loop = {"sample": SC.sample_loop, "ddim_sample": SC.ddim_sample_loop, "dpm_sample": SC.dpm_sample_loop}[which]
    return {"loop": lambda: loop(_NoModel(), fp, device, 2, **kw),
            "diffusion": lambda: getattr(D, which)(_NoModel(), fp, device, 2, **kw),
            "conditional_diffusion": lambda: getattr(C, which)(_NoModel(), fp, device, 2, y=y, **kw),
            "conditional_diffusion_laion": lambda: getattr(LA, which)(_NoModel(), fp, device, text_embeds=te, **kw),
            "latent_diffusion": lambda: getattr(LD, which)(_Vae(), _NoModel(), fp, device, 2, y=y, **kw),
            "diffusion_transformer": lambda: getattr(DT, which)(_Vae(), _NoModel(), fp, device, 2, y=y, **kw)}


def _each(calls, exc, match):
    for name, call in calls.items():
        with pytest.raises(exc, match=match):
            call()


def test_sampler_variance_errors_come_first_everywhere():
    from tiny_diffusion_amd import _lib

    fp = _fp(6)
    m = _moments(6, torch.full((6,), 0.8))
    for bad in ("beta", "posterior", 0.5, torch.ones(6), True):
        _each(_samplers(fp, variance=bad), ValueError, "variance")
        _each(_samplers(fp, "ddim_sample", steps=3, eta=1.0, variance=bad), ValueError, "variance")
    _each(_samplers(fp, variance=m, prediction="v"), ValueError, "prediction")
    _each(_samplers(fp, variance=_moments(6, torch.ones(6), prediction="v")), ValueError, "prediction")
    _each(_samplers(fp, variance=_moments(7, torch.ones(7))), ValueError, "T = 7")
    _each(_samplers(fp, variance=_moments(6, [1.0, 1.0], [0, 1])), ValueError, "no estimate")
    _each(_samplers(fp, "ddim_sample", steps=3, eta=1.0, variance=_moments(6, [1.0, 1.0], [0, 1])), ValueError, "no estimate")
    _each(_samplers(fp, "ddim_sample", steps=3, eta=0.0, variance=m), ValueError, "eta")
    _each(_samplers(fp, "ddim_sample", steps=3, variance=m), ValueError, "eta")               # the default eta is 0
    _each(_samplers(fp, "ddim_sample", steps=1, eta=1.0, variance=m), ValueError, "at least 2")
    _each(_samplers(fp, "dpm_sample", steps=3, variance=m), ValueError, "deterministic")
    _each(_samplers(fp, "dpm_sample", steps=3, variance="beta"), ValueError, "deterministic")
    # accepted arguments reach the device check, and variance=None is every chain as before
    for kw in (dict(variance=m), dict(variance=m, clip_denoised=True), dict(variance=None),
               dict(variance=_moments(6, torch.ones(6), prediction="v"), prediction="v")):
        _each(_samplers(fp, **kw), _lib.TdxError, "GPU only")
    _each(_samplers(fp, "ddim_sample", steps=3, eta=0.5, variance=m), _lib.TdxError, "GPU only")
    _each(_samplers(fp, "ddim_sample", timesteps=[0, 1], eta=1.0, variance=_moments(6, [1.0, 1.0], [0, 1])),
          _lib.TdxError, "GPU only")
    _each(_samplers(fp, "dpm_sample", steps=3, variance=None), _lib.TdxError, "GPU only")


def _bounds(fp, x_0, **kw):
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import conditional_diffusion_laion as LA
    from tiny_diffusion_amd import diffusion as D
    from tiny_diffusion_amd import diffusion_transformer as DT
    from tiny_diffusion_amd import latent_diffusion as LD
    from tiny_diffusion_amd.likelihood import bits_per_dim_loop

    y, te = torch.arange(2), torch.zeros(2, 768)
    return {"loop": lambda: bits_per_dim_loop(_NoModel(), fp, x_0, **kw),
            "diffusion": lambda: D.bits_per_dim(_NoModel(), fp, x_0, **kw),
            "conditional_diffusion": lambda: C.bits_per_dim(_NoModel(), fp, x_0, y=y, **kw),
            "conditional_diffusion_laion": lambda: LA.bits_per_dim(_NoModel(), fp, x_0, text_embeds=te, **kw),
            "latent_diffusion": lambda: LD.bits_per_dim(_NoModel(), fp, x_0, y=y, **kw),
            "diffusion_transformer": lambda: DT.bits_per_dim(_NoModel(), fp, x_0, y=y, **kw)}


def test_likelihood_errors_come_first_everywhere():
    from tiny_diffusion_amd import _lib
    from tiny_diffusion_amd.likelihood import VARIANCES, bits_per_dim_terms, vlb_tables

    assert VARIANCES == ("beta", "posterior")
    fp = _fp(6)
    x0 = torch.zeros(2, 20)
    m = _moments(6, torch.full((6,), 0.8))
    for bad in (None, "learned", "analytic", 0.5):
        _each(_bounds(fp, x0, variance=bad), ValueError, "variance")
        with pytest.raises(ValueError, match="variance"):
            vlb_tables(fp, "eps", bad)
    _each(_bounds(fp, x0, variance=m, prediction="v"), ValueError, "prediction")
    _each(_bounds(fp, x0, variance=_moments(7, torch.ones(7))), ValueError, "T = 7")
    _each(_bounds(fp, x0, variance=_moments(6, [1.0, 1.0], [0, 1])), ValueError, "no estimate")
    _each(_bounds(fp, x0, variance=m, timesteps=[3]), ValueError, "at least 2")
    _each(_bounds(fp, x0, variance="posterior", timesteps=[3]), ValueError, "T >= 2")
    for bad in ([2, 0, 5], [0, 2, 6], [-1, 2], [], [0, 2, 2], [0.5, 2], torch.tensor([0.0, 2.0])):
        _each(_bounds(fp, x0, timesteps=bad), ValueError, "timesteps")
    _each(_bounds(fp, x0, timesteps=[0, 2, 5], noises={0: x0, 2: x0}), ValueError, "noises")   # tau = 5 is missing
    with pytest.raises(ValueError, match="prediction"):
        bits_per_dim_terms(_NoModel(), fp, x0, torch.zeros(2, dtype=torch.int64), variance=m, prediction="v")
    for kw in (dict(variance=m), dict(timesteps=[0, 2, 5]), dict(variance=m, timesteps=[0, 2, 5], philox_seed=1),
               dict(timesteps=[0, 2, 5], noises={0: x0, 2: x0, 5: x0}), dict(timesteps=range(6), variance="posterior"),
               dict(variance=m, bins=16, data_range=(-3, 3)), dict(timesteps=[3], variance="beta")):
        _each(_bounds(fp, x0, **kw), _lib.TdxError, "GPU only")
    with pytest.raises(_lib.TdxError, match="GPU only"):
        bits_per_dim_terms(_NoModel(), fp, x0, torch.zeros(2, dtype=torch.int64), variance=m)


def test_estimate_errors_come_before_any_gpu_work():
    from tiny_diffusion_amd import _lib
    from tiny_diffusion_amd.analytic import estimate_eps_moments

    fp = _fp(6)
    x0 = torch.zeros(2, 20)
    with pytest.raises(ValueError, match="condition"):
        estimate_eps_moments(_CondModel(), fp, x0)
    with pytest.raises(ValueError, match="one row per sample"):
        estimate_eps_moments(_CondModel(), fp, x0, y=torch.arange(3))
    for bad in ([2, 0], [0, 6], [], [0.5], [1, 1]):
        with pytest.raises(ValueError, match="timesteps"):
            estimate_eps_moments(_NoModel(), fp, x0, timesteps=bad)
    for bad in (-1, None, 0.5, True):
        with pytest.raises(ValueError, match="philox_seed"):
            estimate_eps_moments(_NoModel(), fp, x0, philox_seed=bad)
    for bad in (0, -1, 1.5, None, True):
        with pytest.raises(ValueError, match="repeats"):
            estimate_eps_moments(_NoModel(), fp, x0, repeats=bad)
    for bad in (0, -2, 2.0, True):
        with pytest.raises(ValueError, match="batch_size"):
            estimate_eps_moments(_NoModel(), fp, x0, batch_size=bad)
    with pytest.raises(ValueError, match="prediction"):
        estimate_eps_moments(_NoModel(), fp, x0, prediction="x0")
    for bad in (torch.zeros(2, 22), torch.zeros(2, 1, 3, 3)):
        with pytest.raises(ValueError, match="multiple of 4"):
            estimate_eps_moments(_NoModel(), fp, bad)
    for bad in (torch.zeros(20), torch.zeros(0, 20), [[0.0] * 20]):
        with pytest.raises(ValueError, match="x_0"):
            estimate_eps_moments(_NoModel(), fp, bad)
    for kw in (dict(), dict(timesteps=[0, 3, 5], repeats=2, batch_size=1, prediction="v", philox_seed=9)):
        with pytest.raises(_lib.TdxError, match="GPU only"):
            estimate_eps_moments(_NoModel(), fp, x0, **kw)
    with pytest.raises(_lib.TdxError, match="GPU only"):
        estimate_eps_moments(_CondModel(), fp, x0, y=torch.arange(2))


def test_the_keyword_is_documented_in_every_module():
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import conditional_diffusion_laion as LA
    from tiny_diffusion_amd import diffusion as D
    from tiny_diffusion_amd import diffusion_transformer as DT
    from tiny_diffusion_amd import latent_diffusion as LD

    for mod in (D, C, LA, LD, DT):
        assert "variance=m" in mod.sample.__doc__ and "EpsMoments" in mod.sample.__doc__, mod.__name__
        assert "EpsMoments" in mod.bits_per_dim.__doc__ and "timesteps" in mod.bits_per_dim.__doc__, mod.__name__
