"""Variational-bound evaluation, host side (no GPU): the fp64 restatement (tests/vlb_helpers.py) is pinned against
``torch.distributions`` and against itself, the package's tables and host formulas against the restatement, the new C
entry is declared, bound and rejects every bad argument before any GPU call, and every argument error of the Python
functions is a ``ValueError`` that comes before the device check, in all five modules."""
import ctypes
import math
import os
import re

import pytest
import torch

import vlb_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")
TDX_E_BADARG = -1


def _fp(T=1000):
    from tiny_diffusion_amd.schedule import ForwardProcess

    return ForwardProcess(num_timesteps=T)


# ------------------------------------------------------------------ 1. the per-element KL against torch.distributions
@pytest.mark.parametrize("variance", ["beta", "posterior"])
@pytest.mark.parametrize("T", [1000, 6])
def test_kl_term_is_the_kl_of_the_two_normals(T, variance):
    """kc_t + g_t d^2 is KL(N(mu_q, btilde_t) || N(mu_p, sigma2_t)) where the means differ by c0_t d: to 1e-12
    relative, with d chosen so that the means lie 0.5 to 3 sigma apart (c0_t at T - 1 of a thousand steps is 1e-4: an
    error of pixel size moves the mean by next to nothing).  At d = 0 the KL is kc_t alone, down to 1e-13 at T - 1 under
    "beta", and ``kl_divergence`` itself forms it as ``r + t1 - 1 - log r`` from terms of size 1: there the comparison
    allows those four roundings, 4 * 2^-53, next to the 1e-12 relative."""
    from torch.distributions import Normal, kl_divergence

    tab = H.tables64(_fp(T), "eps", variance)
    for t in (1, T // 2, T - 1):
        c0, bt, s2 = tab["c0"][t], tab["bt"][t], tab["s2"][t]
        d = torch.tensor([0.5, -1.0, 3.0], dtype=torch.float64) * s2.sqrt() / c0
        mu_q = torch.full_like(d, 0.25)
        want = kl_divergence(Normal(mu_q, bt.sqrt()), Normal(mu_q - c0 * d, s2.sqrt()))
        got = tab["kc"][t] + tab["g"][t] * d ** 2
        assert ((got - want).abs() <= 1e-12 * want).all(), (T, variance, t, got.tolist(), want.tolist())
        want0 = kl_divergence(Normal(mu_q[:1], bt.sqrt()), Normal(mu_q[:1], s2.sqrt())).item()
        assert abs(tab["kc"][t].item() - want0) <= 1e-12 * want0 + 4 * 2.0 ** -53, (T, variance, t, want0)
        if variance == "posterior":
            assert tab["kc"][t].item() == 0.0 and want0 == 0.0


# ------------------------------------------------------------------ 2. the bins of one element sum to 1
@pytest.mark.parametrize("mu", [-1.0, 0.3, 1.0])
@pytest.mark.parametrize("bins", [256, 257])
def test_decoder_probabilities_sum_to_one(bins, mu):
    """Over the levels of one element the floored probabilities sum to 1 within bins * 1e-12 plus rounding.  The
    rounding: neighbouring bins meet at x_k + half and x_{k+1} - half, which differ by w = |2 half32 - step| because
    half is an fp32 number; a gap or overlap of width w holds at most phi(0) s w of probability.  With 257 levels half
    = 1/256 is exact and w = 0."""
    s = 100.0
    half, _, _ = H.edges32((-1.0, 1.0), bins)
    step = 2.0 / (bins - 1)
    x0 = -1.0 + step * torch.arange(bins, dtype=torch.float64)
    x0[-1] = 1.0
    nll, _ = H.dec_nll(x0, x0 - mu, s, (-1.0, 1.0), bins, torch.float64)
    total = torch.exp(-nll).sum().item()
    w = abs(2.0 * half - step)
    tol = bins * H.FLOOR + (bins - 1) * 0.3990 * s * w + 1e-13
    if bins == 257:
        assert w == 0.0
    assert abs(total - 1.0) <= tol, (bins, mu, total - 1.0, tol)
    tb, _ = H.dec_nll(x0, x0 - mu, s, (-1.0, 1.0), bins, torch.float64, form="textbook")
    assert abs(torch.exp(-tb).sum().item() - 1.0) <= tol


# ------------------------------------------------------------------ 3. a perfect prediction under the posterior variance
@pytest.mark.parametrize("T", [1000, 6])
def test_perfect_prediction_has_zero_kl(T):
    fp = _fp(T)
    tab = H.tables64(fp, "eps", "posterior")
    sums = torch.zeros(2, T, 3, dtype=torch.float64)
    sums[..., 2] = 5.0     # the decoder column is whatever it is: only t >= 1 is asked about
    vb, mse, xs = H.assemble64(tab, sums, torch.arange(T).expand(2, T), 784, 256)
    assert (vb[:, 1:] == 0).all() and (xs == 0).all() and (mse == 0).all()
    assert (H.assemble64(H.tables64(fp, "eps", "beta"), sums, torch.arange(T).expand(2, T), 784, 256)[0][:, 1:] > 0).all()


# ------------------------------------------------------------------ 4. the package's tables
@pytest.mark.parametrize("variance", ["beta", "posterior"])
@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("T", [1000, 6, 2])
def test_package_tables(T, prediction, variance):
    from tiny_diffusion_amd.likelihood import vlb_tables
    from tiny_diffusion_amd.schedule import ddpm_schedule

    fp = _fp(T)
    tb = vlb_tables(fp, prediction, variance)
    assert vlb_tables(fp, prediction, variance) is tb          # cached on the diffusion
    want = H.tables64(fp, prediction, variance)
    assert tb.c0[0].item() == 1.0                              # exactly, not from the rounded tables
    for mine, name in ((tb.p, "p"), (tb.q, "q"), (tb.ex, "ex"), (tb.eo, "eo"), (tb.c0, "c0"), (tb.beta_tilde, "bt"),
                       (tb.sigma2, "s2"), (tb.kc, "kc"), (tb.g, "g")):
        assert mine.dtype == torch.float64 and mine.shape == (T,)
        assert torch.allclose(mine, want[name], rtol=1e-14, atol=0), name
    assert tb.inv_sigma0 == pytest.approx(want["inv_sigma0"], rel=1e-15)
    assert tb.acp_last == fp.alphas_cumprod.double()[-1].item()
    assert torch.equal(torch.stack([tb.p, tb.q], 1), ddpm_schedule(fp).x0_form(fp, prediction, dtype=torch.float64)[:, :2])
    if variance == "beta":
        assert torch.equal(tb.sigma2, fp.betas.double())
    else:
        assert torch.equal(tb.sigma2[1:], tb.beta_tilde[1:]) and tb.sigma2[0] == tb.beta_tilde[1]
        assert tb.beta_tilde[0].item() == 0.0
    rows = tb.rows(bins=True)
    assert rows.dtype == torch.float32 and rows.shape == (T, 5) and torch.equal(rows, H.rows32(want, True))
    assert rows[0, 4].item() > 0 and (rows[1:, 4] == 0).all()   # dec: row 0 only ...
    assert (tb.rows(bins=False)[:, 4] == 0).all()               # ... and only with bins
    assert torch.equal(tb.rows(bins=False), H.rows32(want, False))
    assert tb.rows(dtype=torch.float64)[0, 4].item() == tb.inv_sigma0
    if prediction == "eps":
        assert (rows[:, 2] == 0).all() and (rows[:, 3] == 1).all()


def test_table_errors():
    from tiny_diffusion_amd.likelihood import vlb_tables

    for bad in ("learned", None, 3, "Beta"):
        with pytest.raises(ValueError, match="variance"):
            vlb_tables(_fp(6), "eps", bad)
    with pytest.raises(ValueError, match="prediction"):
        vlb_tables(_fp(6), "x0", "beta")
    with pytest.raises(ValueError, match="T >= 2"):
        vlb_tables(_fp(1), "eps", "posterior")
    assert vlb_tables(_fp(1), "eps", "beta").rows().shape == (1, 5)


def test_package_host_formulas_match_the_restatement():
    from tiny_diffusion_amd.likelihood import _assemble, _prior_bpd, vlb_tables

    g = torch.Generator().manual_seed(3)
    for T, D, bins, variance in ((6, 20, None, "posterior"), (1000, 784, 256, "beta")):
        fp = _fp(T)
        sums = (torch.rand(3, T, 3, generator=g) * 50).float()
        steps = torch.arange(T).expand(3, T)
        want = H.assemble64(H.tables64(fp, "v", variance), sums, steps, D, bins)
        got = _assemble(vlb_tables(fp, "v", variance), sums, steps, D, bins)
        for a, b in zip(got, want):
            assert a.dtype == torch.float64 and torch.allclose(a, b, rtol=1e-14, atol=0)
        x0 = torch.randn(3, D, generator=g)
        sq = (x0.double() ** 2).sum(1)
        assert torch.allclose(_prior_bpd(vlb_tables(fp, "v", variance), sq, D), H.prior64(H.tables64(fp, "v", variance), x0),
                              rtol=1e-14, atol=0)
    # the continuous decoder is the Gaussian negative log-density of x0 under N(x0c, sigma2_0)
    from torch.distributions import Normal
    tab = H.tables64(_fp(6), "eps", "beta")
    d = torch.tensor([0.01, -0.02, 0.005, 0.0], dtype=torch.float64)
    sums = torch.zeros(1, 1, 3, dtype=torch.float64)
    sums[0, 0, 1] = (d ** 2).sum()
    vb = H.assemble64(tab, sums, torch.zeros(1, 1, dtype=torch.int64), 4, None)[0]
    want = -Normal(torch.zeros(4, dtype=torch.float64), tab["s2"][0].sqrt()).log_prob(d).sum() / (4 * H.LN2)
    assert vb.item() == pytest.approx(want.item(), rel=1e-13)
    assert vb.item() < 0            # a density: negative bits per dimension are possible


def test_prior_is_the_kl_to_the_standard_normal():
    from torch.distributions import Normal, kl_divergence

    fp = _fp(1000)
    tab = H.tables64(fp, "eps", "beta")
    x0 = torch.tensor([[0.5, -1.0, 0.25, 1.0]])
    ab = tab["acp_last"]
    want = kl_divergence(Normal(math.sqrt(ab) * x0.double(), math.sqrt(1 - ab)), Normal(0.0, 1.0)).sum() / (4 * H.LN2)
    assert H.prior64(tab, x0).item() == pytest.approx(want.item(), rel=1e-9)


# ------------------------------------------------------------------ 5. the tail form against the textbook form in fp64
@pytest.mark.parametrize("per", [4, 20, 784, 4096, 16384])
def test_tail_form_agrees_with_the_textbook_form_in_double(per):
    fp = _fp(1000)
    rows = H.rows32(H.tables64(fp, "eps", "beta"), True)
    worst32 = 0.0
    for t in ([0], [500, 0, 999]):
        x0, x_t, out, eps = H.gen_inputs(fp, per, t, rows)
        for clip in ((-INF, INF), (-1.0, 1.0)):
            d, _ = H.chain32(x0, x_t, out, eps, rows, torch.tensor(t), clip)
            i = t.index(0)
            s = rows[0, 4].item()
            tail, floored = H.dec_nll(x0[i], d[i], s)
            text, _ = H.dec_nll(x0[i], d[i], s, form="textbook")
            text32, _ = H.dec_nll(x0[i], d[i], s, dtype=torch.float32, form="textbook")
            tail32, _ = H.dec_nll(x0[i], d[i], s, dtype=torch.float32)
            ref = tail.sum().item()
            assert abs(text.sum().item() - ref) <= 1e-6 * ref, (per, t, clip)
            assert floored.double().mean().item() <= H.FLOOR_CAP
            assert abs(tail32.double().sum().item() - ref) <= 1e-6 * ref
            worst32 = max(worst32, abs(text32.double().sum().item() - ref) / ref)
    if per >= 784:     # what makes it a kernel: the textbook form in fp32 misses the 1e-4 cap by 50x and more
        assert worst32 > 50 * H.DEC_CAP, worst32
    print(f"per={per}: textbook form in fp32, worst relative error of the per-sample sum {worst32:.2e}")


# ------------------------------------------------------------------ 6. the C entry
def test_entry_declared_listed_and_bound():
    import tiny_diffusion_amd._lib as L

    hdr = open(os.path.join(ROOT, "include", "tdx.h")).read()
    assert re.search(r"\btdx_vlb_terms\s*\(", hdr)
    assert "tdx_vlb_terms" in L.EXPORTS
    assert len(L.lib.tdx_vlb_terms.argtypes) == 16
    assert L.lib.tdx_version() == 400   # the ABI only grows
    assert os.path.exists(os.path.join(ROOT, "tiny_diffusion_amd", "csrc", "likelihood.hip"))


P = 4096     # a non-null address that is never dereferenced: every case below is refused before any GPU call
GOOD = dict(x0=P, x_t=P, out=P, noise=P, t=P, rows=P, batch=2, per=784, clip_lo=-1.0, clip_hi=1.0, data_lo=-1.0,
            data_hi=1.0, bins=256, terms=P, stride=3)
BAD_ARGS = [dict(x0=None), dict(x_t=None), dict(out=None), dict(t=None), dict(rows=None), dict(terms=None),
            dict(batch=0), dict(batch=-1), dict(per=0), dict(per=-4), dict(per=786), dict(per=3), dict(stride=2),
            dict(stride=0), dict(stride=-3), dict(clip_lo=1.0, clip_hi=1.0), dict(clip_lo=1.0, clip_hi=-1.0),
            dict(clip_lo=NAN), dict(clip_hi=NAN), dict(clip_lo=INF, clip_hi=INF), dict(bins=1), dict(bins=-1),
            dict(bins=-256), dict(data_lo=1.0, data_hi=1.0), dict(data_lo=1.0, data_hi=-1.0), dict(data_lo=NAN),
            dict(data_hi=NAN), dict(data_lo=-INF), dict(data_hi=INF), dict(data_lo=-3e38, data_hi=3e38),
            dict(bins=2, data_hi=INF), dict(noise=None, per=2)]


@pytest.mark.parametrize("bad", BAD_ARGS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_entry_rejects_bad_arguments_before_any_gpu_call(bad):
    from tiny_diffusion_amd._lib import lib

    a = dict(GOOD, **bad)
    rc = lib.tdx_vlb_terms(a["x0"], a["x_t"], a["out"], a["noise"], a["t"], a["rows"], a["batch"], a["per"], a["clip_lo"],
                           a["clip_hi"], a["data_lo"], a["data_hi"], a["bins"], a["terms"], a["stride"], None)
    assert rc == TDX_E_BADARG, (bad, rc)


# ------------------------------------------------------------------ 7. the argument errors of the Python functions
class _NoModel:
    def eval(self):
        raise AssertionError("the argument errors come before the model is touched")


class _CondModel(_NoModel):
    num_classes = 10


def _loops(fp, x_0, **kw):
    """Every public way into the loop, on a model that must not be touched, with a condition where one is needed."""
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import conditional_diffusion_laion as LA
    from tiny_diffusion_amd import diffusion as D
    from tiny_diffusion_amd import diffusion_transformer as DT
    from tiny_diffusion_amd import latent_diffusion as LD
    from tiny_diffusion_amd.likelihood import bits_per_dim_loop

    B = x_0.shape[0] if isinstance(x_0, torch.Tensor) and x_0.dim() else 2
    y, te = torch.arange(B), torch.zeros(B, 768)
    return {"loop": lambda: bits_per_dim_loop(_NoModel(), fp, x_0, **kw),
            "diffusion": lambda: D.bits_per_dim(_NoModel(), fp, x_0, **kw),
            "conditional_diffusion": lambda: C.bits_per_dim(_NoModel(), fp, x_0, y=y, **kw),
            "conditional_diffusion_laion": lambda: LA.bits_per_dim(_NoModel(), fp, x_0, text_embeds=te, **kw),
            "latent_diffusion": lambda: LD.bits_per_dim(_NoModel(), fp, x_0, y=y, **kw),
            "diffusion_transformer": lambda: DT.bits_per_dim(_NoModel(), fp, x_0, y=y, **kw)}


def _terms(fp, x_0, t=None, **kw):
    from tiny_diffusion_amd.likelihood import bits_per_dim_terms

    t = torch.zeros(x_0.shape[0], dtype=torch.int64) if t is None else t
    return lambda: bits_per_dim_terms(_NoModel(), fp, x_0, t, **kw)


X0 = torch.zeros(2, 20)
BAD_KW = [("variance", dict(variance="learned")), ("variance", dict(variance=None)), ("prediction", dict(prediction="x0")),
          ("bins", dict(bins=1)), ("bins", dict(bins=0)), ("bins", dict(bins=-256)), ("bins", dict(bins=2.5)),
          ("bins", dict(bins=True)), ("data_range", dict(data_range=(1, 1))), ("data_range", dict(data_range=(1, -1))),
          ("data_range", dict(data_range=(-INF, 1))), ("data_range", dict(data_range=(NAN, 1))),
          ("data_range", dict(data_range=(0, 1, 2))), ("data_range", dict(data_range=None)),
          ("clip_denoised", dict(clip_denoised=(1, -1))), ("clip_denoised", dict(clip_denoised=(NAN, 1))),
          ("philox_seed", dict(philox_seed=-1)), ("philox_seed", dict(philox_seed=0.5))]


@pytest.mark.parametrize("match,kw", BAD_KW, ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items()))
def test_keyword_errors_come_first_everywhere(match, kw):
    fp = _fp(6)
    for name, call in _loops(fp, X0, **kw).items():
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(ValueError, match=match):
        _terms(fp, X0, **kw)()


def test_sample_size_and_shape_errors():
    fp = _fp(6)
    for bad in (torch.zeros(2, 3), torch.zeros(2, 1, 3, 3), torch.zeros(2, 22)):
        for name, call in _loops(fp, bad).items():
            with pytest.raises(ValueError, match="multiple of 4"):
                call()
        with pytest.raises(ValueError, match="multiple of 4"):
            _terms(fp, bad)()
    for bad in (torch.zeros(20), torch.zeros(0, 20), [[0.0] * 20]):
        with pytest.raises(ValueError, match="x_0"):
            _loops(fp, bad)["loop"]()


def test_noise_errors():
    from tiny_diffusion_amd.likelihood import bits_per_dim_terms

    fp = _fp(6)
    good = [torch.zeros(2, 20)] * 6
    for bad in (good[:5], {t: good[t] for t in range(1, 6)}, good[:3] + [torch.zeros(2, 21)] + good[4:],
                good[:5] + [torch.zeros(1, 20)], good[:5] + [None], 3):
        for name, call in _loops(fp, X0, noises=bad).items():
            with pytest.raises(ValueError, match="noises"):
                call()
    for name, call in _loops(fp, X0, noises=good, philox_seed=1).items():
        with pytest.raises(ValueError, match="not both"):
            call()
    for bad in (torch.zeros(2, 21), torch.zeros(20), "eps"):
        with pytest.raises(ValueError, match="noise"):
            _terms(fp, X0, noise=bad)()
    with pytest.raises(ValueError, match="not both"):
        bits_per_dim_terms(_NoModel(), fp, X0, torch.zeros(2, dtype=torch.int64), noise=X0, philox_seed=1)


@pytest.mark.parametrize("t", [torch.tensor([0, 6]), torch.tensor([-1, 0]), torch.tensor([0, 1, 2]), torch.tensor([0.0, 1.0]),
                               torch.tensor(1), [0, 1], None], ids=repr)
def test_timestep_errors(t):
    from tiny_diffusion_amd.likelihood import bits_per_dim_terms

    with pytest.raises(ValueError, match="t must"):
        bits_per_dim_terms(_NoModel(), _fp(6), X0, t)


def test_a_conditional_model_needs_its_condition():
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import conditional_diffusion_laion as LA
    from tiny_diffusion_amd import diffusion_transformer as DT
    from tiny_diffusion_amd import latent_diffusion as LD
    from tiny_diffusion_amd.likelihood import bits_per_dim_loop, bits_per_dim_terms

    fp = _fp(6)
    for mod in (C, LD, DT):
        with pytest.raises(ValueError, match="labels"):
            mod.bits_per_dim(_NoModel(), fp, X0)
    with pytest.raises(ValueError, match="[Tt]ext embeddings"):
        LA.bits_per_dim(_NoModel(), fp, X0)
    with pytest.raises(ValueError, match="condition"):
        bits_per_dim_loop(_CondModel(), fp, X0)
    with pytest.raises(ValueError, match="condition"):
        bits_per_dim_terms(_CondModel(), fp, X0, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="one row per sample"):
        bits_per_dim_loop(_CondModel(), fp, X0, y=torch.arange(3))


def test_accepted_arguments_reach_the_device_check():
    """A CPU tensor is a TdxError, as in sampling - and only after every ValueError had its chance."""
    from tiny_diffusion_amd import _lib

    fp = _fp(6)
    noises = {t: torch.zeros(2, 20) for t in range(6)}
    for kw in (dict(), dict(noises=noises), dict(philox_seed=3), dict(variance="posterior", prediction="v"),
               dict(bins=256, clip_denoised=True, data_range=(0, 1)), dict(bins=None, clip_denoised=(-INF, INF))):
        for name, call in _loops(fp, X0, **kw).items():
            with pytest.raises(_lib.TdxError, match="GPU only"):
                call()
    for kw in (dict(), dict(noise=torch.zeros(2, 20)), dict(philox_seed=0), dict(bins=2)):
        with pytest.raises(_lib.TdxError, match="GPU only"):
            _terms(fp, X0, t=torch.tensor([0, 5]), **kw)()
    assert not issubclass(_lib.TdxError, ValueError)


def test_module_defaults():
    """Pixels: 256 bins and the clamp; latents: a continuous decoder and no clamp."""
    import inspect

    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import conditional_diffusion_laion as LA
    from tiny_diffusion_amd import diffusion as D
    from tiny_diffusion_amd import diffusion_transformer as DT
    from tiny_diffusion_amd import latent_diffusion as LD

    for mod, bins, clip in ((D, 256, True), (C, 256, True), (LA, None, None), (LD, None, None), (DT, None, None)):
        sig = inspect.signature(mod.bits_per_dim).parameters
        assert list(sig)[:3] == ["noise_model", "diffusion", "x_0"]
        assert sig["bins"].default == bins and sig["clip_denoised"].default is clip
        assert "bits_per_dim" in mod.__all__
