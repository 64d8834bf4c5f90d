"""Dynamic thresholding, host side (no GPU): the new C entries are declared, listed and bound; the fp32 restatement of the
per-sample bound (tests/dynthr_helpers.py) against ``torch.quantile`` in double; the quantile's rank and fraction; the
``dynamic_threshold`` argument errors of the three loop functions and the module wrappers, before the device check."""
import math
import os
import re

import pytest
import torch

from dynthr_helpers import quantile_rank, threshold32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tdx_x0_dyn_threshold", "tdx_p_sample_update_dyn", "tdx_unet_eval_step_update_dyn")
INF = float("inf")


def _fp(T):
    from tiny_diffusion_amd.schedule import ForwardProcess

    return ForwardProcess(num_timesteps=T)


# ------------------------------------------------------------------ 1. ABI
def test_new_symbols_declared_listed_and_exported():
    import tiny_diffusion_amd._lib as L

    hdr = open(os.path.join(ROOT, "include", "tdx.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS, name
        assert getattr(L.lib, name).argtypes is not None, name   # bound: the library exports it
    assert len(L.lib.tdx_x0_dyn_threshold.argtypes) == 14
    assert len(L.lib.tdx_p_sample_update_dyn.argtypes) == len(L.lib.tdx_p_sample_update.argtypes) + 2
    assert len(L.lib.tdx_unet_eval_step_update_dyn.argtypes) == len(L.lib.tdx_unet_eval_step_update.argtypes) + 3
    assert L.lib.tdx_version() == 400   # the ABI only grows


# ------------------------------------------------------------------ 2. the restatement against fp64 torch.quantile
@pytest.mark.parametrize("kind", ["random", "tied", "constant"])
@pytest.mark.parametrize("per", [4, 20, 260, 784, 4096, 16384])
def test_restatement_agrees_with_fp64_quantile(per, kind):
    """s_q = a[rank] + frac (a[rank+1] - a[rank]) in fp32 is three roundings (the fraction, the product, the sum) away
    from the quantile of the same values in double: 2e-7 relative."""
    g = torch.Generator().manual_seed(per)
    u = 1.5 * torch.randn(3, per, generator=g)
    if kind == "tied":
        u = torch.round(u * 4) / 4
    elif kind == "constant":
        u = torch.full((3, per), -0.625) * torch.tensor([[1.0], [2.0], [0.0]])
    worst = 0.0
    for q in (0.001, 0.5, 0.9, 0.995, 1.0):
        rank, frac = quantile_rank(q, per)
        assert 0 <= rank <= per - 1 and 0.0 <= frac < 1.0
        _, _, sq = threshold32(u, -1.0, 1.0, rank, frac)
        want = torch.quantile(u.abs().double(), q, dim=1)
        rel = ((sq.double() - want).abs() / want.abs().clamp(min=1e-30)).max().item()
        worst = max(worst, rel)
        assert rel <= 2e-7, (per, kind, q, rel)
    print(f"per={per} {kind}: fp32 restatement vs fp64 torch.quantile, worst relative difference {worst:.2e}")


def test_threshold_of_the_restatement():
    """s = max(s_q, h), r = h / s: the static clamp (s = h, r = 1) wherever the quantile does not exceed h."""
    u = torch.tensor([[0.1, -0.2, 0.3, 4.0], [3.0, -2.0, 5.0, 0.5]])
    s, r, sq = threshold32(u, -1.0, 1.0, *quantile_rank(0.5, 4))
    assert sq.tolist() == [pytest.approx(0.25), 2.5] and s.tolist() == [1.0, 2.5] and r.tolist() == [1.0, pytest.approx(0.4)]
    s, r, _ = threshold32(u, -0.75, 0.5, *quantile_rank(1.0, 4))      # h = 0.625
    assert s.tolist() == [4.0, 5.0] and r.tolist() == [0.15625, 0.125]


# ------------------------------------------------------------------ 3. rank and fraction
def test_rank_and_fraction():
    from tiny_diffusion_amd.schedule import _quantile_rank

    for fn in (_quantile_rank, quantile_rank):
        for per in (4, 20, 784, 16384):
            assert fn(1.0, per) == (per - 1, 0.0)                     # q = 1: the maximum, no neighbour above
        assert fn(0.5, 21) == (10, 0.0) and fn(0.25, 5) == (1, 0.0)   # pos an integer
        assert fn(0.75, 5) == (3, 0.0)
        rank, frac = fn(0.995, 784)
        assert rank == 779 and frac == torch.tensor(0.995 * 783 - 779, dtype=torch.float64).float().item()
        rank, frac = fn(0.001, 20)
        assert rank == 0 and 0 < frac < 1
    for q in (0.001, 0.3, 0.5, 0.9, 0.995, 1.0):
        for per in (4, 20, 260, 784, 4096, 16384):
            assert _quantile_rank(q, per) == quantile_rank(q, per)


# ------------------------------------------------------------------ 4. argument errors
class _NoModel:
    def eval(self):
        raise AssertionError("the argument errors come before the model is touched")


class _NoVAE:
    def eval(self):
        pass


BAD = [True, False, float("nan"), 0, 0.0, -0.1, 1.5, INF, "0.9", (0.9,)]


def _calls(fp, **kw):
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import conditional_diffusion_laion as LA
    from tiny_diffusion_amd import diffusion as D
    from tiny_diffusion_amd import diffusion_transformer as DT
    from tiny_diffusion_amd import latent_diffusion as LD
    from tiny_diffusion_amd.schedule import ddim_sample_loop, dpm_sample_loop, sample_loop

    y = torch.tensor([1, 2])
    te = torch.zeros(2, 768)
    calls = [lambda: sample_loop(_NoModel(), fp, "cpu", 2, **kw),
             lambda: ddim_sample_loop(_NoModel(), fp, "cpu", 2, steps=5, **kw),
             lambda: dpm_sample_loop(_NoModel(), fp, "cpu", 2, steps=5, **kw),
             lambda: D.sample(_NoModel(), fp, "cpu", n_samples=2, **kw),
             lambda: D.ddim_sample(_NoModel(), fp, "cpu", n_samples=2, steps=5, **kw),
             lambda: D.dpm_sample(_NoModel(), fp, "cpu", n_samples=2, steps=5, **kw),
             lambda: C.sample(_NoModel(), fp, "cpu", n_samples=2, y=y, **kw),
             lambda: C.ddim_sample(_NoModel(), fp, "cpu", n_samples=2, y=y, steps=5, **kw),
             lambda: C.dpm_sample(_NoModel(), fp, "cpu", n_samples=2, y=y, steps=5, **kw),
             lambda: LA.sample(_NoModel(), fp, "cpu", text_embeds=te, **kw),
             lambda: LA.ddim_sample(_NoModel(), fp, "cpu", text_embeds=te, steps=5, **kw),
             lambda: LA.dpm_sample(_NoModel(), fp, "cpu", text_embeds=te, steps=5, **kw)]
    for mod in (LD, DT):
        calls += [lambda mod=mod: mod.sample(_NoVAE(), _NoModel(), fp, "cpu", n_samples=2, y=y, **kw),
                  lambda mod=mod: mod.ddim_sample(_NoVAE(), _NoModel(), fp, "cpu", n_samples=2, y=y, steps=5, **kw),
                  lambda mod=mod: mod.dpm_sample(_NoVAE(), _NoModel(), fp, "cpu", n_samples=2, y=y, steps=5, **kw)]
    return calls


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_dynamic_threshold_argument_errors_come_first(bad):
    from tiny_diffusion_amd.schedule import ddim_sample_loop, dpm_sample_loop

    fp = _fp(20)
    # a CPU device: the "GPU only" error would be a TdxError (not a ValueError), and it must not be reached
    for call in _calls(fp, dynamic_threshold=bad):
        with pytest.raises(ValueError, match="dynamic_threshold"):
            call()
    with pytest.raises(ValueError, match="dynamic_threshold"):     # before the schedule's own errors
        ddim_sample_loop(_NoModel(), fp, "cpu", 2, steps=0, dynamic_threshold=bad)
    with pytest.raises(ValueError, match="dynamic_threshold"):
        dpm_sample_loop(_NoModel(), fp, "cpu", 2, steps=0, dynamic_threshold=bad)


@pytest.mark.parametrize("clip", [(-INF, INF), (-1.0, INF), (-INF, 1.0)], ids=repr)
def test_an_infinite_bound_is_an_argument_error(clip):
    fp = _fp(20)
    for call in _calls(fp, dynamic_threshold=0.9, clip_denoised=clip):
        with pytest.raises(ValueError, match="finite data range"):
            call()
    for call in _calls(fp, dynamic_threshold=None, clip_denoised=clip):      # without the threshold they are allowed
        from tiny_diffusion_amd import _lib
        with pytest.raises(_lib.TdxError, match="GPU only"):
            call()


@pytest.mark.parametrize("good", [(None, None), (0.9, None), (1.0, False), (1e-6, True), (0.995, (-0.75, 0.5)), (1, None)],
                         ids=repr)
def test_accepted_values_reach_the_device_check(good):
    from tiny_diffusion_amd import _lib

    q, clip = good
    for call in _calls(_fp(20), dynamic_threshold=q, clip_denoised=clip):
        with pytest.raises(_lib.TdxError, match="GPU only"):
            call()
    assert issubclass(_lib.TdxError, RuntimeError) and not issubclass(_lib.TdxError, ValueError)


def test_dynamic_threshold_values():
    import numpy as np

    from tiny_diffusion_amd.schedule import _dynamic_threshold

    assert _dynamic_threshold(None) is None and _dynamic_threshold(None, (-INF, INF)) is None
    assert _dynamic_threshold(0.9) == (0.9, (-1.0, 1.0)) and _dynamic_threshold(1) == (1.0, (-1.0, 1.0))
    assert _dynamic_threshold(np.float32(0.5), (-0.75, 0.5)) == (0.5, (-0.75, 0.5))
    for bad in BAD + [np.bool_(True), None.__class__, 1 + 1e-9, -math.inf]:
        with pytest.raises(ValueError, match="dynamic_threshold"):
            _dynamic_threshold(bad)
