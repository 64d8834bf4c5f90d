"""The training timestep sampler, host side (no GPU): the new C entries are declared, listed and bound; every argument
error of the constructor keywords and of ``load_timestep_sampler_state`` comes before any device work; the numpy
restatements (tests/timestep_helpers.py) against hand-worked cases; ``logit_normal_timestep_probs``."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import timestep_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tdx_timestep_cdf", "tdx_timestep_draw", "tdx_mse_per_sample", "tdx_timestep_history_update")


def test_new_symbols_declared_listed_and_bound():
    import tiny_diffusion_amd._lib as L

    hdr = open(os.path.join(ROOT, "include", "tdx.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS, name
        assert getattr(L.lib, name).argtypes is not None, name
    assert L.lib.tdx_version() == 400   # the ABI only grows
    # the argument checks answer before anything is launched (the pointers are never dereferenced)
    one, BAD = C.c_void_p(16), -1
    lib = L.lib
    assert lib.tdx_timestep_cdf(None, None, 1, one, one, 5, None) == BAD
    assert lib.tdx_timestep_cdf(one, None, 1, one, None, 5, None) == BAD
    assert lib.tdx_timestep_cdf(one, None, 1, one, one, 0, None) == BAD
    assert lib.tdx_timestep_draw(None, 5, one, None, 4, 0, 0, None, None) == BAD
    assert lib.tdx_timestep_draw(one, 5, None, None, 4, 0, 0, None, None) == BAD
    assert lib.tdx_timestep_draw(one, 0, one, None, 4, 0, 0, None, None) == BAD
    assert lib.tdx_timestep_draw(one, 5, one, None, 0, 0, 0, None, None) == BAD
    assert lib.tdx_mse_per_sample(None, one, one, None, one, 2, 8, None) == BAD
    assert lib.tdx_mse_per_sample(one, one, None, one, one, 2, 8, None) == BAD     # weights need t
    assert lib.tdx_mse_per_sample(one, one, one, None, None, 2, 8, None) == BAD
    assert lib.tdx_mse_per_sample(one, one, one, None, one, 0, 8, None) == BAD
    assert lib.tdx_mse_per_sample(one, one, one, None, one, 2, 0, None) == BAD
    hu = lambda *a: lib.tdx_timestep_history_update(*a, None)   # noqa: E731
    assert hu(None, one, 4, one, one, 3, 0.001, None, one, one, 5) == BAD          # B > 0 needs t and loss_b
    assert hu(one, one, 4, None, one, 3, 0.001, None, one, one, 5) == BAD
    assert hu(one, one, 4, one, one, 0, 0.001, None, one, one, 5) == BAD           # H < 1
    assert hu(one, one, 4, one, one, 3, 1.5, None, one, one, 5) == BAD
    assert hu(one, one, 4, one, one, 3, -0.1, None, one, one, 5) == BAD
    assert hu(one, one, 4, one, one, 3, float("nan"), None, one, one, 5) == BAD
    assert hu(one, one, -1, one, one, 3, 0.001, None, one, one, 5) == BAD
    assert hu(one, one, 4, one, one, 3, 0.001, None, one, one, 0) == BAD
    assert hu(one, one, 4, one, one, 3, 0.001, None, one, one, 4097) == -2         # TDX_E_SHAPE: T <= 4096


# ------------------------------------------------------------------ argument errors before device work
class _OnDevice:
    """Enough of a CUDA-resident model for TrainStep's argument checks, which come before it touches parameters."""

    def __init__(self, model):
        self._arch, self.num_classes = model._arch, model.num_classes


def _train_step(**kw):
    from tiny_diffusion_amd.conditional_diffusion import NoiseModel
    from tiny_diffusion_amd.schedule import ForwardProcess
    from tiny_diffusion_amd.train import TrainStep

    return TrainStep(_OnDevice(NoiseModel()), ForwardProcess(num_timesteps=20), **kw)


def _transformer_step(**kw):
    from tiny_diffusion_amd.diffusion_transformer import ForwardProcess, NoiseModel, TransformerTrainStep

    return TransformerTrainStep(NoiseModel(time_dim=64, num_layers=1), ForwardProcess(num_timesteps=20), **kw)


_nan = torch.full((20,), 0.05)
_nan[3] = float("nan")
_neg = torch.full((20,), 0.05)
_neg[0] = -0.05
BAD_KEYWORDS = [
    dict(timestep_sampler="uniform"), dict(timestep_sampler="loss-second-moment"), dict(timestep_sampler=1),
    dict(timestep_sampler=[0.05] * 20), dict(timestep_sampler=torch.ones(19)), dict(timestep_sampler=torch.ones(21)),
    dict(timestep_sampler=torch.ones(2, 10)), dict(timestep_sampler=np.ones(7)), dict(timestep_sampler=torch.zeros(20)),
    dict(timestep_sampler=_nan), dict(timestep_sampler=_neg), dict(timestep_sampler=torch.full((20,), float("inf"))),
    dict(timestep_sampler=torch.ones(20, dtype=torch.bool)), dict(timestep_sampler=torch.full((20,), 1e-60, dtype=torch.float64)),
    dict(importance_weights=1), dict(importance_weights="yes"),
    dict(timestep_seed=-1), dict(timestep_seed=2 ** 64), dict(timestep_seed=1.0), dict(timestep_seed=True),
    dict(timestep_seed=None),
    dict(history_per_term=0), dict(history_per_term=-3), dict(history_per_term=2.0), dict(history_per_term=True),
    dict(uniform_prob=-0.1), dict(uniform_prob=1.5), dict(uniform_prob=float("nan")), dict(uniform_prob="0.1"),
    dict(uniform_prob=True),
]


@pytest.mark.parametrize("make", [_train_step, _transformer_step])
def test_keyword_errors_come_before_any_device_work(make):
    for kw in BAD_KEYWORDS:
        for base in ({}, dict(timestep_sampler="loss_second_moment")):
            with pytest.raises(ValueError):
                make(**{**base, **kw})
    # valid keywords get past the checks and only then meet the missing device
    from tiny_diffusion_amd import _lib

    for kw in (dict(timestep_sampler="loss_second_moment"), dict(timestep_sampler=torch.ones(20), importance_weights=True),
               dict(timestep_sampler=np.full(20, 0.05), timestep_seed=2 ** 64 - 1, history_per_term=1, uniform_prob=1.0)):
        with pytest.raises((AttributeError, RuntimeError, _lib.TdxError)) as e:
            make(**kw)
        assert not isinstance(e.value, ValueError)


def _bare_step(sampler="loss_second_moment", T=6, H=3):
    """A TrainStep with nothing but its diffusion and its sampler keywords: no device."""
    from tiny_diffusion_amd.schedule import ForwardProcess
    from tiny_diffusion_amd.train import TrainStep

    step = object.__new__(TrainStep)
    step.diffusion = ForwardProcess(num_timesteps=T)
    step._check_timestep_sampler(sampler, None, 0, H, 0.001)
    return step


def test_keyword_defaults_and_recorded_values():
    step = _bare_step()
    assert step.timestep_sampler == "loss_second_moment" and step.importance_weights is True
    assert step.sample_losses is None and step.last_t is None and step._ts_cdf is None
    step = _bare_step(torch.tensor([0.0, 1, 2, 3, 2, 0]))
    assert step.timestep_sampler == "table" and step.importance_weights is False
    assert step._ts_probs_cpu.dtype == torch.float32 and step._ts_probs_cpu.tolist() == [0.0, 1, 2, 3, 2, 0]
    with pytest.raises(ValueError, match="4096"):      # the adaptive sampler's device entry covers T <= 4096
        _bare_step(T=4097)
    assert _bare_step(torch.ones(4097), T=4097).timestep_sampler == "table"
    step = _bare_step(None)
    assert step.timestep_sampler is None and step.importance_weights is False and step.sample_losses is None
    assert step._loss_table.__func__ is type(step)._loss_table      # and without a sampler the objective's own table
    step._w_table = "the objective's"
    assert step._loss_table() == "the objective's"


def test_load_state_errors_come_before_any_device_work():
    step = _bare_step()     # no device buffer exists: anything past the checks raises AttributeError / TypeError
    good = {"history": torch.zeros(6, 3), "counts": torch.zeros(6, dtype=torch.int32)}
    for bad in (None, 3, {}, {"history": good["history"]}, {"counts": good["counts"]},
                {**good, "history": torch.zeros(6, 2)}, {**good, "history": torch.zeros(5, 3)},
                {**good, "history": torch.zeros(6, 3, dtype=torch.int64)}, {**good, "counts": torch.zeros(5, dtype=torch.int32)},
                {**good, "counts": torch.zeros(6)}, {**good, "counts": torch.full((6,), 4)},
                {**good, "counts": torch.full((6,), -1)}, {**good, "history": torch.full((6, 3), float("nan"))}):
        with pytest.raises(ValueError):
            step.load_timestep_sampler_state(bad)
    with pytest.raises(Exception) as e:
        step.load_timestep_sampler_state(good)
    assert not isinstance(e.value, ValueError)
    for s in (_bare_step(None), _bare_step(torch.ones(6))):
        with pytest.raises(RuntimeError):
            s.timestep_sampler_state()
        with pytest.raises(RuntimeError):
            s.load_timestep_sampler_state(good)


# ------------------------------------------------------------------ the helpers against hand-worked cases
def test_philox_restatement_known_answers():
    """The Random123 known-answer vectors of philox4x32-10 (kat_vectors): counter / key all zero, and all ones."""
    z = H.philox4x32_10(0, 0, 0)
    assert [hex(int(v)) for v in z] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    f = H.philox4x32_10(2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1)
    assert [hex(int(v)) for v in f] == ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]
    # broadcasting over samples, and the uniform: 24 bits of word 1
    b = np.arange(5)
    blk = H.philox4x32_10(b, 7, 11)
    assert blk.shape == (5, 4) and all((blk[i] == H.philox4x32_10(i, 7, 11)).all() for i in range(5))
    u = H.uniform_of(11, 7, b)
    assert u.dtype == np.float32 and (u == (blk[:, 1] >> 8) / 2.0 ** 24).all() and (u < 1).all() and (u >= 0).all()


def test_history_hand_worked():
    """T = 3, H = 2: a duplicate timestep inside one batch, a ring wrap, the end of the warm-up."""
    r = H.LossSecondMoment(3, 2, uniform_prob=0.1)
    r.update([0, 0, 1], [1.0, 2.0, 3.0])
    hist, counts = r.state()
    assert counts.tolist() == [2, 1, 0] and hist[0].tolist() == [1.0, 2.0] and hist[1, 0] == 3.0
    assert not r.warmed_up() and r.weights().tolist() == [1 / 3] * 3
    cdf, w_eff = r.tables(np.array([2.0, 3.0, 4.0], dtype=np.float32))
    assert cdf.tolist() == [np.float32(1 / 3), np.float32(2 / 3), 1.0] and w_eff.tolist() == [2.0, 3.0, 4.0]
    r.update([0, 2, 2, 2, 1], [4.0, 5.0, 6.0, 7.0, 8.0])
    hist, counts = r.state()
    assert counts.tolist() == [2, 2, 2]
    assert hist.tolist() == [[2.0, 4.0], [3.0, 8.0], [6.0, 7.0]]      # oldest first; 1.0 and 5.0 were dropped
    w = np.sqrt(np.array([(4 + 16) / 2, (9 + 64) / 2, (36 + 49) / 2]))
    p = w / w.sum() * 0.9 + 0.1 / 3
    assert r.warmed_up() and np.allclose(r.weights(), p, rtol=1e-15, atol=0) and abs(p.sum() - 1) < 1e-15
    cdf, w_eff = r.tables()
    assert cdf[-1] == 1.0 and np.allclose(cdf, np.cumsum(p), rtol=1e-7) and np.allclose(w_eff, 1 / (3 * p), rtol=1e-7)


def test_cdf_zero_entries_and_chi_square():
    cdf = H.cdf_of([0, .5, 0, .5, 0])
    assert cdf.tolist() == [0.0, 0.5, 0.5, 1.0, 1.0]
    # trailing zeros are never drawn whatever the running sum rounds to: the rule, not luck
    p = np.array([0.1] * 10 + [0.0, 0.0])
    c = H.cdf_of(p)
    assert (c[9:] == 1.0).all() and (np.diff(c) >= 0).all()
    assert H.draw(c, np.float32(1 - 2.0 ** -24)) == 9
    assert H.draw(cdf, np.array([0.0, 0.49999997, 0.5, 0.99999994], dtype=np.float32)).tolist() == [1, 1, 3, 3]
    assert H.w_eff_of([0, .5, 0, .5, 0]).tolist() == [0.0, np.float32(0.4), 0.0, np.float32(0.4), 0.0]   # 1 / (5 * .5)
    u = H.uniform_of(20211, 3, np.arange(4096))     # the fixed key for which the statistic below was computed
    t = H.draw(cdf, u)
    n1, n3 = int((t == 1).sum()), int((t == 3).sum())
    assert n1 + n3 == 4096
    chi2 = (n1 - 2048) ** 2 / 2048 + (n3 - 2048) ** 2 / 2048
    print(f"4096 draws from [0, .5, 0, .5, 0]: {n1} / {n3}, chi-square {chi2:.3f} (0.999 quantile, 1 dof: 10.828)")
    assert chi2 < 10.828
    # word 1, not word 0: the uniforms are not the ones tdx_cond_drop_* compares with p
    assert not (u == (H.philox4x32_10(np.arange(4096), 3, 20211)[:, 0] >> 8) / 2.0 ** 24).all()


def test_logit_normal_timestep_probs():
    from tiny_diffusion_amd.schedule import logit_normal_timestep_probs, timestep_probs

    for T in (1, 2, 7, 1000):
        p = logit_normal_timestep_probs(T)
        assert p.dtype == torch.float64 and p.shape == (T,) and abs(float(p.sum()) - 1) < 1e-12 and bool((p > 0).all())
        assert torch.allclose(p, p.flip(0), rtol=1e-10, atol=0)      # mean 0: symmetric about the centre
        assert timestep_probs(T, p).dtype == torch.float32           # and it is a valid table
    p = logit_normal_timestep_probs(1001, std=0.5)   # std < 1 / sqrt 2: unimodal
    assert int(p.argmax()) == 500 and bool((p[:500].diff() > 0).all()) and bool((p[500:].diff() < 0).all())
    want = lambda t: np.exp(-0.5 * ((np.log((t + .5) / 1001) - np.log1p(-(t + .5) / 1001)) / 0.5) ** 2) / (    # noqa: E731
        ((t + .5) / 1001) * (1 - (t + .5) / 1001))
    assert abs(float(p[100] / p[500]) - want(100) / want(500)) < 1e-12 * want(100) / want(500) + 1e-15
    q = logit_normal_timestep_probs(1000, mean=1.0)
    assert float((q * torch.arange(1000)).sum()) > float((logit_normal_timestep_probs(1000) * torch.arange(1000)).sum())
    for bad in (dict(T=0), dict(T=2.5), dict(T=True), dict(T=10, std=0.0), dict(T=10, std=-1.0), dict(T=10, mean=float("nan")),
                dict(T=10, std="1")):
        with pytest.raises(ValueError):
            logit_normal_timestep_probs(**bad)
