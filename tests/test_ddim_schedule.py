"""DDIM timestep schedules on the host (schedule.ddim_schedule / ddpm_schedule): spacing, argument errors,
the coefficient rows against a fp64 restatement of Song et al. 2021 eq. 12 in x0 form, and the C ABI of the
scheduled device path.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

from tiny_diffusion_amd.schedule import ForwardProcess, ddim_schedule, ddpm_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tdx_step_begin_sched", "tdx_p_sample_step_sched", "tdx_p_sample_step_sched_philox",
               "tdx_unet_prepare_sampling_sched", "tdx_unet_eval_step_update")


@pytest.mark.parametrize("S", [1, 7, 10, 50, 1000])
def test_default_spacing(S):
    fp = ForwardProcess()
    s = ddim_schedule(fp, steps=S)
    assert s.timesteps.dtype == torch.int64 and s.timesteps.shape == (S,)
    assert s.timesteps.tolist() == [i * 1000 // S for i in range(S)]
    if 1000 % S == 0:
        assert s.timesteps.tolist() == list(range(0, 1000, 1000 // S))
    if S == 1000:
        assert s.timesteps.tolist() == list(range(1000))
    assert s.coef.dtype == torch.float32 and s.coef.shape == (S, 3)
    assert s.coef64.dtype == torch.float64 and torch.equal(s.coef, s.coef64.float())
    assert s.steps == S and s.num_timesteps == 1000


def test_explicit_timesteps():
    fp = ForwardProcess()
    for ts in ([0, 5, 999], (3,), np.array([1, 2, 3]), torch.tensor([10, 500])):
        s = ddim_schedule(fp, timesteps=ts)
        assert s.timesteps.tolist() == [int(v) for v in ts]


@pytest.mark.parametrize("kw", [
    dict(timesteps=[]),
    dict(timesteps=[5, 3]),
    dict(timesteps=[3, 3]),
    dict(timesteps=[-1, 3]),
    dict(timesteps=[0, 1000]),
    dict(timesteps=[0, 2.5]),
    dict(timesteps=[0.0, 2.0]),
    dict(timesteps=torch.tensor([0.0, 5.0])),
    dict(timesteps=np.array([0.0, 5.0])),
    dict(timesteps=[0, True]),
    dict(steps=10, timesteps=[0, 5]),
    dict(),
    dict(steps=0),
    dict(steps=1001),
    dict(steps=2.0),
    dict(steps=10, eta=-0.1),
    dict(steps=10, eta=float("nan")),
    dict(steps=10, eta=3.0),          # 1 - ab_prev - sigma^2 < 0
])
def test_validation_errors(kw):
    with pytest.raises(ValueError):
        ddim_schedule(ForwardProcess(), **kw)


def _x0_form(ab, ab_prev, eta, x, eps, z):
    """Song et al. 2021 eq. 12 (with eq. 16's sigma), fp64."""
    sigma = eta * np.sqrt((1 - ab_prev) / (1 - ab)) * np.sqrt(1 - ab / ab_prev)
    x0 = (x - np.sqrt(1 - ab) * eps) / np.sqrt(ab)
    return np.sqrt(ab_prev) * x0 + np.sqrt(1 - ab_prev - sigma ** 2) * eps + sigma * z


@pytest.mark.parametrize("S,eta", [(10, 0.0), (10, 1.0), (50, 0.5), (7, 1.0), (1000, 1.0), (1, 0.0)])
def test_coefficients_match_x0_form(S, eta):
    fp = ForwardProcess()
    s = ddim_schedule(fp, steps=S, eta=eta)
    acp = fp.alphas_cumprod.double().numpy()
    rs = np.random.RandomState(S)
    tau = s.timesteps.tolist()
    for k in range(S):
        ab = acp[tau[k]]
        ab_prev = acp[tau[k - 1]] if k > 0 else 1.0
        x, eps, z = rs.randn(3, 256)
        c1, c2, sg = s.coef64[k].tolist()
        got = c1 * (x - c2 * eps) + sg * z
        want = _x0_form(ab, ab_prev, eta, x, eps, z)
        rel = np.abs(got - want).max() / np.abs(want).max()
        assert rel < 1e-12, (k, rel)


def test_eta_zero_and_last_row():
    fp = ForwardProcess()
    s0 = ddim_schedule(fp, steps=10, eta=0.0)
    assert (s0.coef[:, 2] == 0).all() and (s0.coef64[:, 2] == 0).all()
    s1 = ddim_schedule(fp, steps=10, eta=1.0)
    assert s1.coef64[0, 2] == 0 and (s1.coef64[1:, 2] > 0).all()


def test_ddpm_schedule_is_the_reference_update():
    for T in (1000, 20, 3):
        fp = ForwardProcess(num_timesteps=T)
        s = ddpm_schedule(fp)
        assert s.timesteps.tolist() == list(range(T))
        assert torch.equal(s.coef, fp.tables("cpu")[2])


def test_new_symbols_declared_listed_and_exported():
    from tiny_diffusion_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "tdx.h")).read()
    declared = set(re.findall(r"^\w[\w\s\*]*?\b(tdx_\w+)\s*\(", hdr, flags=re.M))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(_lib.lib, name) is not None, name
    assert _lib.lib.tdx_version() == 400


def test_wrappers_exported():
    from tiny_diffusion_amd import (conditional_diffusion, conditional_diffusion_laion, diffusion,
                                    diffusion_transformer, latent_diffusion)

    for mod in (diffusion, conditional_diffusion, conditional_diffusion_laion, latent_diffusion, diffusion_transformer):
        assert "ddim_sample" in mod.__all__ and callable(mod.ddim_sample), mod.__name__
