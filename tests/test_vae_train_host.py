"""VAE training, host side (no GPU): the new C entries are declared, listed and exported; the torch restatement of the
training step (tests/vae_helpers.py) reproduces the vectors the reference's own ``VAE`` / ``loss_function`` produced
(tests/golden/vae_train_B8.npz, tools/make_golden_vae.py); the BCE-from-logits form the kernel evaluates is the
reference's ``binary_cross_entropy(sigmoid(a))``; ``VAETrainStep``'s argument errors come before any device work."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_helpers as H
from oracle.weights import make_state_dict_vae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tdx_vae_loss_scratch_bytes", "tdx_vae_bce_logits_grad", "tdx_vae_kld_reparam_bwd",
               "tdx_vae_reparameterize_philox", "tdx_vae_train_workspace_floats", "tdx_vae_loss_grads")
RTOL, ATOL = 1e-5, 1e-6     # the bounds of test_oracle_latent.py


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "vae_train_B8.npz"))


def test_new_symbols_declared_listed_and_exported():
    import tiny_diffusion_amd._lib as L

    hdr = open(os.path.join(ROOT, "include", "tdx.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS, name
        assert getattr(L.lib, name).argtypes is not None, name   # bound: the library exports it
    assert L.lib.tdx_version() == 400   # the ABI only grows
    # sizes are host arithmetic: the workspace holds every activation, gradient and the loss scratch
    B, D, Hd, Ld = 8, 784, 400, 20
    n = L.lib.tdx_vae_train_workspace_floats(B, D, Hd, Ld)
    assert n >= B * (2 * D + 4 * Hd + 7 * Ld) + 2 * L.lib.tdx_vae_loss_scratch_bytes() // 4
    assert L.lib.tdx_vae_train_workspace_floats(0, D, Hd, Ld) == 0
    assert L.lib.tdx_vae_loss_scratch_bytes() % 8 == 0
    import tiny_diffusion_amd.vae as V
    from tiny_diffusion_amd.latent_diffusion import VAETrainStep

    assert VAETrainStep is V.VAETrainStep and "VAETrainStep" in V.__all__


def test_fixture_inputs_follow_the_recipe(fixture):
    x, eps = H.recipe_inputs(11, 8, n_eps=3)
    assert np.array_equal(fixture["x"], x.numpy()) and np.array_equal(fixture["eps"], torch.stack(eps).numpy())
    assert list(make_state_dict_vae(0)) == list(H.KEYS)


def test_fp32_restatement_reproduces_the_reference_one_step(fixture):
    sd = make_state_dict_vae(0)
    x, eps = torch.from_numpy(fixture["x"]), torch.from_numpy(fixture["eps"])
    r = H.loss_and_grads(sd, x, eps[0])
    for k in ("loss", "bce", "kld"):
        assert math.isclose(r[k], float(fixture[k]), rel_tol=RTOL, abs_tol=ATOL), k
    for k in H.KEYS:
        kk = k.replace(".", "__")
        g = r["grads"][k].reshape(-1)
        assert math.isclose(g.double().norm().item(), float(fixture[f"gnorm__{kk}"]), rel_tol=RTOL, abs_tol=ATOL), k
        head = torch.from_numpy(fixture[f"ghead__{kk}"])
        assert torch.allclose(g[: head.numel()], head, rtol=RTOL, atol=ATOL), k
    # the inputs are safe: no ReLU sits on a rounding error, no clamp of binary_cross_entropy binds
    margin, max_logit, max_logvar = H.input_margins(H.loss_and_grads(sd, x, eps[0], dtype=torch.float64)["aux"])
    assert margin >= 1e-4 and max_logit <= 15 and max_logvar <= 4


def test_fp32_restatement_reproduces_the_reference_three_adam_steps(fixture):
    sd = make_state_dict_vae(0)
    x, eps = torch.from_numpy(fixture["x"]), torch.from_numpy(fixture["eps"])
    losses, params = H.adam_steps(sd, x, list(eps), lr=1e-3)
    assert np.allclose(losses, fixture["adam_losses"], rtol=RTOL, atol=ATOL)
    assert losses[2] < losses[1] < losses[0]
    for k in H.KEYS:
        kk = k.replace(".", "__")
        v = params[k].reshape(-1)
        assert math.isclose(v.double().norm().item(), float(fixture[f"pnorm__{kk}"]), rel_tol=RTOL, abs_tol=ATOL), k
        head = torch.from_numpy(fixture[f"phead__{kk}"])
        assert torch.allclose(v[: head.numel()], head, rtol=RTOL, atol=ATOL), k


def test_logits_form_is_the_reference_bce_in_fp64():
    """max(a, 0) - a t + log1p(exp(-|a|))  ==  -t log s(a) - (1 - t) log(1 - s(a)) for |a| <= 30, to 1e-12 relative.

    torch's own evaluation ``F.binary_cross_entropy(torch.sigmoid(a), t)`` takes ``1 - s(a)`` from the ROUNDED s(a): for
    a > 0 that difference carries a relative error of 2^-53 e^a, so the literal call can agree to 1e-12 only while
    e^|a| 2^-53 << 1e-12 - measured here: 3e-13 for |a| <= 10, 3e-11 at 15, 2e-9 at 20, 3.4e-5 at a = 30 (the
    sigmoid form's error, not the logits form's: the logits form has no cancellation).  So the literal call is held to
    1e-12 on |a| <= 10, and on the whole range |a| <= 30 the same expression is evaluated from torch's own
    ``F.logsigmoid``, -t log s(a) - (1 - t) log s(-a), which does not form 1 - s(a) (nor log of an s(a) next to 1) from
    a rounded value; that comparison is held to 1e-12 per element and on the sum too.  Beyond |a| = 10 the literal call
    is within its own bound 4 (1 - t) 2^-53 e^a per element."""
    g = torch.Generator().manual_seed(0)
    n = 6272
    a = torch.rand(n, generator=g, dtype=torch.float64) * 60 - 30
    a[:8] = torch.tensor([0.0, -0.0, 20.0, -20.0, 30.0, -30.0, 10.0, -10.0], dtype=torch.float64)
    t = torch.rand(n, generator=g, dtype=torch.float64)
    t[8:12] = torch.tensor([0.0, 0.0, 0.5, 0.5], dtype=torch.float64)
    logits = a.clamp(min=0) - a * t + torch.log1p(torch.exp(-a.abs()))
    assert math.isclose(logits.sum().item(), H.bce_sum(a, t, "logits").item(), rel_tol=1e-15)
    # |a| <= 30: the reference's expression, log s(a) and log(1 - s(a)) = log s(-a) from torch's logsigmoid
    ident = -(t * F.logsigmoid(a) + (1 - t) * F.logsigmoid(-a))
    assert torch.allclose(ident, logits, rtol=1e-12, atol=0.0)
    assert abs(ident.sum().item() - logits.sum().item()) <= 1e-12 * logits.sum().item()
    # the literal call where its own rounding allows 1e-12
    lit = F.binary_cross_entropy(torch.sigmoid(a), t, reduction="none")
    m = a.abs() <= 10
    assert int(m.sum()) > 1000
    assert torch.allclose(lit[m], logits[m], rtol=1e-12, atol=0.0)
    assert abs(lit[m].sum().item() - logits[m].sum().item()) <= 1e-12 * logits[m].sum().item()
    assert math.isclose(H.bce_sum(a[m], t[m], "sigmoid").item(), logits[m].sum().item(), rel_tol=1e-12)
    # and everywhere within the error of its 1 - s(a)
    bound = 4 * (1 - t) * 2.0 ** -53 * torch.exp(a.clamp(min=0)) + 1e-12 * logits
    assert bool(((lit - logits).abs() <= bound).all())


def test_validation_errors_come_before_any_device_work():
    from tiny_diffusion_amd import _lib
    from tiny_diffusion_amd.vae import VAE, VAEConfig, VAETrainStep

    cfg = VAEConfig(device="cpu")
    vae = VAE(cfg)   # on the CPU: every ValueError below must come before the device is looked at
    for kw in (dict(kld_weight=-0.5), dict(kld_weight=float("nan")), dict(kld_weight="1"), dict(lr="1e-3"),
               dict(lr=None), dict(lr=True), dict(betas=(0.9, "x")), dict(betas=(0.9,)), dict(betas=0.9),
               dict(betas=(0.9, float("inf"))), dict(eps=None), dict(max_grad_norm=0.0), dict(philox_seed=-1),
               dict(philox_seed=1.5)):
        with pytest.raises(ValueError):
            VAETrainStep(vae, **kw)
    with pytest.raises(_lib.TdxError, match="CUDA"):
        VAETrainStep(vae)             # valid arguments, CPU module: no fallback
    assert vae.fc1.weight.device.type == "cpu" and vae.fc1.weight.shape == (400, 784)   # and nothing was touched
    x, eps = torch.zeros(4, 784), torch.zeros(4, 20)
    for bad in (torch.zeros(4, 21), torch.zeros(3, 20), torch.zeros(80), torch.zeros(4, 20, 1)):
        with pytest.raises(ValueError, match="eps"):
            VAETrainStep._check_batch(cfg, x, bad)
    for bad_x in (torch.zeros(4, 783), torch.zeros(784), torch.zeros(4, 1, 28, 27)):
        with pytest.raises(ValueError, match="x must"):
            VAETrainStep._check_batch(cfg, bad_x, None)
    with pytest.raises(_lib.TdxError, match="CPU tensor"):
        VAETrainStep._check_batch(cfg, x, eps)                       # right shapes, CPU tensors
    with pytest.raises(_lib.TdxError, match="CPU tensor"):
        VAETrainStep._check_batch(cfg, x.view(4, 1, 28, 28), None)
    assert issubclass(_lib.TdxError, RuntimeError) and not issubclass(_lib.TdxError, ValueError)
