"""Classifier-free guidance, host side (no GPU): argument errors of ``guidance_scale`` and ``cond_drop_prob`` are
raised before anything touches a device, and the new C entries are declared, listed and exported."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tdx_p_sample_step_guided", "tdx_unet_eval_step_update", "tdx_cond_drop_labels", "tdx_cond_drop_rows")


def test_new_symbols_declared_listed_and_exported():
    import tiny_diffusion_amd._lib as L

    hdr = open(os.path.join(ROOT, "include", "tdx.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS, name
        assert getattr(L.lib, name).argtypes is not None, name   # bound: the library exports it
    assert L.lib.tdx_version() == 400   # the ABI only grows


def _unsupported():
    """(module, call) pairs of the models without a null condition; the call takes sample()'s keywords."""
    from tiny_diffusion_amd import diffusion as D
    from tiny_diffusion_amd import diffusion_transformer as DT
    from tiny_diffusion_amd import latent_diffusion as LD
    from tiny_diffusion_amd.vae import VAE, VAEConfig

    y = torch.tensor([1, 2])
    vae = VAE(VAEConfig())
    out = []
    m = D.NoiseModel()
    out += [("diffusion.sample", lambda fp, **kw: D.sample(m, fp, "cuda", n_samples=2, **kw)),
            ("diffusion.ddim_sample", lambda fp, **kw: D.ddim_sample(m, fp, "cuda", n_samples=2, steps=3, **kw))]
    for name, mod in (("latent_diffusion", LD), ("diffusion_transformer", DT)):
        nm = mod.NoiseModel()
        out += [(name + ".sample", lambda fp, mod=mod, nm=nm, **kw: mod.sample(vae, nm, fp, "cuda", n_samples=2, y=y, **kw)),
                (name + ".ddim_sample",
                 lambda fp, mod=mod, nm=nm, **kw: mod.ddim_sample(vae, nm, fp, "cuda", n_samples=2, y=y, steps=3, **kw))]
    return out


def test_guidance_scale_is_refused_without_a_null_condition():
    from tiny_diffusion_amd.schedule import ForwardProcess, ddim_sample_loop, sample_loop

    fp = ForwardProcess(num_timesteps=4)
    for name, call in _unsupported():
        with pytest.raises(ValueError, match="guidance_scale"):
            call(fp, guidance_scale=2.0)
    # a module that is none of the project's models
    foreign = torch.nn.Linear(2, 2)
    for loop in (sample_loop, ddim_sample_loop):
        with pytest.raises(ValueError, match="guidance_scale"):
            loop(foreign, fp, "cuda", 2, torch.tensor([0, 1]), guidance_scale=1.0)


@pytest.mark.parametrize("w", [float("nan"), float("inf"), -float("inf"), "3", True, None])
def test_guidance_scale_must_be_finite(w):
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import conditional_diffusion_laion as L
    from tiny_diffusion_amd import _lib

    fp = C.ForwardProcess(num_timesteps=4)
    y = torch.tensor([1, 2])
    emb = torch.zeros(2, 768)
    calls = [lambda: C.sample(C.NoiseModel(), fp, "cpu", n_samples=2, y=y, guidance_scale=w),
             lambda: C.ddim_sample(C.NoiseModel(), fp, "cpu", n_samples=2, y=y, steps=2, guidance_scale=w),
             lambda: L.sample(L.NoiseModel(), fp, "cpu", text_embeds=emb, guidance_scale=w),
             lambda: L.ddim_sample(L.NoiseModel(), fp, "cpu", text_embeds=emb, steps=2, guidance_scale=w)]
    for call in calls:
        # None is no guidance: the call goes on to the device check (there is no CPU path); anything else that is
        # not a finite number is an argument error first
        with pytest.raises(_lib.TdxError if w is None else ValueError):
            call()


def test_finite_guidance_scale_passes_the_argument_checks():
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import _lib

    fp = C.ForwardProcess(num_timesteps=4)
    for w in (0.0, 1.0, -1.5, 7, 3.0):
        with pytest.raises(_lib.TdxError):   # reaches the device check
            C.sample(C.NoiseModel(), fp, "cpu", n_samples=2, y=torch.tensor([1, 2]), guidance_scale=w)


class _OnDevice:
    """Enough of a CUDA-resident model for TrainStep's argument checks, which come before it touches parameters."""

    def __init__(self, model):
        self._arch, self.num_classes = model._arch, model.num_classes


@pytest.mark.parametrize("p", [-0.1, 1.5, float("nan"), "0.1", True])
def test_cond_drop_prob_outside_unit_interval(p):
    from tiny_diffusion_amd.conditional_diffusion import ForwardProcess, NoiseModel
    from tiny_diffusion_amd.train import TrainStep

    with pytest.raises(ValueError, match="cond_drop_prob"):
        TrainStep(_OnDevice(NoiseModel()), ForwardProcess(), cond_drop_prob=p)


def test_cond_drop_prob_needs_a_condition():
    from tiny_diffusion_amd import diffusion as D
    from tiny_diffusion_amd import latent_diffusion as LD
    from tiny_diffusion_amd.train import TrainStep

    for m in (D.NoiseModel(), LD.NoiseModel()):
        with pytest.raises(ValueError, match="cond_drop_prob"):
            TrainStep(_OnDevice(m), D.ForwardProcess(), cond_drop_prob=0.1)
