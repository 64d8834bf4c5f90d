"""Drop-in for the hot path of the reference's ``diffusion.py`` (unconditional
MNIST DDPM): ``NoiseModel``, ``ForwardProcess``, ``sample`` with the same
signatures (diffusion.py:16, 109, 166, 177, 255), computed by libtdx on MI355X."""
from __future__ import annotations

import torch

from .likelihood import bits_per_dim_loop
from .schedule import ForwardProcess, ddim_sample_loop, dpm_sample_loop, sample_loop
from .unet import NoiseModelBase, TIME_DIM

__all__ = ["NoiseModel", "ForwardProcess", "sample", "ddim_sample", "dpm_sample", "bits_per_dim"]


class NoiseModel(NoiseModelBase):
    """UNet noise predictor eps_theta(x_t, t), diffusion.py:11-162."""

    def __init__(self, time_dim: int = TIME_DIM):
        super().__init__(time_dim=time_dim, num_classes=0)

    def forward(self, x, t):
        return self._forward_impl(x, t, None)


@torch.no_grad()
def sample(noise_model: NoiseModel, diffusion: ForwardProcess, device, n_samples=16, **kw):
    """diffusion.py:254-276: leaves the model in eval mode, returns x_0 in ~[-1, 1].
    Extra keyword arguments (x_T, noises, use_graph, philox_seed, prediction, clip_denoised) are extensions;
    ``clip_denoised=True | (lo, hi)`` clamps the implied x_0 at every step (schedule.sample_loop) and returns x_0 in
    [-1, 1] / [lo, hi] exactly.  ``known=x, mask=m`` (both or neither, broadcast to ``(n_samples, *input shape)``) is
    inpainting: every step blends the implied x_0 with ``known`` where ``mask`` is 1 (a fraction: a soft edge) and the
    returned sample equals ``known`` there exactly; ``x_T`` stays pure noise - an image-to-image start composes from the
    existing ``x_T=`` and ``timesteps=`` arguments and is not part of this (schedule.sample_loop).  ``dynamic_threshold=q`` (through ``**kw``; q in (0, 1]): Imagen's dynamic thresholding on the range of
    ``clip_denoised`` ((-1, 1) when that is off) - per sample and step the q-quantile s of ``|x0 - centre|`` bounds the
    implied x_0 and, where it exceeds the half range h, scales it back by h / s (schedule.sample_loop); ``ddim_sample``
    and ``dpm_sample`` take it too.  ``variance=m`` (through ``**kw``; an ``EpsMoments`` of ``analytic.estimate_eps_moments``): the chain adds noise of
    the KL-optimal scale of this model (Bao et al. 2022, Analytic-DPM) instead of the schedule's - sigma is a table column, the mean of
    every step is unchanged (schedule.sample_loop); ``ddim_sample`` takes it too at ``eta`` > 0, ``dpm_sample`` is deterministic and refuses it."""
    return sample_loop(noise_model, diffusion, device, n_samples, None, **kw)


@torch.no_grad()
def ddim_sample(noise_model: NoiseModel, diffusion: ForwardProcess, device, n_samples=16, steps=50, eta=0.0,
                timesteps=None, **kw):
    """DDIM sampling (Song et al. 2021) of a model trained with ``diffusion``: ``sample()``'s contract over
    ``steps`` timesteps (or the explicit list ``timesteps``) with stochasticity ``eta`` (schedule.ddim_schedule).
    The same extension keywords as ``sample()``, ``known`` / ``mask`` among them."""
    return ddim_sample_loop(noise_model, diffusion, device, n_samples, None, steps=steps, eta=eta,
                            timesteps=timesteps, **kw)


@torch.no_grad()
def dpm_sample(noise_model: NoiseModel, diffusion: ForwardProcess, device, n_samples=16, steps=20, order=2,
               spacing="logsnr", timesteps=None, **kw):
    """DPM-Solver++(2M) sampling (Lu et al. 2022): ``sample()``'s contract over ``steps`` timesteps uniform in
    log-SNR (``spacing="uniform"``: DDIM's spacing) or the explicit list ``timesteps``, deterministic, second order
    (``order=1``: deterministic DDIM), no retraining and one network evaluation per step (schedule.dpm_solver_schedule).
    The extension keywords of ``sample()`` except ``noises`` (``known`` / ``mask``: the history holds the blended
    prediction); ``philox_seed`` only selects the graph mode."""
    return dpm_sample_loop(noise_model, diffusion, device, n_samples, None, steps=steps, order=order, spacing=spacing,
                           timesteps=timesteps, **kw)


def bits_per_dim(noise_model: NoiseModel, diffusion: ForwardProcess, x_0, bins=256, clip_denoised=True, **kw):
    """The variational bound on the negative log-likelihood of ``x_0`` in bits per dimension (Ho et al. 2020 eq. 5;
    likelihood.bits_per_dim_loop): ``BitsPerDim(total_bpd, prior_bpd, vb, mse, xstart_mse)`` over all T timesteps.
    The defaults are Ho et al.'s and improved-DDPM's settings for pixels: the discretised decoder over 256 levels of
    [-1, 1] and the clamped x0 prediction.  ``noises`` / ``philox_seed``, ``prediction``, ``variance`` and
    ``data_range`` pass through.  ``variance`` may also be an ``EpsMoments`` (the KL-optimal variance of this model,
    analytic.py) and ``timesteps=[...]`` evaluates the bound of the K-step chain over an ascending sub-list (likelihood.bits_per_dim_loop)."""
    return bits_per_dim_loop(noise_model, diffusion, x_0, None, bins=bins, clip_denoised=clip_denoised, **kw)
