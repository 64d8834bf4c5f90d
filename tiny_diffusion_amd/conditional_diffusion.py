"""Drop-in for the hot path of the reference's ``conditional_diffusion.py``
(class-conditional MNIST DDPM): same ``NoiseModel(time_dim, num_classes)``,
``forward(x, t, y)``, ``ForwardProcess`` and ``sample(..., y)`` contracts
(conditional_diffusion.py:19, 115, 174, 354-386)."""
from __future__ import annotations

from typing import Optional

import torch

from .likelihood import bits_per_dim_loop
from .schedule import ForwardProcess, ddim_sample_loop, dpm_sample_loop, sample_loop
from .unet import NoiseModelBase, TIME_DIM

__all__ = ["NoiseModel", "ForwardProcess", "sample", "ddim_sample", "dpm_sample", "bits_per_dim"]


class NoiseModel(NoiseModelBase):
    """eps_theta(x_t, t, y): time embedding + nn.Embedding(num_classes, 256)[y],
    conditional_diffusion.py:14-172.  A label ``y[n] = -1`` is the null condition (no class: the time embedding
    alone), what ``TrainStep(cond_drop_prob=...)`` trains and ``sample(guidance_scale=...)`` evaluates."""

    def __init__(self, time_dim: int = TIME_DIM, num_classes: int = 10):
        super().__init__(time_dim=time_dim, num_classes=num_classes)

    def forward(self, x, t, y):
        return self._forward_impl(x, t, y)


@torch.no_grad()
def sample(noise_model: NoiseModel, diffusion: ForwardProcess, device, n_samples=16, y=None,
           guidance_scale: Optional[float] = None, **kw):
    """conditional_diffusion.py:354-386, including its argument errors.  ``guidance_scale=w``: classifier-free
    guidance ``eps_u + w (eps_c - eps_u)`` against the null label (schedule.sample_loop); ``None``: none.
    ``clip_denoised=True | (lo, hi)`` (through ``**kw``, like ``prediction``): clipped-x0 sampling, which keeps guided
    samples inside the data range at w > 1 by pinning what leaves it to the ends of the range (``dynamic_threshold``
    below rescales instead).  ``known=x, mask=m`` (through ``**kw``; both or neither, broadcast to
    ``(n_samples, *input shape)``): inpainting - every step blends the implied x_0 with ``known`` where ``mask`` is 1 (a
    fraction: a soft edge) and the returned sample equals ``known`` there exactly; ``x_T`` stays pure noise - an
    image-to-image start composes from the existing ``x_T=`` and ``timesteps=`` arguments and is not part of this
    (schedule.sample_loop).  ``ddim_sample`` and ``dpm_sample`` take the two keywords too.  ``dynamic_threshold=q`` (through ``**kw``; q in (0, 1]): Imagen's dynamic thresholding on the range of
    ``clip_denoised`` ((-1, 1) when that is off) - per sample and step the q-quantile s of ``|x0 - centre|`` bounds the
    implied x_0 and, where it exceeds the half range h, scales it back by h / s (schedule.sample_loop); ``ddim_sample``
    and ``dpm_sample`` take it too.  ``variance=m`` (through ``**kw``; an ``EpsMoments`` of ``analytic.estimate_eps_moments``): the chain adds noise of
    the KL-optimal scale of this model (Bao et al. 2022, Analytic-DPM) instead of the schedule's - sigma is a table column, the mean of
    every step is unchanged (schedule.sample_loop); ``ddim_sample`` takes it too at ``eta`` > 0, ``dpm_sample`` is deterministic and refuses it."""
    _check_labels(y, n_samples)
    return sample_loop(noise_model, diffusion, device, n_samples, y, guidance_scale=guidance_scale, **kw)


@torch.no_grad()
def ddim_sample(noise_model: NoiseModel, diffusion: ForwardProcess, device, n_samples=16, y=None, steps=50, eta=0.0,
                timesteps=None, guidance_scale: Optional[float] = None, **kw):
    """DDIM sampling (Song et al. 2021): ``sample()``'s contract and argument errors over ``steps`` timesteps (or
    the explicit list ``timesteps``) with stochasticity ``eta`` (schedule.ddim_schedule); ``guidance_scale`` as in
    ``sample()``."""
    _check_labels(y, n_samples)
    return ddim_sample_loop(noise_model, diffusion, device, n_samples, y, steps=steps, eta=eta, timesteps=timesteps,
                            guidance_scale=guidance_scale, **kw)


@torch.no_grad()
def dpm_sample(noise_model: NoiseModel, diffusion: ForwardProcess, device, n_samples=16, y=None, steps=20, order=2,
               spacing="logsnr", timesteps=None, guidance_scale: Optional[float] = None, **kw):
    """DPM-Solver++(2M) sampling (Lu et al. 2022): ``sample()``'s contract and argument errors over ``steps`` timesteps uniform in
    log-SNR (``spacing="uniform"``: DDIM's spacing) or the explicit list ``timesteps``, deterministic, second order
    (``order=1``: deterministic DDIM), no retraining and one network evaluation per step (schedule.dpm_solver_schedule).
    ``guidance_scale`` as in ``sample()``."""
    _check_labels(y, n_samples)
    return dpm_sample_loop(noise_model, diffusion, device, n_samples, y, steps=steps, order=order, spacing=spacing,
                           timesteps=timesteps, guidance_scale=guidance_scale, **kw)


def bits_per_dim(noise_model: NoiseModel, diffusion: ForwardProcess, x_0, y=None, bins=256, clip_denoised=True, **kw):
    """The variational bound on the negative log-likelihood of ``x_0`` in bits per dimension (Ho et al. 2020 eq. 5;
    likelihood.bits_per_dim_loop): ``BitsPerDim(total_bpd, prior_bpd, vb, mse, xstart_mse)`` over all T timesteps,
    under the labels ``y``.  The defaults are Ho et al.'s and improved-DDPM's settings for pixels: the discretised decoder over 256 levels of
    [-1, 1] and the clamped x0 prediction.  ``noises`` / ``philox_seed``, ``prediction``, ``variance`` and
    ``data_range`` pass through.  ``variance`` may also be an ``EpsMoments`` (the KL-optimal variance of this model,
    analytic.py) and ``timesteps=[...]`` evaluates the bound of the K-step chain over an ascending sub-list (likelihood.bits_per_dim_loop)."""
    if y is None:
        raise ValueError("Class labels 'y' must be provided for conditional generation.")
    return bits_per_dim_loop(noise_model, diffusion, x_0, y, bins=bins, clip_denoised=clip_denoised, **kw)


def _check_labels(y, n_samples):
    if y is None:
        raise ValueError("Class labels 'y' must be provided for conditional generation.")
    if y.shape[0] != n_samples:
        raise ValueError("y must have shape (n_samples,)")
