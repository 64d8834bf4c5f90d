"""Drop-in for the hot path of the reference's ``latent_diffusion.py`` (class-conditional DDPM
on the 20-d latents of the MLP VAE): ``NoiseModel(time_dim, num_classes, latent_dim)`` with
``forward(x, t, y)``, ``ForwardProcess`` (2-D ``q_sample``) and
``sample(vae, noise_model, diffusion, device, n_samples, y)`` (latent_diffusion.py:16-128,
131-154, 308-347)."""
from __future__ import annotations

import torch

from .likelihood import bits_per_dim_loop
from .schedule import ForwardProcess, ddim_sample_loop, dpm_sample_loop, sample_loop
from .unet import ARCH_LATENT, NoiseModelBase
from .vae import VAE, VAEConfig, VAETrainStep

__all__ = ["NoiseModel", "ForwardProcess", "sample", "ddim_sample", "dpm_sample", "bits_per_dim", "VAE", "VAEConfig",
           "VAETrainStep"]


class NoiseModel(NoiseModelBase):
    """eps_theta(z_t, t, y): 15 Linear, 13 BatchNorm1d, time/class signal added on the decoder
    path (latent_diffusion.py:16-128)."""

    def __init__(self, time_dim: int = ARCH_LATENT.time_dim, num_classes: int = 10, latent_dim: int = 20):
        if latent_dim != ARCH_LATENT.in_shape[0]:
            raise ValueError(f"libtdx is built for latent_dim={ARCH_LATENT.in_shape[0]} (reference default)")
        super().__init__(time_dim=time_dim, num_classes=num_classes, arch=ARCH_LATENT)
        self.latent_dim = latent_dim

    def forward(self, x, t, y):
        return self._forward_impl(x, t, y)


@torch.no_grad()
def sample(vae: VAE, noise_model: NoiseModel, diffusion: ForwardProcess, device, n_samples=16, y=None, **kw):
    """latent_diffusion.py:308-347: reverse loop over z (n,20), then ``vae.decode(z)`` viewed
    as (n,1,28,28); same argument errors.  ``sample_loop``'s extension keywords pass through (``clip_denoised=(lo, hi)``
    clamps the implied z_0, in the latent's own range).  ``known=x, mask=m`` (through ``**kw``; both or neither, broadcast to
    ``(n_samples, *(20,))``): inpainting - every step blends the implied z_0 with ``known`` where ``mask`` is 1 (a
    fraction: a soft edge) and the latent z handed to the decoder equals ``known`` there exactly; ``x_T`` stays pure noise - an
    image-to-image start composes from the existing ``x_T=`` and ``timesteps=`` arguments and is not part of this
    (schedule.sample_loop).  ``ddim_sample`` and ``dpm_sample`` take the two keywords too.  ``dynamic_threshold=q`` (through ``**kw``; q in (0, 1]): Imagen's dynamic thresholding on the range of
    ``clip_denoised`` ((-1, 1) when that is off) - per sample and step the q-quantile s of ``|x0 - centre|`` bounds the
    implied z_0 and, where it exceeds the half range h, scales it back by h / s (schedule.sample_loop); ``ddim_sample``
    and ``dpm_sample`` take it too.  ``variance=m`` (through ``**kw``; an ``EpsMoments`` of ``analytic.estimate_eps_moments``): the chain adds noise of
    the KL-optimal scale of this model (Bao et al. 2022, Analytic-DPM) instead of the schedule's - sigma is a table column, the mean of
    every step is unchanged (schedule.sample_loop); ``ddim_sample`` takes it too at ``eta`` > 0, ``dpm_sample`` is deterministic and refuses it."""
    _check_labels(y, n_samples)
    vae.eval()
    z = sample_loop(noise_model, diffusion, device, n_samples, y, **kw)
    return vae.decode(z).view(-1, 1, 28, 28)


@torch.no_grad()
def ddim_sample(vae: VAE, noise_model: NoiseModel, diffusion: ForwardProcess, device, n_samples=16, y=None, steps=50,
                eta=0.0, timesteps=None, **kw):
    """DDIM sampling (Song et al. 2021): ``sample()``'s contract, argument errors and VAE decode over ``steps``
    timesteps (or the explicit list ``timesteps``) with stochasticity ``eta`` (schedule.ddim_schedule)."""
    _check_labels(y, n_samples)
    vae.eval()
    z = ddim_sample_loop(noise_model, diffusion, device, n_samples, y, steps=steps, eta=eta, timesteps=timesteps, **kw)
    return vae.decode(z).view(-1, 1, 28, 28)


@torch.no_grad()
def dpm_sample(vae: VAE, noise_model: NoiseModel, diffusion: ForwardProcess, device, n_samples=16, y=None, steps=20,
               order=2, spacing="logsnr", timesteps=None, **kw):
    """DPM-Solver++(2M) sampling (Lu et al. 2022): ``sample()``'s contract, argument errors and VAE decode over ``steps`` timesteps uniform in
    log-SNR (``spacing="uniform"``: DDIM's spacing) or the explicit list ``timesteps``, deterministic, second order
    (``order=1``: deterministic DDIM), no retraining and one network evaluation per step (schedule.dpm_solver_schedule).
    The extension keywords of ``sample()`` except ``noises``."""
    _check_labels(y, n_samples)
    vae.eval()
    z = dpm_sample_loop(noise_model, diffusion, device, n_samples, y, steps=steps, order=order, spacing=spacing,
                        timesteps=timesteps, **kw)
    return vae.decode(z).view(-1, 1, 28, 28)


def bits_per_dim(noise_model: NoiseModel, diffusion: ForwardProcess, x_0, y=None, bins=None, clip_denoised=None, **kw):
    """The variational bound on the negative log-density of the latents ``x_0`` in bits per dimension (Ho et al. 2020
    eq. 5; likelihood.bits_per_dim_loop): ``BitsPerDim(total_bpd, prior_bpd, vb, mse, xstart_mse)`` over all T timesteps
    under the condition ``y``.  The defaults suit latents: a continuous Gaussian decoder at t = 0 and no clamp, so
    the result is a density and can be negative.  ``noises`` / ``philox_seed``, ``prediction``, ``variance``, ``bins``
    and ``data_range`` pass through.  ``variance`` may also be an ``EpsMoments`` (the KL-optimal variance of this model,
    analytic.py) and ``timesteps=[...]`` evaluates the bound of the K-step chain over an ascending sub-list (likelihood.bits_per_dim_loop)."""
    if y is None:
        raise ValueError("Class labels 'y' must be provided for conditional generation.")
    return bits_per_dim_loop(noise_model, diffusion, x_0, y, bins=bins, clip_denoised=clip_denoised, **kw)


def _check_labels(y, n_samples):
    if y is None:
        raise ValueError("Class labels 'y' must be provided for conditional generation.")
    if y.shape[0] != n_samples:
        raise ValueError("y must have shape (n_samples,)")
