"""Drop-in for the hot path of the reference's ``conditional_diffusion_laion.py``
(text-conditioned latent DDPM): the same ``get_timestep_embedding``,
``NoiseModel(time_dim=768)`` with ``forward(x, t, text_embeds)``, ``ForwardProcess`` and
``sample(noise_model, diffusion, device, text_embeds, vae, scaling_factor)`` contracts
(conditional_diffusion_laion.py:222-232, 234-332, 335-358, 561-600).

Only the noise predictor and the reverse loop run on libtdx; the pretrained VAE and CLIP
text encoder the reference pulls from ``diffusers`` / ``transformers`` are external models
and stay whatever object the caller passes in (out of scope)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .likelihood import bits_per_dim_loop
from .schedule import ForwardProcess as _ForwardProcess, ddim_sample_loop, dpm_sample_loop, sample_loop
from .unet import ARCH_LAION, NoiseModelBase

__all__ = ["NoiseModel", "ForwardProcess", "get_timestep_embedding", "sample", "ddim_sample", "dpm_sample", "bits_per_dim",
           "postprocess_images"]

TIME_DIM = ARCH_LAION.time_dim


def get_timestep_embedding(timesteps, embedding_dim):
    """conditional_diffusion_laion.py:222-232 on the device: ``tdx_timestep_embedding`` (the kernel
    the model's own time path runs).  (N,) timesteps -> (N, embedding_dim) fp32.  Integer timesteps go
    through the int64 kernel; floating-point ones (the reference takes ``timesteps[:, None].float()``, so a
    fractional t keeps its fraction) through ``tdx_timestep_embedding_f32``.  A CPU tensor raises: this
    package has no host path."""
    if not timesteps.is_cuda:
        raise _lib.TdxError("get_timestep_embedding runs on the GPU only (no CPU fallback)")
    if timesteps.is_floating_point():
        t, fn, name = timesteps.contiguous().to(torch.float32), _lib.lib.tdx_timestep_embedding_f32, "tdx_timestep_embedding_f32"
    else:
        t, fn, name = timesteps.contiguous().to(torch.int64), _lib.lib.tdx_timestep_embedding, "tdx_timestep_embedding"
    out = torch.empty((t.shape[0], int(embedding_dim)), dtype=torch.float32, device=t.device)
    if t.shape[0]:
        _lib.check(fn(t.data_ptr(), out.data_ptr(), t.shape[0], int(embedding_dim),
                      torch.cuda.current_stream(t.device).cuda_stream), name)
    return out


class NoiseModel(NoiseModelBase):
    """eps_theta(x_t, t, text_embeds) on (4,32,32) latents: sinusoidal embedding -> time_mlp,
    + text_embeds, UNet 32/64/128/256 (conditional_diffusion_laion.py:234-332).  The condition enters only as
    ``emb = t_emb + text_embeds``, so an all-zero ``text_embeds`` row is the null condition: what
    ``TrainStep(cond_drop_prob=...)`` trains and ``sample(guidance_scale=...)`` evaluates."""

    def __init__(self, time_dim: int = TIME_DIM):
        super().__init__(time_dim=time_dim, num_classes=0, arch=ARCH_LAION)

    def forward(self, x, t, text_embeds):
        return self._forward_impl(x, t, text_embeds)


class ForwardProcess(_ForwardProcess):
    """conditional_diffusion_laion.py:335-358 (q_sample(device, x_0, t) draws its own noise)."""


def postprocess_images(decoded):
    """(decoded / 2 + 0.5).clamp(0, 1) with NaN/Inf replaced by zeros, fp32
    (conditional_diffusion_laion.py:590-599)."""
    images = (decoded / 2 + 0.5).clamp(0, 1)
    images = torch.where(torch.logical_or(torch.isnan(images), torch.isinf(images)),
                         torch.zeros_like(images), images)
    return images.to(torch.float32)


@torch.no_grad()
def sample(noise_model: NoiseModel, diffusion: ForwardProcess, device, text_embeds=None, vae=None,
           scaling_factor=1.0, guidance_scale: Optional[float] = None, **kw):
    """conditional_diffusion_laion.py:561-600: the reverse loop over latents, then
    ``vae.decode(x / scaling_factor).sample`` and the image post-processing.  With
    ``vae=None`` the latents are returned (the decoder is an external pretrained model).
    ``guidance_scale=w``: classifier-free guidance ``eps_u + w (eps_c - eps_u)`` against the all-zero text
    embedding (schedule.sample_loop); ``None``: none.  ``clip_denoised=(lo, hi)`` (through ``**kw``): clipped-x0
    sampling with the latents' own range (``True`` is [-1, 1], the range of pixel data).  ``known=x, mask=m`` (through ``**kw``; both or neither, broadcast to
    ``(n_samples, *(4, H, W))``): inpainting - every step blends the implied latent x_0 with ``known`` where ``mask`` is 1 (a
    fraction: a soft edge) and the latent the loop returns (before the decode) equals ``known`` there exactly; ``x_T`` stays pure noise - an
    image-to-image start composes from the existing ``x_T=`` and ``timesteps=`` arguments and is not part of this
    (schedule.sample_loop).  ``ddim_sample`` and ``dpm_sample`` take the two keywords too.  ``dynamic_threshold=q`` (through ``**kw``; q in (0, 1]): Imagen's dynamic thresholding on the range of
    ``clip_denoised`` ((-1, 1) when that is off) - per sample and step the q-quantile s of ``|x0 - centre|`` bounds the
    implied latent x_0 and, where it exceeds the half range h, scales it back by h / s (schedule.sample_loop); ``ddim_sample``
    and ``dpm_sample`` take it too.  ``variance=m`` (through ``**kw``; an ``EpsMoments`` of ``analytic.estimate_eps_moments``): the chain adds noise of
    the KL-optimal scale of this model (Bao et al. 2022, Analytic-DPM) instead of the schedule's - sigma is a table column, the mean of
    every step is unchanged (schedule.sample_loop); ``ddim_sample`` takes it too at ``eta`` > 0, ``dpm_sample`` is deterministic and refuses it."""
    if text_embeds is None:
        raise ValueError("Text embeddings must be provided for conditional generation.")
    n_samples = text_embeds.shape[0]
    x = sample_loop(noise_model, diffusion, device, n_samples, text_embeds, guidance_scale=guidance_scale, **kw)
    return _decode(x, vae, scaling_factor)


@torch.no_grad()
def ddim_sample(noise_model: NoiseModel, diffusion: ForwardProcess, device, text_embeds=None, vae=None,
                scaling_factor=1.0, steps=50, eta=0.0, timesteps=None, guidance_scale: Optional[float] = None, **kw):
    """DDIM sampling (Song et al. 2021): ``sample()``'s contract, argument errors and decode over ``steps`` timesteps
    (or the explicit list ``timesteps``) with stochasticity ``eta`` (schedule.ddim_schedule); ``guidance_scale`` as
    in ``sample()``."""
    if text_embeds is None:
        raise ValueError("Text embeddings must be provided for conditional generation.")
    n_samples = text_embeds.shape[0]
    x = ddim_sample_loop(noise_model, diffusion, device, n_samples, text_embeds, steps=steps, eta=eta,
                         timesteps=timesteps, guidance_scale=guidance_scale, **kw)
    return _decode(x, vae, scaling_factor)


@torch.no_grad()
def dpm_sample(noise_model: NoiseModel, diffusion: ForwardProcess, device, text_embeds=None, vae=None,
               scaling_factor=1.0, steps=20, order=2, spacing="logsnr", timesteps=None,
               guidance_scale: Optional[float] = None, **kw):
    """DPM-Solver++(2M) sampling (Lu et al. 2022): ``sample()``'s contract, argument errors and decode over ``steps`` timesteps uniform in
    log-SNR (``spacing="uniform"``: DDIM's spacing) or the explicit list ``timesteps``, deterministic, second order
    (``order=1``: deterministic DDIM), no retraining and one network evaluation per step (schedule.dpm_solver_schedule).
    ``guidance_scale`` as in ``sample()``."""
    if text_embeds is None:
        raise ValueError("Text embeddings must be provided for conditional generation.")
    n_samples = text_embeds.shape[0]
    x = dpm_sample_loop(noise_model, diffusion, device, n_samples, text_embeds, steps=steps, order=order,
                        spacing=spacing, timesteps=timesteps, guidance_scale=guidance_scale, **kw)
    return _decode(x, vae, scaling_factor)


def bits_per_dim(noise_model: NoiseModel, diffusion: ForwardProcess, x_0, text_embeds=None, bins=None,
                 clip_denoised=None, **kw):
    """The variational bound on the negative log-density of the latents ``x_0`` in bits per dimension (Ho et al. 2020
    eq. 5; likelihood.bits_per_dim_loop): ``BitsPerDim(total_bpd, prior_bpd, vb, mse, xstart_mse)`` over all T timesteps
    under the condition ``text_embeds``.  The defaults suit latents: a continuous Gaussian decoder at t = 0 and no
    clamp, so the result is a density and can be negative.  ``noises`` / ``philox_seed``, ``prediction``, ``variance``, ``bins``
    and ``data_range`` pass through.  ``variance`` may also be an ``EpsMoments`` (the KL-optimal variance of this model,
    analytic.py) and ``timesteps=[...]`` evaluates the bound of the K-step chain over an ascending sub-list (likelihood.bits_per_dim_loop)."""
    if text_embeds is None:
        raise ValueError("Text embeddings must be provided for conditional generation.")
    return bits_per_dim_loop(noise_model, diffusion, x_0, text_embeds, bins=bins, clip_denoised=clip_denoised, **kw)


def _decode(x, vae, scaling_factor):
    if vae is None:
        return x
    decoded = vae.decode(x / scaling_factor).sample
    return postprocess_images(decoded)
