"""Drop-in for the hot path of the reference's ``diffusion_transformer.py``: ``TransformerBlock``,
``NoiseModel(time_dim, num_classes, latent_dim, num_heads, num_layers, dropout)`` with
``forward(x, t, y)``, ``ForwardProcess`` and ``sample(vae, ...)`` (diffusion_transformer.py:16-132,
284-323).

The reference feeds its blocks a LENGTH-1 sequence (``x.unsqueeze(0)``, line 99, with
``nn.MultiheadAttention`` in its default sequence-first layout), so the softmax runs over a single
key and ``attention(x, x, x) == out_proj(v_proj(x))``; in train mode the attention-weight dropout
zeroes or rescales that single weight per (row, head).  That is what runs here (Q and K projections
receive exactly-zero gradients, as in the reference).  The modules below own the parameters under
the reference's names (``nn.MultiheadAttention.in_proj_weight`` etc.) and give the reference's
default initialisation; their torch ``forward`` is never called."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import check, lib
from ._flat_step import (FlatStep, _betas_arg, _ema_args, _i64, _max_grad_norm_arg, _number, _seed_arg,
                         cosine_annealing_lr, ema_decay_at)
from .likelihood import bits_per_dim_loop
from .schedule import ForwardProcess, ddim_sample_loop, dpm_sample_loop, sample_loop
from .vae import VAE, VAEConfig

__all__ = ["TransformerBlock", "NoiseModel", "ForwardProcess", "sample", "ddim_sample", "dpm_sample", "bits_per_dim", "VAE", "VAEConfig",
           "TransformerTrainStep", "cosine_annealing_lr", "ema_decay_at"]


class TransformerBlock(nn.Module):
    """diffusion_transformer.py:16-35 (post-norm block: x = LN(x + drop(attn)); x = LN(x + drop(ff)))."""

    def __init__(self, dim, num_heads, ff_dim, dropout=0.1):
        super().__init__()
        self.attention = nn.MultiheadAttention(dim, num_heads, dropout=dropout)
        self.norm1 = nn.LayerNorm(dim)
        self.ff = nn.Sequential(nn.Linear(dim, ff_dim), nn.GELU(), nn.Linear(ff_dim, dim), nn.Dropout(dropout))
        self.norm2 = nn.LayerNorm(dim)
        self.dropout = nn.Dropout(dropout)
        self.dim, self.num_heads, self.p = dim, num_heads, float(dropout)

    def forward(self, x, rng=None):
        """x: (B, dim) - the reference's (1, B, dim) with the length-1 sequence axis dropped."""
        D = self.dim
        drop = self.training and self.p > 0.0
        att = self.attention
        v = ops.linear(x, att.in_proj_weight[2 * D:], att.in_proj_bias[2 * D:])
        if drop:  # dropout of the (single) attention weight of every head
            v = ops.dropout(v, self.p, D // self.num_heads, *rng())
        a = ops.linear(v, att.out_proj.weight, att.out_proj.bias)
        if drop:
            a = ops.dropout(a, self.p, 1, *rng())
        x = ops.layer_norm(ops.add(x, a), self.norm1.weight, self.norm1.bias, self.norm1.eps)
        f = ops.gelu(ops.linear(x, self.ff[0].weight, self.ff[0].bias))
        f = ops.linear(f, self.ff[2].weight, self.ff[2].bias)
        if drop:  # ff's own nn.Dropout, then self.dropout (lines 25, 33)
            f = ops.dropout(f, self.p, 1, *rng())
            f = ops.dropout(f, self.p, 1, *rng())
        return ops.layer_norm(ops.add(x, f), self.norm2.weight, self.norm2.bias, self.norm2.eps)


class _Shape:
    in_shape = (20,)


class NoiseModel(nn.Module):
    """diffusion_transformer.py:38-107."""

    def __init__(self, time_dim=256, num_classes=10, latent_dim=20, num_heads=4, num_layers=4, dropout=0.05):
        super().__init__()
        if time_dim % 64 or time_dim > 1024:
            raise ValueError("libtdx LayerNorm needs time_dim % 64 == 0 and <= 1024")
        self.time_dim = time_dim
        self.latent_dim = latent_dim
        self.time_embedding = nn.Sequential(nn.Linear(1, time_dim), nn.SiLU(), nn.Linear(time_dim, time_dim))
        self.class_embedding = nn.Embedding(num_classes, time_dim)
        self.input_proj = nn.Linear(latent_dim, time_dim)
        self.pos_encoding = nn.Parameter(torch.randn(1, 1, time_dim))
        self.transformer_blocks = nn.ModuleList(
            [TransformerBlock(time_dim, num_heads, time_dim * 4, dropout) for _ in range(num_layers)])
        self.final_layer = nn.Sequential(nn.LayerNorm(time_dim), nn.Linear(time_dim, latent_dim))
        self._arch = _Shape()
        self._arch.in_shape = (latent_dim,)
        # dropout masks: Philox stream (seed drawn from torch's generator once per forward, so
        # torch.manual_seed reproduces a run), one offset per dropout site
        self._calls = 0

    def _rng_factory(self):
        seed = int(torch.randint(0, 2**62, (1,)).item()) if self.training else 0
        state = {"off": 0}

        def rng():
            state["off"] += 1
            return seed, state["off"]

        return rng

    def forward(self, x, t, y):
        if not x.is_cuda:
            raise _lib.TdxError("tiny_diffusion_amd runs on MI355X only: got a CPU tensor and there is no "
                                "CPU fallback (the CPU restatement lives in oracle/ and is test-only)")
        if x.dim() != 2 or x.shape[1] != self.latent_dim:
            raise ValueError(f"x must be (B,{self.latent_dim})")
        if t.shape != (x.shape[0],) or y.shape != (x.shape[0],):
            raise ValueError("t and y must have shape (B,)")
        rng = self._rng_factory()
        te = self.time_embedding
        tn = (t / 1000).unsqueeze(-1).float()                       # line 86
        h = ops.silu(ops.linear(tn, te[0].weight, te[0].bias))
        emb = ops.add(ops.linear(h, te[2].weight, te[2].bias), ops.embedding(self.class_embedding.weight, y))
        h = ops.add(ops.linear(x, self.input_proj.weight, self.input_proj.bias), emb)   # lines 92-95
        h = ops.add(h, self.pos_encoding.view(-1))                   # line 98 (broadcast over the batch)
        for blk in self.transformer_blocks:
            h = blk(h, rng)
        fl = self.final_layer
        return ops.linear(ops.layer_norm(h, fl[0].weight, fl[0].bias, fl[0].eps), fl[1].weight, fl[1].bias)

    # sample_loop's entry point (inference forward, no autograd graph)
    @torch.no_grad()
    def _run_forward(self, x, t, y, mode=2):
        return self.forward(x, t, y), None, mode


@torch.no_grad()
def sample(vae: VAE, noise_model: NoiseModel, diffusion: ForwardProcess, device, n_samples=16, y=None, **kw):
    """diffusion_transformer.py:284-323 (identical to latent_diffusion.sample, ``clip_denoised`` included).  ``known=x, mask=m`` (through ``**kw``; both or neither, broadcast to
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


class _TShape(C.Structure):
    """``tdx_transformer_shape`` (include/tdx.h)."""
    _fields_ = [("batch", C.c_int), ("latent_dim", C.c_int), ("dim", C.c_int), ("num_heads", C.c_int),
                ("num_layers", C.c_int), ("num_classes", C.c_int), ("dropout_p", C.c_float), ("ln_eps", C.c_float)]


class TransformerTrainStep(FlatStep):
    """The optimisation step of the transformer's training loop (diffusion_transformer.py:193-202: ``randint``,
    ``q_sample``, forward, ``F.mse_loss``, ``zero_grad``, ``backward``, ``optimizer.step``) as one short chain of libtdx
    launches with no autograd graph:

        step = TransformerTrainStep(model, diffusion, lr=3e-4)
        for epoch in range(num_epochs):
            step.lr = cosine_annealing_lr(epoch, 3e-4, num_epochs)     # CosineAnnealingLR(T_max=num_epochs), per epoch
            for z_0, labels in loader:
                loss = step.step(z_0, labels)                          # device tensor, not synchronised
            model.eval(); val = step.evaluate(z_0, labels); model.train()

    ``tdx_transformer_loss_grads`` runs forward, loss and backward (csrc/transformer.hip) on the parameters in
    ``state_dict()`` order; the flat buffers, the one optimizer launch (``max_grad_norm``: ``clip_grad_norm_`` fused into
    it), the objective (``prediction`` / ``loss_weighting`` / ``snr_gamma`` / ``set_objective``), the average
    (``ema_decay`` / ``ema_warmup`` / ``ema_weights()`` ...) and the capture protocol are ``_flat_step.FlatStep``'s and
    behave as in ``train.TrainStep``.  ``state_dict()`` / ``load_state_dict()`` of the module keep working (in-place
    copies land in the flat buffer); moving the module afterwards (``.to``, ``.cpu``) detaches it and the next call
    raises.  ``lr`` is a plain attribute read at every step (a captured step reads it through its device scalars).

    Noise: ``noise`` given - used; else with ``philox_seed`` drawn in the q_sample kernel, keyed by ``(philox_seed,
    step_count)``; else ``torch.randn_like``.  ``t=None`` draws ``torch.randint`` on the device as the reference does.

    Dropout follows ``model.training``, with the blocks' ``p``; the masks are Philox draws, regenerated in the backward.
    ``dropout_seed=None``: one key per step from torch's CPU generator, drawn exactly as the module's own forward
    draws it, with offset 0 - ``torch.manual_seed`` reproduces a step, and with ``t`` and ``noise`` passed the step uses
    the very masks of ``model(z_t, t, y)`` under the same seed.  ``dropout_seed=int``: that key with offset
    ``step_count * 4 * num_layers``.  ``last_dropout_seed`` / ``last_dropout_offset`` hold what the last step used.

    ``timestep_sampler`` / ``importance_weights`` / ``timestep_seed`` / ``history_per_term`` / ``uniform_prob``: as in
    ``train.TrainStep`` - a ``(T,)`` probability table or ``"loss_second_moment"`` replaces ``torch.randint`` by a
    Philox draw on the device keyed by ``(timestep_seed, step_count, sample)``; ``sample_losses``, ``last_t`` and
    ``timestep_sampler_state()`` come with it.  A captured step draws into its static ``t`` right before the replay and
    runs the sampler's other launches inside the graph, so it sees the timesteps and leaves the state of an eager one.

    ``use_graph=True``: the first step with a batch size runs eagerly, the second is captured into a HIP graph, later
    ones replay it; inputs, Adam's step-dependent scalars and the dropout ``{seed, offset}`` live in static device
    buffers refreshed before each replay.  With ``philox_seed`` the step stays eager.

    This model has no null class, so there is no ``cond_drop_prob`` (classifier-free guidance needs a model with one).
    Not covered: data parallelism, the bf16 mode (fp32 only)."""

    def __init__(self, model: "NoiseModel", diffusion: ForwardProcess, lr: float = 3e-4,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, max_grad_norm: Optional[float] = None,
                 prediction: str = "eps", loss_weighting=None, snr_gamma: float = 5.0,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False, philox_seed: Optional[int] = None,
                 dropout_seed: Optional[int] = None, use_graph: bool = False, timestep_sampler=None,
                 importance_weights=None, timestep_seed: int = 0, history_per_term: int = 10,
                 uniform_prob: float = 0.001):
        if not isinstance(model, NoiseModel):
            raise ValueError("TransformerTrainStep needs a diffusion_transformer.NoiseModel")
        if not isinstance(diffusion, ForwardProcess):
            raise ValueError("diffusion must be a ForwardProcess")
        lr, betas, eps = _number(lr, "lr"), _betas_arg(betas), _number(eps, "eps")
        max_grad_norm = _max_grad_norm_arg(max_grad_norm)
        self.model, self.diffusion = model, diffusion
        self._check_objective(prediction, loss_weighting, snr_gamma)
        self._check_timestep_sampler(timestep_sampler, importance_weights, timestep_seed, history_per_term, uniform_prob)
        self._init_optimizer(lr, betas, eps, max_grad_norm, *_ema_args(ema_decay, ema_warmup), use_graph=bool(use_graph))
        self.philox_seed = _seed_arg(philox_seed, "philox_seed")
        self.dropout_seed = _seed_arg(dropout_seed, "dropout_seed")
        blocks = list(model.transformer_blocks)
        if not blocks:
            raise ValueError("the model has no transformer block")
        ps = {b.p for b in blocks}
        epss = {float(b.norm1.eps) for b in blocks} | {float(b.norm2.eps) for b in blocks} | {float(model.final_layer[0].eps)}
        heads = {b.num_heads for b in blocks}
        if len(ps) != 1 or len(epss) != 1 or len(heads) != 1:
            raise ValueError("the fused step needs one dropout p, one LayerNorm eps and one head count for every block")
        self.p = float(ps.pop())
        if not 0.0 <= self.p < 1.0:
            raise ValueError("dropout must lie in [0, 1)")
        self.num_layers, self.num_heads = len(blocks), int(heads.pop())
        self.num_classes = int(model.class_embedding.num_embeddings)
        self._ln_eps = epss.pop()
        self.last_dropout_seed = self.last_dropout_offset = None
        # ---- device work from here on
        named = self._params()
        if len(named) != 12 + 12 * self.num_layers:
            raise ValueError("unexpected parameter list: the fused step knows NoiseModel's 12 + 12 L tensors")
        self._require_fp32_cuda(named, "the model's")
        self._flatten(named)
        self._upload_weights()
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._gz = self._gy = self._gt = self._gnoise = self._grng = None
        self._init_timestep_sampler()

    # ------------------------------------------------------------------ setup
    def _params(self):
        named = dict(self.model.named_parameters())
        return [(k, named[k]) for k in self.model.state_dict().keys()]

    # ------------------------------------------------------------- validation
    def _check_batch(self, z_0, y, t, noise):
        """Shapes first (``ValueError``), then the device (``TdxError``); returns tensors ready for the kernels."""
        Ld = self.model.latent_dim
        if not isinstance(z_0, torch.Tensor) or z_0.dim() != 2 or z_0.shape[0] < 1 or z_0.shape[1] != Ld:
            raise ValueError(f"z_0 must be (B,{Ld})")
        B = z_0.shape[0]
        if not isinstance(y, torch.Tensor) or tuple(y.shape) != (B,) or y.dtype.is_floating_point:
            raise ValueError("y must be an integer tensor of shape (B,)")
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (B,) or t.dtype.is_floating_point):
            raise ValueError("t must be an integer tensor of shape (B,)")
        if noise is not None and (not isinstance(noise, torch.Tensor) or tuple(noise.shape) != (B, Ld)):
            raise ValueError(f"noise must be ({B},{Ld})")
        for name, v in (("z_0", z_0), ("y", y), ("t", t), ("noise", noise)):
            if v is not None and (not v.is_cuda or v.device != self.device):
                raise _lib.TdxError(f"tiny_diffusion_amd runs on MI355X only: {name} is on {v.device}, the step on "
                                    f"{self.device} (there is no CPU fallback)")
        z_0 = z_0.contiguous().float()
        y = y.contiguous().to(torch.int64)
        t = None if t is None else t.contiguous().to(torch.int64)
        noise = None if noise is None else noise.contiguous().float()
        return B, z_0, y, t, noise

    # ------------------------------------------------------------------- step
    def _shape(self, B):
        m = self.model
        return _TShape(B, m.latent_dim, m.time_dim, self.num_heads, self.num_layers, self.num_classes, self.p, self._ln_eps)

    def _workspace_floats(self, B):
        n = lib.tdx_transformer_train_workspace_floats(C.byref(self._shape(B)))
        if n == 0:
            raise _lib.TdxError("tdx_transformer_train_workspace_floats: shape not covered (dim % 64, dim <= 1024, "
                                "dim % num_heads)")
        return n

    def _next_rng(self):
        """(seed, offset) of the dropout masks of the step about to run (see the class docstring)."""
        if self.dropout_seed is not None:
            return self.dropout_seed, self.step_count * 4 * self.num_layers
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if self.model.training else 0   # NoiseModel._rng_factory
        return seed, 0

    def _loss_grads(self, z_t, t, y, target, B, loss, grads: bool, train: bool, rng, rng_dev=None, eps_hat=None):
        """``grads``: the training step - its loss weights are the sampler's where there is one (``_loss_table``);
        ``evaluate()`` reads the objective's own."""
        st = torch.cuda.current_stream(self.device).cuda_stream
        w_table = self._loss_table() if grads else self._w_table
        check(lib.tdx_transformer_loss_grads(C.byref(self._shape(B)), self._p_ptrs, self._g_ptrs if grads else None,
                                             z_t.data_ptr(), t.data_ptr(), y.data_ptr(), target.data_ptr(),
                                             None if w_table is None else w_table.data_ptr(),
                                             1 if train else 0, rng[0], rng[1],
                                             None if rng_dev is None else rng_dev.data_ptr(), 1.0, loss.data_ptr(),
                                             None if eps_hat is None else eps_hat.data_ptr(),
                                             self._workspace(B).data_ptr(), st), "tdx_transformer_loss_grads")

    def _eager_step(self, z_0, y, t, noise, B, rng, hyper=None, rng_dev=None):
        sampler = self.timestep_sampler is not None
        if t is None and sampler:
            t = self._draw_t(B, self.step_count)
        elif t is None:
            t = torch.randint(0, self.diffusion.num_timesteps, (B,), device=self.device)   # line 193
        z_t, target = self._q_sample(z_0, t, noise, self.step_count)                         # line 196
        eps_hat = torch.empty_like(target) if sampler else None
        self._loss_grads(z_t, t, y, target, B, self.loss, True, self.model.training, rng, rng_dev, eps_hat)   # lines 197-201
        if sampler:
            self._after_loss(eps_hat, target, t, B)
        self.last_dropout_seed, self.last_dropout_offset = rng
        self.step_count += 1
        self._adam(hyper)                                                                    # line 202
        return self.loss

    def step(self, z_0: torch.Tensor, y: torch.Tensor, t: Optional[torch.Tensor] = None,
             noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One optimisation step on latents ``z_0`` (B, latent_dim) with labels ``y`` (B,); returns the (device, not
        synchronised) loss - the weighted loss under ``loss_weighting`` - in a buffer that the next step overwrites."""
        B, z_0, y, t, noise = self._check_batch(z_0, y, t, noise)
        if self._ema_swapped:
            raise RuntimeError("step() inside ema_weights(): the model holds the averaged weights")
        self._check_attached()
        if self.use_graph and self.philox_seed is None:
            return self._graph_step(z_0, y, t, noise, B)
        return self._eager_step(z_0, y, t, noise, B, self._next_rng())

    def _graph_step(self, z_0, y, t, noise, B):
        if not self._graph_ready((B, self.model.training), B):   # the first step with this batch size: workspace, set-up
            return self._eager_step(z_0, y, t, noise, B, self._next_rng())
        rng = self._next_rng()
        self._gz.copy_(z_0)
        self._gy.copy_(y)
        sampler = self.timestep_sampler is not None
        if t is None and sampler:
            self._draw_t(B, self.step_count, out=self._gt)      # from the table the replay before this one left
        elif t is None:
            self._gt.random_(0, self.diffusion.num_timesteps)   # outside the graph: torch's generator advances as in
        else:                                                    # the eager step (randint, then randn_like)
            self._gt.copy_(t)
        if noise is None:
            self._gnoise.normal_()
        else:
            self._gnoise.copy_(noise)
        self._grng.copy_(torch.tensor([_i64(rng[0]), _i64(rng[1])], dtype=torch.int64))
        self.last_dropout_seed, self.last_dropout_offset = rng
        if sampler:   # what the replay writes
            self.last_t, self.sample_losses = self._gt, self._sample_losses_buf(B)
        return self._replay()

    def _alloc_static(self, B):
        dev, Ld = self.device, self.model.latent_dim
        self._gz = torch.empty(B, Ld, dtype=torch.float32, device=dev)
        self._gnoise = torch.empty(B, Ld, dtype=torch.float32, device=dev)
        self._gy = torch.empty(B, dtype=torch.int64, device=dev)
        self._gt = torch.zeros(B, dtype=torch.int64, device=dev)
        self._grng = torch.zeros(2, dtype=torch.int64, device=dev)
        # the graph holds the workspace's raw address and replays never pass through _workspace(): keep it alive
        # (and cached under B) for as long as the graph, whatever other batch sizes evaluate() / step() see
        self._gws = self._workspace(B)
        self.diffusion.tables(dev)

    def _static_step(self, hyper):
        keep = (self.last_dropout_seed, self.last_dropout_offset)
        self._eager_step(self._gz, self._gy, self._gt, self._gnoise, self._gz.shape[0], (0, 0), hyper=hyper,
                         rng_dev=self._grng)
        self.last_dropout_seed, self.last_dropout_offset = keep

    @torch.no_grad()
    def evaluate(self, z_0: torch.Tensor, y: torch.Tensor, t: Optional[torch.Tensor] = None,
                 noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The validation loop's loss (diffusion_transformer.py:219-228) as a fresh device scalar: the same forward and
        loss launches with dropout off whatever ``model.training`` says; no gradient, moment, parameter, average or
        ``step_count`` changes."""
        B, z_0, y, t, noise = self._check_batch(z_0, y, t, noise)
        self._check_attached()
        if t is None:
            t = torch.randint(0, self.diffusion.num_timesteps, (B,), device=self.device)
        z_t, target = self._q_sample(z_0, t, noise, self.step_count)
        out = torch.empty(1, dtype=torch.float32, device=self.device)
        self._loss_grads(z_t, t, y, target, B, out, False, False, (0, 0))
        return out[0]
