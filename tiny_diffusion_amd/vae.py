"""Drop-in for the ``VAE`` / ``VAEConfig`` classes of the reference's ``vae.py`` (37-67,
15-26): the frozen encoder / decoder either side of the latent DDPM (latent_diffusion.py:
205-206, 346).  ``encode``, ``reparameterize``, ``decode`` and ``forward`` run on libtdx, inference
only; ``VAETrainStep`` is the optimisation step of the VAE's training loop (vae.py:70-76, 110-115:
BCE + KLD loss, backward, Adam) and ``VAETrainStep.evaluate`` the loss of its test loop
(vae.py:136-137).  The rest of the training script (MNIST download, loaders, wandb, checkpoint
files) is not reproduced.  Unlike the reference module, importing this one has no side effects."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._flat_step import FlatStep, _betas_arg, _max_grad_norm_arg, _number, _seed_arg
from ._lib import lib, check

__all__ = ["VAE", "VAEConfig", "VAETrainStep"]


@dataclass
class VAEConfig:
    """vae.py:15-26 (a pydantic model there; plain dataclass here, same fields/defaults)."""
    latent_dim: int = 20
    hidden_dim: int = 400
    input_dim: int = 784
    batch_size: int = 128
    epochs: int = 100
    learning_rate: float = 1e-3
    device: Any = None
    checkpoint_dir: str = "checkpoints"
    n_images_to_log: int = 8

    def __post_init__(self):
        if self.device is None:
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


class VAE(nn.Module):
    """MLP VAE 784 -> 400 -> 20 -> 400 -> 784 (vae.py:37-67); same parameter names, shapes
    and default initialisation order (fc1, fc21, fc22, fc3, fc4)."""

    def __init__(self, config: VAEConfig):
        super().__init__()
        self.config = config
        self.fc1 = nn.Linear(config.input_dim, config.hidden_dim)
        self.fc21 = nn.Linear(config.hidden_dim, config.latent_dim)
        self.fc22 = nn.Linear(config.hidden_dim, config.latent_dim)
        self.fc3 = nn.Linear(config.latent_dim, config.hidden_dim)
        self.fc4 = nn.Linear(config.hidden_dim, config.input_dim)

    def _ptrs(self, names):
        ts = []
        for n in names:
            lin = getattr(self, n)
            ts += [lin.weight, lin.bias]
        for t in ts:
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.TdxError("VAE parameters must be contiguous fp32 CUDA tensors (call .to('cuda'))")
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    @staticmethod
    def _check(x):
        if not x.is_cuda:
            raise _lib.TdxError("tiny_diffusion_amd runs on MI355X only: got a CPU tensor and there is no "
                                "CPU fallback (the CPU restatement lives in oracle/ and is test-only)")
        return x.contiguous().float()

    def _ws(self, B, dev):
        return torch.empty(lib.tdx_vae_workspace_floats(B, self.config.hidden_dim), dtype=torch.float32, device=dev)

    @torch.no_grad()
    def encode(self, x):
        """vae.py:51-53: x (B,784) -> (mu, logvar).  Inference only (the latent DDPM uses the
        VAE frozen, under no_grad: latent_diffusion.py:204-206)."""
        x = self._check(x)
        c = self.config
        if x.dim() != 2 or x.shape[1] != c.input_dim:
            raise ValueError(f"x must be (B,{c.input_dim})")
        B = x.shape[0]
        mu = torch.empty(B, c.latent_dim, dtype=torch.float32, device=x.device)
        logvar = torch.empty_like(mu)
        ws = self._ws(B, x.device)
        st = torch.cuda.current_stream(x.device).cuda_stream
        check(lib.tdx_vae_encode(x.data_ptr(), self._ptrs(("fc1", "fc21", "fc22")), mu.data_ptr(), logvar.data_ptr(),
                                 ws.data_ptr(), B, c.input_dim, c.hidden_dim, c.latent_dim, st), "tdx_vae_encode")
        return mu, logvar

    @torch.no_grad()
    def reparameterize(self, mu, logvar, eps=None):
        """vae.py:55-58; ``eps=None`` draws ``torch.randn_like(std)`` like the reference."""
        mu, logvar = self._check(mu), self._check(logvar)
        eps = torch.randn_like(mu) if eps is None else self._check(eps)
        z = torch.empty_like(mu)
        st = torch.cuda.current_stream(mu.device).cuda_stream
        check(lib.tdx_vae_reparameterize(mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), z.data_ptr(), mu.numel(), st),
              "tdx_vae_reparameterize")
        return z

    @torch.no_grad()
    def decode(self, z):
        """vae.py:60-62: z (B,20) -> sigmoid output (B,784)."""
        z = self._check(z)
        c = self.config
        if z.dim() != 2 or z.shape[1] != c.latent_dim:
            raise ValueError(f"z must be (B,{c.latent_dim})")
        B = z.shape[0]
        out = torch.empty(B, c.input_dim, dtype=torch.float32, device=z.device)
        ws = self._ws(B, z.device)
        st = torch.cuda.current_stream(z.device).cuda_stream
        check(lib.tdx_vae_decode(z.data_ptr(), self._ptrs(("fc3", "fc4")), out.data_ptr(), ws.data_ptr(), B,
                                 c.input_dim, c.hidden_dim, c.latent_dim, st), "tdx_vae_decode")
        return out

    def forward(self, x):
        """vae.py:64-67."""
        mu, logvar = self.encode(x.reshape(-1, self.config.input_dim))
        z = self.reparameterize(mu, logvar)
        return self.decode(z), mu, logvar


class VAETrainStep(FlatStep):
    """The VAE's optimisation step (vae.py:110-115: ``zero_grad``, forward, ``loss_function``, ``backward``,
    ``optimizer.step``) as one chain of libtdx launches, no autograd graph:

        step = VAETrainStep(vae, lr=1e-3)
        loss = step.step(data)                    # device tensor, not synchronised; step.bce / step.kld: its parts
        loss, bce, kld = step.evaluate(data)      # the test loop: no gradient, no update

    ``tdx_vae_loss_grads`` runs the forward (the last layer without its sigmoid), the BCE on the logits, the KLD and
    the backward of the five Linear layers; the loss is the reference's ``BCE + kld_weight * KLD``, sum-reduced
    (``kld_weight=1``: vae.py:76).  The ten parameters (``fc1.w fc1.b fc21.w fc21.b fc22.w fc22.b fc3.w fc3.b fc4.w
    fc4.b``) live in ``_flat_step.FlatStep``'s flat buffers, which also owns the one optimizer launch (``max_grad_norm``:
    ``clip_grad_norm_`` fused into it) and the capture protocol.  ``state_dict()`` / ``load_state_dict()`` of the module
    keep working (in-place copies land in the flat buffer); moving the module afterwards (``.to``, ``.cpu``) detaches it
    from the buffer and the next call raises.

    Noise: ``eps`` given - used; else with ``philox_seed`` drawn in the reparameterisation kernel, keyed by
    ``(philox_seed, step_count)``; else ``torch.randn``.  ``use_graph=True``: inputs and noise are copied into static
    buffers before each replay; with ``philox_seed`` the step stays eager.

    Not covered: data parallelism, EMA, the bf16 mode (fp32 only)."""

    ORDER = ("fc1", "fc21", "fc22", "fc3", "fc4")

    def __init__(self, vae: "VAE", lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 kld_weight: float = 1.0, max_grad_norm: Optional[float] = None, philox_seed: Optional[int] = None,
                 use_graph: bool = False):
        lr, betas, eps = _number(lr, "lr"), _betas_arg(betas), _number(eps, "eps")
        self.kld_weight = _number(kld_weight, "kld_weight")
        if self.kld_weight < 0:
            raise ValueError("kld_weight must be >= 0")
        self._init_optimizer(lr, betas, eps, _max_grad_norm_arg(max_grad_norm), use_graph=bool(use_graph))
        self.philox_seed = _seed_arg(philox_seed, "philox_seed")
        self.vae = vae
        named = self._params()
        self._require_fp32_cuda(named, "the VAE's")
        self._flatten(named)
        self._out = torch.zeros(3, dtype=torch.float32, device=self.device)
        self.loss, self.bce, self.kld = self._out[0], self._out[1], self._out[2]
        self._gx = self._geps = None

    # ------------------------------------------------------------------ setup
    def _params(self):
        out = []
        for n in self.ORDER:
            lin = getattr(self.vae, n)
            out += [(n + ".weight", lin.weight), (n + ".bias", lin.bias)]
        return out

    # ------------------------------------------------------------- validation
    @staticmethod
    def _check_batch(config, x, eps):
        """Shapes first (``ValueError``), then the device (``TdxError``); returns (B, x2d, eps) ready for the call."""
        if not isinstance(x, torch.Tensor) or x.dim() < 2 or x.shape[0] < 1 or x[0].numel() != config.input_dim:
            raise ValueError(f"x must be (B,{config.input_dim}) or (B,1,28,28)-like with {config.input_dim} values per "
                             f"sample, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
        B = x.shape[0]
        if eps is not None and (not isinstance(eps, torch.Tensor) or tuple(eps.shape) != (B, config.latent_dim)):
            raise ValueError(f"eps must be ({B},{config.latent_dim}), got "
                             f"{tuple(eps.shape) if isinstance(eps, torch.Tensor) else type(eps)}")
        x = VAE._check(x).reshape(B, config.input_dim)
        if eps is not None:
            eps = VAE._check(eps)
        return B, x, eps

    # ------------------------------------------------------------------- step
    def _workspace_floats(self, B):
        c = self.vae.config
        return lib.tdx_vae_train_workspace_floats(B, c.input_dim, c.hidden_dim, c.latent_dim)

    def _loss_grads(self, x, eps, B, out, grads: bool):
        c = self.vae.config
        st = torch.cuda.current_stream(self.device).cuda_stream
        if eps is None and self.philox_seed is None:
            eps = torch.randn(B, c.latent_dim, dtype=torch.float32, device=self.device)   # vae.py:57
        check(lib.tdx_vae_loss_grads(x.data_ptr(), self._p_ptrs, self._g_ptrs if grads else None,
                                     None if eps is None else eps.data_ptr(), self.philox_seed or 0, self.step_count,
                                     self.kld_weight, 1.0, out.data_ptr(), self._workspace(B).data_ptr(), B,
                                     c.input_dim, c.hidden_dim, c.latent_dim, st), "tdx_vae_loss_grads")

    def _eager_step(self, x, eps, B, hyper=None):
        self._loss_grads(x, eps, B, self._out, grads=True)      # vae.py:111-113
        self.step_count += 1
        self._adam(hyper)                                        # vae.py:115
        return self.loss

    def step(self, x: torch.Tensor, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One optimisation step on ``x``: (B,1,28,28) or (B,input_dim) in [-1, 1]; returns the (device, not
        synchronised) loss ``BCE + kld_weight * KLD``, summed over the batch like the reference's ``loss_function``;
        ``self.bce`` / ``self.kld`` hold the two parts.  The three live in one buffer that the next step overwrites."""
        B, x, eps = self._check_batch(self.vae.config, x, eps)
        self._check_attached()
        if self.use_graph and self.philox_seed is None:
            return self._graph_step(x, eps, B)
        return self._eager_step(x, eps, B)

    def _graph_step(self, x, eps, B):
        if not self._graph_ready((B,), B):   # the first step with this batch size: workspace, first-launch set-up
            return self._eager_step(x, eps, B)
        self._gx.copy_(x)
        if eps is None:
            self._geps.normal_()     # outside the graph: torch's generator advances as in the eager step
        else:
            self._geps.copy_(eps)
        return self._replay()

    def _alloc_static(self, B):
        c = self.vae.config
        self._gx = torch.empty(B, c.input_dim, dtype=torch.float32, device=self.device)
        self._geps = torch.empty(B, c.latent_dim, dtype=torch.float32, device=self.device)
        # the graph holds the workspace's raw address and replays never pass through _workspace(): keep it alive
        # (and cached under B) for as long as the graph, whatever other batch sizes evaluate() / step() see
        self._gws = self._workspace(B)

    def _static_step(self, hyper):
        self._eager_step(self._gx, self._geps, self._gx.shape[0], hyper=hyper)

    @torch.no_grad()
    def evaluate(self, x: torch.Tensor, eps: Optional[torch.Tensor] = None):
        """``(loss, bce, kld)`` of ``x`` (vae.py:136-137) from the same forward and loss launches as ``step``, as three
        fresh device scalars; no gradient, moment, parameter or ``step_count`` changes."""
        B, x, eps = self._check_batch(self.vae.config, x, eps)
        self._check_attached()
        out = torch.empty(3, dtype=torch.float32, device=self.device)
        self._loss_grads(x, eps, B, out, grads=False)
        return out[0], out[1], out[2]
