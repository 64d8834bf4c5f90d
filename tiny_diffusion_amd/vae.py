"""Drop-in for the ``VAE`` / ``VAEConfig`` classes of the reference's ``vae.py`` (37-67,
15-26): the frozen encoder / decoder either side of the latent DDPM (latent_diffusion.py:
205-206, 346).  ``encode``, ``reparameterize``, ``decode`` and ``forward`` run on libtdx, inference
only; ``VAETrainStep`` is the optimisation step of the VAE's training loop (vae.py:70-76, 110-115:
BCE + KLD loss, backward, Adam) and ``VAETrainStep.evaluate`` the loss of its test loop
(vae.py:136-137).  The rest of the training script (MNIST download, loaders, wandb, checkpoint
files) is not reproduced.  Unlike the reference module, importing this one has no side effects."""
from __future__ import annotations

import ctypes as C
import math
import struct
from dataclasses import dataclass
from typing import Any, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
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


def _f32(v: float) -> float:
    """``v`` rounded to fp32, as a C ``float`` argument is: the host arithmetic below then repeats libtdx's."""
    return struct.unpack("f", struct.pack("f", v))[0]


def _number(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{what} must be a finite number, got {v!r}")
    return float(v)


class VAETrainStep:
    """The VAE's optimisation step (vae.py:110-115: ``zero_grad``, forward, ``loss_function``, ``backward``,
    ``optimizer.step``) as one chain of libtdx launches, no autograd graph:

        step = VAETrainStep(vae, lr=1e-3)
        loss = step.step(data)                    # device tensor, not synchronised; step.bce / step.kld: its parts
        loss, bce, kld = step.evaluate(data)      # the test loop: no gradient, no update

    ``tdx_vae_loss_grads`` runs the forward (the last layer without its sigmoid), the BCE on the logits, the KLD and
    the backward of the five Linear layers; the loss is the reference's ``BCE + kld_weight * KLD``, sum-reduced
    (``kld_weight=1``: vae.py:76).  The ten parameters become views of one flat fp32 buffer (``fc1.w fc1.b fc21.w
    fc21.b fc22.w fc22.b fc3.w fc3.b fc4.w fc4.b``), with the gradient and the two Adam moments in three more, so the
    optimizer is one ``tdx_adam_step*`` launch (``max_grad_norm``: ``clip_grad_norm_`` fused, ``tdx_adam_step_clip``).
    ``state_dict()`` / ``load_state_dict()`` of the module keep working (in-place copies land in the flat buffer);
    moving the module afterwards (``.to``, ``.cpu``) detaches it from the buffer and the next call raises.

    Noise: ``eps`` given - used; else with ``philox_seed`` drawn in the reparameterisation kernel, keyed by
    ``(philox_seed, step_count)``; else ``torch.randn``.  ``use_graph=True``: the first step with a batch size runs
    eagerly, the second is captured into a HIP graph, later ones replay it (inputs and noise copied into static
    buffers, Adam's step-dependent scalars in a device tensor); with ``philox_seed`` the step stays eager.

    Not covered: data parallelism, EMA, the bf16 mode (fp32 only)."""

    ORDER = ("fc1", "fc21", "fc22", "fc3", "fc4")

    def __init__(self, vae: "VAE", lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 kld_weight: float = 1.0, max_grad_norm: Optional[float] = None, philox_seed: Optional[int] = None,
                 use_graph: bool = False):
        self.lr = _number(lr, "lr")
        if not isinstance(betas, (tuple, list)) or len(betas) != 2:
            raise ValueError("betas must be a pair of numbers")
        self.betas = (_number(betas[0], "betas[0]"), _number(betas[1], "betas[1]"))
        if not (0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0):
            raise ValueError("betas must lie in [0, 1)")
        self.eps = _number(eps, "eps")
        self.kld_weight = _number(kld_weight, "kld_weight")
        if self.kld_weight < 0:
            raise ValueError("kld_weight must be >= 0")
        if max_grad_norm is not None and not _number(max_grad_norm, "max_grad_norm") > 0:
            raise ValueError("max_grad_norm must be None or > 0")
        if philox_seed is not None and (isinstance(philox_seed, bool) or not isinstance(philox_seed, int)
                                        or not 0 <= philox_seed < 2 ** 64):
            raise ValueError("philox_seed must be None or an integer in [0, 2**64)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.philox_seed = philox_seed
        self.use_graph = bool(use_graph)
        self.vae = vae
        self.step_count = 0
        self._flatten()
        dev = self.device
        self._out = torch.zeros(3, dtype=torch.float32, device=dev)
        self.loss, self.bce, self.kld = self._out[0], self._out[1], self._out[2]
        self._ws = {}             # batch size -> workspace of tdx_vae_loss_grads
        self._clip_scratch = None
        self._graph = self._graph_key = self._hyper = self._gx = self._geps = None
        self._gws = None          # the workspace whose address the captured graph holds: owned by the graph's owner

    # ------------------------------------------------------------------ setup
    def _params(self):
        out = []
        for n in self.ORDER:
            lin = getattr(self.vae, n)
            out += [(n + ".weight", lin.weight), (n + ".bias", lin.bias)]
        return out

    def _flatten(self):
        named = self._params()
        dev = named[0][1].device
        for k, p in named:
            if p.device.type != "cuda" or p.device != dev or p.dtype != torch.float32:
                raise _lib.TdxError("VAETrainStep needs the VAE's fp32 parameters on one CUDA (ROCm) device "
                                    f"(call .to('cuda') first): {k} is {p.dtype} on {p.device}")
        self.device = dev
        total = sum(p.numel() for _, p in named)
        flat = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros_like(flat)
        self.offsets, self.grad_views = {}, {}
        o = 0
        for k, p in named:
            n = p.numel()
            flat[o:o + n].copy_(p.detach().reshape(-1))
            p.data = flat[o:o + n].view(p.shape)      # parameters become views of the flat buffer
            self.grad_views[k] = self.flat_grad[o:o + n].view(p.shape)
            self.offsets[k] = (o, o + n)
            o += n
        self.flat_param = flat
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        base, gbase = flat.data_ptr(), self.flat_grad.data_ptr()
        self._p_ptrs = (C.c_void_p * 10)(*[base + 4 * self.offsets[k][0] for k, _ in named])
        self._g_ptrs = (C.c_void_p * 10)(*[gbase + 4 * self.offsets[k][0] for k, _ in named])

    def _check_attached(self):
        for (k, p), want in zip(self._params(), self._p_ptrs):
            if p.data_ptr() != want:
                raise _lib.TdxError(f"{k} no longer lives in VAETrainStep's flat parameter buffer: the module was moved or "
                                    "its parameters were replaced after the step was built (build a new VAETrainStep)")

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
    def _workspace(self, B):
        ws = self._ws.get(B)
        if ws is None:
            c = self.vae.config
            n = lib.tdx_vae_train_workspace_floats(B, c.input_dim, c.hidden_dim, c.latent_dim)
            if len(self._ws) >= 4:   # small cache; the workspace a captured graph replays into is never evicted
                self._ws = {k: v for k, v in self._ws.items() if v is self._gws}
            ws = self._ws[B] = torch.empty(n, dtype=torch.float32, device=self.device)
        return ws

    def _loss_grads(self, x, eps, B, out, grads: bool):
        c = self.vae.config
        st = torch.cuda.current_stream(self.device).cuda_stream
        if eps is None and self.philox_seed is None:
            eps = torch.randn(B, c.latent_dim, dtype=torch.float32, device=self.device)   # vae.py:57
        check(lib.tdx_vae_loss_grads(x.data_ptr(), self._p_ptrs, self._g_ptrs if grads else None,
                                     None if eps is None else eps.data_ptr(), self.philox_seed or 0, self.step_count,
                                     self.kld_weight, 1.0, out.data_ptr(), self._workspace(B).data_ptr(), B,
                                     c.input_dim, c.hidden_dim, c.latent_dim, st), "tdx_vae_loss_grads")

    def _adam_hyper(self):
        """{lr / bc1, 1 / sqrt(bc2), grad_scale} of the step ``step_count`` counts, with tdx_adam_step's own arithmetic
        (fp32 arguments widened to double), so a captured step and an eager one update bit-identically."""
        b1, b2 = _f32(self.betas[0]), _f32(self.betas[1])
        bc1, bc2 = 1.0 - math.pow(b1, self.step_count), 1.0 - math.pow(b2, self.step_count)
        return [_f32(self.lr) / bc1, 1.0 / math.sqrt(bc2), 1.0]

    def _adam(self, hyper=None):
        st = torch.cuda.current_stream(self.device).cuda_stream
        bufs = (self.flat_param.data_ptr(), self.flat_grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr())
        n = self.flat_param.numel()
        if self.max_grad_norm is not None:
            if self._clip_scratch is None:
                self._clip_scratch = torch.empty(lib.tdx_adam_clip_scratch_bytes(), dtype=torch.uint8, device=self.device)
            check(lib.tdx_adam_step_clip(*bufs, n, self.lr, self.betas[0], self.betas[1], self.eps, self.step_count, 1.0,
                                         self.max_grad_norm, None if hyper is None else hyper.data_ptr(),
                                         self._clip_scratch.data_ptr(), st), "tdx_adam_step_clip")
        elif hyper is not None:
            check(lib.tdx_adam_step_dev(*bufs, n, hyper.data_ptr(), self.betas[0], self.betas[1], self.eps, st),
                  "tdx_adam_step_dev")
        else:
            check(lib.tdx_adam_step(*bufs, n, self.lr, self.betas[0], self.betas[1], self.eps, self.step_count, 1.0, st),
                  "tdx_adam_step")

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
        c = self.vae.config
        if B != self._graph_key:
            if self._graph_key != ("warm", B):
                # the first step with this batch size runs eagerly (workspace, first-launch set-up); the next captures
                self._graph, self._gws, self._graph_key = None, None, ("warm", B)
                return self._eager_step(x, eps, B)
            self._gx = torch.empty(B, c.input_dim, dtype=torch.float32, device=self.device)
            self._geps = torch.empty(B, c.latent_dim, dtype=torch.float32, device=self.device)
            self._hyper = torch.zeros(3, dtype=torch.float32, device=self.device)
            # the graph holds the workspace's raw address and replays never pass through _workspace(): keep it alive
            # (and cached under B) for as long as the graph, whatever other batch sizes evaluate() / step() see
            self._graph = None
            self._gws = self._workspace(B)
            if self.max_grad_norm is not None and self._clip_scratch is None:
                self._clip_scratch = torch.empty(lib.tdx_adam_clip_scratch_bytes(), dtype=torch.uint8, device=self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._eager_step(self._gx, self._geps, B, hyper=self._hyper)
            self.step_count -= 1   # the capture ran the host bookkeeping once without executing anything
            self._graph, self._graph_key = g, B
        self._gx.copy_(x)
        if eps is None:
            self._geps.normal_()     # outside the graph: torch's generator advances as in the eager step
        else:
            self._geps.copy_(eps)
        self.step_count += 1
        self._hyper.copy_(torch.tensor(self._adam_hyper(), dtype=torch.float32))
        self._graph.replay()
        return self.loss

    @torch.no_grad()
    def evaluate(self, x: torch.Tensor, eps: Optional[torch.Tensor] = None):
        """``(loss, bce, kld)`` of ``x`` (vae.py:136-137) from the same forward and loss launches as ``step``, as three
        fresh device scalars; no gradient, moment, parameter or ``step_count`` changes."""
        B, x, eps = self._check_batch(self.vae.config, x, eps)
        self._check_attached()
        out = torch.empty(3, dtype=torch.float32, device=self.device)
        self._loss_grads(x, eps, B, out, grads=False)
        return out[0], out[1], out[2]
