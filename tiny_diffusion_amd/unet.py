"""Host side of the MI355X noise predictor: an ``nn.Module`` with the reference's
constructor, ``state_dict`` and ``forward(x, t[, y])`` (diffusion.py:11-162,
conditional_diffusion.py:14-172, conditional_diffusion_laion.py:234-332) whose compute
is libtdx.so (include/tdx.h).

The module tree below exists only to own parameters/buffers under the
reference's names and to give the reference's default initialisation (same
constructors in the same order => bit-identical weights under the same
``torch.manual_seed``); none of the torch layers' ``forward`` is ever called.
There is no CPU/eager fallback: a non-CUDA input raises.

The null condition (classifier-free guidance): a label ``y[n] < 0`` (``NULL_LABEL = -1``) of the class-conditional
UNet means "no class" - ``emb[n] = t_emb[n]``, in every mode, with no read of ``class_embedding`` and no gradient
to it; for the LAION UNet it is an all-zero ``text_embeds`` row (``emb = t_emb + 0``).  No parameter is added: the
``state_dict`` stays the reference's.  Labels are not checked on the host (that would force a sync); labels
``>= num_classes`` are undefined.
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib
from ._lib import lib, check

TIME_DIM = 256
MODE_TRAIN, MODE_EVAL_GRAD, MODE_INFER = 0, 1, 2
_BN_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)   # tdx_allreduce_fn
KIND_MNIST, KIND_LAION, KIND_LATENT = 0, 1, 2


class _Arch:
    """Shape of one reference NoiseModel (mirrors SPECS[] in csrc/unet.hip)."""

    def __init__(self, kind, in_shape, time_dim, time_name, x0, enc, bottleneck, dec, ceil_pool,
                 init_name="initial_conv", final_name="final_conv"):
        self.kind = kind
        self.init_name, self.final_name = init_name, final_name
        self.in_shape = in_shape          # (C, H, W) of x and of the prediction
        self.time_dim = time_dim
        self.time_name = time_name        # module name of the time MLP
        self.x0 = x0                      # initial_conv output channels
        self.enc, self.bottleneck, self.dec = enc, bottleneck, dec  # (name, cin, cout) stages
        self.ceil_pool = ceil_pool


# diffusion.py:16-107 / conditional_diffusion.py:19-113
ARCH_MNIST = _Arch(KIND_MNIST, (1, 28, 28), 256, "time_embedding", 64,
                   (("enc1", 64, 128), ("enc2", 128, 256), ("enc3", 256, 512)), 512,
                   (("dec3", 1024, 256), ("dec2", 512, 128), ("dec1", 256, 64)), True)
# conditional_diffusion_laion.py:235-301
ARCH_LAION = _Arch(KIND_LAION, (4, 32, 32), 768, "time_mlp", 32,
                   (("enc1", 32, 64), ("enc2", 64, 128), ("enc3", 128, 256)), 256,
                   (("dec3", 512, 256), ("dec2", 384, 128), ("dec1", 192, 64)), False)
# conv/BN units in the order of TDX_P_UNIT0.. (include/tdx.h)
_UNIT_PREFIX = (
    ("enc1", 0), ("enc1", 3), ("enc2", 0), ("enc2", 3), ("enc3", 0), ("enc3", 3), ("bottleneck", 0),
    ("dec3", 0), ("dec3", 3), ("dec2", 0), ("dec2", 3), ("dec1", 0), ("dec1", 3),
)


# latent_diffusion.py:16-105: stages are (name, in, mid, out) of two Linear+BatchNorm1d+ReLU units
ARCH_LATENT = _Arch(KIND_LATENT, (20,), 256, "time_embedding", 512,
                    (("enc1", 512, 512, 256), ("enc2", 256, 256, 128), ("enc3", 128, 128, 64)), 64,
                    (("dec3", 128, 128, 128), ("dec2", 256, 256, 256), ("dec1", 512, 512, 512)), False,
                    init_name="initial_fc", final_name="final_fc")


def _lin_bn_relu(cin, cout):
    return [nn.Linear(cin, cout), nn.BatchNorm1d(cout), nn.ReLU()]


def _conv_bn_relu(cin, cout):
    return [nn.Conv2d(cin, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.ReLU()]


def param_slot_names(cond: bool, time_name: str = "time_embedding", init_name: str = "initial_conv",
                     final_name: str = "final_conv") -> List[Optional[str]]:
    """state_dict key of every TDX_P_* slot (None where the slot is unused)."""
    names: List[Optional[str]] = [
        f"{time_name}.0.weight", f"{time_name}.0.bias",
        f"{time_name}.2.weight", f"{time_name}.2.bias",
        "class_embedding.weight" if cond else None,
        f"{init_name}.weight", f"{init_name}.bias",
    ]
    for stage, idx in _UNIT_PREFIX:
        names += [f"{stage}.{idx}.weight", f"{stage}.{idx}.bias",
                  f"{stage}.{idx + 1}.weight", f"{stage}.{idx + 1}.bias"]
    names += [f"{final_name}.weight", f"{final_name}.bias"]
    for k in (1, 2, 3):
        names += [f"time_proj{k}.weight", f"time_proj{k}.bias"]
    return names


def buffer_slot_names() -> List[str]:
    out = []
    for stage, idx in _UNIT_PREFIX:
        out += [f"{stage}.{idx + 1}.running_mean", f"{stage}.{idx + 1}.running_var",
                f"{stage}.{idx + 1}.num_batches_tracked"]
    return out


def backward_stage_params(cond: bool, time_name: str = "time_embedding", init_name: str = "initial_conv",
                          final_name: str = "final_conv") -> List[List[str]]:
    """Parameters whose gradient is final after each backward stage
    (tdx_unet_backward stage order): used to bucket the gradient all-reduce."""
    stages = [[f"{final_name}.weight", f"{final_name}.bias"]]
    for stage, idx in reversed(_UNIT_PREFIX):
        stages.append([f"{stage}.{idx}.weight", f"{stage}.{idx}.bias",
                       f"{stage}.{idx + 1}.weight", f"{stage}.{idx + 1}.bias"])
    last = [f"{init_name}.weight", f"{init_name}.bias",
            f"{time_name}.0.weight", f"{time_name}.0.bias",
            f"{time_name}.2.weight", f"{time_name}.2.bias"]
    if cond:
        last.append("class_embedding.weight")
    for k in (1, 2, 3):
        last += [f"time_proj{k}.weight", f"time_proj{k}.bias"]
    stages.append(last)
    return stages


class _Plan:
    """One tdx_unet handle + workspace per (device, batch size)."""

    def __init__(self, batch: int, num_classes: int, device: torch.device, kind: int = KIND_MNIST, hw: int = 0,
                 time_dim: int = 0):
        _destroy_parked()
        self.batch = batch
        self.device = device
        self.hw = hw
        h = C.c_void_p()
        with torch.cuda.device(device):
            check(lib.tdx_unet_create_full(C.byref(h), batch, kind, num_classes, hw, time_dim), "tdx_unet_create_full")
        self.handle = h
        self.ws_bytes = lib.tdx_unet_workspace_bytes(h, batch, MODE_TRAIN)
        if self.ws_bytes == 0:
            raise _lib.TdxError("tdx_unet_workspace_bytes returned 0")
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.generation = 0      # bumped by every forward that saves state
        self.infer_key = None    # parameter versions the INFER pack was built from
        self.precision = 0       # TDX_PREC_* the handle is set to
        self.bn_sync = None      # SyncBN callback object installed on the handle
        self.stream_mode = -1    # tdx_unet_set_streams mode the handle is set to (-1: the network's default)

    def tensor(self, name: str) -> torch.Tensor:
        """View of a named intermediate inside the workspace (tests / debugging)."""
        off, cnt = C.c_size_t(), C.c_size_t()
        check(lib.tdx_unet_tensor(self.handle, self.batch, name.encode(), C.byref(off), C.byref(cnt)),
              f"tdx_unet_tensor({name})")
        return self.workspace.view(torch.float32)[off.value:off.value + cnt.value]

    def __del__(self):
        # tdx_unet_destroy synchronises the plan's streams and hipFrees its packs: neither is legal while a stream of this
        # process is being captured, and the garbage collector runs whenever it likes - also in the middle of
        # TrainStep's or sample()'s capture, where a dead plan of some earlier model then broke the graph being built
        # (segmentation fault at a later replay, only in long processes: round 4).  A plan that dies during a capture is
        # parked and destroyed by the next _Plan creation outside one.
        try:
            if self.handle:
                if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                    _PARKED.append(self.handle)
                else:
                    lib.tdx_unet_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


_PARKED = []   # handles of plans that died while a capture was under way


def _destroy_parked():
    if _PARKED and not torch.cuda.is_current_stream_capturing():
        while _PARKED:
            lib.tdx_unet_destroy(_PARKED.pop())


class _PtrTable:
    """ctypes array of device pointers, rebuilt only when a tensor moves."""

    def __init__(self):
        self.key = None
        self.arr = None

    def get(self, tensors):
        key = tuple(0 if t is None else t.data_ptr() for t in tensors)
        if key != self.key:
            self.arr = (C.c_void_p * len(key))(*[k or None for k in key])
            self.key = key
        return self.arr


def _dptr(tensor):
    return None if tensor is None else tensor.data_ptr()


def _cond_tensor(kind: int, y):
    """The conditioning input as the kernels read it: fp32 text embeddings for the LAION network, int64 labels for
    every other one (forward and the sampling loop)."""
    if y is None:
        return None
    return y.contiguous().float() if kind == KIND_LAION else y.contiguous().to(torch.int64)


NULL_LABEL = -1   # the null condition of the class-conditional UNet (any negative label): emb = t_emb


def _with_null_cond(kind: int, y):
    """``y`` (n rows, as ``_cond_tensor`` returns it) followed by n rows of the null condition - label ``NULL_LABEL`` or
    an all-zero text embedding: the condition of a guided batch of 2n rows."""
    return torch.cat([y, torch.zeros_like(y) if kind == KIND_LAION else torch.full_like(y, NULL_LABEL)]).contiguous()


class _UNetFunction(torch.autograd.Function):
    """eps_hat = UNet(x, t[, y]); backward returns every parameter gradient."""

    @staticmethod
    def forward(ctx, module, mode, x, t, y, *params):
        # grad mode is off inside Function.forward, so the caller decides the mode
        if x.requires_grad and module._arch.kind == KIND_LATENT:
            raise _lib.TdxError("x.requires_grad: the latent MLP computes parameter gradients only; detach the input")
        # the reference's module is differentiable in x like any nn.Module (diffusion.py:109-162): the UNets
        # form d loss / d x on request (the input gradient of initial_conv, one extra launch)
        ctx.x_grad = bool(x.requires_grad)
        out, plan, mode = module._run_forward(x, t, y, mode=mode)
        module._live_ctx.add(ctx)   # weak: a graph dropped without backward() leaves by itself
        ctx.module = module
        ctx.plan = plan
        ctx.generation = plan.generation
        ctx.saved_for = mode
        ctx.n_params = len(params)
        return out

    @staticmethod
    def backward(ctx, d_out):
        module, plan = ctx.module, ctx.plan
        if plan.generation != ctx.generation:
            raise _lib.TdxError(
                "backward() after another forward() on the same batch size: the saved "
                "activations live in a per-batch-size workspace and were overwritten")
        flat, views = module._grad_buffers(d_out.device)
        gx = None
        if ctx.x_grad:
            gx = torch.empty((plan.batch,) + tuple(d_out.shape[1:]), dtype=torch.float32, device=d_out.device)
            check(lib.tdx_unet_request_input_grad(plan.handle, gx.data_ptr()), "tdx_unet_request_input_grad")
        try:
            module._run_backward(plan, d_out.contiguous(), views)
        except BaseException:
            # the one-shot request must not outlive this call: gx is freed when the exception unwinds, and a later
            # backward on the same plan would write d loss / d x into that memory
            if gx is not None:
                lib.tdx_unet_request_input_grad(plan.handle, None)
            raise
        # The gradients are views of ONE module-wide flat buffer.  With a single forward in the graph
        # autograd copies them into p.grad before anything can overwrite the buffer; with several
        # forwards of the same module in one graph (different batch sizes: the same size raises above)
        # the next node's backward would overwrite them while they are still queued for accumulation,
        # so they are detached from the buffer first.
        shared = len(module._live_ctx) > 1
        module._live_ctx.discard(ctx)
        grads = tuple(views[name].clone() if shared else views[name] for name in module._param_order)
        return (None, None, gx, None, None) + grads


class NoiseModelBase(nn.Module):
    """Shared implementation; ``NoiseModel`` in diffusion.py / conditional_diffusion.py /
    conditional_diffusion_laion.py fixes ``num_classes`` and the architecture."""

    MAX_PLANS = 6   # per-(device, batch, resolution) plans kept per module (LRU; see _plan)

    def __init__(self, time_dim: Optional[int] = None, num_classes: int = 0, arch: _Arch = ARCH_MNIST):
        super().__init__()
        time_dim = arch.time_dim if time_dim is None else int(time_dim)
        # the reference accepts any width (diffusion.py:16-25): so do the UNets (multiples of 256 up to 1024
        # on the fast row kernels, anything else up to 4096 on generic ones; the sinusoidal embedding of the
        # LAION model needs 4 columns).  The latent MLP's fused kernels are built for its default only.
        lo = 4 if arch.kind == KIND_LAION else 1
        if not lo <= time_dim <= 4096 or (arch.kind == KIND_LATENT and time_dim != arch.time_dim):
            raise ValueError(f"time_dim must be in [{lo}, 4096] (reference default {arch.time_dim}; the latent "
                             "model takes its default only)")
        if arch.kind == KIND_LAION and num_classes:
            raise ValueError("the LAION model is conditioned on text embeddings, not class labels")
        self.time_dim = time_dim
        self.num_classes = int(num_classes)
        self._arch = arch
        if arch.kind == KIND_LATENT:
            self._init_latent(arch, time_dim)
        else:
            self._init_unet(arch, time_dim)
        cond = self.num_classes > 0
        self._slot_names = param_slot_names(cond, arch.time_name, arch.init_name, arch.final_name)
        self._buf_names = buffer_slot_names()
        # layout of the flat parameter / gradient buffers: the parameters of the LAST backward stage
        # (time path, class embedding, first layer) sit together so that the final, exposed bucket
        # of the gradient all-reduce is one contiguous slice = one collective
        names = [n for n in self._slot_names if n is not None]
        self._param_order = ([n for n in names if n.startswith("time_proj")]
                             + [n for n in names if not n.startswith("time_proj")])
        self._plans = {}
        self._ptab_p, self._ptab_b, self._ptab_g = _PtrTable(), _PtrTable(), _PtrTable()
        self._grad_flat = None
        self._grad_views = None
        self._buf_epoch = 0
        self._precision = 0   # TDX_PREC_F32
        self._bn_allreduce = self._bn_cb = self._bn_buf = self._bn_error = None
        self._stream_mode = -1   # -1 default schedule; 0 single stream (required while a step is captured in a graph)
        self._live_ctx = weakref.WeakSet()   # autograd nodes of this module whose backward has not run yet

    def _init_latent(self, arch, time_dim):
        # registration order == latent_diffusion.py:23-105
        if self.num_classes <= 0:
            raise ValueError("the latent noise model is class-conditional (num_classes > 0)")
        self.time_embedding = nn.Sequential(nn.Linear(1, time_dim), nn.SiLU(), nn.Linear(time_dim, time_dim))
        self.class_embedding = nn.Embedding(self.num_classes, time_dim)
        self.initial_fc = nn.Linear(arch.in_shape[0], arch.x0)
        for name, cin, mid, cout in arch.enc:
            setattr(self, name, nn.Sequential(*_lin_bn_relu(cin, mid), *_lin_bn_relu(mid, cout)))
        self.bottleneck = nn.Sequential(*_lin_bn_relu(arch.bottleneck, arch.bottleneck))
        for name, cin, mid, cout in arch.dec:
            setattr(self, name, nn.Sequential(*_lin_bn_relu(cin, mid), *_lin_bn_relu(mid, cout)))
        self.final_fc = nn.Linear(512, arch.in_shape[0])
        for k, c in ((1, 64), (2, 128), (3, 256)):
            setattr(self, f"time_proj{k}", nn.Linear(time_dim, c))

    def _init_unet(self, arch, time_dim):
        # registration order == reference (diffusion.py:19-107,
        # conditional_diffusion_laion.py:239-301): identical state_dict order and identical
        # default init under the same seed
        first_in = 1 if arch.kind == KIND_MNIST else time_dim
        setattr(self, arch.time_name,
                nn.Sequential(nn.Linear(first_in, time_dim), nn.SiLU(), nn.Linear(time_dim, time_dim)))
        if self.num_classes > 0:
            self.class_embedding = nn.Embedding(self.num_classes, time_dim)
        self.initial_conv = nn.Conv2d(arch.in_shape[0], arch.x0, 3, padding=1)
        for name, cin, cout in arch.enc:
            setattr(self, name, nn.Sequential(*_conv_bn_relu(cin, cout), *_conv_bn_relu(cout, cout)))
        self.bottleneck = nn.Sequential(*_conv_bn_relu(arch.bottleneck, arch.bottleneck))
        for name, cin, cout in arch.dec:
            setattr(self, name, nn.Sequential(*_conv_bn_relu(cin, cout), *_conv_bn_relu(cout, cout)))
        self.final_conv = nn.Conv2d(64, arch.in_shape[0], 3, padding=1)
        if arch.kind == KIND_MNIST:
            self.pool = nn.MaxPool2d(2, ceil_mode=True)
            self.up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
        for k, (_, _, c) in zip((1, 2, 3), arch.enc):
            setattr(self, f"time_proj{k}", nn.Conv2d(time_dim, c, 1))
        if arch.kind == KIND_LAION:  # registered after the projections in the reference
            self.pool = nn.MaxPool2d(2)
            self.up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)

    # ---------------------------------------------------------------- precision
    def set_compute_dtype(self, dtype) -> "NoiseModelBase":
        """Arithmetic of the 3x3 convolutions (not in the reference, which is fp32-only; BASELINE.json
        configs[3]/[4] name bf16): ``torch.float32`` (default, exact fp32 MFMA) or ``torch.bfloat16``
        (bf16 MFMA operands, fp32 accumulation; parameters, gradients, BatchNorm and the time MLP stay fp32;
        the UNets also store activations in bf16; the latent MLP - BASELINE.json configs[3] - runs its Linear layers
        on the bf16 MFMA and keeps fp32 tensors).  Applies to forwards issued afterwards; tolerance in
        tests/test_gpu_bf16.py / tests/test_gpu_latent.py."""
        name = {torch.float32: 0, torch.bfloat16: 1, "fp32": 0, "f32": 0, "bf16": 1}.get(dtype)
        if name is None:
            raise ValueError("compute dtype must be torch.float32 or torch.bfloat16")
        self._precision = name
        return self

    @property
    def compute_dtype(self):
        return torch.bfloat16 if self._precision == 1 else torch.float32

    def set_bn_sync(self, allreduce=None) -> "NoiseModelBase":
        """Synchronised BatchNorm for data-parallel training (not in the reference, which has no
        distributed code): ``allreduce(tensor)`` must sum a float64 CUDA tensor in place
        across ranks, ordered on the current stream (``torch.distributed.all_reduce`` does).  Train-mode
        statistics and the backward sums are then taken over the global batch, so an N-rank step equals
        the single-process step on the concatenated batch.  ``None`` restores rank-local statistics."""
        if allreduce is not None and self._arch.kind == KIND_LATENT:
            raise ValueError("SyncBN is implemented for the convolutional networks")
        self._bn_allreduce = allreduce
        if allreduce is None:
            self._bn_cb = None
        else:
            def cb(user, ptr, n, stream):   # called by libtdx between two launches on `stream`
                try:
                    buf = self._bn_buf
                    if buf is None or ptr != buf.data_ptr() or n > buf.numel():
                        return -4
                    allreduce(buf[:n])
                    return 0
                except Exception as e:      # an exception cannot cross the C frame: report a status
                    self._bn_error = e
                    return -4
            self._bn_cb = _BN_CALLBACK(cb)
        for plan in self._plans.values():
            plan.bn_sync = None
        return self

    def _apply_bn_sync(self, plan, device):
        want = self._bn_cb
        if plan.bn_sync is want:
            return
        if want is None:
            check(lib.tdx_unet_set_bn_sync(plan.handle, None, None, None), "tdx_unet_set_bn_sync")
        else:
            if self._bn_buf is None or self._bn_buf.device != device:
                self._bn_buf = torch.zeros(2 * 1024 + 8, dtype=torch.float64, device=device)   # 2C + 1, C <= 1024
            check(lib.tdx_unet_set_bn_sync(plan.handle, C.cast(want, C.c_void_p), None, self._bn_buf.data_ptr()),
                  "tdx_unet_set_bn_sync")
        plan.bn_sync = want

    def _apply_streams(self, plan):
        want = self._stream_mode
        if plan.stream_mode != want:
            check(lib.tdx_unet_set_streams(plan.handle, want), "tdx_unet_set_streams")
            plan.stream_mode = want

    def _apply_precision(self, plan):
        if plan.precision != self._precision:
            check(lib.tdx_unet_set_precision(plan.handle, self._precision), "tdx_unet_set_precision")
            plan.precision = self._precision
            plan.infer_key = None

    # ---------------------------------------------------------------- plumbing
    def _named(self):
        d = dict(self.named_parameters())
        d.update(dict(self.named_buffers()))
        return d

    def _plan(self, batch: int, device: torch.device, hw: int = 0) -> _Plan:
        """One plan per (device, batch[, resolution]).  ``hw``: input side when it differs from the
        reference's (LAION network only)."""
        dev = device.index if device.index is not None else torch.cuda.current_device()
        key = (dev, batch) if not hw else (dev, batch, hw)
        p = self._plans.pop(key, None)
        if p is None:
            p = _Plan(batch, self.num_classes, device, self._arch.kind, hw,
                      0 if self.time_dim == self._arch.time_dim else self.time_dim)
            # A plan owns its workspace (~12 MB per image for the MNIST UNet: 3 GB at B = 256).  A loop over many
            # batch sizes (ragged last batches, evaluation sweeps) must not accumulate them: keep the MAX_PLANS most
            # recently used; an evicted plan stays alive only while an autograd graph still refers to it.
            while len(self._plans) >= self.MAX_PLANS:
                self._plans.pop(next(iter(self._plans)))
        self._plans[key] = p   # (re-)inserted last: dicts keep insertion order, so the first key is the LRU one
        return p

    def _input_hw(self, x) -> int:
        """0 for the reference resolution, else the (square) side of x."""
        shp = tuple(self._arch.in_shape)
        return 0 if len(shp) != 3 or x.shape[-1] == shp[-1] else int(x.shape[-1])

    def _param_ptrs(self):
        d = self._named()
        tensors = [None if n is None else d[n] for n in self._slot_names]
        for tns in tensors:
            if tns is not None and (not tns.is_cuda or tns.dtype != torch.float32 or not tns.is_contiguous()):
                raise _lib.TdxError("parameters must be contiguous fp32 CUDA tensors (call .to('cuda'))")
        return self._ptab_p.get(tensors), tensors

    def _buffer_ptrs(self):
        d = self._named()
        tensors = [d[n] for n in self._buf_names]
        return self._ptab_b.get(tensors), tensors

    def _grad_buffers(self, device):
        """One flat fp32 gradient buffer with a view per parameter (reference shapes)."""
        if self._grad_flat is None or self._grad_flat.device != device:
            d = dict(self.named_parameters())
            total = sum(d[n].numel() for n in self._param_order)
            self._grad_flat = torch.zeros(total, dtype=torch.float32, device=device)
            views, o = {}, 0
            for n in self._param_order:
                k = d[n].numel()
                views[n] = self._grad_flat[o:o + k].view(d[n].shape)
                o += k
            self._grad_views = views
        return self._grad_flat, self._grad_views

    def _mode(self) -> int:
        if self.training:
            return MODE_TRAIN
        return MODE_EVAL_GRAD if torch.is_grad_enabled() else MODE_INFER

    def _check_inputs(self, x, t, y):
        if not x.is_cuda:
            raise _lib.TdxError(
                "tiny_diffusion_amd runs on MI355X only: got a CPU tensor and there is no "
                "CPU fallback (the CPU restatement lives in oracle/ and is test-only)")
        shp = tuple(self._arch.in_shape)
        if self._arch.kind == KIND_LAION and x.dim() == 4 and x.shape[1] == shp[0] and x.shape[2] == x.shape[3] \
                and x.shape[2] % 8 == 0 and 32 <= x.shape[2] <= 512:
            pass  # fully convolutional (conditional_diffusion_laion.py:304-332): (B,4,H,H), H a multiple of 8
        elif x.dim() != 1 + len(shp) or tuple(x.shape[1:]) != shp:
            raise ValueError(f"x must be (B,{','.join(map(str, shp))}), got {tuple(x.shape)}")
        if t.shape != (x.shape[0],):
            raise ValueError("t must have shape (B,)")
        if self._arch.kind == KIND_LAION:
            if y is None or tuple(y.shape) != (x.shape[0], self.time_dim):
                raise ValueError(f"text_embeds must have shape (B,{self.time_dim})")
            if not y.is_cuda:
                raise _lib.TdxError("text_embeds must be a CUDA tensor")
            return
        if (self.num_classes > 0) != (y is not None):
            raise ValueError("class labels y are required exactly for the conditional model")
        if y is not None and y.shape != (x.shape[0],):
            raise ValueError("y must have shape (B,)")

    def _run_forward(self, x, t, y, mode: Optional[int] = None):
        self._check_inputs(x, t, y)
        B = x.shape[0]
        if B == 0:
            # torch's layers pass an empty batch through in eval mode; train-mode BatchNorm has no
            # statistics to compute (torch yields NaN running buffers there: refused instead)
            if (self._mode() if mode is None else mode) == MODE_TRAIN:
                raise ValueError("empty batch in train mode: BatchNorm statistics are undefined")
            return x.new_empty((0,) + tuple(self._arch.in_shape), dtype=torch.float32), None, MODE_INFER
        mode = self._mode() if mode is None else mode
        plan, pptr, bptr, st = self._plan_ptrs(x, pack=mode == MODE_INFER)
        self._apply_bn_sync(plan, x.device)
        self._apply_streams(plan)
        x = x.contiguous().float()
        t = t.contiguous().to(torch.int64)
        y = _cond_tensor(self._arch.kind, y)
        out = torch.empty((B,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
        if mode != MODE_INFER:
            plan.infer_key = None
            plan.generation += 1
            if mode == MODE_TRAIN:
                self._buf_epoch += 1
        check(lib.tdx_unet_forward(plan.handle, pptr, bptr, x.data_ptr(), t.data_ptr(), _dptr(y), out.data_ptr(),
                                   plan.workspace.data_ptr(), plan.ws_bytes, B, mode, st),
              "tdx_unet_forward")
        return out, plan, mode

    def _plan_ptrs(self, x, pack: bool = True):
        """(plan, parameter pointers, buffer pointers, stream) of a launch on ``x``: the plan of its batch size and
        resolution in the module's precision.  ``pack`` (every MODE_INFER launch): the packed weights / folded BN are
        reused until a parameter or buffer changes."""
        plan = self._plan(x.shape[0], x.device, self._input_hw(x))
        self._apply_precision(plan)
        pptr, ptens = self._param_ptrs()
        bptr, btens = self._buffer_ptrs()
        st = torch.cuda.current_stream(x.device).cuda_stream
        if pack:
            # running statistics are updated by kernels (no torch version bump): _buf_epoch
            key = tuple(tn._version for tn in ptens if tn is not None) + tuple(tn._version for tn in btens) \
                + tuple(self._ptab_p.key) + tuple(self._ptab_b.key) + (self._buf_epoch,)
            if plan.infer_key != key:
                check(lib.tdx_unet_pack(plan.handle, pptr, bptr, st), "tdx_unet_pack")
                plan.infer_key = key
        return plan, pptr, bptr, st

    def _run_eval_step(self, x, y, coef, counter, t_idx, t_vec, eps, z=None, philox_seed: int = 0, tau=None,
                       S: int = 0, guidance_scale: Optional[float] = None, clip=None, hist=None, known=None,
                       mask=None, dyn=None):
        """One reverse step of sample() in place on ``x``: the step index is read from and decremented in device
        memory, so the call can sit in a HIP graph.  Nothing but ``z`` / ``philox_seed``: tdx_unet_eval_step, the
        reference's chain with ``coef`` its (T,3) table.  Anything else: tdx_unet_eval_step_update.  ``tau``: the device
        timesteps of a schedule of ``S`` steps.  ``guidance_scale``: the guided step - ``x``, ``y`` and ``eps`` hold 2n
        rows, the second half under the null condition, ``z`` n rows.  ``clip=(lo, hi)`` (infinite bounds for none): the
        x0 form, ``coef`` the (S,5) table of ``TimestepSchedule.x0_form``; with ``hist`` the multistep form against that
        history buffer, ``coef`` the (S,5) table of ``MultistepSchedule.multistep_form`` (no ``z``, no seed).
        ``known`` / ``mask`` (with ``clip``; both or neither): the masked step of inpainting - contiguous fp32 device
        tensors of n rows.  ``dyn=(rank, frac, thr)`` (with a finite ``clip``, the data range): dynamic thresholding -
        the quantile as ``schedule._quantile_rank`` gives it and the caller's (n, 2) fp32 device buffer; the step is
        tdx_unet_eval_step_update_dyn (no fused epilogue)."""
        if dyn is not None and clip is None:
            raise ValueError("the thresholded step runs in x0 form: give clip, the data range")
        if (known is None) != (mask is None):
            raise ValueError("known and mask go together")
        if known is not None and clip is None:
            raise ValueError("the masked step runs in x0 form: give clip (infinite bounds for none)")
        plan, pptr, bptr, st = self._plan_ptrs(x)
        g = guidance_scale is not None
        form = _lib.STEP_MS if hist is not None else _lib.STEP_EPS if clip is None else _lib.STEP_X0
        lo, hi = (0.0, 0.0) if clip is None else (float(clip[0]), float(clip[1]))
        if form == _lib.STEP_MS:
            z, philox_seed = None, 0
        if dyn is not None:
            rank, frac, thr = dyn
            check(lib.tdx_unet_eval_step_update_dyn(plan.handle, pptr, bptr, x.data_ptr(), _dptr(y), _dptr(z),
                                                    coef.data_ptr(), _dptr(tau), int(S), counter.data_ptr(),
                                                    t_idx.data_ptr(), t_vec.data_ptr(), eps.data_ptr(),
                                                    x.numel() // 2 if g else x.numel(), plan.workspace.data_ptr(),
                                                    plan.ws_bytes, x.shape[0], philox_seed, form, int(g),
                                                    float(guidance_scale) if g else 0.0, lo, hi, _dptr(hist),
                                                    _dptr(known), _dptr(mask), int(rank), float(frac), thr.data_ptr(),
                                                    st), "tdx_unet_eval_step_update_dyn")
        elif form == _lib.STEP_EPS and not g and tau is None:
            check(lib.tdx_unet_eval_step(plan.handle, pptr, bptr, x.data_ptr(), _dptr(y), _dptr(z), coef.data_ptr(),
                                         counter.data_ptr(), t_idx.data_ptr(), t_vec.data_ptr(), eps.data_ptr(),
                                         x.numel(), plan.workspace.data_ptr(), plan.ws_bytes, x.shape[0], philox_seed,
                                         st), "tdx_unet_eval_step")
        else:
            check(lib.tdx_unet_eval_step_update(plan.handle, pptr, bptr, x.data_ptr(), _dptr(y), _dptr(z),
                                                coef.data_ptr(), _dptr(tau), int(S), counter.data_ptr(),
                                                t_idx.data_ptr(), t_vec.data_ptr(), eps.data_ptr(),
                                                x.numel() // 2 if g else x.numel(), plan.workspace.data_ptr(),
                                                plan.ws_bytes, x.shape[0], philox_seed, form, int(g),
                                                float(guidance_scale) if g else 0.0, lo, hi, _dptr(hist), _dptr(known),
                                                _dptr(mask), st), "tdx_unet_eval_step_update")

    def _drop_sampling_tables(self, x):
        """The eval steps on ``x`` that follow take the direct time path (tdx_unet_drop_sampling_tables): bit for bit
        what the eager chain computes, at the price of the time path's launches in every step.  The next
        ``_prepare_sampling`` builds the tables again.  No-op for the latent MLP (it has none)."""
        if self._arch.kind == KIND_LATENT:
            return
        plan = self._plan_ptrs(x)[0]
        check(lib.tdx_unet_drop_sampling_tables(plan.handle), "tdx_unet_drop_sampling_tables")

    def _prepare_sampling(self, x, y, T: int, tau=None):
        """Once per sample() call, before the reverse loop (and before any graph capture): the per-t table of
        ``time_proj_k(time MLP(t))`` and the per-sample table of ``W_k c`` (c = class / text embedding), so that
        every reverse step replaces the time path's launches by one look-up (tdx_unet_prepare_sampling; SURVEY.md 7:
        the projections are linear in the embedding).  ``y`` must be the very tensor later handed to
        ``_run_eval_step`` (the tables are tied to its pointer).  ``tau``: device timesteps of a schedule of ``T``
        steps, the table rows are then built at them (tdx_unet_prepare_sampling_sched).  No-op for the latent MLP."""
        if self._arch.kind == KIND_LATENT:
            return
        plan, pptr, _, st = self._plan_ptrs(x)
        head = (plan.handle, pptr, _dptr(y), x.shape[0])
        if tau is None:
            check(lib.tdx_unet_prepare_sampling(*head, int(T), st), "tdx_unet_prepare_sampling")
        else:
            check(lib.tdx_unet_prepare_sampling_sched(*head, tau.data_ptr(), int(T), st),
                  "tdx_unet_prepare_sampling_sched")

    def _run_backward(self, plan: _Plan, d_out, grad_views, stage_lo: int = 0, stage_hi: Optional[int] = None):
        pptr, _ = self._param_ptrs()
        gt = [None if n is None else grad_views[n] for n in self._slot_names]
        gptr = self._ptab_g.get(gt)
        nst = lib.tdx_unet_backward_stages()
        stage_hi = nst if stage_hi is None else stage_hi
        st = torch.cuda.current_stream(d_out.device).cuda_stream
        check(lib.tdx_unet_backward(plan.handle, pptr, gptr, d_out.data_ptr(), plan.workspace.data_ptr(),
                                    plan.ws_bytes, plan.batch, stage_lo, stage_hi, st),
              "tdx_unet_backward")

    # ------------------------------------------------------------------ forward
    def _forward_impl(self, x, t, y):
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if not needs_grad or (x.shape[0] == 0 and not self.training):
            return self._run_forward(x, t, y)[0]
        d = dict(self.named_parameters())
        params = [d[n] for n in self._param_order]
        mode = MODE_TRAIN if self.training else MODE_EVAL_GRAD
        return _UNetFunction.apply(self, mode, x, t, y, *params)
