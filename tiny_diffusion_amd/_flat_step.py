"""What the three fused training steps (``train.TrainStep``, ``vae.VAETrainStep``,
``diffusion_transformer.TransformerTrainStep``) share: parameters, gradient, Adam moments and the optional parameter
average in flat fp32 buffers, the one optimizer launch over them, the training objective, the EMA interface, the HIP
graph protocol and the workspace cache.  A subclass adds its constructor arguments, its batch checks, its
``*_loss_grads`` core and its eager body ("The shared base of the three training steps")."""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import struct

import torch

from . import _lib
from ._lib import lib, check
from .schedule import _prediction, _snr_gamma, loss_weights, timestep_probs


# ---------------------------------------------------------------- arguments
def _f32(v: float) -> float:
    """``v`` rounded to fp32, as a C ``float`` argument is: the host arithmetic below then repeats libtdx's."""
    return struct.unpack("f", struct.pack("f", v))[0]


def _number(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{what} must be a finite number, got {v!r}")
    return float(v)


def _seed_arg(v, what):
    if v is not None and (isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 64):
        raise ValueError(f"{what} must be None or an integer in [0, 2**64)")
    return v


def _i64(v: int) -> int:
    """A uint64 as the int64 with the same bits (torch has no uint64 arithmetic; the kernels read the words as uint64)."""
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _betas_arg(betas):
    if not isinstance(betas, (tuple, list)) or len(betas) != 2:
        raise ValueError("betas must be a pair of numbers")
    betas = (_number(betas[0], "betas[0]"), _number(betas[1], "betas[1]"))
    if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
        raise ValueError("betas must lie in [0, 1)")
    return betas


def _max_grad_norm_arg(v):
    if v is not None and not _number(v, "max_grad_norm") > 0:
        raise ValueError("max_grad_norm must be None or > 0")
    return None if v is None else float(v)


def _ema_args(ema_decay, ema_warmup):
    if ema_decay is None:
        if ema_warmup:
            raise ValueError("ema_warmup=True needs an ema_decay")
    elif isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 <= ema_decay <= 1.0:
        raise ValueError("ema_decay must be None or a number in [0, 1]")
    return None if ema_decay is None else float(ema_decay), bool(ema_warmup)


# ---------------------------------------------------------------- schedules
def cosine_annealing_lr(step: int, base_lr: float, T_max: int, eta_min: float = 0.0) -> float:
    """Learning rate after ``step`` calls of ``CosineAnnealingLR(T_max, eta_min).step()``
    (conditional_diffusion_laion.py:436-438, 473: stepped once per BATCH although T_max counts
    epochs, so the rate swings between base_lr and eta_min with period 2*T_max batches -
    reproduced as written; the closed form equals torch's chained recursion)."""
    return eta_min + (base_lr - eta_min) * (1.0 + math.cos(math.pi * step / T_max)) / 2.0


def ema_decay_at(step_index: int, decay: float, warmup: bool) -> float:
    """Decay of the parameter average at optimizer step ``step_index`` (0 at the first one): ``decay``, or with
    ``warmup`` ``min(decay, (1 + k) / (10 + k))`` - the average follows the parameters closely while they still move
    fast (0.1 at the first step, 2/11 at the second) and reaches ``decay`` from the first k with
    ``(1 + k) / (10 + k) >= decay`` on."""
    if not warmup:
        return decay
    k = int(step_index)
    return min(decay, (1 + k) / (10 + k))


def adam_hyper(lr, betas, step_count, gscale, ema_a=None) -> list:
    """``[lr / bc1, 1 / sqrt(bc2), grad_scale[, 1 - decay]]`` of optimizer step ``step_count``: the device scalars of a
    captured step, with tdx_adam_step's own arithmetic (``lr`` and the betas arrive there as C floats and are widened
    to double), so that a captured step and an eager one update bit-identically."""
    bc1 = 1.0 - math.pow(_f32(betas[0]), step_count)
    bc2 = 1.0 - math.pow(_f32(betas[1]), step_count)
    hyper = [_f32(lr) / bc1, 1.0 / math.sqrt(bc2), gscale]
    return hyper if ema_a is None else hyper + [ema_a]


class FlatStep:
    """Base of the fused training steps.  A subclass's constructor checks its arguments, calls ``_init_optimizer`` and
    then ``_flatten`` (the first device work).  For ``use_graph`` it provides ``_alloc_static`` and ``_static_step`` and
    drives ``_graph_ready`` / ``_replay``; for the workspace cache ``_workspace_floats``."""

    # a step without timesteps (the VAE's) never calls _check_timestep_sampler
    timestep_sampler = sample_losses = last_t = None
    importance_weights = False

    def _init_optimizer(self, lr, betas, eps, max_grad_norm, ema_decay=None, ema_warmup=False, use_graph=False):
        self.lr, self.betas, self.eps, self.max_grad_norm = lr, betas, eps, max_grad_norm
        self.ema_decay, self.ema_warmup = ema_decay, ema_warmup
        self.use_graph = use_graph
        self.step_count = 0
        self.ema = None             # flat average of flat_param (_flatten)
        self._ema_swapped = False   # inside ema_weights(): flat_param holds the average, ema the parameters
        self._clip_scratch = None
        self._graph = self._graph_key = self._hyper = None
        self._ws = {}               # batch size -> workspace of the subclass's *_loss_grads entry
        self._gws = None            # the workspace whose address the captured graph holds: owned by the graph's owner

    # ------------------------------------------------------------------ setup
    def _require_fp32_cuda(self, named, whose):
        dev = named[0][1].device
        for k, p in named:
            if p.device.type != "cuda" or p.device != dev or p.dtype != torch.float32:
                raise _lib.TdxError(f"{type(self).__name__} needs {whose} fp32 parameters on one CUDA (ROCm) device "
                                    f"(call .to('cuda') first): {k} is {p.dtype} on {p.device}")

    def _flatten(self, named, grad_buffers=None):
        """The ordered ``(name, parameter)`` list becomes views of one flat fp32 buffer, with the gradient, Adam's two
        moments and, under ``ema_decay``, the average beside it.  ``grad_buffers``: the model's own ``device ->
        (flat_grad, grad_views)`` where its backward writes there; without it the gradient buffer is built here, with
        the per-parameter pointer tables the ``*_loss_grads`` entries take."""
        self.device = dev = named[0][1].device
        flat = torch.empty(sum(p.numel() for _, p in named), dtype=torch.float32, device=dev)
        self.offsets = {}
        o = 0
        for k, p in named:
            n = p.numel()
            flat[o:o + n].copy_(p.detach().reshape(-1))
            p.data = flat[o:o + n].view(p.shape)      # parameters become views of the flat buffer
            self.offsets[k] = (o, o + n)
            o += n
        self.flat_param = flat
        if grad_buffers is not None:
            self.flat_grad, self.grad_views = grad_buffers(dev)
        else:
            self.flat_grad = torch.zeros_like(flat)
            self.grad_views = {k: self.flat_grad[self.offsets[k][0]:self.offsets[k][1]].view(p.shape) for k, p in named}
            base, gbase = flat.data_ptr(), self.flat_grad.data_ptr()
            self._p_ptrs = (C.c_void_p * len(named))(*[base + 4 * self.offsets[k][0] for k, _ in named])
            self._g_ptrs = (C.c_void_p * len(named))(*[gbase + 4 * self.offsets[k][0] for k, _ in named])
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        if self.ema_decay is not None:
            self.ema = flat.clone()

    def _check_attached(self):
        name = type(self).__name__
        for (k, p), want in zip(self._params(), self._p_ptrs):
            if p.data_ptr() != want:
                raise _lib.TdxError(f"{k} no longer lives in {name}'s flat parameter buffer: the module was moved or its "
                                    f"parameters were replaced after the step was built (build a new {name})")

    # -------------------------------------------------------------- optimizer
    def _ema_a(self) -> float:
        """1 - decay of the optimizer step that ``step_count`` (already incremented) counts, in double: the
        conversion to the kernel's fp32 scalar is its one rounding."""
        return 1.0 - ema_decay_at(self.step_count - 1, self.ema_decay, self.ema_warmup)

    def _new_clip_scratch(self):
        return torch.empty(lib.tdx_adam_clip_scratch_bytes(), dtype=torch.uint8, device=self.device)

    def _adam(self, hyper=None, gscale=1.0, st=None):
        """The one optimizer launch over the flat buffers.  ``hyper``: the device scalars of a step being captured
        (``adam_hyper``); an eager step hands ``lr``, the betas and ``step_count`` to the C entry, which derives them.
        ``max_grad_norm``: ``clip_grad_norm_`` fused into the pass (conditional_diffusion_laion.py:469-472) - the flat
        buffer holds every gradient, so one sum of squares gives the total norm and the kernel applies the coefficient.
        ``st``: the current stream's handle where the caller already looked it up (the latent-MLP step is bound by
        launch latency: microseconds of host work per step show)."""
        if st is None:
            st = torch.cuda.current_stream(self.device).cuda_stream
        bufs = [self.flat_param.data_ptr(), self.flat_grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()]
        ema = self.ema is not None
        if ema:
            bufs.append(self.ema.data_ptr())
        bufs.append(self.flat_param.numel())
        b1, b2 = self.betas
        hyp = None if hyper is None else hyper.data_ptr()
        if self.max_grad_norm is not None:
            if self._clip_scratch is None:
                self._clip_scratch = self._new_clip_scratch()
            tail = (hyp, self._clip_scratch.data_ptr(), st)
            clip = float(self.max_grad_norm)
            if ema:
                check(lib.tdx_adam_ema_step_clip(*bufs, self.lr, b1, b2, self.eps, self.step_count, gscale, clip,
                                                 self._ema_a(), *tail), "tdx_adam_ema_step_clip")
            else:
                check(lib.tdx_adam_step_clip(*bufs, self.lr, b1, b2, self.eps, self.step_count, gscale, clip, *tail),
                      "tdx_adam_step_clip")
        elif hyper is not None:   # being captured: the scalars come from device memory at replay time
            if ema:
                check(lib.tdx_adam_ema_step_dev(*bufs, hyp, b1, b2, self.eps, st), "tdx_adam_ema_step_dev")
            else:
                check(lib.tdx_adam_step_dev(*bufs, hyp, b1, b2, self.eps, st), "tdx_adam_step_dev")
        elif ema:
            check(lib.tdx_adam_ema_step(*bufs, self.lr, b1, b2, self.eps, self.step_count, gscale, self._ema_a(), st),
                  "tdx_adam_ema_step")
        else:
            check(lib.tdx_adam_step(*bufs, self.lr, b1, b2, self.eps, self.step_count, gscale, st), "tdx_adam_step")

    # -------------------------------------------------------------- objective
    def _check_objective(self, prediction, loss_weighting, snr_gamma):
        """Validate and record the objective (``ValueError`` before anything changes).  What the eager body reads of it:
        ``self.prediction`` (which q_sample entry) and ``self._w_table`` (None: the unweighted loss entry)."""
        prediction, gamma = _prediction(prediction), _snr_gamma(snr_gamma)
        w_cpu = None if loss_weighting is None else loss_weights(self.diffusion, prediction, loss_weighting, gamma)
        named = loss_weighting is None or isinstance(loss_weighting, str)
        self.prediction, self.snr_gamma = prediction, gamma
        self.loss_weighting = loss_weighting if named else "table"
        self._w_cpu = None if named else w_cpu      # a user table, checked and rounded; named tables: the diffusion's

    def _upload_weights(self):
        if self.loss_weighting is None:
            self._w_table = None     # device (T,) fp32 loss weights; None: unweighted, the plain loss entry
        elif self._w_cpu is not None:
            self._w_table = self._w_cpu.to(self.device)
        else:   # the diffusion's per-device copy, shared by every step on it
            self._w_table = self.diffusion.loss_weight_table(self.device, self.prediction, self.loss_weighting,
                                                             self.snr_gamma)

    def set_objective(self, prediction: str = "eps", loss_weighting=None, snr_gamma: float = 5.0):
        """Change the training objective of an existing step (the constructor's three keywords, same errors): the
        parameters, optimizer state and plans stay; a captured step is dropped and captured again on the next calls,
        because the graph holds the launches of the objective it was captured with.  The defaults give back exactly the
        default step's launches (``tools/gpu_objective_cost.py`` alternates the two on one step).  Under a
        ``timestep_sampler`` the step's own weights are rebuilt from the new table; the loss history stays."""
        self._check_objective(prediction, loss_weighting, snr_gamma)
        self._upload_weights()
        self._rebuild_timestep_table()
        self._drop_graph()

    # ------------------------------------------------------- timestep sampler
    # Which timestep each sample sees when step() is not given one.  The sampler's state is device
    # memory of the step: the CDF the draw inverts (_ts_cdf), the weights the loss entries read in place of _w_table
    # (_w_eff = objective weight / (T p_t) under importance weights), and for "loss_second_moment" the loss history.
    def _check_timestep_sampler(self, timestep_sampler, importance_weights, timestep_seed, history_per_term, uniform_prob):
        """Validate and record the five keywords (``ValueError`` before any device work).  Without a sampler nothing
        else of this section ever runs: the step draws ``torch.randint`` and allocates nothing."""
        T = int(self.diffusion.num_timesteps)
        if importance_weights is not None and not isinstance(importance_weights, bool):
            raise ValueError("importance_weights must be None, True or False")
        if isinstance(timestep_seed, bool) or not isinstance(timestep_seed, int) or not 0 <= timestep_seed < 2 ** 64:
            raise ValueError("timestep_seed must be an integer in [0, 2**64)")
        if isinstance(history_per_term, bool) or not isinstance(history_per_term, int) or history_per_term < 1:
            raise ValueError("history_per_term must be an integer >= 1")
        if not 0.0 <= _number(uniform_prob, "uniform_prob") <= 1.0:
            raise ValueError("uniform_prob must lie in [0, 1]")
        self._ts_probs_cpu = None
        if timestep_sampler is None:
            self.timestep_sampler = None
        elif isinstance(timestep_sampler, str):
            if timestep_sampler != "loss_second_moment":
                raise ValueError(f"timestep_sampler must be None, 'loss_second_moment' or a ({T},) table of "
                                 f"probabilities, got {timestep_sampler!r}")
            if T > 4096:
                raise ValueError(f"timestep_sampler='loss_second_moment' covers T <= 4096 (tdx_timestep_history_update), "
                                 f"the diffusion has T = {T}")
            self.timestep_sampler = "loss_second_moment"
        else:
            self._ts_probs_cpu = timestep_probs(T, timestep_sampler)
            self.timestep_sampler = "table"
        adaptive = self.timestep_sampler == "loss_second_moment"
        self.importance_weights = (adaptive if importance_weights is None else importance_weights) \
            and self.timestep_sampler is not None
        self.timestep_seed, self.history_per_term, self.uniform_prob = timestep_seed, history_per_term, float(uniform_prob)
        self.sample_losses = None   # (B,) device tensor: every sample's objective-weighted loss of the last step
        self.last_t = None          # (B,) the timesteps of the last step under a sampler
        self._ts_cdf = self._w_eff = self._ts_probs = self._ts_history = self._ts_counts = self._ts_rng = None
        self._sl = {}               # batch size -> its sample_losses buffer (a captured step holds its address)

    def _init_timestep_sampler(self):
        """The sampler's device buffers and first table; after ``_upload_weights``."""
        if self.timestep_sampler is None:
            return
        T, dev = int(self.diffusion.num_timesteps), self.device
        self._ts_cdf = torch.empty(T, dtype=torch.float32, device=dev)
        self._w_eff = torch.empty(T, dtype=torch.float32, device=dev)
        if self.timestep_sampler == "table":
            self._ts_probs = self._ts_probs_cpu.to(dev)
        else:
            self._ts_history = torch.zeros(T, self.history_per_term, dtype=torch.float32, device=dev)
            self._ts_counts = torch.zeros(T, dtype=torch.int32, device=dev)
        self._rebuild_timestep_table()

    def _rebuild_timestep_table(self):
        """``_ts_cdf`` and ``_w_eff`` from the probabilities (the fixed table, or the loss history as it stands) and
        the objective's weights, through the device entries."""
        if self.timestep_sampler is None:
            return
        st = torch.cuda.current_stream(self.device).cuda_stream
        T = int(self.diffusion.num_timesteps)
        w_obj = None if self._w_table is None else self._w_table.data_ptr()
        if self.timestep_sampler == "table":
            check(lib.tdx_timestep_cdf(self._ts_probs.data_ptr(), w_obj, 1 if self.importance_weights else 0,
                                       self._ts_cdf.data_ptr(), self._w_eff.data_ptr(), T, st), "tdx_timestep_cdf")
        else:
            self._history_update(None, None, 0, st)

    def _history_update(self, t, loss_b, B, st):
        check(lib.tdx_timestep_history_update(None if t is None else t.data_ptr(),
                                              None if loss_b is None else loss_b.data_ptr(), B,
                                              self._ts_history.data_ptr(), self._ts_counts.data_ptr(),
                                              self.history_per_term, self.uniform_prob,
                                              None if self._w_table is None else self._w_table.data_ptr(),
                                              self._ts_cdf.data_ptr(), self._w_eff.data_ptr(),
                                              int(self.diffusion.num_timesteps), st), "tdx_timestep_history_update")

    def _loss_table(self):
        """The (T,) device weights the loss entry of this step reads; None: the unweighted entry.  Without a sampler
        the objective's table as it always was; with one the step's own ``_w_eff`` whenever it can differ from ones."""
        if self.timestep_sampler is None:
            return self._w_table
        if not self.importance_weights and (self._w_table is None or self.timestep_sampler == "loss_second_moment"):
            return self._w_table    # (the history entry always writes the importance weights of its table into _w_eff)
        return self._w_eff

    def _draw_t(self, B, offset, st=None, rng_dev=None, out=None):
        """``t`` (B,) int64 from the sampler's CDF, keyed by ``(timestep_seed, offset, b)`` - or by the two device
        words ``rng_dev`` that a captured step refreshes before each replay."""
        t = torch.empty(B, dtype=torch.int64, device=self.device) if out is None else out
        if st is None:
            st = torch.cuda.current_stream(self.device).cuda_stream
        check(lib.tdx_timestep_draw(self._ts_cdf.data_ptr(), int(self.diffusion.num_timesteps), t.data_ptr(), None, B,
                                    self.timestep_seed, offset, None if rng_dev is None else rng_dev.data_ptr(), st),
              "tdx_timestep_draw")
        return t

    def _sample_losses_buf(self, B):
        buf = self._sl.get(B)
        if buf is None:
            buf = self._sl[B] = torch.zeros(B, dtype=torch.float32, device=self.device)
        return buf

    def _after_loss(self, pred, target, t, B, st=None):
        """After the loss launch of a step under a sampler: every sample's loss (``sample_losses``: the objective's
        weight times its mean squared error - not the importance weight, which would feed the sampler its own output)
        and, for the adaptive sampler, the history update that also writes the next step's ``_ts_cdf`` / ``_w_eff``."""
        if st is None:
            st = torch.cuda.current_stream(self.device).cuda_stream
        self.last_t = t
        self.sample_losses = out = self._sample_losses_buf(B)
        check(lib.tdx_mse_per_sample(pred.data_ptr(), target.data_ptr(), t.data_ptr(),
                                     None if self._w_table is None else self._w_table.data_ptr(), out.data_ptr(), B,
                                     pred.numel() // B, st), "tdx_mse_per_sample")
        if self.timestep_sampler == "loss_second_moment":
            self._history_update(t, out, B, st)

    def timestep_sampler_state(self):
        """``{"history": (T, H) fp32, oldest first, "counts": (T,) int32}`` of the adaptive sampler, on the CPU (a
        checkpoint entry; it synchronises)."""
        if self.timestep_sampler != "loss_second_moment":
            raise RuntimeError("timestep_sampler_state() needs timestep_sampler='loss_second_moment'")
        return {"history": self._ts_history.cpu(), "counts": self._ts_counts.cpu()}

    def load_timestep_sampler_state(self, state):
        """Inverse of ``timestep_sampler_state()``: shapes and the range of the counts are checked (``ValueError``),
        then the table the next step draws from is rebuilt on the device."""
        if self.timestep_sampler != "loss_second_moment":
            raise RuntimeError("load_timestep_sampler_state() needs timestep_sampler='loss_second_moment'")
        T, H = int(self.diffusion.num_timesteps), self.history_per_term
        try:
            hist, counts = state["history"], state["counts"]
        except (TypeError, KeyError, IndexError):
            raise ValueError("the sampler state is a dict with 'history' and 'counts'") from None
        hist, counts = torch.as_tensor(hist), torch.as_tensor(counts)
        if tuple(hist.shape) != (T, H) or not hist.dtype.is_floating_point:
            raise ValueError(f"history must be a floating-point ({T},{H}) tensor, got {tuple(hist.shape)}")
        if tuple(counts.shape) != (T,) or counts.dtype.is_floating_point or counts.dtype == torch.bool:
            raise ValueError(f"counts must be an integer ({T},) tensor, got {tuple(counts.shape)}")
        if not torch.isfinite(hist).all() or (counts < 0).any() or (counts > H).any():
            raise ValueError(f"history must be finite and counts in [0, {H}]")
        self._ts_history.copy_(hist.to(torch.float32))
        self._ts_counts.copy_(counts.to(torch.int32))
        self._rebuild_timestep_table()

    def _q_sample(self, x_0, t, noise, offset, y=None):
        """``(x_t, target)`` from the forward process's entries: the target is the noise, or v (written by the same
        launch); without ``noise`` and with ``philox_seed`` the noise is drawn in the kernel, keyed by ``offset``.
        ``y``: the step's condition, unused here - for a step whose target is itself a network's work
        (``train.DistillStep``)."""
        fp, dev = self.diffusion, x_0.device
        philox = noise is None and self.philox_seed is not None
        if self.prediction != "eps":
            if philox:
                return fp.q_sample_target_philox(x_0, t, self.philox_seed, offset, self.prediction)
            return fp.q_sample_target(dev, x_0, t, noise=noise, prediction=self.prediction)
        if philox:
            return fp.q_sample_philox(x_0, t, self.philox_seed, offset)
        return fp.q_sample(dev, x_0, t, noise=noise)

    # -------------------------------------------------------------------- EMA
    def _need_ema(self, what: str):
        if self.ema is None:
            raise RuntimeError(f"{what} needs {type(self).__name__}(ema_decay=...)")
        if self._ema_swapped:
            raise RuntimeError(f"{what} inside ema_weights(): the average and the parameters have traded places")

    def reset_ema(self):
        """The average starts again from the current parameters (after loading a checkpoint into the model of a
        step that already exists)."""
        self._need_ema("reset_ema()")
        self.ema.copy_(self.flat_param)

    def ema_state_dict(self):
        """The model's ``state_dict()`` with the averaged parameters: the same keys, clones of the slices of ``self.ema``
        for the parameters and clones of the live buffers (BatchNorm running statistics are averages already, and
        shared).  Loads into the reference's modules unchanged."""
        self._need_ema("ema_state_dict()")
        out = type(self.model.state_dict())()
        for k, v in self.model.state_dict().items():
            if k in self.offsets:
                lo, hi = self.offsets[k]
                out[k] = self.ema[lo:hi].view(v.shape).clone()
            else:
                out[k] = v.detach().clone()
        return out

    def load_ema_state_dict(self, sd):
        """Inverse of ``ema_state_dict()`` for the parameter entries (buffers belong to the model)."""
        self._need_ema("load_ema_state_dict()")
        for k, (lo, hi) in self.offsets.items():
            v = sd[k]
            if v.numel() != hi - lo:
                raise ValueError(f"{k}: {tuple(v.shape)} does not fit the parameter's {hi - lo} elements")
        for k, (lo, hi) in self.offsets.items():
            self.ema[lo:hi].copy_(sd[k].detach().reshape(-1))

    def _swap_ema(self):
        st = torch.cuda.current_stream(self.device).cuda_stream
        check(lib.tdx_swap_f32(self.flat_param.data_ptr(), self.ema.data_ptr(), self.flat_param.numel(), st),
              "tdx_swap_f32")
        # the launch went in: from here on the two buffers hold each other's contents
        self._ema_swapped = not self._ema_swapped
        self._params_swapped()

    def _params_swapped(self):
        """Hook: the parameters were just rewritten through raw pointers (no torch version bump)."""

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the module IS the averaged model: one ``tdx_swap_f32`` launch exchanges the contents of
        ``flat_param`` and ``ema`` on entry and again on exit (also when the body raises), so ``forward``, ``sample``,
        ``ddim_sample``, guidance and ``state_dict()`` see the averaged weights, and no pointer that a plan or a
        captured step holds changes.  ``step()`` and a nested ``ema_weights()`` raise inside."""
        self._need_ema("ema_weights()")
        self._swap_ema()     # flips _ema_swapped once its launch is in; nothing may come between it and the try
        try:
            yield self.model
        finally:
            self._swap_ema()

    # ------------------------------------------------------------------ graph
    def _drop_graph(self):
        self._graph = self._graph_key = self._gws = None

    def _graph_ready(self, key: tuple, *static_args) -> bool:
        """The capture protocol, per ``key`` (whatever a captured graph depends on: shapes, ``model.training``).  False:
        the first step with this key, which the caller runs eagerly (plans, workspaces, first-launch set-up; a graph of
        another key is dropped).  True: ``_graph`` holds this key's step - captured by this call when it is the second
        one - and the caller refreshes its static inputs and calls ``_replay()``.

        The capture runs ``_static_step(hyper)``, the subclass's eager body on the static inputs that
        ``_alloc_static(*static_args)`` made, with Adam's step-dependent scalars in the device tensor ``_hyper``."""
        if key == self._graph_key:
            return True
        if self._graph_key != ("warm",) + key:
            self._drop_graph()
            self._graph_key = ("warm",) + key
            return False
        self._hyper = torch.zeros(3 if self.ema is None else 4, dtype=torch.float32, device=self.device)
        if self.max_grad_norm is not None and self._clip_scratch is None:
            self._clip_scratch = self._new_clip_scratch()
        self._alloc_static(*static_args)
        self._graph = self._capture(lambda: self._static_step(self._hyper))
        self.step_count -= 1   # the capture ran the host bookkeeping once without executing anything
        self._graph_key = key
        return True

    @staticmethod
    def _capture(body):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            body()
        return g

    def _replay(self):
        self.step_count += 1
        ema_a = None if self.ema is None else self._ema_a()
        self._hyper.copy_(torch.tensor(adam_hyper(self.lr, self.betas, self.step_count, 1.0, ema_a), dtype=torch.float32))
        self._graph.replay()
        return self.loss

    # -------------------------------------------------------------- workspace
    def _workspace(self, B):
        ws = self._ws.get(B)
        if ws is None:
            n = self._workspace_floats(B)
            if len(self._ws) >= 4:   # small cache; the workspace a captured graph replays into is never evicted
                self._ws = {k: v for k, v in self._ws.items() if v is self._gws}
            ws = self._ws[B] = torch.empty(n, dtype=torch.float32, device=self.device)
        return ws
