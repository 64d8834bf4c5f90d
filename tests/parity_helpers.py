"""Shared parity helpers of the GPU tests (test infrastructure): the max-pool routing the GPU
forward chose, and the fp64-calibrated bound for parameter gradients."""
import os

import numpy as np
import torch

from oracle import ref_cpu as R


def rel_mse(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b) ** 2).mean().item() / max((b**2).mean().item(), 1e-30)


def is_pre_bn_bias(key):
    stage, idx, kind = (key.split(".") + ["", ""])[:3]
    return kind == "bias" and idx in ("0", "3") and stage[:3] in ("enc", "dec", "bot")


def _plan_of(m, B):
    return [p for key, p in m._plans.items() if key[1] == B][0]


def gpu_pool_idx_raw(m, B):
    """Arg-max index of every max-pool window exactly as the GPU forward decided it (no check)."""
    plan = _plan_of(m, B)
    out = {}
    for name, unit, H, Cc in (("e1", 1, 28, 128), ("e2", 3, 14, 256), ("e3", 5, 7, 512)):
        Y = plan.tensor(f"Y{unit}").view(B, H, H, Cc)
        ss = plan.tensor(f"ss{unit}")
        a = torch.relu(torch.addcmul(ss[Cc:2 * Cc], Y, ss[:Cc])).permute(0, 3, 1, 2).cpu()
        out[name] = R.pool_windows(a).argmax(dim=-1, keepdim=True)
    return out


def gpu_relu_masks_raw(m, B):
    """Active set of every ReLU exactly as the GPU forward decided it (no check)."""
    plan = _plan_of(m, B)
    masks = {}
    for u, (name, (H, Cc)) in enumerate(zip(UNIT_BN, UNIT_SHAPE)):
        Y = plan.tensor(f"Y{u}").view(B, H, H, Cc)
        ss = plan.tensor(f"ss{u}")
        masks[name] = (torch.addcmul(ss[Cc:2 * Cc], Y, ss[:Cc]).permute(0, 3, 1, 2) > 0).cpu()
    return masks


def check_choices(pool_idx, masks, cpu_args, training=True, pool_tol=1e-4, relu_tol=1e-5):
    """The sub-gradient choices of an implementation may differ from the exact (fp64) ones only at
    ties: a pooling window whose picked entry is within ``pool_tol`` of the maximum, a ReLU input
    within ``relu_tol`` of 0 (both relative to the tensor's RMS).  Returns the number of flips."""
    sd, x, t, noise, y = cpu_args
    p64, b64 = R.split_state(sd)
    p64 = {k: v.double() for k, v in p64.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in b64.items()}
    taps = {}
    with torch.no_grad():
        R.unet_forward(p64, b64, x.double(), t, y, training=training, taps=taps, pool_idx=pool_idx)
    flips = {}
    for name, idx in (pool_idx or {}).items():
        w64 = R.pool_windows(taps[name])
        differ = (idx != w64.argmax(dim=-1, keepdim=True)).squeeze(-1)
        if differ.any():
            rms = taps[name].pow(2).mean().sqrt().item()
            picked = torch.gather(w64, -1, idx)[differ].squeeze(-1)
            best = w64[differ].max(dim=-1).values
            gap = (best - picked) / torch.maximum(best.abs(), torch.tensor(rms, dtype=best.dtype))
            assert gap.max().item() < pool_tol, (name, int(differ.sum()), gap.max().item())
            flips[name] = int(differ.sum())
    for name, mask in (masks or {}).items():
        exact = taps["prebn_act:" + name]
        differ = mask != (exact > 0)
        if differ.any():
            rms = exact.pow(2).mean().sqrt().item()
            worst = (exact[differ].abs().max() / rms).item()
            assert worst < relu_tol, (name, int(differ.sum()), worst)
            flips[name] = int(differ.sum())
    return flips


def gpu_pool_routing(m, B, cpu_args, training=True):
    """Arg-max index of every max-pool window as the GPU forward decided it (from its own
    pre-BN tensors and scale/shift), checked against the exact routing: they may differ
    only where the two largest entries of a window agree to 1e-4 (an fp32 coin flip,
    either choice being a valid sub-gradient of max)."""
    plan = [p for (dev, b), p in m._plans.items() if b == B][0]
    taps = {}
    sd, x, t, noise, y = cpu_args
    p64, b64 = R.split_state(sd)
    p64 = {k: v.double() for k, v in p64.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in b64.items()}
    with torch.no_grad():
        R.unet_forward(p64, b64, x.double(), t, y, training=training, taps=taps)
    out = {}
    for name, unit, H, Cc in (("e1", 1, 28, 128), ("e2", 3, 14, 256), ("e3", 5, 7, 512)):
        Y = plan.tensor(f"Y{unit}").view(B, H, H, Cc)
        ss = plan.tensor(f"ss{unit}")
        a = torch.relu(torch.addcmul(ss[Cc:2 * Cc], Y, ss[:Cc])).permute(0, 3, 1, 2).cpu()
        win = R.pool_windows(a)
        idx = win.argmax(dim=-1, keepdim=True)
        w64 = R.pool_windows(taps[name])
        idx64 = w64.argmax(dim=-1, keepdim=True)
        differ = (idx != idx64).squeeze(-1)
        if differ.any():
            # a tie = the exact values of the entry the GPU picked and of the exact arg-max agree to 1e-4
            # of the larger of |value| and the tensor's RMS (relative to the value alone, a window whose
            # entries are all ~0 after the ReLU - exact maximum 1e-9 - would count as a gap of 100 %)
            rms = taps[name].pow(2).mean().sqrt().item()
            picked = torch.gather(w64, -1, idx)[differ].squeeze(-1)
            best = w64[differ].max(dim=-1).values
            gap = (best - picked) / torch.maximum(best.abs(), torch.tensor(rms, dtype=best.dtype))
            assert gap.max().item() < 1e-4, (name, int(differ.sum()), gap.max().item())
        out[name] = idx
    return out


UNIT_BN = ("enc1.1", "enc1.4", "enc2.1", "enc2.4", "enc3.1", "enc3.4", "bottleneck.1",
           "dec3.1", "dec3.4", "dec2.1", "dec2.4", "dec1.1", "dec1.4")
UNIT_SHAPE = ((28, 128), (28, 128), (14, 256), (14, 256), (7, 512), (7, 512), (4, 512),
              (8, 256), (8, 256), (16, 128), (16, 128), (32, 64), (32, 64))


def gpu_relu_masks(m, B, cpu_args, training=True, pool_idx=None, tol=1e-5):
    """Active set of every ReLU as the GPU forward decided it (sign of y*scale+shift from its own
    pre-BN tensors), keyed by BatchNorm module name for ``R.unet_forward(relu_masks=...)``.
    Checked against the exact (fp64) pre-activations: the sets may differ only where the exact
    normalised value is within ``tol`` of 0 relative to the layer's RMS - there the activation is 0
    to rounding either way and on/off are both valid sub-gradients."""
    plan = [p for (dev, b), p in m._plans.items() if b == B][0]
    sd, x, t, noise, y = cpu_args
    p64, b64 = R.split_state(sd)
    p64 = {k: v.double() for k, v in p64.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in b64.items()}
    taps = {}
    with torch.no_grad():
        R.unet_forward(p64, b64, x.double(), t, y, training=training, taps=taps, pool_idx=pool_idx)
    masks, flips = {}, {}
    for u, (name, (H, Cc)) in enumerate(zip(UNIT_BN, UNIT_SHAPE)):
        Y = plan.tensor(f"Y{u}").view(B, H, H, Cc)
        ss = plan.tensor(f"ss{u}")
        act = torch.addcmul(ss[Cc:2 * Cc], Y, ss[:Cc]).permute(0, 3, 1, 2).cpu()
        mask = act > 0
        exact = taps["prebn_act:" + name]
        differ = mask != (exact > 0)
        if differ.any():
            rms = exact.pow(2).mean().sqrt().item()
            worst = (exact[differ].abs().max() / rms).item()
            assert worst < tol, (name, int(differ.sum()), worst)
            flips[name] = int(differ.sum())
        masks[name] = mask
    return masks, flips


def check_relu_ties(masks, taps64, tol=1e-5):
    """``masks``: the GPU run's ReLU active sets (gpu_relu_masks_raw); ``taps64``: the taps of an fp64 oracle run that
    was GIVEN those sets.  The sets may differ from the exact ones only where the exact normalised pre-activation is
    within ``tol`` of 0 relative to the layer's RMS (there the activation is 0 to rounding either way, so the values
    downstream - and hence every later pre-activation of that run - are the exact ones to rounding).  Returns the
    flip counts.  Same rule as gpu_relu_masks, without its extra oracle forward."""
    flips = {}
    for name, mask in masks.items():
        exact = taps64["prebn_act:" + name].detach()
        differ = mask != (exact > 0)
        if differ.any():
            rms = exact.pow(2).mean().sqrt().item()
            worst = (exact[differ].abs().max() / rms).item()
            assert worst < tol, (name, int(differ.sum()), worst)
            flips[name] = int(differ.sum())
    return flips


def grad_precision_failures(got, g32, g64, training, k_factor=10.0, floor=1e-4, floors=None, log=False):
    """Per-parameter: ||g_gpu - g64|| / ||g64|| must be within k_factor x the fp32 CPU
    oracle's own distance from the fp64 ground truth (floor 1e-4: an fp32 MFMA dot product
    is one sequential fma chain, error ~sqrt(K) eps of sum|a*b|, and weight gradients
    cancel heavily - observed worst case 6e-5 on enc1.0.weight in eval mode).  A train-mode
    BatchNorm over a nearly constant channel multiplies rounding noise by up to
    1/sqrt(eps) ~ 300; that noise is a property of fp32 evaluation of this network
    (the reference has it too), so the bound is calibrated per case, not fixed.  ``floors``: per-parameter
    floors that replace ``floor`` for the keys they name; ``log``: print every parameter's distance from fp64
    next to the fp32 CPU oracle's."""
    errs_cpu = {}
    for k in g64:
        n64 = g64[k].norm().item()
        errs_cpu[k] = (g32[k].double() - g64[k]).norm().item() / max(n64, 1e-30)
    usable = [e for k, e in errs_cpu.items() if not (training and is_pre_bn_bias(k))]
    med = float(np.median(usable))
    bad = []
    for k, g in got.items():
        if training and is_pre_bn_bias(k):
            continue  # exactly-zero true gradient: both sides are pure rounding noise
        n64 = g64[k].norm().item()
        err = (g.detach().double().cpu() - g64[k]).norm().item() / max(n64, 1e-30)
        tol = max(k_factor * errs_cpu[k], k_factor * med, (floors or {}).get(k, floor))
        if log:
            print(f"  {k:40s} gpu {err:.2e}  cpu32 {errs_cpu[k]:.2e}  tol {tol:.2e}")
        if not err <= tol:
            bad.append((k, f"gpu {err:.2e}", f"cpu32 {errs_cpu[k]:.2e}", f"tol {tol:.2e}"))
    return bad




# ---------------------------------------------------------------------------------------------------------------
# The bf16 mode's tolerance, anchored on the reference.  The reference has no reduced precision of its own
# (SURVEY.md 0), so the yardstick is what torch's stock bf16 autocast does to the REFERENCE's modules on the same
# inputs and weights (tools/make_golden.py::autocast_fixtures -> tests/golden/bf16_autocast.npz: eps_hat MSE in
# train / eval mode, loss, per-parameter gradient cosine, each against the reference's own fp32 run).  The gate,
# with its one constant stated here: this build's bf16 mode must be NO FURTHER from fp32 than BF16_K x that.
BF16_K = 1.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class AutocastYardstick:
    """Distances of the reference-under-autocast from the reference in fp32 for one fixture tag
    (mnist_B64, laion_B8, laion_B2_hw64, latent_B32); parameters whose exact gradient is 0 are left out of the
    cosines on both sides (``skip``: the biases in front of a train-mode BatchNorm)."""

    def __init__(self, tag, skip=is_pre_bn_bias):
        d = np.load(os.path.join(GOLDEN, "bf16_autocast.npz"))
        self.tag = tag
        self.eps_mse_train = float(d[f"{tag}__eps_mse_train"])
        self.eps_mse_eval = float(d[f"{tag}__eps_mse_eval"])
        self.loss_shift = abs(float(d[f"{tag}__loss_autocast"]) - float(d[f"{tag}__loss_fp32"])) / float(d[f"{tag}__loss_fp32"])
        pre = f"{tag}__gcos__"
        self.cos = {k[len(pre):].replace("__", "."): float(d[k]) for k in d.files if k.startswith(pre)}
        vals = sorted(v for k, v in self.cos.items() if not skip(k) and v == v)
        self.cos_worst, self.cos_median = vals[0], vals[len(vals) // 2]

    def check(self, what, eps_mse=None, cos_sorted=None, loss=None, loss_ref=None, eval_mode=False):
        """``cos_sorted``: ascending [(cosine, name)] of this build's gradients against the fp32 oracle."""
        k = BF16_K
        if eps_mse is not None:
            lim = k * (self.eps_mse_eval if eval_mode else self.eps_mse_train)
            print(f"{what}: eps_hat MSE {eps_mse:.3e}  <= {k} x reference-under-autocast {lim / k:.3e} ({self.tag})")
            assert eps_mse <= lim, (what, eps_mse, lim)
        if cos_sorted is not None:
            worst, med = cos_sorted[0][0], cos_sorted[len(cos_sorted) // 2][0]
            print(f"{what}: gradient cosine vs fp32 worst {worst:.4f} ({cos_sorted[0][1]}) median {med:.5f}; "
                  f"reference-under-autocast {self.cos_worst:.4f} / {self.cos_median:.5f}")
            assert 1.0 - worst <= k * (1.0 - self.cos_worst), (what, cos_sorted[:3], self.cos_worst)
            assert 1.0 - med <= k * (1.0 - self.cos_median), (what, med, self.cos_median)
        if loss is not None:
            # a signed sum of many small errors, not a distance: twice the reference's own shift, floor 0.5 %
            lim = max(2.0 * k * self.loss_shift, 5e-3)
            assert abs(loss - loss_ref) <= lim * abs(loss_ref), (what, loss, loss_ref, lim)
