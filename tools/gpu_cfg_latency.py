#!/usr/bin/env python3
"""Per-step time of classifier-free guidance (graph replay, in-kernel Philox noise, device step counter) on the
class-conditional MNIST UNet: the guided step of n samples (network batch 2n), the unguided step of n and the
unguided step of 2n samples, for n = 16 and 64.  The guided step at n runs the launches of the plain step at 2n with a
last kernel that does the same arithmetic and writes half the state, so it should cost no more than that one.

A ddim_sample call carries fixed work (tables, graph capture), so the per-step time is the slope between two chain
lengths: (median time at S_LONG - median time at S_SHORT) / (S_LONG - S_SHORT).  The fixed work cancels because it
does not depend on S here: both lengths are multiples of GRAPH_STEPS, so either call builds its tables and captures one
ten-step graph and no tail graph.  The unguided rows are timed in this tree: ``guidance_scale=None`` takes the code path
and the kernels the tree had before guidance existed, so "unguided 2n" is that earlier step at batch 2n.

    python3 tools/gpu_cfg_latency.py [--reps 5] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tiny_diffusion_amd import conditional_diffusion as C  # noqa: E402

S_SHORT, S_LONG = 50, 250


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return (time.perf_counter() - t0) * 1e3


def per_step(m, fp, n, w, reps):
    y = torch.arange(n, device="cuda") % 10
    med = {}
    for S in (S_SHORT, S_LONG):
        call = lambda: C.ddim_sample(m, fp, "cuda", n_samples=n, y=y, steps=S, use_graph=True, philox_seed=7,  # noqa: E731
                                     guidance_scale=w)
        call()   # plan, INFER pack, first-launch set-up
        med[S] = statistics.median(timed(call) for _ in range(reps))
    return (med[S_LONG] - med[S_SHORT]) / (S_LONG - S_SHORT), med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    fp = C.ForwardProcess()
    m = C.NoiseModel().cuda().eval()
    lines = []
    for n in (16, 64):
        res = {}
        for name, rows, w in (("guided n", n, 3.0), ("unguided n", n, None), ("unguided 2n", 2 * n, None)):
            res[name], med = per_step(m, fp, rows, w, a.reps)
            line = (f"MNIST cond n={n:<3} {name:<12} (network batch {2 * rows if w is not None else rows:>3})  "
                    f"{res[name]:.4f} ms/step   chains S={S_SHORT}: {med[S_SHORT]:.2f} ms  S={S_LONG}: {med[S_LONG]:.2f} ms")
            print(line, flush=True)
            lines.append(line)
        line = (f"MNIST cond n={n:<3} guided / unguided n = {res['guided n'] / res['unguided n']:.3f}   "
                f"guided / unguided 2n = {res['guided n'] / res['unguided 2n']:.3f}")
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}; per-step = slope of the median chain time ({a.reps} calls) "
                    f"between S = {S_SHORT} and S = {S_LONG}\n")
            f.write("# the unguided rows run guidance_scale=None, the unchanged pre-guidance code path and kernels, in the "
                    "same build\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
