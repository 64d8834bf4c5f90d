#!/usr/bin/env python3
"""Wall time of ddim_sample (DDIM, graph replay, in-kernel Philox noise, device step counter): first call (plan,
INFER pack, tables, graph capture) and the median of later calls, for the MNIST UNet at n = 16 / 64 with
S = 10 / 50 / 100 and the LAION UNet at 32x32, n = 16, S = 50; the sample() reference (T = 1000) per n.

    python3 tools/gpu_ddim_latency.py [--reps 5] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/gpu_ddim_latency.py --trace-one-step

--trace-one-step runs only two MNIST n = 16 chains of S = 10 (one capture, one replay pass) for a trace of the
scheduled reverse step (kernels per step = the trace's count over 10 steps of the second chain)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tiny_diffusion_amd import conditional_diffusion_laion as L  # noqa: E402
from tiny_diffusion_amd import diffusion as D  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def measure(fn, reps):
    first, out = timed(fn)
    later = [timed(fn)[0] for _ in range(reps)]
    assert torch.isfinite(out).all()
    return first, statistics.median(later), min(later), max(later)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-one-step", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    fp = D.ForwardProcess()
    m = D.NoiseModel().cuda().eval()
    if a.trace_one_step:
        for _ in range(2):
            D.ddim_sample(m, fp, "cuda", n_samples=16, steps=10, use_graph=True, philox_seed=7)
        torch.cuda.synchronize()
        return
    lines = []

    def row(name, S, r):
        first, med, lo, hi = r
        line = (f"{name:<28} S={S:>4}  first {first:8.2f} ms   later median {med:8.2f} ms [{lo:.2f}, {hi:.2f}]"
                f"   {med / S:.4f} ms/step")
        print(line, flush=True)
        lines.append(line)

    for n in (16, 64):
        for S in (10, 50, 100):
            row(f"MNIST ddim_sample n={n}", S, measure(
                lambda: D.ddim_sample(m, fp, "cuda", n_samples=n, steps=S, use_graph=True, philox_seed=7), a.reps))
        row(f"MNIST sample n={n}", 1000, measure(
            lambda: D.sample(m, fp, "cuda", n_samples=n, use_graph=True, philox_seed=7), max(2, a.reps // 2)))
    ml = L.NoiseModel().cuda().eval()
    cond = torch.randn(16, 768, device="cuda")
    row("LAION32 ddim_sample n=16", 50, measure(
        lambda: L.ddim_sample(ml, fp, "cuda", text_embeds=cond, steps=50, use_graph=True, philox_seed=7), a.reps))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}; first call = plan + pack + tables + capture + replay; "
                    f"later = median of {a.reps} calls\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
