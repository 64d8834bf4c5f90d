#!/usr/bin/env python3
"""Per-step time of the DPM-Solver++(2M) sampler (``dpm_sample``) against the clipped DDIM step
(``ddim_sample(clip_denoised=True)``), in graph + Philox mode (graph replay, device step counter, sampling tables) on
the unconditional MNIST UNet, n = 16 and 64, and the wall time of the calls a user would compare:
``dpm_sample(steps=20)``, ``ddim_sample(steps=50)`` and ``sample()`` at T = 1000.

The multistep step runs the launches of the clipped DDIM step - the update sits in final_conv's epilogue either way -
and moves 8 B/element more in the last launch (the history, read and written) while drawing no noise, so the expectation
is no difference beyond the run-to-run spread.

A call carries fixed work (tables, graph capture), so the per-step time is the slope between two chain lengths:
(time at S_LONG - time at S_SHORT) / (S_LONG - S_SHORT); both are multiples of GRAPH_STEPS (one ten-step graph, no tail
graph).  The slope runs use ``spacing="uniform"``: log-SNR spacing merges duplicate timesteps, so a request for 250
steps would run fewer, and the cost of a step does not depend on where it sits.  One process; every round times both
samplers back to back at both lengths (interleaved, so clock drift hits both alike) and yields one slope each; the
figures are the median over the rounds and their min .. max.

The clipped DDIM figure of another checkout (the parent commit) in the same session: run the tool a second time with
``--package-root <that checkout>`` (its own built library is loaded) and ``--ddim-only --append``.

    python3 tools/gpu_dpm_latency.py [--rounds 7] [--out profiles/dpm_latency.txt]
    python3 tools/gpu_dpm_latency.py --package-root ../parent --label "parent commit" --ddim-only --append --out ..."""
import argparse
import os
import statistics
import sys
import time

S_SHORT, S_LONG = 50, 250


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--ddim-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch

    from tiny_diffusion_amd import diffusion as D

    torch.manual_seed(0)
    fp = D.ForwardProcess()
    m = D.NoiseModel().cuda().eval()
    mode = dict(use_graph=True, philox_seed=7)

    def ddim(n, S):
        return D.ddim_sample(m, fp, "cuda", n_samples=n, steps=S, clip_denoised=True, **mode)

    def dpm(n, S):
        return D.dpm_sample(m, fp, "cuda", n_samples=n, steps=S, spacing="uniform", clip_denoised=True, **mode)

    variants = [("ddim clipped", ddim)] + ([] if a.ddim_only else [("dpm 2M", dpm)])
    lines = []
    for n in (16, 64):
        for S in (S_SHORT, S_LONG):      # plan, INFER pack, first-launch set-up
            for _, f in variants:
                f(n, S)
        slopes = {name: [] for name, _ in variants}
        for _ in range(a.rounds):
            t = {(name, S): timed(torch, lambda: f(n, S)) for S in (S_SHORT, S_LONG) for name, f in variants}
            for name, _ in variants:
                slopes[name].append((t[(name, S_LONG)] - t[(name, S_SHORT)]) / (S_LONG - S_SHORT))
        med = {}
        for name, _ in variants:
            v = slopes[name]
            med[name] = statistics.median(v)
            line = (f"[{a.label}] MNIST uncond n={n:<3} {name:<13} {med[name]:.4f} ms/step   "
                    f"(min {min(v):.4f} .. max {max(v):.4f} over {a.rounds} rounds)")
            print(line, flush=True)
            lines.append(line)
        if "dpm 2M" in med:
            line = f"[{a.label}] MNIST uncond n={n:<3} dpm 2M / ddim clipped = {med['dpm 2M'] / med['ddim clipped']:.4f}"
            print(line, flush=True)
            lines.append(line)
        if not a.ddim_only:      # the calls a user compares, whole (set-up and graph capture included)
            from tiny_diffusion_amd.schedule import logsnr_timesteps

            walls = [(f"dpm_sample(steps=20) [{len(logsnr_timesteps(fp, 20))} log-SNR steps]",
                      lambda: D.dpm_sample(m, fp, "cuda", n_samples=n, steps=20, clip_denoised=True, **mode)),
                     ("ddim_sample(steps=50)",
                      lambda: D.ddim_sample(m, fp, "cuda", n_samples=n, steps=50, clip_denoised=True, **mode)),
                     ("sample() T=1000",
                      lambda: D.sample(m, fp, "cuda", n_samples=n, clip_denoised=True, **mode))]
            for name, f in walls:
                f()
                v = [timed(torch, f) for _ in range(3)]
                line = (f"[{a.label}] MNIST uncond n={n:<3} wall {name:<42} {statistics.median(v):8.2f} ms   "
                        f"(min {min(v):.2f} .. max {max(v):.2f} over 3 calls)")
                print(line, flush=True)
                lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            if not a.append:
                f.write(f"# {torch.cuda.get_device_name(0)}; graph + Philox mode, clip_denoised=True; per-step = slope of the "
                        f"chain time between S = {S_SHORT} and S = {S_LONG} (uniform spacing), one slope per round (the samplers "
                        f"interleaved), median and min .. max over the rounds; wall = one whole call\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
