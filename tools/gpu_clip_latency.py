#!/usr/bin/env python3
"""Per-step time of clipped-x0 sampling (``clip_denoised=True``) against the unclipped step, in graph + Philox mode
(graph replay, in-kernel noise, device step counter, sampling tables) on the unconditional MNIST UNet, n = 16 and 64.
The clipped step runs the launches of the unclipped one - the update sits in final_conv's epilogue either way - with a
handful of extra VALU operations per element in the last launch, so the expectation is no difference beyond the
run-to-run spread.

A ddim_sample call carries fixed work (tables, graph capture), so the per-step time is the slope between two chain
lengths: (time at S_LONG - time at S_SHORT) / (S_LONG - S_SHORT); both lengths are multiples of GRAPH_STEPS, so either
call captures one ten-step graph and no tail graph.  One process; every round times unclipped and clipped chains
back to back at both lengths (interleaved, so clock drift hits both alike) and yields one slope each; the figures are
the median over the rounds and their min .. max.

The unclipped figure of another checkout (the parent commit) in the same session: run the tool a second time with
``--package-root <that checkout>`` (its own built library is loaded) and ``--unclipped-only --append``.

    python3 tools/gpu_clip_latency.py [--rounds 7] [--out profiles/clip_latency.txt]
    python3 tools/gpu_clip_latency.py --package-root ../parent --label parent --unclipped-only --append --out ..."""
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
    ap.add_argument("--unclipped-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch

    from tiny_diffusion_amd import diffusion as D

    torch.manual_seed(0)
    fp = D.ForwardProcess()
    m = D.NoiseModel().cuda().eval()
    variants = [("unclipped", {})] + ([] if a.unclipped_only else [("clipped", dict(clip_denoised=True))])
    lines = []
    for n in (16, 64):
        def call(S, kw):
            return D.ddim_sample(m, fp, "cuda", n_samples=n, steps=S, use_graph=True, philox_seed=7, **kw)

        for S in (S_SHORT, S_LONG):      # plan, INFER pack, first-launch set-up
            for _, kw in variants:
                call(S, kw)
        slopes = {name: [] for name, _ in variants}
        for _ in range(a.rounds):
            t = {(name, S): timed(torch, lambda: call(S, kw)) for S in (S_SHORT, S_LONG) for name, kw in variants}
            for name, _ in variants:
                slopes[name].append((t[(name, S_LONG)] - t[(name, S_SHORT)]) / (S_LONG - S_SHORT))
        med = {}
        for name, _ in variants:
            v = slopes[name]
            med[name] = statistics.median(v)
            line = (f"[{a.label}] MNIST uncond n={n:<3} {name:<10} {med[name]:.4f} ms/step   "
                    f"(min {min(v):.4f} .. max {max(v):.4f} over {a.rounds} rounds)")
            print(line, flush=True)
            lines.append(line)
        if "clipped" in med:
            line = f"[{a.label}] MNIST uncond n={n:<3} clipped / unclipped = {med['clipped'] / med['unclipped']:.4f}"
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            if not a.append:
                f.write(f"# {torch.cuda.get_device_name(0)}; graph + Philox mode; per-step = slope of the chain time between "
                        f"S = {S_SHORT} and S = {S_LONG}, one slope per round (unclipped and clipped interleaved), median and "
                        f"min .. max over the rounds\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
