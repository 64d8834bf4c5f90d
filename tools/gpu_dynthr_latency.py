#!/usr/bin/env python3
"""Per-step time of dynamically thresholded sampling (``dynamic_threshold=q``) against the static-clipped step
(``clip_denoised=True``), in graph + Philox mode (graph replay, in-kernel noise, device step counter, sampling tables):
the conditional MNIST UNet under guidance at n = 16 and 64, and the LAION UNet at 32 x 32, n = 16.  The thresholded
step cannot keep the update in final_conv's epilogue - a sample's bound needs the whole output - so against the clipped
step it pays the plain final_conv plus two launches: the selection kernel (four passes over the sample's x and output,
one workgroup per sample) and the update kernel.

A ddim_sample call carries fixed work (tables, graph capture), so the per-step time is the slope between two chain
lengths: (time at S_LONG - time at S_SHORT) / (S_LONG - S_SHORT); both lengths are multiples of GRAPH_STEPS, so either
call captures one ten-step graph and no tail graph.  One process; every round times clipped and thresholded chains back
to back at both lengths (interleaved, so clock drift hits both alike) and yields one slope each; the figures are the
median over the rounds and their min .. max.

    python3 tools/gpu_dynthr_latency.py [--rounds 7] [--q 0.995] [--out profiles/dynthr_latency.txt]"""
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
    ap.add_argument("--q", type=float, default=0.995)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import conditional_diffusion_laion as LA

    torch.manual_seed(0)
    fp = C.ForwardProcess()
    mnist = C.NoiseModel().cuda().eval()
    laion = LA.NoiseModel(time_dim=768).cuda().eval()
    g = torch.Generator().manual_seed(1)

    def mnist_call(n):
        y = torch.randint(0, 10, (n,), generator=g).cuda()
        return lambda S, kw: C.ddim_sample(mnist, fp, "cuda", n_samples=n, y=y, steps=S, guidance_scale=3.0,
                                           use_graph=True, philox_seed=7, **kw)

    def laion_call(n):
        te = torch.randn(n, 768, generator=g).cuda()
        x_T = torch.randn(n, 4, 32, 32, generator=g)
        return lambda S, kw: LA.ddim_sample(laion, fp, "cuda", text_embeds=te, steps=S, x_T=x_T, use_graph=True,
                                            philox_seed=7, **kw)

    variants = [("clipped", dict(clip_denoised=True)), ("thresholded", dict(dynamic_threshold=a.q))]
    lines = []
    for what, call in (("MNIST cond guided w=3 n=16", mnist_call(16)), ("MNIST cond guided w=3 n=64", mnist_call(64)),
                       ("LAION 4x32x32 n=16", laion_call(16))):
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
            line = (f"{what:<28} {name:<12} {med[name]:.4f} ms/step   "
                    f"(min {min(v):.4f} .. max {max(v):.4f} over {a.rounds} rounds)")
            print(line, flush=True)
            lines.append(line)
        line = (f"{what:<28} thresholded - clipped = {1e3 * (med['thresholded'] - med['clipped']):.1f} us/step, "
                f"thresholded / clipped = {med['thresholded'] / med['clipped']:.4f}")
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}; graph + Philox mode; dynamic_threshold = {a.q}; per-step = slope of "
                    f"the chain time between S = {S_SHORT} and S = {S_LONG}, one slope per round (clipped and thresholded "
                    f"interleaved), median and min .. max over the rounds\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
