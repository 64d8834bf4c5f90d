#!/usr/bin/env python3
"""Per-step time of masked sampling (inpainting: ``known`` / ``mask``) against the unmasked clipped step, in graph +
Philox mode (graph replay, in-kernel noise, device step counter, sampling tables) on the unconditional MNIST UNet,
n = 16 and 64.  Both chains run ``clip_denoised=True``: the masked step is the clipped step's launches - the update sits
in final_conv's epilogue either way - with two more fp32 loads and one blend per element in the last launch, so the
expectation is no difference beyond the run-to-run spread.

The protocol is tools/gpu_clip_latency.py's.  A ddim_sample call carries fixed work (tables, graph capture, here also
the expansion of known / mask), so the per-step time is the slope between two chain lengths: (time at S_LONG - time at
S_SHORT) / (S_LONG - S_SHORT); both lengths are multiples of GRAPH_STEPS, so either call captures one ten-step graph
and no tail graph.  One process; every round times unmasked and masked chains back to back at both lengths
(interleaved, so clock drift hits both alike) and yields one slope each; the figures are the median over the rounds and
their min .. max.

``--guided W``: the conditional MNIST UNet under guidance scale W instead.  There the masked chain does differ in its
launches: under a condition it runs the step counter, the time MLP and the projections as launches of their own where the
unmasked chain looks them up in the sampling tables (schedule.sample_loop: the three modes of a masked chain return the
same bits), so the ratio is the price of that.

The unmasked figure of another checkout (the parent commit) in the same session: run the tool a second time with
``--package-root <that checkout>`` (its own built library is loaded) and ``--unmasked-only --append``.

    python3 tools/gpu_inpaint_latency.py [--rounds 7] [--out profiles/inpaint_latency.txt]
    python3 tools/gpu_inpaint_latency.py --package-root ../parent --label parent --unmasked-only --append --out ..."""
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
    ap.add_argument("--unmasked-only", action="store_true")
    ap.add_argument("--guided", type=float, default=None, metavar="W",
                    help="the conditional MNIST UNet under guidance scale W instead of the unconditional one: a masked "
                         "chain under a condition runs the time path as launches, not as a table look-up")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch

    if a.guided is None:
        from tiny_diffusion_amd import diffusion as D
    else:
        from tiny_diffusion_amd import conditional_diffusion as D
    what = "MNIST uncond" if a.guided is None else f"MNIST cond w={a.guided:g}"

    torch.manual_seed(0)
    fp = D.ForwardProcess()
    m = D.NoiseModel().cuda().eval()
    lines = []
    for n in (16, 64):
        # the left half of every image is known; the tensors already live on the device, as a caller's would
        known = (2 * torch.rand(n, 1, 28, 28) - 1).cuda()
        mask = torch.zeros(1, 1, 28, 28)
        mask[..., :14] = 1.0
        mask = mask.cuda()
        variants = [("unmasked", dict(clip_denoised=True))]
        if not a.unmasked_only:
            variants.append(("masked", dict(clip_denoised=True, known=known, mask=mask)))

        cond = {} if a.guided is None else dict(y=(torch.arange(n) % 10).cuda(), guidance_scale=a.guided)

        def call(S, kw):
            return D.ddim_sample(m, fp, "cuda", n_samples=n, steps=S, use_graph=True, philox_seed=7, **cond, **kw)

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
            line = (f"[{a.label}] {what} n={n:<3} {name:<10} {med[name]:.4f} ms/step   "
                    f"(min {min(v):.4f} .. max {max(v):.4f} over {a.rounds} rounds)")
            print(line, flush=True)
            lines.append(line)
        if "masked" in med:
            line = f"[{a.label}] {what} n={n:<3} masked / unmasked = {med['masked'] / med['unmasked']:.4f}"
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            if not a.append:
                f.write(f"# {torch.cuda.get_device_name(0)}; graph + Philox mode, clip_denoised=True; per-step = slope of the "
                        f"chain time between S = {S_SHORT} and S = {S_LONG}, one slope per round (unmasked and masked "
                        f"interleaved), median and min .. max over the rounds\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
