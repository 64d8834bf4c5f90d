#!/usr/bin/env python3
"""What the EMA of the parameters costs on the GPU (TrainStep(ema_decay=...), csrc/elementwise.hip).

1. Isolated kernels at n = the MNIST UNet's parameter count as TrainStep reports it: ``tdx_adam_step`` (28 B/element),
   ``tdx_adam_ema_step`` (36 B/element) and ``tdx_swap_f32`` (16 B/element), as time and as achieved bytes/s.  Every
   kernel cycles through enough independent buffer sets to touch >= 1.5 GB between two uses of the same bytes (the
   rule of bench.py's ``adam`` row), so the rates are HBM rates, not Infinity Cache ones.  The yardstick is the
   ``adam`` row of THIS run and its spread over the repeats (rounds interleaved).
2. The whole training step, B = 256 on the MNIST UNet, eager, with ``ema_decay=None`` and with 0.9999: one TrainStep in
   one process, blocks of steps interleaved, the average switched off for every other block.

``--step-only`` times a real ``TrainStep(ema_decay=None)`` alone in its process.  Optional: ``--tree DIR`` imports the
package from ANOTHER checkout of the project (the parent commit, built in DIR) for a same-session figure beside this
tree's; ``--side-by-side`` times two plain TrainSteps on two models in one process, which is why part 2 does not
compare two models; ``--append`` adds to ``--out``.

    python3 tools/gpu_ema_cost.py [--rounds 7] [--out profiles/ema_cost.txt]
    python3 tools/gpu_ema_cost.py --step-only --append --out profiles/ema_cost.txt
    python3 tools/gpu_ema_cost.py --step-only --tree ../parent --label "parent commit" --append --out profiles/ema_cost.txt
    python3 tools/gpu_ema_cost.py --side-by-side --append --out profiles/ema_cost.txt"""
import argparse
import os
import statistics
import sys

HBM_WORKING_SET = 1.5e9   # bytes cycled through per kernel: 6x the 256 MiB Infinity Cache (bench.py)
BATCH = 256


def time_rot_ms(torch, fns, reps, warm=1):
    """Average duration of one call when the calls cycle through ``fns`` (the same kernel on different buffer sets)."""
    k = len(fns)
    for i in range(warm * k):
        fns[i % k]()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps * k):
        fns[i % k]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (reps * k)


def spread(xs):
    return f"median {statistics.median(xs):.4f}  min {min(xs):.4f}  max {max(xs):.4f}"


def isolated(torch, lib, check, n, rounds, say):
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    k = max(2, int(-(-HBM_WORKING_SET // (36.0 * n))))
    sets = []
    for _ in range(k):
        p, g, m, v = (torch.randn(n, device=dev) * 0.01 for _ in range(4))
        v.abs_()
        sets.append((p, g, m, v, p.clone()))
    ptr = lambda q: tuple(t.data_ptr() for t in q)  # noqa: E731
    rows = {
        "adam": (28.0, [(lambda q=q: check(lib.tdx_adam_step(*ptr(q[:4]), n, 1e-3, 0.9, 0.999, 1e-8, 3, 1.0, st)))
                        for q in sets]),
        "adam_ema": (36.0, [(lambda q=q: check(lib.tdx_adam_ema_step(*ptr(q), n, 1e-3, 0.9, 0.999, 1e-8, 3, 1.0, 1e-4, st)))
                            for q in sets]),
        "swap": (16.0, [(lambda q=q: check(lib.tdx_swap_f32(q[0].data_ptr(), q[4].data_ptr(), n, st))) for q in sets]),
    }
    ms = {name: [] for name in rows}
    for _ in range(rounds):
        for name, (_, fns) in rows.items():
            ms[name].append(time_rot_ms(torch, fns, 3))
    say(f"isolated kernels, n = {n} fp32 elements, {k} rotating buffer sets ({k * 36.0 * n / 1e9:.2f} GB touched between "
        f"two uses of the same bytes), {rounds} interleaved rounds of {3 * k} launches")
    for name, (bpe, _) in rows.items():
        med = statistics.median(ms[name])
        say(f"  {name:<16} {bpe:.0f} B/element  ms: {spread(ms[name])}   "
            f"TB/s: median {bpe * n / med / 1e9:.3f}  min {bpe * n / max(ms[name]) / 1e9:.3f}  "
            f"max {bpe * n / min(ms[name]) / 1e9:.3f}")
    rate = lambda name: rows[name][0] * n / statistics.median(ms[name]) / 1e9  # noqa: E731
    adam_spread = 28.0 * n / min(ms["adam"]) / 1e9 - 28.0 * n / max(ms["adam"]) / 1e9
    say(f"  yardstick: adam {rate('adam'):.3f} TB/s, spread over its repeats {adam_spread:.3f} TB/s; "
        f"adam_ema {rate('adam_ema'):.3f} TB/s")
    say(f"  fused average: +{statistics.median(ms['adam_ema']) - statistics.median(ms['adam']):.4f} ms on the adam "
        f"kernel (8/28 of it would be {statistics.median(ms['adam']) * 8 / 28:.4f} ms)")


def whole_step(torch, pkg_train, pkg_diffusion, ema, rounds, block, say, label):
    """ms/step of the eager B = 256 step.  ``ema``: one TrainStep(ema_decay=0.9999) whose average is switched off for
    every other block by hiding its buffer - the eager step then makes exactly the launches of ``ema_decay=None``, on the
    same model, plan and streams (of two TrainSteps on two models in one process the second runs milliseconds slower
    whatever its optimizer does: ``side_by_side``).  Not ``ema``: a real TrainStep(ema_decay=None), nothing emulated."""
    dev = torch.device("cuda", torch.cuda.current_device())
    fp = pkg_diffusion.ForwardProcess()
    g = torch.Generator(device=dev).manual_seed(0)
    x0 = torch.rand(BATCH, 1, 28, 28, device=dev, generator=g) * 2 - 1
    torch.manual_seed(0)
    model = pkg_diffusion.NoiseModel().to(dev).train()
    step = pkg_train.TrainStep(model, fp, lr=1e-3, philox_seed=1234, **(dict(ema_decay=0.9999) if ema else {}))
    buf = step.ema if ema else None
    for _ in range(10):
        step.step(x0)
    torch.cuda.synchronize()
    modes = ["None", "0.9999"] if ema else ["None"]
    ms = {m: [] for m in modes}
    for _ in range(rounds):
        for m in modes:
            if ema:
                step.ema = buf if m == "0.9999" else None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(block):
                loss = step.step(x0)
            e1.record()
            torch.cuda.synchronize()
            assert torch.isfinite(loss).all()
            ms[m].append(e0.elapsed_time(e1) / block)
    if ema:
        step.ema = buf
    n = step.flat_param.numel()
    say(f"whole step ({label}), MNIST UNet B = {BATCH}, eager, {n} parameters, {rounds} interleaved rounds of {block} steps")
    for m in modes:
        say(f"  ema_decay={m:<7} ms/step: {spread(ms[m])}")
    if ema:
        say("  (the None rows here are ONE TrainStep(ema_decay=0.9999) with its average hidden for the block, so that it "
            "makes the launches of ema_decay=None on the same plan; a real TrainStep(ema_decay=None) is timed by --step-only)")
        diffs = [y - x for x, y in zip(ms["None"], ms["0.9999"])]
        say(f"  difference (0.9999 - None) per round, ms: {spread(diffs)}; spread of the ema_decay=None rows "
            f"{max(ms['None']) - min(ms['None']):.4f} ms")
    return n


def side_by_side(torch, pkg_train, pkg_diffusion, rounds, block, say):
    """Two plain TrainSteps (no average) on two models in one process, blocks interleaved: what a comparison of two
    differently configured steps side by side would be measuring."""
    dev = torch.device("cuda", torch.cuda.current_device())
    fp = pkg_diffusion.ForwardProcess()
    g = torch.Generator(device=dev).manual_seed(0)
    x0 = torch.rand(BATCH, 1, 28, 28, device=dev, generator=g) * 2 - 1
    steps = []
    for _ in range(2):
        torch.manual_seed(0)
        steps.append(pkg_train.TrainStep(pkg_diffusion.NoiseModel().to(dev).train(), fp, lr=1e-3, philox_seed=1234))
        for _ in range(10):
            steps[-1].step(x0)
    torch.cuda.synchronize()
    ms = [[], []]
    for _ in range(rounds):
        for i, st in enumerate(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(block):
                st.step(x0)
            e1.record()
            torch.cuda.synchronize()
            ms[i].append(e0.elapsed_time(e1) / block)
    say(f"two plain TrainSteps (ema_decay=None) on two models in one process, {rounds} interleaved rounds of {block} steps")
    say(f"  first constructed   ms/step: {spread(ms[0])}")
    say(f"  second constructed  ms/step: {spread(ms[1])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--block", type=int, default=20, help="steps per timed block of the whole-step part")
    ap.add_argument("--tree", default=None, help="import the package from this checkout (default: the one this tool is in)")
    ap.add_argument("--step-only", action="store_true", help="only the whole step of a real TrainStep(ema_decay=None)")
    ap.add_argument("--side-by-side", action="store_true", help="only two plain TrainSteps on two models in one process")
    ap.add_argument("--label", default=None, help="what --tree holds, for the output")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch

    import tiny_diffusion_amd.diffusion as D
    import tiny_diffusion_amd.train as T
    from tiny_diffusion_amd._lib import check, lib

    assert os.path.abspath(T.__file__).startswith(root + os.sep), T.__file__
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# {torch.cuda.get_device_name(0)}; HIP-event times; tools/gpu_ema_cost.py"
        + (" --step-only" if a.step_only else "") + (" --side-by-side" if a.side_by_side else "")
        + (f" --tree: {a.label or 'another checkout'}" if a.tree else ""))
    if a.side_by_side:
        side_by_side(torch, T, D, min(a.rounds, 4), a.block, say)
    elif a.step_only:
        whole_step(torch, T, D, False, a.rounds, a.block, say, (a.label or "another checkout") if a.tree else "this tree")
    else:
        n = whole_step(torch, T, D, True, a.rounds, a.block, say, "this tree")
        torch.cuda.empty_cache()
        isolated(torch, lib, check, n, a.rounds, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
