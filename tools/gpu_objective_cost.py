#!/usr/bin/env python3
"""What the training objective costs on the GPU (TrainStep(prediction="v", loss_weighting="min_snr"),
csrc/elementwise.hip: tdx_q_sample_target_philox, tdx_mse_loss_grad_weighted).

1. The whole training step, B = 256 on the MNIST UNet, eager, Philox noise, with the default objective and with
   v-prediction + min-SNR weighting: ONE TrainStep in one process, blocks of steps interleaved, the objective switched
   back to the default for every other block (``TrainStep.set_objective()`` - the step then makes exactly the
   launches of a default TrainStep on the same model, plan and streams; of two TrainSteps on two
   models in one process the second runs milliseconds slower whatever it does: tools/gpu_ema_cost.py --side-by-side).
2. The four launches in isolation at the step's size (256 x 784 elements, cache-resident: these are latency figures,
   what the step pays between forward and backward): the old and the new q_sample, the old and the new loss.

``--step-only`` times a real default ``TrainStep`` alone in its process; ``--tree DIR`` imports the package from ANOTHER
checkout of the project (the parent commit, built in DIR) for a same-session figure beside this tree's; ``--append``
adds to ``--out``.

    python3 tools/gpu_objective_cost.py [--rounds 7] [--out profiles/objective_cost.txt]
    python3 tools/gpu_objective_cost.py --step-only --append --out profiles/objective_cost.txt
    python3 tools/gpu_objective_cost.py --step-only --tree ../parent --label "parent commit" --append --out ..."""
import argparse
import os
import statistics
import sys

BATCH = 256


def spread(xs):
    return f"median {statistics.median(xs):.4f}  min {min(xs):.4f}  max {max(xs):.4f}"


def timed_ms(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def whole_step(torch, pkg_train, pkg_diffusion, objective, rounds, block, say, label):
    dev = torch.device("cuda", torch.cuda.current_device())
    fp = pkg_diffusion.ForwardProcess()
    g = torch.Generator(device=dev).manual_seed(0)
    x0 = torch.rand(BATCH, 1, 28, 28, device=dev, generator=g) * 2 - 1
    torch.manual_seed(0)
    model = pkg_diffusion.NoiseModel().to(dev).train()
    kw = dict(prediction="v", loss_weighting="min_snr") if objective else {}
    step = pkg_train.TrainStep(model, fp, lr=1e-3, philox_seed=1234, **kw)
    modes = ["default", "v+min_snr"] if objective else ["default"]

    def select(mode):
        if objective:
            step.set_objective(**(kw if mode == "v+min_snr" else {}))

    for mode in modes:       # warm up every launch of both objectives
        select(mode)
        for _ in range(10):
            step.step(x0)
    torch.cuda.synchronize()
    ms = {m: [] for m in modes}
    for _ in range(rounds):
        for m in modes:
            select(m)
            t, loss = timed_ms(torch, lambda: step.step(x0), block)
            assert torch.isfinite(loss).all()
            ms[m].append(t)
    select(modes[-1])
    say(f"whole step ({label}), MNIST UNet B = {BATCH}, eager, Philox noise, {rounds} interleaved rounds of {block} steps")
    for m in modes:
        say(f"  objective {m:<10} ms/step: {spread(ms[m])}")
    if objective:
        say("  (the default rows here are ONE TrainStep(prediction='v', loss_weighting='min_snr') switched back to the default "
            "objective for the block, so that it makes the launches of a default TrainStep on the same plan; a real default "
            "TrainStep is timed by --step-only)")
        diffs = [y - x for x, y in zip(ms["default"], ms["v+min_snr"])]
        say(f"  difference (v+min_snr - default) per round, ms: {spread(diffs)}; spread of the default rows "
            f"{max(ms['default']) - min(ms['default']):.4f} ms")


def isolated(torch, fp, lib, check, loss_weights, rounds, say, reps=200):
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    per = 784
    g = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.rand(BATCH, per, device=dev, generator=g) * 2 - 1
    out = torch.randn(BATCH, per, device=dev, generator=g)
    t = torch.randint(0, fp.num_timesteps, (BATCH,), device=dev, generator=g)
    sa, s1, _ = fp.tables(dev)
    w = loss_weights(fp, "v", "min_snr").to(dev)
    x_t, tgt, d = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
    loss = torch.zeros(1, device=dev)
    scratch = torch.empty(lib.tdx_mse_scratch_bytes(), dtype=torch.uint8, device=dev)
    p = lambda *ts: tuple(q.data_ptr() for q in ts)  # noqa: E731
    rows = {
        "q_sample_philox": lambda: check(lib.tdx_q_sample_philox(*p(x0, t, sa, s1, x_t, tgt), BATCH, per, 1, 0, st)),
        "q_sample_target_philox (v)": lambda: check(lib.tdx_q_sample_target_philox(*p(x0, t, sa, s1, x_t, tgt), BATCH, per,
                                                                                   1, 1, 0, st)),
        "mse_loss_grad": lambda: check(lib.tdx_mse_loss_grad(*p(out, tgt, loss, d), 1.0, BATCH * per, scratch.data_ptr(), st)),
        "mse_loss_grad_weighted": lambda: check(lib.tdx_mse_loss_grad_weighted(*p(out, tgt, t, w, loss, d), 1.0, BATCH, per,
                                                                               scratch.data_ptr(), st)),
    }
    for fn in rows.values():
        fn()
    ms = {name: [] for name in rows}
    for _ in range(rounds):
        for name, fn in rows.items():
            ms[name].append(timed_ms(torch, fn, reps)[0] * 1e3)
    say(f"isolated entries, {BATCH} x {per} fp32 elements (cache-resident), back to back on one stream, {rounds} interleaved "
        f"rounds of {reps} calls; the two loss entries are two launches each")
    for name in rows:
        say(f"  {name:<28} us/call: {spread(ms[name])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--block", type=int, default=20, help="steps per timed block of the whole-step part")
    ap.add_argument("--tree", default=None, help="import the package from this checkout (default: the one this tool is in)")
    ap.add_argument("--step-only", action="store_true", help="only the whole step of a real default TrainStep")
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

    say(f"# {torch.cuda.get_device_name(0)}; HIP-event times; tools/gpu_objective_cost.py"
        + (" --step-only" if a.step_only else "") + (f" --tree: {a.label or 'another checkout'}" if a.tree else ""))
    if a.step_only:
        whole_step(torch, T, D, False, a.rounds, a.block, say, (a.label or "another checkout") if a.tree else "this tree")
    else:
        from tiny_diffusion_amd.schedule import loss_weights

        whole_step(torch, T, D, True, a.rounds, a.block, say, "this tree")
        isolated(torch, D.ForwardProcess(), lib, check, loss_weights, a.rounds, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
