#!/usr/bin/env python3
"""What a progressive-distillation step costs on the GPU (``train.DistillStep``; csrc/distill.hip:
tdx_distill_teacher_step, tdx_distill_target).

1. ``DistillStep.step`` against the plain training step on the SAME step object, model, plan and streams: the mode is
   switched between blocks by putting ``FlatStep._q_sample`` back in place of the distillation hook and hiding the
   on-grid timestep sampler - exactly the launches of ``TrainStep(prediction="v", loss_weighting=<table>)`` (of two
   steps on two models in one process the second runs milliseconds slower whatever it does: tools/gpu_ema_cost.py
   --side-by-side).  Blocks of steps alternate in rounds; every timed window starts and ends with a device synchronise.
   The conditional MNIST UNet at B = 256 and the latent MLP at B = 128, Philox noise, N = 4 student steps, clamp
   (-1, 1), truncated-SNR weights.
2. The two new launches in isolation at both sizes (cache-resident: latency figures).

    python3 tools/gpu_distill_cost.py [--rounds 7] [--block 20] [--out profiles/distill_cost.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 tools/gpu_distill_cost.py --profile
        (20 distillation steps of each model and nothing else: the two kernels' rows of <dir>/**/*kernel_stats.csv)"""
import argparse
import os
import statistics
import sys
import time
import types


def spread(xs):
    return f"median {statistics.median(xs):.4f}  min {min(xs):.4f}  max {max(xs):.4f}"


def timed_ms(torch, fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def select(step, mode, base_q_sample):
    """"distill": the step as built.  "plain": the same object makes a plain v-prediction step's launches."""
    if mode == "plain":
        step._q_sample = types.MethodType(base_q_sample, step)
        if step.timestep_sampler is not None:
            step._saved_sampler, step.timestep_sampler = step.timestep_sampler, None
    else:
        step.__dict__.pop("_q_sample", None)
        step.timestep_sampler = step.__dict__.pop("_saved_sampler", step.timestep_sampler)


def make_steps(torch, dev):
    import tiny_diffusion_amd.conditional_diffusion as CD
    import tiny_diffusion_amd.latent_diffusion as LD
    import tiny_diffusion_amd.train as TR
    from tiny_diffusion_amd.schedule import truncated_snr_weights

    def build(module, B, shape, lr):
        g = torch.Generator(device=dev).manual_seed(0)
        x0 = torch.rand(B, *shape, device=dev, generator=g) * 2 - 1
        y = torch.randint(0, 10, (B,), device=dev, generator=g)
        torch.manual_seed(0)
        fp = module.ForwardProcess()
        teacher = module.NoiseModel().to(dev)
        student = module.NoiseModel().to(dev).train()
        student.load_state_dict(teacher.state_dict())
        step = TR.DistillStep(student, teacher, fp, 4, teacher_prediction="eps", prediction="v", clip_denoised=True,
                              loss_weighting=truncated_snr_weights(fp, "v"), lr=lr, philox_seed=1234, timestep_seed=7)
        return step, lambda: step.step(x0, y)

    return [("conditional MNIST UNet", 256, lambda: build(CD, 256, (1, 28, 28), 1e-4)),
            ("latent MLP", 128, lambda: build(LD, 128, (20,), 1e-4))]


def whole_step(torch, label, batch, make, rounds, block, say):
    from tiny_diffusion_amd._flat_step import FlatStep

    step, run = make()
    modes = ("plain", "distill")
    for m in modes:       # warm up every launch of both modes
        select(step, m, FlatStep._q_sample)
        for _ in range(10):
            run()
    ms = {m: [] for m in modes}
    for _ in range(rounds):
        for m in modes:
            select(step, m, FlatStep._q_sample)
            t, loss = timed_ms(torch, run, block)
            assert torch.isfinite(loss).all()
            ms[m].append(t)
    select(step, "distill", FlatStep._q_sample)
    say(f"whole step, {label}, B = {batch}, eager, {rounds} alternated rounds of {block} steps, host clock between device "
        f"synchronises")
    say(f"  plain v step      ms/step: {spread(ms['plain'])}")
    say(f"  distillation step ms/step: {spread(ms['distill'])}")
    say(f"  difference (distill - plain) per round, ms: {spread([y - x for x, y in zip(ms['plain'], ms['distill'])])}")
    say(f"  ratio of the medians {statistics.median(ms['distill']) / statistics.median(ms['plain']):.3f}; spread of the "
        f"plain rows {max(ms['plain']) - min(ms['plain']):.4f} ms")


def isolated(torch, rounds, say, reps=200):
    from tiny_diffusion_amd._lib import check, lib
    from tiny_diffusion_amd.schedule import ForwardProcess, distill_tables, trailing_timesteps

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    fp = ForwardProcess()
    tab = distill_tables(fp, 4)
    rows, tmt = tab.rows.to(dev), tab.t_mid.to(dev)
    grid = torch.tensor(trailing_timesteps(fp, 4), device=dev)
    for B, per in ((256, 784), (128, 20)):
        g = torch.Generator(device=dev).manual_seed(1)
        z, o1, o2 = (torch.randn(B, per, device=dev, generator=g) for _ in range(3))
        t = grid[torch.randint(0, 4, (B,), device=dev, generator=g)]
        zm, x1, tg = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
        tm = torch.empty_like(t)
        p = lambda *ts: tuple(q.data_ptr() for q in ts)  # noqa: E731
        entries = {
            "tdx_distill_teacher_step": lambda: check(lib.tdx_distill_teacher_step(*p(z, o1, t, rows, tmt, zm, x1, tm), B,
                                                                                   per, -1.0, 1.0, st)),
            "tdx_distill_target": lambda: check(lib.tdx_distill_target(*p(z, zm, o2, x1, t, rows, tg), None, B, per, -1.0,
                                                                       1.0, st)),
        }
        for fn in entries.values():
            fn()
        us = {name: [] for name in entries}
        for _ in range(rounds):
            for name, fn in entries.items():
                us[name].append(timed_ms(torch, fn, reps)[0] * 1e3)
        say(f"isolated entries, B = {B} x {per} fp32 elements (cache-resident), back to back on one stream, {rounds} "
            f"alternated rounds of {reps} calls")
        for name in entries:
            say(f"  {name:<26} us/call: {spread(us[name])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--block", type=int, default=20, help="steps per timed block of the whole-step part")
    ap.add_argument("--profile", action="store_true", help="20 distillation steps per model and nothing else")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    if a.profile:
        for label, batch, make in make_steps(torch, dev):
            step, run = make()
            for _ in range(20):
                loss = run()
            torch.cuda.synchronize()
            print(f"{label} B = {batch}: 20 distillation steps, loss {loss.item():.5f}", flush=True)
        return
    say(f"# {torch.cuda.get_device_name(0)}; tools/gpu_distill_cost.py")
    for label, batch, make in make_steps(torch, dev):
        whole_step(torch, label, batch, make, a.rounds, a.block * (5 if batch == 128 else 1), say)
    isolated(torch, a.rounds, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
