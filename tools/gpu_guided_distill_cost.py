#!/usr/bin/env python3
"""What the guided distillation steps cost on the GPU (``train.DistillStep(guidance_scale=w)``,
``train.GuidanceDistillStep``; csrc/distill.hip: tdx_distill_teacher_step_guided, tdx_distill_target_guided,
tdx_distill_guidance_target).

1. Four steps on the SAME step object, student, teacher, plans and streams - the conditional MNIST UNet at B = 256,
   Philox noise, clamp (-1, 1), truncated-SNR weights, N = 4 student steps, w = 3:
       plain      a plain v-prediction step: ``FlatStep._q_sample`` in place of the hook, the grid sampler hidden
       distill    the unguided distillation step: two teacher forwards at B rows
       guided     the guided distillation step: two teacher forwards at 2B rows
       guidance   the guidance-distillation step: ONE teacher forward at 2B rows, t uniform over all T -
                  ``GuidanceDistillStep._q_sample`` bound to the object, its (T, 4) table in place of the (T, 12) one
   (of two steps on two models in one process the second runs milliseconds slower whatever it does:
   tools/gpu_ema_cost.py --side-by-side - hence one object).  Blocks of steps alternate in rounds; every timed window
   starts and ends with a device synchronise.
2. The teacher's inference forward alone at B and at 2B rows (the doubled condition included), alternated the same
   way: what the launch list predicts for the guided step is the unguided one plus twice their difference.  Then a
   cross-check of the "guidance" row: a ``GuidanceDistillStep`` built the ordinary way, on a student of its own.
3. The three new launches in isolation at 256 x 784 (cache-resident: latency figures), beside the two unguided ones.

    python3 tools/gpu_guided_distill_cost.py [--rounds 7] [--block 20] [--out profiles/guided_distill_cost.txt]"""
import argparse
import os
import statistics
import sys
import time
import types

W = 3.0
MODES = ("plain", "distill", "guided", "guidance")


def spread(xs):
    return f"median {statistics.median(xs):.4f}  min {min(xs):.4f}  max {max(xs):.4f}"


def timed_ms(torch, fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def select(step, mode, rows12, rows4):
    """Make the one step object issue the launches of ``mode``."""
    from tiny_diffusion_amd._flat_step import FlatStep
    from tiny_diffusion_amd.train import GuidanceDistillStep

    step.__dict__.pop("_q_sample", None)
    step.timestep_sampler = step._grid_sampler
    step._rows, step.guidance_scale = rows12, None
    step._dbufs.clear()     # sized by guidance_scale, which a step never changes by itself: reallocated once per block
    if mode == "plain":
        step._q_sample = types.MethodType(FlatStep._q_sample, step)
        step.timestep_sampler = None
    elif mode == "guided":
        step.guidance_scale = W
    elif mode == "guidance":
        step._q_sample = types.MethodType(GuidanceDistillStep._q_sample, step)
        step.timestep_sampler = None
        step._rows, step.guidance_scale = rows4, W


def whole_step(torch, dev, rounds, block, say):
    import tiny_diffusion_amd.conditional_diffusion as CD
    import tiny_diffusion_amd.train as TR
    from tiny_diffusion_amd.schedule import guidance_distill_table, truncated_snr_weights
    from tiny_diffusion_amd.unet import MODE_INFER, _cond_tensor, _with_null_cond

    B = 256
    g = torch.Generator(device=dev).manual_seed(0)
    x0 = torch.rand(B, 1, 28, 28, device=dev, generator=g) * 2 - 1
    y = torch.randint(0, 10, (B,), device=dev, generator=g)
    torch.manual_seed(0)
    fp = CD.ForwardProcess()
    teacher = CD.NoiseModel().to(dev)
    student = CD.NoiseModel().to(dev).train()
    student.load_state_dict(teacher.state_dict())
    step = TR.DistillStep(student, teacher, fp, 4, teacher_prediction="eps", prediction="v", clip_denoised=True,
                          loss_weighting=truncated_snr_weights(fp, "v"), lr=1e-4, philox_seed=1234, timestep_seed=7)
    step._grid_sampler = step.timestep_sampler
    step._tbufs = {}
    rows12, rows4 = step._rows, guidance_distill_table(fp, "eps", "v").to(dev)
    run = lambda: step.step(x0, y)  # noqa: E731
    for m in MODES:       # warm up every launch of every mode
        select(step, m, rows12, rows4)
        for _ in range(10):
            run()
    ms = {m: [] for m in MODES}
    for _ in range(rounds):
        for m in MODES:
            select(step, m, rows12, rows4)
            t, loss = timed_ms(torch, run, block)
            assert torch.isfinite(loss).all()
            ms[m].append(t)
    select(step, "distill", rows12, rows4)
    say(f"whole step, conditional MNIST UNet, B = {B}, w = {W}, eager, {rounds} alternated rounds of {block} steps, host "
        f"clock between device synchronises")
    names = {"plain": "plain v step", "distill": "distillation step, unguided", "guided": "distillation step, guided",
             "guidance": "guidance-distillation step"}
    for m in MODES:
        say(f"  {names[m]:<28} ms/step: {spread(ms[m])}")
    med = {m: statistics.median(ms[m]) for m in MODES}
    say(f"  guided - unguided distillation step per round, ms: "
        f"{spread([b - a for a, b in zip(ms['distill'], ms['guided'])])}")
    say(f"  guidance-distillation - plain step per round, ms:  "
        f"{spread([b - a for a, b in zip(ms['plain'], ms['guidance'])])}")
    say(f"  ratios of the medians to the plain step: unguided {med['distill'] / med['plain']:.3f}, guided "
        f"{med['guided'] / med['plain']:.3f}, guidance {med['guidance'] / med['plain']:.3f}; spread of the plain rows "
        f"{max(ms['plain']) - min(ms['plain']):.4f} ms")

    # the teacher's inference forward alone, B against 2B rows
    z = torch.randn(B, 1, 28, 28, device=dev, generator=g)
    t = torch.randint(0, 1000, (B,), device=dev, generator=g)
    z2, t2 = torch.cat([z, z]), torch.cat([t, t])
    kind = teacher._arch.kind
    fwd = {"B": lambda: teacher._run_forward(z, t, y, mode=MODE_INFER)[0],
           "2B": lambda: teacher._run_forward(z2, t2, _with_null_cond(kind, _cond_tensor(kind, y)), mode=MODE_INFER)[0]}
    for fn in fwd.values():
        for _ in range(10):
            fn()
    fms = {k: [] for k in fwd}
    for _ in range(rounds):
        for k, fn in fwd.items():
            fms[k].append(timed_ms(torch, fn, block)[0])
    say(f"teacher inference forward alone, back to back, {rounds} alternated rounds of {block} calls")
    for k in fwd:
        say(f"  {k + ' rows':<28} ms/call: {spread(fms[k])}")
    d = statistics.median(fms["2B"]) - statistics.median(fms["B"])
    say(f"  expectation from the launch list: guided = unguided + 2 x (2B - B forward) = {med['distill']:.4f} + "
        f"{2 * d:.4f} = {med['distill'] + 2 * d:.4f} ms; measured {med['guided']:.4f} ms")
    say(f"  expectation from the launch list: guidance = plain + one 2B forward = {med['plain']:.4f} + "
        f"{statistics.median(fms['2B']):.4f} = {med['plain'] + statistics.median(fms['2B']):.4f} ms; measured "
        f"{med['guidance']:.4f} ms")

    # cross-check: the guidance row above comes from GuidanceDistillStep._q_sample bound to the DistillStep object;
    # here a GuidanceDistillStep as a user builds it, on a student of its own (the second model of the process)
    own = CD.NoiseModel().to(dev).train()
    own.load_state_dict(teacher.state_dict())
    real = TR.GuidanceDistillStep(own, teacher, fp, W, teacher_prediction="eps", prediction="v", clip_denoised=True,
                                  loss_weighting=truncated_snr_weights(fp, "v"), lr=1e-4, philox_seed=1234)
    run_real = lambda: real.step(x0, y)  # noqa: E731
    for _ in range(10):
        run_real()
    rms = [timed_ms(torch, run_real, block)[0] for _ in range(rounds)]
    say(f"cross-check, a GuidanceDistillStep object of its own (second student in the process), {rounds} rounds of "
        f"{block} steps")
    say(f"  {'guidance-distillation step':<28} ms/step: {spread(rms)}")


def isolated(torch, rounds, say, reps=200):
    from tiny_diffusion_amd._lib import check, lib
    from tiny_diffusion_amd.schedule import ForwardProcess, distill_tables, guidance_distill_table, trailing_timesteps

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    fp = ForwardProcess()
    tab = distill_tables(fp, 4)
    rows, tmt, rows4 = tab.rows.to(dev), tab.t_mid.to(dev), guidance_distill_table(fp).to(dev)
    grid = torch.tensor(trailing_timesteps(fp, 4), device=dev)
    B, per = 256, 784
    g = torch.Generator(device=dev).manual_seed(1)
    z = torch.randn(B, per, device=dev, generator=g)
    o1, o2 = (torch.randn(2 * B, per, device=dev, generator=g) for _ in range(2))
    t = grid[torch.randint(0, 4, (B,), device=dev, generator=g)]
    zm, x1, tg = torch.empty(2 * B, per, device=dev), torch.empty_like(z), torch.empty_like(z)
    tm = torch.empty(2 * B, dtype=torch.int64, device=dev)
    p = lambda *ts: tuple(q.data_ptr() for q in ts)  # noqa: E731
    entries = {
        "tdx_distill_teacher_step": lambda: check(lib.tdx_distill_teacher_step(*p(z, o1, t, rows, tmt, zm, x1, tm), B, per,
                                                                               -1.0, 1.0, st)),
        "tdx_distill_target": lambda: check(lib.tdx_distill_target(*p(z, zm, o2, x1, t, rows, tg), None, B, per, -1.0, 1.0,
                                                                   st)),
        "tdx_distill_teacher_step_guided": lambda: check(lib.tdx_distill_teacher_step_guided(
            *p(z, o1, t, rows, tmt, zm, x1, tm), B, per, W, -1.0, 1.0, st)),
        "tdx_distill_target_guided": lambda: check(lib.tdx_distill_target_guided(*p(z, zm, o2, x1, t, rows, tg), None, B,
                                                                                 per, W, -1.0, 1.0, st)),
        "tdx_distill_guidance_target, guided": lambda: check(lib.tdx_distill_guidance_target(
            *p(z, o1, t, rows4, tg), None, B, per, 1, W, -1.0, 1.0, st)),
        "tdx_distill_guidance_target, unguided": lambda: check(lib.tdx_distill_guidance_target(
            *p(z, o1, t, rows4, tg), None, B, per, 0, 0.0, -1.0, 1.0, st)),
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
        say(f"  {name:<38} us/call: {spread(us[name])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--block", type=int, default=20, help="steps per timed block of the whole-step part")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# {torch.cuda.get_device_name(0)}; tools/gpu_guided_distill_cost.py")
    whole_step(torch, dev, a.rounds, a.block, say)
    isolated(torch, a.rounds, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
