#!/usr/bin/env python3
"""What the training timestep sampler costs on the GPU (``TrainStep`` / ``TransformerTrainStep`` with
``timestep_sampler=...``; csrc/timestep.hip: tdx_timestep_draw, tdx_mse_per_sample, tdx_timestep_history_update).

1. The whole training step with the sampler off, with a fixed table (logit-normal, importance weights on: the draw,
   the weighted loss entry and the per-sample loss) and with the adaptive sampler (the history update on top): ONE
   step object per model in one process, blocks of steps alternated in rounds, the mode switched between blocks by
   hiding the sampler (``timestep_sampler = None`` makes exactly the launches of a default step on the same model,
   plan and streams; of two TrainSteps on two models in one process the second runs milliseconds slower whatever it
   does: tools/gpu_ema_cost.py --side-by-side).  The MNIST UNet at the benchmark's B = 256 (eager, Philox noise) and the
   transformer at B = 128.  The adaptive sampler is timed warmed up: its history is loaded full (every timestep
   ``history_per_term`` losses of 1), since before that it draws from the uniform table with the same launches.
2. The four launches in isolation at the UNet step's size (B = 256 samples of 784 elements, T = 1000, H = 10,
   cache-resident: latency figures).

Every timed window starts and ends with a device synchronise.

    python3 tools/gpu_timestep_sampler_cost.py [--rounds 7] [--out profiles/timestep_sampler_cost.txt]"""
import argparse
import os
import statistics
import sys
import time

T_STEPS, HIST = 1000, 10


def spread(xs):
    return f"median {statistics.median(xs):.4f}  min {min(xs):.4f}  max {max(xs):.4f}"


def timed_ms(torch, fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, out


class Modes:
    """One step built with the adaptive sampler, switched between off / table / adaptive."""

    names = ("off", "table", "adaptive")

    def __init__(self, torch, step, probs):
        self.torch, self.step = torch, step
        self.probs = probs.to(torch.float32).to(step.device)
        step.load_timestep_sampler_state({"history": torch.ones(T_STEPS, HIST), "counts": torch.full((T_STEPS,), HIST)})

    def select(self, mode):
        s = self.step
        if mode == "off":
            s.timestep_sampler, s.importance_weights = None, False
        elif mode == "table":
            s.timestep_sampler, s.importance_weights, s._ts_probs = "table", True, self.probs
            s._rebuild_timestep_table()
        else:
            s.timestep_sampler, s.importance_weights = "loss_second_moment", True
            s._rebuild_timestep_table()


def whole_step(torch, make, label, batch, rounds, block, say):
    step, run = make()
    from tiny_diffusion_amd.schedule import logit_normal_timestep_probs

    modes = Modes(torch, step, logit_normal_timestep_probs(T_STEPS))
    for m in Modes.names:       # warm up every launch of every mode
        modes.select(m)
        for _ in range(10):
            run()
    ms = {m: [] for m in Modes.names}
    for _ in range(rounds):
        for m in Modes.names:
            modes.select(m)
            t, loss = timed_ms(torch, run, block)
            assert torch.isfinite(loss).all()
            ms[m].append(t)
    say(f"whole step, {label}, B = {batch}, eager, {rounds} alternated rounds of {block} steps, host clock between device "
        f"synchronises")
    for m in Modes.names:
        say(f"  sampler {m:<9} ms/step: {spread(ms[m])}")
    for m in Modes.names[1:]:
        say(f"  difference ({m} - off) per round, ms: {spread([y - x for x, y in zip(ms['off'], ms[m])])}")
    say(f"  spread of the off rows {max(ms['off']) - min(ms['off']):.4f} ms")


def isolated(torch, lib, check, rounds, say, reps=200):
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    B, per = 256, 784
    g = torch.Generator(device=dev).manual_seed(1)
    a = torch.randn(B, per, device=dev, generator=g)
    b = torch.randn(B, per, device=dev, generator=g)
    t = torch.randint(0, T_STEPS, (B,), device=dev, generator=g)
    probs = torch.rand(T_STEPS, device=dev, generator=g)
    w_obj = torch.rand(T_STEPS, device=dev, generator=g) + 0.5
    cdf, w_eff = torch.empty(T_STEPS, device=dev), torch.empty(T_STEPS, device=dev)
    hist = torch.rand(T_STEPS, HIST, device=dev, generator=g) + 0.1
    counts = torch.full((T_STEPS,), HIST, dtype=torch.int32, device=dev)
    t_out = torch.empty(B, dtype=torch.int64, device=dev)
    loss_b = torch.empty(B, device=dev)
    p = lambda *ts: tuple(q.data_ptr() for q in ts)  # noqa: E731
    rows = {
        "timestep_cdf": lambda: check(lib.tdx_timestep_cdf(*p(probs, w_obj), 1, *p(cdf, w_eff), T_STEPS, st)),
        "timestep_draw": lambda: check(lib.tdx_timestep_draw(cdf.data_ptr(), T_STEPS, t_out.data_ptr(), None, B, 1, 2, None, st)),
        "mse_per_sample": lambda: check(lib.tdx_mse_per_sample(*p(a, b, t, w_obj, loss_b), B, per, st)),
        "timestep_history_update": lambda: check(lib.tdx_timestep_history_update(*p(t, loss_b), B, *p(hist, counts), HIST,
                                                                                 0.001, *p(w_obj, cdf, w_eff), T_STEPS, st)),
    }
    for fn in rows.values():
        fn()
    ms = {name: [] for name in rows}
    for _ in range(rounds):
        for name, fn in rows.items():
            ms[name].append(timed_ms(torch, fn, reps)[0] * 1e3)
    say(f"isolated entries, B = {B} x {per} fp32 elements, T = {T_STEPS}, H = {HIST} (cache-resident), back to back on one "
        f"stream, {rounds} alternated rounds of {reps} calls (timestep_cdf runs at construction and set_objective only)")
    for name in rows:
        say(f"  {name:<24} us/call: {spread(ms[name])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--block", type=int, default=20, help="steps per timed block of the whole-step parts")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    import tiny_diffusion_amd.diffusion as D
    import tiny_diffusion_amd.diffusion_transformer as DT
    import tiny_diffusion_amd.train as TR
    from tiny_diffusion_amd._lib import check, lib

    dev = torch.device("cuda", torch.cuda.current_device())
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    kw = dict(timestep_sampler="loss_second_moment", history_per_term=HIST, timestep_seed=7)

    def unet():
        g = torch.Generator(device=dev).manual_seed(0)
        x0 = torch.rand(256, 1, 28, 28, device=dev, generator=g) * 2 - 1
        torch.manual_seed(0)
        step = TR.TrainStep(D.NoiseModel().to(dev).train(), D.ForwardProcess(), lr=1e-3, philox_seed=1234, **kw)
        return step, lambda: step.step(x0)

    def transformer():
        g = torch.Generator(device=dev).manual_seed(0)
        z0 = torch.randn(128, 20, device=dev, generator=g)
        y = torch.randint(0, 10, (128,), device=dev, generator=g)
        torch.manual_seed(0)
        step = DT.TransformerTrainStep(DT.NoiseModel().to(dev).train(), DT.ForwardProcess(), lr=3e-4, philox_seed=1234,
                                       dropout_seed=5, **kw)
        return step, lambda: step.step(z0, y)

    say(f"# {torch.cuda.get_device_name(0)}; tools/gpu_timestep_sampler_cost.py")
    whole_step(torch, unet, "MNIST UNet (TrainStep, Philox noise)", 256, a.rounds, a.block, say)
    whole_step(torch, transformer, "transformer (TransformerTrainStep, Philox noise)", 128, a.rounds, a.block * 5, say)
    isolated(torch, lib, check, a.rounds, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
