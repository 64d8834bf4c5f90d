#!/usr/bin/env python3
"""ms per optimisation step of the transformer noise model (diffusion_transformer.py) on the GPU at B = 128 (the
reference's batch_size) with the default model (dim 256, 4 heads, 4 blocks, dropout 0.05, train mode):

  a) "module + autograd": the path before TransformerTrainStep - the module's op-by-op forward (one libtdx launch per
     ``ops`` function), ``F.mse_loss``, torch autograd, ``torch.optim.Adam`` over the 60 tensors;
  b) "tdx eager":         ``TransformerTrainStep.step``;
  c) "tdx graph":         the same with ``use_graph=True`` (captured, replayed).

Protocol (tools/gpu_vae_train.py's): every variant is built and warmed up (the graph variant past its capture), then
``--rounds`` rounds in one process; in a round each variant runs ``--steps`` steps between two HIP events, the variants
interleaved; median and min .. max over the rounds.  The same latents and labels every step; ``t`` from ``torch.randint``
and the noise from ``torch.randn`` in all three, as the reference's loop draws them.  Every phase on the GPU (a variant's
warm-up, a variant's timed round) runs under its own time limit (``--phase-timeout`` seconds, a watchdog that ends the
process), and the first failure - an exception, a non-finite loss, a time limit - ends the tool: nothing is retried.
Also reports the launches of one step of (a) and (b), counted from the call chain.

    python3 tools/gpu_transformer_train.py [--steps 200] [--rounds 5] [--out profiles/transformer_train.txt]"""
import argparse
import faulthandler
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return f"median {statistics.median(xs):.4f}  min {min(xs):.4f} .. max {max(xs):.4f}"


def launch_counts(L):
    """Launches of one train-mode step, counted from the call chain (diffusion_transformer.py / ops.py for the module
    path, csrc/transformer.hip for the fused one); the loss and the optimizer are counted separately."""
    module_fwd = 8 + 13 * L + 2
    # backward of the module path: Linear = wgrad + bias column sum + dgrad (no dgrad where the input needs none),
    # LayerNorm = 2, activation 1, dropout 1, embedding 1, a broadcast-row add 1; torch's own gradient accumulation
    # kernels (one per tensor used twice: 2 per block + 2 in the stem) are NOT in this count
    module_bwd = (2 + 1 + 3 + 1 + 2 + 1) + (4 * 3 + 2 * 2 + 1 + 4) * L + (2 + 3)
    fused_fwd = 3 + 6 * L + 2
    fused_bwd = 3 + 6 * L + 2
    return module_fwd, module_bwd, fused_fwd, fused_bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="timed steps per round and variant (>= 200, enforced)")
    ap.add_argument("--rounds", type=int, default=5, help="rounds (>= 5, enforced)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--phase-timeout", type=float, default=120.0, help="seconds one GPU phase may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 200 or a.rounds < 5:
        ap.error("the protocol is at least 200 timed steps per round and at least 5 rounds: a shorter window would be "
                 "written in the same format and read as a measurement")
    import torch
    import torch.nn.functional as F

    from tiny_diffusion_amd.diffusion_transformer import ForwardProcess, NoiseModel, TransformerTrainStep

    if not torch.cuda.is_available():
        raise SystemExit("tools/gpu_transformer_train.py measures on the GPU: none visible")
    dev = torch.device("cuda", 0)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def phase(fn):
        """One GPU phase under its own time limit; an exception leaves the tool (no second attempt)."""
        faulthandler.dump_traceback_later(a.phase_timeout, exit=True)
        try:
            return fn()
        finally:
            faulthandler.cancel_dump_traceback_later()

    say(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; HIP-event times; tools/gpu_transformer_train.py "
        f"--steps {a.steps} --rounds {a.rounds} --warmup {a.warmup} --batch {a.batch}")
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in NoiseModel().state_dict().items()}
    L = 4
    mf, mb, ff, fb = launch_counts(L)
    say(f"# NoiseModel default (dim 256, 4 heads, {L} blocks, dropout 0.05), {sum(v.numel() for v in sd.values())} "
        f"parameters in {len(sd)} tensors, default init (seed 0), lr 3e-4, train mode")
    say(f"# launches per step, counted from the call chain: module forward {mf}, backward {mb} (+ torch's gradient "
        f"accumulations, mse_loss and its backward, Adam over {len(sd)} tensors); fused forward {ff}, loss 2, backward "
        f"{fb}, Adam 1; both + randint, randn, q_sample")
    B = a.batch
    g = torch.Generator().manual_seed(B)
    z0 = torch.randn(B, 20, generator=g).to(dev)
    y = torch.randint(0, 10, (B,), generator=g).to(dev)
    fp = ForwardProcess()

    def fresh():
        m = NoiseModel()
        m.load_state_dict(sd)
        return m.to(dev).train()

    def module_step_factory():
        m = fresh()
        opt = torch.optim.Adam(m.parameters(), lr=3e-4)

        def step():
            t = torch.randint(0, fp.num_timesteps, (B,), device=dev)
            z_t, noise = fp.q_sample(dev, z0, t)
            loss = F.mse_loss(m(z_t, t, y), noise)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss.detach()

        return step

    variants = {"module + autograd": module_step_factory()}
    for name, kw in (("tdx eager", {}), ("tdx graph", dict(use_graph=True))):
        ts = TransformerTrainStep(fresh(), fp, lr=3e-4, **kw)
        variants[name] = (lambda ts=ts: ts.step(z0, y))
    first = {}

    def warm(name, fn):
        first[name] = float(fn())
        for _ in range(a.warmup - 1):
            loss = fn()
        torch.cuda.synchronize()
        if not bool(torch.isfinite(loss).all()):
            raise SystemExit(f"{name}: non-finite loss in the warm-up")

    for name, fn in variants.items():
        phase(lambda: warm(name, fn))
    ms = {name: [] for name in variants}
    last = {}

    def timed(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            loss = fn()
        e1.record()
        torch.cuda.synchronize()
        if not bool(torch.isfinite(loss).all()):
            raise SystemExit(f"{name}: non-finite loss")
        ms[name].append(e0.elapsed_time(e1) / a.steps)
        last[name] = float(loss)

    for _ in range(a.rounds):
        for name, fn in variants.items():
            phase(lambda: timed(name, fn))
    say(f"B = {B}: ms/step over {a.rounds} interleaved rounds of {a.steps} steps")
    for name in variants:
        say(f"  {name:<18} {spread(ms[name])}   loss first {first[name]:.3f} -> last {last[name]:.3f}")
    med = {name: statistics.median(ms[name]) for name in variants}
    say(f"  module + autograd / tdx eager = {med['module + autograd'] / med['tdx eager']:.2f}x;  "
        f"tdx graph / tdx eager = {med['tdx graph'] / med['tdx eager']:.2f}x")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
