#!/usr/bin/env python3
"""ms per optimisation step of the VAE (VAETrainStep, tiny_diffusion_amd/vae.py) on the GPU, at B = 128 (the reference's
batch_size) and B = 1024: the eager step, the captured step (``use_graph=True``) and, as the yardstick, a stock
PyTorch-ROCm step of the same model written out here (five ``nn.Linear``, ``F.binary_cross_entropy(reduction="sum")`` +
KLD, ``torch.optim.Adam``) - eager torch, autograd, no compile.

Protocol: every variant is built and warmed up (the graph variant past its capture), then ``--rounds`` rounds in one
process; in a round each variant runs ``--steps`` steps between two HIP events, the variants interleaved; median and
min .. max over the rounds.  The same batch every step; noise from ``torch.randn`` in all three (drawn outside the
graph by the captured step).  Also reports the launches of one eager step counted from the call chain.

    python3 tools/gpu_vae_train.py [--steps 200] [--rounds 5] [--out profiles/vae_train.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return f"median {statistics.median(xs):.4f}  min {min(xs):.4f} .. max {max(xs):.4f}"


def torch_step_factory(torch, cfg, sd, dev):
    import torch.nn as nn
    import torch.nn.functional as F

    class TorchVAE(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1 = nn.Linear(cfg.input_dim, cfg.hidden_dim)
            self.fc21 = nn.Linear(cfg.hidden_dim, cfg.latent_dim)
            self.fc22 = nn.Linear(cfg.hidden_dim, cfg.latent_dim)
            self.fc3 = nn.Linear(cfg.latent_dim, cfg.hidden_dim)
            self.fc4 = nn.Linear(cfg.hidden_dim, cfg.input_dim)

        def forward(self, x):
            h1 = F.relu(self.fc1(x))
            mu, logvar = self.fc21(h1), self.fc22(h1)
            z = mu + torch.randn_like(mu) * torch.exp(0.5 * logvar)
            return torch.sigmoid(self.fc4(F.relu(self.fc3(z)))), mu, logvar

    model = TorchVAE()
    model.load_state_dict(sd)
    model = model.to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)

    def step(x):
        opt.zero_grad()
        recon, mu, logvar = model(x)
        bce = F.binary_cross_entropy(recon, (x + 1) / 2, reduction="sum")
        kld = -0.5 * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())
        loss = bce + kld
        loss.backward()
        opt.step()
        return loss.detach()

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="timed steps per round and variant (>= 200, enforced)")
    ap.add_argument("--rounds", type=int, default=5, help="rounds (>= 5, enforced)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 200 or a.rounds < 5:
        ap.error("the protocol is at least 200 timed steps per round and at least 5 rounds: a shorter window would be "
                 "written in the same format and read as a measurement")
    import torch

    from tiny_diffusion_amd.vae import VAE, VAEConfig, VAETrainStep

    if not torch.cuda.is_available():
        raise SystemExit("tools/gpu_vae_train.py measures on the GPU: none visible")
    dev = torch.device("cuda", 0)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; HIP-event times; tools/gpu_vae_train.py "
        f"--steps {a.steps} --rounds {a.rounds} --warmup {a.warmup}")
    cfg = VAEConfig()
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in VAE(cfg).state_dict().items()}
    n_param = sum(v.numel() for v in sd.values())
    say(f"# VAE {cfg.input_dim}-{cfg.hidden_dim}-{cfg.latent_dim}, {n_param} parameters, default init (seed 0), lr 1e-3; "
        "one eager VAETrainStep = 24 launches: 6 forward (5 GEMM + reparameterise), BCE, KLD, loss finish, 14 backward "
        "(5 wgrad, 3 dgrad + 1 accumulating, 3 bias column sums, 2 ReLU-mask + bias sums), Adam; + torch.randn")
    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        x = (torch.rand(B, cfg.input_dim, generator=g) * 2 - 1).to(dev)
        variants = {}
        for name, kw in (("tdx eager", {}), ("tdx graph", dict(use_graph=True))):
            vae = VAE(cfg)
            vae.load_state_dict(sd)
            ts = VAETrainStep(vae.to(dev), lr=1e-3, **kw)
            variants[name] = (lambda ts=ts: ts.step(x))
        variants["torch eager"] = (lambda f=torch_step_factory(torch, cfg, sd, dev): f(x))
        first = {}
        for name, fn in variants.items():
            first[name] = float(fn())
            for _ in range(a.warmup - 1):
                loss = fn()
            torch.cuda.synchronize()
            assert torch.isfinite(loss).all(), name
        ms = {name: [] for name in variants}
        last = {}
        for _ in range(a.rounds):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    loss = fn()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.steps)
                last[name] = float(loss)
        say(f"B = {B}: ms/step over {a.rounds} interleaved rounds of {a.steps} steps")
        for name in variants:
            say(f"  {name:<12} {spread(ms[name])}   loss/sample first {first[name] / B:.2f} -> last {last[name] / B:.2f}")
        med = {name: statistics.median(ms[name]) for name in variants}
        say(f"  torch eager / tdx eager = {med['torch eager'] / med['tdx eager']:.2f}x;  "
            f"tdx graph / tdx eager = {med['tdx graph'] / med['tdx eager']:.2f}x")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
