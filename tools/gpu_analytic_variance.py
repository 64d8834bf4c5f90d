#!/usr/bin/env python3
"""Cost and effect of the analytic (KL-optimal) reverse variance (``tiny_diffusion_amd/analytic.py``).

1. One estimation pass ``estimate_eps_moments`` at T = 1000, N = 256 on the MNIST UNet and on the latent MLP (T times
   Philox ``q_sample`` + inference forward + ``tdx_eps_sqnorm``, one copy to the host): a host clock around calls that
   end in a synchronise, after a warm-up pass on a short chain at the same batch.
2. ``tdx_eps_sqnorm`` alone against the stock composition ``(ex * x + eo * out).square().sum(1)`` on the same device
   tensors, at both sample sizes and for both row kinds: ``--reps`` launches between two HIP events, alternating within
   every round; the figures are the median over the rounds and their min .. max (the method of
   ``tools/gpu_bpd_latency.py``).
3. Bits per dimension of a briefly trained MNIST UNet under ``variance="beta"``, ``"posterior"`` and the analytic
   table, on chains of K = 10, 50 and 1000 timesteps (``round(i (T - 1) / (K - 1))``: both ends of the grid).  The raw
   IDX files are read from disk (nothing is downloaded); without them the script says so and measures 1 and 2 only.
   The last 512 images are held out of the training: 256 give the moments, 256 are evaluated.

    python3 tools/gpu_analytic_variance.py [--rounds 5] [--reps 2000] [--loops 3] [--data data/MNIST/raw]
                                           [--train-steps 2000] [--out profiles/analytic_variance.txt]"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T = 256, 1000
CHAINS = (10, 50, 1000)


def chain(K):
    return sorted({round(i * (T - 1) / (K - 1)) for i in range(K)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--data", default=os.path.join(ROOT, "data", "MNIST", "raw"))
    ap.add_argument("--train-steps", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    from tiny_diffusion_amd import diffusion as D
    from tiny_diffusion_amd import latent_diffusion as LD
    from tiny_diffusion_amd._lib import check, lib
    from tiny_diffusion_amd.analytic import eps_rows, estimate_eps_moments

    torch.manual_seed(0)
    fp = D.ForwardProcess(num_timesteps=T)
    g = torch.Generator().manual_seed(1)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    # ---- 1. the estimation pass
    unet = D.NoiseModel().cuda().eval()
    pixels = (torch.randint(0, 256, (N, 1, 28, 28), generator=g).float() * (2.0 / 255.0) - 1.0).cuda()
    mlp = LD.NoiseModel().cuda().eval()
    latents, labels = torch.randn(N, 20, generator=g).cuda(), torch.randint(0, 10, (N,), generator=g).cuda()
    for what, model, x0, y in (("MNIST UNet", unet, pixels, None), ("latent MLP", mlp, latents, labels)):
        estimate_eps_moments(model, D.ForwardProcess(num_timesteps=10), x0, y)      # plan, pack, first launches
        torch.cuda.synchronize()
        ms = []
        for i in range(a.loops):
            t0 = time.perf_counter()
            m = estimate_eps_moments(model, fp, x0, y, philox_seed=1 + i)    # returns CPU tensors: it has synchronised
            ms.append((time.perf_counter() - t0) * 1e3)
            assert torch.isfinite(m.g).all()
        med = statistics.median(ms)
        say(f"estimate_eps_moments, {what}, N = {N}, T = {T}, Philox noise: {med:.1f} ms per pass (min {min(ms):.1f} .. "
            f"max {max(ms):.1f} over {a.loops} passes) = {med / T * 1e3:.1f} us per timestep")

    # ---- 2. the kernel and the stock composition on the same tensors
    st = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps * 1e3

    t = torch.randint(0, T, (N,), generator=g).cuda()
    for per in (784, 20):
        x_t, out = torch.randn(N, per, generator=g).cuda(), torch.randn(N, per, generator=g).cuda()
        for prediction in ("eps", "v"):
            rows = eps_rows(fp, prediction).cuda()
            ex, eo = rows[t][:, 0:1].contiguous(), rows[t][:, 1:2].contiguous()
            sums = torch.empty(N, device="cuda")

            def kernel():
                check(lib.tdx_eps_sqnorm(x_t.data_ptr(), out.data_ptr(), t.data_ptr(), rows.data_ptr(), N, per,
                                         sums.data_ptr(), 1, st), "tdx_eps_sqnorm")

            def stock():
                return (ex * x_t + eo * out).square().sum(1)

            for fn in (kernel, stock):       # first launches
                fn()
            torch.cuda.synchronize()
            rel = ((sums.double() - stock().double()).abs() / stock().double()).max().item()
            us = {"kernel": [], "stock": []}
            for _ in range(a.rounds):
                us["kernel"].append(timed(kernel))
                us["stock"].append(timed(stock))
            mk, ms_ = statistics.median(us["kernel"]), statistics.median(us["stock"])
            tag = f"(N, per) = ({N}, {per}), {prediction} rows"
            say(f"{tag:<34} tdx_eps_sqnorm        {mk:8.2f} us per launch (min {min(us['kernel']):.2f} .. max "
                f"{max(us['kernel']):.2f} over {a.rounds} rounds of {a.reps}); 8 B/element = "
                f"{8.0 * N * per / (mk * 1e-6) / 1e9:.0f} GB/s")
            say(f"{tag:<34} stock tensor ops (5)  {ms_:8.2f} us per call   (min {min(us['stock']):.2f} .. max "
                f"{max(us['stock']):.2f}); stock / kernel = {ms_ / mk:.1f}; worst relative difference of the sums "
                f"{rel:.1e}")

    # ---- 3. bits per dimension on MNIST
    files = [os.path.join(a.data, n) for n in ("train-images-idx3-ubyte", "train-labels-idx1-ubyte")]
    where = os.path.relpath(a.data, ROOT)
    if not os.path.exists(files[0]):
        say(f"bits per dimension: NOT MEASURED - no raw MNIST IDX file (train-images-idx3-ubyte) under {where}, and "
            "nothing is downloaded")
    else:
        from distill_mnist import read_idx

        from tiny_diffusion_amd.data import DeviceImageDataset
        from tiny_diffusion_amd.train import TrainStep

        images = torch.from_numpy(read_idx(files[0]).copy())
        train, held = DeviceImageDataset(images[:-2 * N], "cuda"), DeviceImageDataset(images[-2 * N:], "cuda")
        model = D.NoiseModel().cuda().train()
        step = TrainStep(model, fp, lr=1e-3)
        done, batch = 0, 256
        while done < a.train_steps:
            for x in train.epoch(batch):
                if x.shape[0] < batch or done == a.train_steps:
                    break
                loss = step.step(x)
                done += 1
                if done % 500 == 0 or done == a.train_steps:
                    print(f"train step {done}: loss {loss.item():.5f}", flush=True)
        both = held.batch()
        fit, x_eval = both[:N].contiguous(), both[N:].contiguous()
        moments = estimate_eps_moments(model, fp, fit, philox_seed=11)
        say(f"MNIST UNet after {a.train_steps} steps at batch {batch}: g_t over {N} held-out images at t = 0, 99, 499, "
            f"999: " + ", ".join(f"{moments.g[i].item():.4f} +- {moments.stderr[i].item():.4f}" for i in (0, 99, 499, 999)))
        for K in CHAINS:
            cells = []
            for name, variance in (("beta", "beta"), ("posterior", "posterior"), ("analytic", moments)):
                r = D.bits_per_dim(model, fp, x_eval, philox_seed=12, variance=variance, timesteps=chain(K))
                cells.append(f"{name} {r.total_bpd.mean().item():.4f}")
                assert math.isfinite(r.total_bpd.mean().item())
            say(f"bits per dimension, {N} other held-out images, 256 bins, K = {K:4d} timesteps: " + "; ".join(cells))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}; python3 tools/gpu_analytic_variance.py --rounds {a.rounds} --reps "
                    f"{a.reps} --loops {a.loops} --train-steps {a.train_steps}; pass: host clock around synchronising "
                    f"calls; kernel / stock: HIP events around {a.reps} launches, alternating per round, median and "
                    f"min .. max\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
