#!/usr/bin/env python3
"""Time of the variational-bound evaluation (``bits_per_dim``) on the MNIST UNet at B = 256, T = 1000: the whole loop
(T times q_sample + inference forward + ``tdx_vlb_terms``, the prior launch, one copy to the host), ``tdx_vlb_terms``
alone per step, and beside it the same three sums taken by the composition of stock tensor ops a user would write
without the kernel (``stock_terms`` below: x0 prediction, clamp, erf-based CDFs, log, sum - fp32, so its decoder sum is
also the inaccurate one; it is here for its time only).

The loop is timed with a host clock around calls that end in a synchronise (the result is copied to the host), after
a warm-up loop on a short chain at the same batch.  The kernel and the composition run on the same device tensors,
``--reps`` launches between two HIP events, alternating within every round; the figures are the median over the rounds
and their min .. max.  Two rows of timesteps: t = 0 for every sample (the decoder row: an erfc pair and a log per
element) and t >= 1 (the KL rows: the two sums of squares only; the composition still evaluates all of it, as a
per-sample ``t`` forces it to).

    python3 tools/gpu_bpd_latency.py [--rounds 5] [--reps 2000] [--loops 3] [--out profiles/bpd_latency.txt]"""
import argparse
import math
import os
import statistics
import sys
import time

B, T, BINS = 256, 1000, 256
RS2 = 0.70710678118654752


def stock_terms(torch, x0, x_t, out, noise, row, lo_edge, hi_edge, half):
    """(sum e^2, sum d^2, sum -log P) per sample from stock tensor ops, for an eps-model: 32 tensor ops."""
    p, q, s = row[:, 0:1], row[:, 1:2], row[:, 4:5]
    d = x0 - (p * x_t + q * out).clamp(-1.0, 1.0)
    e = noise - out
    cdf_a = 0.5 * (1.0 + torch.erf((d + half) * s * RS2))
    cdf_b = 0.5 * (1.0 + torch.erf((d - half) * s * RS2))
    P = torch.where(x0 < lo_edge, cdf_a, torch.where(x0 > hi_edge, 1.0 - cdf_b, cdf_a - cdf_b))
    return (e * e).sum(1), (d * d).sum(1), -torch.log(P.clamp(min=1e-12)).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    from tiny_diffusion_amd import diffusion as D
    from tiny_diffusion_amd._lib import check, lib
    from tiny_diffusion_amd.likelihood import vlb_tables

    torch.manual_seed(0)
    fp = D.ForwardProcess(num_timesteps=T)
    model = D.NoiseModel().cuda().eval()
    g = torch.Generator().manual_seed(1)
    x0 = (torch.randint(0, 256, (B, 1, 28, 28), generator=g).float() * (2.0 / 255.0) - 1.0).cuda()
    per = x0[0].numel()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    # ---- the whole loop
    D.bits_per_dim(model, D.ForwardProcess(num_timesteps=10), x0, philox_seed=1)    # plan, pack, first launches
    torch.cuda.synchronize()
    loop_ms = []
    for i in range(a.loops):
        t0 = time.perf_counter()
        r = D.bits_per_dim(model, fp, x0, philox_seed=1 + i)     # returns CPU tensors: the call has synchronised
        loop_ms.append((time.perf_counter() - t0) * 1e3)
        assert torch.isfinite(r.total_bpd).all()
    med = statistics.median(loop_ms)
    say(f"bits_per_dim, MNIST UNet, B = {B}, T = {T}, 256 bins, Philox noise: {med:.1f} ms per loop "
        f"(min {min(loop_ms):.1f} .. max {max(loop_ms):.1f} over {a.loops} loops) = {med / T * 1e3:.1f} us per step")

    # ---- the kernel and the stock composition on the same tensors
    rows = vlb_tables(fp, "eps", "beta").rows(True, device="cuda")
    flat = x0.reshape(B, per).contiguous()
    noise = torch.randn(B, per, generator=g).cuda()
    terms = torch.empty(B, 3, device="cuda")
    half = 2.0 / (2.0 * (BINS - 1))
    st = torch.cuda.current_stream().cuda_stream
    for what, t in (("t = 0 (decoder row)", torch.zeros(B, dtype=torch.int64)),
                    ("t >= 1 (KL rows)", torch.randint(1, T, (B,), generator=g))):
        t = t.cuda()
        x_t, _ = fp.q_sample("cuda", flat, t, noise=noise)
        r64 = rows[t].double()
        out = ((flat.double() + 0.02 * torch.randn(B, per, generator=g).cuda().double() - r64[:, 0:1] * x_t.double())
               / r64[:, 1:2]).float().contiguous()          # an x0 prediction 2 sigma_0 off, as a trained model's at t = 0
        row = rows[t].contiguous()

        def kernel():
            check(lib.tdx_vlb_terms(flat.data_ptr(), x_t.data_ptr(), out.data_ptr(), noise.data_ptr(), t.data_ptr(),
                                    rows.data_ptr(), B, per, -1.0, 1.0, -1.0, 1.0, BINS, terms.data_ptr(), 3, st),
                  "tdx_vlb_terms")

        def stock():
            return stock_terms(torch, flat, x_t, out, noise, row, -1.0 + half, 1.0 - half, half)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.reps * 1e3

        for fn in (kernel, stock):       # first launches
            fn()
        torch.cuda.synchronize()
        k_sums, s_sums = terms.clone(), torch.stack(stock(), dim=1)
        us = {"kernel": [], "stock": []}
        for _ in range(a.rounds):
            us["kernel"].append(timed(kernel))
            us["stock"].append(timed(stock))
        mk, ms = statistics.median(us["kernel"]), statistics.median(us["stock"])
        gbs = 16.0 * B * per / (mk * 1e-6) / 1e9
        say(f"{what:<20} tdx_vlb_terms          {mk:8.2f} us per launch (min {min(us['kernel']):.2f} .. max "
            f"{max(us['kernel']):.2f} over {a.rounds} rounds of {a.reps}); 16 B/element = {gbs:.0f} GB/s")
        say(f"{what:<20} stock tensor ops (32)  {ms:8.2f} us per call   (min {min(us['stock']):.2f} .. max "
            f"{max(us['stock']):.2f}); stock / kernel = {ms / mk:.1f}")
        slots = 3 if bool((k_sums[:, 2] != 0).all()) else 2     # no decoder term on the KL rows: the kernel writes 0
        rel = ((k_sums.double() - s_sums.double()).abs() / s_sums.double().abs().clamp(min=1e-30)).max(dim=0).values
        say(f"{what:<20} kernel vs stock sums, worst relative difference per slot (e^2, d^2, -log P)[:{slots}]: "
            + ", ".join(f"{v:.1e}" for v in rel.tolist()[:slots]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}; python3 tools/gpu_bpd_latency.py --rounds {a.rounds} --reps {a.reps} "
                    f"--loops {a.loops}; loop: host clock around synchronising calls; kernel / stock: HIP events around "
                    f"{a.reps} launches, alternating per round, median and min .. max; (B, per) = ({B}, {per})\n")
            f.write("\n".join(lines) + "\n")
    assert math.isfinite(med)


if __name__ == "__main__":
    main()
