#!/usr/bin/env python3
"""Time of the sample-quality metrics (tiny_diffusion_amd/metrics.py) at N = 10 000 real x 10 000 generated features,
d = 20 (the VAE latent) and d = 784 (MNIST pixels): ``precision_recall`` (two radius and two membership launches
chains), ``kernel_distance`` over the full sets (three row-sum chains), ``FeatureStats.update`` of one 10 000-row batch
(three Gram calls on the transposed batch), the three reducing entries alone, and beside them the composition of
stock tensor ops a user would write without the kernels (``stock_precision_recall`` / ``stock_kid`` below:
``torch.cdist``, ``kthvalue``, comparisons, ``.any()``; ``a @ b.T`` and a cube), which stores every N x N pair matrix.

Every figure: ``--reps`` calls between two HIP events after two warm-up calls, library and stock alternating within a
round, the median over ``--rounds`` rounds and their min .. max.  The metric calls end in a copy to the host, so a
call is a whole evaluation.  FLOP are 2 N^2 d per pair product (4 per precision_recall, 3 per kernel_distance), and the
fraction is of the 157.3 TFLOP/s fp32 matrix peak.  Not under a profiler; one N; the machine is shared.

    python3 tools/gpu_metrics_latency.py [--n 10000] [--rounds 5] [--reps 5] [--out profiles/metrics_latency.txt]"""
import argparse
import os
import statistics
import sys

PEAK_TFLOPS = 157.3
K = 3


def stock_precision_recall(torch, x, y, k):
    def radii(f):
        d = torch.cdist(f, f)
        d.fill_diagonal_(float("inf"))
        return d.kthvalue(k, dim=1).values

    rx, ry = radii(x), radii(y)
    precision = (torch.cdist(y, x) <= rx[None, :]).any(dim=1).float().mean()
    recall = (torch.cdist(x, y) <= ry[None, :]).any(dim=1).float().mean()
    return float(precision), float(recall)


def stock_kid(torch, x, y):
    d, m, n = x.shape[1], x.shape[0], y.shape[0]
    kxx, kyy, kxy = ((a @ b.T / d + 1.0) ** 3 for a, b in ((x, x), (y, y), (x, y)))
    s_xx = kxx.double().sum() - kxx.diagonal().double().sum()
    s_yy = kyy.double().sum() - kyy.diagonal().double().sum()
    return float(s_xx / (m * (m - 1)) + s_yy / (n * (n - 1)) - 2.0 * kxy.double().sum() / (m * n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    from tiny_diffusion_amd import metrics as M

    N = a.n
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    def compare(what, products, d, ours, stock=None):
        fns = [ours] + ([stock] if stock else [])
        for fn in fns:
            fn()
            fn()
        torch.cuda.synchronize()
        ms = [[] for _ in fns]
        for _ in range(a.rounds):
            for i, fn in enumerate(fns):
                ms[i].append(timed(fn))
        med = [statistics.median(v) for v in ms]
        tf = products * 2.0 * N * N * d / (med[0] * 1e-3) / 1e12
        line = (f"d = {d:<4} {what:<34} {med[0]:9.3f} ms (min {min(ms[0]):.3f} .. max {max(ms[0]):.3f})")
        if products:
            line += f"; {products} x 2 N^2 d FLOP = {tf:6.2f} TFLOP/s = {100 * tf / PEAK_TFLOPS:5.1f} % of {PEAK_TFLOPS}"
        say(line)
        if stock:
            say(f"d = {d:<4} {'  stock tensor ops':<34} {med[1]:9.3f} ms (min {min(ms[1]):.3f} .. max {max(ms[1]):.3f}); "
                f"stock / library = {med[1] / med[0]:.2f}")

    g = torch.Generator().manual_seed(0)
    for d in (20, 784):
        x = torch.randn(N, d, generator=g).cuda()
        y = (torch.randn(N, d, generator=g) + 0.3).cuda()
        xc, yc = M.centre_on(x, y)
        r2 = M.pair_kth_dist2(xc, xc, K, True)
        pr, spr = M.precision_recall(x, y, K), stock_precision_recall(torch, x, y, K)
        kid, skid = M.kernel_distance(x, y).kid, stock_kid(torch, x, y)
        say(f"d = {d:<4} N = {N} x {N}, k = {K}: precision / recall {pr.precision:.4f} / {pr.recall:.4f} (stock "
            f"{spr[0]:.4f} / {spr[1]:.4f}), KID {kid:.6e} (stock {skid:.6e})")
        compare("precision_recall", 4, d, lambda: M.precision_recall(x, y, K),
                lambda: stock_precision_recall(torch, x, y, K))
        compare("kernel_distance (full sets)", 3, d, lambda: M.kernel_distance(x, y), lambda: stock_kid(torch, x, y))
        compare("FeatureStats.update (one batch)", 0, d, lambda: M.FeatureStats().update(x),
                lambda: (torch.cov(x.T.double()), x.double().mean(0)))
        compare("tdx_pair_kth_dist2 (self, k = 3)", 1, d, lambda: M.pair_kth_dist2(xc, xc, K, True))
        compare("tdx_pair_member", 1, d, lambda: M.pair_member(yc, xc, r2))
        compare("tdx_pair_poly_rowsum", 1, d, lambda: M.pair_poly_rowsum(x, y, 1.0 / d, 1.0))
        del x, y, xc, yc, r2
        torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    say(f"pair matrix in fp32: {4.0 * N * N / 1e9:.1f} GB at N = {N}, 10.0 GB at N = 50 000; the stock precision / recall "
        f"holds two at a time (cdist and its comparison) - device memory {total / 1e9:.0f} GB, so it stops near N = "
        f"{int((total / 8.0) ** 0.5):d} (arithmetic, not run); the library's scratch at N = 50 000, k = 3 is "
        f"{M.lib.tdx_pair_scratch_bytes(50000, 50000, K, 0) / 1e6:.1f} MB")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}; python3 tools/gpu_metrics_latency.py --n {N} --rounds {a.rounds} "
                    f"--reps {a.reps}; HIP events around {a.reps} calls, library and stock alternating per round, median "
                    f"and min .. max over {a.rounds} rounds; no profiler attached\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
