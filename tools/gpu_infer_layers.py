#!/usr/bin/env python3
"""Every 3x3 convolution of one reverse step (diffusion.py:254-276) in isolation at the sampling batch sizes: the
round-3 path (variant 3 + split-K at ~512 workgroups, K-contiguous pack) against the inference convolution of round 4
(conv3x3_ring64_kernel: LDS-DMA ring, tile-major pack, cost-model split), with a sweep of the split count around the
plan's choice.  usage: gpu_infer_layers.py [n ...] [--sweep] [--cus C]     (times: us per launch incl. its reduction)"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tiny_diffusion_amd._lib import lib, check, tuned  # noqa: E402

LAYERS = [("enc1.0", 64, 128, 28), ("enc1.3", 128, 128, 28), ("enc2.0", 128, 256, 14), ("enc2.3", 256, 256, 14),
          ("enc3.0", 256, 512, 7), ("enc3.3", 512, 512, 7), ("bottleneck", 512, 512, 4), ("dec3.0", 1024, 256, 8),
          ("dec3.3", 256, 256, 8), ("dec2.0", 512, 128, 16), ("dec2.3", 128, 128, 16), ("dec1.0", 256, 64, 32),
          ("dec1.3", 64, 64, 32)]
PEAK = 157.3e12
args = [a for a in sys.argv[1:] if not a.startswith("--")]
ns = [int(a) for a in args] or [16, 64]
sweep = "--sweep" in sys.argv
if "--cus" in sys.argv:
    check(lib.tdx_tune_set(b"infer_cus", int(sys.argv[sys.argv.index("--cus") + 1])))
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731


def timed(fn, reps=60):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(3):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    return best


for n in ns:
    tot_old = tot_new = tot_peak = 0.0
    print(f"n = {n}: layer, M, us at the fp32 matrix peak | round-3 path | ring kernel (splits by plan) | fraction of peak")
    for name, cin, cout, hw in LAYERS:
        M = n * hw * hw
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(n, hw, hw, cin, device="cuda", generator=g)
        w = torch.randn(cout, cin, 3, 3, device="cuda", generator=g) * (2.0 / (9 * cin)) ** 0.5
        b = torch.randn(cout, device="cuda", generator=g)
        sc, sh = torch.rand(cout, device="cuda", generator=g) + 0.5, torch.randn(cout, device="cuda", generator=g)
        wf = torch.empty(cout * 9 * cin, device="cuda")
        wt = torch.empty(cout * 9 * cin, device="cuda")
        check(lib.tdx_pack_conv3x3(w.data_ptr(), wf.data_ptr(), None, cout, cin, st()))
        check(lib.tdx_pack_conv3x3_tiled(w.data_ptr(), wt.data_ptr(), cout, cin, st()))
        out = torch.empty(n, hw, hw, cout, device="cuda")
        nk = 9 * cin // 32
        scratch = torch.empty(max(nk // 6, 1) * M * cout, device="cuda")

        def old():
            check(lib.tdx_conv3x3_fwd_splitk(x.data_ptr(), wf.data_ptr(), b.data_ptr(), out.data_ptr(), n, hw, hw, cin, cout,
                                             2, None, None, sc.data_ptr(), sh.data_ptr(), scratch.data_ptr(),
                                             scratch.numel(), st()))

        def new():
            check(lib.tdx_conv3x3_fwd_infer(x.data_ptr(), wt.data_ptr(), b.data_ptr(), out.data_ptr(), n, hw, hw, cin, cout,
                                            sc.data_ptr(), sh.data_ptr(), scratch.data_ptr(), scratch.numel(), st()))

        uf = torch.empty(cout * 16 * cin, device="cuda")
        check(lib.tdx_pack_conv3x3_wino(w.data_ptr(), uf.data_ptr(), None, cout, cin, st()))

        def wino():
            check(lib.tdx_conv3x3_fwd_wino_infer(x.data_ptr(), uf.data_ptr(), b.data_ptr(), out.data_ptr(), n, hw, hw, cin, cout,
                                                 sc.data_ptr(), sh.data_ptr(), scratch.data_ptr(), scratch.numel(), st()))

        t_peak = 2.0 * M * 9 * cin * cout / PEAK * 1e6
        t_old, t_new = timed(old), timed(new)
        t_w = timed(wino) if lib.tdx_conv3x3_wino_ok(n, hw, hw, cin, cout) else float("nan")
        need = lib.tdx_conv3x3_infer_scratch_floats(n, hw, hw, cin, cout)
        splits = need // (M * cout) if need else 1
        line = (f"  {name:11s} M {M:6d}  peak {t_peak:6.1f} | {t_old:6.1f} | {t_new:6.1f} (x{splits}) | "
                f"{t_peak / t_old:.2f} -> {t_peak / t_new:.2f} | winograd {t_w:6.1f} ({t_peak / t_w:.2f})")
        tot_w = globals().get("tot_w", 0.0) + t_w; globals()["tot_w"] = tot_w
        if "--ablate" in sys.argv:   # what a launch costs without one of its parts (wrong results)
            res = []
            for bits, label in ((1, "no barrier"), (4, "no DMA"), (16, "no MFMA"), (32, "no LDS reads"), (20, "no DMA+MFMA"),
                                (52, "barrier only"), (53, "nothing")):
                with tuned(conv_dbg=bits):
                    res.append((label, timed(new)))
            line += "   ablate " + ", ".join(f"{lb} {t:.1f}" for lb, t in res)
        if sweep:
            res = []
            for sp in [1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 24]:
                if sp > max(nk // 6, 1):
                    break
                with tuned(infer_splits=sp):
                    if sp == 1:
                        def f1():
                            check(lib.tdx_conv3x3_fwd_infer(x.data_ptr(), wt.data_ptr(), b.data_ptr(), out.data_ptr(), n, hw,
                                                            hw, cin, cout, sc.data_ptr(), sh.data_ptr(), None, 0, st()))
                        res.append((sp, timed(f1)))
                    else:
                        res.append((sp, timed(new)))
            line += "   sweep " + " ".join(f"{sp}:{t:.1f}" for sp, t in res)
        print(line, flush=True)
        tot_old += t_old; tot_new += t_new; tot_peak += t_peak
    print(f"  sum: peak {tot_peak:.1f} us | round 3 {tot_old:.1f} | ring {tot_new:.1f} | winograd {globals().get('tot_w', 0.0):.1f}")
    globals()["tot_w"] = 0.0
