#!/usr/bin/env python3
"""Where a workgroup of the Winograd forward kernel (conv3x3_wino_kernel) spends its time: every workgroup of ONE launch
stamps s_memrealtime (10 ns) at entry, after requesting the first stage, when it has landed, after the main loop and
after the epilogue (diagnostic knob conv_stamp = 3; no product launch stamps).  Forward with BatchNorm statistics at
B = 256 and the plain input gradient, in isolation, chip warmed by ~0.5 s of the same launch.
usage: gpu_wino_phases.py [B]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tiny_diffusion_amd._lib import lib, check, tuned  # noqa: E402

LAYERS = [("enc1.0", 64, 128, 28), ("enc1.3", 128, 128, 28), ("enc2.0", 128, 256, 14), ("enc2.3", 256, 256, 14),
          ("enc3.0", 256, 512, 7), ("enc3.3", 512, 512, 7), ("bottleneck", 512, 512, 4), ("dec3.0", 1024, 256, 8),
          ("dec3.3", 256, 256, 8), ("dec2.0", 512, 128, 16), ("dec2.3", 128, 128, 16), ("dec1.0", 256, 64, 32),
          ("dec1.3", 64, 64, 32)]
B = int(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else 256
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
stamps = torch.zeros(8 * 65536, dtype=torch.int64, device="cuda")
lib.tdx_diag_set_buffer(stamps.data_ptr(), stamps.numel() * stamps.element_size())


def med(v):
    return float(v.double().median()) / 100.0   # 10-ns ticks -> us


def probe(fn, nst):
    check(lib.tdx_tune_set(b"conv_stamp", 0))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / 20 * 1e3
    stamps.zero_()
    with tuned(conv_stamp=3):
        fn()
        torch.cuda.synchronize()
    s = stamps.cpu().view(-1, 8)
    s = s[s[:, 4] > 0]
    t00 = int(s[:, 0].min())
    cu = (s[:, 6] >> 8) & 0xff | (s[:, 7] & 0xf) << 8   # HW_ID bits 8-15 (CU, SH, SE ids) and the XCC id
    per_cu = torch.bincount(torch.unique(cu, return_inverse=True)[1])
    return {"us": us, "wgs": int(s.shape[0]), "cus": int(per_cu.numel()), "wg_per_cu_max": int(per_cu.max()),
            "prologue": med(s[:, 1] - s[:, 0]), "first_load": med(s[:, 2] - s[:, 1]), "loop": med(s[:, 3] - s[:, 2]),
            "per_stage": med(s[:, 3] - s[:, 2]) / nst, "clock_mhz": float((s[:, 5].double() / (s[:, 3] - s[:, 2]).double()).median() * 100),
            "epilogue": med(s[:, 4] - s[:, 3]), "wg": med(s[:, 4] - s[:, 0]),
            "last_entry": (int(s[:, 0].max()) - t00) / 100.0, "last_end": (int(s[:, 4].max()) - t00) / 100.0}


print(f"B = {B}; us. columns: launch (events) | workgroups, CUs seen, most workgroups on one CU | per workgroup (medians): "
      "prologue, first stage's latency, main loop (per stage), epilogue, whole | entry of the last workgroup, end of the last")
for name, cin, cout, hw in LAYERS:
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, hw, hw, cin, device="cuda", generator=g)
    dy = torch.randn(B, hw, hw, cout, device="cuda", generator=g)
    w = torch.randn(cout, cin, 3, 3, device="cuda", generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, device="cuda", generator=g)
    uf, ug = torch.empty(cout * 16 * cin, device="cuda"), torch.empty(cout * 16 * cin, device="cuda")
    check(lib.tdx_pack_conv3x3_wino(w.data_ptr(), uf.data_ptr(), ug.data_ptr(), cout, cin, st()))
    out = torch.empty(B, hw, hw, cout, device="cuda")
    gin = torch.empty(B, hw, hw, cin, device="cuda")
    stats = torch.empty(lib.tdx_conv3x3_wino_stat_tiles(B, hw, hw) * 2 * max(cin, cout), device="cuda")

    def w_f():
        check(lib.tdx_conv3x3_fwd_wino(x.data_ptr(), uf.data_ptr(), b.data_ptr(), out.data_ptr(), B, hw, hw, cin, cout, 4, None,
                                       None, stats.data_ptr(), st()))

    def w_g():
        check(lib.tdx_conv3x3_fwd_wino(dy.data_ptr(), ug.data_ptr(), None, gin.data_ptr(), B, hw, hw, cout, cin, 0, None, None,
                                       None, st()))

    sp = lib.tdx_conv3x3_wgrad_wino_splits(B, hw, hw, cin, cout)
    slabs = torch.empty(sp * cout * 9 * cin, device="cuda")

    def w_w():
        check(lib.tdx_conv3x3_wgrad_wino(x.data_ptr(), dy.data_ptr(), slabs.data_ptr(), B, hw, hw, cin, cout, st()))

    nt = B * ((hw + 1) // 2) ** 2
    chunk = -(-(-(-nt // sp)) // 8) * 8
    roles = (("wgrad", w_w, max(chunk // 8, 4)),) if "--wgrad" in sys.argv else (("fwd", w_f, cin // 8), ("dgrad", w_g, cout // 8))
    for role, fn, nst in roles:
        r = probe(fn, nst)
        print(f"{name:10s} {role:5s} {cin:4d}->{cout:4d} @{hw:2d} | {r['us']:7.1f} | {r['wgs']:5d} {r['cus']:3d} {r['wg_per_cu_max']:2d} | "
              f"{r['prologue']:5.2f} {r['first_load']:5.2f} {r['loop']:7.2f} ({r['per_stage']:5.3f} x {nst:3d}, {r['clock_mhz']:4.0f} MHz) "
              f"{r['epilogue']:6.2f} {r['wg']:7.2f} | {r['last_entry']:7.1f} {r['last_end']:7.1f}", flush=True)
