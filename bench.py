#!/usr/bin/env python3
"""Headline benchmark of the tiny-diffusion DDPM hot path on MI355X.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]   (N > 1: starts its own N ranks)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one full training step of the unconditional MNIST 28x28 UNet in fp32 on a
per-GPU minibatch of 256 synthetic MNIST-shaped images (BASELINE.json configs[1];
weak scaling for N > 1): t ~ U, q_sample, UNet forward (train-mode BatchNorm), MSE,
backward of every parameter, gradient all-reduce (N > 1), Adam.  Rank 0 prints ONE
JSON line.  `value` = images/s of the whole job, `ms_per_step` = one timed step.

A plain run sets up, warms up, times the K steps and prints the line; nothing else.
--dump-outputs DIR then writes what the last timed step produced (see dump_outputs).
--full adds everything else, outside the timed region: the first-step parity check
against the CPU oracle (`parity_check`), for N > 1 the replica check and the step
without the gradient exchange (`weak_scaling`), and - unless --no-extras - `roofline`
= fp32-MFMA fraction of the 3x3 convolution kernels (>= 99.9 % of the FLOPs) timed
live with HIP events; `cpu_baseline` = the CPU oracle (a port of the reference path,
checked against the reference's own outputs) timed on this host; `sample` = wall-clock
of the reference's 1000-step reverse loop (graph-replayed) at n = 16 and n = 64; the
HBM-bound kernels, the bf16 mode and the LAION / latent legs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PER_GPU_BATCH = 256
FWD_FLOP_PER_IMAGE = 2_250_805_760          # SURVEY.md 8(d), measured on the reference
TRAIN_FLOP_PER_IMAGE = 3 * FWD_FLOP_PER_IMAGE
PEAK_F32_MFMA_TFLOPS = 157.3                # MI355X_MICROARCH.md (dense fp32 matrix)
PEAK_HBM_TBPS = 8.0                         # MI355X_MICROARCH.md (HBM3E spec; ~6.3 achievable)
PROFILE_TAG = "r04"                         # profiles/<tag>_* hold the rocprofv3 evidence of this round

# (cin, cout, H) of the 13 conv/BN units, diffusion.py:32-95
# (cin, cout, hw, in_bn): in_bn = the unit reads the previous unit's pre-BN tensor and applies
# relu(y*scale+shift) on load (the second conv of every stage) - same flags as tdx_unet_forward
UNITS = [(64, 128, 28, 0), (128, 128, 28, 1), (128, 256, 14, 0), (256, 256, 14, 1), (256, 512, 7, 0),
         (512, 512, 7, 1), (512, 512, 4, 0), (1024, 256, 8, 0), (256, 256, 8, 1), (512, 128, 16, 0),
         (128, 128, 16, 1), (256, 64, 32, 0), (64, 64, 32, 1)]


def conv_roofline(B: int, reps: int = 5):
    """Time every MFMA conv launch of one training step (13 x {fwd, dgrad, wgrad}) in
    isolation with HIP events on the launch stream, with the flags the training step uses
    (train-mode statistics epilogue; the six units fed by another unit read its materialised
    relu(bn(.)) tensor, or - with TDX_TUNE=materialize=0 - apply BN+ReLU on load);
    FLOPs are algorithmic (2*M*9*cin*cout)."""
    from tiny_diffusion_amd._lib import lib, check

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    tot_flop = tot_ms = tot_exe = 0.0
    n_launch = 0
    bn_on_load = "materialize=0" in os.environ.get("TDX_TUNE", "")
    for cin, cout, H, in_bn in UNITS:
        in_bn = in_bn if bn_on_load else 0
        M = B * H * H
        flop = 2.0 * M * 9 * cin * cout
        x = torch.randn(M * cin, device=dev)
        dy = torch.randn(M * cout, device=dev)
        wf = torch.randn(cout * 9 * cin, device=dev) * 0.02
        out = torch.empty(M * cout, device=dev)
        gin = torch.empty(M * cin, device=dev)
        tiles = lib.tdx_conv3x3_stat_tiles(B, H, H, cin, cout)
        stats = torch.empty(tiles * 2 * cout, device=dev)
        splits = lib.tdx_conv3x3_wgrad_splits(B, H, H, cin, cout)
        slabs = torch.empty(splits * cout * 9 * cin, device=dev)
        dw = torch.empty(cout * cin * 9, device=dev)
        bias = torch.zeros(cout, device=dev)
        isc = torch.rand(cin, device=dev) + 0.5
        ish = torch.randn(cin, device=dev) * 0.1
        sc_p, sh_p = (isc.data_ptr(), ish.data_ptr()) if in_bn else (None, None)

        # raw-input launches go through the entry point the training step uses (tdx_conv3x3_fwd_train: shapes
        # whose tiles do not fill whole rounds of workgroup slots K-slice the remainder and add one small
        # reduction launch, which is inside the timed region)
        need = max(lib.tdx_conv3x3_train_scratch_floats(B, H, H, cin, cout),
                   lib.tdx_conv3x3_train_scratch_floats(B, H, H, cout, cin))
        scratch = torch.empty(max(need, 1), device=dev)

        wino_f = bool(lib.tdx_conv3x3_train_algo(B, H, H, cin, cout, 0)) and not in_bn
        wino_d = bool(lib.tdx_conv3x3_train_algo(B, H, H, cin, cout, 1))
        uf = ug = wino_stats = None
        if wino_f or wino_d:   # transformed-weight packs (any finite values: timing only)
            uf = torch.randn(cout * 16 * cin, device=dev) * 0.02
            ug = torch.randn(cout * 16 * cin, device=dev) * 0.02
            wino_stats = torch.empty(lib.tdx_conv3x3_wino_stat_tiles(B, H, H) * 2 * cout, device=dev)

        def fwd():
            if wino_f:   # what the step launches for this unit (tdx_conv3x3_train_algo): Winograd F(2x2,3x3)
                check(lib.tdx_conv3x3_fwd_wino(x.data_ptr(), uf.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, H, cin,
                                               cout, 4, None, None, wino_stats.data_ptr(), st))
                return
            if in_bn:
                check(lib.tdx_conv3x3_fwd(x.data_ptr(), wf.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, H, cin,
                                          cout, 4 | in_bn, sc_p, sh_p, None, None, stats.data_ptr(), st))
            else:
                check(lib.tdx_conv3x3_fwd_train(x.data_ptr(), wf.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, H,
                                                cin, cout, 4, stats.data_ptr(), scratch.data_ptr(), need, st))

        def dgrad():
            if wino_d:
                check(lib.tdx_conv3x3_fwd_wino(dy.data_ptr(), ug.data_ptr(), None, gin.data_ptr(), B, H, H, cout, cin, 0,
                                               None, None, None, st))
                return
            check(lib.tdx_conv3x3_fwd_train(dy.data_ptr(), wf.data_ptr(), None, gin.data_ptr(), B, H, H, cout, cin, 0,
                                            None, scratch.data_ptr(), need, st))

        wino_w = bool(lib.tdx_conv3x3_train_algo(B, H, H, cin, cout, 2)) and not in_bn
        wsplits = lib.tdx_conv3x3_wgrad_wino_splits(B, H, H, cin, cout) if wino_w else 0
        if wsplits > splits:
            slabs = torch.empty(wsplits * cout * 9 * cin, device=dev)

        def wgrad():
            # GEMM into the split slabs AND their fixed-order reduction into the OIHW gradient: "wgrad" means
            # gradient-in-memory (round 2 timed the GEMM alone)
            if wino_w:   # Winograd F(3x3,2x2), same slab format and reduction
                check(lib.tdx_conv3x3_wgrad_wino(x.data_ptr(), dy.data_ptr(), slabs.data_ptr(), B, H, H, cin, cout, st))
                check(lib.tdx_conv3x3_wgrad_reduce(slabs.data_ptr(), dw.data_ptr(), wsplits, cout, cin, st))
                return
            check(lib.tdx_conv3x3_wgrad(x.data_ptr(), dy.data_ptr(), slabs.data_ptr(), B, H, H, cin, cout, in_bn,
                                        sc_p, sh_p, st))
            check(lib.tdx_conv3x3_wgrad_reduce(slabs.data_ptr(), dw.data_ptr(), splits, cout, cin, st))

        for name, fn in (("fwd", fwd), ("dgrad", dgrad), ("wgrad", wgrad)):
            fn(); fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
            wino = (name == "fwd" and wino_f) or (name == "dgrad" and wino_d) or (name == "wgrad" and wino_w)
            # multiplications actually issued to the matrix pipe: Winograd F(2x2,3x3) does 16 per 2x2 outputs where the
            # direct form does 36 (on maps with odd sides its tiles cover (H+1)/2*2 pixels per side)
            He = (H + 1) // 2 * 2
            exe = flop * (16.0 / 36.0) * (He * He) / (H * H) if wino else flop
            rows.append({"cin": cin, "cout": cout, "hw": H, "in_bn": in_bn, "role": name,
                         "algo": ("winograd_f3x3_2x2" if name == "wgrad" else "winograd_f2x2_3x3") if wino else "direct",
                         "ms": round(ms, 4),
                         "tflops": round(flop / ms / 1e9, 1), "executed_tflops": round(exe / ms / 1e9, 1)})
            tot_flop += flop
            tot_exe += exe
            tot_ms += ms
            n_launch += 1
    return rows, tot_flop, tot_ms, n_launch, tot_exe


def _lib_source_hash():
    try:
        from tiny_diffusion_amd import _build
        return _build.source_hash()
    except Exception:
        return None


def _committed(name: str):
    """A committed profile of THIS round (profiles/<tag>_<name>.json) plus whether it was taken on the very
    sources the loaded library was built from (`src_sha256`, stamped at collection time by
    tools/collect_evidence.sh): a profile of another build is reported as such, never as a measurement."""
    path = os.path.join(ROOT, "profiles", f"{PROFILE_TAG}_{name}.json")
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        return None
    d["source"] = f"profiles/{PROFILE_TAG}_{name}.json"
    here = _lib_source_hash()
    d["same_build_as_this_run"] = bool(here and d.get("src_sha256") == here)
    return d


def pmc_traffic():
    """HBM bytes per conv launch from the committed PMC passes over this same leg (bench.py cannot collect
    counters itself: rocprofv3 has to wrap the process): tools/pmc_traffic.py -> profiles/<tag>_pmc_hbm_traffic.json."""
    return _committed("pmc_hbm_traffic")


def roofline_block(B: int, steady: bool = False):
    rows, flop, ms, nl, exe = conv_roofline(B)
    ach = flop / ms / 1e9
    pmc = pmc_traffic()
    # algorithmic minimum HBM bytes of the 39 launches: read both operands once, write the result once
    alg = 0.0
    for cin, cout, H, _ in UNITS:
        M = B * H * H
        alg += 3 * 4.0 * (M * cin + M * cout + 9 * cin * cout)
    return {
        "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
        "frac": round(ach / PEAK_F32_MFMA_TFLOPS, 4),
        # PMC counters cannot be collected from inside this process; the figure comes from the committed passes over
        # this same leg and is reported as `traffic` only when they were taken on the build that is running now
        "traffic": round(pmc["traffic_mb_per_launch"] * 1e6) if pmc and pmc["same_build_as_this_run"] else None,
        "traffic_note": "HBM bytes per launch, rocprofv3 PMC 2*FETCH_SIZE+WRITE_SIZE, separate passes over this leg, "
                        "from committed_profile.pmc_hbm_traffic when that profile is of this build (else null); "
                        "algorithmic minimum in algorithmic_bytes_per_launch",
        "committed_profile": {"pmc_hbm_traffic": pmc},
        "algorithmic_bytes_per_launch": round(alg / nl),
        # `achieved` / `frac` are ALGORITHMIC (direct-convolution) FLOPs over time, as SURVEY.md 8(d) defines them; since
        # round 4 the launches that fill the chip run Winograd (F(2x2,3x3) forward / input gradient, F(3x3,2x2) weight
        # gradient: 16 multiplications where the direct form does 36), so a launch's algorithmic rate may exceed the pipe's 157.3 TFLOP/s.  What the
        # matrix pipe itself executes, and how busy that keeps it, is `executed`:
        "executed": {"tflops": round(exe / ms / 1e9, 2), "frac_of_peak": round(exe / ms / 1e9 / PEAK_F32_MFMA_TFLOPS, 4),
                     "gflop_per_step": round(exe / 1e9, 1),
                     "note": "multiplications issued to the fp32 MFMA (Winograd launches: 16/36 of the algorithmic count, "
                             "x64/49 on the 7x7 maps whose 2x2 tiles overhang)"},
        "kernel": "conv3x3_wino_kernel (Winograd F(2x2,3x3): fwd, dgrad) and conv3x3_wgrad_wino_kernel (F(3x3,2x2): wgrad) for "
                  "the launches tdx_conv3x3_train_algo selects, conv3x3_igemm_dma_kernel / conv3x3_wgrad_dma_kernel for the "
                  "others, + wgrad_reduce_kernel (wgrad rows = GEMM into the split slabs AND their reduction: gradient in memory)",
        "launches_per_step": nl, "conv_ms_per_step": round(ms, 3), "avg_launch_us": round(ms / nl * 1e3, 1),
        "algorithmic_gflop_per_step": round(flop / 1e9, 1),
        "per_launch": rows,
        **({"steady_state": steady_state(B)} if steady else {}),
    }


def steady_state(B: int):
    """The same 39 launches timed over 40 back-to-back repetitions each instead of 5.  `achieved` above is the
    figure the training step sees (a launch's first handful of repetitions); the big 28x28 layers get 14-17 %
    faster over ~60 repetitions of the SAME launch, which this second figure includes."""
    rows, flop, ms, _, _ = conv_roofline(B, reps=40)
    return {"tflops": round(flop / ms / 1e9, 2), "frac": round(flop / ms / 1e9 / PEAK_F32_MFMA_TFLOPS, 4),
            "reps_per_launch": 40}


def usable_cores() -> int:
    """CPU threads this process may actually use: the affinity mask and the cgroup quota, not
    os.cpu_count() (the GPU box shows every core of the host but gives a job the share of its GPU -
    16 threads per GPU on this pool; oversubscribing that 10x makes a torch CPU step crawl).
    TDX_BENCH_THREADS overrides."""
    if os.environ.get("TDX_BENCH_THREADS"):
        return max(1, int(os.environ["TDX_BENCH_THREADS"]))
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    try:
        quota = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        period = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if quota > 0:
            n = min(n, max(1, quota // period))
    except (OSError, ValueError):
        pass
    return min(n, 16 * max(1, torch.cuda.device_count()))   # the pool's CPU share per GPU


def note(msg: str):
    """Progress on stderr (the JSON line on stdout stays the only stdout output)."""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(batch: int = 64, steps: int = 24, warm: int = 2, sample_steps: int = 40):
    """the CPU oracle (port of diffusion.py:214-236 and 254-276, checked against
    the reference's own outputs) on ALL host cores of this box, configs[0] (unconditional, B = 64,
    fp32): 2 warm-up + 24 timed train steps (q_sample + fwd + MSE + bwd + Adam) and 2 + 40 timed
    reverse steps (eval forward + p_sample), the latter extrapolated x1000/40 to a chain - about 15 s of CPU
    work on 16 threads.  A bounded sample, reported beside the GPU number, never the target."""
    from oracle import ref_cpu as R
    from oracle.weights import make_state_dict

    threads = usable_cores()
    torch.set_num_threads(threads)
    sd = make_state_dict(0, False)
    sched = R.Schedule()
    g = torch.Generator().manual_seed(0)
    x0 = torch.rand(batch, 1, 28, 28, generator=g) * 2 - 1
    state = {}
    params = {k: v.clone() for k, v in sd.items() if "running" not in k and "num_batches" not in k}
    times = []
    for i in range(warm + steps):
        t0 = time.perf_counter()
        t = torch.randint(0, 1000, (batch,), generator=g)
        noise = torch.randn(x0.shape, generator=g)
        x_t = R.q_sample(sched, x0, t, noise)
        full = dict(sd); full.update(params)
        loss, _, grads, bufs = R.train_step_grads(full, x_t, t, noise)
        R.adam_step(params, grads, state)
        sd.update(bufs)
        times.append(time.perf_counter() - t0)
    dt = sum(times[warm:]) / steps
    # reverse steps (diffusion.py:259-274) at n = 64, eval-mode forward
    full = dict(sd); full.update(params)
    p, b = R.split_state(full)
    x = torch.randn(batch, 1, 28, 28, generator=g)
    stimes = []
    with torch.no_grad():
        for i in range(warm + sample_steps):
            t0 = time.perf_counter()
            tt = 999 - i
            eps = R.unet_forward(p, b, x, torch.full((batch,), tt, dtype=torch.long), training=False)
            x = R.p_sample_step(sched, x, eps, tt, torch.randn(x.shape, generator=g))
            stimes.append(time.perf_counter() - t0)
    sdt = sum(stimes[warm:]) / sample_steps
    return {"value": round(batch / dt, 2), "unit": "images/s", "cores": threads, "kind": "port",
            "cpu_model": _cpu_model(), "host_cpu_count": os.cpu_count(),
            "sample": f"{steps} train steps at B={batch} (configs[0]) after {warm} warm-up, oracle/ref_cpu.py; "
                      f"{sample_steps} reverse steps at n={batch} after {warm} warm-up",
            "train_ms_per_step": round(dt * 1e3, 1),
            "sample_step_ms_n64": round(sdt * 1e3, 1),
            "sample_chain_s_n64_extrapolated": round(sdt * 1000, 1)}


def _time_ms(fn, reps: int, warm: int = 2):
    """Average duration of fn() over `reps` back-to-back calls, HIP events on the launch stream."""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def peak_probes():
    """Measured denominators ('ship a peak_probe and divide by the MEASURED peak,
    reporting both'): tdx_probe_mfma_f32 = back-to-back v_mfma_f32_32x32x2_f32 on four independent
    accumulators per wave, one wave per SIMD on every CU; tdx_probe_stream_copy = float4 copy of
    1 GiB (read + write counted)."""
    from tiny_diffusion_amd._lib import lib, check

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    blocks, iters = 256 * 4, 4096
    out = torch.empty(blocks * 256, device=dev)
    ms = _time_ms(lambda: check(lib.tdx_probe_mfma_f32(out.data_ptr(), iters, blocks, st)), 5)
    flop = blocks * 4 * iters * 4 * (2.0 * 32 * 32 * 2)     # blocks x waves x iters x chains x FLOP/MFMA
    n = 1 << 28                                              # 1 GiB of floats
    a, b = torch.empty(n, device=dev), torch.empty(n, device=dev)
    a.normal_()
    cms = _time_ms(lambda: check(lib.tdx_probe_stream_copy(a.data_ptr(), b.data_ptr(), n, st)), 5)
    return {"mfma_f32_tflops": round(flop / ms / 1e9, 1), "hbm_copy_tbps": round(2 * 4.0 * n / cms / 1e9, 2)}


def _time_rot_ms(fns, reps: int, warm: int = 1):
    """Average duration of one call when the calls cycle through `fns` (the same kernel on DIFFERENT buffer
    sets): consecutive repetitions never touch the same bytes."""
    k = len(fns)
    for i in range(warm * k):
        fns[i % k]()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps * k):
        fns[i % k]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (reps * k)


HBM_WORKING_SET = 1.5e9   # bytes cycled through per kernel: 6x the 256 MiB Infinity Cache


def hbm_kernels(B: int, copy_tbps: float):
    """GB/s of the HBM-bound kernels of the step: algorithmic bytes / HIP-event time, against
    the 8 TB/s spec and against the measured copy rate.  Round 2 repeated each kernel on ONE buffer set of
    154-313 MB, most of which stays in the 256 MiB Infinity Cache between repetitions - those were cache
    figures (up to 1.26x the measured copy rate).  Now every kernel cycles through enough independent buffer
    sets to touch >= 1.5 GB between two uses of the same bytes, so the rate is an HBM rate."""
    from tiny_diffusion_amd._lib import lib, check
    from tiny_diffusion_amd.diffusion import ForwardProcess

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    fp = ForwardProcess()
    rows = {}

    def add(name, nbytes, ms, note, sets):
        tb = nbytes / ms / 1e9
        rows[name] = {"gbps": round(tb * 1e3, 1), "us": round(ms * 1e3, 2), "bytes": int(nbytes),
                      "buffer_sets": sets, "bytes_between_reuse": int(nbytes * sets),
                      "frac_of_8tbps": round(tb / PEAK_HBM_TBPS, 3),
                      "frac_of_measured_copy": round(tb / copy_tbps, 3) if copy_tbps else None, "what": note}

    def nsets(nbytes):
        return max(2, min(48, int(-(-HBM_WORKING_SET // nbytes))))

    # the elementwise kernels at the benchmark's own size are 0.8 MB launches (latency, not bandwidth): they
    # are timed at 64x the batch so that the kernel, not the launch, is what is measured
    nb = 64 * B
    sa, sb, coef = fp.tables(dev)
    ti = torch.tensor([500], dtype=torch.int32, device=dev)
    k = nsets(12.0 * nb * 784)
    xs = [torch.rand(nb, 1, 28, 28, device=dev) for _ in range(k)]
    ts_ = [torch.randint(0, 1000, (nb,), device=dev) for _ in range(k)]
    ms = _time_rot_ms([(lambda x=x, t=t: fp.q_sample_philox(x, t, 1, 0)) for x, t in zip(xs, ts_)], 3)
    add("q_sample_philox_x64", 12.0 * nb * 784, ms, f"read x0, write x_t + eps, in-kernel Philox; B={nb}", k)
    es = [torch.randn_like(x) for x in xs]
    ms = _time_rot_ms([(lambda x=x, e=e: check(lib.tdx_p_sample_step_philox(x.data_ptr(), x.data_ptr(), e.data_ptr(),
                                                                            coef.data_ptr(), ti.data_ptr(), x.numel(), 7,
                                                                            st))) for x, e in zip(xs, es)], 3)
    add("p_sample_philox_x64", 12.0 * nb * 784, ms, f"read x, eps; write x; in-kernel noise; n={nb}", k)
    del xs, es, ts_
    # BatchNorm+ReLU backward of the largest unit (dec1.0 output: 256x32x32x64) and a deep one
    for cout, H in ((64, 32), (128, 28), (512, 7)):
        M = B * H * H
        k = nsets(20.0 * M * cout)
        gs = [torch.randn(M * cout, device=dev) for _ in range(k)]
        ys = [torch.randn(M * cout, device=dev) for _ in range(k)]
        ss = torch.rand(4 * cout, device=dev) + 0.5
        gamma = torch.ones(cout, device=dev)
        dg, db, dbias = (torch.empty(cout, device=dev) for _ in range(3))
        scr = torch.empty(lib.tdx_bn_relu_bwd_scratch_floats(M, cout), device=dev)
        ms = _time_rot_ms([(lambda g=g, y=y: check(lib.tdx_bn_relu_bwd(g.data_ptr(), y.data_ptr(), M, cout, ss.data_ptr(),
                                                                      ss[cout:].data_ptr(), ss[2 * cout:].data_ptr(),
                                                                      ss[3 * cout:].data_ptr(), gamma.data_ptr(),
                                                                      dg.data_ptr(), db.data_ptr(), dbias.data_ptr(),
                                                                      scr.data_ptr(), 1, st))) for g, y in zip(gs, ys)], 2)
        add(f"bn_relu_bwd_c{cout}_hw{H}", 20.0 * M * cout, ms, "read g, y twice; write g (reduce + finalize + apply)", k)
        del gs, ys
    n = 11_182_273
    k = nsets(28.0 * n)
    sets = []
    for _ in range(k):
        pa, gr, m1, m2 = (torch.randn(n, device=dev) * 0.01 for _ in range(4))
        m2.abs_()
        sets.append((pa, gr, m1, m2))
    ms = _time_rot_ms([(lambda q=q: check(lib.tdx_adam_step(q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(),
                                                           q[3].data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 3, 1.0, st)))
                       for q in sets], 3)
    add("adam", 28.0 * n, ms, "read p, g, m, v; write p, m, v; 11.18 M parameters", k)
    del sets
    torch.cuda.empty_cache()
    return rows


def in_situ():
    """Sum of the MFMA convolution kernel durations INSIDE the real training step (three streams,
    kernels sharing CUs), from the committed rocprofv3 kernel trace of the training leg
    (tools/insitu.py -> profiles/<tag>_insitu.json): the isolated-launch roofline above is an upper
    bound on what the step sees.  A committed profile, not a measurement of this run: `same_build_as_this_run`."""
    return _committed("insitu")


def first_step_parity(model, fp, x0, seed: int, cond=None, bf16: bool = False):
    """Outside the timed region: eps_hat of a leg's own first forward (train-mode BatchNorm, the leg's batch
    and resolution, in-kernel Philox noise) against the CPU oracle on the same x_t, t and weights
    (diffusion.py:225-228; conditional_diffusion_laion.py:304-332 when `cond` = text embeddings is given); the
    BatchNorm buffers are put back afterwards.  Gates: fp32 - MSE < 1e-5 (north_star) and relative MSE < 1e-9;
    bf16 compute mode - MSE <= 1.0e-4 against the fp32 oracle: the SMALLEST eps_hat MSE the reference's own modules show
    under torch's bf16 autocast on the fixtures (tests/golden/bf16_autocast.npz: 1.0e-4 .. 4.8e-4 in train mode;
    tests/test_gpu_bf16.py gates every network against its own figure)."""
    from oracle import ref_cpu as R
    from oracle import ref_laion as RL
    from tiny_diffusion_amd.unet import MODE_TRAIN

    dev = x0.device
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    g = torch.Generator(device=dev).manual_seed(4242)
    t = torch.randint(0, fp.num_timesteps, (x0.shape[0],), device=dev, generator=g)
    x_t, noise = fp.q_sample_philox(x0, t, seed, 0)
    eps, _, _ = model._run_forward(x_t, t, cond, mode=MODE_TRAIN)
    torch.cuda.synchronize()
    p, b = R.split_state(sd)
    torch.set_num_threads(usable_cores())
    with torch.no_grad():
        if cond is None:
            ref = R.unet_forward(p, b, x_t.cpu(), t.cpu(), training=True)
        else:
            ref = RL.unet_forward(p, b, x_t.cpu(), t.cpu(), cond.cpu(), training=True)
    d = eps.cpu().double() - ref.double()
    mse = (d ** 2).mean().item()
    rel = mse / max((ref.double() ** 2).mean().item(), 1e-30)
    with torch.no_grad():
        for k, v in model.named_buffers():
            v.copy_(sd[k])
    model._buf_epoch += 1
    ok = mse <= 1.0e-4 if bf16 else (mse < 1e-5 and rel < 1e-9)
    if not ok:
        raise SystemExit(f"bench: eps_hat of the first step disagrees with the CPU oracle: MSE {mse:.3e}, "
                         f"relative {rel:.3e} (shape {tuple(x0.shape)}, bf16={bf16})")
    return {"batch": int(x0.shape[0]), "eps_mse_vs_oracle": float(f"{mse:.3e}"),
            "eps_rel_mse_vs_oracle": float(f"{rel:.3e}"),
            "gate": "MSE <= 1.0e-4 vs the fp32 oracle = the smallest MSE of the reference under bf16 autocast" if bf16
                    else "MSE < 1e-5 (north_star) and relative MSE < 1e-9"}


def self_launch(args) -> int:
    """`python bench.py --gpus N` (N > 1) without a launcher: start N ranks of this script through
    torch.distributed.run (one process per GPU, RCCL) from a parent that has not touched the GPU,
    pass their output through and exit with their status."""
    import socket
    import subprocess

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def sample_latency(model, diffusion, n: int):
    from tiny_diffusion_amd.diffusion import sample

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x = sample(model, diffusion, "cuda", n_samples=n, use_graph=True, philox_seed=7)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert torch.isfinite(x).all()
    return dt


# forward FLOPs per sample of the LAION UNet's 3x3 convs (conditional_diffusion_laion.py:244-296):
# (cin, cout, hw) per conv incl. initial/final
_LAION_CONVS = [(4, 32, 32), (32, 64, 32), (64, 64, 32), (64, 128, 16), (128, 128, 16), (128, 256, 8),
                (256, 256, 8), (256, 256, 4), (512, 256, 8), (256, 256, 8), (384, 128, 16), (128, 128, 16),
                (192, 64, 32), (64, 64, 32), (64, 4, 32)]
LAION_FWD_FLOP = sum(2 * 9 * ci * co * hw * hw for ci, co, hw in _LAION_CONVS)


PEAK_BF16_MFMA_TFLOPS = 2500.0             # MI355X_MICROARCH.md (dense bf16 matrix; the sparse figure is 2x)

# (cin, cout, hw) of the LAION network's 13 conv/BN units at 32x32 (conditional_diffusion_laion.py:246-295; the first
# unit's input is stored zero-padded to 64 channels)
LAION_UNITS = [(64, 64, 32), (64, 64, 32), (64, 128, 16), (128, 128, 16), (128, 256, 8), (256, 256, 8), (256, 256, 4),
               (512, 256, 8), (256, 256, 8), (384, 128, 16), (128, 128, 16), (192, 64, 32), (64, 64, 32)]


def bf16_hbm_roofline(units, B, n_params, ms_per_step):
    """HBM roofline of a training step in the bf16 mode (bf16 MFMA operands AND bf16 activation tensors): at 16x
    the fp32 matrix rate the step is bandwidth-bound, so its yardstick is algorithmic bytes / 8 TB/s.  Algorithmic
    bytes per step = every tensor moved the minimum number of times at its storage width:
      convolutions   3 roles x (read M*cin + M*cout elements, 2 B each) + bf16 weight packs read 3x + the fp32
                     weight gradient written once;
      BatchNorm bwd  read g, read y, write g: 6 B per output element (the reduction rides on the producer);
      pool / resize / concat   each decoder input written once and each pooled map written once, forward and
                     backward (2 B/elt; their reads are the convolutions' outputs, counted above);
      optimizer      28 B per parameter (fp32 p, g, m, v read; p, m, v written).
    What the kernels actually move on top of that (nine taps re-reading rows through L2, split-K slabs, the
    BatchNorm reduction passes that are not fused) is the gap `frac` shows."""
    conv = bn = spatial = wts = 0.0
    for cin, cout, hw in units:
        M = B * hw * hw
        conv += 3 * 2.0 * M * (cin + cout)
        bn += 6.0 * M * cout
        wts += 3 * 2.0 * 9 * cin * cout + 4.0 * 9 * cin * cout
    # decoder inputs (units 7, 9, 11) and pooled maps (inputs of units 2, 4, 6): written once forward, their
    # gradients once backward
    for i in (7, 9, 11, 2, 4, 6):
        cin, _, hw = units[i]
        spatial += 2 * 2.0 * B * hw * hw * cin
    adam = 28.0 * n_params
    total = conv + bn + spatial + wts + adam
    tbps = total / (ms_per_step * 1e-3) / 1e12
    return {"bound": "hbm", "achieved": round(tbps * 1e3, 1), "peak": PEAK_HBM_TBPS * 1e3, "unit": "GB/s",
            "frac": round(tbps / PEAK_HBM_TBPS, 4), "algorithmic_bytes_per_step": int(total),
            "breakdown_mb": {"conv_operands": round(conv / 1e6, 1), "batchnorm_backward": round(bn / 1e6, 1),
                             "pool_resize_concat": round(spatial / 1e6, 1), "weights": round(wts / 1e6, 1),
                             "optimizer": round(adam / 1e6, 1)},
            "hbm_time_at_peak_ms": round(total / (PEAK_HBM_TBPS * 1e12) * 1e3, 3)}


def laion_extras(steps: int = 30, warmup: int = 6):
    """SURVEY.md 8(f) f3 (BASELINE.json configs[4] shape): training step of the LAION-shaped latent UNet
    (q_sample + fwd + MSE + bwd + clip_grad_norm(10) fused into Adam, cosine LR) at the reference's
    batch 8 and at 256, on (4,32,32) latents (the reference's shape) and (4,64,64) (the config's
    wording), in fp32 and in the opt-in bf16 compute mode (bf16 MFMA operands, fp32 accumulation and
    storage - never the headline; tolerance in tests/test_gpu_bf16.py), and the 1000-step reverse chain
    for 4 prompts."""
    from tiny_diffusion_amd.conditional_diffusion_laion import ForwardProcess, NoiseModel, sample
    from tiny_diffusion_amd.train import TrainStep

    out = {"fwd_gflop_per_sample": round(LAION_FWD_FLOP / 1e9, 3), "fwd_gflop_per_sample_hw64": round(4 * LAION_FWD_FLOP / 1e9, 3)}
    fp = ForwardProcess()

    def leg(B, hw, dtype):
        torch.manual_seed(0)
        model = NoiseModel(time_dim=768).cuda().train().set_compute_dtype(dtype)
        ts = TrainStep(model, fp, lr=1e-4, philox_seed=99, max_grad_norm=10.0, cosine_T_max=1000, cosine_eta_min=1e-6)
        x0 = torch.randn(B, 4, hw, hw, device="cuda") * 0.8
        cond = torch.randn(B, 768, device="cuda")
        # untimed: this leg's own first forward against the CPU oracle, at the size it is about to time
        parity = first_step_parity(model, fp, x0, 99, cond=cond, bf16=dtype == torch.bfloat16)
        for _ in range(warmup):
            ts.step(x0, cond)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = ts.step(x0, cond)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lv = loss.item()
        if not (lv == lv) or lv > 1e3:
            raise SystemExit(f"LAION training diverged in the benchmark (B={B}, hw={hw}, {dtype}): loss {lv}")
        flop = 3 * LAION_FWD_FLOP * (hw / 32) ** 2
        res = {"samples_per_s": round(B * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 3),
               "tflops": round(B * steps / dt * flop / 1e12, 2), "loss_after": round(lv, 4), "parity_check": parity}
        return res, model, cond

    r, model, cond = leg(8, 32, torch.float32)
    out["train_B8"] = r
    model.eval()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x = sample(model, fp, "cuda", text_embeds=cond[:4], use_graph=True, philox_seed=7)
    torch.cuda.synchronize()
    assert torch.isfinite(x).all()
    out["sample_n4_s_per_1000_steps"] = round(time.perf_counter() - t0, 3)
    del model
    out["train_B256"], _, _ = leg(256, 32, torch.float32)
    out["train_B256_hw64"], _, _ = leg(256, 64, torch.float32)
    bf = {"arithmetic": "bf16 MFMA operands (v_mfma_f32_32x32x16_bf16), fp32 accumulation; activations and activation "
                        "gradients stored in bf16; fp32 parameters, BatchNorm statistics, time MLP, loss, Adam",
          "peak_tflops": PEAK_BF16_MFMA_TFLOPS}
    for key, B, hw in (("train_B256", 256, 32), ("train_B256_hw64", 256, 64)):
        r, _, _ = leg(B, hw, torch.bfloat16)
        r["roofline"] = bf16_hbm_roofline([(ci, co, h * hw // 32) for ci, co, h in LAION_UNITS], B, 5_793_124,
                                          r["ms_per_step"])
        r["frac_of_bf16_mfma_peak"] = round(r["tflops"] / PEAK_BF16_MFMA_TFLOPS, 4)
        r["speedup_vs_fp32"] = round(out[key]["ms_per_step"] / r["ms_per_step"], 2)
        bf[key] = r
    out["bf16"] = bf
    torch.cuda.empty_cache()
    return out


def bf16_gemm_roofline(units, B, reps: int = 5):
    """The 39 bf16-mode GEMM launches of one training step in isolation (bf16 storage entry points of the C ABI, HIP
    events on the launch stream): forward, input gradient, weight gradient (GEMM into slabs + slab reduction) per
    unit - the bf16-mode counterpart of the fp32 `roofline` block, against the bf16 matrix peak.  These kernels are
    bound by L1 / LDS traffic, not by the matrix core: the fraction says how far."""
    from tiny_diffusion_amd._lib import lib, check
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    tot = {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0}
    flop = 0.0
    for cin, cout, H, in_bn in units:
        M = B * H * H
        x = torch.randn(M * cin, device=dev).to(torch.bfloat16)
        dy = torch.randn(M * cout, device=dev).to(torch.bfloat16)
        w = torch.randn(cout, cin, 3, 3, device=dev) * 0.02
        wf = torch.empty(cout * 9 * cin, dtype=torch.bfloat16, device=dev)
        wd = torch.empty(cout * 9 * cin, dtype=torch.bfloat16, device=dev)
        check(lib.tdx_pack_conv3x3_bf16(w.data_ptr(), wf.data_ptr(), wd.data_ptr(), cout, cin, st))
        out = torch.empty(M * cout, dtype=torch.bfloat16, device=dev)
        gin = torch.empty(M * cin, dtype=torch.bfloat16, device=dev)
        stats = torch.empty(((M + 127) // 128) * 2 * cout, device=dev)
        splits = lib.tdx_conv3x3_wgrad_splits_bf16(B, H, H, cin, cout)
        slabs = torch.empty(splits * cout * 9 * cin, device=dev)
        dw = torch.empty(cout * cin * 9, device=dev)
        bias = torch.zeros(cout, device=dev)

        # (the step materialises relu(bn(Y)) for the units whose input is a BatchNorm output: raw inputs here)
        def fwd():
            check(lib.tdx_conv3x3_fwd_bf16_io(x.data_ptr(), wf.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, H, cin,
                                              cout, 4, None, None, None, None, stats.data_ptr(), 1, st))

        def dgrad():
            check(lib.tdx_conv3x3_fwd_bf16_io(dy.data_ptr(), wd.data_ptr(), None, gin.data_ptr(), B, H, H, cout, cin, 0,
                                              None, None, None, None, None, 1, st))

        def wgrad():
            check(lib.tdx_conv3x3_wgrad_bf16_io(x.data_ptr(), dy.data_ptr(), slabs.data_ptr(), B, H, H, cin, cout, 0, None,
                                                None, 1, st))
            check(lib.tdx_conv3x3_wgrad_reduce(slabs.data_ptr(), dw.data_ptr(), splits, cout, cin, st))

        for name, fn in (("fwd", fwd), ("dgrad", dgrad), ("wgrad", wgrad)):
            tot[name] += _time_ms(fn, reps)
        flop += 3 * 2.0 * M * 9 * cin * cout
    ms = sum(tot.values())
    tf = flop / (ms * 1e-3) / 1e12
    return {"bound": "mfma", "achieved": round(tf, 1), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s",
            "frac": round(tf / PEAK_BF16_MFMA_TFLOPS, 4), "launches_per_step": 3 * len(units),
            "gemm_ms_per_step_isolated": round(ms, 3),
            "by_role_ms": {k: round(v, 3) for k, v in tot.items()},
            "kernel": "conv3x3_bf16_kernel (fwd, dgrad) + conv3x3_wgrad9_bf16_kernel + wgrad_reduce_kernel; "
                      "weight-gradient rows = GEMM into slabs + reduction"}


def mnist_bf16_leg(fp, steps: int = 30, warmup: int = 6):
    """The headline workload in the opt-in bf16 compute mode (same step, same batch): reported beside
    the fp32 value, never in its place."""
    from tiny_diffusion_amd.diffusion import NoiseModel
    from tiny_diffusion_amd.train import TrainStep

    torch.manual_seed(0)
    m = NoiseModel().cuda().train().set_compute_dtype(torch.bfloat16)
    ts = TrainStep(m, fp, lr=1e-3, philox_seed=1234)
    x0 = torch.rand(PER_GPU_BATCH, 1, 28, 28, device="cuda") * 2 - 1
    parity = first_step_parity(m, fp, x0, 1234, bf16=True)   # untimed, at the size about to be timed
    for _ in range(warmup):
        ts.step(x0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = ts.step(x0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lv = loss.item()
    if not (lv == lv) or lv > 1e3:
        raise SystemExit(f"bf16 training diverged in the benchmark: loss {lv}")
    v = PER_GPU_BATCH * steps / dt
    return {"images_per_s": round(v, 1), "ms_per_step": round(dt / steps * 1e3, 3), "loss_after": round(lv, 4),
            "parity_check": parity,
            "tflops": round(v * TRAIN_FLOP_PER_IMAGE / 1e12, 1),
            "frac_of_bf16_mfma_peak": round(v * TRAIN_FLOP_PER_IMAGE / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4),
            "roofline": bf16_hbm_roofline([(ci, co, h) for ci, co, h, _ in UNITS], PER_GPU_BATCH, 11_182_273,
                                          dt / steps * 1e3),
            "gemm_roofline": bf16_gemm_roofline(UNITS, PER_GPU_BATCH),
            "arithmetic": "bf16 MFMA operands, fp32 accumulation; activations and activation gradients stored in bf16 "
                          "(tests/test_gpu_bf16.py)"}


def latent_extras(steps: int = 200, warmup: int = 20):
    """SURVEY.md 8(f) f4 (the model BASELINE.json configs[3] actually refers to): training
    step of the latent MLP noise model at the reference's batch 128 (vae.encode + reparameterize +
    q_sample + fwd + MSE + bwd + Adam, latent_diffusion.py:199-222) and the 1000-step reverse
    chain + vae.decode for n=16 (latent_diffusion.py:308-347).  Launch-latency bound by nature."""
    from tiny_diffusion_amd.latent_diffusion import VAE, ForwardProcess, NoiseModel, VAEConfig, sample
    from tiny_diffusion_amd.train import TrainStep

    torch.manual_seed(0)
    fp = ForwardProcess()
    vae = VAE(VAEConfig()).cuda().eval()
    out = {}
    # (B, graph, dtype): fp32 = the reference's arithmetic; bf16 = BASELINE.json configs[3] as worded (Linear layers on
    # the bf16 MFMA, fp32 BatchNorm1d / time path / tensors: tests/test_gpu_latent.py gates it against the reference's
    # own module under bf16 autocast).  Launch-bound either way: the bf16 leg is reported, not expected to be faster.
    for B, graph, dt16 in ((128, False, False), (1024, False, False), (128, False, True), (1024, False, True)):
        model = NoiseModel().cuda().train()
        if dt16:
            model.set_compute_dtype(torch.bfloat16)
        ts = TrainStep(model, fp, lr=1e-3, use_graph=graph)
        x = torch.rand(B, 784, device="cuda") * 2 - 1
        y = torch.randint(0, 10, (B,), device="cuda")

        def one():
            mu, logvar = vae.encode(x)
            return ts.step(vae.reparameterize(mu, logvar), y)

        for _ in range(warmup):
            one()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = one()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lv = loss.item()
        if not (lv == lv) or lv > 1e3:
            raise SystemExit(f"latent training diverged in the benchmark: loss {lv}")
        out[f"train_B{B}" + ("_graph" if graph else "") + ("_bf16" if dt16 else "")] = {
            "samples_per_s": round(B * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 4)}
    model.set_compute_dtype(torch.float32)
    model.eval()
    y16 = torch.randint(0, 10, (16,), device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    img = sample(vae, model, fp, "cuda", n_samples=16, y=y16, use_graph=True, philox_seed=3)
    torch.cuda.synchronize()
    assert torch.isfinite(img).all()
    out["sample_n16_s_per_1000_steps"] = round(time.perf_counter() - t0, 4)
    return out


def timed_steps(ts, x0, warmup: int, steps: int, barrier):
    for _ in range(warmup):
        ts.step(x0)
    torch.cuda.synchronize(); barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = ts.step(x0)
    torch.cuda.synchronize(); barrier()
    return time.perf_counter() - t0, loss


DUMP_LIMIT_BYTES = 64 << 20


def write_outputs(out_dir: str, arrays: dict) -> dict:
    """Each entry as <out_dir>/<name>.npy in float32 (float64 stays float64); at most DUMP_LIMIT_BYTES in all.
    Returns {name: shape}."""
    import numpy as np

    host = {}
    for name, t in arrays.items():
        t = t.detach().cpu()
        host[name] = t.numpy() if t.dtype == torch.float64 else t.float().numpy()
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"bench: outputs of {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte dump limit")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in host.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: list(a.shape) for name, a in host.items()}


def dump_outputs(out_dir: str, model, ts, loss) -> dict:
    """What a caller of TrainStep.step holds after the last timed step: the returned loss, and the model it
    updated in place - every parameter (the flat fp32 buffer the parameters are views of, 11.18 M floats, in
    TrainStep's order) and the BatchNorm running statistics (floating-point buffers in named_buffers() order)."""
    bufs = [b.detach().reshape(-1).float() for _, b in model.named_buffers() if b.is_floating_point()]
    return write_outputs(out_dir, {"loss": loss.reshape(-1), "params": ts.flat_param,
                                   "bn_running_stats": torch.cat(bufs)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps write the last step's loss, parameters and BatchNorm running statistics "
                         "as DIR/<name>.npy (rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="also run the parity check, the replica check / single-rank step (N > 1) and, unless "
                         "--no-extras, every other leg (roofline, probes, HBM kernels, CPU baseline, sampling, bf16, "
                         "LAION, latent)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip roofline / cpu baseline / sampling legs")
    ap.add_argument("--roofline-only", action="store_true",
                    help="run only the per-launch conv timing leg (for rocprofv3 cross-checks)")
    ap.add_argument("--train-only", action="store_true",
                    help="run only the timed training steps (for rocprofv3 traces of the real step)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench: --steps must be >= 1 and --warmup >= 0")
    extras = args.full and not args.no_extras and not args.train_only
    if args.roofline_only:
        torch.cuda.set_device(0)
        print(json.dumps({"roofline": roofline_block(PER_GPU_BATCH)}))
        return

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "RANK" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher (nothing has touched the GPU yet)
        sys.exit(self_launch(args))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # one rank per GPU; (a rehearsal with more ranks than GPUs - gloo only - wraps around)
    dev_index = local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    use_dist = world > 1 or "RANK" in os.environ      # torch.distributed.run, even with 1 rank
    backend = os.environ.get("TDX_DIST_BACKEND", "nccl")  # "nccl" is RCCL on ROCm
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend == "nccl":
            torch.distributed.init_process_group("nccl", device_id=dev)
        else:
            torch.distributed.init_process_group(backend)

    from tiny_diffusion_amd.diffusion import ForwardProcess, NoiseModel
    from tiny_diffusion_amd.train import TrainStep

    torch.manual_seed(0)                      # identical init on every rank
    model = NoiseModel().to(dev).train()
    fp = ForwardProcess()
    ts = TrainStep(model, fp, lr=1e-3, philox_seed=1234)   # the Philox stream is keyed by (step, rank)
    ts.broadcast_parameters(0)
    g = torch.Generator(device=dev).manual_seed(rank)
    x0 = torch.rand(PER_GPU_BATCH, 1, 28, 28, device=dev, generator=g) * 2 - 1   # Normalize(0.5,0.5) range

    def barrier():
        if use_dist:
            torch.distributed.barrier()

    parity = None
    if rank == 0 and args.full and not args.train_only:
        note("first-step parity check against the CPU oracle (B=256 forward on the host) ...")
        parity = first_step_parity(model, fp, x0, 1234)   # untimed; the other ranks wait at the barrier
        note(f"parity ok: {parity}")
    dt, loss = timed_steps(ts, x0, args.warmup, args.steps, barrier)
    if world > 1:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = tt.item()
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, model, ts, loss)
        note(f"outputs of the last step in {args.dump_outputs}: {dumped}")
    loss_v = loss.item()
    if not (loss_v == loss_v) or loss_v > 1e3:
        raise SystemExit(f"training diverged in the benchmark: loss {loss_v}")
    single = None
    if world > 1 and args.full:
        # outside the timed region: replicas must still hold identical parameters
        probe = torch.stack([ts.flat_param.double().sum(), ts.flat_param.double().pow(2).sum()])
        lo, hi = probe.clone(), probe.clone()
        torch.distributed.all_reduce(lo, op=torch.distributed.ReduceOp.MIN)
        torch.distributed.all_reduce(hi, op=torch.distributed.ReduceOp.MAX)
        if not torch.equal(lo, hi):
            raise SystemExit(f"data-parallel replicas diverged: {lo.tolist()} vs {hi.tolist()}")
        # the same step with the gradient exchange switched off, on every GPU at once: what one rank
        # does alone on this node right now (context for the driver's own scaling computation)
        torch.manual_seed(0)
        m1 = NoiseModel().to(dev).train()
        ts1 = TrainStep(m1, fp, lr=1e-3, philox_seed=1234, data_parallel=False)
        k1 = max(2, min(args.steps, 20))
        dt1, _ = timed_steps(ts1, x0, min(args.warmup, 5), k1, barrier)
        r1 = torch.tensor([PER_GPU_BATCH * k1 / dt1], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(r1)
        single = r1.item() / world
        del ts1, m1

    multi = None
    if world > 1 and extras:
        # BASELINE's metric also names the 1000-step sample latency at every N.  Sampling does not shard (SURVEY.md
        # 8(e): replicas only): every rank runs its OWN chains at n = 16 and n = 64 with no collective in the path,
        # all ranks at once; the line reports the MAX over ranks (what the slowest replica's user waits for).  The
        # collectives below only carry the timings to rank 0, after the chains have finished.
        model.eval()
        s16, s64 = sample_latency(model, fp, 16), sample_latency(model, fp, 64)
        model.train()
        tt = torch.tensor([s16, s64], device=dev, dtype=torch.float64)
        hi, lo = tt.clone(), tt.clone()
        torch.distributed.all_reduce(hi, op=torch.distributed.ReduceOp.MAX)
        torch.distributed.all_reduce(lo, op=torch.distributed.ReduceOp.MIN)
        # and the kernel-level roofline of EVERY rank's GPU (isolated launches, HIP events), all GPUs busy at once
        roof = roofline_block(PER_GPU_BATCH)
        mine = {"rank": rank, "achieved": roof["achieved"], "frac": roof["frac"], "avg_launch_us": roof["avg_launch_us"]}
        per_rank = [None] * world
        torch.distributed.all_gather_object(per_rank, mine)
        multi = {"sample": {"n16_max": hi[0].item(), "n64_max": hi[1].item(), "n16_min": lo[0].item(),
                            "n64_min": lo[1].item()}, "roofline": roof, "per_rank": per_rank}

    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        value = world * PER_GPU_BATCH * args.steps / dt
        res = {
            "metric": "train images/s (q_sample+fwd+MSE+bwd+allreduce+Adam), MNIST 28x28 UNet fp32; "
                      "1000-step sample latency in `sample`",
            "value": round(value, 1), "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "diffusion.py unconditional MNIST 28x28 UNet, fp32, train step, "
                                   f"batch {PER_GPU_BATCH}/GPU (BASELINE.json configs[1])",
                       "global_batch": world * PER_GPU_BATCH, "per_gpu_batch": PER_GPU_BATCH,
                       "parallelism": f"dp{world}", "timesteps": 1000},
            "images_per_s_per_gpu": round(value / world, 1),
            "loss_after": round(loss_v, 5),
            "train_tflops_per_gpu": round(value / world * TRAIN_FLOP_PER_IMAGE / 1e12, 2),
            "parity_check": parity,
        }
        if single is not None:
            res["weak_scaling"] = {
                "single_rank_images_per_s": round(single, 1),
                "efficiency": round(value / world / single, 4),
                "note": "single_rank = the same step with the gradient all-reduce disabled, timed on all "
                        f"{world} GPUs at once after the main region (mean over ranks); backend " + backend}
        if extras and world == 1:
            note(f"train: {value:.0f} images/s, {ms_per_step:.3f} ms/step; peak probes ...")
            probes = peak_probes()
            note(f"probes {probes}; conv roofline leg ...")
            res["roofline"] = roofline_block(PER_GPU_BATCH, steady=True)
            res["roofline"]["peak_measured"] = probes["mfma_f32_tflops"]
            res["roofline"]["frac_of_measured_peak"] = round(res["roofline"]["achieved"] / probes["mfma_f32_tflops"], 4)
            res["roofline"]["whole_step_frac"] = round(
                value * TRAIN_FLOP_PER_IMAGE / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)
            res["roofline"]["committed_profile"]["in_situ"] = in_situ()
            note("HBM-bound kernels ...")
            res["hbm_bound_kernels"] = {"peak_tbps": PEAK_HBM_TBPS, "peak_measured_copy_tbps": probes["hbm_copy_tbps"],
                                        "kernels": hbm_kernels(PER_GPU_BATCH, probes["hbm_copy_tbps"])}
            note(f"CPU baseline on {usable_cores()} threads ...")
            res["cpu_baseline"] = cpu_baseline()
            note(f"cpu baseline {res['cpu_baseline']['value']} images/s; sampling chains ...")
            model.eval()
            s16, s64 = sample_latency(model, fp, 16), sample_latency(model, fp, 64)
            # (n16 / n64 are the FIRST call at that batch size in this process: plan creation, sampling tables, warm-up
            # of the captured steps, capture and instantiation included - what rounds 1-3 reported; the second call is
            # what every later sample() of the same shape costs)
            w16, w64 = sample_latency(model, fp, 16), sample_latency(model, fp, 64)
            fwd = TRAIN_FLOP_PER_IMAGE / 3.0  # forward FLOPs per image and step
            res["sample"] = {"unit": "s per 1000-step chain (HIP-graph replay, in-kernel Philox noise)",
                             "n16": round(s16, 3), "n64": round(s64, 3),
                             "n16_second_call": round(w16, 3), "n64_second_call": round(w64, 3),
                             "n16_tflops": round(16 * 1000 * fwd / s16 / 1e12, 1),
                             "n64_tflops": round(64 * 1000 * fwd / s64 / 1e12, 1),
                             "cpu_n64_extrapolated_s": res["cpu_baseline"]["sample_chain_s_n64_extrapolated"]}
            # the other half of BASELINE's metric inside the object the driver's record keeps (missing 3):
            # seconds per 1000-step chain and the algorithmic fraction of the fp32 matrix peak they correspond to
            res["roofline"]["sample_n16_s"] = round(s16, 3)
            res["roofline"]["sample_n64_s"] = round(s64, 3)
            res["roofline"]["sample_n16_frac"] = round(16 * 1000 * fwd / s16 / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)
            res["roofline"]["sample_n64_frac"] = round(64 * 1000 * fwd / s64 / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)
            note("MNIST UNet in bf16 compute mode (opt-in, separate leg) ...")
            res["bf16_mode"] = mnist_bf16_leg(fp)
            note("LAION leg ...")
            res["laion_unet"] = laion_extras()
            note("latent MLP leg ...")
            res["latent_mlp"] = latent_extras()
            note("done")
        elif multi is not None:
            # N > 1: rank 0's block in full, every rank's headline figures beside it
            res["roofline"] = multi["roofline"]
            res["roofline"]["per_rank"] = multi["per_rank"]
            res["roofline"]["whole_step_frac"] = round(
                value / world * TRAIN_FLOP_PER_IMAGE / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)
            fwd = TRAIN_FLOP_PER_IMAGE / 3.0
            sm = multi["sample"]
            res["roofline"]["sample_n16_s"] = round(sm["n16_max"], 3)
            res["roofline"]["sample_n64_s"] = round(sm["n64_max"], 3)
            res["sample"] = {"unit": "s per 1000-step chain (HIP-graph replay, in-kernel Philox noise); one independent "
                                     f"replica per GPU, all {world} at once, no collective: MAX over ranks",
                             "n16": round(sm["n16_max"], 3), "n64": round(sm["n64_max"], 3),
                             "n16_fastest_rank": round(sm["n16_min"], 3), "n64_fastest_rank": round(sm["n64_min"], 3),
                             "n16_tflops_per_gpu": round(16 * 1000 * fwd / sm["n16_max"] / 1e12, 1),
                             "n64_tflops_per_gpu": round(64 * 1000 * fwd / sm["n64_max"] / 1e12, 1),
                             "chains_per_s_whole_job_n16": round(world / sm["n16_max"], 2)}
        print(json.dumps(res), flush=True)
    if use_dist:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
