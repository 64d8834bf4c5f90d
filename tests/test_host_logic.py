"""CPU: host-side logic and the C-ABI surface (no compute calls)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    import tiny_diffusion_amd._lib as L

    hdr = open(os.path.join(ROOT, "include", "tdx.h")).read()
    declared = set(re.findall(r"\b(tdx_[a-z0-9_]+)\s*\(", hdr))
    raw = ctypes.CDLL(os.path.join(ROOT, "tiny_diffusion_amd", "libtdx.so"))
    missing = [s for s in sorted(declared) if not hasattr(raw, s)]
    assert not missing, missing
    assert declared == set(L.EXPORTS), declared ^ set(L.EXPORTS)
    assert L.lib.tdx_version() == 400
    assert L.lib.tdx_error_string(-2) == b"tdx: unsupported shape"


def test_state_dict_matches_reference_layout():
    from oracle.weights import key_shapes, make_state_dict
    from tiny_diffusion_amd.conditional_diffusion import NoiseModel as Cond
    from tiny_diffusion_amd.diffusion import NoiseModel as Unc

    for cls, cond in ((Unc, False), (Cond, True)):
        m = cls()
        sd = m.state_dict()
        want = key_shapes(cond)
        assert list(sd.keys()) == [k for k, _, _ in want]
        for k, shape, _ in want:
            assert tuple(sd[k].shape) == tuple(shape), k
        m.load_state_dict(make_state_dict(0, cond), strict=True)
        assert sum(p.numel() for p in m.parameters()) == (11_184_833 if cond else 11_182_273)


def test_param_slots_and_stage_buckets_cover_all_parameters():
    from tiny_diffusion_amd.conditional_diffusion import NoiseModel
    from tiny_diffusion_amd.unet import backward_stage_params, buffer_slot_names, param_slot_names

    m = NoiseModel()
    names = [n for n, _ in m.named_parameters()]
    slots = [s for s in param_slot_names(True) if s]
    assert sorted(slots) == sorted(names) and len(param_slot_names(True)) == 67
    assert len(buffer_slot_names()) == 39
    staged = [n for st in backward_stage_params(True) for n in st]
    assert sorted(staged) == sorted(names) and len(backward_stage_params(True)) == 15
    assert param_slot_names(False)[4] is None
    # flat-buffer layout: every bucket of the gradient all-reduce is ONE contiguous slice
    from tiny_diffusion_amd.train import plan_buckets

    params = dict(m.named_parameters())
    assert sorted(m._param_order) == sorted(names)
    offsets, o = {}, 0
    for n in m._param_order:
        offsets[n] = (o, o + params[n].numel())
        o += params[n].numel()
    buckets = plan_buckets(offsets, True, 1 << 20)
    assert all(len(ranges) == 1 for _, ranges in buckets), buckets
    assert sum(hi - lo for _, r in buckets for lo, hi in r) == o


def test_cpu_tensors_fail_loudly():
    from tiny_diffusion_amd import _lib
    from tiny_diffusion_amd.diffusion import ForwardProcess, NoiseModel, sample

    m = NoiseModel()
    with pytest.raises(_lib.TdxError):
        m(torch.zeros(2, 1, 28, 28), torch.zeros(2, dtype=torch.long))
    with pytest.raises(_lib.TdxError):
        ForwardProcess().q_sample("cpu", torch.zeros(2, 1, 28, 28), torch.zeros(2, dtype=torch.long))
    with pytest.raises(_lib.TdxError):
        sample(m, ForwardProcess(num_timesteps=2), "cpu", n_samples=2)


def test_forward_process_tables_match_oracle():
    from oracle import ref_cpu as R
    from tiny_diffusion_amd.diffusion import ForwardProcess

    fp, s = ForwardProcess(), R.Schedule()
    assert torch.equal(fp.betas, s.betas) and torch.equal(fp.alphas_cumprod, s.alphas_cumprod)
    sa, sb, coef = fp.tables("cpu")
    c1, c2, sig = s.p_sample_coeffs()
    assert torch.equal(coef, torch.stack([c1, c2, sig], 1))
    assert torch.equal(sa, torch.sqrt(s.alphas_cumprod))


def test_default_init_is_the_reference_init(golden_dir):
    """Same constructors in the same order: under the same seed the module's initial
    weights are the reference's (hash recorded by tools/make_golden.py)."""
    from oracle.weights import state_dict_sha256
    from tiny_diffusion_amd.diffusion import NoiseModel

    path = os.path.join(golden_dir, "weights.sha256")
    want = {l.split()[0] + " " + l.split()[1]: l.split()[2] for l in open(path)}
    if "init uncond_seed0" not in want:
        pytest.skip("golden file predates the init hash")
    torch.manual_seed(0)
    assert state_dict_sha256(NoiseModel().state_dict()) == want["init uncond_seed0"]


def test_laion_module_layout_and_stage_buckets():
    """conditional_diffusion_laion.NoiseModel: reference state_dict order/shapes, slot and
    backward-stage tables cover every parameter (CPU: no compute)."""
    from oracle.weights import key_shapes_laion, make_state_dict_laion
    from tiny_diffusion_amd import _lib
    from tiny_diffusion_amd.conditional_diffusion_laion import NoiseModel, get_timestep_embedding
    from tiny_diffusion_amd.unet import backward_stage_params, param_slot_names

    m = NoiseModel(time_dim=768)
    sd = m.state_dict()
    assert [k for k, _, _ in key_shapes_laion()] == list(sd.keys())
    m.load_state_dict(make_state_dict_laion(0), strict=True)
    assert sum(p.numel() for p in m.parameters()) == 5_793_124
    names = [n for n, _ in m.named_parameters()]
    slots = param_slot_names(False, "time_mlp")
    assert sorted(s for s in slots if s) == sorted(names) and len(slots) == 67 and slots[4] is None
    staged = [n for st in backward_stage_params(False, "time_mlp") for n in st]
    assert sorted(staged) == sorted(names)
    with pytest.raises(_lib.TdxError):
        m(torch.zeros(2, 4, 32, 32), torch.zeros(2, dtype=torch.long), torch.zeros(2, 768))
    with pytest.raises(_lib.TdxError):  # device-only, like everything else on the path
        get_timestep_embedding(torch.tensor([0, 7, 999]), 768)


def test_cosine_schedule_matches_torch():
    """cosine_annealing_lr == CosineAnnealingLR stepped per batch, past T_max too
    (conditional_diffusion_laion.py:436-438, 473)."""
    from tiny_diffusion_amd.train import cosine_annealing_lr

    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=1e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=7, eta_min=1e-6)
    for step in range(1, 30):
        opt.step()
        sched.step()
        want = opt.param_groups[0]["lr"]
        got = cosine_annealing_lr(step, 1e-4, 7, 1e-6)
        assert abs(got - want) <= 1e-9 * max(abs(want), 1e-6) + 1e-12, (step, got, want)


def test_bench_self_launch_command(monkeypatch):
    """`python bench.py --gpus N` starts its own N ranks through torch.distributed.run on 127.0.0.1
    before anything touches the GPU (the driver's BENCH/SCALE command is exactly that form)."""
    import subprocess
    import sys
    import types

    sys.path.insert(0, ROOT)
    import bench

    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return types.SimpleNamespace(returncode=0)

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    assert bench.self_launch(types.SimpleNamespace(gpus=4)) == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_bench_write_outputs(tmp_path):
    """bench.py --dump-outputs: every array as <name>.npy, float32 unless it is float64, and refused beyond 64 MB."""
    import sys

    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    shapes = bench.write_outputs(str(tmp_path / "out"), {"a": torch.arange(6, dtype=torch.float16).reshape(2, 3),
                                                         "b": torch.ones(4, dtype=torch.float64)})
    assert shapes == {"a": [2, 3], "b": [4]}
    a, b = np.load(tmp_path / "out" / "a.npy"), np.load(tmp_path / "out" / "b.npy")
    assert a.dtype == np.float32 and a.tolist() == [[0, 1, 2], [3, 4, 5]] and b.dtype == np.float64
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "big"), {"x": torch.zeros((64 << 20) // 4 + 1)})
    assert not (tmp_path / "big").exists()


def test_conv_descriptor_bound():
    """32-bit buffer offsets with 0x80000000 as the zero-padding sentinel: shapes whose activation
    tensors reach 2 GiB are refused (TDX_E_SHAPE) instead of silently reading real memory for padding
    taps; the plan constructor applies the bound to every unit at max_batch (no GPU call is made:
    the check precedes any allocation)."""
    import ctypes as C

    import tiny_diffusion_amd._lib as L

    lib = L.lib
    assert lib.tdx_conv3x3_shape_ok(256, 32, 32, 256, 64) == 1
    assert lib.tdx_conv3x3_shape_ok(2047, 32, 32, 256, 64) == 1      # dec1.0 of the MNIST UNet: 1 MiB / sample
    assert lib.tdx_conv3x3_shape_ok(2048, 32, 32, 256, 64) == 0
    assert lib.tdx_conv3x3_shape_ok(2048, 32, 32, 64, 256) == 0      # the dgrad reads the cout-wide tensor
    assert lib.tdx_conv3x3_shape_ok(0, 32, 32, 64, 64) == 0
    h = C.c_void_p()
    assert lib.tdx_unet_create_ex(C.byref(h), 2048, 0, 0) == -2      # TDX_E_SHAPE, before any hipMalloc
    assert lib.tdx_unet_create_ex(C.byref(h), 4096, 1, 0) == -2
    # the entry points themselves refuse too (argument checks come before the launch)
    one = C.c_void_p(16)
    assert lib.tdx_conv3x3_fwd(one, one, None, one, 2048, 32, 32, 256, 64, 0, None, None, None, None, None, None) == -2
    assert lib.tdx_conv3x3_wgrad(one, one, one, 2048, 32, 32, 256, 64, 0, None, None, None) == -2


@pytest.mark.parametrize("B,H,W,cin,cout", [(3, 4, 4, 5, 6), (2, 7, 7, 4, 3), (2, 5, 9, 3, 4), (1, 28, 28, 2, 2)])
def test_slot_space_weight_gradient_identity(B, H, W, cin, cout):
    """The arithmetic identity conv3x3_wgrad9_bf16_kernel is built on (csrc/conv3x3_bf16.hip), checked
    on the host against torch's convolution weight gradient: lay every sample out as a padded (H+1) x (W+1) image with a
    zero column after each row and a zero row after each sample, number the positions ("slots") consecutively, and
    the (dh, dw) neighbour of slot s is slot s + dh (W+1) + dw - every out-of-image neighbour lands on a zero slot (or
    in front of / behind the tensor), so
        dW[co][dh][dw][ci] = sum_s dy[s][co] * x[s + dh (W+1) + dw][ci]
    is a plain shifted inner product over ONE slot axis.  Also the block arithmetic of the kernel's input ring: a
    64-slot K-tile plus its halo lies inside blocks t .. t+NB of 64 slots that start HALOB slots in front of it."""
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64)
    dy = torch.randn(B, cout, H, W, generator=g, dtype=torch.float64)
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(torch.nn.functional.conv2d(x, w, padding=1), w, dy)
    PW, PH = W + 1, H + 1
    S = B * PH * PW

    def slots(t):   # (B, C, H, W) -> [S][C] with the pad slots zero
        p = torch.zeros(B, PH, PW, t.shape[1], dtype=t.dtype)
        p[:, :H, :W] = t.permute(0, 2, 3, 1)
        return p.reshape(S, t.shape[1])

    xs, ds = slots(x), slots(dy)
    halo = PW + 1
    xs_h = torch.cat([torch.zeros(halo, cin, dtype=x.dtype), xs, torch.zeros(halo, cin, dtype=x.dtype)])   # outside the tensor: zero
    got = torch.zeros_like(ref)
    for dh in (-1, 0, 1):
        for dw in (-1, 0, 1):
            sh = dh * PW + dw
            got[:, :, dh + 1, dw + 1] = ds.t() @ xs_h[halo + sh:halo + sh + S]
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)
    # ring geometry of the kernel (launch_wgrad9_bf16): K-tile t covers slots [64 t, 64 t + 64) of its chunk and reads
    # input slots 64 t - PW - 1 .. 64 t + 63 + PW + 1; block b holds slots [64 b - HALOB, 64 b - HALOB + 64)
    for Wk in (4, 7, 8, 14, 16, 28, 32, 64, 95):
        PWk = Wk + 1
        HALOB = (PWk + 1 + 63) // 64 * 64
        NB = (HALOB + 64 + PWk) // 64
        for t in range(5):
            lo, hi = 64 * t - PWk - 1, 64 * t + 63 + PWk + 1
            assert (lo + HALOB) // 64 >= t and (hi + HALOB) // 64 <= t + NB, (Wk, t)
        assert (NB + 2) * 64 * 128 + 64 * 128 + 2 * 64 * 128 <= 98304   # ring + mirror + two dy tiles: the launcher's LDS cap


def test_plan_lru_evicts_but_never_destroys_a_referenced_plan(monkeypatch):
    """NoiseModelBase._plan keeps MAX_PLANS plans, least recently used first out; an evicted plan is destroyed
    (tdx_unet_destroy) only when its last holder lets go - which is what lets TrainStep keep the plan of a captured
    graph alive by holding it (train.py: _graph_plan).  Runs without a GPU on a stand-in for _Plan."""
    import gc

    from tiny_diffusion_amd import unet
    from tiny_diffusion_amd.diffusion import NoiseModel

    destroyed = []

    class FakePlan:
        def __init__(self, batch, *a, **k):
            self.batch = batch

        def __del__(self):
            destroyed.append(self.batch)

    monkeypatch.setattr(unet, "_Plan", FakePlan)
    m = NoiseModel()
    dev = torch.device("cuda", 0)   # only its index is read
    held = m._plan(16, dev)         # what a captured graph's owner holds
    for n in range(1, m.MAX_PLANS + 1):
        m._plan(n, dev)
    gc.collect()
    assert len(m._plans) == m.MAX_PLANS and all(p is not held for p in m._plans.values())
    assert 16 not in destroyed, "evicted AND destroyed although still referenced"
    m._plan(1, dev)                 # touching the oldest survivor makes it the newest
    m._plan(100, dev)               # evicts batch 2, not batch 1
    gc.collect()
    assert 2 in destroyed and 1 not in destroyed
    del held
    gc.collect()
    assert 16 in destroyed


def _div_rcp(n, d):
    """conv3x3_wino.hip::div_rcp in numpy float32: q = (int)((float)n * r) with r = 1.0f / d (host division), then one
    fix-up step of the remainder."""
    import numpy as np

    r = np.float32(1.0) / np.float32(d)
    q = np.trunc(n.astype(np.float32) * r).astype(np.int64)
    m = n - q * d
    lo, hi = m < 0, m >= d
    q = q - lo + hi
    m = m + d * lo - d * hi
    return q, m


def test_winograd_tile_division_in_fp32():
    """The forward Winograd kernel divides tile indices n < 2^24 by th * tw and by tw with one fp32 multiplication by
    the reciprocal and ONE fix-up step: correct only while the estimate is off by at most one.  tdx_conv3x3_wino_ok
    admits launches of fewer than 2^24 - 64 tiles on that claim.  Every n in [0, 2^24) for every divisor of the maps of
    both UNets (MNIST 28x28, LAION 32x32 / 64x64) and 1, then seeded random divisors up to 2^23 with n near their
    multiples and near 2^24."""
    import numpy as np

    from tiny_diffusion_amd import unet as UN

    divisors = {1}
    for arch, sides in ((UN.ARCH_MNIST, (28,)), (UN.ARCH_LAION, (32, 64))):
        for h in sides:
            maps = []
            for _ in arch.enc:
                maps.append(h)
                h = -(-h // 2) if arch.ceil_pool else h // 2
            maps.append(h)                # bottleneck
            for _ in arch.dec:
                h *= 2
                maps.append(h)
            for H in maps:
                tw = (H + 1) // 2
                divisors |= {tw, tw * tw}
    assert {1, 16, 4, 196} <= divisors   # 7x7: 4 x 4 tiles per image; 28x28: 14 x 14
    n = np.arange(1 << 24, dtype=np.int64)
    for d in sorted(divisors):
        q, m = _div_rcp(n, d)
        bad = np.nonzero((q != n // d) | (m != n % d))[0]
        assert bad.size == 0, (d, bad[:5])
    rng = np.random.default_rng(24)
    divs = np.concatenate([rng.integers(2, 1 << 23, 400), rng.integers(2, 4096, 400), [(1 << 23) - 1, 1 << 23, 3, 7, 255]])
    top = (1 << 24) - 1 - np.arange(4096, dtype=np.int64)
    for d in divs.tolist():
        k = rng.integers(0, (1 << 24) // d, 256, dtype=np.int64)
        near = (k[:, None] * d + np.arange(-2, 3)[None, :]).ravel()
        cand = np.concatenate([near, top, (((1 << 24) - 1) // d) * d + np.arange(-2, 3)])
        cand = cand[(cand >= 0) & (cand < (1 << 24))]
        q, m = _div_rcp(cand, d)
        assert np.array_equal(q, cand // d) and np.array_equal(m, cand % d), (d, cand[q != cand // d][:5])
