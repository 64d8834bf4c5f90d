"""GPU parity of every libtdx building block against the CPU oracle
(oracle/ref_cpu.py, itself pinned to the reference by tests/test_oracle_golden.py).
All calls go through the C ABI (ctypes).  Tolerances: fp32, relative to the
tensor's RMS; bit-exact where the arithmetic order is fixed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402


@pytest.fixture(scope="module")
def tdx():
    import tiny_diffusion_amd._lib as L

    assert torch.cuda.is_available()
    return L


_KEEP = []


def dev(t):
    """Copy to the GPU and keep the tensor alive: a temporary whose only use is
    ``.data_ptr()`` would be freed (and its block re-used by the next temporary)
    before the kernel that reads it has even been launched."""
    d = t.cuda().contiguous()
    _KEEP.append(d)
    if len(_KEEP) > 256:
        torch.cuda.synchronize()
        del _KEEP[:128]
    return d


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-30)).item()


def stream():
    return torch.cuda.current_stream().cuda_stream


def test_library_exports(tdx):
    assert tdx.lib.tdx_version() == 400
    maps = open("/proc/self/maps").read()
    assert "libtdx.so" in maps


def test_retired_knobs_are_unknown_keys(tdx):
    """The keys of the retired diagnostic paths are refused like a typo; a live key is still taken
    ("wino" 1 is its default, so nothing changes for the tests that follow)."""
    for key in (b"time_stage", b"time_stage_diag", b"time_l1_impl", b"input_copy", b"time_proj_early",
                b"splitk_fused"):
        assert tdx.lib.tdx_tune_set(key, 0) != 0, key
        assert tdx.lib.tdx_tune_set(key, 14) != 0, key   # the one value "time_stage" used to accept
    assert tdx.lib.tdx_tune_set(b"wino", 1) == 0


def test_q_sample_bit_exact(tdx, golden_dir):
    d = np.load(os.path.join(golden_dir, "fwd_B64_train_uncond.npz"))
    from tiny_diffusion_amd.diffusion import ForwardProcess

    fp = ForwardProcess()
    x0, t, noise = torch.from_numpy(d["x0"]), torch.from_numpy(d["t"]), torch.from_numpy(d["noise"])
    x_t, noise_out = fp.q_sample("cuda", x0.cuda(), t.cuda(), noise=noise.cuda())
    assert torch.equal(noise_out.cpu(), noise)
    # bit-exact against the oracle evaluated on THIS host (the schedule tables are host
    # fp32 arithmetic - linspace/cumprod/sqrt - whose last bit can depend on the CPU's
    # vector ISA, in the reference just the same)
    ref_here = R.q_sample(R.Schedule(), x0, t, noise)
    nbad = int((x_t.cpu() != ref_here).sum())
    assert nbad == 0, (nbad, (x_t.cpu() - ref_here).abs().max().item())
    # and within 2 ulp of the x_t the reference produced in the build container
    ref = torch.from_numpy(d["x_t"])
    assert (x_t.cpu() - ref).abs().max().item() <= 1e-6
    s = np.load(os.path.join(golden_dir, "schedule.npz"))
    assert np.allclose(fp.alphas_cumprod.numpy(), s["alphas_cumprod"], rtol=1e-6, atol=0)
    sa, sb, coef = fp.tables("cuda")
    c1, c2, sig = R.Schedule().p_sample_coeffs()
    assert torch.equal(coef.cpu(), torch.stack([c1, c2, sig], 1))
    print("schedule bit-identical to the build container's:",
          np.array_equal(fp.alphas_cumprod.numpy(), s["alphas_cumprod"]))


def test_q_sample_philox_statistics(tdx):
    from tiny_diffusion_amd.diffusion import ForwardProcess

    fp = ForwardProcess()
    B = 512
    x0 = torch.zeros(B, 1, 28, 28, device="cuda")
    t = torch.full((B,), 999, device="cuda")
    x_t, noise = fp.q_sample_philox(x0, t, seed=7)
    n = noise.double()
    assert abs(n.mean().item()) < 0.01 and abs(n.std().item() - 1.0) < 0.01
    assert abs((n**4).mean().item() - 3.0) < 0.1  # gaussian kurtosis
    x2, n2 = fp.q_sample_philox(x0, t, seed=7)
    assert torch.equal(n2, noise)  # counter-based: reproducible
    x3, n3 = fp.q_sample_philox(x0, t, seed=8)
    assert not torch.equal(n3, noise)
    sa, sb, _ = fp.tables("cuda")
    assert torch.equal(x_t, sb[999] * noise)


@pytest.mark.parametrize("t", [999, 500, 1, 0])
def test_p_sample_step_bit_exact(tdx, t):
    from tiny_diffusion_amd.diffusion import ForwardProcess
    from tiny_diffusion_amd.schedule import p_sample_step

    fp = ForwardProcess()
    sched = R.Schedule()
    g = torch.Generator().manual_seed(t)
    x, eps, z = (torch.randn(16, 1, 28, 28, generator=g) for _ in range(3))
    if t == 0:
        z = torch.zeros_like(z)
    ref = R.p_sample_step(sched, x, eps, t, z)
    ti = torch.tensor([t], dtype=torch.int32, device="cuda")
    got = p_sample_step(fp, x.cuda(), eps.cuda(), ti, None if t == 0 else z.cuda())
    assert torch.equal(got.cpu(), ref)


CONV_CASES = [
    # B, H, cin, cout  (every (cin, cout, H) of the UNet + ragged M)
    (4, 28, 64, 128), (2, 28, 128, 128), (3, 14, 128, 256), (3, 14, 256, 256), (5, 7, 256, 512),
    (3, 7, 512, 512), (7, 4, 512, 512), (3, 8, 1024, 256), (3, 8, 256, 256), (2, 16, 512, 128),
    (2, 16, 128, 128), (2, 32, 256, 64), (2, 32, 64, 64), (1, 7, 64, 64), (33, 28, 64, 128),
    # shapes that resolve to the big tiles the B=256 benchmark launches (pick_tile / pick_wgrad):
    (32, 16, 64, 512),    # forward 128x128, wgrad 128x64
    (64, 16, 128, 128),   # forward and dgrad 128x64, wgrad 128x128
    (256, 4, 512, 512),   # forward and dgrad 128x64 at the bottleneck shape of the benchmark
    (32, 16, 512, 128),   # dgrad 128x128
    (660, 7, 128, 128),   # ragged: 32340 rows = 252 full 128-row tiles + 84 rows, forward and dgrad 128x64
]
# (case, role: 0 forward / 2 dgrad / 1 wgrad) -> tile that the library must pick for it; together
# with the small cases (64x64 everywhere) every tile template has a direct oracle check
BIG_TILE_EXPECT = {
    ((32, 16, 64, 512), 0): 128128, ((32, 16, 64, 512), 1): 128064,
    ((64, 16, 128, 128), 0): 128064, ((64, 16, 128, 128), 2): 128064, ((64, 16, 128, 128), 1): 128128,
    ((256, 4, 512, 512), 0): 128064, ((256, 4, 512, 512), 2): 128064, ((256, 4, 512, 512), 1): 64064,
    ((32, 16, 512, 128), 2): 128128, ((2, 32, 256, 64), 1): 64128,
    ((660, 7, 128, 128), 0): 128064, ((660, 7, 128, 128), 2): 128064,
}


def test_conv_cases_cover_every_tile_template(tdx):
    seen = set()
    for (case, role), want in BIG_TILE_EXPECT.items():
        B, H, cin, cout = case
        if role == 2:    # dgrad = the forward kernel with the channel roles swapped
            got = tdx.lib.tdx_conv3x3_tile_shape(B, H, H, cout, cin, 0)
        else:
            got = tdx.lib.tdx_conv3x3_tile_shape(B, H, H, cin, cout, role)
        assert got == want, (case, role, got, want)
        assert case in CONV_CASES
        seen.add((role == 1, got))
    assert {(False, 128128), (False, 128064), (True, 128128), (True, 128064), (True, 64128), (True, 64064)} <= seen
    assert tdx.lib.tdx_conv3x3_tile_shape(4, 28, 28, 64, 128, 0) == 64064


def _conv_inputs(B, H, cin, cout, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, H, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    return x, w, b


def _pack(tdx, w):
    cout, cin = w.shape[:2]
    wd = dev(w)
    wf = torch.empty(cout * 9 * cin, device="cuda")
    wg = torch.empty(cout * 9 * cin, device="cuda")
    tdx.check(tdx.lib.tdx_pack_conv3x3(wd.data_ptr(), wf.data_ptr(), wg.data_ptr(), cout, cin, stream()))
    return wf, wg


@pytest.mark.parametrize("B,H,cin,cout", CONV_CASES)
def test_conv3x3_fwd_plain_and_stats(tdx, B, H, cin, cout):
    x, w, b = _conv_inputs(B, H, cin, cout)
    ref = F.conv2d(x, w, b, padding=1)
    wf, _ = _pack(tdx, w)
    xin = dev(nhwc(x))
    out = torch.full((B, H, H, cout), float("nan"), device="cuda")
    tiles = tdx.lib.tdx_conv3x3_stat_tiles(B, H, H, cin, cout)
    stats = torch.full((tiles, 2, cout), float("nan"), device="cuda")
    tdx.check(tdx.lib.tdx_conv3x3_fwd(xin.data_ptr(), wf.data_ptr(), dev(b).data_ptr(), out.data_ptr(), B, H, H,
                                      cin, cout, 4, None, None, None, None, stats.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert rel_err(nchw(out), ref) < 2e-6
    # per-tile (sum, M2 about the tile mean) partials
    rows = tdx.lib.tdx_conv3x3_stat_tile_rows(B, H, H, cin, cout)
    flat = nhwc(ref).reshape(-1, cout).double()
    for ti in range(tiles):
        blk = flat[ti * rows:(ti + 1) * rows]
        assert torch.allclose(stats[ti, 0].double().cpu(), blk.sum(0), rtol=1e-4, atol=1e-3)
        assert torch.allclose(stats[ti, 1].double().cpu(), (blk - blk.mean(0)).pow(2).sum(0), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("B,H,cin,cout", [(3, 14, 128, 256), (2, 32, 64, 64), (5, 7, 512, 512)])
def test_conv3x3_fwd_fused_bn_relu(tdx, B, H, cin, cout):
    """input BN+ReLU on load and output BN+ReLU epilogue (inference path)."""
    x, w, b = _conv_inputs(B, H, cin, cout, seed=1)
    g = torch.Generator().manual_seed(5)
    isc, ish = torch.randn(cin, generator=g), torch.randn(cin, generator=g) * 0.3
    osc, osh = torch.randn(cout, generator=g), torch.randn(cout, generator=g) * 0.3
    a = F.relu(x * isc.view(1, -1, 1, 1) + ish.view(1, -1, 1, 1))
    ref = F.relu(F.conv2d(a, w, b, padding=1) * osc.view(1, -1, 1, 1) + osh.view(1, -1, 1, 1))
    wf, _ = _pack(tdx, w)
    out = torch.empty((B, H, H, cout), device="cuda")
    tdx.check(tdx.lib.tdx_conv3x3_fwd(dev(nhwc(x)).data_ptr(), wf.data_ptr(), dev(b).data_ptr(), out.data_ptr(),
                                      B, H, H, cin, cout, 1 | 2, dev(isc).data_ptr(), dev(ish).data_ptr(),
                                      dev(osc).data_ptr(), dev(osh).data_ptr(), None, stream()))
    assert rel_err(nchw(out), ref) < 3e-6


@pytest.mark.parametrize("B,H,cin,cout", [(16, 4, 512, 512), (16, 8, 1024, 256), (1, 28, 128, 128), (5, 7, 512, 512),
                                          (2, 16, 512, 128), (64, 4, 512, 512)])
def test_conv3x3_fwd_splitk_inference(tdx, B, H, cin, cout):
    """latency-bound shapes: K split over workgroups + deterministic reduce with the fused
    bias/BN/ReLU epilogue; must equal the unsplit kernel's result up to summation order."""
    x, w, b = _conv_inputs(B, H, cin, cout, seed=7)
    g = torch.Generator().manual_seed(8)
    osc, osh = torch.randn(cout, generator=g), torch.randn(cout, generator=g) * 0.3
    ref = F.relu(F.conv2d(x, w, b, padding=1) * osc.view(1, -1, 1, 1) + osh.view(1, -1, 1, 1))
    wf, _ = _pack(tdx, w)
    need = tdx.lib.tdx_conv3x3_splitk_scratch_floats(B, H, H, cin, cout)
    assert need > 0, "shape was expected to take the split-K path"
    scratch = torch.full((need,), float("nan"), device="cuda")
    xin, bd, oscd, oshd = dev(nhwc(x)), dev(b), dev(osc), dev(osh)
    outs = []
    for _ in range(2):
        out = torch.full((B, H, H, cout), float("nan"), device="cuda")
        tdx.check(tdx.lib.tdx_conv3x3_fwd_splitk(xin.data_ptr(), wf.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, H,
                                                 cin, cout, 2, None, None, oscd.data_ptr(), oshd.data_ptr(),
                                                 scratch.data_ptr(), need, stream()))
        outs.append(out)
    assert rel_err(nchw(outs[0]), ref) < 3e-6
    assert torch.equal(outs[0], outs[1])  # fixed reduction order: bitwise reproducible
    # a scratch that is too small silently uses fewer splits (or none), same result
    small = torch.empty(max(need // 3, 1), device="cuda")
    out2 = torch.empty((B, H, H, cout), device="cuda")
    tdx.check(tdx.lib.tdx_conv3x3_fwd_splitk(xin.data_ptr(), wf.data_ptr(), bd.data_ptr(), out2.data_ptr(), B, H, H,
                                             cin, cout, 2, None, None, oscd.data_ptr(), oshd.data_ptr(),
                                             small.data_ptr(), small.numel(), stream()))
    assert rel_err(nchw(out2), ref) < 3e-6


@pytest.mark.parametrize("B,H,cin,cout", [(16, 4, 512, 512), (1, 28, 128, 128)])
def test_conv3x3_fwd_splitk_bn_on_load(tdx, B, H, cin, cout):
    """split-K of a BN+ReLU-on-load input (the register-staging split-K kernel) with the BN+ReLU epilogue in the
    reduction: against torch, bitwise reproducible, and equal to the unsplit launch up to summation order."""
    x, w, b = _conv_inputs(B, H, cin, cout, seed=1)
    g = torch.Generator().manual_seed(5)
    isc, ish = torch.randn(cin, generator=g), torch.randn(cin, generator=g) * 0.3
    osc, osh = torch.randn(cout, generator=g), torch.randn(cout, generator=g) * 0.3
    a = F.relu(x * isc.view(1, -1, 1, 1) + ish.view(1, -1, 1, 1))
    ref = F.relu(F.conv2d(a, w, b, padding=1) * osc.view(1, -1, 1, 1) + osh.view(1, -1, 1, 1))
    wf, _ = _pack(tdx, w)
    need = tdx.lib.tdx_conv3x3_splitk_scratch_floats(B, H, H, cin, cout)
    assert need > 0, "shape was expected to take the split-K path"
    scratch = torch.full((need,), float("nan"), device="cuda")
    xin, bd = dev(nhwc(x)), dev(b)
    iscd, ishd, oscd, oshd = dev(isc), dev(ish), dev(osc), dev(osh)
    outs = []
    for _ in range(2):
        out = torch.full((B, H, H, cout), float("nan"), device="cuda")
        tdx.check(tdx.lib.tdx_conv3x3_fwd_splitk(xin.data_ptr(), wf.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, H,
                                                 cin, cout, 1 | 2, iscd.data_ptr(), ishd.data_ptr(), oscd.data_ptr(),
                                                 oshd.data_ptr(), scratch.data_ptr(), need, stream()))
        outs.append(out)
    assert rel_err(nchw(outs[0]), ref) < 3e-6
    assert torch.equal(outs[0], outs[1])  # fixed reduction order: bitwise reproducible
    unsplit = torch.full((B, H, H, cout), float("nan"), device="cuda")
    tdx.check(tdx.lib.tdx_conv3x3_fwd(xin.data_ptr(), wf.data_ptr(), bd.data_ptr(), unsplit.data_ptr(), B, H, H, cin,
                                      cout, 1 | 2, iscd.data_ptr(), ishd.data_ptr(), oscd.data_ptr(), oshd.data_ptr(),
                                      None, stream()))
    assert rel_err(outs[0], unsplit) < 3e-6


WINO_CASES =[(4, 28, 64, 128), (3, 14, 128, 256), (5, 7, 256, 512), (7, 4, 512, 512), (3, 8, 1024, 256), (2, 16, 512, 128),
              (2, 32, 256, 64), (2, 32, 64, 64), (1, 64, 64, 64), (33, 8, 128, 128), (3, 16, 384, 128), (2, 32, 192, 64),
              (1, 2, 64, 64), (9, 4, 64, 64)]


@pytest.mark.parametrize("B,H,cin,cout", WINO_CASES)
def test_conv3x3_winograd_fwd_dgrad(tdx, B, H, cin, cout):
    """Winograd F(2x2, 3x3) on the fp32 MFMA (csrc/conv3x3_wino.hip) against F.conv2d in fp64: plain (+ bias), with the
    BatchNorm statistics partials, with the inference epilogue, and - on the mirrored pack - as the input gradient.
    The transforms add and halve in fp32: tolerance 1e-5 relative (measured ~1e-6; the direct kernel: 2e-6 gate).
    Odd maps (7x7: 4x4 tiles per image, the last row / column of tiles half outside), ragged last workgroup, every
    width of the two UNets."""
    lib, check = tdx.lib, tdx.check
    assert lib.tdx_conv3x3_wino_ok(B, H, H, cin, cout) == 1
    x, w, b = _conv_inputs(B, H, cin, cout, seed=21)
    g = torch.Generator().manual_seed(22)
    osc, osh = torch.randn(cout, generator=g), torch.randn(cout, generator=g) * 0.3
    dy = torch.randn(B, cout, H, H, generator=g)
    xd, wd = x.double().requires_grad_(True), w.double()
    ref = F.conv2d(xd, wd, b.double(), padding=1)
    ref_dx, = torch.autograd.grad(ref, xd, dy.double())
    ref = ref.detach()
    uf = torch.full((cout * cin * 16,), float("nan"), device="cuda")
    ug = torch.full((cout * cin * 16,), float("nan"), device="cuda")
    check(lib.tdx_pack_conv3x3_wino(dev(w).data_ptr(), uf.data_ptr(), ug.data_ptr(), cout, cin, stream()))
    xin, bd = dev(nhwc(x)), dev(b)
    out = torch.full((B, H, H, cout), float("nan"), device="cuda")
    check(lib.tdx_conv3x3_fwd_wino(xin.data_ptr(), uf.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, H, cin, cout, 0,
                                   None, None, None, stream()))
    e = rel_err(nchw(out), ref)
    print(f"winograd {B}x{H}x{H} {cin}->{cout}: rel err {e:.2e}")
    assert e < 1e-5
    # statistics partials: per tile of `rows` output pixels (in the kernel's own tile order) sum and centred M2 - checked
    # through what bn_finalize makes of them: the batch mean and biased variance per channel
    tiles = lib.tdx_conv3x3_wino_stat_tiles(B, H, H)
    rows = lib.tdx_conv3x3_wino_stat_tile_rows(B, H, H)
    assert (tiles - 1) * rows < B * H * H <= tiles * rows
    stats = torch.full((tiles, 2, cout), float("nan"), device="cuda")
    out2 = torch.full((B, H, H, cout), float("nan"), device="cuda")
    check(lib.tdx_conv3x3_fwd_wino(xin.data_ptr(), uf.data_ptr(), bd.data_ptr(), out2.data_ptr(), B, H, H, cin, cout, 4,
                                   None, None, stats.data_ptr(), stream()))
    assert torch.equal(out, out2)
    sd = stats.double().cpu()
    n = B * H * H
    counts = torch.full((tiles,), float(rows), dtype=torch.float64); counts[-1] = n - (tiles - 1) * rows
    S, Q = sd[:, 0].sum(0), sd[:, 1].sum(0)
    mean = S / n
    m2 = Q + (sd[:, 0] ** 2 / counts[:, None]).sum(0) - S * S / n
    flat = nhwc(ref).reshape(-1, cout)
    assert torch.allclose(mean, flat.mean(0), rtol=1e-4, atol=1e-5)
    assert torch.allclose(m2 / n, flat.var(0, unbiased=False), rtol=1e-4, atol=1e-6)
    # inference epilogue
    out3 = torch.full((B, H, H, cout), float("nan"), device="cuda")
    check(lib.tdx_conv3x3_fwd_wino(xin.data_ptr(), uf.data_ptr(), bd.data_ptr(), out3.data_ptr(), B, H, H, cin, cout, 2,
                                   dev(osc).data_ptr(), dev(osh).data_ptr(), None, stream()))
    ref3 = F.relu(ref * osc.double().view(1, -1, 1, 1) + osh.double().view(1, -1, 1, 1))
    assert rel_err(nchw(out3), ref3) < 1e-5
    # input gradient: the same entry on dy with the mirrored pack, channel roles swapped
    gin = torch.full((B, H, H, cin), float("nan"), device="cuda")
    check(lib.tdx_conv3x3_fwd_wino(dev(nhwc(dy)).data_ptr(), ug.data_ptr(), None, gin.data_ptr(), B, H, H, cout, cin, 0,
                                   None, None, None, stream()))
    assert rel_err(nchw(gin), ref_dx) < 1e-5
    # weight gradient by F(3x3, 2x2): both operands transformed on the fly, slabs summed by the shared reduction
    splits = lib.tdx_conv3x3_wgrad_wino_splits(B, H, H, cin, cout)
    assert splits >= 1
    slabs = torch.full((splits, cout, 9, cin), float("nan"), device="cuda")
    dwt = torch.full((cout, cin, 3, 3), float("nan"), device="cuda")
    gyd = dev(nhwc(dy))
    check(lib.tdx_conv3x3_wgrad_wino(xin.data_ptr(), gyd.data_ptr(), slabs.data_ptr(), B, H, H, cin, cout, stream()))
    check(lib.tdx_conv3x3_wgrad_reduce(slabs.data_ptr(), dwt.data_ptr(), splits, cout, cin, stream()))
    wq = w.double().clone().requires_grad_(True)
    ref_dw, = torch.autograd.grad(F.conv2d(x.double(), wq, None, padding=1), wq, dy.double())
    ew = rel_err(dwt, ref_dw)
    print(f"winograd wgrad {B}x{H}x{H} {cin}->{cout}: rel err {ew:.2e} ({splits} splits)")
    assert ew < 1e-5
    dwt2 = torch.empty_like(dwt)
    check(lib.tdx_conv3x3_wgrad_wino(xin.data_ptr(), gyd.data_ptr(), slabs.data_ptr(), B, H, H, cin, cout, stream()))
    check(lib.tdx_conv3x3_wgrad_reduce(slabs.data_ptr(), dwt2.data_ptr(), splits, cout, cin, stream()))
    assert torch.equal(dwt, dwt2)
    # inference form: K split over workgroups by the launch's own plan (any scratch size), or not at all; reproducible
    big = torch.full((max(cin // 16, 1) * B * H * H * cout,), float("nan"), device="cuda")
    outs = []
    for scr in (big, big, big[: B * H * H * cout * 2], None):
        o = torch.full((B, H, H, cout), float("nan"), device="cuda")
        check(lib.tdx_conv3x3_fwd_wino_infer(xin.data_ptr(), uf.data_ptr(), bd.data_ptr(), o.data_ptr(), B, H, H, cin, cout,
                                             dev(osc).data_ptr(), dev(osh).data_ptr(), None if scr is None else scr.data_ptr(),
                                             0 if scr is None else scr.numel(), stream()))
        assert rel_err(nchw(o), ref3) < 1e-5
        outs.append(o)
    assert torch.equal(outs[0], outs[1])


# every layer of the MNIST UNet at the reverse process's default n = 16 (diffusion.py:255), ragged M (5 x 7 x 7 = 245
# pixels: the last 64-row tile has 53 rows), the LAION widths (192, 384), a 64 x 64 map, n = 64, and K = 576 (18 K-tiles:
# fewer than the ring is deep after a 3-way split)
INFER_CASES = [(16, 28, 64, 128), (16, 28, 128, 128), (16, 14, 128, 256), (16, 14, 256, 256), (16, 7, 256, 512),
               (16, 7, 512, 512), (16, 4, 512, 512), (16, 8, 1024, 256), (16, 8, 256, 256), (16, 16, 512, 128),
               (16, 16, 128, 128), (16, 32, 256, 64), (16, 32, 64, 64), (5, 7, 256, 512), (1, 4, 64, 64),
               (3, 16, 384, 128), (2, 32, 192, 64), (1, 64, 64, 64), (64, 7, 512, 512), (3, 3, 32, 64)]


def _pack_tiled(tdx, w):
    cout, cin = w.shape[:2]
    wt = torch.full((cout * 9 * cin,), float("nan"), device="cuda")
    tdx.check(tdx.lib.tdx_pack_conv3x3_tiled(dev(w).data_ptr(), wt.data_ptr(), cout, cin, stream()))
    return wt


def test_pack_conv3x3_tiled_layout(tdx):
    """[cout/64][(ci/32)*9 + tap][64 rows][8 chunks of 4], chunk position q of row r holding logical chunk q ^ ((r >> 1) & 7)."""
    cout, cin = 128, 96
    w = torch.arange(cout * cin * 9, dtype=torch.float32).reshape(cout, cin, 3, 3)
    wt = _pack_tiled(tdx, w).cpu().reshape(cout // 64, 9 * (cin // 32), 64, 8, 4)
    for blk, kn, row, q in [(0, 0, 0, 0), (1, 26, 63, 7), (0, 13, 5, 3), (1, 9, 34, 0), (0, 8, 2, 6)]:
        c = q ^ ((row >> 1) & 7)
        ci0, tap, co = (kn // 9) * 32 + c * 4, kn % 9, blk * 64 + row
        assert torch.equal(wt[blk, kn, row, q], w[co, ci0:ci0 + 4, tap // 3, tap % 3]), (blk, kn, row, q)


@pytest.mark.parametrize("B,H,cin,cout", INFER_CASES)
def test_conv3x3_fwd_infer(tdx, B, H, cin, cout):
    """The inference convolution of the reverse process (conv3x3_ring64_kernel: 64x64 tiles on an LDS-DMA ring,
    tile-major weights, cost-model split of K) against F.conv2d: with the BN+ReLU epilogue and with bias only; split
    by its own plan, unsplit (no scratch) and at forced split counts; 3 and 4 ring stages; bitwise reproducible."""
    lib, check = tdx.lib, tdx.check
    x, w, b = _conv_inputs(B, H, cin, cout, seed=11)
    g = torch.Generator().manual_seed(12)
    osc, osh = torch.randn(cout, generator=g), torch.randn(cout, generator=g) * 0.3
    conv = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ref = F.relu(conv * osc.double().view(1, -1, 1, 1) + osh.double().view(1, -1, 1, 1))
    wt = _pack_tiled(tdx, w)
    xin, bd, oscd, oshd = dev(nhwc(x)), dev(b), dev(osc), dev(osh)
    nk = 9 * (cin // 32)
    big = torch.full((max(nk // 6, 1) * B * H * H * cout,), float("nan"), device="cuda")   # room for any split count

    def run(scratch, scale=True):
        out = torch.full((B, H, H, cout), float("nan"), device="cuda")
        check(lib.tdx_conv3x3_fwd_infer(xin.data_ptr(), wt.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, H, cin, cout,
                                        oscd.data_ptr() if scale else None, oshd.data_ptr() if scale else None,
                                        None if scratch is None else scratch.data_ptr(),
                                        0 if scratch is None else scratch.numel(), stream()))
        return out

    need = lib.tdx_conv3x3_infer_scratch_floats(B, H, H, cin, cout)
    planned = run(torch.full((max(need, 1),), float("nan"), device="cuda") if need else None)
    assert rel_err(nchw(planned), ref) < 3e-6
    assert torch.equal(planned, run(big if need else None)) or need == 0   # same plan whenever the scratch suffices
    assert rel_err(nchw(run(None)), ref) < 3e-6                            # never split without scratch
    assert rel_err(nchw(run(None, scale=False)), conv) < 3e-6              # bias-only epilogue
    for stages in (3, 4):
        with tdx.tuned(infer_stages=stages):
            for sp in (2, 3, 5, 24):
                with tdx.tuned(infer_splits=sp):
                    o1, o2 = run(big), run(big)
                assert rel_err(nchw(o1), ref) < 3e-6, (stages, sp)
                assert torch.equal(o1, o2), (stages, sp)
            assert rel_err(nchw(run(big, scale=False)), conv) < 3e-6, stages


@pytest.mark.parametrize("B,H,cin,cout,split", [(256, 4, 512, 512, True), (64, 4, 256, 256, True), (37, 4, 512, 512, True),
                                                (256, 8, 256, 256, False), (9, 7, 128, 512, True),
                                                # hybrid launches: whole rounds of tiles + K-slices of the last row tiles
                                                (256, 28, 64, 128, True), (251, 14, 128, 256, True), (256, 32, 64, 64, False)])
def test_conv3x3_fwd_train_splitk(tdx, B, H, cin, cout, split):
    """training convolutions of latency-bound shapes (the UNet bottleneck at the benchmarked batch): K split over
    64x64 workgroups, then ONE launch reduces the partials in a fixed order, adds the bias and writes the same
    BatchNorm statistics partials the unsplit epilogue writes.  Also the plain (input-gradient) form."""
    x, w, b = _conv_inputs(B, H, cin, cout, seed=11)
    ref = F.conv2d(x, w, b, padding=1)
    wf, _ = _pack(tdx, w)
    xin, bd = dev(nhwc(x)), dev(b)
    hybrid = B * H * H > 16384      # the big shapes exercise the hybrid launch (off by default: knob conv_hybrid)
    with tdx.tuned(**({"conv_hybrid": 1} if hybrid else {})):
        _fwd_train_checks(tdx, x, w, b, ref, wf, xin, bd, B, H, cin, cout, split)


def _fwd_train_checks(tdx, x, w, b, ref, wf, xin, bd, B, H, cin, cout, split):
    need = tdx.lib.tdx_conv3x3_train_scratch_floats(B, H, H, cin, cout)
    assert (need > 0) == split
    scratch = torch.full((max(need, 1),), float("nan"), device="cuda")
    tiles = tdx.lib.tdx_conv3x3_stat_tiles(B, H, H, cin, cout)
    rows = tdx.lib.tdx_conv3x3_stat_tile_rows(B, H, H, cin, cout)
    outs = []
    for _ in range(2):
        out = torch.full((B, H, H, cout), float("nan"), device="cuda")
        stats = torch.full((tiles, 2, cout), float("nan"), device="cuda")
        tdx.check(tdx.lib.tdx_conv3x3_fwd_train(xin.data_ptr(), wf.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, H, cin,
                                                cout, 4, stats.data_ptr(), scratch.data_ptr(), need, stream()))
        outs.append((out, stats))
    out, stats = outs[0]
    assert rel_err(nchw(out), ref) < 3e-6
    assert torch.equal(out, outs[1][0]) and torch.equal(stats, outs[1][1])   # fixed order: reproducible
    flat = nhwc(ref).reshape(-1, cout).double()
    for ti in range(tiles):
        blk = flat[ti * rows:(ti + 1) * rows]
        assert torch.allclose(stats[ti, 0].double().cpu(), blk.sum(0), rtol=1e-4, atol=1e-3)
        assert torch.allclose(stats[ti, 1].double().cpu(), (blk - blk.mean(0)).pow(2).sum(0), rtol=1e-4, atol=1e-3)
    # no statistics, no bias: the form the input gradient uses
    out0 = torch.full((B, H, H, cout), float("nan"), device="cuda")
    tdx.check(tdx.lib.tdx_conv3x3_fwd_train(xin.data_ptr(), wf.data_ptr(), None, out0.data_ptr(), B, H, H, cin, cout, 0,
                                            None, scratch.data_ptr(), need, stream()))
    assert rel_err(nchw(out0), F.conv2d(x, w, None, padding=1)) < 3e-6
    # a scratch that is too small uses fewer splits or none
    small = torch.empty(max(need // 3, 1), device="cuda")
    out2 = torch.full((B, H, H, cout), float("nan"), device="cuda")
    tdx.check(tdx.lib.tdx_conv3x3_fwd_train(xin.data_ptr(), wf.data_ptr(), bd.data_ptr(), out2.data_ptr(), B, H, H, cin, cout,
                                            4, stats.data_ptr(), small.data_ptr(), small.numel(), stream()))
    assert rel_err(nchw(out2), ref) < 3e-6
    assert tdx.lib.tdx_conv3x3_fwd_train(xin.data_ptr(), wf.data_ptr(), bd.data_ptr(), out2.data_ptr(), B, H, H, cin, cout,
                                         2, None, None, 0, stream()) != 0      # BN+ReLU epilogue is not a training flag


@pytest.mark.parametrize("B,H,cin,cout", CONV_CASES)
def test_conv3x3_dgrad_and_wgrad(tdx, B, H, cin, cout):
    x, w, b = _conv_inputs(B, H, cin, cout, seed=2)
    x.requires_grad_(True); w.requires_grad_(True)
    y = F.conv2d(x, w, b, padding=1)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(3))
    y.backward(g)
    _, wd = _pack(tdx, w.detach())
    gd = dev(nhwc(g))
    gin = torch.empty((B, H, H, cin), device="cuda")
    tdx.check(tdx.lib.tdx_conv3x3_fwd(gd.data_ptr(), wd.data_ptr(), None, gin.data_ptr(), B, H, H, cout, cin, 0,
                                      None, None, None, None, None, stream()))
    assert rel_err(nchw(gin), x.grad) < 2e-6
    splits = tdx.lib.tdx_conv3x3_wgrad_splits(B, H, H, cin, cout)
    slabs = torch.full((splits, cout, 9, cin), float("nan"), device="cuda")
    dw = torch.empty((cout, cin, 3, 3), device="cuda")
    tdx.check(tdx.lib.tdx_conv3x3_wgrad(dev(nhwc(x.detach())).data_ptr(), gd.data_ptr(), slabs.data_ptr(), B, H, H,
                                        cin, cout, 0, None, None, stream()))
    tdx.check(tdx.lib.tdx_conv3x3_wgrad_reduce(slabs.data_ptr(), dw.data_ptr(), splits, cout, cin, stream()))
    assert rel_err(dw, w.grad) < 3e-6


def test_conv3x3_wgrad_bnrelu_input(tdx):
    B, H, cin, cout = 3, 14, 128, 256
    x, w, b = _conv_inputs(B, H, cin, cout, seed=4)
    g = torch.Generator().manual_seed(6)
    isc, ish = torch.randn(cin, generator=g), torch.randn(cin, generator=g) * 0.3
    a = F.relu(x * isc.view(1, -1, 1, 1) + ish.view(1, -1, 1, 1))
    w.requires_grad_(True)
    y = F.conv2d(a, w, b, padding=1)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    splits = tdx.lib.tdx_conv3x3_wgrad_splits(B, H, H, cin, cout)
    slabs = torch.empty((splits, cout, 9, cin), device="cuda")
    dw = torch.empty((cout, cin, 3, 3), device="cuda")
    tdx.check(tdx.lib.tdx_conv3x3_wgrad(dev(nhwc(x)).data_ptr(), dev(nhwc(gy)).data_ptr(), slabs.data_ptr(), B, H, H,
                                        cin, cout, 1, dev(isc).data_ptr(), dev(ish).data_ptr(), stream()))
    tdx.check(tdx.lib.tdx_conv3x3_wgrad_reduce(slabs.data_ptr(), dw.data_ptr(), splits, cout, cin, stream()))
    assert rel_err(dw, w.grad) < 3e-6


@pytest.mark.parametrize("training", [1, 0])
def test_bn_finalize_and_backward(tdx, training):
    """BatchNorm2d train/eval forward statistics + BN/ReLU backward vs autograd."""
    B, H, Cc = 6, 14, 128
    g = torch.Generator().manual_seed(11)
    # large per-channel offsets: E[y^2]-E[y]^2 would lose ~4 digits here
    y = torch.randn(B, Cc, H, H, generator=g) * 0.3 + 30.0 * torch.randn(1, Cc, 1, 1, generator=g)
    gamma = (1 + 0.1 * torch.randn(Cc, generator=g)).requires_grad_(True)
    beta = (0.1 * torch.randn(Cc, generator=g)).requires_grad_(True)
    rm, rv = torch.randn(Cc, generator=g) * 0.1, 1 + torch.rand(Cc, generator=g)
    nbt = torch.tensor(3)
    yy = y.clone().requires_grad_(True)
    rm_ref, rv_ref, nbt_ref = rm.clone(), rv.clone(), nbt.clone()
    a = F.relu(R.batchnorm2d(yy, gamma, beta, rm_ref, rv_ref, bool(training), nbt_ref))
    ga = torch.randn(a.shape, generator=g)
    a.backward(ga)
    # ---- device
    yd = dev(nhwc(y))
    rows = B * H * H
    # emulate the conv epilogue partials: tiles of 500 rows (last one ragged)
    tile_rows = 500
    ntile = (rows + tile_rows - 1) // tile_rows
    y2 = yd.view(rows, Cc).double()
    stats = torch.stack([torch.stack([blk.sum(0), (blk - blk.mean(0)).pow(2).sum(0)])
                         for blk in y2.split(tile_rows)]).float().contiguous()
    sc, sh, mu, rs = (torch.empty(Cc, device="cuda") for _ in range(4))
    rmd, rvd, nbtd = dev(rm), dev(rv), nbt.cuda()
    tdx.check(tdx.lib.tdx_bn_finalize(stats.data_ptr(), ntile, tile_rows, rows, Cc, dev(gamma.detach()).data_ptr(),
                                      dev(beta.detach()).data_ptr(), rmd.data_ptr(), rvd.data_ptr(), nbtd.data_ptr(),
                                      sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), rs.data_ptr(), training, stream()))
    act = F.relu(yd * sc + sh)
    # y*scale+shift (ATen's own CPU form) cancels |mean|*scale against the result: with the
    # |mean|/std ~ 100 of this test that costs ~2 digits relative to (y-mean)*rstd*w+b
    assert rel_err(nchw(act), a.detach()) < 2e-5
    if training:
        assert torch.allclose(rmd.cpu(), rm_ref, rtol=1e-5, atol=1e-6)
        assert torch.allclose(rvd.cpu(), rv_ref, rtol=1e-5, atol=1e-6)
        assert int(nbtd) == int(nbt_ref) == 4
    else:
        assert torch.equal(rmd.cpu(), rm) and int(nbtd) == 3
    gd = dev(nhwc(ga))
    n_scr = tdx.lib.tdx_bn_relu_bwd_scratch_floats(rows, Cc)
    scr = torch.empty(n_scr, device="cuda")
    dg, db, dbias = (torch.empty(Cc, device="cuda") for _ in range(3))
    tdx.check(tdx.lib.tdx_bn_relu_bwd(gd.data_ptr(), yd.data_ptr(), rows, Cc, sc.data_ptr(), sh.data_ptr(),
                                      mu.data_ptr(), rs.data_ptr(), dev(gamma.detach()).data_ptr(), dg.data_ptr(),
                                      db.data_ptr(), dbias.data_ptr(), scr.data_ptr(), training, stream()))
    # (|mean|/std ~ 100 in this test: xhat carries ~1e-5 relative rounding on both sides)
    assert rel_err(nchw(gd), yy.grad) < 2e-5
    assert rel_err(dg, gamma.grad) < 2e-5
    assert rel_err(db, beta.grad) < 2e-5
    ref_dbias = yy.grad.sum((0, 2, 3))
    if training:
        assert dbias.abs().max().item() == 0.0 and ref_dbias.abs().max().item() < 1e-3
    else:
        assert rel_err(dbias, ref_dbias) < 5e-6


@pytest.mark.parametrize("H,Cc", [(28, 128), (14, 256), (7, 512), (5, 64)])
def test_maxpool_ceil_fwd_bwd(tdx, H, Cc):
    B = 3
    g = torch.Generator().manual_seed(H)
    y = torch.randn(B, Cc, H, H, generator=g)
    sc, sh = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g) * 0.2
    a = F.relu(y * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).requires_grad_(True)
    ref = R.maxpool2_ceil(a)
    assert torch.equal(ref, F.max_pool2d(a, 2, ceil_mode=True))
    Ho = (H + 1) // 2
    yd = dev(nhwc(y))
    out = torch.empty((B, Ho, Ho, Cc), device="cuda")
    tdx.check(tdx.lib.tdx_maxpool2_ceil_fwd(yd.data_ptr(), dev(sc).data_ptr(), dev(sh).data_ptr(), out.data_ptr(),
                                            B, H, H, Cc, stream()))
    assert rel_err(nchw(out), ref.detach()) < 1e-6
    go = torch.randn(ref.shape, generator=g)
    skip = torch.randn(a.shape, generator=g)
    # many exact ties (zeros after ReLU): torch routes to the first maximum
    F.max_pool2d(a, 2, ceil_mode=True).backward(go)
    gin = torch.empty((B, H, H, Cc), device="cuda")
    tdx.check(tdx.lib.tdx_maxpool2_ceil_bwd(yd.data_ptr(), dev(sc).data_ptr(), dev(sh).data_ptr(),
                                            dev(nhwc(go)).data_ptr(), dev(nhwc(skip)).data_ptr(), gin.data_ptr(),
                                            B, H, H, Cc, stream()))
    assert torch.allclose(nchw(gin).cpu(), a.grad + skip, rtol=1e-6, atol=1e-6)


RESIZES = [(4, 8, 512), (7, 8, 512), (8, 16, 256), (14, 16, 256), (16, 32, 128), (28, 32, 128), (32, 28, 64)]


@pytest.mark.parametrize("hi,ho,Cc", RESIZES)
def test_bilinear_align_corners_fwd_bwd(tdx, hi, ho, Cc):
    """The 7 resizes of the UNet (diffusion.py:135-159), with BN+ReLU on load,
    broadcast addend and channel-slice destination."""
    B = 2
    g = torch.Generator().manual_seed(hi * 100 + ho)
    y = torch.randn(B, Cc, hi, hi, generator=g)
    sc, sh = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g) * 0.2
    add = torch.randn(B, Cc, generator=g)
    a = (F.relu(y * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) + add.view(B, Cc, 1, 1)).requires_grad_(True)
    ref = F.interpolate(a, size=(ho, ho), mode="bilinear", align_corners=True)
    assert rel_err(R.bilinear_ac(a.detach(), (ho, ho)), ref.detach()) < 1e-7
    cs, co = 2 * Cc, Cc  # write into the upper channel half of a wider buffer
    out = torch.zeros((B, ho, ho, cs), device="cuda")
    tdx.check(tdx.lib.tdx_bilinear_ac_fwd(dev(nhwc(y)).data_ptr(), dev(sc).data_ptr(), dev(sh).data_ptr(),
                                          dev(add).data_ptr(), out.data_ptr(), B, hi, hi, ho, ho, Cc, cs, co, stream()))
    assert rel_err(nchw(out[..., co:]), ref.detach()) < 1e-6
    assert out[..., :co].abs().max().item() == 0.0
    go = torch.randn(ref.shape, generator=g)
    ref.backward(go)
    gbuf = torch.zeros((B, ho, ho, cs), device="cuda")
    gbuf[..., co:] = dev(nhwc(go))
    gin = torch.empty((B, hi, hi, Cc), device="cuda")
    tdx.check(tdx.lib.tdx_bilinear_ac_bwd(gbuf.data_ptr(), gin.data_ptr(), B, hi, hi, ho, ho, Cc, cs, co, stream()))
    assert rel_err(nchw(gin), a.grad) < 2e-6


def test_mse_and_adam(tdx):
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(64, 784, generator=g), torch.randn(64, 784, generator=g)
    ar = a.clone().requires_grad_(True)
    loss = F.mse_loss(ar, b); loss.backward()
    lo, da = torch.empty(1, device="cuda"), torch.empty(a.shape, device="cuda")
    tdx.check(tdx.lib.tdx_mse_loss(dev(a).data_ptr(), dev(b).data_ptr(), lo.data_ptr(), da.data_ptr(), 1.0,
                                   a.numel(), stream()))
    assert abs(lo.item() - loss.item()) < 1e-6 * loss.item()
    assert rel_err(da, ar.grad) < 1e-6
    # Adam vs torch.optim.Adam, 3 steps
    p = torch.randn(10000, generator=g)
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-3)
    pd, m, v = dev(p), torch.zeros(10000, device="cuda"), torch.zeros(10000, device="cuda")
    for step in range(1, 4):
        gr = torch.randn(10000, generator=g)
        pr.grad = gr.clone(); opt.step()
        tdx.check(tdx.lib.tdx_adam_step(pd.data_ptr(), dev(gr).data_ptr(), m.data_ptr(), v.data_ptr(), 10000,
                                        1e-3, 0.9, 0.999, 1e-8, step, 1.0, stream()))
    assert (pd.cpu() - pr.detach()).abs().max().item() < 2e-6


@pytest.mark.parametrize("gscale", [1.0, 0.25])
@pytest.mark.parametrize("hyper_form", [False, True])
@pytest.mark.parametrize("gnorm,max_norm", [(37.5, 10.0), (3.0, 10.0), (10.0, 10.0)])
def test_adam_step_clip_three_steps(tdx, gnorm, max_norm, hyper_form, gscale):
    """tdx_adam_step_clip = torch.nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.Adam.step()
    (conditional_diffusion_laion.py:469-472) on the flat gradient, over THREE steps with gradients of a
    known norm (clip active: 37.5 > 10; inactive: 3 < 10; on the edge: 10, where torch's
    max_norm / (norm + 1e-6) < 1 still scales), comparing exp_avg, exp_avg_sq and the parameters.  One step
    from zero moments would not do: Adam's first update lr*g/(|g|+eps) is invariant to a uniform scale of
    g, so a wrong clip coefficient would pass (the moments and the later steps are not invariant).
    `gscale` is the 1/world of the data-parallel mean: the reference then clips the AVERAGED gradient.
    `hyper_form`: step scalars read from device memory (the graph-capturable form)."""
    import math

    n = 70001   # not a multiple of the block size
    g = torch.Generator().manual_seed(int(gnorm * 10) + int(hyper_form))
    p0 = torch.randn(n, generator=g)
    # several "parameters" on the torch side (the norm is taken over all of them together)
    cuts = [0, 1000, 1001, 40000, n]
    ref = [p0[a:b].clone().requires_grad_(True) for a, b in zip(cuts[:-1], cuts[1:])]
    lr, b1, b2, eps = 1e-4, 0.9, 0.999, 1e-8
    opt = torch.optim.Adam(ref, lr=lr, betas=(b1, b2), eps=eps)
    pd = dev(p0.clone())
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    scratch = torch.empty(tdx.lib.tdx_adam_clip_scratch_bytes(), dtype=torch.uint8, device="cuda")
    hyper = torch.zeros(3, device="cuda")
    for step in range(1, 4):
        gr = torch.randn(n, generator=g)
        # the averaged gradient has norm gnorm * (1, 1.7, 0.4): the 3-norm case is clipped in step 2 only...
        gr = gr * (gnorm * (1.0, 1.7, 0.4)[step - 1] / gr.norm()) / gscale
        for r, a, b in zip(ref, cuts[:-1], cuts[1:]):
            r.grad = (gr[a:b] * gscale).clone()
        total = torch.nn.utils.clip_grad_norm_(ref, max_norm=max_norm)
        assert abs(total.item() - gnorm * (1.0, 1.7, 0.4)[step - 1]) < 1e-3 * gnorm
        opt.step()
        if hyper_form:
            bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
            hyper.copy_(torch.tensor([lr / bc1, 1.0 / math.sqrt(bc2), gscale], dtype=torch.float32))
            torch.cuda.synchronize()
        tdx.check(tdx.lib.tdx_adam_step_clip(pd.data_ptr(), dev(gr).data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1,
                                             b2, eps, step, gscale, max_norm, hyper.data_ptr() if hyper_form else None,
                                             scratch.data_ptr(), stream()))
        st = [opt.state[r] for r in ref]
        m_ref = torch.cat([s["exp_avg"] for s in st])
        v_ref = torch.cat([s["exp_avg_sq"] for s in st])
        p_ref = torch.cat([r.detach() for r in ref])
        # moments: a coefficient off by 2x would show as a 2x / 4x error.  The bound is the rounding of the
        # NORM: torch sums the squares in fp32 (measured: its coefficient is 6e-6 off the double-precision
        # one over 70 k elements), the kernel in double
        assert rel_err(m, m_ref) < 3e-5, (step, rel_err(m, m_ref))
        assert rel_err(v, v_ref) < 6e-5, (step, rel_err(v, v_ref))
        assert (pd.cpu() - p_ref).abs().max().item() < 2e-6, step


def test_adam_step_clip_detects_wrong_coefficient(tdx):
    """Sensitivity of the gate above: the same three steps against a torch run whose clip threshold is
    DOUBLED must fail the moment comparison by a wide margin (so a kernel with a wrong coefficient cannot
    pass test_adam_step_clip_three_steps)."""
    n = 5000
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=g)
    ref = [p0.clone().requires_grad_(True)]
    opt = torch.optim.Adam(ref, lr=1e-4)
    pd = dev(p0.clone())
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    scratch = torch.empty(tdx.lib.tdx_adam_clip_scratch_bytes(), dtype=torch.uint8, device="cuda")
    for step in range(1, 4):
        gr = torch.randn(n, generator=g)
        gr = gr * (40.0 / gr.norm())
        ref[0].grad = gr.clone()
        torch.nn.utils.clip_grad_norm_(ref, max_norm=20.0)   # the kernel is given 10.0
        opt.step()
        tdx.check(tdx.lib.tdx_adam_step_clip(pd.data_ptr(), dev(gr).data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-4,
                                             0.9, 0.999, 1e-8, step, 1.0, 10.0, None, scratch.data_ptr(), stream()))
    s = opt.state[ref[0]]
    assert rel_err(m, s["exp_avg"]) > 0.3 and rel_err(v, s["exp_avg_sq"]) > 0.5


def test_u8_gather_normalize_bit_exact(tdx):
    """ToTensor + Normalize((0.5,),(0.5,)) (diffusion.py:202-204) fused with the gather."""
    from tiny_diffusion_amd.data import DeviceImageDataset

    g = torch.Generator().manual_seed(3)
    imgs = torch.randint(0, 256, (500, 28, 28), generator=g, dtype=torch.uint8)
    imgs[0].fill_(0); imgs[1].fill_(255)
    ds = DeviceImageDataset(imgs)
    idx = torch.randint(0, 500, (77,), generator=g)
    got = ds.batch(idx.cuda())
    ref = imgs[idx].float().div(255).sub(0.5).div(0.5).unsqueeze(1)   # the reference's transforms
    assert got.shape == (77, 1, 28, 28) and torch.equal(got.cpu(), ref)
    allb = ds.batch()
    assert torch.equal(allb.cpu(), imgs.float().div(255).sub(0.5).div(0.5).unsqueeze(1))
    assert allb.min().item() == -1.0 and allb.max().item() == 1.0
    seen = torch.cat([b for b in ds.epoch(128, shuffle=True)])
    assert seen.shape[0] == 500
    # a shuffled epoch visits every image exactly once: compare per-image checksums as multisets
    key = lambda t: torch.sort((t.double().view(t.shape[0], -1) * torch.arange(1, 785, device=t.device)).sum(1)).values
    assert torch.equal(key(seen), key(allb))
    with pytest.raises(IndexError):
        ds.batch(torch.tensor([500]).cuda())


@pytest.mark.parametrize("B,H,cin,cout", [(3, 14, 128, 256), (2, 28, 64, 128)])
def test_conv3x3_dgrad_entry(tdx, B, H, cin, cout):
    """tdx_conv3x3_dgrad (the name SURVEY.md 8(b) lists) against autograd."""
    x, w, b = _conv_inputs(B, H, cin, cout, seed=21)
    x.requires_grad_(True)
    y = F.conv2d(x, w, b, padding=1)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(22))
    y.backward(g)
    _, wd = _pack(tdx, w)
    gd = dev(nhwc(g))
    dx = torch.full((B, H, H, cin), float("nan"), device="cuda")
    tdx.check(tdx.lib.tdx_conv3x3_dgrad(gd.data_ptr(), wd.data_ptr(), dx.data_ptr(), B, H, H, cin, cout, stream()))
    assert rel_err(nchw(dx), x.grad) < 2e-6


def test_bn_apply_relu_fwd_bit_exact(tdx):
    g = torch.Generator().manual_seed(23)
    rows, Cc = 5 * 14 * 14, 128
    y = torch.randn(rows, Cc, generator=g)
    sc, sh = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g) * 0.3
    out = torch.full((rows, Cc), float("nan"), device="cuda")
    tdx.check(tdx.lib.tdx_bn_apply_relu_fwd(dev(y).data_ptr(), out.data_ptr(), rows, Cc, dev(sc).data_ptr(),
                                            dev(sh).data_ptr(), stream()))
    ref = torch.relu(torch.addcmul(sh, y, sc))          # one fma per element, as the kernel
    assert (out.cpu() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
    assert tdx.lib.tdx_bn_apply_relu_fwd(None, out.data_ptr(), rows, Cc, None, None, stream()) != 0


@pytest.mark.parametrize("cond", [False, True])
def test_time_mlp_fwd_bwd(tdx, cond):
    """Time MLP + class embedding + the three 1x1 projections on their own (diffusion.py:21-25,
    105-113, 130-132; conditional_diffusion.py:121-125) against torch autograd on the CPU."""
    from tiny_diffusion_amd.unet import param_slot_names

    B, TD, ncls = 37, 256, 10
    g = torch.Generator().manual_seed(31 + cond)
    names = param_slot_names(cond)
    shapes = {"time_embedding.0.weight": (TD, 1), "time_embedding.0.bias": (TD,),
              "time_embedding.2.weight": (TD, TD), "time_embedding.2.bias": (TD,),
              "class_embedding.weight": (ncls, TD),
              "time_proj1.weight": (128, TD, 1, 1), "time_proj1.bias": (128,),
              "time_proj2.weight": (256, TD, 1, 1), "time_proj2.bias": (256,),
              "time_proj3.weight": (512, TD, 1, 1), "time_proj3.bias": (512,)}
    P = {k: (torch.randn(v, generator=g) * (0.002 if k == "time_embedding.0.weight" else 0.06)).requires_grad_(True)
         for k, v in shapes.items() if cond or k != "class_embedding.weight"}
    t = torch.randint(0, 1000, (B,), generator=g)
    y = torch.randint(0, ncls, (B,), generator=g) if cond else None
    pre = t.float().unsqueeze(1) @ P["time_embedding.0.weight"].t() + P["time_embedding.0.bias"]
    emb = F.silu(pre) @ P["time_embedding.2.weight"].t() + P["time_embedding.2.bias"]
    if cond:
        emb = emb + P["class_embedding.weight"][y]
    outs = [emb @ P[f"time_proj{k}.weight"].flatten(1).t() + P[f"time_proj{k}.bias"] for k in (1, 2, 3)]
    gts = [torch.randn(o.shape, generator=g) for o in outs]
    sum((o * gt).sum() for o, gt in zip(outs, gts)).backward()

    pd = {k: dev(v.detach()) for k, v in P.items()}
    gd = {k: torch.full_like(v, float("nan")) for k, v in pd.items()}
    ptab = (C.c_void_p * len(names))(*[pd[n].data_ptr() if n in pd else None for n in names])
    gtab = (C.c_void_p * len(names))(*[gd[n].data_ptr() if n in gd else None for n in names])
    td, yd = dev(t), (dev(y) if cond else None)
    pre_d, emb_d = torch.empty(B, TD, device="cuda"), torch.empty(B, TD, device="cuda")
    o_d = [torch.empty(B, c, device="cuda") for c in (128, 256, 512)]
    tdx.check(tdx.lib.tdx_time_mlp_fwd(td.data_ptr(), yd.data_ptr() if cond else None, ptab, pre_d.data_ptr(),
                                       emb_d.data_ptr(), o_d[0].data_ptr(), o_d[1].data_ptr(), o_d[2].data_ptr(),
                                       B, stream()))
    assert rel_err(emb_d, emb.detach()) < 2e-6
    for got, ref in zip(o_d, outs):
        assert rel_err(got, ref.detach()) < 2e-6
    scratch = torch.empty((3 * TD + 1) * B, device="cuda")
    gt_d = [dev(x) for x in gts]
    tdx.check(tdx.lib.tdx_time_mlp_bwd(td.data_ptr(), yd.data_ptr() if cond else None, ptab, gtab, pre_d.data_ptr(),
                                       emb_d.data_ptr(), gt_d[0].data_ptr(), gt_d[1].data_ptr(), gt_d[2].data_ptr(),
                                       scratch.data_ptr(), B, ncls if cond else 0, stream()))
    for k, v in P.items():
        assert rel_err(gd[k], v.grad) < 1e-5, k


@pytest.mark.parametrize("B,H,cin,cout", [(3, 28, 1, 64), (2, 32, 4, 32), (37, 28, 1, 64), (5, 64, 4, 32), (21, 7, 1, 64),
                                          (4, 9, 4, 32)])
def test_initial_conv_fwd_bwd(tdx, B, H, cin, cout):
    """diffusion.py:28 / conditional_diffusion_laion.py:244 on the MFMA (thin operand gathered from NCHW): forward and
    the weight / bias gradients against F.conv2d; pixel counts that are not multiples of the 128-pixel forward
    tile or of the 512-pixel gradient chunk, odd image sizes."""
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn(B, cin, H, H, generator=g)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * 0.3).requires_grad_(True)
    b = (torch.randn(cout, generator=g) * 0.1).requires_grad_(True)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    gout = torch.randn(B, H, H, 64, generator=g)   # all 64 stored channels carry a gradient; only `cout` are real
    ref.backward(nchw(gout)[:, :cout].double())
    out = torch.full((B, H, H, 64), float("nan"), device="cuda")
    tdx.check(tdx.lib.tdx_initial_conv_forward(dev(x).data_ptr(), dev(w.detach()).data_ptr(), dev(b.detach()).data_ptr(),
                                               out.data_ptr(), B, H, H, cin, cout, stream()))
    got = nchw(out)
    assert rel_err(got[:, :cout], ref.detach()) < 2e-6
    assert bool((got[:, cout:] == 0).all())
    scratch = torch.full((tdx.lib.tdx_edge_conv_wgrad_scratch_floats(B, H, H),), float("nan"), device="cuda")
    dw = torch.full((cout, cin, 3, 3), float("nan"), device="cuda")
    db = torch.full((cout,), float("nan"), device="cuda")
    tdx.check(tdx.lib.tdx_initial_conv_backward(dev(x).data_ptr(), dev(gout).data_ptr(), dw.data_ptr(), db.data_ptr(),
                                                scratch.data_ptr(), B, H, H, cin, cout, stream()))
    assert rel_err(dw, w.grad) < 3e-6 and rel_err(db, b.grad) < 3e-6
    assert tdx.lib.tdx_initial_conv_forward(dev(x).data_ptr(), dev(w.detach()).data_ptr(), None, out.data_ptr(), B, H, H,
                                            2, 64, stream()) != 0


@pytest.mark.parametrize("B,H,cout", [(3, 28, 1), (2, 32, 4), (37, 28, 1), (5, 64, 4), (21, 7, 1), (4, 9, 4)])
def test_final_conv_fwd_bwd(tdx, B, H, cout):
    """diffusion.py:98 / conditional_diffusion_laion.py:296: forward (NCHW out), input gradient (mirrored taps on
    the MFMA), weight and bias gradients against F.conv2d."""
    g = torch.Generator().manual_seed(B * 100 + H + 7)
    x = torch.randn(B, 64, H, H, generator=g, requires_grad=True)
    w = (torch.randn(cout, 64, 3, 3, generator=g) * 0.05).requires_grad_(True)
    b = (torch.randn(cout, generator=g) * 0.1).requires_grad_(True)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    gout = torch.randn(B, cout, H, H, generator=g)
    ref.backward(gout.double())
    xin = dev(nhwc(x.detach()))
    out = torch.full((B, cout, H, H), float("nan"), device="cuda")
    tdx.check(tdx.lib.tdx_final_conv_forward(xin.data_ptr(), dev(w.detach()).data_ptr(), dev(b.detach()).data_ptr(),
                                             out.data_ptr(), B, H, H, cout, stream()))
    assert rel_err(out, ref.detach()) < 2e-6
    scratch = torch.full((tdx.lib.tdx_edge_conv_wgrad_scratch_floats(B, H, H),), float("nan"), device="cuda")
    gin = torch.full((B, H, H, 64), float("nan"), device="cuda")
    dw = torch.full((cout, 64, 3, 3), float("nan"), device="cuda")
    db = torch.full((cout,), float("nan"), device="cuda")
    tdx.check(tdx.lib.tdx_final_conv_backward(xin.data_ptr(), dev(gout).data_ptr(), dev(w.detach()).data_ptr(),
                                              gin.data_ptr(), dw.data_ptr(), db.data_ptr(), scratch.data_ptr(), B, H, H,
                                              cout, stream()))
    assert rel_err(nchw(gin), x.grad) < 3e-6
    assert rel_err(dw, w.grad) < 3e-6 and rel_err(db, b.grad) < 3e-6


@pytest.mark.parametrize("B,H,cin,cout", [(3, 28, 1, 64), (2, 32, 4, 32), (1, 7, 1, 64), (2, 40, 4, 32)])
def test_initial_conv_input_grad(tdx, B, H, cin, cout):
    """tdx_initial_conv_input_grad = d/dx of nn.Conv2d(cin, cout, 3, padding=1) (diffusion.py:28, 116) given the
    gradient of its (channels-last, 64 stored channels) output."""
    g = torch.Generator().manual_seed(B * H + cin)
    x = torch.randn(B, cin, H, H, generator=g, requires_grad=True)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.3
    go = torch.randn(B, cout, H, H, generator=g)
    F.conv2d(x, w, None, padding=1).backward(go)
    gfat = torch.full((B, H, H, 64), 7.0)          # padding channels hold junk: they must not leak in
    gfat[..., :cout] = nhwc(go)
    gx = torch.full((B, cin, H, H), float("nan"), device="cuda")
    tdx.check(tdx.lib.tdx_initial_conv_input_grad(dev(gfat).data_ptr(), dev(w).data_ptr(), gx.data_ptr(), B, H, H, cin,
                                                  cout, stream()))
    assert rel_err(gx, x.grad) < 2e-6
