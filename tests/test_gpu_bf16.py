"""GPU: the opt-in bf16 mode (BASELINE.json configs[3]/[4] name bf16; the reference itself is
fp32-only, SURVEY.md 0, so there is no reference behaviour to match bit for bit).

Arithmetic: the three 3x3-convolution GEMMs (forward, input gradient, weight gradient) run on
v_mfma_f32_32x32x16_bf16 with operands rounded to bf16 (nearest even) and fp32 accumulation.  Since round 3 the
activation tensors and activation gradients are also STORED in bf16 (every HBM-bound kernel widens on load, computes
in fp32 and rounds on store: io16.h); BatchNorm statistics / scale / shift, the time MLP, the loss, parameter
gradients and Adam stay fp32.  The kernel tests below call the fp32-tensor entry points (bf16 operands only).

Tolerances stated here:
  * kernels: against the SAME arithmetic on the CPU (operands rounded to bf16, fp64 accumulation):
    relative error <= 2e-5 (fp32 accumulation order only);
  * whole network (storage mode): pinned to the REFERENCE under torch's own bf16 autocast
    (tests/golden/bf16_autocast.npz, written by tools/make_golden.py from the reference's modules on the inputs of
    the fp32 fixtures; tests/parity_helpers.py::AutocastYardstick, constant BF16_K = 1): eps_hat MSE against the
    reference's fp32 vectors <= the MSE of the reference's autocast run (train / eval mode each), 1 - cosine of the
    parameter gradients with the fp32 oracle's <= the reference's autocast figure, worst parameter and median, and
    the loss within twice the reference's own shift (floor 0.5 %).  Measured (round 3 -> the reference's figure):
    eps_hat MSE MNIST B = 64 7.5e-5 (4.3e-4), LAION 32x32 6.8e-5 (1.0e-4), 64x64 at B = 2 3.8e-4 (4.8e-4);
    worst / median cosine 0.989 / 0.9998 (0.985 / 0.9996), 0.962 / 0.9987 (0.952 / 0.9984), 0.940 / 0.9906
    (0.913 / 0.9879)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oracle import ref_laion as RL  # noqa: E402
from oracle.weights import make_state_dict, make_state_dict_laion  # noqa: E402
from parity_helpers import AutocastYardstick, is_pre_bn_bias  # noqa: E402


@pytest.fixture(scope="module")
def tdx():
    import tiny_diffusion_amd._lib as L

    return L


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float64)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-30)).item()


def st():
    return torch.cuda.current_stream().cuda_stream


BF16_CASES = [
    # B, H, cin, cout: every tile template (128x128 / 128x64 forward; 128x128, 128x64, 64x128, 64x64 wgrad),
    # ragged M, the LAION widths (192, 384) and a 64x64 map
    (4, 28, 64, 128), (3, 14, 128, 256), (5, 7, 256, 512), (7, 4, 512, 512), (3, 8, 1024, 256),
    (2, 16, 384, 128), (2, 32, 192, 64), (2, 32, 64, 64), (1, 64, 64, 64), (33, 8, 128, 128),
]


@pytest.mark.parametrize("B,H,cin,cout", BF16_CASES)
def test_bf16_conv_fwd_dgrad_wgrad(tdx, B, H, cin, cout):
    lib, check = tdx.lib, tdx.check
    g = torch.Generator().manual_seed(B * 1000 + H)
    x = torch.randn(B, cin, H, H, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    dy = torch.randn(B, cout, H, H, generator=g)
    # the same arithmetic on the host: bf16-rounded operands, exact products, fp64 sums
    xr, wr, dyr = bf16_round(x), bf16_round(w), bf16_round(dy)
    xr.requires_grad_(True); wr.requires_grad_(True)
    ref = F.conv2d(xr, wr, b.double(), padding=1)
    ref_dw, = torch.autograd.grad(ref, wr, dyr, retain_graph=True)   # weight gradient: dy and x rounded
    ref_dx, = torch.autograd.grad(ref, xr, dyr)                      # input gradient: dy and w rounded

    wd = w.cuda().contiguous()
    wf16 = torch.empty(cout * 9 * cin, dtype=torch.bfloat16, device="cuda")
    wg16 = torch.empty(cout * 9 * cin, dtype=torch.bfloat16, device="cuda")
    check(lib.tdx_pack_conv3x3_bf16(wd.data_ptr(), wf16.data_ptr(), wg16.data_ptr(), cout, cin, st()))
    assert torch.equal(wf16.view(cout, 9, cin).float().cpu(), w.permute(0, 2, 3, 1).reshape(cout, 9, cin).bfloat16().float())
    xin = nhwc(x).cuda()
    out = torch.full((B, H, H, cout), float("nan"), device="cuda")
    M = B * H * H
    rows = lib.tdx_conv3x3_bf16_stat_tile_rows()
    tiles = -(-M // rows)
    stats = torch.full((tiles, 2, cout), float("nan"), device="cuda")
    bd = b.cuda()
    check(lib.tdx_conv3x3_fwd_bf16(xin.data_ptr(), wf16.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, H, cin, cout,
                                   4, None, None, None, None, stats.data_ptr(), st()))
    torch.cuda.synchronize()
    assert rel_err(nchw(out), ref.detach()) < 2e-5
    flat = out.reshape(-1, cout).double().cpu()   # statistics of what was written
    for ti in range(tiles):
        blk = flat[ti * rows:(ti + 1) * rows]
        assert torch.allclose(stats[ti, 0].double().cpu(), blk.sum(0), rtol=1e-4, atol=1e-3)
        assert torch.allclose(stats[ti, 1].double().cpu(), (blk - blk.mean(0)).pow(2).sum(0), rtol=1e-4, atol=1e-3)
    # input gradient = the same kernel on dy with the mirrored pack, channel roles swapped
    gd = nhwc(dy).cuda()
    gin = torch.full((B, H, H, cin), float("nan"), device="cuda")
    check(lib.tdx_conv3x3_fwd_bf16(gd.data_ptr(), wg16.data_ptr(), None, gin.data_ptr(), B, H, H, cout, cin, 0,
                                   None, None, None, None, None, st()))
    assert rel_err(nchw(gin), ref_dx) < 2e-5
    splits = lib.tdx_conv3x3_wgrad_splits_bf16(B, H, H, cin, cout)
    slabs = torch.full((splits, cout, 9, cin), float("nan"), device="cuda")
    dw = torch.empty((cout, cin, 3, 3), device="cuda")
    check(lib.tdx_conv3x3_wgrad_bf16(xin.data_ptr(), gd.data_ptr(), slabs.data_ptr(), B, H, H, cin, cout, 0, None, None,
                                     st()))
    check(lib.tdx_conv3x3_wgrad_reduce(slabs.data_ptr(), dw.data_ptr(), splits, cout, cin, st()))
    assert rel_err(dw, ref_dw) < 2e-5


# bf16-STORAGE entry points (tdx_conv3x3_fwd_bf16_io / tdx_conv3x3_wgrad_bf16_io, io16 = 1: activations and activation
# gradients are bf16 tensors), every kernel variant the tuning knobs select:
#   default  nine-tap weight gradient (conv3x3_wgrad9_bf16_kernel), 128-row forward / input-gradient kernel
#   ring     + the 256-row DMA ring forward kernel where M % 256 == 0 (off by default: slower inside the step)
#   per_tap  one workgroup per tap with the swizzled transposing stage (conv3x3_wgrad_bf16s_kernel)
#   round2   the round-2 staging of the per-tap kernel
#   wgs256   the nine-tap kernel with its pixel split aimed at 256 workgroups (fewer, longer chunks; off by default)
#   thin2 / thin1 / thin0   the slot-window forward kernel (conv3x3_bf16_thin_kernel; default: every raw-input launch with
#            M % 256 == 0) only for layers with 64 output or input channels / 64 output channels / nowhere
IO16_VARIANTS = {"default": {}, "ring": {"bf16_ring": 1, "bf16_thin": 0}, "per_tap": {"bf16_wgrad9": 0},
                 "round2": {"bf16_wgrad9": 0, "bf16_wgrad_swz": 0}, "wgs256": {"wgrad9_wgs": 256},
                 "thin2": {"bf16_thin": 2}, "thin1": {"bf16_thin": 1}, "thin0": {"bf16_thin": 0}}
IO16_CASES = [
    # B, H, cin, cout, in_bn: M % 256 == 0 (ring) and ragged M; 4x4 .. 64x64 maps (the padded-slot ring of the nine-tap
    # kernel: 64 slots span 2.5 samples at 4x4, its halo 4 blocks at 64x64); 64- and 128-wide tiles; BN+ReLU on load
    (16, 28, 64, 128, 0), (16, 28, 128, 128, 1), (3, 14, 128, 256, 0), (16, 4, 512, 512, 1), (5, 7, 256, 512, 0),
    (4, 8, 1024, 256, 0), (1, 64, 64, 64, 1), (2, 32, 192, 64, 0), (33, 8, 128, 128, 1), (4, 16, 384, 128, 0),
    # thin layers (64 output or input channels, M % 256 == 0): tiles that cross sample boundaries at 28x28, whole samples
    # inside one tile at 4x4 .. 16x16, a 64x64 map
    (16, 28, 64, 64, 0), (16, 28, 256, 64, 0), (16, 4, 64, 64, 0), (8, 8, 64, 128, 0), (4, 16, 64, 64, 0), (1, 64, 64, 64, 0),
]


@pytest.mark.parametrize("variant", list(IO16_VARIANTS))
@pytest.mark.parametrize("B,H,cin,cout,in_bn", IO16_CASES)
def test_bf16_storage_kernels(tdx, variant, B, H, cin, cout, in_bn):
    lib, check = tdx.lib, tdx.check
    knobs = IO16_VARIANTS[variant]
    g = torch.Generator().manual_seed(B * 1000 + H + cin)
    x = torch.randn(B, cin, H, H, generator=g).bfloat16()
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    dy = torch.randn(B, cout, H, H, generator=g).bfloat16()
    isc, ish = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    # host arithmetic: the tensors ARE bf16; BN + ReLU on load is an fp32 fma rounded to bf16; exact products, fp64 sums
    a = x.float()
    if in_bn:
        a = F.relu(torch.addcmul(ish.view(1, -1, 1, 1), a, isc.view(1, -1, 1, 1))).bfloat16().float()
    a = a.double().requires_grad_(True)
    wr = bf16_round(w).requires_grad_(True)
    ref = F.conv2d(a, wr, b.double(), padding=1)
    ref_dw, = torch.autograd.grad(ref, wr, dy.double(), retain_graph=True)
    ref_dx, = torch.autograd.grad(ref, a, dy.double())
    wf16 = torch.empty(cout * 9 * cin, dtype=torch.bfloat16, device="cuda")
    wg16 = torch.empty(cout * 9 * cin, dtype=torch.bfloat16, device="cuda")
    check(lib.tdx_pack_conv3x3_bf16(w.cuda().contiguous().data_ptr(), wf16.data_ptr(), wg16.data_ptr(), cout, cin, st()))
    xin, gd = nhwc(x).cuda(), nhwc(dy).cuda()
    iscd, ishd, bd = isc.cuda(), ish.cuda(), b.cuda()
    scp, shp = (iscd.data_ptr(), ishd.data_ptr()) if in_bn else (None, None)
    M = B * H * H
    rows = lib.tdx_conv3x3_bf16_stat_tile_rows()
    tiles = -(-M // rows)
    out = torch.full((B, H, H, cout), float("nan"), dtype=torch.bfloat16, device="cuda")
    stats = torch.full((tiles, 2, cout), float("nan"), device="cuda")
    gin = torch.full((B, H, H, cin), float("nan"), dtype=torch.bfloat16, device="cuda")
    out_inf = torch.full((B, H, H, cout), float("nan"), dtype=torch.bfloat16, device="cuda")
    osc, osh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    oscd, oshd = osc.cuda(), osh.cuda()
    dw = torch.empty((cout, cin, 3, 3), device="cuda")
    with tdx.tuned(**knobs):
        splits = lib.tdx_conv3x3_wgrad_splits_bf16(B, H, H, cin, cout)   # (the split plan follows wgrad9_wgs)
        slabs = torch.full((splits, cout, 9, cin), float("nan"), device="cuda")
        check(lib.tdx_conv3x3_fwd_bf16_io(xin.data_ptr(), wf16.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, H, cin, cout,
                                          4 | (1 if in_bn else 0), scp, shp, None, None, stats.data_ptr(), 1, st()))
        check(lib.tdx_conv3x3_fwd_bf16_io(gd.data_ptr(), wg16.data_ptr(), None, gin.data_ptr(), B, H, H, cout, cin, 0,
                                          None, None, None, None, None, 1, st()))
        # the inference epilogue relu((acc + bias) * scale + shift) of the same launch (flag 2)
        check(lib.tdx_conv3x3_fwd_bf16_io(xin.data_ptr(), wf16.data_ptr(), bd.data_ptr(), out_inf.data_ptr(), B, H, H, cin,
                                          cout, 2 | (1 if in_bn else 0), scp, shp, oscd.data_ptr(), oshd.data_ptr(), None, 1,
                                          st()))
        check(lib.tdx_conv3x3_wgrad_bf16_io(xin.data_ptr(), gd.data_ptr(), slabs.data_ptr(), B, H, H, cin, cout,
                                            1 if in_bn else 0, scp, shp, 1, st()))
        check(lib.tdx_conv3x3_wgrad_reduce(slabs.data_ptr(), dw.data_ptr(), splits, cout, cin, st()))
        torch.cuda.synchronize()
    # outputs are rounded to bf16 once: 2^-9 relative per element at most
    assert torch.isfinite(out.float()).all() and torch.isfinite(gin.float()).all()
    assert rel_err(nchw(out.float()), ref.detach()) < 3e-3
    assert (nchw(out.float()).double().cpu() - ref.detach()).abs().max() <= 2.0 ** -8 * ref.detach().abs().max() + 1e-6
    assert rel_err(nchw(gin.float()), ref_dx) < 3e-3
    ref_inf = F.relu(ref.detach() * osc.double().view(1, -1, 1, 1) + osh.double().view(1, -1, 1, 1))
    assert torch.isfinite(out_inf.float()).all() and rel_err(nchw(out_inf.float()), ref_inf) < 3e-3
    # the statistics partials come from the fp32 accumulators, not from the rounded output
    flat = ref.detach().permute(0, 2, 3, 1).reshape(-1, cout)
    for ti in range(tiles):
        blk = flat[ti * rows:(ti + 1) * rows]
        assert torch.allclose(stats[ti, 0].double().cpu(), blk.sum(0), rtol=1e-4, atol=2e-3)
        assert torch.allclose(stats[ti, 1].double().cpu(), (blk - blk.mean(0)).pow(2).sum(0), rtol=1e-4, atol=2e-3)
    # the weight gradient is fp32 all the way: accumulation order only
    assert rel_err(dw, ref_dw) < 2e-5


def test_bf16_conv_bn_relu_on_load_and_fused_epilogue(tdx):
    """BN+ReLU of the producing layer applied while staging (forward and weight gradient) and the
    inference epilogue relu((acc + bias) * scale + shift)."""
    lib, check = tdx.lib, tdx.check
    B, H, cin, cout = 3, 14, 128, 256
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, cin, H, H, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    isc, ish = torch.randn(cin, generator=g), torch.randn(cin, generator=g) * 0.3
    osc, osh = torch.randn(cout, generator=g), torch.randn(cout, generator=g) * 0.3
    dy = torch.randn(B, cout, H, H, generator=g)
    a = bf16_round(F.relu(torch.addcmul(ish.view(1, -1, 1, 1), x, isc.view(1, -1, 1, 1))))  # fp32 fma, then rounded
    wr = bf16_round(w).requires_grad_(True)
    conv = F.conv2d(a, wr, b.double(), padding=1)
    ref = F.relu(conv * osc.double().view(1, -1, 1, 1) + osh.double().view(1, -1, 1, 1))
    ref_dw, = torch.autograd.grad(conv, wr, bf16_round(dy))
    wf16 = torch.empty(cout * 9 * cin, dtype=torch.bfloat16, device="cuda")
    check(lib.tdx_pack_conv3x3_bf16(w.cuda().data_ptr(), wf16.data_ptr(), None, cout, cin, st()))
    xin, iscd, ishd, oscd, oshd, bd = nhwc(x).cuda(), isc.cuda(), ish.cuda(), osc.cuda(), osh.cuda(), b.cuda()
    out = torch.empty((B, H, H, cout), device="cuda")
    check(lib.tdx_conv3x3_fwd_bf16(xin.data_ptr(), wf16.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, H, cin, cout,
                                   1 | 2, iscd.data_ptr(), ishd.data_ptr(), oscd.data_ptr(), oshd.data_ptr(), None, st()))
    assert rel_err(nchw(out), ref.detach()) < 3e-5
    splits = lib.tdx_conv3x3_wgrad_splits_bf16(B, H, H, cin, cout)
    slabs = torch.empty((splits, cout, 9, cin), device="cuda")
    dw = torch.empty((cout, cin, 3, 3), device="cuda")
    gd = nhwc(dy).cuda()
    check(lib.tdx_conv3x3_wgrad_bf16(xin.data_ptr(), gd.data_ptr(), slabs.data_ptr(), B, H, H, cin, cout, 1,
                                     iscd.data_ptr(), ishd.data_ptr(), st()))
    check(lib.tdx_conv3x3_wgrad_reduce(slabs.data_ptr(), dw.data_ptr(), splits, cout, cin, st()))
    assert rel_err(dw, ref_dw) < 3e-5


def _cos(a, b):
    a, b = a.double().reshape(-1).cpu(), b.double().reshape(-1).cpu()
    return (a @ b / (a.norm() * b.norm()).clamp_min(1e-300)).item()


def _check_against_fp32(m, args_gpu, noise, eps_ref, loss_ref, grads_ref, tag, yard):
    """One train-mode forward + backward in bf16 mode against the fp32 vectors, gated by the distance the reference
    itself moves under bf16 autocast (``yard``: AutocastYardstick of the same network and inputs)."""
    eps = m(*args_gpu)
    loss = F.mse_loss(eps, noise.cuda())
    loss.backward()
    mse = ((eps.detach().cpu().double() - eps_ref.double()) ** 2).mean().item()
    print(f"{tag}: loss {loss.item():.5f} vs {loss_ref:.5f}")
    cos = []
    for k, p in m.named_parameters():
        if is_pre_bn_bias(k) or k not in grads_ref:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        cos.append((_cos(p.grad, grads_ref[k]), k))
    cos.sort()
    yard.check(tag, eps_mse=mse, cos_sorted=cos, loss=loss.item(), loss_ref=loss_ref)


@pytest.mark.parametrize("materialize", [1, 0])
def test_bf16_mnist_unet_against_fp32_golden(golden_dir, tdx, materialize):
    """configs[1] network in bf16 mode against the reference's fp32 vectors (B = 64, train-mode BN).  materialize = 1
    (default): relu(bn(Y)) of a unit that feeds another convolution is written out in bf16 once; 0: recomputed while
    the consuming GEMMs stage their tiles (the same values: fp32 fma, one rounding)."""
    from tiny_diffusion_amd.diffusion import NoiseModel

    d = np.load(os.path.join(golden_dir, "grad_B64_uncond.npz"))
    sd = make_state_dict(int(d["seed"]), False)
    m = NoiseModel(); m.load_state_dict(sd); m = m.cuda().train()
    assert m.compute_dtype == torch.float32
    m.set_compute_dtype(torch.bfloat16)
    x_t, t, noise = torch.from_numpy(d["x_t"]), torch.from_numpy(d["t"]), torch.from_numpy(d["noise"])
    _, _, g32, _ = R.train_step_grads(sd, x_t, t, noise)
    with tdx.tuned(bf16_materialize=materialize):
        _check_against_fp32(m, (x_t.cuda(), t.cuda()), noise, torch.from_numpy(d["eps_hat"]), float(d["loss"]), g32,
                            f"mnist B64 materialize={materialize}", AutocastYardstick("mnist_B64"))
    # and back: the same module in fp32 mode reproduces the fp32 vectors exactly as before
    m.set_compute_dtype(torch.float32)
    m.load_state_dict(sd)
    with torch.no_grad():
        eps = m(x_t.cuda(), t.cuda())
    assert ((eps.cpu().double() - torch.from_numpy(d["eps_hat"]).double()) ** 2).mean().item() < 1e-10


@pytest.mark.parametrize("name,hw", [("laion_B8", 32), ("laion_B2_hw64", 64)])
def test_bf16_laion_unet_against_fp32_golden(golden_dir, name, hw):
    """configs[4] network (4 x hw x hw latents, hw = 32 and 64) in bf16 mode: train and eval forward,
    gradients, and a graph-replayed reverse chain against the reference's fp32 vectors."""
    from tiny_diffusion_amd.conditional_diffusion_laion import ForwardProcess, NoiseModel, sample

    d = np.load(os.path.join(golden_dir, name + ".npz"))
    sd = make_state_dict_laion(0)
    x_t, t = torch.from_numpy(d["x_t"]), torch.from_numpy(d["t"])
    cond, noise = torch.from_numpy(d["cond"]), torch.from_numpy(d["noise"])
    assert x_t.shape[-1] == hw
    m = NoiseModel(time_dim=768); m.load_state_dict(sd); m = m.cuda().train()
    m.set_compute_dtype(torch.bfloat16)
    _, _, g32, _ = RL.train_step_grads(sd, x_t, t, noise, cond)
    _check_against_fp32(m, (x_t.cuda(), t.cuda(), cond.cuda()), noise, torch.from_numpy(d["eps_train"]),
                        float(d["loss_train"]), g32, f"laion {hw}x{hw}", AutocastYardstick(name))
    m.load_state_dict(sd); m.eval()
    with torch.no_grad():
        eps = m(x_t.cuda(), t.cuda(), cond.cuda())
    ref = torch.from_numpy(d["eps_eval"]).double()
    rel = ((eps.cpu().double() - ref) ** 2).mean().item() / (ref ** 2).mean().item()
    print(f"laion {hw}x{hw} eval: relative MSE {rel:.3e}")
    AutocastYardstick(name).check(f"laion {hw}x{hw} eval", eps_mse=rel * (ref ** 2).mean().item(), eval_mode=True)
    assert rel <= 2e-4   # (and the round-3 figure: eval-mode outputs of this random-weight net are O(4), so relative)
    T = int(d["chain_T"])
    n = d["chain_x_T"].shape[0]
    x = sample(m, ForwardProcess(num_timesteps=T), "cuda", text_embeds=cond[:n], x_T=torch.from_numpy(d["chain_x_T"]),
               noises=torch.from_numpy(d["chain_zs"]), use_graph=True)
    fin = torch.from_numpy(d["chain_final"]).double()
    relc = ((x.cpu().double() - fin) ** 2).mean().item() / (fin ** 2).mean().item()
    print(f"laion {hw}x{hw} chain T={T}: relative MSE of x_0 {relc:.3e}")
    assert torch.isfinite(x).all() and relc <= 1e-3


def test_bf16_train_step_decreases_loss_like_fp32():
    """A few optimisation steps (TrainStep: q_sample, forward, MSE, backward, Adam) in both modes from the
    same initial weights and the same data: the loss curves stay within 3 % of each other."""
    from tiny_diffusion_amd.diffusion import ForwardProcess, NoiseModel
    from tiny_diffusion_amd.train import TrainStep

    curves = {}
    for dt in (torch.float32, torch.bfloat16):
        torch.manual_seed(0)
        m = NoiseModel().cuda().train().set_compute_dtype(dt)
        ts = TrainStep(m, ForwardProcess(), lr=1e-3, philox_seed=5)
        g = torch.Generator(device="cuda").manual_seed(1)
        x0 = torch.rand(64, 1, 28, 28, device="cuda", generator=g) * 2 - 1
        t = torch.randint(0, 1000, (64,), device="cuda", generator=g)
        curves[dt] = [float(ts.step(x0, t=t)) for _ in range(8)]
    a, b = curves[torch.float32], curves[torch.bfloat16]
    print("fp32", [f"{v:.4f}" for v in a], "bf16", [f"{v:.4f}" for v in b])
    assert b[-1] < b[0] and a[-1] < a[0]
    assert all(abs(x - y) <= 0.03 * abs(x) for x, y in zip(a, b)), (a, b)
