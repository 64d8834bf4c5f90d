"""Every 3x3 convolution launch of the benchmarked workloads, run as the plan runs it, against an fp64 reference of
the same operation.

The launch table is built from the library, not written by hand: the 13 conv/BN units of the MNIST UNet at 28x28 and
of the LAION UNet at 32x32 and 64x64 (shapes from the model's modules and the plan's own tensors), the training
algorithm of every role at the per-GPU batch bench.py times (tdx_conv3x3_train_algo) and the sampling algorithm at
n = 16 / 64 (tdx_conv3x3_infer_algo).  Each distinct launch runs through the public entry the plan uses, with the
plan's flags, and is gated three ways:

  (a) norm-wise: ||got - ref|| / ||ref|| within the bounds of tests/test_gpu_ops.py (direct 2e-6 / 3e-6 where that
      file has 3e-6, Winograd 1e-5);
  (b) per element: |got - ref| / (u sqrt(K) (|x| * |w|)), the error over that element's magnitude-sum (the same fp64
      reference on absolute values), u = 2^-24, K the length of the dot product - catches one wrong tile or one
      missing K-stage of one workgroup, which moves (a) very little on a 25 M-element tensor;
  (c) Winograd error budget: where a Winograd kernel runs, the direct kernel runs on the same operands too, and the
      Winograd norm-wise error may be at most K_WINO times the direct one.

Plus the launches the B = 256 table does not reach: the compact / XCD-grouped workgroup mapping boundary (63, 64 and
65 tile blocks, the last one ragged), a ragged 7x7 launch in the grouped mapping, and the weight gradient's chunk at its
1024-tile cap with a ragged last chunk."""
import math

import pytest
import torch
import torch.nn.functional as F

from conv_helpers import (ELEM_DIRECT, ELEM_WINO, K_WINO, REL_DIRECT, REL_WINO, U, Operands, check_launch, conv_ref64,  # noqa: F401
                          dgrad_ref64, elem_ratio, p, rel_err, run_dgrad, run_fwd, run_infer, run_wgrad, stream, tile_blocks,
                          wgrad_ref64)

pytestmark = pytest.mark.gpu

B_TRAIN = 256                 # per-GPU batch of the benchmarked training step (bench.py)
N_SAMPLE = (16, 64)           # sampling batches: the reverse process's default and bench.py's larger one
ROLES = ("fwd", "dgrad", "wgrad")

# The references, the error measures, the gates (REL_*, ELEM_*, K_WINO) and the launch wrappers live in
# tests/conv_helpers.py, shared with tests/test_gpu_conv_nonsquare.py.


@pytest.fixture(scope="module")
def tdx():
    import tiny_diffusion_amd._lib as L

    assert torch.cuda.is_available()
    return L


def test_reference_helpers_against_cpu_conv2d():
    """The device fp64 helpers are the convolution, its input gradient and its weight gradient (CPU F.conv2d in fp64)."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 5, 7, 6, generator=g, dtype=torch.float64)
    w = torch.randn(4, 6, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(4, generator=g, dtype=torch.float64)
    dy = torch.randn(3, 5, 7, 4, generator=g, dtype=torch.float64)
    xc = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wc = w.clone().requires_grad_(True)
    y = F.conv2d(xc, wc, b, padding=1)
    y.backward(dy.permute(0, 3, 1, 2))
    d = torch.device("cuda")
    got = conv_ref64(x.to(d), w.to(d), b.to(d)).cpu()
    assert torch.allclose(got, y.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(dgrad_ref64(dy.to(d), w.to(d)).cpu(), xc.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(wgrad_ref64(x.to(d), dy.to(d)).cpu(), wc.grad, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------- the table
def model_units(kind, hw):
    """(cin as stored, cin of the reference weight, cout, H) of the 13 conv/BN units of one network, from the model's
    modules (channels) and the plan's own tensors (map sizes; the stored width of the first unit's input)."""
    from tiny_diffusion_amd import unet as UN

    if kind == UN.KIND_MNIST:
        from tiny_diffusion_amd.diffusion import NoiseModel
        model = NoiseModel()
    else:
        from tiny_diffusion_amd.conditional_diffusion_laion import NoiseModel
        model = NoiseModel()
    arch = model._arch
    plan = UN._Plan(1, 0, torch.device("cuda"), kind, 0 if hw == arch.in_shape[1] else hw)
    out = []
    for i, (stage, idx) in enumerate(UN._UNIT_PREFIX):
        conv = getattr(model, stage)[idx]
        assert isinstance(conv, torch.nn.Conv2d) and conv.kernel_size == (3, 3) and conv.padding == (1, 1)
        cin, cout = conv.in_channels, conv.out_channels
        H = math.isqrt(plan.tensor(f"Y{i}").numel() // cout)
        assert H * H * cout == plan.tensor(f"Y{i}").numel()
        stored = cin
        if i == 0:   # the first unit reads x0 (initial_conv's output), stored at the plan's width
            stored = plan.tensor("x0").numel() // (H * H)
        out.append((stored, cin, cout, H))
    del plan
    assert len(out) == 13
    return out


def launch_table(lib):
    """Distinct launches [(B, H, cin, cin_real, cout, role, algo, models)] of the benchmarked workloads."""
    from tiny_diffusion_amd import unet as UN

    nets = [("mnist28", UN.KIND_MNIST, 28, True), ("laion32", UN.KIND_LAION, 32, True), ("laion64", UN.KIND_LAION, 64, False)]
    table = {}
    for name, kind, hw, sampled in nets:
        units = model_units(kind, hw)
        for cin, cin_real, cout, H in units:
            for r, role in enumerate(ROLES):
                algo = "wino" if lib.tdx_conv3x3_train_algo(B_TRAIN, H, H, cin, cout, r) else "direct"
                table.setdefault((B_TRAIN, H, cin, cin_real, cout, role, algo), []).append(name)
            if sampled:
                for n in N_SAMPLE:
                    algo = "wino" if lib.tdx_conv3x3_infer_algo(n, H, H, cin, cout) else "direct"
                    table.setdefault((n, H, cin, cin_real, cout, "infer", algo), []).append(f"{name}/n{n}")
    return [k + (v,) for k, v in table.items()]


def test_launch_table_covers_the_kernels(tdx):
    """The table reaches every kernel family and the XCD-grouped Winograd mapping with a padded grid."""
    table = launch_table(tdx.lib)
    kinds = {(e[5], e[6]) for e in table}
    for need in (("fwd", "wino"), ("dgrad", "wino"), ("wgrad", "wino"), ("infer", "wino"), ("infer", "direct")):
        assert need in kinds, need
    assert any(e[6] == "direct" and e[5] != "infer" for e in table)
    grouped = [e for e in table if e[6] == "wino" and e[5] in ("fwd", "dgrad") and tile_blocks(e[0], e[1]) >= 64]
    assert any(tile_blocks(e[0], e[1]) % 8 for e in grouped), "no grouped launch pads its grid"


def run_table(tdx, entries):
    failures = []
    print(f"\n{'B':>4s} {'H':>3s} {'cin':>5s} {'cout':>5s} role   algo")
    for i, (B, H, cin, cin_real, cout, role, algo, tag) in enumerate(entries):
        row, fails = check_launch(tdx, B, H, cin, cin_real, cout, role, algo, seed=i)
        print(f"{row}  {tag}{'  FAIL ' + '; '.join(fails) if fails else ''}", flush=True)
        failures += [(B, H, cin, cout, role, algo, f) for f in fails]
    return failures


def test_every_launch_of_the_benchmarked_workloads(tdx):
    """Every distinct 3x3 convolution launch of the B = 256 training step (MNIST, LAION 32x32 and 64x64) and of the
    n = 16 / 64 reverse step (MNIST, LAION 32x32), as the plan runs it, against fp64."""
    table = launch_table(tdx.lib)
    failures = run_table(tdx, [e[:7] + (",".join(e[7]),) for e in table])
    assert not failures, failures


def test_edge_launches(tdx):
    """The launches the B = 256 table does not reach: 63 / 64 / 65 tile blocks around the compact / XCD-grouped mapping
    boundary (65: ragged last block), a ragged 7x7 launch in the grouped mapping (66 blocks of four whole images, the
    last with one), and the Winograd weight gradient with its pixel chunk at the 1024-tile cap (wino_wgrad_target = 1:
    one split per channel tile wanted, so the cap decides; 2156 and 1120 tiles -> a ragged last chunk)."""
    lib = tdx.lib
    entries = []
    for B, H, cin, cout in ((252, 8, 64, 128), (256, 8, 128, 64), (257, 8, 64, 64), (261, 7, 64, 128)):
        assert lib.tdx_conv3x3_wino_ok(B, H, H, cin, cout) and lib.tdx_conv3x3_wino_ok(B, H, H, cout, cin)
        for role in ("fwd", "dgrad", "infer"):
            entries.append((B, H, cin, cin, cout, role, "wino", f"{tile_blocks(B, H)} tile blocks"))
    assert sorted({tile_blocks(e[0], e[1]) for e in entries}) == [63, 64, 65, 66]
    with tdx.tuned(wino_wgrad_target=1):
        for B, H, cin, cout in ((11, 28, 64, 128), (70, 7, 64, 64)):
            nt = B * ((H + 1) // 2) ** 2
            assert lib.tdx_conv3x3_wgrad_wino_splits(B, H, H, cin, cout) == -(-nt // 1024) and nt % 1024
            entries.append((B, H, cin, cin, cout, "wgrad", "wino", f"{nt} tiles in chunks of 1024"))
        failures = run_table(tdx, entries)
    assert lib.tdx_conv3x3_wgrad_wino_splits(256, 28, 28, 64, 128) == 251   # the default plan is back
    assert not failures, failures
