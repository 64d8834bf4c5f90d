"""The Winograd forward / input gradient with its waves split by transform row (conv3x3_wino_kernel<EPI, false, true>,
knob wino_rows) against the channel split it replaces (wino_rows = 0): the row split accumulates the same products in
the same order, so outputs and BatchNorm statistics partials must be bit-identical, not merely close.

Launches: every training forward (statistics epilogue) and input gradient that runs on Winograd in the B = 256 step of
the MNIST UNet and of the LAION UNet at 32x32 and 64x64 (from tdx_conv3x3_train_algo, as tests/test_gpu_conv_launches.py
builds its table), plus edge shapes: 7x7 maps (whole images per workgroup), the 4x4 bottleneck, ragged last
workgroups, 63 / 64 / 65 tile blocks around the compact / XCD-grouped mapping boundary, and 8-stage launches (64 input
channels: the shortest loop, where the epilogue's row exchange weighs most)."""
import pytest
import torch

from test_gpu_conv_launches import model_units, tile_blocks

pytestmark = pytest.mark.gpu

B_TRAIN = 256

EDGE = [   # (B, H, cin, cout)
    (64, 7, 64, 128),     # 7x7: four whole images per workgroup, odd maps
    (261, 7, 64, 128),    # 7x7 with a ragged last workgroup (one image), grouped mapping
    (256, 4, 64, 64),     # the 4x4 bottleneck geometry: every tile touches the border
    (252, 8, 64, 128),    # 63 tile blocks: compact mapping
    (256, 8, 128, 64),    # 64 tile blocks: XCD-grouped
    (257, 8, 64, 64),     # 65 tile blocks, the last one ragged
    (16, 8, 64, 64),      # 8 stages, 16 workgroups
    (256, 28, 64, 128),   # 8 stages at the first layer's size
]


@pytest.fixture(scope="module")
def tdx():
    import tiny_diffusion_amd._lib as L

    assert torch.cuda.is_available()
    return L


def stream():
    return torch.cuda.current_stream().cuda_stream


def launches(lib):
    """Distinct (B, H, cin, cout, role) with role 0 = forward with statistics, 1 = input gradient; for the input gradient
    cin / cout are those of the convolution the kernel computes (the layer's cout -> cin)."""
    from tiny_diffusion_amd import unet as UN

    out = set()
    for kind, hw in ((UN.KIND_MNIST, 28), (UN.KIND_LAION, 32), (UN.KIND_LAION, 64)):
        for cin, _, cout, H in model_units(kind, hw):
            if lib.tdx_conv3x3_train_algo(B_TRAIN, H, H, cin, cout, 0):
                out.add((B_TRAIN, H, cin, cout, 0))
            if lib.tdx_conv3x3_train_algo(B_TRAIN, H, H, cin, cout, 1):
                out.add((B_TRAIN, H, cout, cin, 1))
    assert {r for *_, r in out} == {0, 1}
    for B, H, cin, cout in EDGE:
        assert lib.tdx_conv3x3_wino_ok(B, H, H, cin, cout)
        out.add((B, H, cin, cout, 0))
        out.add((B, H, cin, cout, 1))
    return sorted(out)


def run(tdx, x, u, b, B, H, cin, cout, role):
    lib = tdx.lib
    out = torch.full((B, H, H, cout), float("nan"), device="cuda")
    if role == 0:
        stats = torch.full((lib.tdx_conv3x3_wino_stat_tiles(B, H, H), 2, cout), float("nan"), device="cuda")
        tdx.check(lib.tdx_conv3x3_fwd_wino(x.data_ptr(), u.data_ptr(), b.data_ptr(), out.data_ptr(), B, H, H, cin, cout, 4,
                                           None, None, stats.data_ptr(), stream()))
    else:
        stats = None
        tdx.check(lib.tdx_conv3x3_fwd_wino(x.data_ptr(), u.data_ptr(), None, out.data_ptr(), B, H, H, cin, cout, 0,
                                           None, None, None, stream()))
    return out, stats


def test_launch_list(tdx):
    """The list holds the 8-stage launches and both sides of the compact / grouped boundary."""
    ls = launches(tdx.lib)
    assert any(cin == 64 and r == 0 and B == B_TRAIN for B, _, cin, _, r in ls)
    assert any(cin == 64 and r == 1 and B == B_TRAIN for B, _, cin, _, r in ls)
    assert {63, 64, 65} <= {tile_blocks(B, H) for B, H, *_ in ls}


def test_rows_bit_identical_to_channel_split(tdx):
    lib = tdx.lib
    failures = []
    for i, (B, H, cin, cout, role) in enumerate(launches(lib)):
        g = torch.Generator(device="cuda").manual_seed(1000 + i)
        x = torch.randn(B, H, H, cin, generator=g, device="cuda")
        w = torch.randn(cout, cin, 3, 3, generator=g, device="cuda") * (2.0 / (9 * cin)) ** 0.5
        b = torch.randn(cout, generator=g, device="cuda") * 0.1
        u = torch.full((cout * cin * 16,), float("nan"), device="cuda")
        tdx.check(lib.tdx_pack_conv3x3_wino(w.data_ptr(), u.data_ptr(), None, cout, cin, stream()))
        with tdx.tuned(wino_rows_min_stages=1, wino_rows=0):
            ref, ref_st = run(tdx, x, u, b, B, H, cin, cout, role)
        with tdx.tuned(wino_rows_min_stages=1, wino_rows=1):
            got, got_st = run(tdx, x, u, b, B, H, cin, cout, role)
            again, again_st = run(tdx, x, u, b, B, H, cin, cout, role)
        torch.cuda.synchronize()
        tag = f"B{B} {H}x{H} {cin}->{cout} {'fwd' if role == 0 else 'dgrad'} ({cin // 8} stages, {tile_blocks(B, H)} blocks)"
        bad = []
        if torch.isnan(got).any() or (got_st is not None and torch.isnan(got_st).any()):
            bad.append("NaN (unwritten) elements")
        if not torch.equal(got, again) or (got_st is not None and not torch.equal(got_st, again_st)):
            bad.append("two launches differ")
        if not torch.equal(got, ref):
            bad.append(f"output differs from the channel split at {int((got != ref).sum())} elements")
        if got_st is not None and not torch.equal(got_st, ref_st):
            bad.append("statistics partials differ from the channel split")
        print(f"{tag}: {'ok' if not bad else '; '.join(bad)}", flush=True)
        failures += [f"{tag}: {m}" for m in bad]
    assert not failures, failures
