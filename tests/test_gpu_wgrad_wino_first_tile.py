"""The Winograd weight gradient's first tile-iteration and per-stage DMA state (conv3x3_wgrad_wino_kernel).  The
accumulators are never zeroed: the first tile-iteration of a workgroup's first stage takes the constant 0 as C, from a
second copy of the stage's code, and the scalar DMA state of stage s+2 (offsets, lane masks) is built a tile-iteration
ahead of its requests.  Checked on the smallest shapes at which those parts can go wrong: every slab element written
(slabs pre-filled with NaN), two launches bit-identical, the reduced gradient against fp64 within the Winograd bound of
tests/test_gpu_conv_launches.py, and one all-ones case against the closed-form integer counts (every product exact: a
dropped or doubled first tile is an integer difference, not an error under a tolerance)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REL_WINO = 1e-5   # norm-wise, as tests/test_gpu_conv_launches.py

# (B, H, cin, cout, wino_wgrad_target or None for the default plan, splits the plan must give)
CASES = [
    (2, 8, 64, 64, None, 1),      # 32 tiles: one chunk of exactly four stages, the zero-C copy is a quarter of the first
    (3, 9, 64, 64, None, 3),      # 75 tiles in chunks of 32: the last workgroup has 11, a ragged stage after its first
    (1, 7, 64, 64, None, 1),      # first tile on the border, odd map: masked rows and columns under the zero-C MFMAs
    (1, 5, 64, 64, None, 1),      # the same with 9 tiles: the second stage holds one tile
    (6, 28, 64, 64, 1, 2),        # 1176 tiles: a chunk at the 1024-tile cap (128 stages) and one of 152
    (4, 8, 128, 192, None, 2),    # several channel blocks both ways: the tile table is per tile, shared by the blocks
    (4, 8, 192, 128, None, 2),
]


@pytest.fixture(scope="module")
def tdx():
    import tiny_diffusion_amd._lib as L

    assert torch.cuda.is_available()
    return L


def stream():
    return torch.cuda.current_stream().cuda_stream


def wgrad_ref64(x, dy):
    """dL/dw [cout, cin, 3, 3] of a 3x3 / pad 1 convolution of NHWC x for dL/dy = dy, in fp64."""
    B, H, W, cin = x.shape
    cout = dy.shape[-1]
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    g = dy.double().reshape(-1, cout).t()
    dw = torch.empty(cout, cin, 3, 3, dtype=torch.float64, device=x.device)
    for kh in range(3):
        for kw in range(3):
            dw[:, :, kh, kw] = g @ xp[:, kh:kh + H, kw:kw + W, :].reshape(-1, cin)
    return dw


def launch(tdx, x, dy):
    lib = tdx.lib
    B, H, W, cin = x.shape
    cout = dy.shape[-1]
    splits = lib.tdx_conv3x3_wgrad_wino_splits(B, H, W, cin, cout)
    slabs = torch.full((splits, cout, 9, cin), float("nan"), device="cuda")
    tdx.check(lib.tdx_conv3x3_wgrad_wino(x.data_ptr(), dy.data_ptr(), slabs.data_ptr(), B, H, W, cin, cout, stream()))
    return slabs, splits


def reduce(tdx, slabs, splits):
    _, cout, _, cin = slabs.shape
    dw = torch.full((cout, cin, 3, 3), float("nan"), device="cuda")
    tdx.check(tdx.lib.tdx_conv3x3_wgrad_reduce(slabs.data_ptr(), dw.data_ptr(), splits, cout, cin, stream()))
    return dw


@pytest.mark.parametrize("B,H,cin,cout,target,want_splits", CASES,
                         ids=[f"B{c[0]}_{c[1]}x{c[1]}_{c[2]}to{c[3]}" + ("_cap" if c[4] else "") for c in CASES])
def test_wgrad_wino_first_tile(tdx, B, H, cin, cout, target, want_splits):
    lib = tdx.lib
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + H * 10 + cin + cout)
    x = torch.randn(B, H, H, cin, generator=g, device="cuda")
    dy = torch.randn(B, H, H, cout, generator=g, device="cuda")
    with tdx.tuned(**({} if target is None else {"wino_wgrad_target": target})):
        assert lib.tdx_conv3x3_wgrad_wino_splits(B, H, H, cin, cout) == want_splits
        s1, splits = launch(tdx, x, dy)
        s2, _ = launch(tdx, x, dy)
    torch.cuda.synchronize()
    assert not torch.isnan(s1).any(), "slab elements left unwritten"
    assert torch.equal(s1, s2), "two launches differ"
    dw = reduce(tdx, s1, splits)
    ref = wgrad_ref64(x, dy)
    rel = ((dw.double() - ref).norm() / ref.norm()).item()
    print(f"rel err {rel:.2e}")
    assert rel < REL_WINO, f"rel err {rel:.2e}"


def test_wgrad_wino_all_ones_exact(tdx):
    """x = dy = 1 at B = 2, 4x4, 64 -> 64 (8 tiles: the zero-C tile-iteration carries every real tile of lanes 0-31):
    dW[co][ci][kh][kw] = B * n(kh) * n(kw), n = (3, 4, 3) the in-image positions of a tap on a 4-wide map."""
    B, H, c = 2, 4, 64
    x = torch.ones(B, H, H, c, device="cuda")
    dy = torch.ones(B, H, H, c, device="cuda")
    assert tdx.lib.tdx_conv3x3_wgrad_wino_splits(B, H, H, c, c) == 1
    s1, splits = launch(tdx, x, dy)
    s2, _ = launch(tdx, x, dy)
    torch.cuda.synchronize()
    assert not torch.isnan(s1).any(), "slab elements left unwritten"
    assert torch.equal(s1, s2), "two launches differ"
    dw = reduce(tdx, s1, splits)
    n = torch.tensor([3.0, 4.0, 3.0], device="cuda")
    want = (B * torch.outer(n, n)).expand(c, c, 3, 3)
    assert torch.equal(dw, want), f"max abs difference {(dw - want).abs().max().item()}"
