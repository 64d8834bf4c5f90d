"""The Winograd weight gradient with its waves split by transform row (conv3x3_wgrad_wino_kernel): every slab element
written (slabs pre-filled with NaN), two launches bit-identical, and the reduced gradient against fp64 within the
Winograd bound of tests/test_gpu_conv_launches.py, on the shapes that stress the epilogue's row exchange and the
scalar DMA masks: 7x7, 5x5 and 4x4 maps, a chunk that ends partway through a stage, the 1024-tile chunk cap, cin != cout
both ways and several 64-channel blocks per side."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REL_WINO = 1e-5   # norm-wise, as tests/test_gpu_conv_launches.py

# (B, H, cin, cout, wino_wgrad_target or None for the default plan)
CASES = [
    (64, 7, 64, 64, None),        # odd map: patch column / row 3 and output row / column 1 out of the image
    (40, 5, 64, 128, None),       # odd map, cin < cout
    (128, 4, 128, 64, None),      # 4x4: every tile touches the border
    (3, 9, 64, 64, None),         # 75 tiles in chunks of 32: the last chunk ends partway through its second stage
    (11, 28, 64, 128, 1),         # 2156 tiles, chunks at the 1024-tile cap, a ragged last one
    (70, 7, 64, 64, 1),           # 1120 tiles at the cap
    (32, 14, 64, 128, None),      # cin < cout
    (16, 8, 1024, 256, None),     # cin > cout, 16 x 4 channel blocks
    (16, 8, 256, 192, None),      # 4 x 3 channel blocks
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


def launch(tdx, x, dy, B, H, cin, cout):
    lib = tdx.lib
    splits = lib.tdx_conv3x3_wgrad_wino_splits(B, H, H, cin, cout)
    slabs = torch.full((splits, cout, 9, cin), float("nan"), device="cuda")
    tdx.check(lib.tdx_conv3x3_wgrad_wino(x.data_ptr(), dy.data_ptr(), slabs.data_ptr(), B, H, H, cin, cout, stream()))
    return slabs, splits


@pytest.mark.parametrize("B,H,cin,cout,target", CASES, ids=[f"B{c[0]}_{c[1]}x{c[1]}_{c[2]}to{c[3]}" +
                                                             ("_cap" if c[4] else "") for c in CASES])
def test_wgrad_wino_rows(tdx, B, H, cin, cout, target):
    lib = tdx.lib
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + H * 10 + cin + cout)
    x = torch.randn(B, H, H, cin, generator=g, device="cuda")
    dy = torch.randn(B, H, H, cout, generator=g, device="cuda")
    with tdx.tuned(**({} if target is None else {"wino_wgrad_target": target})):
        nt = B * ((H + 1) // 2) ** 2
        if target is not None:
            assert lib.tdx_conv3x3_wgrad_wino_splits(B, H, H, cin, cout) == -(-nt // 1024) and nt % 1024
        s1, splits = launch(tdx, x, dy, B, H, cin, cout)
        s2, _ = launch(tdx, x, dy, B, H, cin, cout)
    torch.cuda.synchronize()
    assert not torch.isnan(s1).any(), "slab elements left unwritten"
    assert torch.equal(s1, s2), "two launches differ"
    dw = torch.full((cout, cin, 3, 3), float("nan"), device="cuda")
    tdx.check(lib.tdx_conv3x3_wgrad_reduce(s1.data_ptr(), dw.data_ptr(), splits, cout, cin, stream()))
    ref = wgrad_ref64(x, dy)
    rel = ((dw.double() - ref).norm() / ref.norm()).item()
    assert rel < REL_WINO, f"rel err {rel:.2e}"
