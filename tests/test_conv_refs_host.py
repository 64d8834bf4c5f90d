"""Host checks (no GPU) of the fp64 convolution references of tests/conv_helpers.py, which gate every kernel-level
convolution test:

  * conv_ref64 / dgrad_ref64 / wgrad_ref64 are F.conv2d and its autograd in fp64, at non-square maps;
  * they see the fault the non-square GPU tests hunt: on the operands those tests draw, the reference of the same buffers
    read as (B, W, H) maps - what a kernel that exchanged H and W, used H as the row stride or swapped the edge
    conditions would produce - is at least 0.1 (relative, norm-wise) away from the true one for every shape of every
    family, five orders of magnitude above the gates (1e-5 and tighter)."""
import pytest
import torch
import torch.nn.functional as F

import conv_helpers as CH
from conv_helpers import conv_ref64, dgrad_ref64, exchanged, rel_err, wgrad_ref64


@pytest.mark.parametrize("B,H,W,cin,cout", [(3, 5, 7, 6, 4), (2, 6, 4, 3, 5), (2, 1, 9, 4, 4), (1, 8, 3, 2, 3)])
def test_references_equal_conv2d_autograd(B, H, W, cin, cout):
    g = torch.Generator().manual_seed(B * 100 + H * 10 + W)
    x = torch.randn(B, H, W, cin, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    dy = torch.randn(B, H, W, cout, generator=g, dtype=torch.float64)
    xc = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wc = w.clone().requires_grad_(True)
    y = F.conv2d(xc, wc, b, padding=1)
    y.backward(dy.permute(0, 3, 1, 2))
    assert torch.allclose(conv_ref64(x, w, b), y.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(dgrad_ref64(dy, w), xc.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(wgrad_ref64(x, dy), wc.grad, rtol=1e-12, atol=1e-12)


def _distances(x, w, dy):
    """Relative distance of the exchanged-map reference from the true one: forward, input gradient, weight gradient."""
    return (rel_err(exchanged(lambda a: conv_ref64(a, w), x), conv_ref64(x, w)),
            rel_err(exchanged(lambda a: dgrad_ref64(a, w), dy), dgrad_ref64(dy, w)),
            rel_err(exchanged(wgrad_ref64, x, dy), wgrad_ref64(x, dy)))


FAMILIES = {
    "winograd": CH.WINO_SHAPES + CH.WINO_REFUSED,
    "direct": CH.DIRECT_SHAPES + [CH.DIRECT_WIDE] + CH.DIRECT_WGRAD_NARROW,
    "bf16": CH.BF16_SHAPES + [CH.BF16_BN_SHAPE],
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_exchange_of_h_and_w_moves_the_reference(family):
    for i, (B, H, W) in enumerate(FAMILIES[family]):
        assert H != W
        o = CH.Operands(B, H, 64, 64, 128, i, W=W, device="cpu")
        x, dy = (o.x.bfloat16().float(), o.dy.bfloat16().float()) if family == "bf16" else (o.x, o.dy)
        d = _distances(x, o.w, dy)
        print(f"{family} {B}x{H}x{W}: fwd {d[0]:.2f} dgrad {d[1]:.2f} wgrad {d[2]:.2f}")
        assert min(d) >= 0.1, (family, B, H, W, d)


@pytest.mark.parametrize("ct,cf", CH.EDGE_PAIRS)
def test_exchange_of_h_and_w_moves_the_edge_references(ct, cf):
    """The boundary convolutions: every small map, and the 40 x 50 map of the large-batch cases (two samples of it: the
    exchange acts inside a sample, the batch only repeats it)."""
    for i, (B, H, W) in enumerate(CH.EDGE_SMALL + [(2,) + s[1:] for s in CH.EDGE_LARGE[:1]]):
        assert H != W
        e = CH.EdgeOperands(B, H, W, ct, cf, i, device="cpu")
        d = _distances(e.x_nhwc, e.w_init, e.g_fat[..., :cf]) + _distances(e.fat, e.w_fin, e.g_thin_nhwc)
        print(f"edge {ct}->{cf} {B}x{H}x{W}: " + " ".join(f"{v:.2f}" for v in d))
        assert min(d) >= 0.1, (ct, cf, B, H, W, d)
