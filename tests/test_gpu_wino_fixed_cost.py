"""The Winograd forward / input-gradient kernel (conv3x3_wino_kernel) anchored to things its prologue and epilogue do not
touch.  tests/test_gpu_wino_rows.py compares the row split with the channel split, which share the prologue (tile
table, DMA offsets, request order) and most of the epilogue (output image, stores, statistics): a mistake there moves
both sides together.  Here every launch is held against

  1. an fp64 direct convolution computed on the CPU - no NaN left in the NaN-filled outputs, the norm-wise and the
     per-element bound tests/test_gpu_conv_launches.py applies to this entry (REL_WINO, ELEM_WINO: taken from there) -
     and, for the statistics partials, sum and centred M2 recomputed in fp64 from the kernel's OWN output per tile block
     (64 tiles = tdx_conv3x3_wino_stat_tile_rows pixels when full);
  2. SHA-256 digests of the output and statistics bits, recorded once from the commit before the prologue / epilogue
     were reordered (tests/golden/wino_fixed_cost_digests.json; recorder: this module run as a script with
     --package-root <checkout whose library records>): the reordering must not move a bit;
  3. itself: two launches give identical bits.

Shapes (B, H x W, cin -> cout), the smallest at which this code can go wrong: 12 tiles in a single ragged block with every
tile on the border; an odd map with overhanging tiles, validity bits and a ragged last block (80 tiles); a non-square
map with 16 stages (the row split's default threshold); 65 tile blocks - the XCD-grouped id mapping with padding ids and
a ragged 20-tile last block; 8 stages with two channel blocks in the compact mapping.  Each in both roles (forward with
statistics, plain input gradient - the same entry on the mirrored pack, no bias) and under both wave splits
(wino_rows = 0 | wino_rows = 1 with wino_rows_min_stages = 1).  Operands come from a seeded CPU generator.

Statistics tolerance.  Distances of the kernel's partials from the fp64 recomputation, in units of u = 2^-24:
|S - S64| / (u sum|y|) for the sums, |M2 - M2_64| / (u M2_64) for the centred squares, maxima over blocks and channels.
Measured with the recording commit's library on these shapes (sums / M2): 3, 4x4: 1.162 / 2.951; 5, 7x7: 0.880 / 3.678;
2, 6x10: 1.590 / 4.520; 21, 28x28: 1.124 / 4.375; 16, 8x8: 1.111 / 3.431 - identical for both wave splits.  The gates
are four times the maxima, 1.590 and 4.520."""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino_fixed_cost_digests.json")
U = 2.0 ** -24
STAT_SUM_GATE = 4 * 1.590
STAT_M2_GATE = 4 * 4.520

SHAPES = [   # (B, H, W, cin, cout)
    (3, 4, 4, 64, 64),
    (5, 7, 7, 64, 128),
    (2, 6, 10, 128, 64),
    (21, 28, 28, 64, 64),
    (16, 8, 8, 64, 128),
]
ROLES = ("fwd", "dgrad")
SPLITS = {"channels": dict(wino_rows=0), "rows": dict(wino_rows=1, wino_rows_min_stages=1)}
CASES = [(s, role, split) for s in SHAPES for role in ROLES for split in SPLITS]


def case_id(shape, role, split):
    B, H, W, cin, cout = shape
    return f"B{B}_{H}x{W}_{cin}to{cout}_{role}_{split}"


@functools.lru_cache(maxsize=None)
def operands(shape, role):
    """CPU operands of one launch: the kernel's input [B, H, W, cin], the layer's OIHW weight (for the input gradient
    the layer runs cout -> cin, so that the kernel's convolution is cin -> cout in both roles) and the bias."""
    B, H, W, cin, cout = shape
    g = torch.Generator().manual_seed(7000 + 16 * SHAPES.index(shape) + ROLES.index(role))
    x = torch.randn(B, H, W, cin, generator=g)
    wshape = (cout, cin, 3, 3) if role == "fwd" else (cin, cout, 3, 3)
    w = torch.randn(*wshape, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1 if role == "fwd" else None
    return x, w, b


@functools.lru_cache(maxsize=None)
def reference(shape, role):
    """(fp64 reference, magnitude-sum, K) on the CPU, computed once per (shape, role)."""
    from test_gpu_conv_launches import conv_ref64, dgrad_ref64

    x, w, b = operands(shape, role)
    if role == "fwd":
        return conv_ref64(x, w, b), conv_ref64(x.abs(), w.abs(), b.abs()), 9 * shape[3]
    return dgrad_ref64(x, w), dgrad_ref64(x.abs(), w.abs()), 9 * shape[3]


def stream():
    return torch.cuda.current_stream().cuda_stream


def launch(L, shape, role, split):
    """One launch into NaN-filled buffers; returns (out, stats or None) on the CPU."""
    lib = L.lib
    B, H, W, cin, cout = shape
    x, w, b = operands(shape, role)
    xd, wd = x.cuda(), w.cuda()
    u = torch.full((cout * cin * 16,), float("nan"), device="cuda")
    out = torch.full((B, H, W, cout), float("nan"), device="cuda")
    assert lib.tdx_conv3x3_wino_ok(B, H, W, cin, cout)
    with L.tuned(**SPLITS[split]):
        if role == "fwd":
            L.check(lib.tdx_pack_conv3x3_wino(wd.data_ptr(), u.data_ptr(), None, cout, cin, stream()))
            bd = b.cuda()
            stats = torch.full((lib.tdx_conv3x3_wino_stat_tiles(B, H, W), 2, cout), float("nan"), device="cuda")
            L.check(lib.tdx_conv3x3_fwd_wino(xd.data_ptr(), u.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, W, cin, cout, 4,
                                             None, None, stats.data_ptr(), stream()))
        else:   # the layer is cout -> cin: its input-gradient pack serves the kernel's cin -> cout convolution
            L.check(lib.tdx_pack_conv3x3_wino(wd.data_ptr(), None, u.data_ptr(), cin, cout, stream()))
            stats = None
            L.check(lib.tdx_conv3x3_fwd_wino(xd.data_ptr(), u.data_ptr(), None, out.data_ptr(), B, H, W, cin, cout, 0,
                                             None, None, None, stream()))
        torch.cuda.synchronize()
    return out.cpu(), None if stats is None else stats.cpu()


def digest(t):
    return None if t is None else hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def block_of_pixel(B, H, W):
    """[B, H, W] index of the tile block (64 consecutive 2x2 tiles, images row-major) every output pixel belongs to."""
    th, tw = (H + 1) // 2, (W + 1) // 2
    b = torch.arange(B).view(B, 1, 1)
    ty = (torch.arange(H) // 2).view(1, H, 1)
    tx = (torch.arange(W) // 2).view(1, 1, W)
    return ((b * th + ty) * tw + tx) // 64


def stat_distances(out, stats, shape, rows):
    """(sum distance, M2 distance) of the partials from fp64 sums of the kernel's own output, in units of u."""
    B, H, W, cin, cout = shape
    blk = block_of_pixel(B, H, W).reshape(-1)
    nb = int(blk.max()) + 1
    assert stats.shape == (nb, 2, cout)
    y = out.double().reshape(-1, cout)
    cnt = torch.zeros(nb, dtype=torch.float64).index_add_(0, blk, torch.ones_like(blk, dtype=torch.float64))
    assert bool((cnt[:-1] == rows).all()) and 0 < cnt[-1] <= rows   # full blocks hold tdx_conv3x3_wino_stat_tile_rows pixels
    S = torch.zeros(nb, cout, dtype=torch.float64).index_add_(0, blk, y)
    A = torch.zeros(nb, cout, dtype=torch.float64).index_add_(0, blk, y.abs())
    mean = S / cnt[:, None]
    Q = torch.zeros(nb, cout, dtype=torch.float64).index_add_(0, blk, (y - mean[blk]) ** 2)
    sd = stats.double()
    assert bool((A > 0).all()) and bool((Q > 0).all())
    return ((sd[:, 0] - S).abs() / (U * A)).max().item(), ((sd[:, 1] - Q).abs() / (U * Q)).max().item()


@pytest.fixture(scope="module")
def tdx():
    import tiny_diffusion_amd._lib as L

    assert torch.cuda.is_available()
    return L


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["cases"] == [case_id(*c) for c in CASES], "the recorded case list is not this module's"
    return g["digests"]


@pytest.mark.parametrize("shape,role,split", CASES, ids=[case_id(*c) for c in CASES])
def test_wino_launch(tdx, golden, shape, role, split):
    from test_gpu_conv_launches import ELEM_WINO, REL_WINO, elem_ratio, rel_err

    B, H, W, cin, cout = shape
    out, stats = launch(tdx, shape, role, split)
    out2, stats2 = launch(tdx, shape, role, split)
    ref, mag, K = reference(shape, role)
    bad = []
    # 1. fp64
    nan = int(torch.isnan(out).sum()) + (0 if stats is None else int(torch.isnan(stats).sum()))
    if nan:
        bad.append(f"{nan} NaN (unwritten) elements")
    e, r = rel_err(out, ref), elem_ratio(out, ref, mag, K)
    print(f"\n{case_id(shape, role, split)}: rel {e:.2e} (gate {REL_WINO:.0e}), per-element ratio {r:.3f} (gate {ELEM_WINO:g})", end="")
    if not e < REL_WINO:
        bad.append(f"rel err {e:.2e} >= {REL_WINO:.0e}")
    if not r <= ELEM_WINO:
        bad.append(f"per-element ratio {r:.3g} > {ELEM_WINO:g}")
    if stats is not None and not nan:
        ds, dq = stat_distances(out, stats, shape, tdx.lib.tdx_conv3x3_wino_stat_tile_rows(B, H, W))
        print(f", statistics: sums {ds:.2f} u (gate {STAT_SUM_GATE:.2f}), M2 {dq:.2f} u (gate {STAT_M2_GATE:.2f})", end="")
        if not ds <= STAT_SUM_GATE:
            bad.append(f"statistics sums {ds:.2f} u from fp64 > {STAT_SUM_GATE:.2f}")
        if not dq <= STAT_M2_GATE:
            bad.append(f"statistics M2 {dq:.2f} u from fp64 > {STAT_M2_GATE:.2f}")
    print(flush=True)
    # 2. the recorded bits
    want = golden[case_id(shape, role, split)]
    if digest(out) != want["out"]:
        bad.append("output bits differ from the recorded ones")
    if digest(stats) != want["stats"]:
        bad.append("statistics bits differ from the recorded ones")
    # 3. deterministic
    if digest(out2) != digest(out) or digest(stats2) != digest(stats):
        bad.append("two launches differ")
    assert not bad, bad


def record(package_root, path):
    """Digests (and, printed, the statistics distances) of every case from the library of the checkout at package_root."""
    sys.path.insert(0, os.path.abspath(package_root))
    import tiny_diffusion_amd._lib as L

    assert os.path.abspath(L.__file__).startswith(os.path.abspath(package_root)), L.__file__
    digests = {}
    for shape, role, split in CASES:
        out, stats = launch(L, shape, role, split)
        assert not torch.isnan(out).any() and (stats is None or not torch.isnan(stats).any())
        digests[case_id(shape, role, split)] = {"out": digest(out), "stats": digest(stats)}
        line = case_id(shape, role, split)
        if stats is not None:
            ds, dq = stat_distances(out, stats, shape, L.lib.tdx_conv3x3_wino_stat_tile_rows(*shape[:3]))
            line += f": statistics distances from fp64: sums {ds:.3f} u, M2 {dq:.3f} u"
        print(line, flush=True)
    with open(path, "w") as f:
        json.dump({"cases": [case_id(*c) for c in CASES], "digests": digests}, f, indent=1)
        f.write("\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description="record the digests of tests/golden/wino_fixed_cost_digests.json")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    record(a.package_root, a.out)
