"""Every 3x3 convolution entry of include/tdx.h at maps with H != W, and the boundary convolutions at large batches,
against the fp64 references of tests/conv_helpers.py.

Every other kernel-level convolution test passes (B, H, H) and the plans of csrc/unet.hip are square, so a row stride of
H where W is meant, oh = r / H, tw used for th or exchanged bottom-row / right-column conditions would pass the whole
suite.  tests/test_conv_refs_host.py shows that such an exchange moves the reference of every map below by more than 1
(relative), against gates of 1e-5 and tighter.  Each launch goes through the public C entry with NaN-filled outputs and a
guard region behind every output, statistics and slab buffer (conv_helpers.Guards), and the activation operands lie
between NaN fences (Operands(fenced=True)): what a kernel reads outside its input and uses, be it times zero, shows as NaN;
the gates are the existing ones
(conv_helpers, tests/test_gpu_bf16.py, tests/test_gpu_ops.py), none new.  Shapes are (B, H, W), 64 -> 128 channels unless
said otherwise, each the smallest that reaches its branch; the branch is asserted through the library's introspection
where there is one.  Run with -s for the figures.

Winograd: both sides even - (3,6,10) 45 tiles, one ragged workgroup; (9,6,10) 135 tiles, three, the last ragged; H even
and W odd (5,8,7) - only the column flag c1 of the edge tiles is ever false - and its mirror (5,7,8); both odd (9,3,7); one
row (5,1,16); the row-split and the channel-split main loop, bit for bit; (2,14,7) and (2,5,6) refused by the forward
entries, computed by the weight gradient.
Direct fp32: (3,6,10), (5,8,7), (5,7,8), (2,5,12), (7,4,3); the three forward tiles forced at (5,8,7); the four
weight-gradient tiles (256 -> 256 and 512 -> 512 at (2,4,6)); narrow maps whose 32-pixel K-step spans 3 H rows or more.
bf16: (8,4,8) M % 256 == 0 with whole samples in a tile; (4,8,7) / (4,7,8) ragged M; (1,8,96) / (1,96,8) on the two sides
of the slot window's fit and of W <= 95 of the nine-tap weight gradient; BN + ReLU on load at (4,6,10).
Boundary convolutions: (3,6,5), (2,9,4) at the minimal W, (2,4,9), (5,7,8); W = 3 refused by the backward entries and
computed by the others; (33,40,50) = 129 partial rows -> the fold level; (66,40,50) = 8250 groups of 16 pixels > 8192
and (263,40,50) = 4110 tiles of 128 pixels > 4096 -> the grid-stride wraps."""
import pytest
import torch

import conv_helpers as CH
from conv_helpers import (ELEM_DIRECT, ELEM_WINO, REL_DIRECT, REL_WINO, TDX_E_SHAPE, EdgeOperands, Guards, Operands,
                          check_launch, conv_ref64, dgrad_ref64, elem_ratio, merge_stats, p, rel_err, run_dgrad, stream,
                          tile_blocks, wgrad_ref64)

pytestmark = pytest.mark.gpu

CIN, COUT = 64, 128
SMALLP_W = 2368   # floats per partial row of the boundary weight gradients (csrc/edge_conv.hip)


@pytest.fixture(scope="module")
def tdx():
    import tiny_diffusion_amd._lib as L

    assert torch.cuda.is_available()
    return L


def _id(s):
    return "x".join(str(v) for v in s)


def gate(fails, tag, got, ref, mag, K, rel_gate, elem_gate):
    """Norm-wise and per-element gate of one output; prints the figures, appends to fails."""
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    e, r = rel_err(got, ref), elem_ratio(got, ref, mag, K)
    print(f"  {tag}: rel {e:.2e} (gate {rel_gate:.0e})  elem {r:.3f} (gate {elem_gate:g})", flush=True)
    if not e < rel_gate:
        fails.append(f"{tag}: rel err {e:.2e} >= {rel_gate:.0e}")
    if not r <= elem_gate:
        fails.append(f"{tag}: per-element ratio {r:.3g} > {elem_gate:g}")


def gate_stats(fails, tag, stats, tiles, rows, ref):
    """Batch mean / biased variance rebuilt from the partials, at check_launch's tolerances."""
    flat = ref.reshape(-1, ref.shape[-1])
    mean, var = merge_stats(stats, tiles, rows, flat.shape[0])
    if not torch.allclose(mean, flat.mean(0), rtol=1e-4, atol=1e-5):
        fails.append(f"{tag}: batch mean")
    if not torch.allclose(var, flat.var(0, unbiased=False), rtol=1e-4, atol=1e-6):
        fails.append(f"{tag}: batch variance")


def launches(tdx, fails, B, H, W, cin, cout, roles, algo, seed, guards):
    for role in roles:
        row, f = check_launch(tdx, B, H, cin, cin, cout, role, algo, seed=seed, W=W, guards=guards, fenced=True)
        print(f"  {row}{'  FAIL ' + '; '.join(f) if f else ''}", flush=True)
        fails += [f"{role} {algo}: {m}" for m in f]


# ------------------------------------------------------------------------------------------------------------ Winograd
def test_wino_geometry(tdx):
    """The tile geometry the library reports for the maps below: 256 output pixels per workgroup where both sides are
    even, whole images per workgroup otherwise, the workgroup counts, and the two refused maps."""
    lib = tdx.lib
    for B, H, W in CH.WINO_SHAPES:
        assert lib.tdx_conv3x3_wino_ok(B, H, W, CIN, COUT) == 1 and lib.tdx_conv3x3_wino_ok(B, H, W, COUT, CIN) == 1
        th, tw = (H + 1) // 2, (W + 1) // 2
        rows = lib.tdx_conv3x3_wino_stat_tile_rows(B, H, W)
        if H % 2 == 0 and W % 2 == 0:
            assert rows == 256
        else:
            assert 64 % (th * tw) == 0 and rows == (64 // (th * tw)) * H * W
        assert lib.tdx_conv3x3_wino_stat_tiles(B, H, W) == tile_blocks(B, H, W)
    assert tile_blocks(3, 6, 10) == 1 and 3 * 3 * 5 == 45
    assert tile_blocks(9, 6, 10) == 3 and (9 * 3 * 5) % 64
    assert tile_blocks(5, 8, 7) == 2 and tile_blocks(9, 3, 7) == 2 and tile_blocks(5, 1, 16) == 1   # ragged last ones
    for B, H, W in CH.WINO_REFUSED:
        assert lib.tdx_conv3x3_wino_ok(B, H, W, CIN, COUT) == 0 and lib.tdx_conv3x3_wino_stat_tile_rows(B, H, W) == 0


def _wino_fwd(tdx, o, flags, guards):
    lib, B, H, W = tdx.lib, o.B, o.H, o.W
    out = guards.new((B, H, W, o.cout))
    tiles = lib.tdx_conv3x3_wino_stat_tiles(B, H, W)
    stats = guards.new((tiles, 2, o.cout))
    tdx.check(lib.tdx_conv3x3_fwd_wino(p(o.x), p(o.pack(tdx, "uf")), p(o.b), p(out), B, H, W, o.cin, o.cout, flags, None,
                                       None, p(stats) if flags else None, stream()))
    return out, stats


@pytest.mark.parametrize("shape", CH.WINO_SHAPES, ids=_id)
def test_wino_nonsquare(tdx, shape):
    """tdx_conv3x3_fwd_wino (statistics epilogue, plain, and as the input gradient), tdx_conv3x3_fwd_wino_infer split and
    unsplit and tdx_conv3x3_wgrad_wino, each beside the direct kernel on the same operands; then the training launches
    on the row-split and on the channel-split main loop, which must agree bit for bit."""
    B, H, W = shape
    G, fails = Guards(), []
    seed = 100 + CH.WINO_SHAPES.index(shape)
    launches(tdx, fails, B, H, W, CIN, COUT, ("fwd", "dgrad", "wgrad", "infer"), "wino", seed, G)
    o = Operands(B, H, CIN, CIN, COUT, seed, W=W, fenced=True)
    res = {}
    for rows in (0, 1):
        with tdx.tuned(wino_rows=rows, wino_rows_min_stages=1):
            res[rows] = (_wino_fwd(tdx, o, 4, G), _wino_fwd(tdx, o, 0, G)[0], run_dgrad(tdx, o, "wino", G))
        torch.cuda.synchronize()
    (y_c, st_c), y0_c, g_c = res[0]
    (y_r, st_r), y0_r, g_r = res[1]
    for name, a, b in (("output", y_r, y_c), ("statistics partials", st_r, st_c), ("plain output", y0_r, y0_c),
                       ("input gradient", g_r, g_c), ("plain vs statistics launch", y0_c, y_c)):
        if torch.isnan(a).any() or not torch.equal(a, b):
            fails.append(f"row split vs channel split: {name} differ or hold NaN")
    ref, mag, K = CH.role_reference(o, "fwd")
    gate(fails, "plain forward, row split", y0_r, ref, mag, K, REL_WINO, ELEM_WINO)
    # the inference launch with an ample scratch does split K at these sizes: its partials land in the scratch
    scr, out = G.new((8 * B * H * W * COUT,)), G.new((B, H, W, COUT))
    tdx.check(tdx.lib.tdx_conv3x3_fwd_wino_infer(p(o.x), p(o.pack(tdx, "uf")), p(o.b), p(out), B, H, W, CIN, COUT, p(o.osc),
                                                 p(o.osh), p(scr), scr.numel(), stream()))
    iref, imag, _ = CH.role_reference(o, "infer")
    gate(fails, "tdx_conv3x3_fwd_wino_infer, K split", out, iref, imag, K, REL_WINO, ELEM_WINO)
    if torch.isnan(scr).all():
        fails.append("tdx_conv3x3_fwd_wino_infer did not split K")
    assert G.intact(), "guard region written"
    assert not fails, fails


@pytest.mark.parametrize("shape", CH.WINO_REFUSED, ids=_id)
def test_wino_refused_geometries(tdx, shape):
    """Odd maps whose tiles do not pack into whole images per workgroup: the forward entries return TDX_E_SHAPE and write
    nothing; the weight gradient ("any H, W") computes."""
    lib = tdx.lib
    B, H, W = shape
    G, fails = Guards(), []
    o = Operands(B, H, CIN, CIN, COUT, 7, W=W, fenced=True)
    out, stats = G.new((B, H, W, COUT)), G.new((lib.tdx_conv3x3_wino_stat_tiles(B, H, W), 2, COUT))
    scratch = G.new((8 * B * H * W * COUT,))
    uf = o.pack(tdx, "uf")
    assert lib.tdx_conv3x3_fwd_wino(p(o.x), p(uf), p(o.b), p(out), B, H, W, CIN, COUT, 0, None, None, None,
                                    stream()) == TDX_E_SHAPE
    assert lib.tdx_conv3x3_fwd_wino(p(o.x), p(uf), p(o.b), p(out), B, H, W, CIN, COUT, 4, None, None, p(stats),
                                    stream()) == TDX_E_SHAPE
    assert lib.tdx_conv3x3_fwd_wino(p(o.dy), p(o.pack(tdx, "ug")), None, p(out), B, H, W, COUT, CIN, 0, None, None, None,
                                    stream()) == TDX_E_SHAPE
    for scr in (scratch, None):
        assert lib.tdx_conv3x3_fwd_wino_infer(p(o.x), p(uf), p(o.b), p(out), B, H, W, CIN, COUT, p(o.osc), p(o.osh), p(scr),
                                              0 if scr is None else scr.numel(), stream()) == TDX_E_SHAPE
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(stats).all() and torch.isnan(scratch).all()
    launches(tdx, fails, B, H, W, CIN, COUT, ("wgrad",), "wino", 7, G)
    assert G.intact(), "guard region written"
    assert not fails, fails


# --------------------------------------------------------------------------------------------------------- direct fp32
def _bn_operands(o, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    isc = torch.randn(o.cin, generator=g, device="cuda")
    ish = torch.randn(o.cin, generator=g, device="cuda") * 0.3
    a = torch.relu(o.x.double() * isc.double() + ish.double())
    amag = o.x.abs().double() * isc.abs().double() + ish.abs().double()   # what the fp32 fma's rounding scales with
    return isc, ish, a, amag


@pytest.mark.parametrize("shape", CH.DIRECT_SHAPES, ids=_id)
def test_direct_nonsquare(tdx, shape):
    """tdx_conv3x3_fwd_train (statistics; as the input gradient with its K split), tdx_conv3x3_fwd_splitk and
    tdx_conv3x3_fwd with the inference epilogue, tdx_conv3x3_wgrad + reduce (through check_launch); then tdx_conv3x3_fwd
    plain / statistics / BN + ReLU on load and in the epilogue, tdx_conv3x3_dgrad, tdx_conv3x3_fwd_infer at 3 and 4
    stages and the weight gradient of a BN + ReLU input."""
    lib = tdx.lib
    B, H, W = shape
    G, fails = Guards(), []
    seed = 200 + CH.DIRECT_SHAPES.index(shape)
    assert lib.tdx_conv3x3_train_scratch_floats(B, H, W, COUT, CIN) > 0, "the input gradient was expected to split K"
    assert lib.tdx_conv3x3_splitk_scratch_floats(B, H, W, CIN, COUT) > 0, "the inference launch was expected to split K"
    launches(tdx, fails, B, H, W, CIN, COUT, ("fwd", "dgrad", "wgrad", "infer"), "direct", seed, G)

    o = Operands(B, H, CIN, CIN, COUT, seed, W=W, fenced=True)
    wf, wg = o.pack(tdx, "wf"), o.pack(tdx, "wg")
    ref, mag, K = CH.role_reference(o, "fwd")
    tiles, rows = lib.tdx_conv3x3_stat_tiles(B, H, W, CIN, COUT), lib.tdx_conv3x3_stat_tile_rows(B, H, W, CIN, COUT)
    for flags in (0, 4):
        out, stats = G.new((B, H, W, COUT)), G.new((tiles, 2, COUT))
        tdx.check(lib.tdx_conv3x3_fwd(p(o.x), p(wf), p(o.b), p(out), B, H, W, CIN, COUT, flags, None, None, None, None,
                                      p(stats) if flags else None, stream()))
        gate(fails, f"tdx_conv3x3_fwd flags {flags}", out, ref, mag, K, REL_DIRECT["fwd"], ELEM_DIRECT)
        if flags:
            gate_stats(fails, "tdx_conv3x3_fwd statistics", stats, tiles, rows, ref)
    # BN + ReLU on load, BN + ReLU epilogue
    isc, ish, a, amag = _bn_operands(o, seed + 50)
    sc, sh = o.osc.double(), o.osh.double()
    ref_bn = torch.relu(conv_ref64(a, o.w, o.b) * sc + sh)
    mag_bn = conv_ref64(amag, o.w.abs(), o.b.abs()) * sc.abs() + sh.abs()
    out = G.new((B, H, W, COUT))
    tdx.check(lib.tdx_conv3x3_fwd(p(o.x), p(wf), p(o.b), p(out), B, H, W, CIN, COUT, 1 | 2, p(isc), p(ish), p(o.osc),
                                  p(o.osh), None, stream()))
    gate(fails, "tdx_conv3x3_fwd IN_BNRELU | OUT_BNRELU", out, ref_bn, mag_bn, K, REL_DIRECT["infer"], ELEM_DIRECT)
    # the input-gradient entry
    dref, dmag, dK = CH.role_reference(o, "dgrad")
    dx = G.new((B, H, W, CIN))
    tdx.check(lib.tdx_conv3x3_dgrad(p(o.dy), p(wg), p(dx), B, H, W, CIN, COUT, stream()))
    gate(fails, "tdx_conv3x3_dgrad", dx, dref, dmag, dK, REL_DIRECT["dgrad"], ELEM_DIRECT)
    # the inference convolution on the tile-major pack, both ring depths
    iref, imag, _ = CH.role_reference(o, "infer")
    wt = torch.full((COUT * 9 * CIN,), float("nan"), device="cuda")
    tdx.check(lib.tdx_pack_conv3x3_tiled(p(o.w), p(wt), COUT, CIN, stream()))
    need = lib.tdx_conv3x3_infer_scratch_floats(B, H, W, CIN, COUT)
    for stages in (3, 4):
        with tdx.tuned(infer_stages=stages):
            for scr in ((G.new((need,)) if need else None), None):
                out = G.new((B, H, W, COUT))
                tdx.check(lib.tdx_conv3x3_fwd_infer(p(o.x), p(wt), p(o.b), p(out), B, H, W, CIN, COUT, p(o.osc), p(o.osh),
                                                    p(scr), 0 if scr is None else scr.numel(), stream()))
                gate(fails, f"tdx_conv3x3_fwd_infer {stages} stages, {'planned' if scr is not None else 'unsplit'}", out,
                     iref, imag, K, REL_DIRECT["infer"], ELEM_DIRECT)
    # weight gradient of a BN + ReLU input
    splits = lib.tdx_conv3x3_wgrad_splits(B, H, W, CIN, COUT)
    slabs, dw = G.new((splits, COUT, 9, CIN)), G.new((COUT, CIN, 3, 3))
    tdx.check(lib.tdx_conv3x3_wgrad(p(o.x), p(o.dy), p(slabs), B, H, W, CIN, COUT, 1, p(isc), p(ish), stream()))
    tdx.check(lib.tdx_conv3x3_wgrad_reduce(p(slabs), p(dw), splits, COUT, CIN, stream()))
    gate(fails, "tdx_conv3x3_wgrad IN_BNRELU", dw, wgrad_ref64(a, o.dy), wgrad_ref64(amag, o.dy.abs()), B * H * W,
         REL_DIRECT["wgrad"], ELEM_DIRECT)
    assert G.intact(), "guard region written"
    assert not fails, fails


def test_direct_forward_tile_templates(tdx):
    """Each of the three forward tile templates, forced with the knob conv_tile, at (5,8,7): 280 pixels = three ragged
    128-row tiles or five 64-row ones."""
    lib = tdx.lib
    B, H, W = 5, 8, 7
    G, fails = Guards(), []
    o = Operands(B, H, CIN, CIN, COUT, 300, W=W, fenced=True)
    ref, mag, K = CH.role_reference(o, "fwd")
    for force, want in ((1, 128128), (2, 128064), (3, 64064)):
        with tdx.tuned(conv_tile=force):
            assert lib.tdx_conv3x3_tile_shape(B, H, W, CIN, COUT, 0) == want
            tiles, rows = lib.tdx_conv3x3_stat_tiles(B, H, W, CIN, COUT), lib.tdx_conv3x3_stat_tile_rows(B, H, W, CIN, COUT)
            out, stats = G.new((B, H, W, COUT)), G.new((tiles, 2, COUT))
            tdx.check(lib.tdx_conv3x3_fwd(p(o.x), p(o.pack(tdx, "wf")), p(o.b), p(out), B, H, W, CIN, COUT, 4, None, None,
                                          None, None, p(stats), stream()))
        gate(fails, f"tile {want}", out, ref, mag, K, REL_DIRECT["fwd"], ELEM_DIRECT)
        gate_stats(fails, f"tile {want} statistics", stats, tiles, rows, ref)
    assert lib.tdx_conv3x3_tile_shape(B, H, W, CIN, COUT, 0) == 64064   # the heuristic is back
    assert G.intact(), "guard region written"
    assert not fails, fails


WGRAD_TILES = [((3, 6, 10), 64, 128, 128064), ((3, 6, 10), 128, 64, 64128), (CH.DIRECT_WIDE, 256, 256, 128128),
               (CH.DIRECT_WIDE, 512, 512, 64064)]


@pytest.mark.parametrize("shape,cin,cout,want", WGRAD_TILES, ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_direct_wgrad_tile_shapes(tdx, shape, cin, cout, want):
    """Every weight-gradient tile the plan can pick at these sizes (128 wide where the channel count divides by 128,
    64 x 64 for big weights on few pixels)."""
    B, H, W = shape
    G, fails = Guards(), []
    assert tdx.lib.tdx_conv3x3_tile_shape(B, H, W, cin, cout, 1) == want
    launches(tdx, fails, B, H, W, cin, cout, ("wgrad",), "direct", 400 + cin, G)
    assert not fails, fails


def test_wgrad_tile_cases_cover_the_templates():
    assert {c[3] for c in WGRAD_TILES} == {128128, 128064, 64128, 64064}


@pytest.mark.parametrize("shape", CH.DIRECT_WGRAD_NARROW, ids=_id)
def test_direct_narrow_maps(tdx, shape):
    """Maps on which the 32 pixels of a K-step span 3 H rows or more ((6,4,2), (9,8,1)) or that have fewer than four rows
    ((7,2,5), (5,1,16)): the weight-gradient kernels advance (oh, ow) by adds and conditional subtracts, which the host
    must keep within one wrap of H (it returned wrong numbers at (6,4,2) and refused the last two).  The forwards on the
    same maps, which divide."""
    B, H, W = shape
    G, fails = Guards(), []
    assert B * H * W > 32, "more than one K-step"
    launches(tdx, fails, B, H, W, CIN, COUT, ("wgrad", "fwd", "dgrad", "infer"), "direct", 500 + H * W, G)
    assert not fails, fails


def test_direct_wgrad_reads_nothing_behind_its_input(tdx):
    """(9,3,7): 189 pixels, the last 32-pixel K-step has 29.  The weight-gradient kernels judge a row's taps on (oh, ow)
    alone, so the three rows past the end have valid taps too; the input descriptor must end with the tensor, or they
    are fetched from whatever follows it (and 0 x NaN is NaN).  Plain and BN + ReLU on load: one kernel each."""
    lib = tdx.lib
    B, H, W = 9, 3, 7
    assert (B * H * W) % 32
    G, fails = Guards(), []
    o = Operands(B, H, CIN, CIN, COUT, 9, W=W, fenced=True)
    isc, ish, a, amag = _bn_operands(o, 59)
    splits = lib.tdx_conv3x3_wgrad_splits(B, H, W, CIN, COUT)
    for flags, x64, m64 in ((0, o.x, o.x.abs()), (1, a, amag)):
        slabs, dw = G.new((splits, COUT, 9, CIN)), G.new((COUT, CIN, 3, 3))
        tdx.check(lib.tdx_conv3x3_wgrad(p(o.x), p(o.dy), p(slabs), B, H, W, CIN, COUT, flags, p(isc), p(ish), stream()))
        tdx.check(lib.tdx_conv3x3_wgrad_reduce(p(slabs), p(dw), splits, COUT, CIN, stream()))
        gate(fails, f"tdx_conv3x3_wgrad flags {flags}, fenced input", dw, wgrad_ref64(x64, o.dy), wgrad_ref64(m64, o.dy.abs()),
             B * H * W, REL_DIRECT["wgrad"], ELEM_DIRECT)
    assert G.intact(), "guard region written"
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------- bf16
def _bf16_pack(tdx, w):
    cout, cin = w.shape[:2]
    wf16 = torch.empty(cout * 9 * cin, dtype=torch.bfloat16, device="cuda")
    wg16 = torch.empty(cout * 9 * cin, dtype=torch.bfloat16, device="cuda")
    tdx.check(tdx.lib.tdx_pack_conv3x3_bf16(p(w), p(wf16), p(wg16), cout, cin, stream()))
    return wf16, wg16


def _r16(t):
    return t.bfloat16().double()


def _tile_stats_ok(stats, flat, rows, atol):
    for ti in range(stats.shape[0]):
        blk = flat[ti * rows:(ti + 1) * rows]
        if not (torch.allclose(stats[ti, 0].double(), blk.sum(0), rtol=1e-4, atol=atol)
                and torch.allclose(stats[ti, 1].double(), (blk - blk.mean(0)).pow(2).sum(0), rtol=1e-4, atol=atol)):
            return False
    return True


def _bf16_fp32_entries(tdx, B, H, W, seed, in_bn, G, fails):
    """tdx_conv3x3_fwd_bf16 (statistics; as the input gradient) and tdx_conv3x3_wgrad_bf16 against fp64 on bf16-rounded
    operands, 2e-5 (tests/test_gpu_bf16.py::test_bf16_conv_fwd_dgrad_wgrad)."""
    lib = tdx.lib
    o = Operands(B, H, CIN, CIN, COUT, seed, W=W, fenced=True)
    wf16, wg16 = _bf16_pack(tdx, o.w)
    isc = ish = None
    a = _r16(o.x)
    if in_bn:   # the kernel's fp32 fma (exact product, one rounding), then bf16
        isc, ish, _, _ = _bn_operands(o, seed + 50)
        a = _r16(torch.relu((o.x.double() * isc.double() + ish.double()).float()))
    wr, dyr = _r16(o.w), _r16(o.dy)
    ref = conv_ref64(a, wr, o.b)
    rows = lib.tdx_conv3x3_bf16_stat_tile_rows()
    tiles = -(-B * H * W // rows)
    out, stats = G.new((B, H, W, COUT)), G.new((tiles, 2, COUT))
    tdx.check(lib.tdx_conv3x3_fwd_bf16(p(o.x), p(wf16), p(o.b), p(out), B, H, W, CIN, COUT, 4 | (1 if in_bn else 0), p(isc),
                                       p(ish), None, None, p(stats), stream()))
    gin = G.new((B, H, W, CIN))
    tdx.check(lib.tdx_conv3x3_fwd_bf16(p(o.dy), p(wg16), None, p(gin), B, H, W, COUT, CIN, 0, None, None, None, None, None,
                                       stream()))
    splits = lib.tdx_conv3x3_wgrad_splits_bf16(B, H, W, CIN, COUT)
    slabs, dw = G.new((splits, COUT, 9, CIN)), G.new((COUT, CIN, 3, 3))
    tdx.check(lib.tdx_conv3x3_wgrad_bf16(p(o.x), p(o.dy), p(slabs), B, H, W, CIN, COUT, 1 if in_bn else 0, p(isc), p(ish),
                                         stream()))
    tdx.check(lib.tdx_conv3x3_wgrad_reduce(p(slabs), p(dw), splits, COUT, CIN, stream()))
    torch.cuda.synchronize()
    figs = {"fwd": rel_err(out, ref), "dgrad": rel_err(gin, dgrad_ref64(dyr, wr)), "wgrad": rel_err(dw, wgrad_ref64(a, dyr))}
    print(f"  bf16 fp32-tensor entries {B}x{H}x{W} in_bn={in_bn}: " + " ".join(f"{k} {v:.2e}" for k, v in figs.items())
          + " (gate 2e-05)", flush=True)
    fails += [f"fp32-tensor {k}: rel err {v:.2e} >= 2e-5" for k, v in figs.items() if not v < 2e-5]
    if not _tile_stats_ok(stats, out.reshape(-1, COUT).double(), rows, 1e-3):   # statistics of what was written
        fails.append("fp32-tensor statistics partials")


def _bf16_io16(tdx, B, H, W, seed, in_bn, knobs, G, fails):
    """tdx_conv3x3_fwd_bf16_io / tdx_conv3x3_wgrad_bf16_io with io16 = 1 at the gates of
    tests/test_gpu_bf16.py::test_bf16_storage_kernels; returns (out, gin, dw)."""
    lib = tdx.lib
    o = Operands(B, H, CIN, CIN, COUT, seed, W=W, fenced=True)
    x16, dy16 = o.x.bfloat16(), o.dy.bfloat16()
    wf16, wg16 = _bf16_pack(tdx, o.w)
    isc = ish = None
    a = x16.double()
    if in_bn:
        g = torch.Generator(device="cuda").manual_seed(seed + 50)
        isc = torch.rand(CIN, generator=g, device="cuda") + 0.5
        ish = torch.randn(CIN, generator=g, device="cuda") * 0.3
        a = _r16(torch.relu((x16.double() * isc.double() + ish.double()).float()))
    wr = _r16(o.w)
    ref = conv_ref64(a, wr, o.b)
    rows = lib.tdx_conv3x3_bf16_stat_tile_rows()
    tiles = -(-B * H * W // rows)
    out, stats = G.new((B, H, W, COUT), torch.bfloat16), G.new((tiles, 2, COUT))
    gin = G.new((B, H, W, CIN), torch.bfloat16)
    dw = G.new((COUT, CIN, 3, 3))
    with tdx.tuned(**knobs):
        splits = lib.tdx_conv3x3_wgrad_splits_bf16(B, H, W, CIN, COUT)
        slabs = G.new((splits, COUT, 9, CIN))
        tdx.check(lib.tdx_conv3x3_fwd_bf16_io(p(x16), p(wf16), p(o.b), p(out), B, H, W, CIN, COUT, 4 | (1 if in_bn else 0),
                                              p(isc), p(ish), None, None, p(stats), 1, stream()))
        tdx.check(lib.tdx_conv3x3_fwd_bf16_io(p(dy16), p(wg16), None, p(gin), B, H, W, COUT, CIN, 0, None, None, None, None,
                                              None, 1, stream()))
        tdx.check(lib.tdx_conv3x3_wgrad_bf16_io(p(x16), p(dy16), p(slabs), B, H, W, CIN, COUT, 1 if in_bn else 0, p(isc),
                                                p(ish), 1, stream()))
        tdx.check(lib.tdx_conv3x3_wgrad_reduce(p(slabs), p(dw), splits, COUT, CIN, stream()))
        torch.cuda.synchronize()
    dref = dgrad_ref64(dy16.double(), wr)
    e_out, e_gin, e_dw = rel_err(out, ref), rel_err(gin, dref), rel_err(dw, wgrad_ref64(a, dy16.double()))
    worst = ((out.double() - ref).abs().max() / (2.0 ** -8 * ref.abs().max() + 1e-6)).item()
    print(f"  bf16 io16 {B}x{H}x{W} in_bn={in_bn} {knobs or 'default'}: fwd {e_out:.2e} dgrad {e_gin:.2e} (gate 3e-03)  "
          f"max elem / bound {worst:.3f}  wgrad {e_dw:.2e} (gate 2e-05)", flush=True)
    if not (torch.isfinite(out.float()).all() and torch.isfinite(gin.float()).all()):
        fails.append("io16: unwritten or non-finite elements")
    if not e_out < 3e-3:
        fails.append(f"io16 forward rel err {e_out:.2e}")
    if not worst <= 1.0:
        fails.append(f"io16 forward element error {worst:.3f} x (2^-8 max|ref| + 1e-6)")
    if not e_gin < 3e-3:
        fails.append(f"io16 input gradient rel err {e_gin:.2e}")
    if not e_dw < 2e-5:
        fails.append(f"io16 weight gradient rel err {e_dw:.2e}")
    if not _tile_stats_ok(stats, ref.reshape(-1, COUT), rows, 2e-3):   # from the fp32 accumulators
        fails.append("io16 statistics partials")
    return out, gin, dw


BF16_VARIANTS = {"default": {}, "per_tap": {"bf16_wgrad9": 0}, "thin0": {"bf16_thin": 0}}


@pytest.mark.parametrize("shape", CH.BF16_SHAPES, ids=_id)
def test_bf16_nonsquare(tdx, shape):
    """The fp32-tensor entries, then the bf16-storage forms in the default variant, with the per-tap weight gradient and
    without the slot-window forward.  At (1,8,96) the window does not fit and W > 95: the default variant must then be
    the other two, bit for bit."""
    B, H, W = shape
    G, fails = Guards(), []
    seed = 600 + CH.BF16_SHAPES.index(shape)
    _bf16_fp32_entries(tdx, B, H, W, seed, 0, G, fails)
    res = {v: _bf16_io16(tdx, B, H, W, seed, 0, k, G, fails) for v, k in BF16_VARIANTS.items()}
    if shape == (1, 8, 96):
        if not (torch.equal(res["default"][0], res["thin0"][0]) and torch.equal(res["default"][1], res["thin0"][1])):
            fails.append("W = 96: the forward did not fall through to the variant without the slot window")
        if not torch.equal(res["default"][2], res["per_tap"][2]):
            fails.append("W = 96: the weight gradient did not fall through to the per-tap kernel")
    assert G.intact(), "guard region written"
    assert not fails, fails


def test_bf16_bn_relu_on_load_nonsquare(tdx):
    B, H, W = CH.BF16_BN_SHAPE
    G, fails = Guards(), []
    _bf16_fp32_entries(tdx, B, H, W, 650, 1, G, fails)
    _bf16_io16(tdx, B, H, W, 650, 1, {}, G, fails)
    assert G.intact(), "guard region written"
    assert not fails, fails


# ----------------------------------------------------------------------------------------------- boundary convolutions
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _edge_initial_forward(tdx, e, G, fails):
    B, H, W, ct, cf = e.B, e.H, e.W, e.ct, e.cf
    out = G.new((B, H, W, 64))
    tdx.check(tdx.lib.tdx_initial_conv_forward(p(e.x), p(e.w_init), p(e.b_init), p(out), B, H, W, ct, cf, stream()))
    x = e.x_nhwc
    gate(fails, "tdx_initial_conv_forward", out[..., :cf], conv_ref64(x, e.w_init, e.b_init),
         conv_ref64(x.abs(), e.w_init.abs(), e.b_init.abs()), 9 * ct, 2e-6, ELEM_DIRECT)
    if cf < 64 and not bool((out[..., cf:] == 0).all()):
        fails.append("tdx_initial_conv_forward: padding channels are not zero")


def _edge_initial_backward(tdx, e, G, fails):
    B, H, W, ct, cf = e.B, e.H, e.W, e.ct, e.cf
    scratch = G.new((tdx.lib.tdx_edge_conv_wgrad_scratch_floats(B, H, W),))
    dw, db = G.new((cf, ct, 3, 3)), G.new((cf,))
    tdx.check(tdx.lib.tdx_initial_conv_backward(p(e.x), p(e.g_fat), p(dw), p(db), p(scratch), B, H, W, ct, cf, stream()))
    x, g = e.x_nhwc, e.g_fat[..., :cf]
    gate(fails, "tdx_initial_conv_backward dw", dw, wgrad_ref64(x, g), wgrad_ref64(x.abs(), g.abs()), B * H * W, 3e-6,
         ELEM_DIRECT)
    gate(fails, "tdx_initial_conv_backward db", db, g.double().sum((0, 1, 2)), g.double().abs().sum((0, 1, 2)), B * H * W,
         3e-6, ELEM_DIRECT)


def _edge_initial_input_grad(tdx, e, G, fails):
    B, H, W, ct, cf = e.B, e.H, e.W, e.ct, e.cf
    gx = G.new((B, ct, H, W))
    tdx.check(tdx.lib.tdx_initial_conv_input_grad(p(e.g_fat), p(e.w_init), p(gx), B, H, W, ct, cf, stream()))
    g = e.g_fat[..., :cf]   # the stored channels >= cf hold values that must not leak in
    gate(fails, "tdx_initial_conv_input_grad", gx, _nchw(dgrad_ref64(g, e.w_init)),
         _nchw(dgrad_ref64(g.abs(), e.w_init.abs())), 9 * 64, 2e-6, ELEM_DIRECT)


def _edge_final_forward(tdx, e, G, fails):
    B, H, W, ct = e.B, e.H, e.W, e.ct
    out = G.new((B, ct, H, W))
    tdx.check(tdx.lib.tdx_final_conv_forward(p(e.fat), p(e.w_fin), p(e.b_fin), p(out), B, H, W, ct, stream()))
    gate(fails, "tdx_final_conv_forward", out, _nchw(conv_ref64(e.fat, e.w_fin, e.b_fin)),
         _nchw(conv_ref64(e.fat.abs(), e.w_fin.abs(), e.b_fin.abs())), 9 * 64, 2e-6, ELEM_DIRECT)


def _edge_final_backward(tdx, e, G, fails):
    B, H, W, ct = e.B, e.H, e.W, e.ct
    scratch = G.new((tdx.lib.tdx_edge_conv_wgrad_scratch_floats(B, H, W),))
    gin, dw, db = G.new((B, H, W, 64)), G.new((ct, 64, 3, 3)), G.new((ct,))
    tdx.check(tdx.lib.tdx_final_conv_backward(p(e.fat), p(e.g_thin), p(e.w_fin), p(gin), p(dw), p(db), p(scratch), B, H, W,
                                              ct, stream()))
    g = e.g_thin_nhwc
    gate(fails, "tdx_final_conv_backward g_in", gin, dgrad_ref64(g, e.w_fin), dgrad_ref64(g.abs(), e.w_fin.abs()), 9 * ct,
         3e-6, ELEM_DIRECT)
    gate(fails, "tdx_final_conv_backward dw", dw, wgrad_ref64(e.fat, g), wgrad_ref64(e.fat.abs(), g.abs()), B * H * W, 3e-6,
         ELEM_DIRECT)
    gate(fails, "tdx_final_conv_backward db", db, g.double().sum((0, 1, 2)), g.double().abs().sum((0, 1, 2)), B * H * W,
         3e-6, ELEM_DIRECT)


EDGE_ENTRIES = (_edge_initial_forward, _edge_initial_backward, _edge_initial_input_grad, _edge_final_forward,
                _edge_final_backward)


@pytest.mark.parametrize("ct,cf", CH.EDGE_PAIRS)
@pytest.mark.parametrize("shape", CH.EDGE_SMALL, ids=_id)
def test_edge_conv_nonsquare(tdx, shape, ct, cf):
    """All five entries of the boundary convolutions: forwards at 2e-6, gradients at 3e-6 (tests/test_gpu_ops.py), and per
    element with K = 9 cin (forwards), 9 x the stored channels of the gradient read (input gradients), B H W (weight and
    bias gradients)."""
    B, H, W = shape
    G, fails = Guards(), []
    e = EdgeOperands(B, H, W, ct, cf, 700 + H * W + ct)
    print(f"\nedge {ct}->{cf} {B}x{H}x{W}")
    for entry in EDGE_ENTRIES:
        entry(tdx, e, G, fails)
    assert G.intact(), "guard region written"
    assert not fails, fails


@pytest.mark.parametrize("ct,cf", CH.EDGE_PAIRS)
def test_edge_conv_w3(tdx, ct, cf):
    """W < 4: the weight-gradient kernel walks pixel pairs and needs W >= 4, so both backward entries return TDX_E_SHAPE
    and write nothing (not the input gradient of tdx_final_conv_backward either); the two forwards and
    tdx_initial_conv_input_grad have no such limit and compute."""
    lib = tdx.lib
    B, H, W = 2, 5, 3
    G, fails = Guards(), []
    e = EdgeOperands(B, H, W, ct, cf, 11)
    scratch = G.new((lib.tdx_edge_conv_wgrad_scratch_floats(B, H, W),))
    dw, db, gin = G.new((cf, ct, 3, 3)), G.new((cf,)), G.new((B, H, W, 64))
    assert lib.tdx_initial_conv_backward(p(e.x), p(e.g_fat), p(dw), p(db), p(scratch), B, H, W, ct, cf,
                                         stream()) == TDX_E_SHAPE
    dw2, db2 = G.new((ct, 64, 3, 3)), G.new((ct,))
    assert lib.tdx_final_conv_backward(p(e.fat), p(e.g_thin), p(e.w_fin), p(gin), p(dw2), p(db2), p(scratch), B, H, W, ct,
                                       stream()) == TDX_E_SHAPE
    torch.cuda.synchronize()
    for t in (dw, db, dw2, db2, gin, scratch):
        assert torch.isnan(t).all()
    print(f"\nedge {ct}->{cf} {B}x{H}x{W}")
    for entry in (_edge_initial_forward, _edge_initial_input_grad, _edge_final_forward):
        entry(tdx, e, G, fails)
    assert G.intact(), "guard region written"
    assert not fails, fails


def test_edge_large_batch_counts(tdx):
    """The arithmetic behind the three large shapes, from the constants of csrc/edge_conv.hip: 512 pixels per partial row
    and a fold level above 128 rows; grids capped at 8192 groups of 16 pixels and at 4096 tiles of 128 pixels."""
    lib = tdx.lib
    assert lib.tdx_edge_conv_wgrad_scratch_floats(33, 40, 50) == 129 * SMALLP_W and 33 * 40 * 50 % 512
    assert lib.tdx_edge_conv_wgrad_scratch_floats(32, 40, 50) == 125 * SMALLP_W     # (under the fold's threshold)
    assert -(-66 * 40 * 50 // 16) == 8250 > 8192 and 66 * 40 * 50 % 16 == 0 and 66 * 40 * 50 % 128
    assert -(-263 * 40 * 50 // 128) == 4110 > 4096 and 263 * 40 * 50 % 128
    for B, H, W in CH.EDGE_LARGE:
        assert H != W


@pytest.mark.parametrize("ct,cf", CH.EDGE_PAIRS)
def test_edge_fold_level_of_the_weight_gradients(tdx, ct, cf):
    """(33,40,50): 66 000 pixels = 129 partial rows, the last one ragged - more than 128, so both weight gradients take
    the in-place first reduction level.  dw and db per element with K = 66 000."""
    G, fails = Guards(), []
    e = EdgeOperands(33, 40, 50, ct, cf, 801 + ct)
    print(f"\nedge {ct}->{cf} 33x40x50")
    _edge_initial_backward(tdx, e, G, fails)
    _edge_final_backward(tdx, e, G, fails)
    assert G.intact(), "guard region written"
    assert not fails, fails


@pytest.mark.parametrize("ct,cf", CH.EDGE_PAIRS)
def test_edge_wrap_of_the_fat_to_thin_kernel(tdx, ct, cf):
    """(66,40,50): 8250 groups of 16 pixels on a grid of 8192 - tdx_final_conv_forward and tdx_initial_conv_input_grad
    stride over the grid once more."""
    G, fails = Guards(), []
    e = EdgeOperands(66, 40, 50, ct, cf, 802 + ct)
    print(f"\nedge {ct}->{cf} 66x40x50")
    _edge_final_forward(tdx, e, G, fails)
    _edge_initial_input_grad(tdx, e, G, fails)
    assert G.intact(), "guard region written"
    assert not fails, fails


@pytest.mark.parametrize("ct,cf", CH.EDGE_PAIRS)
def test_edge_wrap_of_the_thin_to_fat_kernel(tdx, ct, cf):
    """(263,40,50): 4110 tiles of 128 pixels on a grid of 4096 - tdx_initial_conv_forward and the input gradient of
    tdx_final_conv_backward stride over the grid once more (the fat tensor is 135 MB)."""
    G, fails = Guards(), []
    e = EdgeOperands(263, 40, 50, ct, cf, 803 + ct)
    print(f"\nedge {ct}->{cf} 263x40x50")
    _edge_initial_forward(tdx, e, G, fails)
    _edge_final_backward(tdx, e, G, fails)
    assert G.intact(), "guard region written"
    assert not fails, fails
