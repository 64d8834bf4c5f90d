"""Every branch of csrc/bn.hip and csrc/spatial.hip against fp64, per element: tdx_bn_finalize,
tdx_bn_apply_relu_fwd, tdx_bn_relu_bwd, tdx_maxpool2_ceil_{fwd,bwd} and tdx_bilinear_ac_{fwd,bwd} through the C ABI, at
non-square shapes, at every kernel the host code can pick and at both sides of every grid cap and stride loop.

References, bounds and input builders are those of tests/spatial_helpers.py (checked on the CPU by
tests/test_spatial_refs_host.py, which also states which branch each case below reaches): fp64 from the kernel's own fp32
operands; |got - ref| <= 9 u sqrt(K) x magnitude-sum per element, K read off the kernel in each docstring; bit for bit
where the operands are dyadic.  Every output is pre-filled with a sentinel and followed by guard floats; a slice
destination sits inside a wider tensor whose other channels must not move.  The norm-wise gates of
tests/test_gpu_ops.py stay where they are."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import spatial_helpers as S  # noqa: E402

DEV = "cuda"
GUARD = 64
NAN = float("nan")


@pytest.fixture(scope="module")
def tdx():
    import tiny_diffusion_amd._lib as L

    assert torch.cuda.is_available()
    return L


def call(tdx, name, *args):
    """One C-ABI call on the current stream: tensors by address, None as NULL.  Synchronises, so the operands outlive
    the kernel.  Returns the status."""
    rc = getattr(tdx.lib, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args],
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def guarded(shape, fill, init=None, dtype=torch.float32):
    """(buffer, view): a tensor of `shape` filled with `fill` (or holding `init`), GUARD more elements behind it."""
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    view = buf[:n].view(shape)
    if init is not None:
        view.copy_(init)
    return buf, view


def untouched(t, fill):
    return bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all())


def guard_ok(buf, fill):
    return untouched(buf[-GUARD:], fill)


def _id(case):
    return "-".join(str(int(x)) for x in case)


# ------------------------------------------------------------------------------------------------ tdx_bn_finalize
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("case", S.FINALIZE_CASES, ids=_id)
def test_bn_finalize_per_channel(tdx, case, training):
    """scale, shift, save_mean, save_rstd, running_mean, running_var of every channel against the fp64 merge of the same
    partials (spatial_helpers.bn_finalize_ref, which derives K = 1 ... 7 per quantity), num_batches_tracked advanced once;
    in eval mode the running buffers and the counter must not move.  tiles = 1, 2, 3, 256, 257 and 600 walk the 256-wide
    tile loop zero to three times per thread; two cases end in a one-row tile; count = 2 and count > 2^24; C = 4 is one
    block, 1024 is 256 blocks."""
    tiles, tile_rows, count, C, big = case
    d = S.bn_finalize_operands(tiles, tile_rows, count, C, S.case_seed(tiles, tile_rows, C), DEV, big)
    out = {k: guarded((C,), 7.0) for k in ("scale", "shift", "save_mean", "save_rstd")}
    rm_buf, rm = guarded((C,), 7.0, d["running_mean"])
    rv_buf, rv = guarded((C,), 7.0, d["running_var"])
    nbt = torch.tensor([3, 77], dtype=torch.int64, device=DEV)
    rc = call(tdx, "tdx_bn_finalize", d["stats"], tiles, tile_rows, count, C, d["gamma"], d["beta"], rm, rv, nbt,
              out["scale"][1], out["shift"][1], out["save_mean"][1], out["save_rstd"][1], training)
    assert rc == 0
    ref = S.bn_finalize_ref(d["stats"], tile_rows, count, d["gamma"], d["beta"], d["running_mean"], d["running_var"],
                            bool(training))
    got = {k: v[1] for k, v in out.items()}
    got["running_mean"], got["running_var"] = rm, rv
    ratios = {k: S.elem_ratio(got[k], *ref[k]) for k in ref}
    print("bn_finalize", case, training, {k: round(v, 3) for k, v in ratios.items()})
    assert all(r <= 1.0 for r in ratios.values()), ratios
    if training:
        assert nbt.tolist() == [4, 77]
    else:
        assert torch.equal(rm, d["running_mean"]) and torch.equal(rv, d["running_var"]) and nbt.tolist() == [3, 77]
    assert all(guard_ok(b, 7.0) for b, _ in out.values()) and guard_ok(rm_buf, 7.0) and guard_ok(rv_buf, 7.0)


@pytest.mark.parametrize("C", [6, 2, 1022])
def test_bn_finalize_refuses_widths_that_are_no_multiple_of_four(tdx, C):
    """The kernel reads one float4 = 4 channels of a tile: C % 4 != 0 is TDX_E_SHAPE before any launch, like every
    sibling entry, and nothing is written."""
    d = S.bn_finalize_operands(3, 5, 13, 1024, 1, DEV, False)    # buffers larger than any read such a C could ask for
    out = [guarded((1024,), 7.0) for _ in range(4)]
    nbt = torch.tensor([3], dtype=torch.int64, device=DEV)
    for training in (1, 0):
        rm, rv = d["running_mean"].clone(), d["running_var"].clone()
        rc = call(tdx, "tdx_bn_finalize", d["stats"], 3, 5, 13, C, d["gamma"], d["beta"], rm, rv, nbt,
                  out[0][1], out[1][1], out[2][1], out[3][1], training)
        assert rc == S.TDX_E_SHAPE
        assert all(untouched(b, 7.0) for b, _ in out) and int(nbt) == 3
        assert torch.equal(rm, d["running_mean"]) and torch.equal(rv, d["running_var"])


# ------------------------------------------------------------------------------------------------ tdx_bn_apply_relu_fwd
@pytest.mark.parametrize("rows,C", S.APPLY_CASES)
def test_bn_apply_relu_fwd_per_element(tdx, rows, C):
    """relu(y scale + shift), one fma per element: |got - ref| <= 2 u (|y scale| + |shift|).  One row of one quad, and
    rows C / 4 = 2 097 160 > 8192 workgroups x 256: the grid-stride loop's second trip."""
    d = S.bn_operands(rows, C, S.case_seed(C, rows), DEV)
    buf, out = guarded((rows, C), 7.0)
    assert call(tdx, "tdx_bn_apply_relu_fwd", d["y"], out, rows, C, d["scale"], d["shift"]) == 0
    ref, bound = S.bn_relu_fwd_ref(d["y"], d["scale"], d["shift"])
    r = S.elem_ratio(out, ref, bound)
    print("bn_apply", rows, C, round(r, 3))
    assert r <= 1.0 and guard_ok(buf, 7.0)


# ------------------------------------------------------------------------------------------------ tdx_bn_relu_bwd
def _bn_bwd_case(tdx, rows, C, training, big_mean=False):
    d = S.bn_operands(rows, C, S.case_seed(C, rows), DEV, big_mean)
    plan = S.bn_bwd_plan(rows, C)
    n_scr = tdx.lib.tdx_bn_relu_bwd_scratch_floats(rows, C)
    assert n_scr >= plan["nblk"] * 2 * C + 3 * C
    scr = torch.full((n_scr,), NAN, device=DEV)
    gbuf, g = guarded((rows, C), 7.0, d["g"])
    small = {k: guarded((C,), 7.0) for k in ("dgamma", "dbeta", "dbias")}
    rc = call(tdx, "tdx_bn_relu_bwd", g, d["y"], rows, C, d["scale"], d["shift"], d["mean"], d["rstd"], d["gamma"],
              small["dgamma"][1], small["dbeta"][1], small["dbias"][1], scr, training)
    assert rc == 0
    ref = S.bn_relu_bwd_ref(d["g"], d["y"], d["scale"], d["shift"], d["mean"], d["rstd"], d["gamma"], bool(training),
                            plan["K"])
    got = {"g": g, **{k: v[1] for k, v in small.items()}}
    ratios = {k: S.elem_ratio(got[k], *ref[k]) for k in ref}
    print("bn_relu_bwd", rows, C, training, plan["regime"], plan["rpb"], plan["nblk"],
          {k: round(v, 3) for k, v in ratios.items()})
    assert all(r <= 1.0 for r in ratios.values()), (rows, C, ratios)
    if training:
        assert torch.equal(small["dbias"][1], torch.zeros(C, device=DEV))
    assert guard_ok(gbuf, 7.0) and all(guard_ok(b, 7.0) for b, _ in small.values())


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("C", S.BN_BWD_WIDTHS)
def test_bn_relu_bwd_every_width_at_the_floor(tdx, C, training):
    """All nine widths of the contract (rgroups = 256 ... 1), rows = 1, rpb - 1, rpb, rpb + 1 at rpb = 2 rgroups: one
    block that is nearly empty, ragged, full, and a second block of one row.  Per element: g against
    9 u sqrt(K + 13) |gamma rstd| (|gz| + sum |gz| / N + |xhat| sum |gz xhat| / N), dgamma / dbeta per channel against
    9 u sqrt(K + 4 | K + 1) x their magnitude-sums, K = rpb / rgroups + rgroups the fp32 additions of the reduction
    (spatial_helpers.bn_relu_bwd_ref); dbias exactly 0 in train mode, per channel in eval mode."""
    for rows in S.bn_floor_rows(C):
        _bn_bwd_case(tdx, rows, C, training)


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("C,rows,regime,why", S.BN_BWD_OTHER, ids=[f"{c}x{r}" for c, r, _, _ in S.BN_BWD_OTHER])
def test_bn_relu_bwd_other_regimes_and_second_trips(tdx, C, rows, regime, why, training):
    """rows / 2048 regime (C = 1024 and 128), the 512 cap (C = 4), 300 block partials (the finalize kernel's loop over
    256 takes a second trip), and 4097 apply workgroups against the cap of 4096 (C = 8, one row past its floor regime).
    Same gates as at the floor, with K of the regime; C = 128 runs the |mean| / std ~ 100 data."""
    assert S.bn_bwd_plan(rows, C)["regime"] == regime
    _bn_bwd_case(tdx, rows, C, training, big_mean=(C == 128))


@pytest.mark.parametrize("C", [12, 6, 2048])
def test_bn_relu_bwd_refuses_illegal_widths(tdx, C):
    rows = 5
    assert tdx.lib.tdx_bn_relu_bwd_scratch_floats(rows, C) == 0
    g = torch.full((rows * C + GUARD,), 7.0, device=DEV)
    y, vec, scr = torch.zeros(rows * C, device=DEV), torch.ones(C, device=DEV), torch.zeros(4096 * 2 * C, device=DEV)
    outs = torch.full((3, C), 7.0, device=DEV)
    for training in (1, 0):
        rc = call(tdx, "tdx_bn_relu_bwd", g, y, rows, C, vec, vec, vec, vec, vec, outs[0], outs[1], outs[2], scr, training)
        assert rc == S.TDX_E_SHAPE and untouched(g, 7.0) and untouched(outs, 7.0)


# ------------------------------------------------------------------------------------------------ max-pool
def _pool_case(tdx, B, H, W, C, bn, with_skip, chunk=None):
    y, sc, sh, go, skip = S.maxpool_inputs(B, H, W, C, S.case_seed(H, W, C, bn), DEV, bn)
    if not with_skip:
        skip = None
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    obuf, out = guarded((B, Ho, Wo, C), 7.0)
    assert call(tdx, "tdx_maxpool2_ceil_fwd", y, sc, sh, out, B, H, W, C) == 0
    ibuf, gin = guarded((B, H, W, C), NAN)     # NaN: every input position has to be written
    assert call(tdx, "tdx_maxpool2_ceil_bwd", y, sc, sh, go, skip, gin, B, H, W, C) == 0
    for b0 in range(0, B, chunk or B):
        sl = slice(b0, b0 + (chunk or B))
        ref_out, ref_gin = S.maxpool_refs(y[sl], sc, sh, go[sl], None if skip is None else skip[sl])
        assert torch.equal(out[sl].double(), ref_out), (H, W, C, bn, b0)
        assert torch.equal(gin[sl].double(), ref_gin), (H, W, C, bn, with_skip, b0)
    assert guard_ok(obuf, 7.0) and guard_ok(ibuf, NAN)


@pytest.mark.parametrize("C", [4, 1024])
@pytest.mark.parametrize("H,W", S.POOL_SHAPES)
def test_maxpool_bit_for_bit_at_non_square_shapes(tdx, H, W, C):
    """Dyadic operands (spatial_helpers.maxpool_inputs: exact in fp32, ties and dead windows planted), so forward and
    backward equal the fp64 reference bit for bit and first-maximum routing is decided.  Odd and unit extents clip the
    last window to one row and / or column; scale given (BN+ReLU on load) and NULL (raw input, negative maxima);
    skip_grad given and NULL.  g_in starts as NaN: every input position must have been written."""
    for bn in (True, False):
        for with_skip in (True, False):
            _pool_case(tdx, 2, H, W, C, bn, with_skip)


@pytest.mark.parametrize("bn", [True, False])
def test_maxpool_above_the_grid_cap(tdx, bn):
    """B Ho Wo C / 4 = 1 048 800 > 4096 workgroups x 256: the grid-stride loops' second trip, 3 x 3 maps (every window
    kind: full, one column, one row, one element)."""
    B, H, W, C = S.POOL_BIG
    _pool_case(tdx, B, H, W, C, bn, bn, chunk=65550)


# ------------------------------------------------------------------------------------------------ bilinear resize
def _resize_fwd(tdx, d, shape, bn, add, sliced):
    Hi, Wi, Ho, Wo = shape
    B, C = d["y"].shape[0], d["y"].shape[3]
    cs, co = (3 * C, C + 4) if sliced else (C, 0)
    buf, out = guarded((B, Ho, Wo, cs), 7.0)
    sc, sh = (d["scale"], d["shift"]) if bn else (None, None)
    ad = d["addend"] if add else None
    assert call(tdx, "tdx_bilinear_ac_fwd", d["y"], sc, sh, ad, out, B, Hi, Wi, Ho, Wo, C, cs, co) == 0
    ref, bound = S.resize_fwd_ref(d["y"], sc, sh, ad, Ho, Wo)
    r = S.elem_ratio(out[..., co:co + C], ref, bound)
    assert untouched(out[..., :co], 7.0) and untouched(out[..., co + C:], 7.0) and guard_ok(buf, 7.0)
    return r, out[..., co:co + C], bound


def _resize_bwd(tdx, d, shape, sliced):
    Hi, Wi, Ho, Wo = shape
    B, C = d["y"].shape[0], d["y"].shape[3]
    cs, co = (3 * C, C + 4) if sliced else (C, 0)
    gbuf = torch.full((B, Ho, Wo, cs), NAN, device=DEV)    # NaN in the channels that are not the kernel's to read
    gbuf[..., co:co + C] = d["g"]
    buf, gin = guarded((B, Hi, Wi, C), 7.0)
    rc = call(tdx, "tdx_bilinear_ac_bwd", gbuf, gin, B, Hi, Wi, Ho, Wo, C, cs, co)
    assert guard_ok(buf, 7.0)
    return rc, gin


ALL_RESIZES = list(S.RESIZE_CASES) + [(hi, 3, ho, 5) for hi, ho in S.RESIZE_REJECTED_AXES] \
    + [(3, wi, 5, wo) for wi, wo in S.RESIZE_REJECTED_AXES]


@pytest.mark.parametrize("shape", ALL_RESIZES, ids=_id)
def test_bilinear_fwd_bwd_at_non_square_pairs(tdx, shape):
    """(Hi, Wi) -> (Ho, Wo) with Hi != Wi or Ho != Wo throughout, B = 3, C = 8; BN-on-load x addend x channel slice in
    four combinations that cover each operand present and NULL, slice (cstride 24, offset 12) and whole tensor.

    Forward, per element against R.bilinear_ac in fp64 (its coordinates are the kernel's fp32 ones): 9 u sqrt(K) x the
    same resize of the input's magnitude, K = 4 (product and sum along W, product and sum along H) + 1 with BN on load
    (the fma) + 1 with an addend.  Backward against the transpose of the exact-coordinate fp64 operator,
    g_in = Wh^T g Ww: 9 u sqrt(hn wn + 3) Wh^T |g| Ww + the coordinate term (|delta src| <= 2 u (n_in - 1) per axis on
    every weight a contributor touches; spatial_helpers.resize_adj_ref); an input no output reaches must be exactly 0.
    The branch the adjoint takes is the one tests/test_spatial_refs_host.py pins for the shape: row kernel with batched
    loads (wn <= 5), its loop (wn > 5), the generic kernel (Hi or Wi > 64) or TDX_E_SHAPE with g_in untouched - the
    forward covers those shapes all the same.  Adjoint identity of the two kernels on the raw operands, sums in fp64:
    |<g, fwd(y)> - <bwd(g), y>| <= sum |g| bound_fwd + sum |y| bound_bwd (rounding parts only: both kernels form their
    weights with the same arithmetic)."""
    Hi, Wi, Ho, Wo = shape
    d = S.resize_inputs(3, Hi, Wi, Ho, Wo, 8, S.case_seed(*shape), DEV)
    branch = S.adjoint_branch(*shape)
    assert branch == S.RESIZE_CASES.get(shape, "rejected")
    ratios = {}
    for bn, add, sliced in ((True, True, True), (False, False, False), (True, False, False), (False, True, True)):
        ratios[f"fwd{int(bn)}{int(add)}{int(sliced)}"], out, fbound = _resize_fwd(tdx, d, shape, bn, add, sliced)
        if not (bn or add):
            raw_out, raw_bound = out, fbound
    for sliced in (True, False):
        rc, gin = _resize_bwd(tdx, d, shape, sliced)
        if branch == "rejected":
            assert rc == S.TDX_E_SHAPE and untouched(gin, 7.0)
            continue
        assert rc == 0
        ref, bound, rounding = S.resize_adj_ref(d["g"], Hi, Wi)
        ratios[f"bwd{int(sliced)}"] = S.elem_ratio(gin, ref, bound)
        lhs = float((d["g"].double() * raw_out.double()).sum())
        rhs = float((gin.double() * d["y"].double()).sum())
        tol = float((d["g"].double().abs() * raw_bound).sum() + (d["y"].double().abs() * rounding).sum())
        ratios[f"adjoint{int(sliced)}"] = abs(lhs - rhs) / tol
    print("bilinear", shape, branch, {k: round(v, 3) for k, v in ratios.items()})
    assert all(r <= 1.0 for r in ratios.values()), (shape, branch, ratios)


def test_bilinear_fwd_above_the_grid_cap(tdx):
    """B Ho Wo C / 4 = 1 053 000 > 4096 workgroups x 256, BN on load and addend, (3, 5) -> (6, 9)."""
    B, Hi, Wi, Ho, Wo, C = S.RESIZE_FWD_BIG
    d = S.resize_inputs(B, Hi, Wi, Ho, Wo, C, S.case_seed(Hi, Wi, Ho, Wo), DEV)
    r, _, _ = _resize_fwd(tdx, d, (Hi, Wi, Ho, Wo), True, True, False)
    print("bilinear fwd big", round(r, 3))
    assert r <= 1.0


def test_bilinear_bwd_above_the_row_cap(tdx):
    """B Hi = 16500 rows > the row kernel's 16384 workgroups at C = 4 (one thread per column), (3, 2) -> (6, 5), the
    gradient a slice: the rows of the second trip against the same per-element bound."""
    B, Hi, Wi, Ho, Wo, C = S.RESIZE_BWD_BIG
    d = S.resize_inputs(B, Hi, Wi, Ho, Wo, C, S.case_seed(Hi, Wi, Ho, Wo), DEV)
    rc, gin = _resize_bwd(tdx, d, (Hi, Wi, Ho, Wo), True)
    assert rc == 0
    ref, bound, _ = S.resize_adj_ref(d["g"], Hi, Wi)
    r = S.elem_ratio(gin, ref, bound)
    print("bilinear bwd big", round(r, 3))
    assert r <= 1.0


@pytest.mark.parametrize("cs,co", [(26, 4), (24, 6), (8, 4), (12, 8)])
def test_bilinear_refuses_bad_channel_slices(tdx, cs, co):
    """cstride or offset no multiple of 4, or offset + C > cstride: TDX_E_SHAPE from both entries, nothing written."""
    B, Hi, Wi, Ho, Wo, C = 2, 3, 4, 5, 7, 8
    y = torch.zeros(B, Hi, Wi, C, device=DEV)
    big = torch.full((B * Ho * Wo * 32,), 7.0, device=DEV)
    assert call(tdx, "tdx_bilinear_ac_fwd", y, None, None, None, big, B, Hi, Wi, Ho, Wo, C, cs, co) == S.TDX_E_SHAPE
    assert untouched(big, 7.0)
    gin = torch.full((B, Hi, Wi, C), 7.0, device=DEV)
    assert call(tdx, "tdx_bilinear_ac_bwd", big, gin, B, Hi, Wi, Ho, Wo, C, cs, co) == S.TDX_E_SHAPE
    assert untouched(gin, 7.0)
