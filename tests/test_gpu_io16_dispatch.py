"""The bf16-storage (`io16`) instantiations of csrc/bn.hip, csrc/spatial.hip and csrc/edge_conv.hip and the kernels that
emit BatchNorm-backward partial sums, per element against fp64, one kernel at a time through the `_io` entries of
include/tdx.h.  The whole-network gates of tests/test_gpu_bf16.py stay where they are.

References, bounds, builders and the branch each case reaches: tests/io16_helpers.py, checked on the CPU by
tests/test_io16_refs_host.py.  Every reference is fp64 on the operands the kernel reads (bf16 widened exactly, fp32
parameters).  fp32 outputs: |got - ref| <= 9 u sqrt(K) x magnitude-sum, the bound of their fp32 tests.  bf16 outputs:
RNE_bf16(ref - b) <= got <= RNE_bf16(ref + b) with b that same fp32 bound, every element, none left out - bit for bit
wherever both ends round alike, and everywhere for the max-pool (dyadic operands).  Outputs start as NaN and have NaN
guard elements behind them; `partial` rows past *nblk must stay NaN.  `-s` prints the worst |error| / bound per case."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_helpers as CH  # noqa: E402
import io16_helpers as H  # noqa: E402
import spatial_helpers as S  # noqa: E402

DEV = "cuda"
GUARD = 64
NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def tdx():
    import tiny_diffusion_amd._lib as L

    assert torch.cuda.is_available()
    return L


def call(tdx, name, *args):
    """One C-ABI call on the current stream: tensors by address, None as NULL; synchronises.  Returns the status."""
    rc = getattr(tdx.lib, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args],
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def dt(io16):
    return BF16 if io16 else F32


def st(t, io16):
    """A tensor of bf16-representable fp32 values in the storage type of the call."""
    if t is None:
        return None
    assert H.is16(t)
    return t.to(BF16).contiguous() if io16 else t.contiguous()


def guarded(shape, dtype=F32, init=None):
    """(buffer, view): NaN-filled, GUARD more NaN elements behind the view."""
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), NAN, dtype=dtype, device=DEV)
    view = buf[:n].view(shape)
    if init is not None:
        view.copy_(init)
    return buf, view


def all_nan(t):
    return bool(torch.isnan(t).all())


def guard_ok(buf):
    return all_nan(buf[-GUARD:])


def held(got, ref, bound, io16):
    """-> (passes, figure): the interval check of a bf16 output / the per-element bound of an fp32 one."""
    if io16:
        assert got.dtype == BF16
        return H.outside16(got, ref, bound) == 0, H.ratio16(got, ref, bound)
    r = S.elem_ratio(got, ref, bound)
    return r <= 1.0, r


def _id(case):
    return "-".join(str(x) for x in case) if isinstance(case, (tuple, list)) else str(case)


# ------------------------------------------------------------------------------------------------ bn_relu_apply16_kernel
@pytest.mark.parametrize("rows,C", H.APPLY16_CASES + [H.APPLY16_BIG], ids=_id)
def test_bn_apply16_per_element(tdx, rows, C):
    """relu(y scale + shift) on bf16 tensors, eight channels per thread: C = 8 at 1 and 3 rows (one thread, three), C =
    1024 (128 threads per row), and rows C / 8 = 2 097 160 > 8192 x 256: the stride loop's second trip.  One fma and the
    store's rounding: the interval of 2 u (|y scale| + |shift|), exactly 0 where the ReLU is closed."""
    assert H.apply16_plan(rows, C)["trips"] == (2 if (rows, C) == H.APPLY16_BIG else 1)
    d = H.bn_operands16(rows, C, S.case_seed(C, rows), DEV)
    buf, out = guarded((rows, C), BF16)
    assert call(tdx, "tdx_bn_apply_relu_fwd_io", st(d["y"], 1), out, rows, C, d["scale"], d["shift"], 1) == 0
    ref, b = H.bn_apply_ref16(d["y"], d["scale"], d["shift"])
    ok, fig = held(out, ref, b, 1)
    print("bn_apply16", rows, C, round(fig, 3))
    assert ok and guard_ok(buf)


def test_bn_apply_width_12_is_refused_in_bf16_and_computed_in_fp32(tdx):
    rows, C = 3, 12
    d = H.bn_operands16(rows, C, 5, DEV)
    buf, out = guarded((rows, C), BF16)
    assert call(tdx, "tdx_bn_apply_relu_fwd_io", st(d["y"], 1), out, rows, C, d["scale"], d["shift"], 1) == H.TDX_E_SHAPE
    assert all_nan(buf)
    buf, out = guarded((rows, C), F32)
    assert call(tdx, "tdx_bn_apply_relu_fwd_io", d["y"], out, rows, C, d["scale"], d["shift"], 0) == 0
    ref, b = H.bn_apply_ref16(d["y"], d["scale"], d["shift"])
    assert held(out, ref, b, 0)[0] and guard_ok(buf)
    twin = torch.empty_like(out)
    assert call(tdx, "tdx_bn_apply_relu_fwd", d["y"], twin, rows, C, d["scale"], d["shift"]) == 0
    assert torch.equal(out, twin)


# ------------------------------------------------------------------------------------------------ tdx_bn_relu_bwd_io
def _bn_bwd16(tdx, rows, C, training, big_mean=False):
    d = H.bn_operands16(rows, C, S.case_seed(C, rows), DEV, big_mean)
    plan = S.bn_bwd_plan(rows, C)
    scr = torch.full((tdx.lib.tdx_bn_relu_bwd_scratch_floats(rows, C),), NAN, device=DEV)
    gbuf, g = guarded((rows, C), BF16, d["g"])
    small = {k: guarded((C,)) for k in ("dgamma", "dbeta", "dbias")}
    rc = call(tdx, "tdx_bn_relu_bwd_io", g, st(d["y"], 1), rows, C, d["scale"], d["shift"], d["mean"], d["rstd"],
              d["gamma"], small["dgamma"][1], small["dbeta"][1], small["dbias"][1], scr, training, 1)
    assert rc == 0
    ref = S.bn_relu_bwd_ref(d["g"], d["y"], d["scale"], d["shift"], d["mean"], d["rstd"], d["gamma"], bool(training),
                            plan["K"])
    ok, fig = held(g, *ref["g"], 1)
    ratios = {k: S.elem_ratio(small[k][1], *ref[k]) for k in ("dgamma", "dbeta", "dbias")}
    print("bn_relu_bwd_io", rows, C, training, plan["nblk"], "g", round(fig, 3), {k: round(v, 3) for k, v in ratios.items()})
    assert ok, (rows, C, training, H.outside16(g, *ref["g"]))
    assert all(r <= 1.0 for r in ratios.values()), ratios
    assert guard_ok(gbuf) and all(guard_ok(b) for b, _ in small.values())


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("C", H.BN_WIDTHS)
def test_bn_relu_bwd_bf16_two_blocks(tdx, C, training):
    """bn_bwd_reduce_kernel<bf16> and bn_bwd_apply_kernel<bf16> at rows = rpb + 1 (two blocks, the second of one row):
    rgroups = 256, 16 and 1.  The reduction reads the stored bf16 gradient: dgamma / dbeta / dbias (fp32) at the bound of
    the fp32 test, K = rpb / rgroups + rgroups; g' by the interval of the K + 13 bound (train) or of one product (eval)."""
    _bn_bwd16(tdx, H.bn_two_block_rows(C), C, training)


def test_bn_relu_bwd_bf16_apply_pass_second_trip(tdx):
    """rows C / 4 = 1 048 578 > 4096 workgroups x 256 at C = 8: the apply pass's stride loop takes a second trip."""
    C, rows = H.BN_APPLY_BIG
    assert H.bwd_apply_trips(rows, C) == 2
    _bn_bwd16(tdx, rows, C, 1)


# ------------------------------------------------------------------------------------------------ from partials
@pytest.mark.parametrize("io16", [1, 0])
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("nblk", H.FROM_PARTIALS_NBLK)
def test_bn_relu_bwd_from_partials(tdx, nblk, training, io16):
    """Finalize + apply from GIVEN operands: g, y and a host-made partial [nblk][2][C]; the reference sums are the fp64
    sums of those fp32 partials.  nblk = 1, 255, 256 (one trip of the 256-wide block loop, the last thread idle / busy),
    257 (a second trip of one thread) and 2048 (eight trips: the largest a producer writes).  NaN behind the last block:
    a loop one too long poisons every sum."""
    rows, C = H.FROM_PARTIALS_SHAPE
    d = H.bn_operands16(rows, C, S.case_seed(C, rows, nblk), DEV)
    pbuf, part = guarded((nblk, 2, C), F32, H.host_partials(d, nblk, nblk))
    cbuf, coef = guarded((3 * C,))
    gbuf, g = guarded((rows, C), dt(io16), d["g"])
    small = {k: guarded((C,)) for k in ("dgamma", "dbeta", "dbias")}
    rc = call(tdx, "tdx_bn_relu_bwd_from_partials", g, st(d["y"], io16), rows, C, d["scale"], d["shift"], d["mean"],
              d["rstd"], d["gamma"], small["dgamma"][1], small["dbeta"][1], small["dbias"][1], part, nblk, coef, training,
              io16)
    assert rc == 0
    ref = H.bn_from_partials_ref(d["g"], d["y"], part, d["scale"], d["shift"], d["mean"], d["rstd"], d["gamma"],
                                 bool(training))
    ok, fig = held(g, *ref["g"], io16)
    ratios = {k: S.elem_ratio(small[k][1], *ref[k]) for k in ("dgamma", "dbeta", "dbias")}
    print("from_partials", nblk, training, io16, "g", round(fig, 3), {k: round(v, 3) for k, v in ratios.items()})
    assert ok and all(r <= 1.0 for r in ratios.values()), (fig, ratios)
    assert guard_ok(gbuf) and guard_ok(cbuf) and guard_ok(pbuf) and all(guard_ok(b) for b, _ in small.values())


# ------------------------------------------------------------------------------------------------ max-pool, bf16
@pytest.mark.parametrize("C", [4, 1024])
@pytest.mark.parametrize("Hh,W", H.POOL_SHAPES, ids=_id)
def test_maxpool_bf16_bit_for_bit(tdx, Hh, W, C):
    """maxpool_fwd_kernel<*, bf16> and maxpool_bwd_kernel<*, false, bf16> on dyadic operands (exact in bf16, asserted):
    forward and backward equal the fp64 reference bit for bit, first-maximum routing included; BN given / NULL, skip
    given / NULL; odd and unit extents."""
    B = 2
    for bn in (True, False):
        y, sc, sh, go, skip = H.pool_inputs16(B, Hh, W, C, S.case_seed(Hh, W, C, bn), DEV, bn)
        for with_skip in (True, False):
            sk = skip if with_skip else None
            obuf, out = guarded((B, (Hh + 1) // 2, (W + 1) // 2, C), BF16)
            assert call(tdx, "tdx_maxpool2_ceil_fwd_io", st(y, 1), sc, sh, out, B, Hh, W, C, 1) == 0
            ibuf, gin = guarded((B, Hh, W, C), BF16)
            assert call(tdx, "tdx_maxpool2_ceil_bwd_io", st(y, 1), sc, sh, st(go, 1), st(sk, 1), gin, B, Hh, W, C,
                        None, None, None, None, 1) == 0
            ref_out, ref_gin = S.maxpool_refs(y, sc, sh, go, sk)
            assert torch.equal(out.double(), ref_out), (Hh, W, C, bn)
            assert torch.equal(gin.double(), ref_gin), (Hh, W, C, bn, with_skip)
            assert guard_ok(obuf) and guard_ok(ibuf)


# ------------------------------------------------------------------------------------------------ max-pool producer
def _pool_producer(tdx, B, Hh, W, C, io16, with_skip=True, chunk=None):
    y, sc, sh, go, skip = H.pool_inputs16(B, Hh, W, C, S.case_seed(Hh, W, C, True), DEV, True)
    sk = skip if with_skip else None
    mean, rstd = H.pool_bn_stats(C, C + Hh, DEV)
    plan = H.pool_producer_plan(B, Hh, W, C)
    assert plan["branch"] == "producer"
    pbuf, part = guarded((H.PRODUCER_CAP, 2, C))
    ibuf, gin = guarded((B, Hh, W, C), dt(io16))
    nb = ctypes.c_int(-1)
    rc = call(tdx, "tdx_maxpool2_ceil_bwd_io", st(y, io16), sc, sh, st(go, io16), st(sk, io16), gin, B, Hh, W, C, mean,
              rstd, part, ctypes.byref(nb), io16)
    assert rc == 0 and nb.value == plan["nblk"], (rc, nb.value, plan)
    assert not bool(torch.isnan(part[:nb.value]).any()) and all_nan(part[nb.value:]) and guard_ok(pbuf) and guard_ok(ibuf)
    s1 = s2 = b1 = b2 = 0
    for b0 in range(0, B, chunk or B):
        sl = slice(b0, b0 + (chunk or B))
        _, ref_gin = S.maxpool_refs(y[sl], sc, sh, go[sl], None if sk is None else sk[sl])
        assert torch.equal(gin[sl].double(), ref_gin), (Hh, W, C, io16, b0)
        r = H.partial_sums_ref(ref_gin, 0.0, y[sl], sc, sh, mean, rstd, plan["K"])
        s1, b1, s2, b2 = s1 + r["s1"][0], b1 + r["s1"][1], s2 + r["s2"][0], b2 + r["s2"][1]
    g1, g2 = H.partial_totals(part, nb.value)
    r1, r2 = S.elem_ratio(g1, s1, b1), S.elem_ratio(g2, s2, b2)
    print("pool producer", (B, Hh, W, C), "io16", io16, "nblk", nb.value, "trips", plan["trips"], round(r1, 3), round(r2, 3))
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)


@pytest.mark.parametrize("io16", [1, 0])
@pytest.mark.parametrize("C", H.POOL_PRODUCER_WIDTHS)
def test_maxpool_producer_sums_and_gradient(tdx, C, io16):
    """maxpool_bwd_kernel<true, true, T>: g_in bit for bit (skip gradient included), and per channel the sum over the
    *nblk blocks of `partial` (added in fp64) against the fp64 sums of gz and gz xhat over the gradient it wrote: K = 4
    positions per trip + rgroups (+ 3 for the second sum).  C = 4, 64, 1024 (rgroups 256, 16, 1), odd maps; rows of
    `partial` past *nblk stay NaN."""
    for Hh, W in H.POOL_SHAPES:
        _pool_producer(tdx, 2, Hh, W, C, io16, with_skip=(Hh + W) % 2 == 0 or C == 64)


@pytest.mark.parametrize("io16", [1, 0])
def test_maxpool_producer_second_trip_carries_the_sums(tdx, io16):
    """B Ho Wo C / 4 = 1 048 400 > 2048 workgroups x 256 at C = 4, 3 x 3 maps: all but the last 176 threads take a
    second trip of the grid-stride loop and their registers carry the sums across it."""
    B, Hh, W, C = H.POOL_PRODUCER_BIG
    assert H.pool_producer_plan(B, Hh, W, C)["trips"] == 2
    _pool_producer(tdx, B, Hh, W, C, io16, chunk=65550)


@pytest.mark.parametrize("io16", [1, 0])
@pytest.mark.parametrize("why", ["knob bit 2 off", "width", "scale == NULL"])
def test_maxpool_producer_fallbacks(tdx, why, io16):
    """Knob bit 2 off, C = 12, scale == NULL: *nblk == 0, `partial` untouched, g_in bit-identical to the plain entry."""
    B, Hh, W = 2, 5, 4
    C = 12 if why == "width" else 64
    bn = why != "scale == NULL"
    assert H.pool_producer_plan(B, Hh, W, C, knob=2 if why == "knob bit 2 off" else 6, scale_given=bn)["why"] == why
    gen = torch.Generator(device=DEV).manual_seed(3)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, device=DEV, generator=gen).float() / 8.0   # noqa: E731
    y, go, skip = ri(-2, 3, B, Hh, W, C), ri(-8, 9, B, 3, 2, C), ri(-8, 9, B, Hh, W, C)
    sc = torch.tensor(S.POOL_SCALES, device=DEV)[torch.arange(C, device=DEV) % 4] if bn else None
    sh = torch.tensor(S.POOL_SHIFTS, device=DEV)[torch.arange(C, device=DEV) % 4] if bn else None
    mean, rstd = H.pool_bn_stats(C, 1, DEV)
    pbuf, part = guarded((H.PRODUCER_CAP, 2, C))
    ibuf, gin = guarded((B, Hh, W, C), dt(io16))
    nb = ctypes.c_int(-1)
    args = (st(y, io16), sc, sh, st(go, io16), st(skip, io16))
    with tdx.tuned(bnbwd_fused=2 if why == "knob bit 2 off" else 6):
        rc = call(tdx, "tdx_maxpool2_ceil_bwd_io", *args, gin, B, Hh, W, C, mean, rstd, part, ctypes.byref(nb), io16)
    assert rc == 0 and nb.value == 0 and all_nan(pbuf) and guard_ok(ibuf)
    twin = torch.full((B, Hh, W, C), NAN, dtype=dt(io16), device=DEV)
    if io16:
        assert call(tdx, "tdx_maxpool2_ceil_bwd_io", *args, twin, B, Hh, W, C, None, None, None, None, 1) == 0
    else:
        assert call(tdx, "tdx_maxpool2_ceil_bwd", *args, twin, B, Hh, W, C) == 0
    assert torch.equal(gin, twin)
    _, ref_gin = S.maxpool_refs(y, sc, sh, go, skip)
    assert torch.equal(gin.double(), ref_gin)


# ------------------------------------------------------------------------------------------------ resize forward, bf16
@pytest.mark.parametrize("shape", H.RESIZE_FWD_PAIRS, ids=_id)
def test_bilinear_fwd_bf16(tdx, shape):
    """bilinear_fwd_kernel<*, bf16>: BN-on-load x addend in the four combinations, two of them into a channel slice
    (cstride 24 > C = 8, offset 12) whose other channels must stay NaN.  K = 4 + 1 (BN) + 1 (addend)."""
    Hi, Wi, Ho, Wo = shape
    B, C = 3, 8
    d = H.resize_inputs16(B, Hi, Wi, Ho, Wo, C, S.case_seed(*shape), DEV)
    figs = {}
    for bn, add, sliced in ((True, True, True), (False, False, False), (True, False, False), (False, True, True)):
        cs, co = (3 * C, C + 4) if sliced else (C, 0)
        buf, out = guarded((B, Ho, Wo, cs), BF16)
        sc, sh = (d["scale"], d["shift"]) if bn else (None, None)
        ad = d["addend"] if add else None
        assert call(tdx, "tdx_bilinear_ac_fwd_io", st(d["y"], 1), sc, sh, ad, out, B, Hi, Wi, Ho, Wo, C, cs, co, 1) == 0
        ref, b = S.resize_fwd_ref(d["y"], sc, sh, ad, Ho, Wo)
        ok, figs[f"{int(bn)}{int(add)}{int(sliced)}"] = held(out[..., co:co + C], ref, b, 1)
        assert ok, (shape, bn, add, sliced, H.outside16(out[..., co:co + C], ref, b))
        assert all_nan(out[..., :co]) and all_nan(out[..., co + C:]) and guard_ok(buf)
    print("bilinear fwd bf16", shape, {k: round(v, 3) for k, v in figs.items()})


# ------------------------------------------------------------------------------------------------ resize adjoint, bf16
def _adjoint(tdx, d, shape, io16, sliced, bn=None, knob=6):
    """-> (status, g_in, *nblk, partial, buffers).  bn: the producer operands (bn_y) or None for partial == NULL."""
    Hi, Wi, Ho, Wo = shape
    B, C = d["g"].shape[0], d["g"].shape[3]
    cs, co = (3 * C, C + 4) if sliced else (C, 0)
    gout = torch.full((B, Ho, Wo, cs), NAN, dtype=dt(io16), device=DEV)    # NaN in the channels that are not to be read
    gout[..., co:co + C] = d["g"]
    buf, gin = guarded((B, Hi, Wi, C), dt(io16))
    nb = ctypes.c_int(-1)
    if bn is None:
        rc = call(tdx, "tdx_bilinear_ac_bwd_io", gout, gin, B, Hi, Wi, Ho, Wo, C, cs, co, None, None, None, None, None,
                  None, ctypes.byref(nb), io16)
        return rc, gin, nb.value, None, (buf,)
    pbuf, part = guarded((H.PRODUCER_CAP, 2, C))
    with tdx.tuned(bnbwd_fused=knob):
        rc = call(tdx, "tdx_bilinear_ac_bwd_io", gout, gin, B, Hi, Wi, Ho, Wo, C, cs, co, st(bn, io16), d["scale"],
                  d["shift"], d["mean"], d["rstd"], part, ctypes.byref(nb), io16)
    return rc, gin, nb.value, part, (buf, pbuf)


@pytest.mark.parametrize("shape", list(H.RESIZE_BWD_CASES), ids=_id)
def test_bilinear_adjoint_bf16(tdx, shape):
    """bilinear_bwd_rows_kernel<false, bf16> with batched loads ((4,7)->(8,8); (3,2)->(7,6): wn = 5 exactly) and in its
    loop ((2,3)->(7,8): wn = 6), bilinear_bwd_kernel<bf16> ((65,3)->(66,6)), the gradient whole and as a channel slice:
    the interval of 9 u sqrt(hn wn + 3) Wh^T |g| Ww + the coordinate term, an input no output reaches exactly 0."""
    Hi, Wi, Ho, Wo = shape
    assert S.adjoint_branch(*shape) == H.RESIZE_BWD_CASES[shape]
    d = H.resize_inputs16(3, Hi, Wi, Ho, Wo, 8, S.case_seed(*shape), DEV)
    ref, bound, _ = S.resize_adj_ref(d["g"], Hi, Wi)
    for sliced in (False, True):
        rc, gin, nb, _, bufs = _adjoint(tdx, d, shape, 1, sliced)
        assert rc == 0 and nb == 0 and guard_ok(bufs[0])
        ok, fig = held(gin, ref, bound, 1)
        print("bilinear adjoint bf16", shape, H.RESIZE_BWD_CASES[shape], "sliced", sliced, round(fig, 3))
        assert ok, (shape, sliced, H.outside16(gin, ref, bound))


def test_bilinear_adjoint_io_refusals(tdx):
    """The refusals of tdx_bilinear_ac_bwd hold in bf16 and in the producer form: a contributor window past 8, a bad
    channel slice; g_in and `partial` untouched."""
    d = H.resize_inputs16(2, 7, 4, 8, 16, 8, 1, DEV)
    bn_y = H.r16(torch.randn(2, 7, 4, 8, device=DEV))
    for bn in (None, bn_y):
        rc, gin, nb, part, bufs = _adjoint(tdx, d, (7, 4, 8, 16), 1, False, bn)
        assert rc == H.TDX_E_SHAPE and all(all_nan(b) for b in bufs)
    B, Hi, Wi, Ho, Wo, C = 2, 3, 4, 5, 7, 8
    gin = torch.full((B, Hi, Wi, C), NAN, dtype=BF16, device=DEV)
    big = torch.zeros(B * Ho * Wo * 32, dtype=BF16, device=DEV)
    for cs, co in ((26, 4), (24, 6), (8, 4), (12, 8)):
        assert call(tdx, "tdx_bilinear_ac_bwd_io", big, gin, B, Hi, Wi, Ho, Wo, C, cs, co, None, None, None, None, None,
                    None, None, 1) == H.TDX_E_SHAPE
        assert call(tdx, "tdx_bilinear_ac_fwd_io", gin, None, None, None, big, B, Hi, Wi, Ho, Wo, C, cs, co,
                    1) == H.TDX_E_SHAPE
    assert all_nan(gin) and bool((big == 0).all())


# ------------------------------------------------------------------------------------------------ resize producer
def _resize_producer(tdx, B, shape, C, io16, sliced=False):
    Hi, Wi, Ho, Wo = shape
    d = H.resize_inputs16(B, Hi, Wi, Ho, Wo, C, S.case_seed(*shape, C), DEV)
    gen = torch.Generator(device=DEV).manual_seed(C + Hi)
    bn_y = S.nudge_relu(torch.randn(B, Hi, Wi, C, device=DEV, generator=gen), d["scale"], d["shift"], bf16=True)
    plan = H.resize_producer_plan(B, Hi, Wi, Ho, Wo, C)
    assert plan["branch"].startswith("producer:")
    rc, gin, nb, part, bufs = _adjoint(tdx, d, shape, io16, sliced, bn_y)
    assert rc == 0 and nb == plan["nblk"], (rc, nb, plan)
    assert not bool(torch.isnan(part[:nb]).any()) and all_nan(part[nb:]) and all(guard_ok(b) for b in bufs)
    ref, bound, _ = S.resize_adj_ref(d["g"], Hi, Wi)
    ok, fig = held(gin, ref, bound, io16)
    sums = H.partial_sums_ref(ref, bound, bn_y, d["scale"], d["shift"], d["mean"], d["rstd"], plan["K"])
    g1, g2 = H.partial_totals(part, nb)
    r1, r2 = S.elem_ratio(g1, *sums["s1"]), S.elem_ratio(g2, *sums["s2"])
    print("resize producer", B, shape, C, "io16", io16, plan["branch"], "nblk", nb, "g", round(fig, 3), round(r1, 3),
          round(r2, 3))
    assert ok and r1 <= 1.0 and r2 <= 1.0, (fig, r1, r2)
    return d, gin


@pytest.mark.parametrize("io16", [1, 0])
@pytest.mark.parametrize("C", [4, 64, 1024])
@pytest.mark.parametrize("shape", H.RESIZE_PRODUCER_SHAPES, ids=_id)
def test_bilinear_producer_sums_and_gradient(tdx, shape, C, io16):
    """bilinear_bwd_rows_kernel<true, T> in both row branches (batched loads, loop) at C = 4, 64, 1024: g_in at the
    adjoint's bound / interval, and the sums of `partial` over its *nblk = B Hi blocks against the fp64 sums of the
    reference gradient: K = elements a thread adds + rgroups (+ 3), plus the gradient's own per-element bound carried
    into the sums (they are formed from the fp32 accumulator, before the store rounds it)."""
    _resize_producer(tdx, 3, shape, C, io16, sliced=(C == 64))


@pytest.mark.parametrize("io16", [1, 0])
def test_bilinear_producer_workgroup_owns_several_rows(tdx, io16):
    """B Hi = 3000 > 2048 workgroups: 952 workgroups walk two rows and carry their sums from one to the next."""
    B, Hi, Wi, Ho, Wo, C = H.RESIZE_PRODUCER_MANY_ROWS
    assert H.resize_producer_plan(B, Hi, Wi, Ho, Wo, C)["rows_per_wg"] == 2
    _resize_producer(tdx, B, (Hi, Wi, Ho, Wo), C, io16)


@pytest.mark.parametrize("io16", [1, 0])
@pytest.mark.parametrize("why", ["knob bit 1 off", "Hi or Wi > 64", "width"])
def test_bilinear_producer_fallbacks(tdx, why, io16):
    """Knob bit 1 off, Hi = 65, C = 12: *nblk == 0, `partial` untouched, g_in bit-identical to the plain entry."""
    shape = (65, 3, 66, 6) if why == "Hi or Wi > 64" else (4, 7, 8, 8)
    C = 12 if why == "width" else 8
    knob = 4 if why == "knob bit 1 off" else 6
    assert H.resize_producer_plan(2, *shape, C, knob=knob)["why"] == why
    d = H.resize_inputs16(2, *shape, C, 9, DEV)
    bn_y = H.r16(torch.randn(2, shape[0], shape[1], C, device=DEV))
    rc, gin, nb, part, bufs = _adjoint(tdx, d, shape, io16, False, bn_y, knob)
    assert rc == 0 and nb == 0 and all_nan(bufs[1]) and guard_ok(bufs[0])
    rc, twin, _, _, _ = _adjoint(tdx, d, shape, io16, False)
    assert rc == 0 and torch.equal(gin, twin)
    if not io16:
        fp32 = torch.full_like(twin, NAN)
        assert call(tdx, "tdx_bilinear_ac_bwd", d["g"], fp32, 2, *shape, C, C, 0) == 0
        assert torch.equal(gin, fp32)


@pytest.mark.parametrize("shape", H.RESIZE_PRODUCER_SHAPES, ids=_id)
def test_bilinear_producer_adjoint_identity(tdx, shape):
    """<g, fwd(y)> = <bwd(g), y> between the producer form of the adjoint and the forward at io16 = 0, sums in fp64,
    within sum |g| bound_fwd + sum |y| bound_bwd (rounding parts: both kernels form their weights alike)."""
    Hi, Wi, Ho, Wo = shape
    B, C = 3, 64
    d, gin = _resize_producer(tdx, B, shape, C, 0)
    buf, out = guarded((B, Ho, Wo, C))
    assert call(tdx, "tdx_bilinear_ac_fwd_io", d["y"], None, None, None, out, B, Hi, Wi, Ho, Wo, C, C, 0, 0) == 0
    _, fbound = S.resize_fwd_ref(d["y"], None, None, None, Ho, Wo)
    _, _, rounding = S.resize_adj_ref(d["g"], Hi, Wi)
    lhs = float((d["g"].double() * out.double()).sum())
    rhs = float((gin.double() * d["y"].double()).sum())
    tol = float((d["g"].double().abs() * fbound).sum() + (d["y"].double().abs() * rounding).sum())
    print("adjoint identity", shape, abs(lhs - rhs) / tol)
    assert abs(lhs - rhs) <= tol and guard_ok(buf)


# ------------------------------------------------------------------------------------------------ pair kernel
@pytest.mark.parametrize("io16", [1, 0])
@pytest.mark.parametrize("case", H.PAIR_CASES, ids=_id)
def test_bilinear_pair_fwd(tdx, case, io16):
    """bilinear_pair_fwd_kernel<T>: (Ca, Cb) = (64, 64), (4, 128), (64, 0), the two sources of different sizes, the
    addend given / NULL; source A plain and as a deferred split-K result of 1, 2 and 3 fp32 slabs (64 NaN floats between
    slabs) with the bias given / NULL.  Per element at K = 4 (+ 1 addend; + splits + 1 deferred); at io16 = 0 the plain
    form equals two tdx_bilinear_ac_fwd calls bit for bit."""
    Ca, Cb, (Ha, Wa), (Hb, Wb), (Ho, Wo) = case
    B = 3
    gen = torch.Generator(device=DEV).manual_seed(S.case_seed(Ca, Cb, Ha, Wa))
    a = H.r16(torch.randn(B, Ha, Wa, Ca, device=DEV, generator=gen))
    b_ = H.r16(torch.randn(B, Hb, Wb, Cb, device=DEV, generator=gen)) if Cb else None
    addend = torch.randn(B, Cb, device=DEV, generator=gen) if Cb else None
    figs = {}

    def run(tag, a_t, df, ad):
        buf, out = guarded((B, Ho, Wo, Ca + Cb), dt(io16))
        dfa = (None, 0, 0, None, None, None) if df is None else (df["buf"], len(df["parts"]), df["slab"], df["bias"],
                                                                   df["scale"], df["shift"])
        rc = call(tdx, "tdx_bilinear_pair_fwd_io", st(a_t, io16), *dfa, Ha, Wa, Ca, st(b_, io16), ad, Hb, Wb, Cb, out, B,
                  Ho, Wo, io16)
        assert rc == 0 and guard_ok(buf)
        ref, bound = H.pair_ref(a_t, df, b_, ad, Ho, Wo)
        ok, figs[tag] = held(out, ref, bound, io16)
        assert ok, (case, tag, io16, figs[tag])
        return out

    for ad in ((addend, None) if Cb else (None,)):
        out = run("plain" + ("+add" if ad is not None else ""), a, None, ad)
        if not io16:
            twin = torch.full_like(out, NAN)
            assert call(tdx, "tdx_bilinear_ac_fwd", a, None, None, None, twin, B, Ha, Wa, Ho, Wo, Ca, Ca + Cb, 0) == 0
            if Cb:
                assert call(tdx, "tdx_bilinear_ac_fwd", b_, None, None, ad, twin, B, Hb, Wb, Ho, Wo, Cb, Ca + Cb, Ca) == 0
            assert torch.equal(out, twin)
    for splits in (1, 2, 3):
        for with_bias in (True, False):
            df = H.defer_operands(B, Ha, Wa, Ca, splits, 7 + splits, DEV, with_bias)
            run(f"defer{splits}{'b' if with_bias else ''}", None, df, addend)
    print("pair", case, "io16", io16, {k: round(v, 3) for k, v in figs.items()})


# ------------------------------------------------------------------------------------------------ pixel sum
@pytest.mark.parametrize("io16", [1, 0])
@pytest.mark.parametrize("C", H.PIXEL_WIDTHS)
def test_pixel_sum(tdx, C, io16):
    """pixel_sum_kernel<T>: out[b][c] = sum over HW pixels, HW = 1, rgroups - 1, rgroups + 1 and 784 (threads without a
    pixel, one pixel each, a second pixel for the first thread, 28 x 28), C = 4, 64, 1024; K = ceil(HW / rgroups) +
    rgroups."""
    B = 3
    for HW in H.pixel_sum_hw(C):
        g = H.r16(torch.randn(B, HW, C, device=DEV, generator=torch.Generator(device=DEV).manual_seed(HW + C)))
        buf, out = guarded((B, C))
        assert call(tdx, "tdx_pixel_sum_io", st(g, io16), out, B, HW, C, io16) == 0
        ref, b = H.pixel_sum_ref(g, C)
        r = S.elem_ratio(out, ref, b)
        print("pixel_sum", C, HW, "io16", io16, round(r, 3))
        assert r <= 1.0 and guard_ok(buf)


def test_pixel_sum_refusals(tdx):
    g = torch.zeros(4096, device=DEV)
    buf, out = guarded((2, 2048))
    for C in H.PIXEL_REFUSED:
        for io16 in (0, 1):
            assert call(tdx, "tdx_pixel_sum_io", g, out, 2, 1, C, io16) == H.TDX_E_SHAPE
    for bad in ((None, out, 2, 1, 4), (g, None, 2, 1, 4), (g, out, 0, 1, 4), (g, out, 2, 0, 4), (g, out, 2, 1, 0)):
        assert call(tdx, "tdx_pixel_sum_io", *bad, 1) == H.TDX_E_BADARG
    assert all_nan(buf)


# ------------------------------------------------------------------------------------------------ boundary convolutions
def _edge_fp32(fails, tag, got, refs):
    ref, mag, K = refs[tag]
    e, r = CH.rel_err(got, ref), CH.elem_ratio(got, ref, mag, K)
    print(f"  {tag}: rel {e:.2e} (gate {H.EDGE_REL[tag]:.0e})  elem {r:.3f} (gate {CH.ELEM_DIRECT:g})")
    if not (e < H.EDGE_REL[tag] and r <= CH.ELEM_DIRECT):
        fails.append((tag, e, r))


def _edge_bf16(fails, tag, got, refs):
    ref, mag, K = refs[tag]
    b = H.edge_bound(mag, K)
    n = H.outside16(got, ref, b)
    print(f"  {tag}: {n} outside, worst {H.ratio16(got, ref, b):.3f}")
    if n:
        fails.append((tag, n))


@pytest.mark.parametrize("ct,cf", CH.EDGE_PAIRS)
@pytest.mark.parametrize("shape", CH.EDGE_SMALL, ids=_id)
def test_edge_conv_bf16_fat_tensor(tdx, shape, ct, cf):
    """All five boundary-convolution entries with the fat channels-last tensor in bf16: the fat OUTPUTS (initial_conv's
    activation, final_conv's input gradient) by the interval of the fp32 per-element bound; the thin outputs and dw / db
    (fp32) at the gates of tests/test_gpu_conv_nonsquare.py, from the bf16 operands widened exactly."""
    B, Hh, W = shape
    e = H.edge_operands16(B, Hh, W, ct, cf, 700 + Hh * W + ct)
    refs = H.edge_refs(e)
    G, fails = CH.Guards(), []
    g_fat16, fat16 = e.g_fat.to(BF16), e.fat.to(BF16)
    print(f"\nedge bf16 {ct}->{cf} {B}x{Hh}x{W}")
    out = G.new((B, Hh, W, 64), BF16)
    assert call(tdx, "tdx_initial_conv_forward_io", e.x, e.w_init, e.b_init, out, B, Hh, W, ct, cf, 1) == 0
    _edge_bf16(fails, "init_fwd", out[..., :cf], refs)
    assert cf == 64 or bool((out[..., cf:] == 0).all()), "padding channels are not zero"
    scratch = G.new((tdx.lib.tdx_edge_conv_wgrad_scratch_floats(B, Hh, W),))
    dw, db = G.new((cf, ct, 3, 3)), G.new((cf,))
    assert call(tdx, "tdx_initial_conv_backward_io", e.x, g_fat16, dw, db, scratch, B, Hh, W, ct, cf, 1) == 0
    _edge_fp32(fails, "init_dw", dw, refs)
    _edge_fp32(fails, "init_db", db, refs)
    gx = G.new((B, ct, Hh, W))
    assert call(tdx, "tdx_initial_conv_input_grad_io", g_fat16, e.w_init, gx, B, Hh, W, ct, cf, 1) == 0
    _edge_fp32(fails, "init_gx", gx, refs)
    thin = G.new((B, ct, Hh, W))
    assert call(tdx, "tdx_final_conv_forward_io", fat16, e.w_fin, e.b_fin, thin, B, Hh, W, ct, 1) == 0
    _edge_fp32(fails, "fin_fwd", thin, refs)
    scratch2 = G.new((tdx.lib.tdx_edge_conv_wgrad_scratch_floats(B, Hh, W),))
    gin, dw2, db2 = G.new((B, Hh, W, 64), BF16), G.new((ct, 64, 3, 3)), G.new((ct,))
    assert call(tdx, "tdx_final_conv_backward_io", fat16, e.g_thin, e.w_fin, gin, dw2, db2, scratch2, B, Hh, W, ct, 1) == 0
    _edge_bf16(fails, "fin_gin", gin, refs)
    _edge_fp32(fails, "fin_dw", dw2, refs)
    _edge_fp32(fails, "fin_db", db2, refs)
    assert G.intact(), "guard region written"
    assert not fails, fails


@pytest.mark.parametrize("ct,cf", CH.EDGE_PAIRS)
def test_edge_conv_bf16_w3_refusals(tdx, ct, cf):
    """W < 4 with io16: both backward entries return TDX_E_SHAPE and write nothing, g_in included."""
    B, Hh, W = 2, 5, 3
    e = H.edge_operands16(B, Hh, W, ct, cf, 11)
    G = CH.Guards()
    scratch = G.new((tdx.lib.tdx_edge_conv_wgrad_scratch_floats(B, Hh, W),))
    dw, db, gin = G.new((cf, ct, 3, 3)), G.new((cf,)), G.new((B, Hh, W, 64), BF16)
    dw2, db2 = G.new((ct, 64, 3, 3)), G.new((ct,))
    assert call(tdx, "tdx_initial_conv_backward_io", e.x, e.g_fat.to(BF16), dw, db, scratch, B, Hh, W, ct, cf,
                1) == H.TDX_E_SHAPE
    assert call(tdx, "tdx_final_conv_backward_io", e.fat.to(BF16), e.g_thin, e.w_fin, gin, dw2, db2, scratch, B, Hh, W, ct,
                1) == H.TDX_E_SHAPE
    for t in (dw, db, dw2, db2, gin, scratch):
        assert all_nan(t)
    assert G.intact()
