"""CPU: the references, intervals, builders and the dispatch model of tests/io16_helpers.py, before any kernel is held
against them (tests/test_gpu_io16_dispatch.py).  For every family: torch's own fp32 evaluation of the operation on the
bf16 operands, rounded with .bfloat16(), lies inside every interval and bound; the same fp32 values TRUNCATED to bf16 do
not; one dropped contributor, row or split does not; the share of elements whose interval spans more than one bf16 value
stays under its cap.  Nothing here reads a kernel's output."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv_helpers as CH
import io16_helpers as H
import spatial_helpers as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = "cpu"


def _src(name):
    return open(os.path.join(ROOT, "tiny_diffusion_amd", "csrc", name)).read()


# ------------------------------------------------------------------------------------------------ bf16 arithmetic
def test_rne16_64_is_round_to_nearest_even_from_fp64():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -0.3, 0.0, 3e-5, 1e30],
                     dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, float(torch.tensor(-0.3).bfloat16()), 0.0,
                         float(torch.tensor(3e-5).bfloat16()), float(torch.tensor(1e30).bfloat16())], dtype=torch.float64)
    assert torch.equal(H.rne16_64(x), want)
    # a tie that a detour through fp32 would break the wrong way: 1 + 2^-8 + 2^-30 is above the tie, its fp32 value is not
    y = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30], dtype=torch.float64)
    assert float(H.rne16_64(y)) == 1.0 + 2.0 ** -7 and float(y.float().bfloat16()) == 1.0
    g = torch.randn(4096, generator=torch.Generator().manual_seed(1))
    assert torch.equal(H.rne16_64(g.double()), g.bfloat16().double())          # fp32 values: torch's own rounding
    t = H.trunc16(g)
    assert H.is16(t) and bool((t.abs() <= g.abs()).all()) and not torch.equal(t, H.r16(g))
    assert H.outside16(H.r16(g), g.double(), torch.zeros(4096, dtype=torch.float64)) == 0
    assert H.outside16(t, g.double(), torch.zeros(4096, dtype=torch.float64)) > 1000


def test_nudge_relu_in_bf16_moves_offenders_to_another_bf16_value():
    sc, sh = torch.tensor([1.0, -2.0, 0.5, 3.0]), torch.tensor([-0.5, 1.0, 0.25, 0.0])
    y = torch.tensor([[0.5, 0.5, -0.5, 0.0], [0.3, 0.7, 1.0, -1.0]])            # the first row is all offenders
    assert not S.relu_decidable(y, sc, sh)
    z = S.nudge_relu(y, sc, sh, bf16=True)
    assert H.is16(z) and S.relu_decidable(z, sc, sh) and bool((z[0] != y[0]).all())
    assert torch.equal(z[1], H.r16(y[1]))
    assert torch.equal(S.nudge_relu(y[1:], sc, sh), y[1:])                       # the fp32 form is what it was


# ------------------------------------------------------------------------------------------------ BatchNorm
def _bn32(d, training, s1=None, s2=None):
    """fp32 evaluation of the backward as torch computes it -> g' (fp32), dbeta, dgamma."""
    g, y = d["g"], d["y"]
    gz = torch.where(y * d["scale"] + d["shift"] > 0, g, torch.zeros_like(g))
    xh = (y - d["mean"]) * d["rstd"]
    s1 = gz.sum(0) if s1 is None else s1
    s2 = (gz * xh).sum(0) if s2 is None else s2
    N = g.shape[0]
    if training:
        return (d["gamma"] * d["rstd"]) * (gz - s1 / N - xh * (s2 / N)), s1, s2
    return gz * d["scale"], s1, s2


BN_CASES = [(C, H.bn_two_block_rows(C), False) for C in H.BN_WIDTHS] + H.BN_SHARE_CASES


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("C,rows,big", BN_CASES)
def test_bn_backward_interval(C, rows, big, training):
    d = H.bn_operands16(rows, C, S.case_seed(C, rows), CPU, big)
    K = S.bn_bwd_plan(rows, C)["K"]
    ref = S.bn_relu_bwd_ref(d["g"], d["y"], d["scale"], d["shift"], d["mean"], d["rstd"], d["gamma"], bool(training), K)
    g32, s1, s2 = _bn32(d, training)
    share = H.undecided_share(*ref["g"])
    print(f"bn g' C={C} rows={rows} train={training} undecided {100 * share:.2f} %")
    assert share <= (H.UNDECIDED_CAP_TRAIN_G if training else H.UNDECIDED_CAP)
    assert H.outside16(H.r16(g32), *ref["g"]) == 0
    assert S.elem_ratio(s1, *ref["dbeta"]) <= 1.0 and S.elem_ratio(s2, *ref["dgamma"]) <= 1.0
    out = H.outside16(H.trunc16(g32), *ref["g"])
    nz = int((ref["g"][0] != 0).sum())
    print(f"   truncated: {out} of {nz} non-zero elements outside")
    assert out > 0.1 * nz
    # one row dropped from the sums: dbeta / dgamma leave their bounds
    gz = torch.where(d["y"] * d["scale"] + d["shift"] > 0, d["g"], torch.zeros_like(d["g"]))
    if rows > 1 and bool((gz[0] != 0).any()):
        assert S.elem_ratio(s1 - gz[0], *ref["dbeta"]) > 1.0


@pytest.mark.parametrize("rows,C", H.APPLY16_CASES + [(3, 12)])
def test_bn_apply_interval(rows, C):
    d = H.bn_operands16(rows, C, S.case_seed(C, rows), CPU)
    ref, b = H.bn_apply_ref16(d["y"], d["scale"], d["shift"])
    o32 = torch.relu(d["y"] * d["scale"] + d["shift"])
    assert H.undecided_share(ref, b) <= H.UNDECIDED_CAP
    assert H.outside16(H.r16(o32), ref, b) == 0
    if rows * C >= 24:
        assert H.outside16(H.trunc16(o32), ref, b) > 0
    # the second channel quad normalised with the first quad's scale / shift
    if C >= 8:
        wrong = o32.clone()
        wrong[:, 4:8] = torch.relu(d["y"][:, 4:8] * d["scale"][0:4] + d["shift"][0:4])
        assert H.outside16(H.r16(wrong), ref, b) > 0


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("nblk", H.FROM_PARTIALS_NBLK)
def test_from_partials_reference(nblk, training):
    rows, C = H.FROM_PARTIALS_SHAPE
    d = H.bn_operands16(rows, C, S.case_seed(C, rows, nblk), CPU)
    part = H.host_partials(d, nblk, nblk)
    ref = H.bn_from_partials_ref(d["g"], d["y"], part, d["scale"], d["shift"], d["mean"], d["rstd"], d["gamma"],
                                 bool(training))
    s1, s2 = part[:, 0].double().sum(0).float(), part[:, 1].double().sum(0).float()
    g32, _, _ = _bn32(d, training, s1, s2)
    assert H.undecided_share(*ref["g"]) <= H.UNDECIDED_CAP      # nine roundings, no reduction: far below the 20 %
    assert H.outside16(H.r16(g32), *ref["g"]) == 0
    assert S.elem_ratio(s1, *ref["dbeta"]) <= 1.0 and S.elem_ratio(s2, *ref["dgamma"]) <= 1.0
    # one block of the caller's partials dropped (the last: a finalize loop one short)
    t1 = part[:-1, 0].double().sum(0).float() if nblk > 1 else torch.zeros(C)
    assert S.elem_ratio(t1, *ref["dbeta"]) > 1.0
    assert H.finalize_trips(nblk) == {1: 1, 255: 1, 256: 1, 257: 2, 2048: 8}[nblk]


# ------------------------------------------------------------------------------------------------ max-pool
@pytest.mark.parametrize("C", [4, 64])
@pytest.mark.parametrize("Hh,W", H.POOL_SHAPES)
def test_pool_operands_are_exact_in_bf16_and_sums_hold(Hh, W, C):
    for bn in (True, False):
        y, sc, sh, go, skip = H.pool_inputs16(2, Hh, W, C, S.case_seed(Hh, W, C, bn), CPU, bn)
        out, gin = S.maxpool_refs(y, sc, sh, go, skip)
        assert H.is16(out.float()) and H.is16(gin.float())                   # so the bf16 kernels are held bit for bit
        a = S.nchw(y) if not bn else torch.relu(S.nchw(y) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
        assert torch.equal(S.nhwc(F.max_pool2d(a, 2, ceil_mode=True)).double(), out)
    # the producer's sums (BN given): fp32 evaluation inside the bound; the skip gradient left out of them is not
    y, sc, sh, go, skip = H.pool_inputs16(2, Hh, W, C, S.case_seed(Hh, W, C, True), CPU, True)
    mean, rstd = H.pool_bn_stats(C, 5, CPU)
    _, gin = S.maxpool_refs(y, sc, sh, go, skip)
    _, gin_noskip = S.maxpool_refs(y, sc, sh, go, None)
    plan = H.pool_producer_plan(2, Hh, W, C)
    assert plan["branch"] == "producer" and plan["trips"] == 1
    ref = H.partial_sums_ref(gin, 0.0, y, sc, sh, mean, rstd, plan["K"])

    def sums32(gi):
        g2, y2 = gi.float().reshape(-1, C), y.reshape(-1, C)
        gz = torch.where(y2 * sc + sh > 0, g2, torch.zeros_like(g2))
        return gz.sum(0), (gz * ((y2 - mean) * rstd)).sum(0)

    s1, s2 = sums32(gin)
    assert S.elem_ratio(s1, *ref["s1"]) <= 1.0 and S.elem_ratio(s2, *ref["s2"]) <= 1.0
    if Hh * W > 1:
        t1, t2 = sums32(gin_noskip)
        assert S.elem_ratio(t1, *ref["s1"]) > 1.0 or S.elem_ratio(t2, *ref["s2"]) > 1.0


# ------------------------------------------------------------------------------------------------ resize
def _interp32(a_nhwc, Ho, Wo):
    return S.nhwc(F.interpolate(S.nchw(a_nhwc), size=(Ho, Wo), mode="bilinear", align_corners=True))


@pytest.mark.parametrize("shape", H.RESIZE_FWD_PAIRS, ids=str)
def test_resize_forward_interval(shape):
    Hi, Wi, Ho, Wo = shape
    d = H.resize_inputs16(3, Hi, Wi, Ho, Wo, 8, S.case_seed(*shape), CPU)
    assert H.is16(d["y"]) and H.is16(d["g"])
    for bn, add in ((True, True), (True, False), (False, True), (False, False)):
        sc, sh = (d["scale"], d["shift"]) if bn else (None, None)
        ad = d["addend"] if add else None
        ref, b = S.resize_fwd_ref(d["y"], sc, sh, ad, Ho, Wo)
        a = torch.relu(d["y"] * sc + sh) if bn else d["y"]
        if add:
            a = a + ad.view(3, 1, 1, -1)
        o32 = _interp32(a, Ho, Wo)
        share = H.undecided_share(ref, b)
        print(f"resize fwd {shape} bn={bn} add={add} undecided {100 * share:.2f} %")
        assert share <= H.UNDECIDED_CAP
        assert H.outside16(H.r16(o32), ref, b) == 0
        if o32.numel() >= 96:
            assert H.outside16(H.trunc16(o32), ref, b) > 0
    # a dropped tap: the W-axis interpolation replaced by its left neighbour
    if Wo > 1 and Wi > 1:
        ref, b = S.resize_fwd_ref(d["y"], None, None, None, Ho, Wo)
        wrong = _interp32(d["y"], Ho, Wo).clone()
        wrong[:, :, 1] = wrong[:, :, 0]
        assert H.outside16(H.r16(wrong), ref, b) > 0


@pytest.mark.parametrize("shape", list(H.RESIZE_BWD_CASES), ids=str)
def test_resize_adjoint_interval(shape):
    Hi, Wi, Ho, Wo = shape
    assert S.adjoint_branch(*shape) == H.RESIZE_BWD_CASES[shape]
    d = H.resize_inputs16(2, Hi, Wi, Ho, Wo, 8, S.case_seed(*shape), CPU)
    ref, b, _ = S.resize_adj_ref(d["g"], Hi, Wi)
    x = torch.zeros(2, Hi, Wi, 8, requires_grad=True)
    (g32,) = torch.autograd.grad(_interp32(x, Ho, Wo), x, d["g"])
    share = H.undecided_share(ref, b)
    print(f"resize adjoint {shape} undecided {100 * share:.2f} %")
    assert share <= H.UNDECIDED_CAP
    assert H.outside16(H.r16(g32), ref, b) == 0
    assert H.outside16(H.trunc16(g32), ref, b) > 0
    # one contributor dropped: the last output column does not reach its inputs
    gd = d["g"].clone()
    gd[:, :, -1] = 0
    (g_drop,) = torch.autograd.grad(_interp32(x, Ho, Wo), x, gd)
    assert H.outside16(H.r16(g_drop), ref, b) > 0
    # the producer's sums over the fp32 gradient, and with one row of it left out
    if H.RESIZE_BWD_CASES[shape] != "generic":
        plan = H.resize_producer_plan(2, Hi, Wi, Ho, Wo, 8)
        assert plan["branch"] == "producer:" + H.RESIZE_BWD_CASES[shape]
        bn_y = S.nudge_relu(torch.randn(2, Hi, Wi, 8, generator=torch.Generator().manual_seed(3)), d["scale"], d["shift"],
                            bf16=True)
        sums = H.partial_sums_ref(ref, b, bn_y, d["scale"], d["shift"], d["mean"], d["rstd"], plan["K"])
        y2, g2 = bn_y.reshape(-1, 8), g32.reshape(-1, 8)
        gz = torch.where(y2 * d["scale"] + d["shift"] > 0, g2, torch.zeros_like(g2))
        xh = (y2 - d["mean"]) * d["rstd"]
        assert S.elem_ratio(gz.sum(0), *sums["s1"]) <= 1.0 and S.elem_ratio((gz * xh).sum(0), *sums["s2"]) <= 1.0
        assert S.elem_ratio(gz[Wi:].sum(0), *sums["s1"]) > 1.0


@pytest.mark.parametrize("case", H.PAIR_CASES, ids=str)
def test_pair_reference(case):
    Ca, Cb, (Ha, Wa), (Hb, Wb), (Ho, Wo) = case
    B = 2
    gen = torch.Generator().manual_seed(S.case_seed(Ca, Cb, Ha, Wa))
    a, b_ = H.r16(torch.randn(B, Ha, Wa, Ca, generator=gen)), (H.r16(torch.randn(B, Hb, Wb, Cb, generator=gen)) if Cb else None)
    ad = torch.randn(B, Cb, generator=gen) if Cb else None
    ref, bound = H.pair_ref(a, None, b_, ad, Ho, Wo)
    parts = [_interp32(a, Ho, Wo)] + ([_interp32(b_ + ad.view(B, 1, 1, -1), Ho, Wo)] if Cb else [])
    o32 = torch.cat(parts, -1)
    assert ref.shape == (B, Ho, Wo, Ca + Cb) and H.undecided_share(ref, bound) <= H.UNDECIDED_CAP
    assert H.outside16(H.r16(o32), ref, bound) == 0 and S.elem_ratio(o32, ref, bound) <= 1.0
    assert H.outside16(H.trunc16(o32), ref, bound) > 0
    if Cb:    # the second source read at the channel index of the output
        wrong = o32.clone()
        wrong[..., Ca:] = torch.roll(o32[..., Ca:], 4, -1)
        assert H.outside16(H.r16(wrong), ref, bound) > 0
    for splits in (1, 2, 3):
        for with_bias in (True, False):
            df = H.defer_operands(B, Ha, Wa, Ca, splits, 7 + splits, CPU, with_bias)
            ref, bound = H.pair_ref(None, df, b_, ad, Ho, Wo)
            v = (df["bias"] if with_bias else torch.zeros(Ca)) + sum(df["parts"])
            o32 = torch.cat([_interp32(torch.relu(v * df["scale"] + df["shift"]), Ho, Wo)] + parts[1:], -1)
            assert S.elem_ratio(o32, ref, bound) <= 1.0 and H.outside16(H.r16(o32), ref, bound) == 0
            short = (df["bias"] if with_bias else torch.zeros(Ca)) + sum(df["parts"][:-1], torch.zeros_like(df["parts"][0]))
            w32 = torch.cat([_interp32(torch.relu(short * df["scale"] + df["shift"]), Ho, Wo)] + parts[1:], -1)
            assert S.elem_ratio(w32, ref, bound) > 1.0                      # the split loop one short
            if with_bias:
                late = torch.relu(sum(df["parts"]) * df["scale"] + df["shift"]) + df["bias"]
                w32 = torch.cat([_interp32(late, Ho, Wo)] + parts[1:], -1)
                assert S.elem_ratio(w32, ref, bound) > 1.0                  # the bias added after the ReLU


# ------------------------------------------------------------------------------------------------ pixel sum
@pytest.mark.parametrize("C", H.PIXEL_WIDTHS)
def test_pixel_sum_reference(C):
    rgroups = 256 // (C // 4)
    assert H.pixel_sum_hw(C) == sorted({1, rgroups + 1, 784} | ({rgroups - 1} if rgroups > 1 else set()))
    for HW in H.pixel_sum_hw(C):
        g = H.r16(torch.randn(2, HW, C, generator=torch.Generator().manual_seed(HW + C)))
        ref, b = H.pixel_sum_ref(g, C)
        assert S.elem_ratio(g.sum(1), ref, b) <= 1.0
        if HW > rgroups:
            assert S.elem_ratio(g[:, rgroups:].sum(1), ref, b) > 1.0         # the first rgroups rows skipped
    for Cbad in H.PIXEL_REFUSED:
        assert not H.width_ok(Cbad)


# ------------------------------------------------------------------------------------------------ boundary convolutions
@pytest.mark.parametrize("ct,cf", CH.EDGE_PAIRS)
@pytest.mark.parametrize("shape", CH.EDGE_SMALL, ids=str)
def test_edge_conv_intervals(shape, ct, cf):
    B, Hh, W = shape
    e = H.edge_operands16(B, Hh, W, ct, cf, 700 + Hh * W + ct, CPU)
    assert H.is16(e.g_fat) and H.is16(e.fat)
    refs = H.edge_refs(e)
    o32 = S.nhwc(F.conv2d(e.x, e.w_init, e.b_init, padding=1))
    gin32 = S.nhwc(F.conv_transpose2d(e.g_thin, e.w_fin, padding=1))
    fin32 = F.conv2d(S.nchw(e.fat), e.w_fin, e.b_fin, padding=1)
    for name, got in (("init_fwd", o32), ("fin_gin", gin32)):
        ref, mag, K = refs[name]
        b = H.edge_bound(mag, K)
        share = H.undecided_share(ref, b)
        print(f"edge {name} {shape} {ct}->{cf} undecided {100 * share:.2f} %")
        assert share <= H.UNDECIDED_CAP
        assert H.outside16(H.r16(got), ref, b) == 0
        assert H.outside16(H.trunc16(got), ref, b) > 0
    ref, mag, K = refs["fin_fwd"]
    assert CH.elem_ratio(fin32, ref, mag, K) <= CH.ELEM_DIRECT and CH.rel_err(fin32, ref) < H.EDGE_REL["fin_fwd"]
    # the fat operand read as if it were still fp32 (not rounded) moves the thin output out of its gate
    assert set(H.EDGE_REL) == set(refs) and set(H.EDGE_FAT_OUT) <= set(refs)


# ------------------------------------------------------------------------------------------------ host model
def test_constants_match_the_source():
    bn, sp, inl, knobs = _src("bn.hip"), _src("spatial.hip"), _src("internal.h"), _src("knobs.h")
    assert f"if (grid > {H.APPLY16_CAP}) grid = {H.APPLY16_CAP};" in bn and "(io16 ? n4 / 2 : n4)" in bn
    assert "const int c8n = C / 8;" in bn and "(io16 && C % 8)" in bn
    assert f"if (grid > {S.BN_BWD_APPLY_CAP}) grid = {S.BN_BWD_APPLY_CAP};" in bn
    assert "for (int t = sl; t < nblk; t += 256)" in bn
    assert f"#define TDX_BNBWD_MAX_PRODUCER_BLOCKS {H.PRODUCER_CAP} " in inl
    assert f"int cap = {H.PLAIN_CAP})" in sp
    assert f"g_knobs.bnbwd_fused & {H.KNOB_POOL})" in sp and f"g_knobs.bnbwd_fused & {H.KNOB_RESIZE})" in sp
    assert "C > 1024 || 256 % (C / 4)" in sp
    assert f"#define BIL_ROW_MAXW {S.BIL_ROW_MAXW}" in sp and f"#define BIL_BATCH {S.BIL_BATCH}" in sp
    assert "ew_grid(n, 256, TDX_BNBWD_MAX_PRODUCER_BLOCKS)" in sp
    assert "rows < TDX_BNBWD_MAX_PRODUCER_BLOCKS ? rows : TDX_BNBWD_MAX_PRODUCER_BLOCKS" in sp
    assert f"int bnbwd_fused = {H.BNBWD_FUSED_DEFAULT};" in knobs
    io = _src("io16.h")
    assert "o[0] = (tdx_bf16)v.x;" in io       # the store converts (round to nearest even), it does not shift


def test_dispatch_model_names_the_branch_of_every_case():
    # io16 apply grid
    assert H.apply16_plan(3, 12)["branch"] == "refused" and H.apply16_plan(3, 4)["branch"] == "refused"
    for rows, C in H.APPLY16_CASES:
        assert H.apply16_plan(rows, C) == {"branch": "apply16", "grid": -(-rows * C // 8 // 256), "trips": 1}
    assert H.apply16_plan(*H.APPLY16_BIG) == {"branch": "apply16", "grid": 8192, "trips": 2}
    assert H.apply16_plan(H.APPLY16_BIG[0] - 8, 8)["trips"] == 1
    # the backward's apply pass
    C, rows = H.BN_APPLY_BIG
    assert H.bwd_apply_trips(rows, C) == 2 and H.bwd_apply_trips(rows - 1, C) == 1
    for C in H.BN_WIDTHS:
        plan = S.bn_bwd_plan(H.bn_two_block_rows(C), C)
        assert plan["nblk"] == 2 and plan["regime"] == "floor"
    # max-pool producer: 2048 workgroups against 4096 of the plain form, and every fall-back
    B, Hh, W, C = H.POOL_PRODUCER_BIG
    big = H.pool_producer_plan(B, Hh, W, C)
    assert big["branch"] == "producer" and big["grid"] == 2048 and big["trips"] == 2 and big["K"] == 8 + 256
    plain = H.pool_producer_plan(B, Hh, W, C, partial_given=False)       # the same map under the plain cap: one trip
    assert plain["grid"] == 4096 and plain["trips"] == 1 and plain["nblk"] == 0
    assert H.pool_producer_plan(*S.POOL_BIG, partial_given=False)["grid"] == 4096
    assert H.pool_producer_plan(*S.POOL_BIG)["grid"] == 2048 and H.pool_producer_plan(*S.POOL_BIG)["trips"] == 3
    for C in H.POOL_PRODUCER_WIDTHS:
        for Hh, W in H.POOL_SHAPES:
            p = H.pool_producer_plan(2, Hh, W, C)
            assert p["branch"] == "producer" and p["trips"] == 1 and p["nblk"] == p["grid"] <= 2048
    assert H.pool_producer_plan(2, 5, 4, 64, knob=2)["why"] == "knob bit 2 off"
    assert H.pool_producer_plan(2, 5, 4, 12)["why"] == "width"
    assert H.pool_producer_plan(2, 5, 4, 2048)["why"] == "width"
    assert H.pool_producer_plan(2, 5, 4, 64, scale_given=False)["why"] == "scale == NULL"
    assert all(H.pool_producer_plan(2, 5, 4, 64, **kw)["nblk"] == 0 for kw in ({"knob": 2}, {"scale_given": False}))
    # resize producer
    for shape in H.RESIZE_PRODUCER_SHAPES:
        for C in (4, 64, 1024):
            p = H.resize_producer_plan(3, *shape, C)
            assert p["branch"] == "producer:" + H.RESIZE_BWD_CASES[shape] and p["nblk"] == 3 * shape[0]
            assert p["rows_per_wg"] == 1
    B, Hi, Wi, Ho, Wo, C = H.RESIZE_PRODUCER_MANY_ROWS
    many = H.resize_producer_plan(B, Hi, Wi, Ho, Wo, C)
    assert many["grid"] == 2048 and many["rows_per_wg"] == 2 and B * Hi > 2048
    assert H.resize_producer_plan(3, 4, 7, 8, 8, 64, knob=4)["why"] == "knob bit 1 off"
    assert H.resize_producer_plan(3, 65, 3, 66, 6, 64)["why"] == "Hi or Wi > 64"
    assert H.resize_producer_plan(3, 3, 65, 6, 66, 64)["why"] == "Hi or Wi > 64"
    assert H.resize_producer_plan(3, 4, 7, 8, 8, 12)["why"] == "width"
    assert H.resize_producer_plan(3, 4, 7, 8, 8, 2048)["why"] == "width"
    assert H.resize_producer_plan(3, 7, 4, 8, 16, 64)["branch"] == "rejected"
    for shape, branch in H.RESIZE_BWD_CASES.items():
        assert S.adjoint_branch(*shape) == branch
    assert set(H.RESIZE_BWD_CASES.values()) == {"rows-batched", "rows-loop", "generic"}
    assert {H.finalize_trips(n) for n in H.FROM_PARTIALS_NBLK} == {1, 2, 8}


def test_every_new_entry_is_declared_and_bound():
    import tiny_diffusion_amd._lib as L

    hdr = open(os.path.join(ROOT, "include", "tdx.h")).read()
    for name in ("tdx_bn_apply_relu_fwd_io", "tdx_bn_relu_bwd_io", "tdx_bn_relu_bwd_from_partials",
                 "tdx_maxpool2_ceil_fwd_io", "tdx_maxpool2_ceil_bwd_io", "tdx_bilinear_ac_fwd_io", "tdx_bilinear_ac_bwd_io",
                 "tdx_bilinear_pair_fwd_io", "tdx_pixel_sum_io", "tdx_initial_conv_forward_io",
                 "tdx_initial_conv_backward_io", "tdx_initial_conv_input_grad_io", "tdx_final_conv_forward_io",
                 "tdx_final_conv_backward_io"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.EXPORTS, name
    # refusals that need no device: checked before any launch, so NULL tensors never reach a kernel
    lib = L.lib
    one = torch.zeros(64)
    p = one.data_ptr()
    assert lib.tdx_bn_apply_relu_fwd_io(p, p, 3, 12, p, p, 1, None) == H.TDX_E_SHAPE
    assert lib.tdx_bn_apply_relu_fwd_io(None, p, 3, 8, p, p, 1, None) == H.TDX_E_BADARG
    assert lib.tdx_pixel_sum_io(None, p, 1, 1, 4, 1, None) == H.TDX_E_BADARG
    for C in H.PIXEL_REFUSED:
        assert lib.tdx_pixel_sum_io(p, p, 1, 1, C, 1, None) == H.TDX_E_SHAPE
    assert lib.tdx_maxpool2_ceil_bwd_io(p, p, p, p, None, p, 1, 2, 2, 4, p, p, p, None, 1, None) == H.TDX_E_BADARG  # nblk
    assert lib.tdx_bilinear_ac_bwd_io(p, p, 1, 2, 2, 3, 3, 4, 4, 0, p, p, p, p, p, p, None, 0, None) == H.TDX_E_BADARG
    assert lib.tdx_bilinear_ac_bwd_io(p, p, 1, 2, 2, 9, 3, 4, 4, 0, None, None, None, None, None, None, None, 1,
                                      None) == H.TDX_E_SHAPE
    assert lib.tdx_bn_relu_bwd_from_partials(p, p, 4, 4, p, p, p, p, p, p, p, p, None, 1, p, 1, 1, None) == H.TDX_E_BADARG
    assert lib.tdx_bn_relu_bwd_from_partials(p, p, 4, 4, p, p, p, p, p, p, p, p, p, 0, p, 1, 1, None) == H.TDX_E_BADARG
    assert lib.tdx_bn_relu_bwd_from_partials(p, p, 4, 6, p, p, p, p, p, p, p, p, p, 1, p, 1, 1, None) == H.TDX_E_SHAPE
    assert lib.tdx_bn_relu_bwd_io(p, p, 4, 12, p, p, p, p, p, p, p, p, p, 1, 1, None) == H.TDX_E_SHAPE
    assert lib.tdx_bilinear_pair_fwd_io(None, None, 0, 0, None, None, None, 2, 2, 4, None, None, 1, 1, 0, p, 1, 2, 2, 1,
                                        None) == H.TDX_E_BADARG
    assert lib.tdx_bilinear_pair_fwd_io(None, p, 2, 8, None, p, p, 2, 2, 4, None, None, 1, 1, 0, p, 1, 2, 2, 1,
                                        None) == H.TDX_E_BADARG          # slabs that overlap
    assert lib.tdx_bilinear_pair_fwd_io(p, None, 0, 0, None, None, None, 2, 2, 6, None, None, 1, 1, 0, p, 1, 2, 2, 1,
                                        None) == H.TDX_E_SHAPE
    assert lib.tdx_final_conv_backward_io(p, p, p, p, p, p, p, 1, 4, 3, 1, 1, None) == H.TDX_E_SHAPE
    assert lib.tdx_initial_conv_backward_io(p, p, p, p, p, 1, 4, 3, 1, 64, 1, None) == H.TDX_E_SHAPE
