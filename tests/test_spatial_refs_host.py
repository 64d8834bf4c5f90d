"""CPU checks of tests/spatial_helpers.py: the fp64 references against torch at non-square shapes, the
adjoint identity of the reference pair, every input builder on every shape and seed of
tests/test_gpu_spatial_bn_dispatch.py, and the host model of the dispatch - which branch of csrc/bn.hip and
csrc/spatial.hip each of those cases is there to reach."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spatial_helpers as S
from oracle import ref_cpu as R

ALL_RESIZES = list(S.RESIZE_CASES) + [(hi, 3, ho, 5) for hi, ho in S.RESIZE_REJECTED_AXES] \
    + [(3, wi, 5, wo) for wi, wo in S.RESIZE_REJECTED_AXES]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("shape", ALL_RESIZES)
def test_resize_references_against_torch_fp64(shape):
    """Exact-coordinate operator == F.interpolate(align_corners=True) in fp64, its transpose == autograd; the oracle's
    R.bilinear_ac (fp32 coordinates) lies within the coordinate term of it; <g, fwd(a)> == <bwd(g), a> to 1e-12."""
    Hi, Wi, Ho, Wo = shape
    g = torch.Generator().manual_seed(S.case_seed(*shape))
    a = torch.randn(2, Hi, Wi, 4, generator=g, dtype=torch.float64)
    go = torch.randn(2, Ho, Wo, 4, generator=g, dtype=torch.float64)
    an = S.nchw(a).requires_grad_(True)
    ref = F.interpolate(an, size=(Ho, Wo), mode="bilinear", align_corners=True)
    (ga,) = torch.autograd.grad(ref, an, S.nchw(go))
    fwd = S.resize_fwd_exact(a, Ho, Wo)
    adj, bound, rounding = S.resize_adj_ref(go, Hi, Wi)
    assert _rel(fwd, S.nhwc(ref.detach())) < 1e-12
    assert _rel(adj, S.nhwc(ga)) < 1e-12
    assert bool((bound >= rounding).all())
    lhs, rhs = float((go * fwd).sum()), float((adj * a).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((go.abs() * S.resize_fwd_exact(a.abs(), Ho, Wo)).sum())
    oracle, _ = S.resize_fwd_ref(a.float(), None, None, None, Ho, Wo)
    a32 = a.float().double()
    slack = S.resize_coord_term_fwd(a32.abs(), Ho, Wo) + 2 * S.U * S.resize_fwd_exact(a32.abs(), Ho, Wo)
    assert bool(((oracle - S.resize_fwd_exact(a32, Ho, Wo)).abs() <= slack).all())


@pytest.mark.parametrize("shape", ALL_RESIZES)
def test_resize_bounds_hold_for_torch_fp32_and_not_for_a_dropped_contributor(shape):
    """ATen's own fp32 resize and its fp32 backward (same taps, other summation order) sit inside the bounds the GPU
    test applies; the adjoint with its largest contribution to one input element dropped does not."""
    Hi, Wi, Ho, Wo = shape
    d = S.resize_inputs(2, Hi, Wi, Ho, Wo, 8, S.case_seed(*shape), "cpu")
    ref, bound = S.resize_fwd_ref(d["y"], None, None, None, Ho, Wo)
    an = S.nchw(d["y"]).requires_grad_(True)
    out = F.interpolate(an, size=(Ho, Wo), mode="bilinear", align_corners=True)
    assert S.elem_ratio(S.nhwc(out.detach()), ref, bound) <= 1.0
    (ga,) = torch.autograd.grad(out, an, S.nchw(d["g"]))
    adj, abound, _ = S.resize_adj_ref(d["g"], Hi, Wi)
    assert S.elem_ratio(S.nhwc(ga), adj, abound) <= 1.0
    # one output's contribution to one input: Wh[o, h] Ww[p, w] g[o, p]
    Mh, Mw = S.ac_matrix(Hi, Ho), S.ac_matrix(Wi, Wo)
    contrib = torch.einsum("oh,pw,bopc->bophwc", Mh, Mw, d["g"].double())
    worst = contrib.abs().amax(dim=(1, 2))
    assert S.elem_ratio(adj - worst, adj, abound) > 1.0


@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("H,W", S.POOL_SHAPES)
def test_maxpool_references_against_torch_fp64(H, W, bn):
    y, sc, sh, go, skip = S.maxpool_inputs(3, H, W, 8, S.case_seed(H, W, 8, bn), "cpu", bn)
    out, gin = S.maxpool_refs(y, sc, sh, go, skip)
    a = S.nchw(y.double())
    if bn:
        a = torch.relu(a * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
    a.requires_grad_(True)
    ref = F.max_pool2d(a, 2, ceil_mode=True)
    (ga,) = torch.autograd.grad(ref, a, S.nchw(go.double()))
    assert torch.equal(out, S.nhwc(ref.detach()))
    assert torch.equal(gin, S.nhwc(ga + S.nchw(skip.double())))
    out2, gin2 = S.maxpool_refs(y, sc, sh, go, None)
    assert torch.equal(out2, out) and torch.equal(gin2, S.nhwc(ga))
    # dyadic: the fp32 evaluation is the fp64 one
    assert torch.equal(out.float().double(), out) and torch.equal(gin.float().double(), gin)


@pytest.mark.parametrize("training", [True, False])
def test_bn_references_against_torch_fp64(training):
    """bn_finalize_ref from tile partials == R.batchnorm2d / F.batch_norm in fp64 (scale, shift, running statistics);
    bn_relu_bwd_ref == autograd through F.batch_norm + ReLU, train and eval mode, at a non-square map."""
    B, H, W, C = 3, 5, 7, 8
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 0.7 + 3.0 * torch.randn(1, C, 1, 1, generator=g, dtype=torch.float64)
    gamma = 1 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    rm, rv = 0.1 * torch.randn(C, generator=g, dtype=torch.float64), 1 + torch.rand(C, generator=g, dtype=torch.float64)
    go = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    rows = S.nhwc(x).view(-1, C)
    # (the partials stay in fp64 here: this test is about the formulas)
    tile_rows = 13
    stats = torch.stack([torch.stack([blk.sum(0), (blk - blk.mean(0)).pow(2).sum(0)]) for blk in rows.split(tile_rows)])
    fin = S.bn_finalize_ref(stats, tile_rows, rows.shape[0], gamma, beta, rm, rv, training)
    rm2, rv2 = rm.clone(), rv.clone()
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    act = torch.relu(F.batch_norm(xr, rm2, rv2, gr, br, training, 0.1, 1e-5))
    act_oracle = torch.relu(R.batchnorm2d(x, gamma, beta, rm.clone(), rv.clone(), training))
    mine = torch.relu(rows * fin["scale"][0] + fin["shift"][0])
    assert _rel(mine, S.nhwc(act.detach()).view(-1, C)) < 1e-12
    assert _rel(mine, S.nhwc(act_oracle).view(-1, C)) < 1e-12
    if training:
        assert _rel(fin["running_mean"][0], rm2) < 1e-12 and _rel(fin["running_var"][0], rv2) < 1e-12
        assert _rel(fin["save_mean"][0], rows.mean(0)) < 1e-12
    else:
        assert "running_mean" not in fin and torch.equal(fin["save_mean"][0], rm)
    act.backward(go)
    bw = S.bn_relu_bwd_ref(S.nhwc(go).view(-1, C), rows, fin["scale"][0], fin["shift"][0], fin["save_mean"][0],
                           fin["save_rstd"][0], gamma, training, K=10)
    assert _rel(bw["g"][0], S.nhwc(xr.grad).view(-1, C)) < 1e-11
    assert _rel(bw["dgamma"][0], gr.grad) < 1e-11 and _rel(bw["dbeta"][0], br.grad) < 1e-11
    dbias = xr.grad.sum((0, 2, 3))
    if training:
        assert float(bw["dbias"][0].abs().max()) == 0.0 and float(dbias.abs().max()) < 1e-12
    else:
        assert _rel(bw["dbias"][0], dbias) < 1e-11


@pytest.mark.parametrize("training", [True, False])
def test_bn_bounds_hold_for_torch_fp32_and_not_for_a_dropped_row(training):
    """The same formulas in fp32 on the CPU (torch sums pairwise: fewer roundings than the kernel's chains) sit inside
    the bounds; sums that miss one row do not."""
    rows, C = 513, 64
    d = S.bn_operands(rows, C, 3, "cpu", big_mean=True)
    K = S.bn_bwd_plan(rows, C)["K"]
    ref = S.bn_relu_bwd_ref(d["g"], d["y"], d["scale"], d["shift"], d["mean"], d["rstd"], d["gamma"], training, K)
    gz = torch.where(torch.addcmul(d["shift"], d["y"], d["scale"]) > 0, d["g"], torch.zeros(()))
    xh = (d["y"] - d["mean"]) * d["rstd"]
    s1, s2 = gz.sum(0), (gz * xh).sum(0)
    if training:
        out = (d["gamma"] * d["rstd"]) * (gz - s1 / rows - xh * (s2 / rows))
    else:
        out = gz * d["scale"]
    assert S.elem_ratio(out, *ref["g"]) <= 1.0
    assert S.elem_ratio(s1, *ref["dbeta"]) <= 1.0 and S.elem_ratio(s2, *ref["dgamma"]) <= 1.0
    assert S.elem_ratio(s1 - gz[-1], *ref["dbeta"]) > 1.0
    assert S.elem_ratio(s2 - (gz * xh)[-1], *ref["dgamma"]) > 1.0


def test_bn_finalize_bounds_hold_for_a_float_evaluation():
    """bn_finalize_ref's bounds against the kernel's formulas evaluated in numpy (double merge, float results)."""
    for tiles, tile_rows, count, C, big in S.FINALIZE_CASES:
        d = S.bn_finalize_operands(tiles, tile_rows, count, C, S.case_seed(tiles, tile_rows, C), "cpu", big)
        ref = S.bn_finalize_ref(d["stats"], tile_rows, count, d["gamma"], d["beta"], d["running_mean"],
                                d["running_var"], True)
        st = d["stats"].double().numpy()
        n_t = np.full((tiles, 1), float(tile_rows))
        n_t[-1] = count - (tiles - 1) * tile_rows
        Ssum, Q, Rr = st[:, 0].sum(0), st[:, 1].sum(0), (st[:, 0] ** 2 / n_t).sum(0)
        mean = Ssum / count
        m2 = np.maximum(Q + (Rr - Ssum * Ssum / count), 0.0)
        f = np.float32
        rstd = (1.0 / np.sqrt(m2 / count + float(f(1e-5)))).astype(f)
        sc = d["gamma"].numpy() * rstd
        got = {"save_mean": mean.astype(f), "save_rstd": rstd, "scale": sc,
               "shift": d["beta"].numpy() - mean.astype(f) * sc,
               "running_mean": f(f(1) - f(0.1)) * d["running_mean"].numpy() + f(0.1) * mean.astype(f),
               "running_var": f(f(1) - f(0.1)) * d["running_var"].numpy()
               + f(0.1) * (m2 / (count - 1) if count > 1 else m2 / count).astype(f)}
        for k, v in got.items():
            assert v.dtype == np.float32
            assert S.elem_ratio(torch.from_numpy(v), *ref[k]) <= 1.0, (tiles, count, C, k)


# ------------------------------------------------------------------------------------------------ builders
def test_relu_builder_leaves_every_element_decidable():
    g = torch.Generator().manual_seed(0)
    scale, shift = torch.tensor([1.0, -2.0, 0.5, 3.0]), torch.tensor([0.0, 1.0, -0.25, 1e-3])
    y = torch.randn(1000, 4, generator=g)
    y[:50] = (-shift / scale) * (1 + 2.0 ** -23 * torch.randint(-3, 4, (50, 4), generator=g))   # on the threshold
    y[50:60] = 0.0
    assert not S.relu_decidable(y, scale, shift)
    y2 = S.nudge_relu(y, scale, shift)
    assert S.relu_decidable(y2, scale, shift) and y2.shape == y.shape
    assert float((y2 - y).abs().max()) < 1e-5 and int((y2 != y).sum()) >= 50


def test_bn_builders_on_every_gpu_case():
    """bn_operands asserts decidability itself; every (C, rows) of the GPU test, same seeds."""
    for C in S.BN_BWD_WIDTHS:
        for rows in S.bn_floor_rows(C):
            S.bn_operands(rows, C, S.case_seed(C, rows), "cpu")
    for C, rows, _, _ in S.BN_BWD_OTHER:
        d = S.bn_operands(rows, C, S.case_seed(C, rows), "cpu", big_mean=(C == 128))
        assert S.relu_decidable(d["y"], d["scale"], d["shift"])
    for rows, C in S.APPLY_CASES:
        S.bn_operands(rows, C, S.case_seed(C, rows), "cpu")


def test_pool_and_resize_builders_on_every_gpu_case():
    for bn in (True, False):
        for C in (4, 1024):
            for H, W in S.POOL_SHAPES:
                S.maxpool_inputs(2, H, W, C, S.case_seed(H, W, C, bn), "cpu", bn)
        B, H, W, C = S.POOL_BIG
        S.maxpool_inputs(B, H, W, C, S.case_seed(H, W, C, bn), "cpu", bn)
    for shape in ALL_RESIZES:
        d = S.resize_inputs(3, *shape, 8, S.case_seed(*shape), "cpu")
        assert S.relu_decidable(d["y"], d["scale"], d["shift"])
    for B, Hi, Wi, Ho, Wo, C in (S.RESIZE_FWD_BIG, S.RESIZE_BWD_BIG):
        S.resize_inputs(B, Hi, Wi, Ho, Wo, C, S.case_seed(Hi, Wi, Ho, Wo), "cpu")


# ------------------------------------------------------------------------------------------------ dispatch model
def test_resize_adjoint_branch_of_every_case():
    """include/tdx.h: at most 8 contributing outputs per input index and axis, decided on the candidate window.  Which
    branch each case of the GPU test reaches; BIL_BATCH = 5 and BIL_MAXC = 8 are what these expectations pin."""
    for shape, want in S.RESIZE_CASES.items():
        assert S.adjoint_branch(*shape) == want, shape
    assert set(S.RESIZE_CASES.values()) == {"rows-batched", "rows-loop", "generic", "rejected"}
    span = lambda a, b: max(S.axis_spans32(a, b))   # noqa: E731
    # what the unit tests of test_gpu_ops.py and the networks reach: never more than 4
    for hi, ho in [(4, 8), (7, 8), (8, 16), (14, 16), (16, 32), (28, 32), (32, 28), (32, 64)]:
        assert S.adjoint_axis_ok(hi, ho) and span(hi, ho) <= 4
    assert span(3, 7) == 5 and span(2, 6) == 5 and span(2, 7) == 6 and span(2, 8) == 7 and span(1, 8) == 8
    for hi, ho in S.RESIZE_REJECTED_AXES + [(4, 16)]:
        assert not S.adjoint_axis_ok(hi, ho)
    assert span(2, 9) == 8 and span(3, 9) == 7 and span(1, 9) == 9 and span(4, 16) == 9   # the window rule is the stricter one
    # an accepted axis never has more than BIL_MAXC contributors
    for n_in in range(1, 40):
        for n_out in range(1, 80):
            if S.adjoint_axis_ok(n_in, n_out):
                assert span(n_in, n_out) <= S.BIL_MAXC, (n_in, n_out)
    # include/tdx.h: n_out <= 2 n_in always passes
    assert all(S.adjoint_axis_ok(n_in, n_out) for n_in in range(1, 70) for n_out in range(1, 2 * n_in + 1))
    # the particular things the case list is there for
    assert span(2, 6) == S.BIL_BATCH and S.adjoint_branch(3, 2, 7, 6) == "rows-batched"      # wn == BIL_BATCH exactly
    assert span(2, 7) > S.BIL_BATCH >= span(3, 5) and span(3, 8) > S.BIL_BATCH             # (2, 3, 7, 5): hn alone
    assert span(2, 7) > S.BIL_BATCH and span(1, 8) > S.BIL_BATCH                            # (1, 2, 8, 7): both
    assert S.axis_spans32(64, 2).count(0) == 62 and S.axis_spans32(5, 1) == [1, 0, 0, 0, 0]   # empty windows
    assert S.axis_spans32(1, 8) == [8] and S.axis_spans32(1, 1) == [1]
    B, Hi, Wi, Ho, Wo, C = S.RESIZE_BWD_BIG
    assert B * Hi > S.BIL_ROW_GRID and S.adjoint_branch(Hi, Wi, Ho, Wo) == "rows-batched"
    B, Hi, Wi, Ho, Wo, C = S.RESIZE_FWD_BIG
    assert B * Ho * Wo * C // 4 > S.EW_GRID_CAP * 256
    B, H, W, C = S.POOL_BIG
    assert B * ((H + 1) // 2) * ((W + 1) // 2) * C // 4 > S.EW_GRID_CAP * 256


def test_bn_branch_of_every_case():
    assert [C for C in range(1, 2049) if S.bn_bwd_width_ok(C)] == list(S.BN_BWD_WIDTHS)
    for C in S.BN_BWD_WIDTHS:
        rg = 256 // (C // 4)
        for rows in S.bn_floor_rows(C):
            p = S.bn_bwd_plan(rows, C)
            assert p["regime"] == "floor" and p["rpb"] == 2 * rg and p["nblk"] == -(-rows // p["rpb"])
        assert {S.bn_bwd_plan(r, C)["nblk"] for r in S.bn_floor_rows(C)} == {1, 2}
    for C, rows, regime, _ in S.BN_BWD_OTHER:
        assert S.bn_bwd_plan(rows, C)["regime"] == regime, (C, rows)
    assert S.bn_bwd_plan(4100, 1024)["rpb"] == 3 and S.bn_bwd_plan(40000, 128)["rpb"] == 24
    assert S.bn_bwd_plan(1048582, 4)["rpb"] == 512 and S.bn_bwd_plan(1048582, 4)["nblk"] == 2049
    assert S.bn_bwd_plan(4800, 128)["nblk"] == 300 > 256
    p = S.bn_bwd_plan(524289, 8)
    assert p["rpb"] == 384 and p["apply_grid"] == 4097 > S.BN_BWD_APPLY_CAP
    assert S.bn_bwd_plan(524288, 8)["rpb"] == 256 == 2 * p["rgroups"]      # the floor's last row count: that case is one past it
    rows, C = S.APPLY_CASES[1]
    assert rows * C // 4 > S.BN_APPLY_CAP * 256
    assert sorted({t for t, *_ in S.FINALIZE_CASES}) == [1, 2, 3, 256, 257, 600]


def test_argument_checks_of_the_library_return_before_any_launch():
    """The refusals involve no launch, so they run without a GPU (host pointers, never dereferenced): C % 4 != 0 in
    tdx_bn_finalize, the illegal widths of tdx_bn_relu_bwd, and every axis pair the model above calls rejected in
    tdx_bilinear_ac_bwd (the other direction - what the model accepts, the library runs - is the GPU test's)."""
    import ctypes as C

    import tiny_diffusion_amd._lib as L

    buf = (C.c_float * 65536)()
    p = C.addressof(buf)
    for training in (1, 0):
        for width in (6, 2, 1022, 7):
            assert L.lib.tdx_bn_finalize(p, 3, 5, 13, width, p, p, p, p, p, p, p, p, p, training, None) == S.TDX_E_SHAPE
        for width in (12, 6, 2048):
            assert L.lib.tdx_bn_relu_bwd_scratch_floats(5, width) == 0
            assert L.lib.tdx_bn_relu_bwd(p, p, 5, width, p, p, p, p, p, p, p, p, p, training, None) == S.TDX_E_SHAPE
    rejected = [(a, b) for a in range(1, 20) for b in range(1, 60) if not S.adjoint_axis_ok(a, b)]
    assert set(S.RESIZE_REJECTED_AXES) <= set(rejected) and (4, 16) in rejected
    for n_in, n_out in rejected:
        assert L.lib.tdx_bilinear_ac_bwd(p, p, 2, n_in, 3, n_out, 5, 8, 8, 0, None) == S.TDX_E_SHAPE, (n_in, n_out)
        assert L.lib.tdx_bilinear_ac_bwd(p, p, 2, 3, n_in, 5, n_out, 8, 8, 0, None) == S.TDX_E_SHAPE, (n_in, n_out)
    for cs, co in [(26, 4), (24, 6), (8, 4), (12, 8)]:
        assert L.lib.tdx_bilinear_ac_fwd(p, None, None, None, p, 2, 3, 4, 5, 7, 8, cs, co, None) == S.TDX_E_SHAPE
        assert L.lib.tdx_bilinear_ac_bwd(p, p, 2, 3, 4, 5, 7, 8, cs, co, None) == S.TDX_E_SHAPE
