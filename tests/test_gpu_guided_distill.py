"""Guided distillation on the device: ``tdx_distill_teacher_step_guided``,
``tdx_distill_target_guided`` and ``tdx_distill_guidance_target`` bit for bit against the fp32 restatements of
tests/guided_distill_helpers.py, against their unguided siblings, against the guided sampler update, and against the
properties that define the two targets; ``DistillStep(guidance_scale=w)`` and ``GuidanceDistillStep`` against the same
launches issued by hand, the adaptive timestep sampler under the latter, and one short learning check.

The bitwise comparisons hold because the build has fp contraction off and every operation of the kernels is rounded on
its own: a numpy fp32 expression with one operation per rounding is the same arithmetic."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import distill_helpers as H  # noqa: E402
import guided_distill_helpers as GH  # noqa: E402
from oracle.weights import make_state_dict, make_state_dict_laion  # noqa: E402

from tiny_diffusion_amd import _lib  # noqa: E402
from tiny_diffusion_amd._lib import check, lib  # noqa: E402
from tiny_diffusion_amd.schedule import (ForwardProcess, ddim_schedule, ddpm_schedule, distill_tables,  # noqa: E402
                                         guidance_distill_table, trailing_timesteps, truncated_snr_weights)

TDX_E_BADARG = -1
T = 1000
INF = math.inf
POISON = float("nan")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if dtype is None else torch.tensor(a, dtype=dtype).cuda()


def _assert_bits(got, want, what):
    g, w = H.bits(got), H.bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = int((g != w).sum())
    assert bad == 0, f"{what}: {bad} of {g.size} elements differ in their bits"


def _run_pair(tab, t, z, o1, o2, w, lo, hi, x_tilde=True):
    """The guided pair on numpy inputs (o1, o2: (2, B, ...)); w None: the unguided pair on o1[0], o2[0].  Outputs start
    as NaN / -7 so that an element left unwritten shows."""
    rows, tmt = tab.rows.cuda(), tab.t_mid.cuda()
    B, per = z.shape[0], z[0].size
    zt, td = _dev(z), _dev(t, torch.int64)
    x1c, target = torch.full_like(zt, POISON), torch.full_like(zt, POISON)
    xt = torch.full_like(zt, POISON) if x_tilde else None
    if w is None:
        d1, d2 = _dev(o1[0]), _dev(o2[0])
        z_mid = torch.full_like(zt, POISON)
        t_mid = torch.full((B,), -7, dtype=torch.int64, device="cuda")
        check(lib.tdx_distill_teacher_step(zt.data_ptr(), d1.data_ptr(), td.data_ptr(), rows.data_ptr(), tmt.data_ptr(),
                                           z_mid.data_ptr(), x1c.data_ptr(), t_mid.data_ptr(), B, per, lo, hi, _st()))
        check(lib.tdx_distill_target(zt.data_ptr(), z_mid.data_ptr(), d2.data_ptr(), x1c.data_ptr(), td.data_ptr(),
                                     rows.data_ptr(), target.data_ptr(), _lib.ptr(xt), B, per, lo, hi, _st()))
    else:
        d1, d2 = _dev(o1), _dev(o2)
        z_mid = torch.full((2,) + tuple(zt.shape), POISON, device="cuda")
        t_mid = torch.full((2, B), -7, dtype=torch.int64, device="cuda")
        check(lib.tdx_distill_teacher_step_guided(zt.data_ptr(), d1.data_ptr(), td.data_ptr(), rows.data_ptr(),
                                                  tmt.data_ptr(), z_mid.data_ptr(), x1c.data_ptr(), t_mid.data_ptr(), B,
                                                  per, w, lo, hi, _st()), "tdx_distill_teacher_step_guided")
        check(lib.tdx_distill_target_guided(zt.data_ptr(), z_mid.data_ptr(), d2.data_ptr(), x1c.data_ptr(),
                                            td.data_ptr(), rows.data_ptr(), target.data_ptr(), _lib.ptr(xt), B, per, w,
                                            lo, hi, _st()), "tdx_distill_target_guided")
    torch.cuda.synchronize()
    return {"z_mid": z_mid, "x1c": x1c, "target": target, "x_tilde": xt, "t_mid": t_mid}


def _run_same(rows4, t, z, o, w, lo, hi, x0c=True):
    """tdx_distill_guidance_target on numpy inputs; o is (2, B, ...) and w None runs guided = 0 on o[0]."""
    B, per = z.shape[0], z[0].size
    zt, td, rows = _dev(z), _dev(t, torch.int64), rows4.cuda()
    d = _dev(o[0] if w is None else o)
    target = torch.full_like(zt, POISON)
    xc = torch.full_like(zt, POISON) if x0c else None
    check(lib.tdx_distill_guidance_target(zt.data_ptr(), d.data_ptr(), td.data_ptr(), rows.data_ptr(), target.data_ptr(),
                                          _lib.ptr(xc), B, per, int(w is not None), 0.0 if w is None else w, lo, hi,
                                          _st()), "tdx_distill_guidance_target")
    torch.cuda.synchronize()
    return {"target": target, "x0c": xc}


def _check_pair(tab, t, z, o1, o2, w, lo, hi):
    want = GH.guided_kernels_np(tab.rows.numpy(), t, z, o1, o2, w, lo, hi)
    got = _run_pair(tab, t, z, o1, o2, w, lo, hi)
    what = f"B={z.shape[0]} per={z[0].size} w={w}"
    for k in ("x1c", "x_tilde", "target"):
        assert np.isfinite(want[k]).all()
        _assert_bits(got[k], want[k], f"{k} {what}")
    _assert_bits(got["z_mid"][0], want["z_mid"], f"z_mid {what}")
    _assert_bits(got["z_mid"][1], want["z_mid"], f"second half of z_mid {what}")
    tm = tab.t_mid[torch.from_numpy(np.asarray(t))].tolist()
    assert got["t_mid"][0].tolist() == tm and got["t_mid"][1].tolist() == tm, what
    return want


# ------------------------------------------------------------------ 1. the kernels, bitwise
@pytest.mark.parametrize("N", [4, 256])
@pytest.mark.parametrize("tp,sp", [("eps", "v"), ("v", "eps")])
@pytest.mark.parametrize("bounds", [(-1.0, 1.0), (-INF, INF)])
def test_guided_pair_bitwise(N, tp, sp, bounds):
    """Batch 3 and 5, 8 / 20 / 784 elements per sample (two float4; a row that changes inside a wave; more than one
    block), every w, samples on distinct grid rows - the j = 0 row and t = T - 1 among them."""
    fp = H.forward_process()
    tab = distill_tables(fp, N, tp, sp)
    g = trailing_timesteps(fp, N)
    lo, hi = bounds
    for B in (3, 5):
        t = np.array([g[0], g[-1], g[N // 2], g[1], g[N // 2]][:B])
        for per in (8, 20, 784):
            for w in GH.WS:
                z, o1, o2 = GH.guided_case(np.random.default_rng(N + B + per), tab.rows.numpy(), t, (B, per), w)
                want = _check_pair(tab, t, z, o1, o2, w, lo, hi)
                if hi == 1.0:     # the clamp binds on some elements and not on others
                    for k in ("x1c", "x2c"):
                        assert (np.abs(want[k]) == 1.0).any() and (np.abs(want[k]) < 1.0).any(), (k, B, per, w)
    # x_tilde is optional: the target is the same bits without it
    again = _run_pair(tab, t, z, o1, o2, w, lo, hi, x_tilde=False)
    assert again["x_tilde"] is None
    _assert_bits(again["target"], want["target"], "target without x_tilde")


@pytest.mark.parametrize("tp,sp", [("eps", "v"), ("v", "eps")])
@pytest.mark.parametrize("bounds", [(-1.0, 1.0), (-INF, INF)])
def test_guidance_target_bitwise(tp, sp, bounds):
    """The same sizes, guided at every w and unguided; timesteps 0, T - 1 and three in between."""
    fp = H.forward_process()
    tab = guidance_distill_table(fp, tp, sp)
    lo, hi = bounds
    for B in (3, 5):
        t = np.array([0, T - 1, 500, 1, 250][:B])
        for per in (8, 20, 784):
            for w in (None,) + GH.WS:
                z, o, _ = GH.guided_case(np.random.default_rng(B + per), tab.numpy(), t, (B, per), 1.0 if w is None else w)
                e = o[0] if w is None else GH.cfg_np(o[0], o[1], w)
                want = GH.guidance_target_np(tab.numpy(), t, z, e, lo, hi)
                got = _run_same(tab, t, z, o, w, lo, hi)
                for k in ("x0c", "target"):
                    assert np.isfinite(want[k]).all()
                    _assert_bits(got[k], want[k], f"{k} B={B} per={per} w={w}")
                if hi == 1.0:
                    assert (np.abs(want["x0c"]) == 1.0).any() and (np.abs(want["x0c"]) < 1.0).any(), (B, per, w)
    again = _run_same(tab, t, z, o, w, lo, hi, x0c=False)
    assert again["x0c"] is None
    _assert_bits(again["target"], want["target"], "target without x0c")


def test_kernels_bitwise_past_one_grid():
    """5 x 419 440 elements = 524 300 float4 > 2048 x 256: the last 12 float4 are a second trip of the grid-stride
    loop, in a sample whose row differs from the first trip's."""
    B, per, N, w = 5, 419_440, 4, 3.5
    assert B * per // 4 == 524_300 > 2048 * 256
    fp = H.forward_process()
    tab = distill_tables(fp, N, "eps", "v")
    g = trailing_timesteps(fp, N)
    t = np.array([g[1], g[0], g[3], g[2], g[0]])
    z, o1, o2 = GH.guided_case(np.random.default_rng(11), tab.rows.numpy(), t, (B, per), w)
    _check_pair(tab, t, z, o1, o2, w, -1.0, 1.0)
    tab4 = guidance_distill_table(fp, "eps", "v")
    want = GH.guidance_target_np(tab4.numpy(), t, z, GH.cfg_np(o1[0], o1[1], w), -1.0, 1.0)
    got = _run_same(tab4, t, z, o1, w, -1.0, 1.0)
    for k in ("x0c", "target"):
        _assert_bits(got[k], want[k], k)


# ------------------------------------------------------------------ 2. out_c == out_u: the unguided sibling
@pytest.mark.parametrize("w", GH.WS + (1e30,))
def test_equal_halves_give_the_unguided_bits(w):
    fp = H.forward_process()
    N, B, per = 4, 5, 20
    tab = distill_tables(fp, N, "eps", "v")
    g = trailing_timesteps(fp, N)
    t = np.array([g[0], g[3], g[1], g[2], g[3]])
    z, o1, o2 = GH.guided_case(np.random.default_rng(2), tab.rows.numpy(), t, (B, per), 1.0)
    o1[1], o2[1] = o1[0], o2[0]
    guided, plain = _run_pair(tab, t, z, o1, o2, w, -1.0, 1.0), _run_pair(tab, t, z, o1, o2, None, -1.0, 1.0)
    for k in ("x1c", "x_tilde", "target"):
        assert torch.isfinite(plain[k]).all()
        _assert_bits(guided[k], plain[k], k)
    _assert_bits(guided["z_mid"][0], plain["z_mid"], "z_mid")
    assert guided["t_mid"][0].tolist() == plain["t_mid"].tolist()
    tab4 = guidance_distill_table(fp, "eps", "v")
    a, b = _run_same(tab4, t, z, o1, w, -1.0, 1.0), _run_same(tab4, t, z, o1, None, -1.0, 1.0)
    for k in ("x0c", "target"):
        assert torch.isfinite(b[k]).all()
        _assert_bits(a[k], b[k], f"guidance target {k}")


# ------------------------------------------------------------------ 3. the guided sampler update
def _p_sample_update(x, out, coef, k, lo, hi, w=None, z=None):
    """tdx_p_sample_update in x0 form at row k; w None: n = x.numel(), out of place; else guided and in place on a
    copy of x (2n elements), the first half returned."""
    t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
    if w is None:
        res = torch.full_like(x, POISON)
        check(lib.tdx_p_sample_update(res.data_ptr(), x.data_ptr(), out.data_ptr(), x.numel(), _lib.STEP_X0,
                                      coef.data_ptr(), t_idx.data_ptr(), None, _lib.ptr(z), 0, 0, 0, 0.0, lo, hi, None,
                                      None, None, None, _st()), "tdx_p_sample_update")
        return res
    res = x.clone()
    half = x.numel() // 2
    check(lib.tdx_p_sample_update(res.data_ptr(), res.data_ptr(), out.data_ptr(), half, _lib.STEP_X0, coef.data_ptr(),
                                  t_idx.data_ptr(), None, _lib.ptr(z), 0, 0, 1, w, lo, hi, None, None, None, None, _st()),
          "tdx_p_sample_update")
    assert torch.equal(res[: res.shape[0] // 2], res[res.shape[0] // 2:])
    return res[: res.shape[0] // 2]


@pytest.mark.parametrize("N", [4, 256])
@pytest.mark.parametrize("tp", ["eps", "v"])
def test_guided_z_mid_is_the_guided_samplers_update(N, tp):
    """Every sample on one t: z_mid is the first half of tdx_p_sample_update(form = TDX_STEP_X0, guided = 1, w, no
    noise) on the x0-form table of g_2N at row 2j + 1, bit for bit.  j = 0 and j = N - 1."""
    fp = H.forward_process()
    tab = distill_tables(fp, N, tp, "v")
    g2 = trailing_timesteps(fp, 2 * N)
    coef = ddim_schedule(fp, timesteps=g2, eta=0.0).x0_form(fp, tp, device="cuda")
    for j in (0, N - 1):
        for w in (3.5, -0.5):
            t = np.full(3, g2[2 * j + 1])
            z, o1, o2 = GH.guided_case(np.random.default_rng(j + 3), tab.rows.numpy(), t, (3, 8), w)
            got = _run_pair(tab, t, z, o1, o2, w, -1.0, 1.0)
            want = _p_sample_update(_dev(np.concatenate([z, z])), _dev(o1.reshape(6, 8)), coef, 2 * j + 1, -1.0, 1.0, w)
            torch.cuda.synchronize()
            assert (got["x1c"].abs() == 1).any() and (got["x1c"].abs() < 1).any()
            _assert_bits(got["z_mid"][0], want, f"z_mid at j = {j}, w = {w}")


# ------------------------------------------------------------------ 4. the defining properties
@pytest.mark.parametrize("sp", ["v", "eps"])
@pytest.mark.parametrize("tp", ["eps", "v"])
def test_one_student_step_with_the_guided_target_lands_on_the_teachers_guided_z_end(sp, tp):
    """(a) The guided target, fed as the student's output into the UNGUIDED x0-form update on the student's row (grid
    g_N), gives the teacher's guided z_end.  Reference: z_end in fp64 from the unrounded tables and the fp64
    combinations.  Bound: the guided target's chain (n = 14), the update's 4 more, and one rounding for each of the 7
    fp32 table entries along the longest path (p1, A1, p2, W2, G, q_s, A_s) as in test_gpu_distill: n = 25, on the S of
    the student's expanded update."""
    N, w = 4, 3.5
    fp = H.forward_process()
    tab = distill_tables(fp, N, tp, sp)
    rows64 = distill_tables(fp, N, tp, sp, dtype=torch.float64).rows.numpy()
    g = trailing_timesteps(fp, N)
    form = ddim_schedule(fp, timesteps=g, eta=0.0).x0_form(fp, sp)
    coef = form.cuda()
    n = GH.N_TARGET_G + 4 + 7
    for j in range(N):
        t = np.full(2, g[j])
        z, o1, o2 = GH.guided_case(np.random.default_rng(40 + j), tab.rows.numpy(), t, (2, 8), w)
        got = _run_pair(tab, t, z, o1, o2, w, -1.0, 1.0)
        landed = _p_sample_update(_dev(z), got["target"], coef, j, -1.0, 1.0)
        torch.cuda.synchronize()
        want = GH.guided_kernels_np(rows64, t, *(v.astype(np.float64) for v in (z, o1, o2)), w, -1.0, 1.0)["z_end"]
        _, S_target, _ = GH.guided_magnitudes(tab.rows.numpy(), t, z, o1, o2, w)
        p_s, q_s, A_s, B_s = (abs(float(form[j, c])) for c in range(4))
        az = np.abs(z.astype(np.float64))
        S = A_s * (p_s * az + q_s * S_target) + B_s * az
        err = np.abs(landed.cpu().numpy().astype(np.float64) - want)
        share = (err / (n * GH.U * S)).max()
        print(f"teacher {tp} student {sp} j={j}: max |student step - guided z_end| = {err.max():.3e}, "
              f"largest share of the bound {share:.3f}")
        assert (err <= n * GH.U * S).all(), (j, share)


@pytest.mark.parametrize("sp", ["v", "eps"])
@pytest.mark.parametrize("tp", ["eps", "v"])
def test_one_student_step_with_the_guidance_target_is_the_teachers_guided_step(sp, tp):
    """(b) tdx_distill_guidance_target's target, fed as the student's output into the UNGUIDED x0-form update on the
    student's row of the DDPM chain, lands where the GUIDED update of the teacher's two outputs on the teacher's row
    does, under the same noise and the same clamp.  Reference: the guided update in fp64 from the unrounded table.
    Student: the guided target's chain (n = 8), the update's 5 (product, sum, product, sum, noise sum) and one rounding
    for each of the 4 table entries along the longest path (p, G, q_s, A_s): n = 17, on the S of the student's expanded
    update.  Teacher: combination 3, x0 2, update 3, plus 1 as everywhere, and the entries q, A: n = 11 on its own S.
    The two device results differ by no more than the sum of the two bounds."""
    w = 3.5
    fp = H.forward_process()
    tab = guidance_distill_table(fp, tp, sp)
    sched = ddpm_schedule(fp)
    form_t, form_s = sched.x0_form(fp, tp), sched.x0_form(fp, sp)
    form_t64 = sched.x0_form(fp, tp, dtype=torch.float64).numpy()
    n_s, n_t = GH.N_SAME_G + 5 + 4, GH.N_CFG + 2 + 3 + 1 + 2
    for k in (1, 500, T - 1):
        t = np.full(2, k)
        rng = np.random.default_rng(60 + k)
        z, o, _ = GH.guided_case(rng, tab.numpy(), t, (2, 8), w)
        noise = rng.standard_normal((2, 8)).astype(np.float32)
        got = _run_same(tab, t, z, o, w, -1.0, 1.0)
        assert (got["x0c"].abs() == 1).any() and (got["x0c"].abs() < 1).any()
        student = _p_sample_update(_dev(z), got["target"], form_s.cuda(), k, -1.0, 1.0, z=_dev(noise))
        teacher = _p_sample_update(_dev(np.concatenate([z, z])), _dev(o.reshape(4, 8)), form_t.cuda(), k, -1.0, 1.0, w,
                                   z=_dev(noise))
        torch.cuda.synchronize()
        z64, o64, nz = z.astype(np.float64), o.astype(np.float64), np.abs(noise.astype(np.float64))
        p, q, A, Bx, sg = form_t64[k]
        want = A * np.clip(p * z64 + q * GH.cfg_np(o64[0], o64[1], w), -1.0, 1.0) + Bx * z64 + sg * noise
        az = np.abs(z64)
        p_s, q_s, A_s, B_s, sg_s = (abs(float(form_s[k, c])) for c in range(5))
        S_s = A_s * (p_s * az + q_s * GH.guidance_magnitude(tab.numpy(), t, z, GH.cfg_mag(o[0], o[1], w))) + B_s * az \
            + sg_s * nz
        S_t = abs(A) * (abs(p) * az + abs(q) * GH.cfg_mag(o[0], o[1], w)) + abs(Bx) * az + abs(sg) * nz
        err_s = np.abs(student.cpu().numpy().astype(np.float64) - want)
        err_t = np.abs(teacher.cpu().numpy().astype(np.float64) - want)
        both = np.abs(student.cpu().numpy().astype(np.float64) - teacher.cpu().numpy().astype(np.float64))
        print(f"teacher {tp} student {sp} t={k}: student {err_s.max():.3e} (share {(err_s / (n_s * GH.U * S_s)).max():.3f})"
              f", teacher {err_t.max():.3e} (share {(err_t / (n_t * GH.U * S_t)).max():.3f}), apart {both.max():.3e}")
        assert (err_s <= n_s * GH.U * S_s).all() and (err_t <= n_t * GH.U * S_t).all()
        assert (both <= GH.U * (n_s * S_s + n_t * S_t)).all()


# ------------------------------------------------------------------ 5. bad arguments
def test_bad_arguments_write_nothing():
    fp = H.forward_process()
    tab = distill_tables(fp, 4, "eps", "v")
    rows, tmt, rows4 = tab.rows.cuda(), tab.t_mid.cuda(), guidance_distill_table(fp, "eps", "v").cuda()
    B, per = 3, 8
    f = lambda k=1: torch.full((k * B, per), 7.0, device="cuda")  # noqa: E731
    z, x1, tg, xt = (f() for _ in range(4))
    o, zm = f(2), f(2)
    t = torch.full((B,), T - 1, dtype=torch.int64, device="cuda")
    tm = torch.full((2 * B,), -7, dtype=torch.int64, device="cuda")
    a1 = [z.data_ptr(), o.data_ptr(), t.data_ptr(), rows.data_ptr(), tmt.data_ptr(), zm.data_ptr(), x1.data_ptr(),
          tm.data_ptr()]
    a2 = [z.data_ptr(), zm.data_ptr(), o.data_ptr(), x1.data_ptr(), t.data_ptr(), rows.data_ptr(), tg.data_ptr(),
          xt.data_ptr()]
    a3 = [z.data_ptr(), o.data_ptr(), t.data_ptr(), rows4.data_ptr(), tg.data_ptr(), xt.data_ptr()]
    pair = lambda fn: (lambda ptrs, b, p, w, lo, hi: fn(*ptrs, b, p, w, lo, hi, _st()))  # noqa: E731
    same = lambda g: (lambda ptrs, b, p, w, lo, hi: lib.tdx_distill_guidance_target(*ptrs, b, p, g, w, lo, hi, _st()))  # noqa: E731
    entries = (("teacher_step_guided", pair(lib.tdx_distill_teacher_step_guided), a1, ()),
               ("target_guided", pair(lib.tdx_distill_target_guided), a2, (7,)),
               ("guidance_target guided", same(1), a3, (5,)),
               ("guidance_target unguided", same(0), a3, (5,)))
    for name, fn, args, nullable in entries:
        for i in range(len(args)):
            if i in nullable:
                continue
            bad = list(args)
            bad[i] = None
            assert fn(bad, B, per, 3.0, -1.0, 1.0) == TDX_E_BADARG, (name, i)
        for batch, p in ((0, per), (-1, per), (B, 0), (B, -4), (B, 6), (B, 7)):
            assert fn(args, batch, p, 3.0, -1.0, 1.0) == TDX_E_BADARG, (name, batch, p)
        for lo, hi in ((1.0, -1.0), (0.5, 0.5), (float("nan"), 1.0), (-1.0, float("nan")), (INF, INF)):
            assert fn(args, B, per, 3.0, lo, hi) == TDX_E_BADARG, (name, lo, hi)
        if name != "guidance_target unguided":          # without guidance w is not read
            for w in (INF, -INF, float("nan")):
                assert fn(args, B, per, w, -1.0, 1.0) == TDX_E_BADARG, (name, w)
    torch.cuda.synchronize()
    for buf in (z, o, zm, x1, tg, xt):
        assert torch.equal(buf, torch.full_like(buf, 7.0))
    assert (tm == -7).all()
    # and the same arguments, valid, do write (the calls above were refused for their one bad argument)
    assert entries[0][1](a1, B, per, 3.0, -INF, INF) == 0
    assert entries[1][1](a2, B, per, 3.0, -INF, INF) == 0
    torch.cuda.synchronize()
    assert (tm == int(tab.t_mid[T - 1])).all() and not torch.equal(tg, torch.full_like(tg, 7.0))
    assert not (zm == 7.0).any()
    tg.fill_(7.0)
    assert entries[3][1](a3, B, per, INF, -INF, INF) == 0
    torch.cuda.synchronize()
    assert not (tg == 7.0).any()


# ------------------------------------------------------------------ 6. the steps are the hand-issued launches
SHAPES = {"cond": (1, 28, 28), "laion": (4, 32, 32)}


def _model(kind, seed):
    if kind == "cond":
        from tiny_diffusion_amd.conditional_diffusion import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict(seed, True), strict=True)
    else:
        from tiny_diffusion_amd.conditional_diffusion_laion import NoiseModel
        m = NoiseModel(time_dim=768)
        m.load_state_dict(make_state_dict_laion(seed), strict=True)
    return m.cuda()


def _batch(kind, B, seed, ts):
    g = torch.Generator().manual_seed(seed)
    x0 = (torch.rand(B, *SHAPES[kind], generator=g) * 2 - 1).cuda()
    noise = torch.randn(B, *SHAPES[kind], generator=g).cuda()
    t = torch.tensor([ts[i % len(ts)] for i in (0, len(ts) - 1, 1, 2)][:B], dtype=torch.int64).cuda()
    y = (torch.randn(B, 768, generator=g) if kind == "laion" else torch.randint(0, 10, (B,), generator=g)).cuda()
    return x0, noise, t, y


def _dropped(kind, y, prob):
    """(seed, y after dropout) for the first seed whose Philox mask at step 0 drops some rows and keeps others."""
    from tiny_diffusion_amd.unet import KIND_LAION, KIND_MNIST, _cond_tensor

    yc = _cond_tensor(KIND_LAION if kind == "laion" else KIND_MNIST, y)
    for seed in range(64):
        out = torch.empty_like(yc)
        if kind == "laion":
            check(lib.tdx_cond_drop_rows(yc.data_ptr(), out.data_ptr(), yc.shape[0], yc.shape[1], prob, seed, 0, _st()))
            gone = (out == 0).all(dim=1)
        else:
            check(lib.tdx_cond_drop_labels(yc.data_ptr(), out.data_ptr(), yc.shape[0], prob, seed, 0, _st()))
            gone = out < 0
        if bool(gone.any()) and not bool(gone.all()):
            return seed, out
    raise AssertionError("no seed with a mixed mask")


def _loss_launch(out, target, t, w_dev):
    """The step's own loss launch, by hand: ``tdx_mse_loss_grad_weighted`` on the (T,) device table ``w_dev``, or
    ``tdx_mse_loss_grad`` when there is none, with a scratch of its own.  ``(loss, d_out)``."""
    B = out.shape[0]
    loss = torch.zeros(1, dtype=torch.float32, device="cuda")
    d_out = torch.full_like(out, POISON)
    scratch = torch.empty(lib.tdx_mse_scratch_bytes(), dtype=torch.uint8, device="cuda")
    if w_dev is None:
        check(lib.tdx_mse_loss_grad(out.data_ptr(), target.data_ptr(), loss.data_ptr(), d_out.data_ptr(), 1.0,
                                    out.numel(), scratch.data_ptr(), _st()), "tdx_mse_loss_grad")
    else:
        check(lib.tdx_mse_loss_grad_weighted(out.data_ptr(), target.data_ptr(), t.data_ptr(), w_dev.data_ptr(),
                                             loss.data_ptr(), d_out.data_ptr(), 1.0, B, out.numel() // B,
                                             scratch.data_ptr(), _st()), "tdx_mse_loss_grad_weighted")
    return loss, d_out


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("kind,B", [("cond", 4), ("laion", 2)])
@pytest.mark.parametrize("which", ["DistillStep", "GuidanceDistillStep"])
def test_guided_step_is_the_hand_issued_launches(which, kind, B, drop):
    """The step's gradient and loss against the same launches issued by hand on a second, identical student: the
    teacher's inference forward(s) at 2B rows around the new entries, the student's training forward at B rows, the
    step's own loss launch (``tdx_mse_loss_grad_weighted`` on the same table), the existing backward on its ``d_out`` -
    flat gradient, loss and target expected bit-equal.  The teacher is left exactly as it was, and a second step of
    the same shapes allocates no second set of buffers."""
    from tiny_diffusion_amd.train import DistillStep, GuidanceDistillStep
    from tiny_diffusion_amd.unet import MODE_INFER, MODE_TRAIN, _cond_tensor, _with_null_cond

    N, w = 4, 3.0
    fp = H.forward_process()
    two_step = which == "DistillStep"
    ts = trailing_timesteps(fp, N) if two_step else [0, 333, 666, T - 1]
    x0, noise, t, y = _batch(kind, B, 31, ts)
    m1, m2 = _model(kind, 3).train(), _model(kind, 3).train()
    teacher = _model(kind, 5).train()          # the step puts it in eval()
    before = {k: v.detach().clone() for k, v in teacher.state_dict().items()}
    w_tab = truncated_snr_weights(fp, "v")
    kw = dict(teacher_prediction="eps", prediction="v", clip_denoised=True, loss_weighting=w_tab, keep_target=True,
              lr=1e-3)
    y_seen = y
    if drop:
        seed, y_seen = _dropped(kind, y, 0.5)
        kw.update(cond_drop_prob=0.5, cond_drop_seed=seed)
    step = DistillStep(m1, teacher, fp, N, guidance_scale=w, **kw) if two_step \
        else GuidanceDistillStep(m1, teacher, fp, w, **kw)
    assert not teacher.training and m1.training and step.guidance_scale == w
    loss = step.step(x0, y, t=t, noise=noise).clone()
    grad1 = step.flat_grad.clone()

    mk = m1._arch.kind
    z_t, _ = fp.q_sample("cuda", x0, t, noise=noise)
    per = z_t.numel() // B
    z2, t2 = torch.cat([z_t, z_t]), torch.cat([t, t])
    y2 = _with_null_cond(mk, _cond_tensor(mk, y_seen))
    target = torch.empty_like(z_t)
    out1 = teacher._run_forward(z2, t2, y2, mode=MODE_INFER)[0]
    assert out1.shape[0] == 2 * B
    if two_step:
        tab = distill_tables(fp, N, "eps", "v")
        rows, tmt = tab.rows.cuda(), tab.t_mid.cuda()
        z_mid, x1c, t_mid = torch.empty_like(z2), torch.empty_like(z_t), torch.empty_like(t2)
        check(lib.tdx_distill_teacher_step_guided(z_t.data_ptr(), out1.data_ptr(), t.data_ptr(), rows.data_ptr(),
                                                  tmt.data_ptr(), z_mid.data_ptr(), x1c.data_ptr(), t_mid.data_ptr(), B,
                                                  per, w, -1.0, 1.0, _st()), "tdx_distill_teacher_step_guided")
        out2 = teacher._run_forward(z_mid, t_mid, y2, mode=MODE_INFER)[0]
        check(lib.tdx_distill_target_guided(z_t.data_ptr(), z_mid.data_ptr(), out2.data_ptr(), x1c.data_ptr(),
                                            t.data_ptr(), rows.data_ptr(), target.data_ptr(), None, B, per, w, -1.0, 1.0,
                                            _st()), "tdx_distill_target_guided")
        assert t_mid.tolist() == 2 * tab.t_mid[t.cpu()].tolist() and torch.equal(z_mid[:B], z_mid[B:])
    else:
        rows4 = guidance_distill_table(fp, "eps", "v").cuda()
        check(lib.tdx_distill_guidance_target(z_t.data_ptr(), out1.data_ptr(), t.data_ptr(), rows4.data_ptr(),
                                              target.data_ptr(), None, B, per, 1, w, -1.0, 1.0, _st()),
              "tdx_distill_guidance_target")
    out, plan, _ = m2._run_forward(z_t, t, y_seen, mode=MODE_TRAIN)
    n = out.numel()
    loss2, d_out = _loss_launch(out, target, t, w_tab.cuda())         # the step's loss launch on the same table
    flat2, views2 = m2._grad_buffers(torch.device("cuda", torch.cuda.current_device()))
    m2._run_backward(plan, d_out, views2)
    torch.cuda.synchronize()
    assert torch.isfinite(target).all() and torch.isfinite(grad1).all() and grad1.abs().max() > 0
    _assert_bits(step.last_target, target, "last_target")
    diff = (grad1 - flat2).abs().max().item()
    print(f"{which} {kind} B={B} drop={drop}: max |grad - hand-issued grad| = {diff:.3e}, loss {loss.item():.9g} "
          f"against hand-issued {loss2.item():.9g}")
    assert torch.equal(grad1, flat2), diff
    assert torch.isfinite(loss).all() and loss.item() > 0
    _assert_bits(loss, loss2, "loss")
    # and the launch computes the weighted mean squared error (a coarse check of the reference itself, in fp64)
    bshape = (B,) + (1,) * (out.dim() - 1)
    want = (w_tab.cuda()[t].double().view(bshape) * (out.double() - target.double()) ** 2).sum().item() / n
    assert abs(loss2.item() - want) <= 1e-6 * want
    after = teacher.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    # one set of 2B-row buffers per input shape, reused by the next step
    def buffer_sets():
        sets = [step._gbufs] + ([step._dbufs] if two_step else [])
        assert all(len(s) == 1 for s in sets)
        return [b.data_ptr() for s in sets for bufs in s.values() for b in bufs]

    held = buffer_sets()
    assert [tuple(b.shape) for b in step._gbufs[tuple(z_t.shape)]] == [(2 * B,) + tuple(z_t.shape[1:]), (2 * B,)]
    step.keep_target = False
    step.step(x0, y, t=t, noise=noise)
    assert step.last_target is None
    assert buffer_sets() == held
    # a guided step without a condition is refused
    with pytest.raises(ValueError, match="condition"):
        step.step(x0, None, t=t, noise=noise)


def test_reparameterisation_step_without_guidance_is_the_hand_issued_launches():
    """``GuidanceDistillStep(guidance_scale=None)``: the teacher at B rows, guided = 0 - target, loss and gradient
    bit-equal to the launches by hand (the unweighted ``tdx_mse_loss_grad``); no 2B-row buffer is allocated."""
    from tiny_diffusion_amd.train import GuidanceDistillStep
    from tiny_diffusion_amd.unet import MODE_INFER, MODE_TRAIN

    fp = H.forward_process()
    B = 4
    x0, noise, t, y = _batch("cond", B, 8, [0, 333, 666, T - 1])
    m1, m2, teacher = _model("cond", 3).train(), _model("cond", 3).train(), _model("cond", 5)
    step = GuidanceDistillStep(m1, teacher, fp, None, teacher_prediction="eps", prediction="v", clip_denoised=True,
                               keep_target=True, lr=1e-3)
    loss = step.step(x0, y, t=t, noise=noise).clone()
    z_t, _ = fp.q_sample("cuda", x0, t, noise=noise)
    out1 = teacher._run_forward(z_t, t, y, mode=MODE_INFER)[0]
    target = torch.empty_like(z_t)
    check(lib.tdx_distill_guidance_target(z_t.data_ptr(), out1.data_ptr(), t.data_ptr(),
                                          guidance_distill_table(fp, "eps", "v").cuda().data_ptr(), target.data_ptr(),
                                          None, B, 784, 0, 0.0, -1.0, 1.0, _st()), "tdx_distill_guidance_target")
    out, plan, _ = m2._run_forward(z_t, t, y, mode=MODE_TRAIN)
    loss2, d_out = _loss_launch(out, target, t, None)                 # unweighted: the plain loss entry
    flat2, views2 = m2._grad_buffers(torch.device("cuda", torch.cuda.current_device()))
    m2._run_backward(plan, d_out, views2)
    torch.cuda.synchronize()
    _assert_bits(step.last_target, target, "last_target")
    assert torch.equal(step.flat_grad, flat2) and not step._gbufs
    assert torch.isfinite(loss).all() and loss.item() > 0
    _assert_bits(loss, loss2, "loss")
    step.set_objective("eps")                  # the table follows the student's prediction
    assert torch.equal(step._rows.cpu(), guidance_distill_table(fp, "eps", "eps"))


# ------------------------------------------------------------------ 7. the adaptive timestep sampler
def test_guidance_distill_step_under_the_loss_second_moment_sampler():
    """T = 8, one loss per term: two steps with explicit t cover every timestep, so the history is full and the third
    step draws its own t from it."""
    from tiny_diffusion_amd.train import GuidanceDistillStep

    fp = ForwardProcess(num_timesteps=8)
    B = 4
    x0, _, _, y = _batch("cond", B, 12, [0])
    step = GuidanceDistillStep(_model("cond", 3).train(), _model("cond", 5), fp, 3.0, clip_denoised=True, lr=1e-4,
                               timestep_sampler="loss_second_moment", history_per_term=1, philox_seed=5, timestep_seed=6)
    for lo in (0, 4):
        step.step(x0, y, t=torch.arange(lo, lo + 4, device="cuda"))
    state = step.timestep_sampler_state()
    assert (state["counts"] >= 1).all() and (state["history"] > 0).all() and torch.isfinite(state["history"]).all()
    step.step(x0, y)
    torch.cuda.synchronize()
    assert step.last_t.shape == (B,) and bool(((step.last_t >= 0) & (step.last_t < 8)).all())
    assert step.sample_losses.shape == (B,) and torch.isfinite(step.sample_losses).all() and torch.isfinite(step.loss).all()


# ------------------------------------------------------------------ 8. it learns
def test_thirty_guidance_distillation_steps_lower_the_loss():
    """30 steps at B = 4 on synthetic data, conditional MNIST UNet, w = 3, eps -> v, clamp on, Philox noise, student
    initialised from the teacher, fixed seeds: the mean loss of the last 5 steps is below that of the first 5.  Measured
    on an MI355X: see DESIGN.md 3.22.  No tighter number is asserted."""
    from tiny_diffusion_amd.train import GuidanceDistillStep

    fp = H.forward_process()
    B = 4
    g = torch.Generator().manual_seed(4)
    x0 = (torch.rand(B, 1, 28, 28, generator=g) * 2 - 1).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    teacher, student = _model("cond", 5), _model("cond", 0).train()
    student.load_state_dict(teacher.state_dict())
    step = GuidanceDistillStep(student, teacher, fp, 3.0, teacher_prediction="eps", prediction="v", clip_denoised=True,
                               lr=1e-3, philox_seed=21, timestep_sampler=torch.ones(T), timestep_seed=22)
    losses = [step.step(x0, y).clone() for _ in range(30)]
    torch.cuda.synchronize()
    losses = [v.item() for v in losses]
    first, last = sum(losses[:5]) / 5, sum(losses[-5:]) / 5
    print(f"loss, first 5 steps {first:.5f}, last 5 steps {last:.5f}")
    assert all(math.isfinite(v) for v in losses)
    assert last < first, (first, last)
    # and the student is sampled WITHOUT guidance by the unchanged sampler
    from tiny_diffusion_amd.conditional_diffusion import ddim_sample
    x = ddim_sample(student, fp, "cuda", 4, y[:4], steps=4, prediction="v", clip_denoised=True)
    assert x.shape == (4, 1, 28, 28) and torch.isfinite(x).all() and x.abs().max().item() <= 1.0
