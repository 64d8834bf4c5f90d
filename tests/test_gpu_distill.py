"""Progressive distillation on the device: ``tdx_distill_teacher_step`` / ``tdx_distill_target``
bit for bit against the fp32 restatement of tests/distill_helpers.py, against the sampler's own x0-form update, and
against the property that defines the target; ``DistillStep`` against the same launches issued by hand, its timestep
draws, the plain ``TrainStep`` beside it, and one short learning check.

The bitwise comparisons hold because the build has fp contraction off and every product / sum of the two kernels is
rounded on its own: a numpy fp32 expression with one operation per rounding is the same arithmetic."""
import gc
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import distill_helpers as H  # noqa: E402
from oracle.weights import make_state_dict, make_state_dict_laion, make_state_dict_latent  # noqa: E402

from tiny_diffusion_amd import _lib  # noqa: E402
from tiny_diffusion_amd._lib import check, lib  # noqa: E402
from tiny_diffusion_amd.schedule import (ddim_schedule, distill_tables, trailing_timesteps,  # noqa: E402
                                         truncated_snr_weights)

TDX_E_BADARG = -1
T = 1000
INF = math.inf


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if dtype is None else torch.tensor(a, dtype=dtype).cuda()


def _run_kernels(tab, t, z, o1, o2, lo, hi, x_tilde=True):
    """Both entries on numpy inputs; the outputs start as NaN / -7 so that an element left unwritten shows."""
    rows, t_mid_table = tab.rows.cuda(), tab.t_mid.cuda()
    B, per = z.shape[0], z[0].size
    zt, d1, d2, td = _dev(z), _dev(o1), _dev(o2), _dev(t, torch.int64)
    z_mid, x1c, target = (torch.full_like(zt, float("nan")) for _ in range(3))
    xt = torch.full_like(zt, float("nan")) if x_tilde else None
    t_mid = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    check(lib.tdx_distill_teacher_step(zt.data_ptr(), d1.data_ptr(), td.data_ptr(), rows.data_ptr(),
                                       t_mid_table.data_ptr(), z_mid.data_ptr(), x1c.data_ptr(), t_mid.data_ptr(), B,
                                       per, lo, hi, _st()), "tdx_distill_teacher_step")
    check(lib.tdx_distill_target(zt.data_ptr(), z_mid.data_ptr(), d2.data_ptr(), x1c.data_ptr(), td.data_ptr(),
                                 rows.data_ptr(), target.data_ptr(), _lib.ptr(xt), B, per, lo, hi, _st()),
          "tdx_distill_target")
    torch.cuda.synchronize()
    return {"z_mid": z_mid, "x1c": x1c, "target": target, "x_tilde": xt, "t_mid": t_mid}


def _assert_bits(got, want, what):
    g, w = H.bits(got), H.bits(want)
    assert g.shape == w.shape, what
    bad = int((g != w).sum())
    assert bad == 0, f"{what}: {bad} of {g.size} elements differ in their bits"


# ------------------------------------------------------------------ 1. the kernels, bitwise
@pytest.mark.parametrize("N", [4, 256])
@pytest.mark.parametrize("tp,sp", [("eps", "v"), ("v", "eps")])
@pytest.mark.parametrize("bounds", [(-1.0, 1.0), (-INF, INF)])
def test_kernels_bitwise(N, tp, sp, bounds):
    """batch 3 x 8 elements: two float4 per sample, every sample on its own grid row - the j = 0 row, t = T - 1 and one
    in between."""
    fp = H.forward_process()
    tab = distill_tables(fp, N, tp, sp)
    g = trailing_timesteps(fp, N)
    t = np.array([g[0], g[-1], g[N // 2]])
    assert g[-1] == T - 1 and len(set(t.tolist())) == 3
    z, o1, o2 = H.clamp_case(np.random.default_rng(7 * N), tab.rows.numpy(), t, (3, 8))
    lo, hi = bounds
    want = H.kernels_np(tab.rows.numpy(), t, z, o1, o2, lo, hi)
    if hi == 1.0:      # the clamp binds on some elements and not on others, in both teacher predictions
        for k in ("x1c", "x2c"):
            assert (np.abs(want[k]) == 1.0).any() and (np.abs(want[k]) < 1.0).any(), k
    else:
        unclamped = H.kernels_np(tab.rows.numpy(), t, z, o1, o2, -1.0, 1.0)
        assert not np.array_equal(unclamped["target"], want["target"])
    got = _run_kernels(tab, t, z, o1, o2, lo, hi)
    for k in ("x1c", "z_mid", "x_tilde", "target"):
        assert np.isfinite(want[k]).all()
        _assert_bits(got[k], want[k], k)
    mid_of = {tr[0]: tr[1] for tr in H.student_triples(fp, N)}
    assert got["t_mid"].tolist() == [mid_of[int(v)] for v in t] == tab.t_mid[torch.from_numpy(t)].tolist()
    # x_tilde is optional: the target is the same bits without it
    again = _run_kernels(tab, t, z, o1, o2, lo, hi, x_tilde=False)
    assert again["x_tilde"] is None
    _assert_bits(again["target"], want["target"], "target without x_tilde")


# ------------------------------------------------------------------ 2. the second grid-stride trip
def test_kernels_bitwise_past_one_grid():
    """5 x 419 440 elements = 524 300 float4 > 2048 x 256: the last 12 float4 are a second trip of the grid-stride
    loop, in a sample whose row differs from the first trip's."""
    B, per, N = 5, 419_440, 4
    assert B * per // 4 == 524_300 > 2048 * 256
    fp = H.forward_process()
    tab = distill_tables(fp, N, "eps", "v")
    g = trailing_timesteps(fp, N)
    t = np.array([g[1], g[0], g[3], g[2], g[0]])
    z, o1, o2 = H.clamp_case(np.random.default_rng(11), tab.rows.numpy(), t, (B, per))
    want = H.kernels_np(tab.rows.numpy(), t, z, o1, o2, -1.0, 1.0)
    got = _run_kernels(tab, t, z, o1, o2, -1.0, 1.0)
    for k in ("x1c", "z_mid", "x_tilde", "target"):
        _assert_bits(got[k], want[k], k)
    assert got["t_mid"].tolist() == tab.t_mid[torch.from_numpy(t)].tolist()


# ------------------------------------------------------------------ 3. the sampler's own update
def _p_sample_update(x, out, coef, k, lo, hi):
    """tdx_p_sample_update in x0 form at row k, no noise, out of place."""
    res = torch.full_like(x, float("nan"))
    t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
    check(lib.tdx_p_sample_update(res.data_ptr(), x.data_ptr(), out.data_ptr(), x.numel(), _lib.STEP_X0, coef.data_ptr(),
                                  t_idx.data_ptr(), None, None, 0, 0, 0, 0.0, lo, hi, None, None, None, None, _st()),
          "tdx_p_sample_update")
    return res


@pytest.mark.parametrize("N", [4, 256])
@pytest.mark.parametrize("tp", ["eps", "v"])
def test_z_mid_is_the_samplers_x0_form_update(N, tp):
    """Every sample on the same t: z_mid is tdx_p_sample_update(form=TDX_STEP_X0) on the x0-form table of g_2N at row
    2j + 1, bit for bit - the teacher's step IS the sampler's step.  j = 0 and j = N - 1."""
    fp = H.forward_process()
    tab = distill_tables(fp, N, tp, "v")
    g2 = trailing_timesteps(fp, 2 * N)
    coef = ddim_schedule(fp, timesteps=g2, eta=0.0).x0_form(fp, tp, device="cuda")
    for j in (0, N - 1):
        t = np.full(3, g2[2 * j + 1])
        z, o1, o2 = H.clamp_case(np.random.default_rng(j + 3), tab.rows.numpy(), t, (3, 8))
        got = _run_kernels(tab, t, z, o1, o2, -1.0, 1.0)
        want = _p_sample_update(_dev(z), _dev(o1), coef, 2 * j + 1, -1.0, 1.0)
        torch.cuda.synchronize()
        assert (got["x1c"].abs() == 1).any() and (got["x1c"].abs() < 1).any()
        _assert_bits(got["z_mid"], want, f"z_mid at j = {j}")
        # and the teacher's second step, from the same entry at row 2j, is where the student has to land
        z_end = _p_sample_update(got["z_mid"], _dev(o2), coef, 2 * j, -1.0, 1.0)
        torch.cuda.synchronize()
        ref = H.kernels_np(tab.rows.numpy(), t, z, o1, o2, -1.0, 1.0)["z_end"]
        assert np.array_equal(z_end.cpu().numpy(), ref)      # (== : a -0 + 0 of the sampler's absent noise term is +0)


# ------------------------------------------------------------------ 4. the defining property
@pytest.mark.parametrize("sp", ["v", "eps"])
@pytest.mark.parametrize("tp", ["eps", "v"])
def test_one_student_step_with_the_target_lands_on_the_teachers_z_end(sp, tp):
    """The target, fed as the student's output into the sampler's x0-form update on the student's own row (grid g_N),
    gives the teacher's z_end.  Reference: z_end in fp64 from the UNROUNDED tables.  Bound (distill_helpers, 3.): the
    target's chain of 11 roundings, the update's 4 more (product, sum, product, sum), and one rounding for each of the
    7 fp32 table entries that multiply along the longest path (p1, A1, p2, W2, G, q_s, A_s) - the identity holds for the
    exact entries, the device reads their fp32 roundings: n = 22, on the S of the student's expanded update.  The
    student's clamp is the identity on the exact x~ (a convex combination of clamped values) and 1-Lipschitz."""
    N = 4
    fp = H.forward_process()
    tab = distill_tables(fp, N, tp, sp)
    rows64 = distill_tables(fp, N, tp, sp, dtype=torch.float64).rows.numpy()
    g = trailing_timesteps(fp, N)
    form = ddim_schedule(fp, timesteps=g, eta=0.0).x0_form(fp, sp)
    coef = form.cuda()
    n = H.N_TARGET + 4 + 7
    for j in range(N):
        t = np.full(2, g[j])
        z, o1, o2 = H.clamp_case(np.random.default_rng(40 + j), tab.rows.numpy(), t, (2, 8))
        got = _run_kernels(tab, t, z, o1, o2, -1.0, 1.0)
        landed = _p_sample_update(_dev(z), got["target"], coef, j, -1.0, 1.0)
        torch.cuda.synchronize()
        want = H.kernels_np(rows64, t, *(v.astype(np.float64) for v in (z, o1, o2)), -1.0, 1.0)["z_end"]
        _, S_target, _ = H.magnitudes(tab.rows.numpy(), t, z, o1, o2)
        p_s, q_s, A_s, B_s = (abs(float(form[j, c])) for c in range(4))
        S = A_s * (p_s * np.abs(z.astype(np.float64)) + q_s * S_target) + B_s * np.abs(z.astype(np.float64))
        err = np.abs(landed.cpu().numpy().astype(np.float64) - want)
        share = (err / (n * H.U * S)).max()
        print(f"teacher {tp} student {sp} j={j}: max |student step - z_end| = {err.max():.3e}, "
              f"largest share of the bound {share:.3f}")
        assert (err <= n * H.U * S).all(), (j, share)


# ------------------------------------------------------------------ 5. bad arguments
def test_bad_arguments_write_nothing():
    fp = H.forward_process()
    tab = distill_tables(fp, 4, "eps", "v")
    rows, tmt = tab.rows.cuda(), tab.t_mid.cuda()
    B, per = 3, 8
    f = lambda: torch.full((B, per), 7.0, device="cuda")  # noqa: E731
    z, o, zm, x1, tg, xt = (f() for _ in range(6))
    t = torch.full((B,), T - 1, dtype=torch.int64, device="cuda")
    tm = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    a1 = [z.data_ptr(), o.data_ptr(), t.data_ptr(), rows.data_ptr(), tmt.data_ptr(), zm.data_ptr(), x1.data_ptr(),
          tm.data_ptr()]
    a2 = [z.data_ptr(), zm.data_ptr(), o.data_ptr(), x1.data_ptr(), t.data_ptr(), rows.data_ptr(), tg.data_ptr(),
          xt.data_ptr()]
    for fn, args, nullable in ((lib.tdx_distill_teacher_step, a1, ()), (lib.tdx_distill_target, a2, (7,))):
        for i in range(8):
            if i in nullable:
                continue
            bad = list(args)
            bad[i] = None
            assert fn(*bad, B, per, -1.0, 1.0, _st()) == TDX_E_BADARG, (fn, i)
        for batch, p in ((0, per), (-1, per), (B, 0), (B, -4), (B, 6), (B, 7)):
            assert fn(*args, batch, p, -1.0, 1.0, _st()) == TDX_E_BADARG, (batch, p)
        for lo, hi in ((1.0, -1.0), (0.5, 0.5), (float("nan"), 1.0), (-1.0, float("nan")), (INF, INF)):
            assert fn(*args, B, per, lo, hi, _st()) == TDX_E_BADARG, (lo, hi)
    torch.cuda.synchronize()
    for buf in (z, o, zm, x1, tg, xt):
        assert torch.equal(buf, torch.full_like(buf, 7.0))
    assert (tm == -7).all()
    # and the same arguments, valid, do write (the calls above were refused for their one bad argument)
    assert lib.tdx_distill_teacher_step(*a1, B, per, -INF, INF, _st()) == 0
    assert lib.tdx_distill_target(*a2, B, per, -INF, INF, _st()) == 0
    torch.cuda.synchronize()
    assert (tm == int(tab.t_mid[T - 1])).all() and not torch.equal(tg, torch.full_like(tg, 7.0))


# ------------------------------------------------------------------ DistillStep
SHAPES = {"cond": (1, 28, 28), "laion": (4, 32, 32), "latent": (20,)}


def _model(kind, seed):
    if kind == "cond":
        from tiny_diffusion_amd.conditional_diffusion import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict(seed, True), strict=True)
    elif kind == "laion":
        from tiny_diffusion_amd.conditional_diffusion_laion import NoiseModel
        m = NoiseModel(time_dim=768)
        m.load_state_dict(make_state_dict_laion(seed), strict=True)
    else:
        from tiny_diffusion_amd.latent_diffusion import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict_latent(seed), strict=True)
    return m.cuda()


def _batch(kind, B, seed, grid):
    g = torch.Generator().manual_seed(seed)
    x0 = (torch.rand(B, *SHAPES[kind], generator=g) * 2 - 1).cuda()
    noise = torch.randn(B, *SHAPES[kind], generator=g).cuda()
    t = torch.tensor([grid[i % len(grid)] for i in (0, len(grid) - 1, 1, 2)][:B], dtype=torch.int64).cuda()
    y = (torch.randn(B, 768, generator=g) if kind == "laion" else torch.randint(0, 10, (B,), generator=g)).cuda()
    return x0, noise, t, y


@pytest.mark.parametrize("kind,B", [("cond", 4), ("laion", 2), ("latent", 4)])
def test_distill_step_is_the_hand_issued_launches(kind, B):
    """The step's gradient against the same launches issued by hand on a second, identical student: the teacher's
    inference forward twice around the two new entries, the student's training forward, a ``d_out`` from torch
    operations, the existing backward - expected bit-equal.  The teacher is left exactly as it was."""
    from tiny_diffusion_amd.train import DistillStep
    from tiny_diffusion_amd.unet import MODE_INFER, MODE_TRAIN

    N = 4
    fp = H.forward_process()
    grid = trailing_timesteps(fp, N)
    x0, noise, t, y = _batch(kind, B, 31, grid)
    assert int(t[0]) == grid[0] and int(t[1]) == T - 1
    m1, m2 = _model(kind, 3).train(), _model(kind, 3).train()
    teacher = _model(kind, 5).train()          # DistillStep puts it in eval()
    before = {k: v.detach().clone() for k, v in teacher.state_dict().items()}
    w_tab = truncated_snr_weights(fp, "v")
    step = DistillStep(m1, teacher, fp, N, teacher_prediction="eps", prediction="v", clip_denoised=True,
                       loss_weighting=w_tab, keep_target=True, lr=1e-3)
    assert not teacher.training and m1.training
    assert step.timesteps == grid and step.teacher_timesteps == trailing_timesteps(fp, 2 * N)
    loss = step.step(x0, y, t=t, noise=noise).clone()
    grad1 = step.flat_grad.clone()
    assert torch.equal(step.last_t, t) and step.sample_losses.shape == (B,)

    tab = distill_tables(fp, N, "eps", "v")
    rows, tmt = tab.rows.cuda(), tab.t_mid.cuda()
    z_t, _ = fp.q_sample("cuda", x0, t, noise=noise)
    per = z_t.numel() // B
    out1 = teacher._run_forward(z_t, t, y, mode=MODE_INFER)[0]
    z_mid, x1c, target = torch.empty_like(z_t), torch.empty_like(z_t), torch.empty_like(z_t)
    t_mid = torch.empty_like(t)
    check(lib.tdx_distill_teacher_step(z_t.data_ptr(), out1.data_ptr(), t.data_ptr(), rows.data_ptr(), tmt.data_ptr(),
                                       z_mid.data_ptr(), x1c.data_ptr(), t_mid.data_ptr(), B, per, -1.0, 1.0, _st()),
          "tdx_distill_teacher_step")
    out2 = teacher._run_forward(z_mid, t_mid, y, mode=MODE_INFER)[0]
    check(lib.tdx_distill_target(z_t.data_ptr(), z_mid.data_ptr(), out2.data_ptr(), x1c.data_ptr(), t.data_ptr(),
                                 rows.data_ptr(), target.data_ptr(), None, B, per, -1.0, 1.0, _st()),
          "tdx_distill_target")
    out, plan, _ = m2._run_forward(z_t, t, y, mode=MODE_TRAIN)
    n = out.numel()
    w = w_tab.cuda()[t]
    scale = torch.tensor(2.0, dtype=torch.float32, device="cuda") / torch.tensor(float(n), dtype=torch.float32, device="cuda")
    bshape = (B,) + (1,) * (out.dim() - 1)
    d_out = (out - target) * (scale * w).view(bshape)
    flat2, views2 = m2._grad_buffers(torch.device("cuda", torch.cuda.current_device()))
    m2._run_backward(plan, d_out, views2)
    torch.cuda.synchronize()
    assert torch.isfinite(target).all() and torch.isfinite(grad1).all() and grad1.abs().max() > 0
    assert t_mid.tolist() == tab.t_mid[t.cpu()].tolist()
    assert torch.equal(step.last_target, target)
    _assert_bits(step.last_target, target, "last_target")
    diff = (grad1 - flat2).abs().max().item()
    print(f"DistillStep {kind} B={B}: max |grad - hand-issued grad| = {diff:.3e}")
    assert torch.equal(grad1, flat2), diff
    want = (w.double().view(bshape) * (out.double() - target.double()) ** 2).sum().item() / n
    rel = abs(loss.item() - want) / want
    print(f"  returned loss {loss.item():.9g} vs fp64 {want:.9g}: rel {rel:.2e}")
    assert rel < 1e-6, rel
    after = teacher.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    # without keep_target nothing is retained
    step.keep_target = False
    step.step(x0, y, t=t, noise=noise)
    assert step.last_target is None


# ------------------------------------------------------------------ 7. the draws stay on the grid
def _latent_step(seed_model=3, **kw):
    from tiny_diffusion_amd.train import DistillStep

    fp = H.forward_process()
    return DistillStep(_model("latent", seed_model).train(), _model("latent", 5), fp, 4, lr=1e-4, **kw)


def test_draws_stay_on_the_grid_and_repeat_under_the_same_seeds():
    """64 steps at B = 8 draw 512 timesteps, every one in g_4 and every entry of g_4 among them (a miss of one of four
    equally likely values in 512 draws has probability 4 (3/4)^512 < 1e-60); a second step with the same seeds draws the
    same t."""
    B, grid = 8, trailing_timesteps(H.forward_process(), 4)
    g = torch.Generator().manual_seed(2)
    z0 = torch.randn(B, 20, generator=g).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    a = _latent_step(philox_seed=11, timestep_seed=12)
    drawn = []
    for _ in range(64):
        a.step(z0, y)
        drawn.append(a.last_t.clone())
    torch.cuda.synchronize()
    seen = torch.cat(drawn).tolist()
    assert len(seen) == 512 and set(seen) == set(grid), sorted(set(seen))
    assert torch.isfinite(a.loss).all() and torch.isfinite(a.flat_param).all()
    b = _latent_step(philox_seed=11, timestep_seed=12)
    for k in range(2):
        b.step(z0, y)
        assert torch.equal(b.last_t, drawn[k]), k
    c = _latent_step(philox_seed=11, timestep_seed=13)       # another seed, other draws (16 equal ones: 4^-16)
    other = []
    for _ in range(2):
        c.step(z0, y)
        other.append(c.last_t.clone())
    assert not torch.equal(torch.cat(other), torch.cat(drawn[:2]))


def test_the_averaged_student_becomes_the_next_teacher():
    """The documented hand-over, ``with step.ema_weights(): teacher.load_state_dict(student.state_dict())``: the
    teacher's parameters are the step's average bit for bit, its next inference forward runs on them (the packed weights
    are rebuilt), and the student has its own parameters back."""
    from tiny_diffusion_amd.unet import MODE_INFER

    B = 8
    g = torch.Generator().manual_seed(6)
    z0 = torch.randn(B, 20, generator=g).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    t = torch.full((B,), T - 1, dtype=torch.int64).cuda()
    step = _latent_step(philox_seed=3, timestep_seed=4, ema_decay=0.5)
    student, teacher = step.model, step.teacher
    out_before = teacher._run_forward(z0, t, y, mode=MODE_INFER)[0].clone()
    for _ in range(3):
        step.step(z0, y)
    live = step.flat_param.clone()
    with step.ema_weights():
        teacher.load_state_dict(student.state_dict())
    torch.cuda.synchronize()
    assert torch.equal(step.flat_param, live) and not torch.equal(step.ema, live)
    for k, p in teacher.named_parameters():
        lo, hi = step.offsets[k]
        assert torch.equal(p.detach().reshape(-1), step.ema[lo:hi]), k
    for (k, a), (_, b) in zip(teacher.named_buffers(), student.named_buffers()):
        assert torch.equal(a, b), k
    assert not teacher.training
    out_after = teacher._run_forward(z0, t, y, mode=MODE_INFER)[0]
    assert torch.isfinite(out_after).all() and not torch.equal(out_after, out_before)
    step.step(z0, y)                                          # and the round after it runs
    assert torch.isfinite(step.loss).all()


# ------------------------------------------------------------------ 8. the plain TrainStep is untouched
def test_plain_train_step_makes_the_calls_it_made(monkeypatch):
    """Every library entry one ``TrainStep.step`` calls, in order, before and after a ``DistillStep`` was built and
    stepped in the same process: the same list, and neither new entry in it."""
    from tiny_diffusion_amd.train import DistillStep, TrainStep

    fp = H.forward_process()
    B = 4
    x0, noise, t, y = _batch("cond", B, 9, trailing_timesteps(fp, 4))
    calls = []
    for name in _lib.EXPORTS:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])

    def plain(**kw):
        gc.collect()                               # a finalizer of an earlier model's plan is no call of this step
        calls.clear()
        step = TrainStep(_model("cond", 1).train(), fp, lr=1e-3, **kw)
        built = len(calls)
        step.step(x0, y, t=t, noise=noise)
        torch.cuda.synchronize()
        rec = [[c for c in part if c != "tdx_unet_destroy"] for part in (calls[:built], calls[built:])]
        return rec[0], rec[1], step.flat_param.clone()

    plain()                                        # first-use set-up of the process is not what is compared
    build0, step0, p0 = plain()
    v0 = plain(prediction="v", loss_weighting="min_snr")
    calls.clear()
    d = DistillStep(_model("cond", 1).train(), _model("cond", 2), fp, 4, lr=1e-3)
    d.step(x0, y, t=t, noise=noise)
    torch.cuda.synchronize()
    assert calls.count("tdx_distill_teacher_step") == 1 and calls.count("tdx_distill_target") == 1
    assert calls.count("tdx_unet_forward") == 3 and calls.count("tdx_unet_backward") == step0.count("tdx_unet_backward")
    build1, step1, p1 = plain()
    v1 = plain(prediction="v", loss_weighting="min_snr")
    assert step0 and "tdx_unet_forward" in step0 and "tdx_q_sample" in step0
    assert build1 == build0 and step1 == step0 and torch.equal(p1, p0)
    assert v1[0] == v0[0] and v1[1] == v0[1] and torch.equal(v1[2], v0[2])
    for rec in (step0, step1, v0[1], v1[1], build0, build1):
        assert "tdx_distill_teacher_step" not in rec and "tdx_distill_target" not in rec


# ------------------------------------------------------------------ 9. it learns
def test_a_short_round_lowers_the_loss():
    """30 steps at B = 16, N = 2 on synthetic data, conditional MNIST UNet, student initialised from the teacher, fixed
    seeds: the mean weighted loss of the last 5 steps is below that of the first 5.  No tighter number: nobody has
    measured one."""
    from tiny_diffusion_amd.train import DistillStep

    fp = H.forward_process()
    B = 16
    g = torch.Generator().manual_seed(4)
    x0 = (torch.rand(B, 1, 28, 28, generator=g) * 2 - 1).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    teacher, student = _model("cond", 5), _model("cond", 0).train()
    student.load_state_dict(teacher.state_dict())
    step = DistillStep(student, teacher, fp, 2, teacher_prediction="eps", prediction="v", clip_denoised=True,
                       loss_weighting=truncated_snr_weights(fp, "v"), lr=1e-3, philox_seed=21, timestep_seed=22)
    losses = [step.step(x0, y).clone() for _ in range(30)]
    torch.cuda.synchronize()
    losses = [v.item() for v in losses]
    first, last = sum(losses[:5]) / 5, sum(losses[-5:]) / 5
    print(f"weighted loss, first 5 steps {first:.5f}, last 5 steps {last:.5f}")
    assert all(math.isfinite(v) for v in losses)
    assert last < first, (first, last)
    # and the student is sampled on its own grid by the unchanged sampler
    from tiny_diffusion_amd.conditional_diffusion import ddim_sample
    x = ddim_sample(student, fp, "cuda", 4, y[:4], timesteps=step.timesteps, prediction="v", clip_denoised=True)
    assert x.shape == (4, 1, 28, 28) and torch.isfinite(x).all() and x.abs().max().item() <= 1.0
