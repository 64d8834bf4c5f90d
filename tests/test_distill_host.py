"""CPU: the host side of progressive distillation - the trailing grids, ``distill_tables`` against an
independent fp64 restatement from alpha and sigma, ``truncated_snr_weights``, the fp32 restatement of the two kernels
against its fp64 twin within the derived forward-error bound, and ``DistillStep``'s argument errors (all raised before
any device work: the modules here live on the CPU)."""
import numpy as np
import pytest
import torch

import distill_helpers as H
from tiny_diffusion_amd.schedule import (ddim_schedule, distill_tables, loss_weights, timestep_probs,
                                         trailing_timesteps, truncated_snr_weights)

T = 1000
NS = (1, 2, 4, 8, 64, 128, 256, 500)


# ------------------------------------------------------------------ grids
@pytest.mark.parametrize("T_", [1000, 20])
def test_trailing_grids_nest_ascend_and_end_at_pure_noise(T_):
    fp = H.forward_process(T_)
    for N in [n for n in NS if 2 * n <= T_] + ([10] if T_ == 20 else []):
        g, g2 = trailing_timesteps(fp, N), trailing_timesteps(fp, 2 * N)
        assert g == g2[1::2], N
        for grid in (g, g2):
            assert all(isinstance(v, int) for v in grid)
            assert all(b > a for a, b in zip(grid, grid[1:])) and grid[0] >= 0 and grid[-1] == T_ - 1
        assert len(g) == N and len(g2) == 2 * N
        assert g == [(i + 1) * T_ // N - 1 for i in range(N)]
        ddim_schedule(fp, timesteps=g)                      # accepted unchanged
    assert trailing_timesteps(fp, T_) == list(range(T_))
    assert trailing_timesteps(fp, 1) == [T_ - 1]


@pytest.mark.parametrize("bad", [0, -1, 1001, 2.0, True, None, "4"])
def test_trailing_timesteps_rejects(bad):
    with pytest.raises(ValueError, match="steps"):
        trailing_timesteps(H.forward_process(), bad)


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("tp,sp", [("eps", "v"), ("v", "v"), ("eps", "eps"), ("v", "eps")])
def test_tables_fp64_against_alpha_sigma_restatement(tp, sp):
    fp = H.forward_process()
    worst = 0.0
    for N in NS:
        rows, t_mid, probs = distill_tables(fp, N, tp, sp, dtype=torch.float64)
        assert rows.dtype == torch.float64 and rows.shape == (T, 12)
        assert t_mid.dtype == torch.int64 and t_mid.shape == (T,) and probs.shape == (T,)
        want = H.paper_rows64(fp, N, tp, sp)
        g = trailing_timesteps(fp, N)
        assert sorted(want) == g
        on = torch.zeros(T, dtype=torch.bool)
        on[g] = True
        assert torch.isnan(rows[~on]).all() and torch.isfinite(rows[on]).all()
        assert (t_mid[~on] == -1).all()
        for (t, tm, _), j in zip(H.student_triples(fp, N), range(N)):
            assert int(t_mid[t]) == tm
            got, ref = rows[t].numpy(), want[t]
            rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
            rel[ref == 0] = np.abs(got[ref == 0])
            worst = max(worst, rel.max())
            assert rel.max() <= 1e-12, (N, j, rel)
        W2, W1 = rows[on, H.COL["W2"]], rows[on, H.COL["W1"]]
        assert ((W1 + W2 - 1).abs() < 1e-12).all()
        assert (W2 > 0).all() and (W2 <= 1).all() and (W2 >= 0.33).all()
        assert probs.sum().item() == pytest.approx(1.0, abs=1e-12)
        assert torch.equal(torch.nonzero(probs).flatten(), torch.tensor(g))
        assert torch.equal(probs[on], torch.full((N,), 1.0 / N, dtype=torch.float64))
        timestep_probs(T, probs)                            # what TrainStep's fixed-table sampler accepts
        for dt in (torch.float32, torch.float64):           # the j = 0 row: the step to x0 itself, exactly
            r0 = distill_tables(fp, N, tp, sp, dtype=dt).rows[g[0]]
            assert r0[H.COL["W2"]] == 1 and r0[H.COL["W1"]] == 0 and r0[H.COL["A2"]] == 1 and r0[H.COL["B2"]] == 0
    print(f"teacher {tp} student {sp}: worst relative difference of a table entry {worst:.2e}")


@pytest.mark.parametrize("tp", ["eps", "v"])
def test_teacher_columns_are_the_x0_form_rows_bit_for_bit(tp):
    fp = H.forward_process()
    for N in NS:
        g2 = trailing_timesteps(fp, 2 * N)
        form = ddim_schedule(fp, timesteps=g2, eta=0.0).x0_form(fp, tp)
        rows = distill_tables(fp, N, tp, "v").rows
        assert rows.dtype == torch.float32
        for j in range(N):
            r = rows[g2[2 * j + 1]]
            assert np.array_equal(H.bits(r[0:4]), H.bits(form[2 * j + 1, 0:4])), (N, j)
            assert np.array_equal(H.bits(r[4:8]), H.bits(form[2 * j, 0:4])), (N, j)
        # and the fp32 table is the one rounding of the fp64 one
        r64 = distill_tables(fp, N, tp, "v", dtype=torch.float64).rows
        on = ~torch.isnan(r64[:, 0])
        assert torch.equal(rows[on], r64[on].to(torch.float32))


@pytest.mark.parametrize("kw", [dict(student_steps=0), dict(student_steps=501), dict(student_steps=4.0),
                                dict(student_steps=True), dict(student_steps=4, teacher_prediction="x0"),
                                dict(student_steps=4, student_prediction="x0"),
                                dict(student_steps=4, dtype=torch.float16)])
def test_distill_tables_rejects(kw):
    with pytest.raises(ValueError):
        distill_tables(H.forward_process(), **kw)


def test_truncated_snr_weights():
    fp = H.forward_process()
    snr = fp.snr()
    for pred, den in (("v", snr + 1.0), ("eps", snr)):
        w = truncated_snr_weights(fp, pred)
        assert w.dtype == torch.float32 and w.shape == (T,)
        assert torch.equal(w, (torch.clamp(snr, min=1.0) / den).to(torch.float32))
        assert torch.equal(loss_weights(fp, pred, w), w)    # accepted as loss_weighting=<tensor>
    wv = truncated_snr_weights(fp, "v").double()
    assert wv.min() >= 0.5 - 1e-7 and wv.max() <= 1.0      # max(s, 1) / (s + 1) lies in [1/2, 1)
    with pytest.raises(ValueError, match="prediction"):
        truncated_snr_weights(fp, "x0")


# ------------------------------------------------------------------ arithmetic
@pytest.mark.parametrize("N", [4, 256])
@pytest.mark.parametrize("tp,sp", [("eps", "v"), ("v", "eps")])
def test_fp32_restatement_within_the_derived_bound_of_fp64(N, tp, sp):
    """Every grid row, random inputs, clamp (-1, 1) binding on part of them: |fp32 - fp64| <= n u S for z_mid (n = 5)
    and the target (n = 11); and the fp64 convex form against the paper's form from alpha and sigma."""
    fp = H.forward_process()
    rows32 = distill_tables(fp, N, tp, sp).rows.numpy()
    rows64 = distill_tables(fp, N, tp, sp, dtype=torch.float64).rows.numpy()
    triples = H.student_triples(fp, N)
    t = np.array([tr[0] for tr in triples])
    rng = np.random.default_rng(N)
    z, o1, o2 = H.clamp_case(rng, rows32, t, (N, 16))
    f32 = H.kernels_np(rows32, t, z, o1, o2, -1.0, 1.0)
    f64 = H.kernels_np(rows32, t, z.astype(np.float64), o1.astype(np.float64), o2.astype(np.float64), -1.0, 1.0)
    assert f32["target"].dtype == np.float32 and f64["target"].dtype == np.float64
    S_zmid, S_target, _ = H.magnitudes(rows32, t, z, o1, o2)
    for name, n, S in (("z_mid", H.N_ZMID, S_zmid), ("target", H.N_TARGET, S_target)):
        err = np.abs(f32[name].astype(np.float64) - f64[name])
        ratio = (err / (n * H.U * S)).max()
        print(f"N={N} {tp}->{sp} {name}: max |fp32 - fp64| = {err.max():.3e}, largest share of the bound {ratio:.3f}")
        assert (err <= n * H.U * S).all(), (name, ratio)
    for k in ("x1c", "x2c"):
        c = f64[k]
        assert (np.abs(c) == 1.0).any() and (np.abs(c) < 1.0).any(), k
    # fp64, unrounded tables: the convex form is the paper's form up to that form's own cancellation
    conv = H.kernels_np(rows64, t, z.astype(np.float64), o1.astype(np.float64), o2.astype(np.float64), -1.0, 1.0)
    worst = 0.0
    for b, (tt, tm, te) in enumerate(triples):
        z_end, xt, tg, tol = H.paper64(fp, tt, tm, te, z[b].astype(np.float64), o1[b].astype(np.float64),
                                       o2[b].astype(np.float64), -1.0, 1.0, tp, sp)
        assert np.abs(conv["z_end"][b] - z_end).max() <= 1e-13 * (1 + np.abs(z_end).max())
        d = np.abs(conv["target"][b] - tg)
        worst = max(worst, (d / tol).max())
        assert (d <= tol).all(), (b, (d / tol).max())
        # the defining identity: one student step with x~ lands on the teacher's z_end
        (a, s), (ae, se) = H.alpha_sigma(fp, tt), H.alpha_sigma(fp, te)
        As, Bs = ae - (se / s) * a, se / s
        ident = np.abs(As * conv["x_tilde"][b] + Bs * z[b].astype(np.float64) - conv["z_end"][b])
        assert ident.max() <= 1e-14 * (1 + np.abs(conv["z_end"][b]).max())
    print(f"N={N} {tp}->{sp}: convex form vs paper form, largest share of the cancellation bound {worst:.3f}")


# ------------------------------------------------------------------ DistillStep's argument errors
def _cpu_models():
    from tiny_diffusion_amd.conditional_diffusion import NoiseModel as Cond
    from tiny_diffusion_amd.diffusion import NoiseModel as Unc
    return Unc(), Unc(), Cond()


def test_distill_step_argument_errors_come_before_device_work():
    from tiny_diffusion_amd.schedule import ForwardProcess
    from tiny_diffusion_amd.train import DistillStep, TrainStep

    assert issubclass(DistillStep, TrainStep)
    fp = H.forward_process()
    student, teacher, other = _cpu_models()
    on_grid = torch.zeros(T)
    on_grid[trailing_timesteps(fp, 4)] = torch.tensor([1.0, 2.0, 3.0, 4.0])
    off_grid = on_grid.clone()
    off_grid[0] = 0.5
    cases = [
        (dict(student=student, teacher=student), "two modules"),
        (dict(teacher=other), "same architecture"),
        (dict(teacher_diffusion=ForwardProcess(num_timesteps=500)), "another forward process"),
        (dict(student_steps=501), "student_steps"),
        (dict(student_steps=2.0), "student_steps"),
        (dict(timestep_sampler="loss_second_moment"), "loss_second_moment"),
        (dict(timestep_sampler=off_grid), "off the student's grid"),
        (dict(use_graph=True), "later change"),
        (dict(prediction="x0"), "prediction"),
        (dict(teacher_prediction="x0"), "prediction"),
        (dict(clip_denoised=(1.0, -1.0)), "clip_denoised"),
    ]
    for kw, match in cases:
        args = dict(student=student, teacher=teacher, diffusion=fp, student_steps=4)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            DistillStep(**args)
    # every check passed: the first device work is TrainStep's own, which refuses a CPU module
    with pytest.raises(RuntimeError, match="CUDA"):
        DistillStep(student, teacher, fp, 4, timestep_sampler=on_grid)
    assert teacher.training and not any(p.is_cuda for p in teacher.parameters())
