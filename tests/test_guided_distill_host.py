"""CPU: the host side of guided distillation - ``guidance_distill_table`` against ``x0_form`` and an
fp64 restatement from alpha and sigma, the fp32 restatements of the three kernels against their fp64 twins within the
derived forward-error bounds, and the argument errors of ``DistillStep(guidance_scale=...)`` and
``GuidanceDistillStep`` (all raised before any device work: the modules here live on the CPU)."""
import math

import numpy as np
import pytest
import torch

import distill_helpers as H
import guided_distill_helpers as GH
from tiny_diffusion_amd.schedule import ddpm_schedule, distill_tables, guidance_distill_table, trailing_timesteps

T = 1000


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("tp", ["eps", "v"])
@pytest.mark.parametrize("sp", ["eps", "v"])
def test_table_columns(tp, sp):
    fp = H.forward_process()
    tab = guidance_distill_table(fp, tp, sp)
    assert tab.dtype == torch.float32 and tab.shape == (T, 4) and tab.is_contiguous()
    assert torch.isfinite(tab).all()                         # every row is filled
    form = ddpm_schedule(fp).x0_form(fp, tp)
    assert np.array_equal(H.bits(tab[:, 0:2]), H.bits(form[:, 0:2]))
    tab64 = guidance_distill_table(fp, tp, sp, dtype=torch.float64)
    assert tab64.dtype == torch.float64
    assert torch.equal(tab64[:, 0:2], ddpm_schedule(fp).x0_form(fp, tp, dtype=torch.float64)[:, 0:2])
    assert torch.equal(tab[:, 2:4], tab64[:, 2:4].to(torch.float32))    # rounded once
    worst = 0.0
    for t in range(T):
        a, s = H.alpha_sigma(fp, t)
        G, Hh = (-1.0 / s, a / s) if sp == "v" else (-a / s, 1.0 / s)
        for got, ref in ((tab64[t, 2].item(), G), (tab64[t, 3].item(), Hh)):
            worst = max(worst, abs(got - ref) / abs(ref))
    assert worst <= 1e-14, worst
    # and they are distill_tables' (G, H) wherever that table has a row
    for N in (1, 4, 256):
        rows = distill_tables(fp, N, tp, sp).rows
        g = trailing_timesteps(fp, N)
        assert np.array_equal(H.bits(rows[g][:, 10:12]), H.bits(tab[g][:, 2:4])), N


@pytest.mark.parametrize("pred", ["eps", "v"])
def test_equal_predictions_without_a_clamp_give_the_teachers_output_back(pred):
    """G (p z + q e) + H z == e in fp64 on the unrounded table: the student's target IS the (w = 1: conditional)
    output when nothing clamps and both predict the same thing.  G q = 1 and G p + H = 0 carry a few fp64 roundings of
    quantities as large as 1 / (alpha sigma): 8 of them on the magnitudes that cancel."""
    fp = H.forward_process()
    tab = guidance_distill_table(fp, pred, pred, dtype=torch.float64).numpy()
    rng = np.random.default_rng(5)
    t = np.arange(T)
    z, oc, ou = (rng.standard_normal((T, 8)) for _ in range(3))
    e = GH.cfg_np(oc, ou, 1.0)
    got = GH.guidance_target_np(tab, t, z, e, -math.inf, math.inf)["target"]
    S = GH.guidance_magnitude(tab, t, z, np.abs(e))
    assert (np.abs(got - e) <= 8 * 2.0 ** -53 * S).all(), (np.abs(got - e) / (2.0 ** -53 * S)).max()


@pytest.mark.parametrize("kw", [dict(teacher_prediction="x0"), dict(student_prediction="x0"),
                                dict(dtype=torch.float16), dict(teacher_prediction=None)])
def test_table_rejects(kw):
    with pytest.raises(ValueError):
        guidance_distill_table(H.forward_process(), **kw)


# ------------------------------------------------------------------ arithmetic
def test_cfg_restatement():
    rng = np.random.default_rng(0)
    oc, ou = (rng.standard_normal(64).astype(np.float32) for _ in range(2))
    for w in GH.WS:
        assert np.float32(w) == w                                        # exact inputs
        e32, e64 = GH.cfg_np(oc, ou, w), GH.cfg_np(oc.astype(np.float64), ou.astype(np.float64), w)
        assert e32.dtype == np.float32
        assert (np.abs(e32 - e64) <= GH.N_CFG * GH.U * GH.cfg_mag(oc, ou, w)).all()
        assert np.array_equal(H.bits(GH.cfg_np(ou, ou, w)), H.bits(ou))  # out_c == out_u: out_u exactly, any w
    assert np.array_equal(GH.cfg_np(oc, ou, 0.0), ou) and np.array_equal(GH.cfg_np(oc, ou, 1.0), ou + (oc - ou))


@pytest.mark.parametrize("N", [4, 256])
@pytest.mark.parametrize("tp,sp", [("eps", "v"), ("v", "eps")])
def test_guided_pair_fp32_within_the_derived_bound_of_fp64(N, tp, sp):
    """Every grid row, every w, clamp (-1, 1) binding on part of the elements: |fp32 - fp64| <= n u S with n = 8 for
    z_mid and n = 14 for the target (guided_distill_helpers, 3.)."""
    fp = H.forward_process()
    rows32 = distill_tables(fp, N, tp, sp).rows.numpy()
    t = np.array([tr[0] for tr in H.student_triples(fp, N)])
    for w in GH.WS:
        z, o1, o2 = GH.guided_case(np.random.default_rng(N + 1), rows32, t, (N, 16), w)
        f32 = GH.guided_kernels_np(rows32, t, z, o1, o2, w, -1.0, 1.0)
        f64 = GH.guided_kernels_np(rows32, t, *(v.astype(np.float64) for v in (z, o1, o2)), w, -1.0, 1.0)
        assert f32["target"].dtype == np.float32 and f64["target"].dtype == np.float64
        S_zmid, S_target, _ = GH.guided_magnitudes(rows32, t, z, o1, o2, w)
        for name, n, S in (("z_mid", GH.N_ZMID_G, S_zmid), ("target", GH.N_TARGET_G, S_target)):
            err = np.abs(f32[name].astype(np.float64) - f64[name])
            share = (err / (n * GH.U * S)).max()
            print(f"N={N} {tp}->{sp} w={w} {name}: max |fp32 - fp64| = {err.max():.3e}, largest share of the bound "
                  f"{share:.3f}")
            assert (err <= n * GH.U * S).all(), (name, w, share)
        for k in ("x1c", "x2c"):
            assert (np.abs(f64[k]) == 1.0).any() and (np.abs(f64[k]) < 1.0).any(), (k, w)


@pytest.mark.parametrize("tp,sp", [("eps", "v"), ("v", "eps")])
def test_guidance_target_fp32_within_the_derived_bound_of_fp64(tp, sp):
    """Every timestep, unguided (n = 5) and every w (n = 8), clamp (-1, 1) binding on part of the elements."""
    fp = H.forward_process()
    rows32 = guidance_distill_table(fp, tp, sp).numpy()
    t = np.arange(T)
    for w in (None,) + GH.WS:
        z, o, _ = GH.guided_case(np.random.default_rng(3), rows32, t, (T, 8), 1.0 if w is None else w)
        o64 = o.astype(np.float64)
        if w is None:
            e32, e64, mag, n = o[0], o64[0], np.abs(o64[0]), GH.N_SAME
        else:
            e32, e64, mag, n = GH.cfg_np(o[0], o[1], w), GH.cfg_np(o64[0], o64[1], w), GH.cfg_mag(o[0], o[1], w), GH.N_SAME_G
        f32 = GH.guidance_target_np(rows32, t, z, e32, -1.0, 1.0)
        f64 = GH.guidance_target_np(rows32, t, z.astype(np.float64), e64, -1.0, 1.0)
        assert f32["target"].dtype == np.float32
        S = GH.guidance_magnitude(rows32, t, z, mag)
        err = np.abs(f32["target"].astype(np.float64) - f64["target"])
        share = (err / (n * GH.U * S)).max()
        print(f"{tp}->{sp} w={w}: max |fp32 - fp64| = {err.max():.3e}, largest share of the bound {share:.3f}")
        assert (err <= n * GH.U * S).all(), (w, share)
        assert (np.abs(f64["x0c"]) == 1.0).any() and (np.abs(f64["x0c"]) < 1.0).any(), w


# ------------------------------------------------------------------ argument errors of the two steps
def _cpu_models():
    from tiny_diffusion_amd.conditional_diffusion import NoiseModel as Cond
    from tiny_diffusion_amd.diffusion import NoiseModel as Unc
    from tiny_diffusion_amd.latent_diffusion import NoiseModel as Latent
    return {"cond": (Cond(), Cond()), "unc": (Unc(), Unc()), "latent": (Latent(), Latent())}


def _steps():
    from tiny_diffusion_amd.train import DistillStep, GuidanceDistillStep

    def distill(student, teacher, fp, w, **kw):
        return DistillStep(student, teacher, fp, 4, guidance_scale=w, **kw)

    def guidance(student, teacher, fp, w, **kw):
        return GuidanceDistillStep(student, teacher, fp, w, **kw)

    return {"DistillStep": distill, "GuidanceDistillStep": guidance}


@pytest.mark.parametrize("which", ["DistillStep", "GuidanceDistillStep"])
def test_argument_errors_come_before_device_work(which):
    from tiny_diffusion_amd.schedule import ForwardProcess
    from tiny_diffusion_amd.train import TrainStep

    make = _steps()[which]
    fp = H.forward_process()
    models = _cpu_models()
    student, teacher = models["cond"]
    for kind in ("unc", "latent"):                       # no null condition: a finite w is refused, None is not
        s, t_ = models[kind]
        with pytest.raises(ValueError, match="conditional UNet"):
            make(s, t_, fp, 3.0)
        with pytest.raises(RuntimeError, match="CUDA"):
            make(s, t_, fp, None)
    for w in (math.inf, -math.inf, math.nan, True, False, "3", [3.0]):
        with pytest.raises(ValueError, match="finite number"):
            make(student, teacher, fp, w)
    with pytest.raises(ValueError, match="later change"):
        make(student, teacher, fp, 3.0, use_graph=True)
    with pytest.raises(ValueError, match="two modules"):
        make(student, student, fp, 3.0)
    with pytest.raises(ValueError, match="same architecture"):
        make(student, models["unc"][0], fp, 3.0)
    with pytest.raises(ValueError, match="another forward process"):
        make(student, teacher, fp, 3.0, teacher_diffusion=ForwardProcess(num_timesteps=500))
    for kw in (dict(prediction="x0"), dict(teacher_prediction="x0")):
        with pytest.raises(ValueError, match="prediction"):
            make(student, teacher, fp, 3.0, **kw)
    with pytest.raises(ValueError, match="clip_denoised"):
        make(student, teacher, fp, 3.0, clip_denoised=(1.0, -1.0))
    # every check passed: the first device work is TrainStep's own, which refuses a CPU module
    for w in (3.0, 0, -0.5, None):
        with pytest.raises(RuntimeError, match="CUDA"):
            make(student, teacher, fp, w)
    assert teacher.training and not any(p.is_cuda for p in teacher.parameters())
    from tiny_diffusion_amd import train
    assert issubclass(getattr(train, which), TrainStep)
