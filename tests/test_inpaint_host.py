"""Inpainting (``known`` / ``mask``), host side (no GPU): the new C entries are declared, bound and exported; every
argument error of the two keywords is a ``ValueError`` in every module's three samplers before a device is touched, after
the existing argument errors; the marginal invariant of the known region in fp64 from the repository's own tables
(and that a history of clamped rather than blended predictions breaks it); the fp32 blend is exact for a binary mask."""
import math
import os
import re

import pytest
import torch

from inpaint_helpers import blend32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tdx_p_sample_step_x0_masked", "tdx_p_sample_step_x0_guided_masked", "tdx_p_sample_step_ms_masked",
               "tdx_p_sample_step_ms_guided_masked", "tdx_unet_eval_step_update",
               "tdx_unet_drop_sampling_tables")
NAN, INF = float("nan"), float("inf")


def _fp(T=1000):
    from tiny_diffusion_amd.schedule import ForwardProcess

    return ForwardProcess(num_timesteps=T)


# ------------------------------------------------------------------ 1. ABI
def test_new_symbols_declared_listed_and_exported():
    import tiny_diffusion_amd._lib as L

    hdr = open(os.path.join(ROOT, "include", "tdx.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS, name
        assert getattr(L.lib, name).argtypes is not None, name   # bound: the library exports it
    assert L.lib.tdx_version() == 400   # the ABI only grows


# ------------------------------------------------------------------ 2. argument errors
class _NoModel:      # no _arch: the samplers take the default input shape (1, 28, 28)
    def eval(self):
        raise AssertionError("the argument errors come before the model is touched")


class _NoVAE:
    def eval(self):
        pass


N = 2
_K = torch.zeros(N, 1, 28, 28)
_M = torch.ones(1, 1, 28, 28)


def _with(t, value):
    t = t.clone()
    t.view(-1)[3] = value
    return t


BAD = {
    "known alone": (dict(known=_K), "known and mask"),
    "mask alone": (dict(mask=_M), "known and mask"),
    "known does not broadcast": (dict(known=torch.zeros(3, 1, 28, 28), mask=_M), "known.*broadcast"),
    "mask does not broadcast": (dict(known=_K, mask=torch.ones(1, 1, 28, 27)), "mask.*broadcast"),
    "mask has more dimensions": (dict(known=_K, mask=torch.ones(1, N, 1, 28, 28)), "mask.*broadcast"),
    "known NaN": (dict(known=_with(_K, NAN), mask=_M), "known must be finite"),
    "known inf": (dict(known=_with(_K, -INF), mask=_M), "known must be finite"),
    "mask below 0": (dict(known=_K, mask=_with(_M, -0.125)), r"mask must lie in \[0, 1\]"),
    "mask above 1": (dict(known=_K, mask=_with(_M, 1.5)), r"mask must lie in \[0, 1\]"),
    "mask NaN": (dict(known=_K, mask=_with(_M, NAN)), r"mask must lie in \[0, 1\]"),
}


def _samplers():
    """(name, call(**kw)) for sample / ddim_sample / dpm_sample of the five drop-in modules and the three loops, on a
    CPU device: the "GPU only" error would be a TdxError (not a ValueError), and it must not be reached."""
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import conditional_diffusion_laion as LA
    from tiny_diffusion_amd import diffusion as D
    from tiny_diffusion_amd import diffusion_transformer as DT
    from tiny_diffusion_amd import latent_diffusion as LD
    from tiny_diffusion_amd.schedule import ddim_sample_loop, dpm_sample_loop, sample_loop

    fp = _fp(20)
    y = torch.tensor([1, 2])
    te = torch.zeros(N, 768)
    extra = {"sample": {}, "ddim_sample": dict(steps=5), "dpm_sample": dict(steps=5)}
    out = [("sample_loop", lambda **kw: sample_loop(_NoModel(), fp, "cpu", N, **kw)),
           ("ddim_sample_loop", lambda **kw: ddim_sample_loop(_NoModel(), fp, "cpu", N, steps=5, **kw)),
           ("dpm_sample_loop", lambda **kw: dpm_sample_loop(_NoModel(), fp, "cpu", N, steps=5, **kw))]
    for fn, ex in extra.items():
        out.append((f"diffusion.{fn}",
                    lambda _f=getattr(D, fn), _e=ex, **kw: _f(_NoModel(), fp, "cpu", n_samples=N, **_e, **kw)))
        out.append((f"conditional_diffusion.{fn}",
                    lambda _f=getattr(C, fn), _e=ex, **kw: _f(_NoModel(), fp, "cpu", n_samples=N, y=y, **_e, **kw)))
        out.append((f"conditional_diffusion_laion.{fn}",
                    lambda _f=getattr(LA, fn), _e=ex, **kw: _f(_NoModel(), fp, "cpu", text_embeds=te, **_e, **kw)))
        for mod in (LD, DT):
            out.append((f"{mod.__name__.rsplit('.', 1)[-1]}.{fn}",
                        lambda _f=getattr(mod, fn), _e=ex, **kw: _f(_NoVAE(), _NoModel(), fp, "cpu", n_samples=N, y=y,
                                                                   **_e, **kw)))
    assert len(out) == 18
    return out


@pytest.mark.parametrize("case", list(BAD), ids=lambda c: c.replace(" ", "_"))
def test_known_mask_argument_errors_in_every_sampler(case):
    from tiny_diffusion_amd import _lib

    kw, match = BAD[case]
    for name, call in _samplers():
        with pytest.raises(ValueError, match=match):
            call(**kw)
        # ... and before the schedule's own errors where the sampler builds one
        if "ddim" in name or "dpm" in name:
            with pytest.raises(ValueError, match=match):
                call(timesteps=[3, 3], **kw)
    assert issubclass(_lib.TdxError, RuntimeError) and not issubclass(_lib.TdxError, ValueError)


def test_the_existing_argument_errors_still_come_first():
    bad = dict(known=_K)      # mask missing
    for name, call in _samplers():
        with pytest.raises(ValueError, match="prediction"):
            call(prediction="x0", **bad)
        with pytest.raises(ValueError, match="clip_denoised"):
            call(clip_denoised=(1, -1), **bad)
        if name.startswith(("diffusion.", "latent", "diffusion_transformer")) or name.endswith("_loop"):
            with pytest.raises(ValueError, match="guidance_scale"):     # no conditional UNet: no null condition
                call(guidance_scale=2.0, **bad)
        if "dpm" in name:
            with pytest.raises(ValueError, match="deterministic"):
                call(noises=[None], **bad)


def test_accepted_values_reach_the_device_check():
    from tiny_diffusion_amd import _lib

    good = [dict(), dict(known=None, mask=None), dict(known=_K, mask=_M),
            dict(known=torch.zeros(1, 1, 28, 28), mask=torch.tensor(0.5)),          # both broadcast
            dict(known=_K.double(), mask=_M.to(torch.int64)),                       # any real dtype
            dict(known=_K.numpy(), mask=_with(_M, 0.0).numpy()),
            dict(known=_K, mask=_M, clip_denoised=True), dict(known=_K, mask=_M, prediction="v")]
    for name, call in _samplers():
        for kw in good:
            with pytest.raises(_lib.TdxError, match="GPU only"):
                call(**kw)


# ------------------------------------------------------------------ 3. the marginal invariant, fp64
def _invariant(sched, table, acp, hist_of):
    """Feed the chain x0m = known at every step and return the worst deviation of the known region from the forward
    marginal a_{k-1} known + b_{k-1} eps0 (from ``known`` itself after step 0).  ``hist_of(k, known)``: the history the
    multistep rows see at step k."""
    g = torch.Generator().manual_seed(5)
    known = 2 * torch.rand(257, dtype=torch.float64, generator=g) - 1
    x_T = torch.randn(257, dtype=torch.float64, generator=g)
    taus = sched.timesteps.tolist()
    S = len(taus)
    a = [math.sqrt(acp[t].item()) for t in taus]
    b = [math.sqrt(1 - acp[t].item()) for t in taus]
    eps0 = (x_T - a[S - 1] * known) / b[S - 1]
    x, worst = x_T, 0.0
    for k in range(S - 1, -1, -1):
        _, _, A, Bx, last = table[k].tolist()
        x = A * known + Bx * x              # x0m = known; no noise: eta = 0 / the multistep chain
        if hist_of is not None:
            if last != 0.0:
                x = x + last * hist_of(k, known)
        else:
            assert last == 0.0              # sigma
        want = known if k == 0 else a[k - 1] * known + b[k - 1] * eps0
        worst = max(worst, (x - want).abs().max().item())
    return worst


@pytest.mark.parametrize("steps", [10, 50])
def test_known_region_stays_on_the_forward_marginal_ddim(steps):
    from tiny_diffusion_amd.schedule import ddim_schedule

    fp = _fp()
    sched = ddim_schedule(fp, steps=steps, eta=0.0)
    worst = _invariant(sched, sched.x0_form(fp, "eps", dtype=torch.float64), fp.alphas_cumprod.double(), None)
    print(f"DDIM eta=0 S={steps}: worst deviation from the forward marginal {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("steps", [10, 20])
def test_known_region_stays_on_the_forward_marginal_dpm(steps):
    from tiny_diffusion_amd.schedule import dpm_solver_schedule

    fp = _fp()
    sched = dpm_solver_schedule(fp, steps=steps)
    tab = sched.multistep_form(fp, "eps", dtype=torch.float64)
    assert (tab[1:-1, 4] != 0).all() and sched.steps > 3       # second-order rows in the middle
    acp = fp.alphas_cumprod.double()
    worst = _invariant(sched, tab, acp, lambda k, known: known)          # hist = x0m = known
    print(f"DPM-Solver++(2M) S={sched.steps}: worst deviation from the forward marginal {worst:.2e}")
    assert worst <= 1e-12
    # the other design: the history holds the clamped prediction x0c of a (wrong) model, not the blend
    g = torch.Generator().manual_seed(6)
    wrong = 0.5 * torch.randn(257, dtype=torch.float64, generator=g)
    miss = _invariant(sched, tab, acp, lambda k, known: known + wrong)
    print(f"DPM-Solver++(2M) S={sched.steps}, hist = x0c of a wrong model: deviation {miss:.2e}")
    assert miss > 1e-3


# ------------------------------------------------------------------ 4. the blend is exact for a binary mask
def test_fp32_blend_is_exact_for_a_binary_mask():
    g = torch.Generator().manual_seed(7)
    x0c = torch.cat([torch.randn(4096, generator=g), torch.tensor([0.0, -0.0, 1.0, -1.0, 3e38, -3e38, 1e-45, -1e-45])])
    known = torch.cat([3 * torch.randn(4096, generator=g), torch.tensor([-0.0, 0.0, -1.0, 1.0, -3e38, 3e38, -1e-45, 1e-45])])
    assert x0c.dtype == torch.float32
    ones, zeros = torch.ones_like(x0c), torch.zeros_like(x0c)
    assert torch.equal(blend32(x0c, known, ones), known)
    assert torch.equal(blend32(x0c, known, zeros), x0c)
    half = blend32(x0c[:4096], known[:4096], torch.full((4096,), 0.5))
    assert torch.equal(half, 0.5 * x0c[:4096] + 0.5 * known[:4096]) and not torch.equal(half, known[:4096])
