"""EMA of the parameters on the device: the fused Adam + EMA kernel against the existing Adam entries and torch's
``e + a * (p - e)`` bit for bit, the buffer swap, ``TrainStep`` keeping the recurrence in its three optimizer call
sites, and ``ema_weights()`` really putting the average under the forward and both samplers.

Everything is compared with ``torch.equal``: the build has fp contraction off, the new kernel shares the Adam
expressions with the old ones, the clip partial sums use a fixed grid and order, and the average is three separately
rounded fp32 operations - what torch does with three tensor operations."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.weights import make_state_dict, make_state_dict_latent  # noqa: E402

from tiny_diffusion_amd._lib import check, lib  # noqa: E402

TDX_E_BADARG = -1
LR, B1, B2, EPS, GSCALE = 1e-3, 0.9, 0.999, 1e-8, 0.5
# 1027 = 4 x 256 + 3: four full blocks and three lanes of a fifth; 2 097 157 = 2048 x 256 x 4 + 5: the grid is capped at
# 2048 blocks, so every lane takes four grid-stride iterations and five lanes a fifth; (1027, True): views one float
# into their allocations, so no pointer is 16-byte aligned
SIZES = [(1, False), (3, False), (4, False), (1027, False), (2_097_157, False), (1027, True)]
DECAYS = (0.9999, 0.5, 0.0, 1.0)
FORMS = ("host", "dev", "clip_host", "clip_dev")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _view(t, misaligned):
    """A fresh device copy of ``t``: at the start of its allocation (512-byte aligned), or one float in."""
    if not misaligned:
        out = t.clone()
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:]
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


@functools.lru_cache(maxsize=None)
def _data(n):
    """p, g, m, v, e of one size (shared by every test of that size, never written: the tests copy)."""
    gen = torch.Generator(device="cuda").manual_seed(1000 + n % 997)
    p, g, m, e = (torch.randn(n, device="cuda", generator=gen) for _ in range(4))
    v = torch.rand(n, device="cuda", generator=gen) * 0.1
    g[2::5] = 0.0    # exact zeros (n = 1 keeps its one non-zero gradient: the clip forms need a norm)
    m *= 0.1
    return p, g, m, v, e


def _hyper(step, a):
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    return torch.tensor([LR / bc1, 1.0 / math.sqrt(bc2), GSCALE, a], dtype=torch.float32).cuda()


def _old_entry(form, p, g, m, v, step, max_norm, hyper4, scratch):
    n = p.numel()
    if form == "host":
        return lib.tdx_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, B1, B2, EPS, step, GSCALE,
                                 _st())
    if form == "dev":   # reads the first three floats
        return lib.tdx_adam_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, hyper4.data_ptr(), B1, B2,
                                     EPS, _st())
    return lib.tdx_adam_step_clip(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, B1, B2, EPS, step, GSCALE,
                                  max_norm, hyper4.data_ptr() if form == "clip_dev" else None, scratch.data_ptr(), _st())


def _new_entry(form, p, g, m, v, e, step, max_norm, a, hyper4, scratch):
    n = p.numel()
    bufs = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr())
    if form == "host":
        return lib.tdx_adam_ema_step(*bufs, n, LR, B1, B2, EPS, step, GSCALE, a, _st())
    if form == "dev":
        return lib.tdx_adam_ema_step_dev(*bufs, n, hyper4.data_ptr(), B1, B2, EPS, _st())
    return lib.tdx_adam_ema_step_clip(*bufs, n, LR, B1, B2, EPS, step, GSCALE, max_norm, a,
                                      hyper4.data_ptr() if form == "clip_dev" else None, scratch.data_ptr(), _st())


@pytest.mark.parametrize("n,misaligned", SIZES)
@pytest.mark.parametrize("form", FORMS)
def test_fused_kernel_bitwise_against_existing_entry_and_torch(form, n, misaligned):
    p0, g0, m0, v0, e0 = _data(n)
    scratch = torch.empty(lib.tdx_adam_clip_scratch_bytes(), dtype=torch.uint8, device="cuda")
    gnorm = g0.double().norm().item() * GSCALE
    # the clip forms: one threshold that clips (half the norm of the averaged gradient), one that does not
    norms = (0.5 * gnorm, 2.0 * gnorm) if form.startswith("clip") else (0.0,)
    for max_norm in norms:
        for decay in DECAYS:
            a = 1.0 - decay
            a_t = torch.tensor(a, dtype=torch.float32).cuda()
            p, g, m, v, e = (_view(t, misaligned) for t in (p0, g0, m0, v0, e0))
            pr, gr, mr, vr, er = (_view(t, misaligned) for t in (p0, g0, m0, v0, e0))
            for step in (1, 2, 3):
                hyper4 = _hyper(step, a)
                check(_new_entry(form, p, g, m, v, e, step, max_norm, a, hyper4, scratch), "new entry")
                check(_old_entry(form, pr, gr, mr, vr, step, max_norm, hyper4, scratch), "existing entry")
                d = pr - er
                d = a_t * d
                er = er + d
                where = (form, n, misaligned, max_norm, decay, step)
                assert torch.equal(p, pr), where
                assert torch.equal(m, mr), where
                assert torch.equal(v, vr), where
                assert torch.equal(e, er), where
                assert torch.equal(g, g0), where
            if decay == 1.0:
                assert torch.equal(e, e0), (form, n, misaligned)
            else:
                assert not torch.equal(e, e0), (form, n, misaligned)


def test_fused_entries_refuse_bad_arguments():
    p, g, m, v, e = (t.clone() for t in _data(1027))
    scratch = torch.empty(lib.tdx_adam_clip_scratch_bytes(), dtype=torch.uint8, device="cuda")
    h = _hyper(1, 0.1)
    ptrs = [t.data_ptr() for t in (p, g, m, v, e)]
    n = 1027
    for i in range(5):
        bad = list(ptrs)
        bad[i] = None
        assert lib.tdx_adam_ema_step(*bad, n, LR, B1, B2, EPS, 1, 1.0, 0.1, _st()) == TDX_E_BADARG
        assert lib.tdx_adam_ema_step_dev(*bad, n, h.data_ptr(), B1, B2, EPS, _st()) == TDX_E_BADARG
        assert lib.tdx_adam_ema_step_clip(*bad, n, LR, B1, B2, EPS, 1, 1.0, 1.0, 0.1, None, scratch.data_ptr(),
                                          _st()) == TDX_E_BADARG
    assert lib.tdx_adam_ema_step_dev(*ptrs, n, None, B1, B2, EPS, _st()) == TDX_E_BADARG
    assert lib.tdx_adam_ema_step(*ptrs, 0, LR, B1, B2, EPS, 1, 1.0, 0.1, _st()) == TDX_E_BADARG
    for a in (-0.1, 1.5, float("nan")):
        assert lib.tdx_adam_ema_step(*ptrs, n, LR, B1, B2, EPS, 1, 1.0, a, _st()) == TDX_E_BADARG
        assert lib.tdx_adam_ema_step_clip(*ptrs, n, LR, B1, B2, EPS, 1, 1.0, 1.0, a, None, scratch.data_ptr(),
                                          _st()) == TDX_E_BADARG
    alias = ptrs[:4] + [ptrs[0]]
    assert lib.tdx_adam_ema_step(*alias, n, LR, B1, B2, EPS, 1, 1.0, 0.1, _st()) == TDX_E_BADARG
    assert lib.tdx_adam_ema_step_dev(*alias, n, h.data_ptr(), B1, B2, EPS, _st()) == TDX_E_BADARG
    assert lib.tdx_adam_ema_step_clip(*alias, n, LR, B1, B2, EPS, 1, 1.0, 1.0, 0.1, None, scratch.data_ptr(),
                                      _st()) == TDX_E_BADARG
    torch.cuda.synchronize()
    for t, t0 in zip((p, g, m, v, e), _data(1027)):
        assert torch.equal(t, t0)   # a refused call launches nothing


@pytest.mark.parametrize("n,misaligned", SIZES)
def test_swap_exchanges_bits_and_twice_restores(n, misaligned):
    p0, _, _, _, e0 = _data(n)
    a, b = _view(p0, misaligned), _view(e0, misaligned)
    check(lib.tdx_swap_f32(a.data_ptr(), b.data_ptr(), n, _st()), "tdx_swap_f32")
    assert torch.equal(a, e0) and torch.equal(b, p0)
    check(lib.tdx_swap_f32(a.data_ptr(), b.data_ptr(), n, _st()), "tdx_swap_f32")
    assert torch.equal(a, p0) and torch.equal(b, e0)


def test_swap_refuses_aliases_and_overlap():
    buf = torch.arange(64, dtype=torch.float32, device="cuda")
    keep = buf.clone()
    assert lib.tdx_swap_f32(buf.data_ptr(), buf.data_ptr(), 16, _st()) == TDX_E_BADARG
    assert lib.tdx_swap_f32(buf.data_ptr(), buf[8:].data_ptr(), 16, _st()) == TDX_E_BADARG
    assert lib.tdx_swap_f32(buf[8:].data_ptr(), buf.data_ptr(), 16, _st()) == TDX_E_BADARG
    assert lib.tdx_swap_f32(None, buf.data_ptr(), 16, _st()) == TDX_E_BADARG
    assert lib.tdx_swap_f32(buf.data_ptr(), buf[16:].data_ptr(), 0, _st()) == TDX_E_BADARG
    check(lib.tdx_swap_f32(buf.data_ptr(), buf[16:].data_ptr(), 16, _st()), "adjacent ranges")   # touching is fine
    assert torch.equal(buf[:16], keep[16:32]) and torch.equal(buf[16:32], keep[:16]) and torch.equal(buf[32:], keep[32:])


# ------------------------------------------------------------------ TrainStep
T_STEPS = 20
N_STEPS = 5


def _cond_model(seed=0):
    from tiny_diffusion_amd.conditional_diffusion import NoiseModel

    m = NoiseModel()
    m.load_state_dict(make_state_dict(seed, True), strict=True)
    return m.cuda()


def _latent_model(seed=0):
    from tiny_diffusion_amd.latent_diffusion import NoiseModel

    m = NoiseModel()
    m.load_state_dict(make_state_dict_latent(seed), strict=True)
    return m.cuda()


CASES = {
    "eager": dict(kind="cond", B=8, kw=dict(ema_decay=0.9)),
    "eager_clip": dict(kind="cond", B=8, kw=dict(ema_decay=0.9, max_grad_norm=10.0)),
    "graph_warmup": dict(kind="cond", B=8, kw=dict(ema_decay=0.9999, ema_warmup=True, use_graph=True)),
    "latent": dict(kind="latent", B=32, kw=dict(ema_decay=0.9)),
}


def _train(case):
    """N_STEPS steps; returns (step, model, initial parameters, the parameter snapshot after every step)."""
    from tiny_diffusion_amd.schedule import ForwardProcess
    from tiny_diffusion_amd.train import TrainStep

    c = CASES[case]
    B = c["B"]
    model = (_cond_model() if c["kind"] == "cond" else _latent_model()).train()
    fp = ForwardProcess(num_timesteps=T_STEPS)
    step = TrainStep(model, fp, lr=1e-3, **c["kw"])
    p0 = step.flat_param.clone()
    assert torch.equal(step.ema, p0) and step.ema.data_ptr() != step.flat_param.data_ptr()
    g = torch.Generator().manual_seed(11)
    shape = (B, 1, 28, 28) if c["kind"] == "cond" else (B, 20)
    x0 = (torch.rand(*shape, generator=g) * 2 - 1).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    snaps = []
    for _ in range(N_STEPS):
        if c["kw"].get("use_graph"):
            step.step(x0, y)    # t and the noise are drawn inside the captured step
        else:
            t = torch.randint(0, T_STEPS, (B,), generator=g).cuda()
            noise = torch.randn(*shape, generator=g).cuda()
            step.step(x0, y, t=t, noise=noise)
        snaps.append(step.flat_param.clone())
    if c["kw"].get("use_graph"):
        assert step._graph is not None and step._hyper.numel() == 4
    return step, model, p0, snaps


def _recurrence(p0, snaps, decay, warmup):
    from tiny_diffusion_amd.train import ema_decay_at

    e = p0.clone()
    for k, p in enumerate(snaps):
        a_t = torch.tensor(1.0 - ema_decay_at(k, decay, warmup), dtype=torch.float32).cuda()
        d = p - e
        d = a_t * d
        e = e + d
    return e


@pytest.fixture(scope="module")
def trained():
    """The five eager steps at decay 0.9 on the conditional MNIST UNet, shared by the tests below (which leave the
    step as they found it)."""
    return _train("eager")


def test_train_step_keeps_the_recurrence_eager(trained):
    step, _, p0, snaps = trained
    assert not torch.equal(snaps[-1], p0) and not torch.equal(snaps[-1], snaps[-2])
    assert torch.equal(step.ema, _recurrence(p0, snaps, 0.9, False))
    assert not torch.equal(step.ema, step.flat_param)


@pytest.mark.parametrize("case", ["eager_clip", "graph_warmup", "latent"])
def test_train_step_keeps_the_recurrence(case):
    step, _, p0, snaps = _train(case)
    kw = CASES[case]["kw"]
    assert not torch.equal(snaps[-1], snaps[-2])
    want = _recurrence(p0, snaps, kw["ema_decay"], kw.get("ema_warmup", False))
    assert torch.equal(step.ema, want)
    if case == "graph_warmup":
        # the decay a captured step would keep if 1 - decay froze at its capture (step index 1) gives another average
        from tiny_diffusion_amd.train import ema_decay_at
        frozen = p0.clone()
        for k, p in enumerate(snaps):
            a_t = torch.tensor(1.0 - ema_decay_at(min(k, 1), 0.9999, True), dtype=torch.float32).cuda()
            frozen = frozen + a_t * (p - frozen)
        assert not torch.equal(frozen, want)


def test_without_ema_decay_nothing_is_allocated():
    from tiny_diffusion_amd.schedule import ForwardProcess
    from tiny_diffusion_amd.train import TrainStep

    model = _cond_model().train()
    step = TrainStep(model, ForwardProcess(num_timesteps=T_STEPS), lr=1e-3, use_graph=True)
    assert step.ema is None and step.ema_decay is None
    g = torch.Generator().manual_seed(2)
    x0 = (torch.rand(8, 1, 28, 28, generator=g) * 2 - 1).cuda()
    y = torch.randint(0, 10, (8,), generator=g).cuda()
    for _ in range(3):
        step.step(x0, y)
    assert step._graph is not None and step._hyper.numel() == 3
    for call in (step.reset_ema, step.ema_state_dict, lambda: step.load_ema_state_dict({}),
                 lambda: step.ema_weights().__enter__()):
        with pytest.raises(RuntimeError, match="ema_decay"):
            call()


def _second_model(step):
    m2 = type(step.model)()
    m2.load_state_dict(step.ema_state_dict(), strict=True)
    return m2.cuda().eval()


def _xty():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 1, 28, 28, generator=g).cuda()
    t = torch.randint(0, T_STEPS, (8,), generator=g).cuda()
    y = torch.randint(0, 10, (8,), generator=g).cuda()
    return x, t, y


def test_ema_weights_swaps_what_the_kernels_read(trained):
    step, model, _, _ = trained
    m2 = _second_model(step)
    x, t, y = _xty()
    model.eval()
    ema_sd = step.ema_state_dict()
    before = step.flat_param.clone()
    ema_before = step.ema.clone()
    with torch.no_grad():
        out_raw = model(x, t, y)     # also warms the inference packs: a stale pack would show below
        out_ema = m2(x, t, y)
        assert not torch.equal(out_raw, out_ema)
        with step.ema_weights() as inside:
            assert inside is model
            got = model(x, t, y)
            assert torch.equal(got, out_ema)
            assert not torch.equal(got, out_raw)
            sd = model.state_dict()
            for k in step.offsets:
                assert torch.equal(sd[k], ema_sd[k]), k
            with pytest.raises(RuntimeError):
                step.step(x, y)
            with pytest.raises(RuntimeError):
                with step.ema_weights():
                    pass
            assert torch.equal(model(x, t, y), out_ema)    # neither refusal disturbed the swap
        assert torch.equal(step.flat_param, before) and torch.equal(step.ema, ema_before)
        assert torch.equal(model(x, t, y), out_raw)
        with pytest.raises(KeyError, match="boom"):
            with step.ema_weights():
                assert torch.equal(step.flat_param, ema_before)
                raise KeyError("boom")
        assert torch.equal(step.flat_param, before) and torch.equal(step.ema, ema_before)
        assert torch.equal(model(x, t, y), out_raw)
    model.train()


def test_sampling_from_the_average(trained):
    from tiny_diffusion_amd.conditional_diffusion import ddim_sample, sample
    from tiny_diffusion_amd.schedule import ForwardProcess

    step, model, _, _ = trained
    m2 = _second_model(step)
    fp = ForwardProcess(num_timesteps=T_STEPS)
    g = torch.Generator().manual_seed(9)
    x_T = torch.randn(4, 1, 28, 28, generator=g)
    noises = torch.randn(T_STEPS, 4, 1, 28, 28, generator=g)
    y = torch.randint(0, 10, (4,), generator=g).cuda()
    before = step.flat_param.clone()
    raw = sample(model, fp, "cuda", n_samples=4, y=y, x_T=x_T, noises=noises)
    want = sample(m2, fp, "cuda", n_samples=4, y=y, x_T=x_T, noises=noises)
    with step.ema_weights():
        got = sample(model, fp, "cuda", n_samples=4, y=y, x_T=x_T, noises=noises)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert not torch.equal(got, raw)
    kw = dict(n_samples=4, y=y, x_T=x_T, noises=noises, steps=5, guidance_scale=2.0)
    want = ddim_sample(m2, fp, "cuda", **kw)
    with step.ema_weights():
        got = ddim_sample(model, fp, "cuda", **kw)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert torch.equal(step.flat_param, before)
    assert torch.equal(sample(model, fp, "cuda", n_samples=4, y=y, x_T=x_T, noises=noises), raw)
    model.train()


def test_state_dict_round_trip(trained):
    step, model, _, _ = trained
    live = model.state_dict()
    sd = step.ema_state_dict()
    assert list(sd.keys()) == list(live.keys())
    for k, v in live.items():
        assert sd[k].shape == v.shape and sd[k].dtype == v.dtype and sd[k].device == v.device, k
        assert sd[k].data_ptr() != v.data_ptr(), k
        if k in step.offsets:
            lo, hi = step.offsets[k]
            assert torch.equal(sd[k].reshape(-1), step.ema[lo:hi]), k
        else:
            assert torch.equal(sd[k], v), k     # BatchNorm buffers: the live ones
    assert any(k not in step.offsets for k in live) and not torch.equal(step.ema, step.flat_param)
    saved = step.ema.clone()
    step.ema.zero_()
    step.load_ema_state_dict(sd)
    assert torch.equal(step.ema, saved)
    step.reset_ema()
    assert torch.equal(step.ema, step.flat_param)
    step.load_ema_state_dict(sd)     # leave the shared step as it was
    assert torch.equal(step.ema, saved)
