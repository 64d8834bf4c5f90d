"""VAE training on the MI355X: the BCE-from-logits, KLD / reparameterisation-backward and Philox reparameterisation
kernels against fp64, ``tdx_vae_loss_grads`` through ``VAETrainStep`` against the fp64 restatement of the step
(tests/vae_helpers.py) and against the vectors of the reference's own ``VAE`` / ``loss_function``
(tests/golden/vae_train_B8.npz), eager = captured, determinism, ``evaluate``, and that the inference entries did not move.

Measured on MI355X (relative L2 error per parameter gradient / relative error of the loss, GPU vs fp64; the bound is
8 x the fp32 CPU restatement's error against the same fp64): see DESIGN.md 3.11."""
import functools
import os

import numpy as np
import pytest
import torch

import vae_helpers as H
from oracle.weights import make_state_dict_vae

pytestmark = pytest.mark.gpu

SPECIAL_LOGITS = (0.0, -0.0, 20.0, -20.0, 30.0, -30.0)
MAX_DIFF, LOOSE_SHARE = 2.1e-3, 5e-3     # test_gpu_latent.py::test_latent_train_step's two parameter bounds


def _lib():
    from tiny_diffusion_amd._lib import check, lib

    return lib, check


def _scratch():
    lib, _ = _lib()
    return torch.empty(lib.tdx_vae_loss_scratch_bytes(), dtype=torch.uint8, device="cuda")


def build(sd=None, cfg=None):
    from tiny_diffusion_amd.vae import VAE, VAEConfig

    v = VAE(cfg or VAEConfig())
    v.load_state_dict(make_state_dict_vae(0) if sd is None else sd, strict=True)
    return v.cuda()


def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "vae_train_B8.npz"))


def params_of(vae):
    return {k: v.detach().clone() for k, v in vae.state_dict().items()}


# ------------------------------------------------------------------ 1. BCE from logits
def _bce_inputs(n):
    g = torch.Generator().manual_seed(100 + n)
    a = torch.rand(n, generator=g) * 60 - 30
    sp = torch.tensor(SPECIAL_LOGITS)
    k = min(n, sp.numel())
    a[:k] = sp.roll(n % sp.numel())[:k]          # n = 3, 4 take different specials; the larger sizes all six
    x = torch.rand(n, generator=g) * 2 - 1
    return a, x


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("n", [3, 4, 1036, 1037, 8 * 784])     # 1037: a float4 body AND a tail
def test_bce_logits_kernel_vs_fp64(n, gscale):
    lib, check = _lib()
    a, x = _bce_inputs(n)
    a64, t64 = a.double(), (x.double() + 1) / 2
    want_sum = (a64.clamp(min=0) - a64 * t64 + torch.log1p(torch.exp(-a64.abs()))).sum().item()
    want_d = gscale * (torch.sigmoid(a64) - t64)
    want_r = torch.sigmoid(a64)
    scratch = _scratch()
    # 16-byte aligned buffers (the float4 body + scalar tail) and the same data one float further (the scalar kernel)
    for shift in (0, 1):
        buf = lambda v: torch.cat([torch.zeros(shift), v]).cuda()[shift:]   # noqa: E731
        ad, xd = buf(a), buf(x)
        d, r = buf(torch.full((n + 2,), 7.0)), buf(torch.full((n + 2,), 7.0))
        loss = torch.zeros(2, device="cuda")
        check(lib.tdx_vae_bce_logits_grad(ad.data_ptr(), xd.data_ptr(), loss.data_ptr(), d.data_ptr(), r.data_ptr(),
                                          gscale, n, scratch.data_ptr(), None), "bce")
        got_sum, got_d, got_r = loss[0].item(), d[:n].double().cpu(), r[:n].double().cpu()
        e_d, e_r = (got_d - want_d).abs().max().item(), (got_r - want_r).abs().max().item()
        e_s = abs(got_sum - want_sum) / want_sum
        print(f"bce n={n} gscale={gscale} shift={shift}: |d_a| err {e_d:.2e}, recon err {e_r:.2e}, sum rel {e_s:.2e}")
        assert torch.isfinite(d[:n]).all() and torch.isfinite(r[:n]).all() and np.isfinite(got_sum)
        assert e_d <= 5e-7 and e_r <= 5e-7 and e_s <= 1e-6
        assert bool((d[n:] == 7.0).all()) and bool((r[n:] == 7.0).all()) and loss[1].item() == 0.0   # nothing past n
        # bit-identical over two launches; and the sum does not depend on which outputs are asked for
        loss2, d2 = torch.zeros(1, device="cuda"), torch.empty_like(d)
        check(lib.tdx_vae_bce_logits_grad(ad.data_ptr(), xd.data_ptr(), loss2.data_ptr(), d2.data_ptr(), None, gscale, n,
                                          scratch.data_ptr(), None), "bce")
        assert torch.equal(loss2, loss[:1]) and torch.equal(d2[:n], d[:n])
        loss3 = torch.zeros(1, device="cuda")
        check(lib.tdx_vae_bce_logits_grad(ad.data_ptr(), xd.data_ptr(), loss3.data_ptr(), None, None, gscale, n,
                                          scratch.data_ptr(), None), "bce")
        assert torch.equal(loss3, loss[:1])


# ------------------------------------------------------------------ 2. KLD + reparameterisation backward
@pytest.mark.parametrize("with_gz", [True, False])
@pytest.mark.parametrize("beta", [1.0, 0.25])
@pytest.mark.parametrize("n", [3, 20, 1036])
def test_kld_reparam_bwd_kernel_vs_fp64(n, beta, with_gz):
    lib, check = _lib()
    g = torch.Generator().manual_seed(200 + n)
    mu = torch.randn(n, generator=g) * 1.5
    logvar = torch.rand(n, generator=g) * 10 - 6
    logvar[0], logvar[1] = -6.0, 4.0
    eps = torch.randn(n, generator=g)
    gz = torch.randn(n, generator=g) * 3
    m64, l64, e64, g64 = mu.double(), logvar.double(), eps.double(), gz.double()
    want_sum = (-0.5 * (1 + l64 - m64 ** 2 - l64.exp())).sum().item()
    want_gmu = g64 + beta * m64
    want_glv = 0.5 * g64 * e64 * torch.exp(0.5 * l64) + 0.5 * beta * (l64.exp() - 1)
    scratch = _scratch()
    mud, lvd, epd, gzd = mu.cuda(), logvar.cuda(), eps.cuda(), gz.cuda()
    outs = []
    for _ in range(2):
        kld = torch.zeros(2, device="cuda")
        gmu, glv = torch.full((n + 1,), 7.0, device="cuda"), torch.full((n + 1,), 7.0, device="cuda")
        check(lib.tdx_vae_kld_reparam_bwd(mud.data_ptr(), lvd.data_ptr(), epd.data_ptr() if with_gz else None,
                                          gzd.data_ptr() if with_gz else None, kld.data_ptr(),
                                          gmu.data_ptr() if with_gz else None, glv.data_ptr() if with_gz else None, beta, n,
                                          scratch.data_ptr(), None), "kld")
        outs.append((kld, gmu, glv))
    (kld, gmu, glv), (kld2, gmu2, glv2) = outs
    e_s = abs(kld[0].item() - want_sum) / want_sum
    print(f"kld n={n} beta={beta} g_z={with_gz}: sum rel {e_s:.2e}")
    assert e_s <= 1e-6 and kld[1].item() == 0.0
    assert torch.equal(kld, kld2)                                 # bit-identical over two launches
    if with_gz:
        for got, want in ((gmu, want_gmu), (glv, want_glv)):
            err = (got[:n].double().cpu() - want).abs()
            assert bool((err <= 1e-6 * want.abs() + 1e-6).all()), (err / (1e-6 * want.abs() + 1e-6)).max().item()
            assert got[n].item() == 7.0
        assert torch.equal(gmu, gmu2) and torch.equal(glv, glv2)
    else:
        assert bool((gmu == 7.0).all()) and bool((glv == 7.0).all())   # the sum only: nothing else is written


# ------------------------------------------------------------------ 3. Philox reparameterisation
def test_reparameterize_philox():
    lib, check = _lib()
    n = 20480
    g = torch.Generator().manual_seed(3)
    mu, logvar = torch.randn(n, generator=g).cuda(), (torch.rand(n, generator=g) * 6 - 4).cuda()

    def run(seed, offset, count=n):
        z, e = torch.full((n,), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
        check(lib.tdx_vae_reparameterize_philox(mu.data_ptr(), logvar.data_ptr(), z.data_ptr(), e.data_ptr(), count, seed,
                                                offset, None), "reparam_philox")
        return z, e

    z, e = run(5, 9)
    z2, e2 = run(5, 9)
    assert torch.equal(z, z2) and torch.equal(e, e2)
    z3, e3 = run(5, 10)
    assert not torch.equal(e, e3) and (e != e3).float().mean().item() > 0.99
    z4, e4 = run(6, 9)
    assert (e != e4).float().mean().item() > 0.99
    want = mu.double() + e.double() * torch.exp(0.5 * logvar.double())
    assert torch.allclose(z.double(), want, rtol=1e-6, atol=1e-6)
    ed = e.double()
    mean, var = ed.mean().item(), ed.var(unbiased=False).item()
    print(f"philox eps n={n}: mean {mean:.4f} var {var:.4f}")
    assert torch.isfinite(e).all()
    assert abs(mean) < 5 / np.sqrt(n) and abs(var - 1) < 5 * np.sqrt(2 / n)
    # n no multiple of 4: the same stream, exactly n elements written
    z5, e5 = run(5, 9, count=15)
    assert torch.equal(e5[:15], e[:15]) and torch.equal(z5[:15], z[:15])
    assert bool((e5[15:] == 7.0).all()) and bool((z5[15:] == 7.0).all())


# ------------------------------------------------------------------ 4. the whole step against fp64
CASES = {
    # name: (seed, B, (input_dim, hidden_dim, latent_dim) or None for the default model with oracle weights, kld_weight)
    "fixture_B8": (11, 8, None, 1.0),
    "B1": (12, 1, None, 1.0),
    "B33": (21, 33, None, 1.0),          # crosses the GEMM's 32-row tile (seed 12 puts a pre-activation at 7e-6)
    "odd_50_36_5_B3": (12, 3, (50, 36, 5), 1.0),
    "kld_weight_0.25": (11, 8, None, 0.25),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs, weights and the CPU restatement in fp64 and fp32 - computed once per case, never modified."""
    seed, B, dims, beta = CASES[name]
    if dims is None:
        sd, dims = make_state_dict_vae(0), (784, 400, 20)
    else:
        sd = H.default_init_state_dict(seed, *dims)
    x, eps = H.recipe_inputs(seed, B, dims[0], dims[2])
    r64 = H.loss_and_grads(sd, x, eps, beta, torch.float64, "logits")
    r32 = H.loss_and_grads(sd, x, eps, beta, torch.float32, "sigmoid")
    return sd, dims, x, eps, beta, r64, r32


@pytest.mark.parametrize("name", list(CASES))
def test_loss_grads_vs_fp64_restatement(name):
    from tiny_diffusion_amd.vae import VAEConfig, VAETrainStep

    sd, dims, x, eps, beta, r64, r32 = reference(name)
    margin, max_logit, _ = H.input_margins(r64["aux"])
    assert margin >= 1e-4 and max_logit <= 15, (margin, max_logit)   # a flipped mask cannot hide behind the tolerance
    vae = build(sd, VAEConfig(input_dim=dims[0], hidden_dim=dims[1], latent_dim=dims[2]))
    ts = VAETrainStep(vae, kld_weight=beta)
    loss = ts.step(x.cuda(), eps.cuda())
    got = dict(loss=loss.item(), bce=ts.bce.item(), kld=ts.kld.item())
    bad = []
    for k in ("loss", "bce", "kld"):
        e_gpu, e_cpu = H.rel_err(got[k], r64[k]), H.rel_err(r32[k], r64[k])
        print(f"{name} {k}: gpu {e_gpu:.2e} cpu32 {e_cpu:.2e}")
        if not e_gpu <= 8 * e_cpu:
            bad.append((k, e_gpu, e_cpu))
    for k in H.KEYS:
        e_gpu, e_cpu = H.rel_l2(ts.grad_views[k], r64["grads"][k]), H.rel_l2(r32["grads"][k], r64["grads"][k])
        print(f"{name} grad {k}: gpu {e_gpu:.2e} cpu32 {e_cpu:.2e}")
        if not e_gpu <= 8 * e_cpu:
            bad.append((k, e_gpu, e_cpu))
    assert not bad, bad


# ------------------------------------------------------------------ 5. the reference's numbers
def test_one_step_gradients_match_the_reference(golden_dir):
    from tiny_diffusion_amd.vae import VAETrainStep

    d = fixture(golden_dir)
    ts = VAETrainStep(build())
    loss = ts.step(torch.from_numpy(d["x"]).cuda(), torch.from_numpy(d["eps"][0]).cuda())
    for k, got in (("loss", loss), ("bce", ts.bce), ("kld", ts.kld)):
        assert H.rel_err(got.item(), float(d[k])) <= 2e-6, k
    for k in H.KEYS:
        kk = k.replace(".", "__")
        g = ts.grad_views[k].reshape(-1).cpu()
        gn = float(d[f"gnorm__{kk}"])
        assert abs(g.double().norm().item() - gn) <= 1e-5 * gn, k
        head = torch.from_numpy(d[f"ghead__{kk}"])
        rtol, atol = H.head_tolerance(gn, g.numel())
        assert torch.allclose(g[: head.numel()], head, rtol=rtol, atol=atol), k


def _assert_params_close(got, want, what):
    for k in H.KEYS:
        diff = (got[k].cpu() - want[k]).abs()
        assert diff.max().item() <= MAX_DIFF, (what, k, diff.max().item())
        share = (diff > 1e-5).float().mean().item()
        assert share <= LOOSE_SHARE, (what, k, share)


def test_three_adam_steps_match_the_reference(golden_dir):
    from tiny_diffusion_amd.vae import VAETrainStep

    d = fixture(golden_dir)
    vae = build()
    ts = VAETrainStep(vae, lr=1e-3)
    x, eps = torch.from_numpy(d["x"]).cuda(), torch.from_numpy(d["eps"]).cuda()
    losses = [ts.step(x, eps[i]).item() for i in range(3)]
    assert ts.step_count == 3
    for got, want in zip(losses, d["adam_losses"]):
        assert abs(got - want) <= 2e-6 * want, (losses, d["adam_losses"])
    got = params_of(vae)
    # every element against the fp32 restatement (which test_vae_train_host.py holds to the reference's vectors) ...
    _, want = H.adam_steps(make_state_dict_vae(0), torch.from_numpy(d["x"]), list(torch.from_numpy(d["eps"])), lr=1e-3)
    _assert_params_close(got, want, "restatement")
    # ... and the recorded heads of the reference's own parameters
    diffs = []
    for k in H.KEYS:
        head = torch.from_numpy(d["phead__" + k.replace(".", "__")])
        diffs.append((got[k].reshape(-1)[: head.numel()].cpu() - head).abs())
    diffs = torch.cat(diffs)      # 10 x 64 recorded elements: the same two bounds over all of them
    assert diffs.max().item() <= MAX_DIFF and (diffs > 1e-5).float().mean().item() <= LOOSE_SHARE


# ------------------------------------------------------------------ 6. / 7. graph and determinism
def _run_steps(n_steps, use_graph=False, philox_seed=None, give_eps=True, **kw):
    from tiny_diffusion_amd.vae import VAETrainStep

    vae = build()
    ts = VAETrainStep(vae, use_graph=use_graph, philox_seed=philox_seed, **kw)
    x, eps = H.recipe_inputs(11, 8, n_eps=n_steps)
    if n_steps == 1:
        eps = [eps]
    losses = [ts.step(x.cuda(), eps[i].cuda() if give_eps else None).clone() for i in range(n_steps)]
    assert ts.step_count == n_steps
    return torch.stack(losses), params_of(vae), ts


@pytest.mark.parametrize("max_grad_norm", [None, 50.0])     # 50 < the gradient norm of these steps: the clip binds
def test_captured_step_equals_eager(max_grad_norm):
    le, pe, _ = _run_steps(4, max_grad_norm=max_grad_norm)
    lg, pg, ts = _run_steps(4, use_graph=True, max_grad_norm=max_grad_norm)     # warm, capture, two replays
    assert ts._graph is not None
    assert torch.equal(le, lg), (le, lg)
    for k in H.KEYS:
        assert torch.equal(pe[k], pg[k]), k
    # without eps the captured step draws into its static buffer before the replay: finite, and it moves the parameters
    before = params_of(ts.vae)
    assert torch.isfinite(ts.step(H.recipe_inputs(11, 8)[0].cuda())).all() and ts.step_count == 5
    assert not torch.equal(before["fc4.weight"], ts.vae.fc4.weight)


def test_captured_step_owns_its_workspace():
    """The graph holds the raw address of the batch size's workspace and replays never look it up again, while
    ``evaluate()`` at other batch sizes goes through the step's small workspace cache: whatever that cache evicts, the
    captured step's workspace stays allocated and the replays stay bit-identical to the eager step."""
    le, pe, _ = _run_steps(5)
    from tiny_diffusion_amd.vae import VAETrainStep

    vae = build()
    ts = VAETrainStep(vae, use_graph=True)
    x, eps = H.recipe_inputs(11, 8, n_eps=5)
    xd = x.cuda()
    losses = [ts.step(xd, eps[i].cuda()).clone() for i in range(3)]            # warm, capture, one replay
    assert ts._graph is not None and ts._gws is not None
    ws_ptr, ws_numel = ts._gws.data_ptr(), ts._gws.numel()
    for B in (1, 2, 3, 5, 6, 7, 9):                                             # seven other batch sizes: the cache holds four
        xe, ee = H.recipe_inputs(40 + B, B)
        assert all(torch.isfinite(v) for v in ts.evaluate(xe.cuda(), ee.cuda()))
    assert len(ts._ws) <= 4
    assert ts._gws.data_ptr() == ws_ptr and ts._gws.numel() == ws_numel and ts._ws.get(8) is ts._gws
    filler = [torch.full((ws_numel,), float("nan"), device="cuda") for _ in range(4)]   # would land in a freed block
    losses += [ts.step(xd, eps[i].cuda()).clone() for i in range(3, 5)]         # two more replays
    assert all(f.data_ptr() != ws_ptr for f in filler) and all(bool(torch.isnan(f).all()) for f in filler)
    assert ts.step_count == 5 and torch.equal(torch.stack(losses), le)
    got = params_of(vae)
    for k in H.KEYS:
        assert torch.equal(got[k], pe[k]), k
    # a step at another batch size drops the graph (and its hold on the workspace); coming back captures again
    ts.step(H.recipe_inputs(41, 4)[0].cuda())
    assert ts._graph is None and ts._gws is None
    for _ in range(3):
        assert torch.isfinite(ts.step(xd)).all()
    assert ts._graph is not None and ts._gws is not None and ts._ws.get(8) is ts._gws


def test_steps_are_deterministic():
    l1, p1, _ = _run_steps(2)
    l2, p2, _ = _run_steps(2)
    assert torch.equal(l1, l2) and all(torch.equal(p1[k], p2[k]) for k in H.KEYS)
    l3, p3, _ = _run_steps(2, philox_seed=7, give_eps=False)
    l4, p4, _ = _run_steps(2, philox_seed=7, give_eps=False)
    assert torch.equal(l3, l4) and all(torch.equal(p3[k], p4[k]) for k in H.KEYS)
    l5, _, _ = _run_steps(2, philox_seed=8, give_eps=False)
    assert not torch.equal(l3, l5) and not torch.equal(l3, l1)


# ------------------------------------------------------------------ 8. evaluate
def test_evaluate_is_the_steps_loss_and_changes_nothing():
    from tiny_diffusion_amd.vae import VAETrainStep

    vae = build()
    ts = VAETrainStep(vae, kld_weight=0.5)
    x, eps = H.recipe_inputs(11, 8, n_eps=2)
    x, eps = x.cuda(), [e.cuda() for e in eps]
    ts.step(x, eps[0])        # so that gradients and moments are not all zero
    state = [t.clone() for t in (ts.flat_param, ts.flat_grad, ts.exp_avg, ts.exp_avg_sq)]
    loss, bce, kld = ts.evaluate(x.view(8, 1, 28, 28), eps[1])
    assert ts.step_count == 1
    for before, now in zip(state, (ts.flat_param, ts.flat_grad, ts.exp_avg, ts.exp_avg_sq)):
        assert torch.equal(before, now)
    assert loss.dim() == 0 and H.rel_err(loss.item(), bce.item() + 0.5 * kld.item()) <= 2e-7
    got = ts.step(x, eps[1])
    assert torch.equal(got, loss) and torch.equal(ts.bce, bce) and torch.equal(ts.kld, kld)
    # torch.randn noise when none is given: finite, and again nothing moves
    state = [t.clone() for t in (ts.flat_param, ts.flat_grad, ts.exp_avg, ts.exp_avg_sq)]
    assert all(torch.isfinite(v) for v in ts.evaluate(x)) and ts.step_count == 2
    for before, now in zip(state, (ts.flat_param, ts.flat_grad, ts.exp_avg, ts.exp_avg_sq)):
        assert torch.equal(before, now)


# ------------------------------------------------------------------ 9. nothing else moved
def test_module_contract_around_the_step(golden_dir):
    from tiny_diffusion_amd import _lib as L
    from tiny_diffusion_amd.vae import VAETrainStep

    d = fixture(golden_dir)
    x, eps = torch.from_numpy(d["x"]).cuda(), torch.from_numpy(d["eps"]).cuda()
    vae = build()

    def inference():
        mu, logvar = vae.encode(x)
        z = vae.reparameterize(mu, logvar, eps=eps[0])
        return mu, logvar, z, vae.decode(z)

    before = inference()
    ts = VAETrainStep(vae, max_grad_norm=1.0)
    for a, b in zip(before, inference()):
        assert torch.equal(a, b)
    ref = make_state_dict_vae(0)
    sd = vae.state_dict()
    assert list(sd) == list(ref) == list(H.KEYS)
    for k in ref:
        assert tuple(sd[k].shape) == tuple(ref[k].shape) and sd[k].dtype == ref[k].dtype
        assert torch.equal(sd[k].cpu(), ref[k])
    # clip_grad_norm_(1.0) + Adam against the restatement (the gradient norm here is 6.2e3: the clip binds)
    loss = ts.step(x, eps[0])
    losses, want = H.adam_steps(ref, x.cpu(), [eps[0].cpu()], lr=1e-3, max_grad_norm=1.0)
    assert H.rel_err(loss.item(), losses[0]) <= 2e-6
    _assert_params_close(params_of(vae), want, "clip")
    # load_state_dict after construction lands in the flat buffer: the next step sees it
    sd1 = make_state_dict_vae(1)
    vae.load_state_dict(sd1)
    assert vae.fc1.weight.data_ptr() == ts.flat_param.data_ptr()
    got = ts.step(x, eps[1]).clone()
    fresh = VAETrainStep(build(sd1), max_grad_norm=1.0)
    assert torch.equal(got, fresh.step(x, eps[1]))
    # shapes and devices
    with pytest.raises(ValueError, match="eps"):
        ts.step(x, eps[0][:, :19])
    with pytest.raises(L.TdxError):
        ts.step(x.cpu(), eps[0])
    n = ts.step_count
    # a moved module is detached from the flat buffer: a clear error, not a silent step on stale weights
    vae.cpu()
    with pytest.raises(L.TdxError, match="flat parameter buffer"):
        ts.step(x, eps[0])
    assert ts.step_count == n


# ------------------------------------------------------------------ 10. it trains
def test_fifty_steps_reduce_the_loss():
    from tiny_diffusion_amd.vae import VAETrainStep

    x, _ = H.recipe_inputs(14, 32)
    ts = VAETrainStep(build(), lr=1e-3, philox_seed=3)
    xd = x.cuda()
    losses = torch.stack([ts.step(xd).clone() for _ in range(50)]).cpu()
    g = torch.Generator().manual_seed(3)
    cpu, _ = H.adam_steps(make_state_dict_vae(0), x, [torch.randn(32, 20, generator=g) for _ in range(50)], lr=1e-3)
    print(f"50 steps B=32: gpu {losses[0].item():.2f} -> {losses[-1].item():.2f}; cpu32 restatement (its own noise) "
          f"{cpu[0]:.2f} -> {cpu[-1]:.2f}")
    assert torch.isfinite(losses).all() and losses[-1].item() < losses[0].item()
