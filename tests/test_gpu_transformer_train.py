"""Transformer training on the MI355X: ``tdx_transformer_loss_grads`` against the fp64 restatement of the step
(tests/transformer_train_helpers.py) with the dropout masks rebuilt by the existing ``ops.dropout``;
``TransformerTrainStep`` against the module's own op-by-op path, against the vectors of the reference's own
``NoiseModel`` + ``torch.optim.Adam`` (tests/golden/transformer_train_B16.npz), v-prediction with min-SNR weights,
captured = eager, determinism, ``evaluate``, the average, the module contract, and that training trains.

Bounds are test_gpu_transformer.py's: eps_hat relative MSE < 1e-10, loss within 2e-5, per-parameter gradient error
<= max(10 x the CPU-fp32 restatement's error against fp64, 1e-4); parameters after Adam steps: test_gpu_latent.py's
MAX_DIFF / LOOSE_SHARE."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transformer_train_helpers as H
from oracle.weights import make_state_dict_transformer

pytestmark = pytest.mark.gpu

MAX_DIFF, LOOSE_SHARE = 2.1e-3, 5e-3     # test_gpu_latent.py::test_latent_train_step's two parameter bounds
T = 1000


def rel_mse(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b) ** 2).mean().item() / max((b ** 2).mean().item(), 1e-30)


def build(sd=None, seed=0, **kw):
    from tiny_diffusion_amd.diffusion_transformer import NoiseModel

    torch.manual_seed(seed)
    m = NoiseModel(**kw)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.cuda()


def default_model(**kw):
    return build(make_state_dict_transformer(0), **kw)


def params_of(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def make_inputs(B, Ld, seed, ncls=10):
    """t holds 0 and T - 1, y repeats a label and never holds class ncls - 1."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, Ld, generator=g)
    noise = torch.randn(B, Ld, generator=g)
    t = torch.randint(0, T, (B,), generator=g)
    t[0], t[1] = 0, T - 1
    y = torch.randint(0, ncls - 1, (B,), generator=g)
    y[1] = y[0]
    return z, t, y, noise


def check_against_fp64(sd_cpu, heads, inputs, masks, got_loss, got_eps, got_grads, w_table=None, what=""):
    """The bounds of this file's docstring; returns the measured figures."""
    z_t, t, y, target = (v.cpu() for v in inputs)
    l64, e64, g64 = H.loss_grads(sd_cpu, z_t, t, y, target, heads, torch.float64, masks, w_table)
    _, _, g32 = H.loss_grads(sd_cpu, z_t, t, y, target, heads, torch.float32, masks, w_table)
    fig = {"eps": rel_mse(got_eps, e64), "loss": abs(float(got_loss) - float(l64)) / float(l64), "grad": {}}
    print(f"{what}: eps_hat rel. MSE {fig['eps']:.3g}, loss rel. err {fig['loss']:.3g}")
    assert fig["eps"] < 1e-10, (what, fig["eps"])
    assert fig["loss"] <= 2e-5, (what, fig["loss"])
    for k in sd_cpu:
        got = got_grads[k].detach().double().cpu()
        n64 = g64[k].norm().item()
        err = (got - g64[k]).norm().item() / max(n64, 1e-30)
        err32 = (g32[k].double() - g64[k]).norm().item() / max(n64, 1e-30)
        fig["grad"][k] = (err, err32)
        assert err <= max(10 * err32, 1e-4), (what, k, err, err32)
        if k.endswith("in_proj_weight") or k.endswith("in_proj_bias"):
            n = got.shape[0] // 3
            assert float(got[:2 * n].abs().max()) == 0.0, (what, k)      # Q, K: exactly zero
        if k == "class_embedding.weight":
            absent = [c for c in range(got.shape[0]) if c not in set(y.tolist())]
            assert absent and float(got[absent].abs().max()) == 0.0, what
    worst = max(fig["grad"].items(), key=lambda kv: kv[1][0])
    print(f"{what}: worst gradient {worst[0]} err {worst[1][0]:.3g} (fp32 CPU {worst[1][1]:.3g})")
    return fig


# ------------------------------------------------------------------ 1. the C entry
class Call:
    """tdx_transformer_loss_grads on a module's own parameter tensors, gradients into fresh buffers filled with junk."""

    def __init__(self, m, B, p):
        from tiny_diffusion_amd._lib import lib
        from tiny_diffusion_amd.diffusion_transformer import _TShape

        self.lib = lib
        blk = m.transformer_blocks[0]
        self.shape = _TShape(B, m.latent_dim, m.time_dim, blk.num_heads, len(m.transformer_blocks),
                             m.class_embedding.num_embeddings, p, 1e-5)
        self.sd = {k: v.detach().contiguous() for k, v in m.state_dict().items()}
        n = len(self.sd)
        self.P = (C.c_void_p * n)(*[v.data_ptr() for v in self.sd.values()])
        self.ws = torch.empty(lib.tdx_transformer_train_workspace_floats(C.byref(self.shape)), device="cuda")
        assert self.ws.numel() > 0 and n == 12 + 12 * len(m.transformer_blocks)
        self.B, self.Ld = B, m.latent_dim

    def __call__(self, z_t, t, y, target, train=1, seed=0, offset=0, rng_dev=None, w=None, grads=True):
        from tiny_diffusion_amd._lib import check

        g = {k: torch.full_like(v, 7.0) for k, v in self.sd.items()}
        G = (C.c_void_p * len(g))(*[v.data_ptr() for v in g.values()])
        loss = torch.full((1,), -1.0, device="cuda")
        eps = torch.full((self.B, self.Ld), 7.0, device="cuda")
        check(self.lib.tdx_transformer_loss_grads(
            C.byref(self.shape), self.P, G if grads else None, z_t.data_ptr(), t.data_ptr(), y.data_ptr(),
            target.data_ptr(), None if w is None else w.data_ptr(), train, seed, offset,
            None if rng_dev is None else rng_dev.data_ptr(), 1.0, loss.data_ptr(), eps.data_ptr(), self.ws.data_ptr(),
            None), "tdx_transformer_loss_grads")
        torch.cuda.synchronize()
        return loss, eps, g


CASES = [(5, 64, 4, 1, 20, 0.0), (33, 192, 4, 2, 20, 0.05), (16, 256, 4, 4, 20, 0.5), (3, 1024, 8, 1, 7, 0.05),
         (128, 256, 4, 4, 20, 0.05)]


@pytest.mark.parametrize("B,dim,heads,L,Ld,p", CASES)
def test_loss_grads_vs_fp64(B, dim, heads, L, Ld, p):
    m = build(seed=B + dim, time_dim=dim, num_heads=heads, num_layers=L, latent_dim=Ld, dropout=p)
    z, t, y, noise = make_inputs(B, Ld, 7 * B + L)
    inp = tuple(v.cuda() for v in (z, t, y, noise))
    call = Call(m, B, p)
    sd_cpu = {k: v.cpu() for k, v in call.sd.items()}
    seed = 0x1234567 + B
    loss, eps, g = call(*inp, train=1, seed=seed, offset=0)
    masks = H.site_masks(seed, 0, B, dim, heads, L, p)
    check_against_fp64(sd_cpu, heads, inp, masks, loss.item(), eps, g, what=f"case {(B, dim, heads, L, Ld, p)}")
    # forward only: the same loss and eps_hat bits, no gradient pointer needed
    loss_f, eps_f, _ = call(*inp, train=1, seed=seed, offset=0, grads=False)
    assert torch.equal(loss_f, loss) and torch.equal(eps_f, eps)
    # another offset: other masks (checked against fp64 too), and {seed, offset} read from the device give the same bits
    off = 4 * L + 3
    loss_o, eps_o, g_o = call(*inp, train=1, seed=seed, offset=off)
    rng_dev = torch.tensor([seed, off], dtype=torch.int64, device="cuda")
    loss_d, eps_d, g_d = call(*inp, train=1, seed=99, offset=1, rng_dev=rng_dev)
    assert torch.equal(loss_o, loss_d) and torch.equal(eps_o, eps_d)
    assert all(torch.equal(g_o[k], g_d[k]) for k in g_o)
    if p > 0:
        assert not torch.equal(eps_o, eps)
        check_against_fp64(sd_cpu, heads, inp, H.site_masks(seed, off, B, dim, heads, L, p), loss_o.item(), eps_o, g_o,
                           what=f"case {(B, dim, heads, L, Ld, p)} offset {off}")
    # train = 0: no dropout whatever p says
    loss_e, eps_e, g_e = call(*inp, train=0, seed=seed, offset=0)
    if p > 0:
        check_against_fp64(sd_cpu, heads, inp, None, loss_e.item(), eps_e, g_e, what="eval")
    else:
        assert torch.equal(eps_e, eps) and torch.equal(loss_e, loss)


# ------------------------------------------------------------------ 2. the step against the module's own path
def test_step_matches_the_modules_own_path():
    from tiny_diffusion_amd.diffusion_transformer import ForwardProcess, TransformerTrainStep

    fp = ForwardProcess()
    B, seed = 16, 4242
    z0, t, y, noise = (v.cuda() for v in make_inputs(B, 20, 5))
    z_t, _ = fp.q_sample("cuda", z0, t, noise=noise)
    m = default_model().train()           # p = 0.05
    sd_cpu = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    torch.manual_seed(seed)
    eps_mod = m(z_t, t, y)
    loss_mod = F.mse_loss(eps_mod, noise)
    loss_mod.backward()
    g_mod = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    torch.manual_seed(seed)
    key = int(torch.randint(0, 2 ** 62, (1,)).item())
    m2 = default_model().train()
    ts = TransformerTrainStep(m2, fp, lr=0.0)          # lr 0: the update leaves the parameters where they are
    torch.manual_seed(seed)
    loss = ts.step(z0, y, t, noise).clone()
    assert (ts.last_dropout_seed, ts.last_dropout_offset) == (key, 0) and ts.step_count == 1
    assert all(torch.equal(v.cpu(), sd_cpu[k]) for k, v in m2.state_dict().items())
    eps_step = torch.empty(B, 20, device="cuda")
    ts._loss_grads(z_t, t, y, noise, B, torch.empty(1, device="cuda"), False, True, (key, 0), eps_hat=eps_step)
    masks = H.site_masks(key, 0, B, 256, 4, 4, 0.05)
    inp = (z_t, t, y, noise)
    check_against_fp64(sd_cpu, 4, inp, masks, loss.item(), eps_step, ts.grad_views, what="fused step")
    check_against_fp64(sd_cpu, 4, inp, masks, loss_mod.item(), eps_mod.detach(), g_mod, what="module path")
    assert rel_mse(eps_step, eps_mod.detach()) < 1e-10


# ------------------------------------------------------------------ 3. three Adam steps on the reference's vectors
def fed_forward():
    """A forward process that hands the step the fixture's z_t as it is (the fixture records z_t, not z_0)."""
    from tiny_diffusion_amd.diffusion_transformer import ForwardProcess

    class Fed(ForwardProcess):
        def q_sample(self, device, x_0, t, noise=None):
            return x_0.contiguous().float(), noise.contiguous().float()

    return Fed()


@functools.lru_cache(maxsize=None)
def fixture_runs(golden_dir):
    d = np.load(os.path.join(golden_dir, "transformer_train_B16.npz"))
    src = np.load(os.path.join(golden_dir, "transformer_B16.npz"))
    z_t, t, y, noise = (torch.from_numpy(src[k]) for k in ("z_t", "t", "y", "noise"))
    inputs = [(z_t + float(d["pert_scale"]) * torch.from_numpy(d["pert"][k]), t, y, noise) for k in range(3)]
    l32, o32 = H.train_steps(make_state_dict_transformer(0), inputs, dtype=torch.float32, lr=1e-3)
    return d, inputs, l32, o32


def test_three_adam_steps_match_the_reference(golden_dir):
    """Loss bound: 2e-6 relative, loosened per step to 8 x the CPU-fp32 restatement's own distance from the recorded
    loss where that is larger (steps 2 and 3 run on parameters that three sign-like Adam updates have moved: the
    restatement itself is 4e-6 / 3.5e-6 from the reference there)."""
    from tiny_diffusion_amd.diffusion_transformer import TransformerTrainStep

    d, inputs, l32, o32 = fixture_runs(golden_dir)
    sd0 = make_state_dict_transformer(0)
    m = default_model(dropout=0.0).train()
    ts = TransformerTrainStep(m, fed_forward(), lr=1e-3)
    losses = [ts.step(z.cuda(), y.cuda(), t.cuda(), n.cuda()).item() for z, t, y, n in inputs]
    assert ts.step_count == 3
    for k, (got, want) in enumerate(zip(losses, d["losses"])):
        bound = max(2e-6, 8 * abs(l32[k] - want) / want)
        print(f"step {k + 1}: loss {got:.9g} recorded {want:.9g} rel. err {abs(got - want) / want:.3g} bound {bound:.3g}")
        assert abs(got - want) <= bound * want, (losses, d["losses"])
    got = params_of(m)
    heads = []
    for k in sd0:
        diff = (got[k].cpu() - o32.p[k]).abs()
        assert diff.max().item() <= MAX_DIFF, (k, diff.max().item())
        assert (diff > 1e-5).float().mean().item() <= LOOSE_SHARE, k
        head = torch.from_numpy(d["phead__" + k.replace(".", "__")])
        heads.append((got[k].reshape(-1)[: head.numel()].cpu() - head).abs())
        if k.endswith("in_proj_weight") or k.endswith("in_proj_bias"):
            n = sd0[k].shape[0] // 3
            assert torch.equal(got[k][:2 * n].cpu(), sd0[k][:2 * n]), k      # zero gradient: bit-unchanged
    heads = torch.cat(heads)
    assert heads.max().item() <= MAX_DIFF and (heads > 1e-5).float().mean().item() <= LOOSE_SHARE


# ------------------------------------------------------------------ 4. v-prediction, min-SNR
def test_v_prediction_min_snr_and_set_objective():
    from tiny_diffusion_amd.diffusion_transformer import ForwardProcess, TransformerTrainStep
    from tiny_diffusion_amd.schedule import loss_weights

    fp = ForwardProcess()
    B = 16
    z0, t, y, noise = (v.cuda() for v in make_inputs(B, 20, 9))
    m = default_model(dropout=0.0).train()
    sd_cpu = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    ts = TransformerTrainStep(m, fp, lr=0.0, prediction="v", loss_weighting="min_snr")
    loss = ts.step(z0, y, t, noise).clone()
    z_t, v = fp.q_sample_target("cuda", z0, t, noise=noise, prediction="v")
    acp = fp.alphas_cumprod.double()[t.cpu()].unsqueeze(-1)
    v64 = acp.sqrt() * noise.double().cpu() - (1 - acp).sqrt() * z0.double().cpu()
    assert rel_mse(v, v64) < 1e-12
    eps_hat = torch.empty(B, 20, device="cuda")
    ts._loss_grads(z_t, t, y, v, B, torch.empty(1, device="cuda"), False, True, (0, 0), eps_hat=eps_hat)
    w = loss_weights(fp, "v", "min_snr", 5.0)
    check_against_fp64(sd_cpu, 4, (z_t, t, y, v), None, loss.item(), eps_hat, ts.grad_views, w_table=w, what="v + min-SNR")
    g_v = {k: g.clone() for k, g in ts.grad_views.items()}
    # back to the defaults: the default step's bits
    ts.set_objective()
    loss_b = ts.step(z0, y, t, noise).clone()
    ts0 = TransformerTrainStep(default_model(dropout=0.0).train(), fp, lr=0.0)
    loss_0 = ts0.step(z0, y, t, noise).clone()
    assert torch.equal(loss_b, loss_0) and not torch.equal(loss_b, loss)
    assert all(torch.equal(ts.grad_views[k], ts0.grad_views[k]) for k in g_v)
    assert not torch.equal(g_v["final_layer.1.weight"], ts0.grad_views["final_layer.1.weight"])
    with pytest.raises(ValueError):
        ts.set_objective(prediction="x0")


# ------------------------------------------------------------------ 5. / 6. graph and determinism
def _run_steps(n_steps, use_graph=False, give=True, B=16, seed=77, **kw):
    from tiny_diffusion_amd.diffusion_transformer import ForwardProcess, TransformerTrainStep

    m = default_model().train()           # dropout 0.05 on
    ts = TransformerTrainStep(m, ForwardProcess(), lr=1e-3, use_graph=use_graph, **kw)
    torch.manual_seed(seed)
    losses, seeds = [], []
    for i in range(n_steps):
        z0, t, y, noise = (v.cuda() for v in make_inputs(B, 20, 100 + i))
        losses.append((ts.step(z0, y, t, noise) if give else ts.step(z0, y)).clone())
        seeds.append((ts.last_dropout_seed, ts.last_dropout_offset))
    assert ts.step_count == n_steps
    state = dict(params_of(m), exp_avg=ts.exp_avg.clone(), exp_avg_sq=ts.exp_avg_sq.clone())
    if ts.ema is not None:
        state["ema"] = ts.ema.clone()
    return torch.stack(losses), state, seeds, ts


@pytest.mark.parametrize("max_grad_norm,give", [(None, True), (0.05, True), (None, False)])
def test_captured_step_equals_eager(max_grad_norm, give):
    kw = dict(max_grad_norm=max_grad_norm, ema_decay=0.99, ema_warmup=True, give=give)
    le, se, seeds_e, ts_e = _run_steps(4, **kw)
    lg, sg, seeds_g, ts = _run_steps(4, use_graph=True, **kw)      # warm, capture, two replays
    assert ts._graph is not None and seeds_e == seeds_g
    if max_grad_norm is not None:
        assert ts_e.flat_grad.double().norm().item() > 2 * max_grad_norm     # the clip binds
    assert torch.equal(le, lg), (le, lg)
    for k in se:
        assert torch.equal(se[k], sg[k]), k
    assert not torch.equal(se["ema"], ts.flat_param)
    # two replays on the same inputs draw different masks: a per-step key (or offset) reaches the captured kernels
    z0, t, y, noise = (v.cuda() for v in make_inputs(16, 20, 300))
    a = ts.step(z0, y, t, noise).clone()
    sa = (ts.last_dropout_seed, ts.last_dropout_offset)
    ts.lr = 0.0          # read at every step, through the device scalars of a captured one: this replay moves nothing
    before = ts.flat_param.clone()
    b = ts.step(z0, y, t, noise).clone()
    assert sa != (ts.last_dropout_seed, ts.last_dropout_offset) and not torch.equal(a, b)
    assert torch.equal(before, ts.flat_param) and ts.step_count == 6


def test_fixed_dropout_seed_offsets_and_graph():
    le, se, seeds_e, _ = _run_steps(4, dropout_seed=2 ** 63 + 5)
    lg, sg, seeds_g, ts = _run_steps(4, use_graph=True, dropout_seed=2 ** 63 + 5)
    assert seeds_e == seeds_g == [(2 ** 63 + 5, 16 * i) for i in range(4)]
    assert ts._graph is not None and torch.equal(le, lg) and all(torch.equal(se[k], sg[k]) for k in se)


def test_captured_step_owns_its_workspace():
    """The graph holds the raw address of the batch size's workspace and replays never look it up again, while
    ``evaluate()`` at other batch sizes goes through the step's small workspace cache: whatever that cache evicts, the
    captured step's workspace stays allocated and the replays stay bit-identical to the eager step."""
    le, se, _, _ = _run_steps(5)
    from tiny_diffusion_amd.diffusion_transformer import ForwardProcess, TransformerTrainStep

    m = default_model().train()
    ts = TransformerTrainStep(m, ForwardProcess(), lr=1e-3, use_graph=True)
    torch.manual_seed(77)
    batches = [tuple(v.cuda() for v in make_inputs(16, 20, 100 + i)) for i in range(5)]
    step = lambda b: ts.step(b[0], b[2], b[1], b[3]).clone()      # noqa: E731
    losses = [step(b) for b in batches[:3]]                        # warm, capture, one replay
    assert ts._graph is not None and ts._gws is not None
    ws_ptr, ws_numel = ts._gws.data_ptr(), ts._gws.numel()
    for B in (2, 3, 5, 6, 7, 9, 10):                               # seven other batch sizes: the cache holds four
        z0, t, y, noise = (v.cuda() for v in make_inputs(B, 20, 40 + B))
        assert torch.isfinite(ts.evaluate(z0, y, t, noise))
    assert len(ts._ws) <= 4
    assert ts._gws.data_ptr() == ws_ptr and ts._gws.numel() == ws_numel and ts._ws.get(16) is ts._gws
    filler = [torch.full((ws_numel,), float("nan"), device="cuda") for _ in range(4)]   # would land in a freed block
    losses += [step(b) for b in batches[3:]]                       # two more replays
    assert all(f.data_ptr() != ws_ptr for f in filler) and all(bool(torch.isnan(f).all()) for f in filler)
    assert ts.step_count == 5 and torch.equal(torch.stack(losses), le)
    got = params_of(m)
    assert all(torch.equal(got[k], se[k]) for k in got)
    # a step at another batch size drops the graph (and its hold on the workspace); coming back captures again
    z0, t, y, noise = (v.cuda() for v in make_inputs(4, 20, 41))
    ts.step(z0, y)
    assert ts._graph is None and ts._gws is None
    for _ in range(3):
        assert torch.isfinite(ts.step(batches[0][0], batches[0][2])).all()
    assert ts._graph is not None and ts._gws is not None and ts._ws.get(16) is ts._gws


def test_steps_are_deterministic():
    l1, s1, k1, _ = _run_steps(3, give=False)
    l2, s2, k2, _ = _run_steps(3, give=False)
    assert k1 == k2 and torch.equal(l1, l2) and all(torch.equal(s1[k], s2[k]) for k in s1)
    l3, s3, _, _ = _run_steps(2, give=False, philox_seed=7)
    l4, s4, _, _ = _run_steps(2, give=False, philox_seed=7)
    assert torch.equal(l3, l4) and all(torch.equal(s3[k], s4[k]) for k in s3)
    l5, _, _, _ = _run_steps(2, give=False, philox_seed=8)
    assert not torch.equal(l3, l5)
    l6, _, k6, _ = _run_steps(3, give=False, seed=78)
    assert k6 != k1 and not torch.equal(l6, l1)


# ------------------------------------------------------------------ 7. evaluate
def test_evaluate_is_the_dropout_free_loss_and_changes_nothing():
    from tiny_diffusion_amd.diffusion_transformer import ForwardProcess, TransformerTrainStep

    fp = ForwardProcess()
    m = default_model().train()           # train mode: evaluate() still runs without dropout
    ts = TransformerTrainStep(m, fp, lr=1e-3, ema_decay=0.9)
    z0, t, y, noise = (v.cuda() for v in make_inputs(16, 20, 3))
    ts.step(z0, y, t, noise)
    before = dict(params_of(m), g=ts.flat_grad.clone(), m1=ts.exp_avg.clone(), m2=ts.exp_avg_sq.clone(), e=ts.ema.clone())
    state = torch.get_rng_state()
    got = ts.evaluate(z0, y, t, noise)
    assert got.shape == () and torch.equal(torch.get_rng_state(), state)
    after = dict(params_of(m), g=ts.flat_grad.clone(), m1=ts.exp_avg.clone(), m2=ts.exp_avg_sq.clone(), e=ts.ema.clone())
    assert ts.step_count == 1 and all(torch.equal(before[k], after[k]) for k in before)
    z_t, _ = fp.q_sample("cuda", z0, t, noise=noise)
    sd_cpu = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    l64, _, _ = H.loss_grads(sd_cpu, z_t.cpu(), t.cpu(), y.cpu(), noise.cpu(), 4, torch.float64)
    assert abs(got.item() - float(l64)) <= 2e-5 * float(l64)
    m.eval()
    with torch.no_grad():
        want = F.mse_loss(m(z_t, t, y), noise).item()
    assert abs(got.item() - want) <= 2e-5 * want
    assert torch.equal(ts.evaluate(z0, y, t, noise), got)       # eval mode: the same launches
    assert torch.isfinite(ts.evaluate(z0, y))                   # t and the noise drawn as the validation loop draws them


# ------------------------------------------------------------------ 8. EMA
def test_ema_follows_the_host_recurrence():
    from tiny_diffusion_amd.diffusion_transformer import ForwardProcess, TransformerTrainStep, ema_decay_at

    m = default_model().train()
    ts = TransformerTrainStep(m, ForwardProcess(), lr=1e-3, ema_decay=0.5, ema_warmup=True)
    e = ts.flat_param.clone()
    assert torch.equal(ts.ema, e)
    for k in range(6):       # (1 + k) / (10 + k) passes 0.5 at k = 8: warm-up all the way, 0.1 .. 0.4
        z0, t, y, noise = (v.cuda() for v in make_inputs(16, 20, 50 + k))
        ts.step(z0, y, t, noise)
        a = torch.tensor(1.0 - ema_decay_at(k, 0.5, True), dtype=torch.float32).item()
        e = e + a * (ts.flat_param - e)
        assert torch.equal(ts.ema, e), k
    ts2 = TransformerTrainStep(default_model().train(), ForwardProcess(), lr=1e-3, ema_decay=0.25)
    e = ts2.flat_param.clone()
    z0, t, y, noise = (v.cuda() for v in make_inputs(16, 20, 50))
    ts2.step(z0, y, t, noise)
    assert torch.equal(ts2.ema, e + 0.75 * (ts2.flat_param - e))
    # ema_weights(): the module is the averaged model inside, the live one again outside
    live, avg = ts.flat_param.clone(), ts.ema.clone()
    sd_avg = ts.ema_state_dict()
    with ts.ema_weights() as mm:
        assert mm is m and torch.equal(ts.flat_param, avg) and torch.equal(ts.ema, live)
        assert all(torch.equal(v, sd_avg[k]) for k, v in m.state_dict().items())
        with pytest.raises(RuntimeError):
            ts.step(z0, y, t, noise)
        with pytest.raises(RuntimeError):
            with ts.ema_weights():
                pass
    assert torch.equal(ts.flat_param, live) and torch.equal(ts.ema, avg) and ts.step_count == 6
    ts.reset_ema()
    assert torch.equal(ts.ema, live)
    ts.load_ema_state_dict(sd_avg)
    assert torch.equal(ts.ema, avg)
    with pytest.raises(RuntimeError):
        TransformerTrainStep(default_model(), ForwardProcess()).ema_state_dict()


# ------------------------------------------------------------------ 9. module contract
def test_module_contract():
    from tiny_diffusion_amd import _lib
    from tiny_diffusion_amd.diffusion_transformer import ForwardProcess, TransformerTrainStep

    m = default_model().train()
    ts = TransformerTrainStep(m, ForwardProcess(), lr=1e-3)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    assert list(sd0) == list(ts.offsets) and ts.flat_param.numel() == sum(v.numel() for v in sd0.values())
    z0, t, y, noise = (v.cuda() for v in make_inputs(16, 20, 1))
    ts.step(z0, y, t, noise)
    assert not torch.equal(m.final_layer[1].weight, sd0["final_layer.1.weight"])
    m.load_state_dict(make_state_dict_transformer(1), strict=True)       # in-place copies land in the flat buffer
    lo, hi = ts.offsets["final_layer.1.weight"]
    assert torch.equal(ts.flat_param[lo:hi].cpu(), make_state_dict_transformer(1)["final_layer.1.weight"].reshape(-1))
    m.load_state_dict(sd0, strict=True)
    assert all(torch.equal(v, sd0[k]) for k, v in m.state_dict().items())
    ts._check_attached()
    # the samplers still see the module: an inference forward on the trained weights
    m.eval()
    with torch.no_grad():
        assert torch.isfinite(m(z0, t, y)).all()
    m.train()
    for bad in ((z0.cpu(), y, t, noise), (z0, y.cpu(), t, noise), (z0, y, t.cpu(), noise), (z0, y, t, noise.cpu())):
        with pytest.raises(_lib.TdxError):
            ts.step(*bad)
    for bad in ((z0[:, :19], y, t, noise), (z0, y[:3], t, noise), (z0, y.float(), t, noise), (z0, y, t, noise[:4])):
        with pytest.raises(ValueError):
            ts.step(*bad)
    assert ts.step_count == 1
    m.cpu()
    with pytest.raises(_lib.TdxError, match="flat parameter buffer"):
        ts.step(z0, y, t, noise)
    with pytest.raises(_lib.TdxError, match="flat parameter buffer"):
        ts.evaluate(z0, y, t, noise)


# ------------------------------------------------------------------ 10. training trains
def test_fifty_steps_reduce_the_loss():
    from tiny_diffusion_amd.diffusion_transformer import ForwardProcess, TransformerTrainStep, cosine_annealing_lr

    torch.manual_seed(0)
    m = build(seed=3).train()             # the default model, default initialisation, dropout 0.05
    ts = TransformerTrainStep(m, ForwardProcess(), lr=1e-3, max_grad_norm=1.0, ema_decay=0.99)
    z0, t, y, noise = (v.cuda() for v in make_inputs(128, 20, 8))
    losses = []
    for k in range(50):
        ts.lr = cosine_annealing_lr(k, 1e-3, 100)
        losses.append(ts.step(z0, y, t, noise).clone())
    losses = torch.stack(losses).cpu().reshape(-1)
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(ts.flat_param).all())
    assert losses[-5:].mean().item() < 0.8 * losses[:5].mean().item(), losses
