"""Classifier-free guidance on the device: the null condition (label -1 / a zero text embedding) in the forward and
the backward, condition dropout for training, and guided sampling - one step and whole chains against a fp64
restatement, consistency with the unguided chain (same noise stream), fused = unfused update, ``guidance_scale=None``
is the existing path, nothing stale between calls.

fp64 yardstick: oracle.ref_cpu / oracle.ref_laion in double.  For the null label the tests append one zero row to
their own copy of ``class_embedding.weight`` and map -1 -> num_classes."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oracle import ref_laion as RLA  # noqa: E402
from oracle.weights import make_state_dict, make_state_dict_laion  # noqa: E402
from parity_helpers import gpu_pool_routing, gpu_relu_masks, grad_precision_failures, rel_mse  # noqa: E402

from tiny_diffusion_amd._lib import check, lib, tuned  # noqa: E402
from tiny_diffusion_amd.schedule import GRAPH_STEPS, ForwardProcess, ddim_schedule, sample_loop  # noqa: E402

NUM_CLASSES = 10
SHAPES = {"cond": (1, 28, 28), "laion": (4, 32, 32)}
MODES = {"eager": dict(use_graph=False), "graph": dict(use_graph=True), "philox": dict(use_graph=True, philox_seed=7)}
CHAIN_TOL = 1e-8    # the project's chain tolerance (test_gpu_ddim.py: relative MSE against fp64)


def _amp(w):
    """How e = eps_u + w (eps_c - eps_u) = w eps_c + (1 - w) eps_u amplifies an error in either prediction
    (squared: the tolerances are mean squares)."""
    return (abs(w) + abs(w - 1.0)) ** 2


def _model(kind, seed=0, time_dim=None):
    if kind == "cond":
        from tiny_diffusion_amd.conditional_diffusion import NoiseModel
        m = NoiseModel() if time_dim is None else NoiseModel(time_dim=time_dim)
        m.load_state_dict(make_state_dict(seed, True, **({} if time_dim is None else dict(time_dim=time_dim))), strict=True)
    else:
        from tiny_diffusion_amd.conditional_diffusion_laion import NoiseModel
        m = NoiseModel(time_dim=768)
        m.load_state_dict(make_state_dict_laion(seed), strict=True)
    return m.cuda()


def _inputs(kind, n, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    x_T = torch.randn(n, *SHAPES[kind], generator=g)
    zs = torch.randn(T, n, *SHAPES[kind], generator=g)
    y = torch.randn(n, 768, generator=g).cuda() if kind == "laion" else torch.randint(0, NUM_CLASSES, (n,), generator=g).cuda()
    return x_T, zs, y


def _null(kind, y):
    return torch.zeros_like(y) if kind == "laion" else torch.full_like(y, -1)


def _extended_state(seed, time_dim=None):
    """The conditional MNIST state dict with one zero row appended to class_embedding.weight: label -1 -> row 10."""
    sd = make_state_dict(seed, True, **({} if time_dim is None else dict(time_dim=time_dim)))
    w = sd["class_embedding.weight"]
    sd["class_embedding.weight"] = torch.cat([w, torch.zeros(1, w.shape[1], dtype=w.dtype)])
    return sd


def _map_null(y):
    y = y.cpu()
    return torch.where(y < 0, torch.full_like(y, NUM_CLASSES), y)


def _fp64_forward(kind, seed, time_dim=None):
    """fwd(x, t, y[, training]) in double; y may hold -1 (cond) or zero rows (laion)."""
    sd = make_state_dict_laion(seed) if kind == "laion" else _extended_state(seed, time_dim)
    p, b = R.split_state(sd)
    p = {k: v.double() for k, v in p.items()}

    def fwd(x, t, y, training=False):
        bb = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in b.items()}
        with torch.no_grad():
            if kind == "laion":
                return RLA.unet_forward(p, bb, x.double(), t, y.cpu().double(), training=training)
            return R.unet_forward(p, bb, x.double(), t, None if y is None else _map_null(y), training=training)
    return fwd


def _guided_eps64(fwd, kind, x, t, y, w):
    """eps_u + w (eps_c - eps_u) in fp64; w = 1 and w = 0 are eps_c and eps_u exactly, so only that one is run."""
    if w == 1.0:
        return fwd(x, t, y)
    if w == 0.0:
        return fwd(x, t, _null(kind, y))
    n = x.shape[0]
    e = fwd(torch.cat([x, x]), torch.cat([t, t]), torch.cat([y, _null(kind, y)]))
    return e[n:] + w * (e[:n] - e[n:])


# ---------------------------------------------------------------- 1. null condition, forward
@pytest.mark.parametrize("time_dim", [256, 64])
def test_null_condition_forward(time_dim):
    B = 5
    g = torch.Generator().manual_seed(time_dim)
    x = torch.randn(B, 1, 28, 28, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    fwd = _fp64_forward("cond", 5, time_dim)
    m = _model("cond", 5, time_dim)
    # train mode last: its forwards move the BatchNorm running statistics the eval modes read (the oracle keeps the
    # loaded ones)
    for mode in ("infer", "eval_grad", "train"):
        for y in (torch.tensor([3, -1, 0, -1, 9]), torch.full((B,), -1)):
            m.train(mode == "train")
            with torch.set_grad_enabled(mode != "infer"):
                got = m(x.cuda(), t.cuda(), y.cuda()).detach()
            want = fwd(x, t, y, training=mode == "train")
            r = rel_mse(got, want)
            print(f"null forward time_dim={time_dim} y={y.tolist()} {mode}: relative MSE vs fp64 {r:.3e}")
            assert r < 1e-10, (mode, r)
            if (y < 0).all():   # no condition at all: the time embedding alone
                assert rel_mse(got, fwd(x, t, None, training=mode == "train")) < 1e-10


# ---------------------------------------------------------------- 2. null condition, backward
@pytest.mark.parametrize("time_dim,training", [(256, True), (64, False)])
def test_null_condition_backward(time_dim, training):
    """Tolerance and tie handling of test_gpu_unet.py::test_backward_vs_oracle_full_tensors, on the extended state dict."""
    B = 5
    g = torch.Generator().manual_seed(40 + time_dim)
    x = torch.randn(B, 1, 28, 28, generator=g)
    noise = torch.randn(B, 1, 28, 28, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    y = torch.tensor([3, -1, 0, -1, 3])
    sd = _extended_state(2, time_dim)
    m = _model("cond", 2, time_dim)
    m.train(training)
    loss = F.mse_loss(m(x.cuda(), t.cuda(), y.cuda()), noise.cuda())
    loss.backward()
    cpu_args = (sd, x, t, noise, _map_null(y))
    pidx = gpu_pool_routing(m, B, cpu_args, training)
    masks, _ = gpu_relu_masks(m, B, cpu_args, training, pool_idx=pidx)
    kw = dict(training=training, pool_idx=pidx, relu_masks=masks)
    loss_ref, _, g32, _ = R.train_step_grads(*cpu_args, **kw)
    _, _, g64, _ = R.train_step_grads(*cpu_args, dtype=torch.float64, **kw)
    assert abs(loss.item() - loss_ref.item()) < 2e-5 * loss_ref.item()
    for gd in (g32, g64):   # the gradient of the appended zero row is not the model's
        gd["class_embedding.weight"] = gd["class_embedding.weight"][:NUM_CLASSES]
    bad = grad_precision_failures({k: p.grad for k, p in m.named_parameters()}, g32, g64, training)
    assert not bad, bad
    ge = m.class_embedding.weight.grad
    absent = [c for c in range(NUM_CLASSES) if c not in y.tolist()]
    assert torch.equal(ge[absent], torch.zeros_like(ge[absent]))   # a null row feeds no class
    assert ge[3].abs().max() > 0 and ge[0].abs().max() > 0


# ---------------------------------------------------------------- 3. condition dropout
def _drop_labels(y, p, seed, offset, out=None):
    out = torch.empty_like(y) if out is None else out
    check(lib.tdx_cond_drop_labels(y.data_ptr(), out.data_ptr(), y.shape[0], p, seed, offset,
                                   torch.cuda.current_stream().cuda_stream))
    return out


def _drop_rows(c, p, seed, offset, out=None):
    out = torch.empty_like(c) if out is None else out
    check(lib.tdx_cond_drop_rows(c.data_ptr(), out.data_ptr(), c.shape[0], c.shape[1], p, seed, offset,
                                 torch.cuda.current_stream().cuda_stream))
    return out


def test_cond_drop_kernel():
    B, dim, p = 4096, 24, 0.25
    g = torch.Generator().manual_seed(1)
    y = torch.randint(0, NUM_CLASSES, (B,), generator=g).cuda()
    c = (torch.rand(B, dim, generator=g) + 0.5).cuda()    # no zero entry: a zero row is a dropped row
    assert torch.equal(_drop_labels(y, 0.0, 5, 9), y) and torch.equal(_drop_rows(c, 0.0, 5, 9), c)
    assert (_drop_labels(y, 1.0, 5, 9) == -1).all() and (_drop_rows(c, 1.0, 5, 9) == 0).all()
    a = _drop_labels(y, p, 5, 9)
    mask = a == -1
    assert torch.equal(a[~mask], y[~mask])
    assert torch.equal(_drop_labels(y, p, 5, 9), a)                       # same key, same mask
    assert not torch.equal(_drop_labels(y, p, 5, 10) == -1, mask)         # another offset
    assert not torch.equal(_drop_labels(y, p, 6, 9) == -1, mask)          # another seed
    frac = mask.float().mean().item()
    sigma = math.sqrt(p * (1 - p) / B)
    print(f"cond drop: B={B} p={p} dropped fraction {frac:.4f} (sigma {sigma:.4f})")
    assert abs(frac - p) < 5 * sigma
    r = _drop_rows(c, p, 5, 9)
    assert torch.equal((r == 0).all(dim=1), mask) and torch.equal((r == 0).any(dim=1), mask)   # whole rows, the same ones
    assert torch.equal(r[~mask], c[~mask])
    y2, c2 = y.clone(), c.clone()                                          # in place
    assert torch.equal(_drop_labels(y2, p, 5, 9, out=y2), a) and torch.equal(_drop_rows(c2, p, 5, 9, out=c2), r)


def _train_grad(seed, x0, y, t, noise, **kw):
    from tiny_diffusion_amd.train import TrainStep

    m = _model("cond", seed).train()
    ts = TrainStep(m, ForwardProcess(), **kw)
    ts.step(x0, y, t=t, noise=noise)
    torch.cuda.synchronize()
    return ts.flat_grad.clone(), ts.flat_param.clone()


def test_train_step_condition_dropout():
    B = 8
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(B, 1, 28, 28, generator=g).cuda()
    noise = torch.randn(B, 1, 28, 28, generator=g).cuda()
    t = torch.randint(0, 1000, (B,), generator=g).cuda()
    y = torch.randint(0, NUM_CLASSES, (B,), generator=g).cuda()
    plain = _train_grad(4, x0, y, t, noise)
    zero = _train_grad(4, x0, y, t, noise, cond_drop_prob=0.0, cond_drop_seed=11)
    assert torch.equal(zero[0], plain[0]) and torch.equal(zero[1], plain[1])
    dropped = _train_grad(4, x0, y, t, noise, cond_drop_prob=1.0, cond_drop_seed=11)
    direct = _train_grad(4, x0, torch.full_like(y, -1), t, noise)
    assert torch.equal(dropped[0], direct[0]) and torch.equal(dropped[1], direct[1])
    assert not torch.equal(dropped[0], plain[0])
    assert torch.equal(y, y.clamp(min=0))   # the caller's labels are untouched: the step works on a copy


def test_train_step_condition_dropout_captured():
    """The captured step applies the dropout into its own label buffer before each replay: with p = 1 three steps
    equal three steps on null labels, with p = 0 three plain ones."""
    from tiny_diffusion_amd.train import TrainStep

    B = 8
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(B, 1, 28, 28, generator=g).cuda()
    y = torch.randint(0, NUM_CLASSES, (B,), generator=g).cuda()

    def run(labels, **kw):
        m = _model("cond", 4).train()
        ts = TrainStep(m, ForwardProcess(), use_graph=True, **kw)
        torch.manual_seed(123)   # t and the noise are torch draws inside the step
        for _ in range(3):
            ts.step(x0, labels)
        torch.cuda.synchronize()
        assert ts._graph is not None
        return ts.flat_param.clone()

    assert torch.equal(run(y, cond_drop_prob=1.0), run(torch.full_like(y, -1)))
    assert torch.equal(run(y, cond_drop_prob=0.0), run(y))


# ---------------------------------------------------------------- 4. one guided step against fp64
@pytest.mark.parametrize("kind", ["cond", "laion"])
def test_one_guided_step_against_fp64(kind):
    """A chain of one step (no noise: its only step is the last) in the three modes, then the single step k = 1 of a
    two-step schedule with recorded noise - the fused epilogue (one eval step) and the separate update kernel.  One step
    must meet the chain tolerance without the amplification factor of the combination."""
    n, w = 3, 3.0
    fp = ForwardProcess()
    m = _model(kind, 1)
    fwd = _fp64_forward(kind, 1)
    x_T, zs, y = _inputs(kind, n, 2, seed=21)
    sched = ddim_schedule(fp, timesteps=[400])
    c1, c2, _ = sched.coef64[0].tolist()
    tt = torch.full((n,), 400, dtype=torch.long)
    want = c1 * (x_T.double() - c2 * _guided_eps64(fwd, kind, x_T, tt, y, w))
    for mode, kw in MODES.items():
        got = sample_loop(m, fp, "cuda", n, y, x_T=x_T, schedule=sched, guidance_scale=w, **kw)
        r = rel_mse(got, want)
        print(f"one guided step {kind} {mode}: relative MSE vs fp64 {r:.3e}")
        assert got.shape == x_T.shape and r < CHAIN_TOL, (mode, r)
    # step k = 1 of (200, 700), eta = 1: sigma > 0, recorded noise of n rows
    sched = ddim_schedule(fp, timesteps=[200, 700], eta=1.0)
    tau, coef = sched.device_tables("cuda")
    c1, c2, sg = sched.coef64[1].tolist()
    assert sg > 0
    tt = torch.full((n,), 700, dtype=torch.long)
    z = zs[0]
    want = c1 * (x_T.double() - c2 * _guided_eps64(fwd, kind, x_T, tt, y, w)) + sg * z.double()
    y2 = torch.cat([y, _null(kind, y)]).contiguous()
    for fused in (True, False):
        x = torch.cat([x_T, x_T]).cuda().contiguous()
        counter = torch.tensor([1], dtype=torch.int64, device="cuda")
        t_idx = torch.empty(1, dtype=torch.int32, device="cuda")
        t_vec = torch.empty(2 * n, dtype=torch.int64, device="cuda")
        eps = torch.empty_like(x)
        with torch.no_grad():
            if fused:
                m._run_eval_step(x, y2, coef, counter, t_idx, t_vec, eps, z=z.cuda().contiguous(), tau=tau, S=2,
                                 guidance_scale=w)
                assert counter.item() == 0 and t_idx.item() == 1 and int(t_vec[-1]) == 700
            else:
                t_idx.fill_(1); t_vec.fill_(700)
                eps = m._run_forward(x, t_vec, y2, mode=2)[0]
                check(lib.tdx_p_sample_step_guided(x.data_ptr(), eps.data_ptr(), z.cuda().contiguous().data_ptr(),
                                                   coef.data_ptr(), tau.data_ptr(), t_idx.data_ptr(), x.numel() // 2, w,
                                                   0, 0, None, torch.cuda.current_stream().cuda_stream))
        assert torch.equal(x[:n], x[n:])   # the two halves of the state stay equal
        r = rel_mse(x[:n], want)
        print(f"guided step k=1 with recorded noise {kind} fused={fused}: relative MSE vs fp64 {r:.3e}")
        assert r < CHAIN_TOL, (fused, r)


# ---------------------------------------------------------------- 5. guided chains against fp64
@torch.no_grad()
def _guided_chain64(fwd, kind, sched_coef64, taus, x_T, y, w, zs=None):
    """x' = c1 (x - c2 e) + sigma z with the fp64 coefficient rows and e the guided prediction, fp64 state."""
    x = x_T.double()
    n = x.shape[0]
    for k in reversed(range(len(taus))):
        c1, c2, sg = sched_coef64[k].tolist()
        e = _guided_eps64(fwd, kind, x, torch.full((n,), taus[k], dtype=torch.long), y, w)
        x = c1 * (x - c2 * e)
        if k > 0 and sg > 0:
            x = x + sg * zs[taus[k]].double()
    return x


@pytest.mark.parametrize("w", [0.0, 1.0, 3.0])
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("kind", ["cond", "laion"])
def test_guided_ddim_chain_against_fp64(kind, n, w):
    S = 10
    fp = ForwardProcess()
    m = _model(kind, 1)
    x_T, _, y = _inputs(kind, n, 1, seed=11 + n)
    sched = ddim_schedule(fp, steps=S)
    want = _guided_chain64(_fp64_forward(kind, 1), kind, sched.coef64, sched.timesteps.tolist(), x_T, y, w)
    for mode, kw in MODES.items():   # eta = 0 draws no noise: the Philox mode is comparable too
        got = sample_loop(m, fp, "cuda", n, y, x_T=x_T, schedule=sched, guidance_scale=w, **kw)
        r = rel_mse(got, want)
        print(f"guided DDIM eta=0 S={S} {kind} n={n} w={w} {mode}: relative MSE vs fp64 {r:.3e} (bound {CHAIN_TOL * _amp(w):.1e})")
        assert r < CHAIN_TOL * _amp(w), (mode, r)


@pytest.mark.parametrize("w", [0.0, 1.0, 3.0])
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("kind", ["cond", "laion"])
def test_guided_ddpm_chain_against_fp64(kind, n, w):
    T = 20
    fp = ForwardProcess(num_timesteps=T)
    m = _model(kind, 1)
    x_T, zs, y = _inputs(kind, n, T, seed=5 + n)
    coef64 = fp.tables("cpu")[2].double()   # the reference's fp32 rows are the chain's coefficients
    want = _guided_chain64(_fp64_forward(kind, 1), kind, coef64, list(range(T)), x_T, y, w, zs)
    for mode in ("eager", "graph"):
        got = sample_loop(m, fp, "cuda", n, y, x_T=x_T, noises=zs, guidance_scale=w, **MODES[mode])
        r = rel_mse(got, want)
        print(f"guided DDPM T={T} recorded noise {kind} n={n} w={w} {mode}: relative MSE vs fp64 {r:.3e} (bound {CHAIN_TOL * _amp(w):.1e})")
        assert r < CHAIN_TOL * _amp(w), (mode, r)


# ---------------------------------------------------------------- 6. consistency with the unguided chain
@pytest.mark.parametrize("kind,S", [("cond", 7), ("cond", 23), ("laion", 7)])
def test_guided_w1_w0_equal_the_unguided_chains(kind, S):
    """w = 1 is the conditional chain of n samples, w = 0 the chain on all-null conditions - with in-kernel noise under
    the same seed too, which holds only if the guided chain of 2n rows draws the noise of the unguided chain of n.
    Not bitwise: the convolution kernels chosen at batch 2n and n differ."""
    assert S % GRAPH_STEPS   # a tail graph
    n = 3
    fp = ForwardProcess()
    m = _model(kind, 4)
    x_T, zs, y = _inputs(kind, n, 1000, seed=S)
    sched = ddim_schedule(fp, steps=S, eta=0.7)
    assert float(sched.coef[1:, 2].min()) > 0   # every step but the last adds noise
    noises = {t: zs[t] for t in sched.timesteps.tolist()}
    for w, cond in ((1.0, y), (0.0, _null(kind, y))):
        for name, kw in (("philox", dict(use_graph=True, philox_seed=5)), ("philox eager", dict(philox_seed=5)),
                         ("recorded", dict(noises=noises)), ("recorded graph", dict(noises=noises, use_graph=True))):
            plain = sample_loop(m, fp, "cuda", n, cond, x_T=x_T, schedule=sched, **kw)
            got = sample_loop(m, fp, "cuda", n, y, x_T=x_T, schedule=sched, guidance_scale=w, **kw)
            r = rel_mse(got, plain)
            print(f"guided w={w} vs unguided {kind} S={S} {name}: relative MSE {r:.3e}")
            assert torch.isfinite(got).all() and r < 1e-8, (w, name, r)
    # the comparison above can tell one noise stream from another
    a, b = (sample_loop(m, fp, "cuda", n, y, x_T=x_T, schedule=sched, use_graph=True, philox_seed=s) for s in (5, 6))
    assert rel_mse(a, b) > 1e-4


# ---------------------------------------------------------------- 7. fused = unfused
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kind", ["cond", "laion"])
def test_guided_fused_update_equals_separate_kernel(kind, bf16):
    """The guided update in final_conv's epilogue against the separate kernel behind the plain convolution (knob
    sample_fuse without bit 2): the same accumulation order, the same cfg_eps / p_step expressions, the same Philox
    indexing - bit-identical, like the unguided pair."""
    n, S = 4, 3
    fp = ForwardProcess()
    m = _model(kind, 8)
    if bf16:
        m.set_compute_dtype(torch.bfloat16)
    x_T, _, y = _inputs(kind, n, 1, seed=2)
    sched = ddim_schedule(fp, steps=S, eta=0.5)
    kw = dict(x_T=x_T, schedule=sched, guidance_scale=2.5, use_graph=True, philox_seed=9)
    fused = sample_loop(m, fp, "cuda", n, y, **kw)
    with tuned(sample_fuse=2):
        separate = sample_loop(m, fp, "cuda", n, y, **kw)
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, separate), rel_mse(fused, separate)


# ---------------------------------------------------------------- 8. guidance_scale=None is the existing path
def test_guidance_none_is_the_existing_path():
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import conditional_diffusion_laion as L

    n = 3
    fp = ForwardProcess(num_timesteps=20)
    for kind, mod in (("cond", C), ("laion", L)):
        m = _model(kind, 2)
        x_T, zs, y = _inputs(kind, n, 20, seed=4)
        cond = dict(text_embeds=y) if kind == "laion" else dict(n_samples=n, y=y)
        for kw in (dict(x_T=x_T, noises=zs), dict(x_T=x_T, use_graph=True, philox_seed=3), dict()):
            outs = []
            for extra in ({}, dict(guidance_scale=None)):
                torch.manual_seed(77)   # the default mode draws from torch's generators
                outs.append((mod.sample(m, fp, "cuda", **cond, **kw, **extra),
                             mod.ddim_sample(m, fp, "cuda", **cond, steps=6, eta=0.4, **kw, **extra)))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (kind, list(kw))


# ---------------------------------------------------------------- 9. no stale state
def test_no_stale_state_between_guided_and_unguided_calls():
    from tiny_diffusion_amd.conditional_diffusion import ddim_sample

    n = 4
    fp = ForwardProcess()
    m = _model("cond", 6)
    x_T, _, y = _inputs("cond", n, 1, seed=8)
    y_other = (y + 3) % NUM_CLASSES
    kw = dict(n_samples=n, x_T=x_T, use_graph=True, philox_seed=3, eta=0.3, steps=12)
    calls = [dict(y=y, guidance_scale=2.0), dict(y=y), dict(y=y_other, guidance_scale=2.0), dict(y=y_other),
             dict(y=torch.cat([y, y]), n_samples=2 * n, x_T=torch.cat([x_T, x_T]))]   # unguided at the guided batch
    outs = []
    for c in calls:
        got = ddim_sample(m, fp, "cuda", **{**kw, **c})
        fresh = ddim_sample(_model("cond", 6), fp, "cuda", **{**kw, **c})
        assert torch.equal(got, fresh), list(c)
        outs.append(got)
    assert not torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])
