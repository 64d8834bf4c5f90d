"""DDIM sampling on the device (timestep schedules, schedule.ddim_schedule): the identity schedule reproduces
the existing sampler bit for bit in every mode, DDIM chains agree with a fp64 restatement of Song et al. 2021
eq. 12, schedules of any length run graph = eager, table mode agrees with the direct time path, nothing stale
survives between calls, and the drop-in modules' ddim_sample wrappers keep sample()'s contracts."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oracle import ref_laion as RLA  # noqa: E402
from oracle import ref_latent as RLT  # noqa: E402
from oracle import ref_transformer as RT  # noqa: E402
from oracle.weights import (make_state_dict, make_state_dict_latent, make_state_dict_laion,  # noqa: E402
                            make_state_dict_transformer, make_state_dict_vae)
from parity_helpers import rel_mse  # noqa: E402

from tiny_diffusion_amd._lib import tuned  # noqa: E402
from tiny_diffusion_amd.schedule import ForwardProcess, ddim_schedule, ddpm_schedule, sample_loop  # noqa: E402


def _model(kind, seed=0):
    if kind == "uncond":
        from tiny_diffusion_amd.diffusion import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict(seed, False), strict=True)
    elif kind == "cond":
        from tiny_diffusion_amd.conditional_diffusion import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict(seed, True), strict=True)
    elif kind == "laion":
        from tiny_diffusion_amd.conditional_diffusion_laion import NoiseModel
        m = NoiseModel(time_dim=768)
        m.load_state_dict(make_state_dict_laion(seed), strict=True)
    elif kind == "latent":
        from tiny_diffusion_amd.latent_diffusion import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict_latent(seed), strict=True)
    else:
        from tiny_diffusion_amd.diffusion_transformer import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict_transformer(seed), strict=True)
    return m.cuda()


SHAPES = {"uncond": (1, 28, 28), "cond": (1, 28, 28), "laion": (4, 32, 32), "latent": (20,), "transformer": (20,)}


def _inputs(kind, n, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    x_T = torch.randn(n, *SHAPES[kind], generator=g)
    zs = torch.randn(T, n, *SHAPES[kind], generator=g)
    if kind == "uncond":
        y = None
    elif kind == "laion":
        y = torch.randn(n, 768, generator=g).cuda()
    else:
        y = torch.randint(0, 10, (n,), generator=g).cuda()
    return x_T, zs, y


MODES = {"eager": dict(use_graph=False), "graph": dict(use_graph=True), "philox": dict(use_graph=True, philox_seed=7)}


# ---------------------------------------------------------------- 1. the identity schedule is the existing sampler
@pytest.mark.parametrize("kind,n,bf16", [("uncond", 4, False), ("uncond", 5, False), ("cond", 4, False),
                                         ("cond", 5, False), ("laion", 4, False), ("latent", 4, False),
                                         ("transformer", 4, False), ("uncond", 4, True), ("laion", 4, True)])
def test_ddpm_schedule_reproduces_sample_loop(kind, n, bf16):
    T = 20
    m = _model(kind, 3)
    if bf16:
        m.set_compute_dtype(torch.bfloat16)
    fp = ForwardProcess(num_timesteps=T)
    x_T, zs, y = _inputs(kind, n, T, seed=n)
    for mode, kw in MODES.items():
        noise = {} if "philox_seed" in kw else dict(noises=zs)
        ref = sample_loop(m, fp, "cuda", n, y, x_T=x_T, **noise, **kw)
        got = sample_loop(m, fp, "cuda", n, y, x_T=x_T, schedule=ddpm_schedule(fp), **noise, **kw)
        assert torch.isfinite(ref).all()
        assert torch.equal(got, ref), (kind, n, bf16, mode, rel_mse(got, ref))


# ---------------------------------------------------------------- 2./3. DDIM against fp64
def _fp64_forward(kind, seed):
    if kind in ("uncond", "cond", "laion"):
        sd = make_state_dict_laion(seed) if kind == "laion" else make_state_dict(seed, kind == "cond")
        p, b = R.split_state(sd)
    elif kind == "latent":
        p, b = R.split_state(make_state_dict_latent(seed))
    else:
        p, b = dict(make_state_dict_transformer(seed)), {}
    p = {k: v.double() for k, v in p.items()}
    b = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in b.items()}

    def fwd(x, t, y):
        yy = None if y is None else y.cpu()
        if kind == "laion":
            return RLA.unet_forward(p, b, x, t, yy.double(), training=False)
        if kind == "latent":
            return RLT.noise_forward(p, b, x, t, yy, training=False)
        if kind == "transformer":
            return RT.noise_forward(p, x, t, yy)
        return R.unet_forward(p, b, x, t, yy, training=False)
    return fwd


@torch.no_grad()
def _ddim_chain64(fwd, fp, taus, eta, x_T, y, zs=None):
    """Song et al. 2021 eq. 12 in x0 form, fp64 state; zs[t] is the noise of the step at timestep t."""
    acp = fp.alphas_cumprod.double()
    x = x_T.double()
    n = x.shape[0]
    for k in reversed(range(len(taus))):
        t = taus[k]
        ab = acp[t].item()
        ab_prev = acp[taus[k - 1]].item() if k > 0 else 1.0
        eps = fwd(x, torch.full((n,), t, dtype=torch.long), y)
        sigma = eta * math.sqrt((1 - ab_prev) / (1 - ab)) * math.sqrt(1 - ab / ab_prev)
        x0 = (x - math.sqrt(1 - ab) * eps) / math.sqrt(ab)
        x = math.sqrt(ab_prev) * x0 + math.sqrt(1 - ab_prev - sigma ** 2) * eps
        if k > 0 and sigma > 0:
            x = x + sigma * zs[t].double()
    return x


@pytest.mark.parametrize("kind,S", [("uncond", 10), ("uncond", 50), ("cond", 10), ("laion", 10), ("latent", 10),
                                    ("transformer", 10)])
def test_ddim_eta0_against_fp64(kind, S):
    n = 4
    fp = ForwardProcess()
    m = _model(kind, 1)
    x_T, _, y = _inputs(kind, n, 1, seed=11)
    sched = ddim_schedule(fp, steps=S)
    want = _ddim_chain64(_fp64_forward(kind, 1), fp, sched.timesteps.tolist(), 0.0, x_T, y)
    for mode, kw in MODES.items():
        got = sample_loop(m, fp, "cuda", n, y, x_T=x_T, schedule=sched, **kw)
        r = rel_mse(got, want)
        print(f"DDIM eta=0 {kind} S={S} {mode}: relative MSE vs fp64 {r:.3e}")
        assert r < 1e-8, (mode, r)


def test_ddim_eta1_recorded_noise_against_fp64():
    n, S = 4, 10
    fp = ForwardProcess()
    m = _model("uncond", 2)
    x_T, zs, _ = _inputs("uncond", n, 1000, seed=5)
    sched = ddim_schedule(fp, steps=S, eta=1.0)
    want = _ddim_chain64(_fp64_forward("uncond", 2), fp, sched.timesteps.tolist(), 1.0, x_T, None, zs)
    eager = sample_loop(m, fp, "cuda", n, None, x_T=x_T, noises=zs, schedule=sched)
    graph = sample_loop(m, fp, "cuda", n, None, x_T=x_T, noises=zs, schedule=sched, use_graph=True)
    r = rel_mse(eager, want)
    print(f"DDIM eta=1 S={S} recorded noise: relative MSE vs fp64 {r:.3e}")
    assert r < 1e-8, r
    assert torch.equal(eager, graph)
    # in-kernel noise: the graph (device counter, fused update) equals the eager chain on the direct time path
    # bit for bit, and the table-mode graph equals it up to the reassociation of the projection sums
    pe = sample_loop(m, fp, "cuda", n, None, x_T=x_T, schedule=sched, philox_seed=4)
    pt = sample_loop(m, fp, "cuda", n, None, x_T=x_T, schedule=sched, philox_seed=4, use_graph=True)
    with tuned(sample_tables=0):
        pg = sample_loop(m, fp, "cuda", n, None, x_T=x_T, schedule=sched, philox_seed=4, use_graph=True)
    assert torch.isfinite(pe).all() and not torch.equal(pe, eager)
    assert torch.equal(pg, pe)
    assert rel_mse(pt, pe) < 1e-10


# ---------------------------------------------------------------- 4. any schedule length
@pytest.mark.parametrize("S", [1, 7, 23])
@pytest.mark.parametrize("kind", ["cond", "transformer"])
def test_schedules_not_multiple_of_graph_steps(kind, S):
    n = 3
    fp = ForwardProcess()
    m = _model(kind, 4)
    x_T, zs, y = _inputs(kind, n, 1000, seed=S)
    sched = ddim_schedule(fp, steps=S, eta=0.7)
    tau0 = sched.timesteps[0].item()
    junk = {t: zs[t] for t in sched.timesteps.tolist()}
    junk[tau0] = torch.full_like(zs[0], 1e6)          # noise handed in for the last step is ignored
    eager = sample_loop(m, fp, "cuda", n, y, x_T=x_T, noises=zs, schedule=sched)
    assert torch.isfinite(eager).all()
    assert torch.equal(sample_loop(m, fp, "cuda", n, y, x_T=x_T, noises=junk, schedule=sched), eager)
    assert torch.equal(sample_loop(m, fp, "cuda", n, y, x_T=x_T, noises=junk, schedule=sched, use_graph=True), eager)
    pe = sample_loop(m, fp, "cuda", n, y, x_T=x_T, schedule=sched, philox_seed=2)
    with tuned(sample_tables=0):
        pg = sample_loop(m, fp, "cuda", n, y, x_T=x_T, schedule=sched, philox_seed=2, use_graph=True)
    assert torch.equal(pg, pe)
    if kind == "transformer":
        return
    # the one-call eval step on the device counter: after the chain the counter is -1 and t_idx 0
    tau, coef = sched.device_tables("cuda")
    x = x_T.cuda().contiguous()
    counter = torch.tensor([S - 1], dtype=torch.int64, device="cuda")
    t_idx = torch.empty(1, dtype=torch.int32, device="cuda")
    t_vec = torch.empty(n, dtype=torch.int64, device="cuda")
    eps = torch.empty_like(x)
    with torch.no_grad():
        for k in reversed(range(S)):
            t = sched.timesteps[k].item()
            m._run_eval_step(x, y, coef, counter, t_idx, t_vec, eps, z=junk[t].cuda(), tau=tau, S=S)
    assert counter.item() == -1 and t_idx.item() == 0 and int(t_vec[0]) == tau0
    assert torch.equal(x, eager)


# ---------------------------------------------------------------- 5. table mode against the direct time path
@pytest.mark.parametrize("kind", ["uncond", "cond", "laion"])
def test_schedule_tables_match_direct_time_path(kind):
    n, S = 5, 10
    fp = ForwardProcess()
    m = _model(kind, 21).eval()
    sched = ddim_schedule(fp, timesteps=[0, 3, 50, 51, 200, 333, 600, 777, 900, 999], eta=0.5)
    tau, coef = sched.device_tables("cuda")
    x_T, _, y = _inputs(kind, n, 1, seed=3)
    outs = []
    for tables in (False, True, False):
        x = x_T.cuda().contiguous()
        counter = torch.full((1,), S - 1, dtype=torch.int64, device="cuda")
        t_idx = torch.empty(1, dtype=torch.int32, device="cuda")
        t_vec = torch.empty(n, dtype=torch.int64, device="cuda")
        eps = torch.empty_like(x)
        with torch.no_grad():
            if outs and not tables:   # third round: a new pack generation switches the (now stale) tables off
                m._buf_epoch += 1
            m._run_eval_step(x, y, coef, counter, t_idx, t_vec, eps, philox_seed=11, tau=tau, S=S)
            if tables:
                m._prepare_sampling(x, y, S, tau=tau)
            for _ in range(S - 1):
                m._run_eval_step(x, y, coef, counter, t_idx, t_vec, eps, philox_seed=11, tau=tau, S=S)
        torch.cuda.synchronize()
        assert int(counter) == -1 and int(t_idx) == 0 and int(t_vec[0]) == 0
        outs.append(x.clone())
    assert torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0], outs[2])
    r = rel_mse(outs[1], outs[0])
    print(f"scheduled table mode vs direct, {kind}: relative MSE {r:.2e}")
    assert r < 1e-10
    # an identity table of the same length never serves the scheduled step
    x = x_T.cuda().contiguous()
    with torch.no_grad():
        m._prepare_sampling(x, y, 10)            # identity table, T = 10 rows, same batch and cond
        counter = torch.full((1,), S - 1, dtype=torch.int64, device="cuda")
        t_idx = torch.empty(1, dtype=torch.int32, device="cuda")
        t_vec = torch.empty(n, dtype=torch.int64, device="cuda")
        for _ in range(S):
            m._run_eval_step(x, y, coef, counter, t_idx, t_vec, eps, philox_seed=11, tau=tau, S=S)
    assert torch.equal(x, outs[0])


# ---------------------------------------------------------------- 6. nothing stale between calls
def test_no_stale_tables_or_graphs():
    from tiny_diffusion_amd.conditional_diffusion import ddim_sample, sample

    n = 4
    fp = ForwardProcess()
    m = _model("cond", 6)
    x_T, _, y = _inputs("cond", n, 1, seed=8)
    calls = [dict(steps=10), dict(steps=20), dict(timesteps=[i * 100 + 7 for i in range(10)]), dict(steps=10)]
    for kw in calls:
        got = ddim_sample(m, fp, "cuda", n_samples=n, y=y, x_T=x_T, use_graph=True, philox_seed=3, eta=0.3, **kw)
        fresh = ddim_sample(_model("cond", 6), fp, "cuda", n_samples=n, y=y, x_T=x_T, use_graph=True, philox_seed=3,
                            eta=0.3, **kw)
        eager = ddim_sample(m, fp, "cuda", n_samples=n, y=y, x_T=x_T, philox_seed=3, eta=0.3, **kw)
        assert torch.equal(got, fresh), kw
        assert rel_mse(got, eager) < 1e-10, kw
    fp10 = ForwardProcess(num_timesteps=10)   # an identity table as long as the last schedule
    got = sample(m, fp10, "cuda", n_samples=n, y=y, x_T=x_T, use_graph=True, philox_seed=3)
    fresh = sample(_model("cond", 6), fp10, "cuda", n_samples=n, y=y, x_T=x_T, use_graph=True, philox_seed=3)
    assert torch.equal(got, fresh)


# ---------------------------------------------------------------- 7. module wrappers
def test_module_wrappers():
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import conditional_diffusion_laion as L
    from tiny_diffusion_amd import diffusion as D
    from tiny_diffusion_amd import diffusion_transformer as DT
    from tiny_diffusion_amd import latent_diffusion as LD
    from tiny_diffusion_amd.vae import VAE, VAEConfig

    fp = ForwardProcess()
    m = _model("uncond").train()
    x = D.ddim_sample(m, fp, "cuda", n_samples=3, steps=5)
    assert x.shape == (3, 1, 28, 28) and torch.isfinite(x).all() and m.training is False
    with pytest.raises(ValueError):
        D.ddim_sample(m, fp, "cuda", n_samples=3, steps=0)
    with pytest.raises(ValueError):
        D.ddim_sample(m, fp, "cuda", n_samples=3, timesteps=[5, 1])
    with pytest.raises(ValueError):
        D.ddim_sample(m, fp, "cuda", n_samples=3, steps=5, eta=-1.0)

    m = _model("cond").train()
    x = C.ddim_sample(m, fp, "cuda", n_samples=3, y=torch.tensor([1, 2, 3]), steps=5, use_graph=True, philox_seed=1)
    assert x.shape == (3, 1, 28, 28) and torch.isfinite(x).all() and m.training is False
    with pytest.raises(ValueError):
        C.ddim_sample(m, fp, "cuda", n_samples=3)
    with pytest.raises(ValueError):
        C.ddim_sample(m, fp, "cuda", n_samples=3, y=torch.tensor([1, 2]))

    v = VAE(VAEConfig()); v.load_state_dict(make_state_dict_vae(0)); v = v.cuda().train()
    for mod, kind in ((LD, "latent"), (DT, "transformer")):
        m = _model(kind).train()
        img = mod.ddim_sample(v, m, fp, "cuda", n_samples=2, y=torch.tensor([0, 9]), steps=4, eta=1.0)
        assert img.shape == (2, 1, 28, 28) and torch.isfinite(img).all() and m.training is False and not v.training
        with pytest.raises(ValueError):
            mod.ddim_sample(v, m, fp, "cuda", n_samples=2)
        with pytest.raises(ValueError):
            mod.ddim_sample(v, m, fp, "cuda", n_samples=2, y=torch.tensor([0]))

    m = _model("laion").train()
    cond = torch.randn(2, 768, generator=torch.Generator().manual_seed(1)).cuda()
    x_T = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(2))
    with pytest.raises(ValueError):
        L.ddim_sample(m, fp, "cuda")
    lat = L.ddim_sample(m, fp, "cuda", text_embeds=cond, x_T=x_T, steps=5, use_graph=True, philox_seed=1)
    assert lat.shape == (2, 4, 32, 32) and m.training is False

    class FakeVAE:  # the decoder is an external model: only its call contract is exercised
        def __init__(self):
            self.seen = None

        def decode(self, z):
            self.seen = z.clone()

            class Out:
                sample = torch.cat([z[:, :3] * float("nan"), z[:, :3] * 10.0], dim=0)
            return Out()

    fv = FakeVAE()
    imgs = L.ddim_sample(m, fp, "cuda", text_embeds=cond, x_T=x_T, vae=fv, scaling_factor=0.18215, steps=5,
                         use_graph=True, philox_seed=1)
    assert torch.equal(fv.seen, lat / 0.18215)
    assert imgs.dtype == torch.float32 and imgs.min() >= 0 and imgs.max() <= 1 and not torch.isnan(imgs).any()
