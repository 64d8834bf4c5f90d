"""Clipped-x0 sampling on the device (``clip_denoised``): the x0-form update kernels bit for bit against a CPU fp32
restatement, the fused epilogue of final_conv against the separate kernel, whole chains against a fp64 chain in x0 form
with the clamp (the oracle's network in double), the range of the returned samples, never-binding bounds against the
unclipped chain, ``clip_denoised=None`` is the existing path, nothing stale between clipped and unclipped calls.

The clamp is 1-Lipschitz, so the chain tolerances are the unclipped chains' (no tie handling)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oracle import ref_laion as RLA  # noqa: E402
from oracle import ref_latent as RLT  # noqa: E402
from oracle import ref_transformer as RT  # noqa: E402
from oracle.weights import (make_state_dict, make_state_dict_laion, make_state_dict_latent,  # noqa: E402
                            make_state_dict_transformer)
from inpaint_helpers import cpu_x0_step as _cpu_x0_step, spy_entries  # noqa: E402
from parity_helpers import rel_mse  # noqa: E402

from tiny_diffusion_amd._lib import check, lib, tuned  # noqa: E402
from tiny_diffusion_amd.schedule import (GRAPH_STEPS, ForwardProcess, ddim_schedule, ddpm_schedule,  # noqa: E402
                                         sample_loop)

INF = float("inf")
NUM_CLASSES = 10
TDX_E_BADARG = -1
CHAIN_TOL = 1e-8    # the project's chain tolerance (test_gpu_ddim.py: relative MSE against fp64)
SHAPES = {"uncond": (1, 28, 28), "cond": (1, 28, 28), "laion": (4, 32, 32), "latent": (20,), "transformer": (20,)}
MODES = {"eager": dict(use_graph=False), "graph": dict(use_graph=True), "philox": dict(use_graph=True, philox_seed=7)}


def _amp(w):
    """How out_u + w (out_c - out_u) amplifies an error in either output (squared: the tolerances are mean squares)."""
    return 1.0 if w is None else (abs(w) + abs(w - 1.0)) ** 2


def _stream():
    return torch.cuda.current_stream().cuda_stream


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


def _inputs(kind, n, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    x_T = torch.randn(n, *SHAPES[kind], generator=g)
    zs = torch.randn(T, n, *SHAPES[kind], generator=g)
    if kind == "uncond":
        y = None
    elif kind == "laion":
        y = torch.randn(n, 768, generator=g).cuda()
    else:
        y = torch.randint(0, NUM_CLASSES, (n,), generator=g).cuda()
    return x_T, zs, y


def _null(kind, y):
    return torch.zeros_like(y) if kind == "laion" else torch.full_like(y, -1)


def _fp64_forward(kind, seed):
    """out(x, t, y) of the oracle's network in double; for the conditional MNIST UNet a label -1 is the null condition
    (one zero row appended to this copy of class_embedding.weight, as tests/test_gpu_cfg.py does)."""
    if kind in ("uncond", "cond", "laion"):
        sd = make_state_dict_laion(seed) if kind == "laion" else make_state_dict(seed, kind == "cond")
        if kind == "cond":
            w = sd["class_embedding.weight"]
            sd["class_embedding.weight"] = torch.cat([w, torch.zeros(1, w.shape[1], dtype=w.dtype)])
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
        if kind == "cond":
            yy = torch.where(yy < 0, torch.full_like(yy, NUM_CLASSES), yy)
        return R.unet_forward(p, b, x, t, yy, training=False)
    return fwd


# ---------------------------------------------------------------- the fp64 chain in x0 form, with the clamp
def _x0_rows64(fp, sched):
    """(a, b, A, Bx, sigma) per step in Python doubles, from this file's own expressions: DDIM rows from Song et al.'s
    closed forms on the fp64 ``alphas_cumprod``, DDPM rows from the reference's fp32 (c1, c2, sigma) (its chain is
    defined by them) through A = c1 c2 a / b, Bx = c1 (b - c2) / b.  Row 0: A = 1, Bx = 0."""
    acp = fp.alphas_cumprod.double()
    taus = sched.timesteps.tolist()
    rows = []
    for k, t in enumerate(taus):
        ab = acp[t].item()
        a, b = math.sqrt(ab), math.sqrt(1 - ab)
        if sched.eta is None:
            c1, c2, sg = fp.tables("cpu")[2][t].double().tolist()
            A, Bx = c1 * c2 * a / b, c1 * (b - c2) / b
        else:
            ab_prev = acp[taus[k - 1]].item() if k > 0 else 1.0
            sg = sched.eta * math.sqrt((1 - ab_prev) / (1 - ab)) * math.sqrt(1 - ab / ab_prev)
            r = math.sqrt(1 - ab_prev - sg * sg)
            A, Bx = math.sqrt(ab_prev) - a * r / b, r / b
        rows.append((a, b, 1.0, 0.0, sg) if k == 0 else (a, b, A, Bx, sg))
    return rows


@torch.no_grad()
def _clip_chain64(fwd, kind, fp, sched, x_T, y, lo, hi, prediction="eps", w=None, zs=None):
    """x0 = (x - b out) / a (eps) or a x - b out (v);  x' = A clamp(x0) + Bx x + sigma z, fp64 state.  ``w``: the
    guided output out_u + w (out_c - out_u).  Returns (x, clamped elements, untouched elements) over the chain."""
    x = x_T.double()
    n = x.shape[0]
    taus = sched.timesteps.tolist()
    clamped = untouched = 0
    for k, (a, b, A, Bx, sg) in reversed(list(enumerate(_x0_rows64(fp, sched)))):
        t = torch.full((n,), taus[k], dtype=torch.long)
        if w is None:
            out = fwd(x, t, y)
        else:
            o = fwd(torch.cat([x, x]), torch.cat([t, t]), torch.cat([y, _null(kind, y)]))
            out = o[n:] + w * (o[:n] - o[n:])
        x0 = (x - b * out) / a if prediction == "eps" else a * x - b * out
        x0c = torch.clamp(x0, lo, hi)
        clamped += int((x0c != x0).sum())
        untouched += int((x0c == x0).sum())
        x = A * x0c + Bx * x
        if k > 0 and sg > 0:
            x = x + sg * zs[taus[k]].double()
    return x, clamped, untouched


# ---------------------------------------------------------------- 4. the kernels, bit for bit
S_K = 10


def _table():
    fp = ForwardProcess()
    sched = ddim_schedule(fp, steps=S_K, eta=0.5)
    return sched, sched.x0_form(fp, "eps"), sched.x0_form(fp, "eps", device="cuda")


def _draw(shape, row, guided, w, seed):
    """x ~ N(0, 1) and an output such that the implied x0 is about N(0, 1.5^2): out = (x0 - p x) / q (the guided pair
    combines to it: out_c = out + (1 - w) d, out_u = out - w d)."""
    g = torch.Generator().manual_seed(seed)
    p, q = row[0].item(), row[1].item()
    x = torch.randn(shape, generator=g)
    x0 = 1.5 * torch.randn(shape, generator=g)
    out = (x0 - p * x) / q
    z = torch.randn(shape, generator=g)
    if guided:
        d = torch.randn(shape, generator=g)
        out = torch.cat([out + (1 - w) * d, out - w * d])
    return x.contiguous(), out.contiguous(), z.contiguous()


def _call_x0(xo, x, out, z, coef, tau, t_idx, lo, hi, philox=0, seed=0, w=None, n=None):
    zp = None if z is None else z.data_ptr()
    tp = None if tau is None else tau.data_ptr()
    if w is None:
        return lib.tdx_p_sample_step_x0(xo.data_ptr(), x.data_ptr(), out.data_ptr(), zp, coef.data_ptr(), tp,
                                        t_idx.data_ptr(), x.numel() if n is None else n, lo, hi, philox, seed, None,
                                        _stream())
    return lib.tdx_p_sample_step_x0_guided(x.data_ptr(), out.data_ptr(), zp, coef.data_ptr(), tp, t_idx.data_ptr(),
                                           x.numel() // 2 if n is None else n, w, lo, hi, philox, seed, None, _stream())


def _philox_noise(shape, k, tau, seed):
    """The noise the existing Philox update draws at step k: that update on x = 0, eps = 0 with the row (1, 0, 1)."""
    zero = torch.zeros(shape, device="cuda")
    got = torch.empty(shape, device="cuda")
    coef3 = torch.tensor([[1.0, 0.0, 1.0]] * S_K, device="cuda")
    t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
    if tau is None:
        check(lib.tdx_p_sample_step_philox(got.data_ptr(), zero.data_ptr(), zero.data_ptr(), coef3.data_ptr(),
                                           t_idx.data_ptr(), zero.numel(), seed, _stream()))
    else:
        check(lib.tdx_p_sample_step_sched_philox(got.data_ptr(), zero.data_ptr(), zero.data_ptr(), coef3.data_ptr(),
                                                 tau.data_ptr(), t_idx.data_ptr(), zero.numel(), seed, _stream()))
    return got


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("shape", [(3, 1, 28, 28), (5, 4, 8, 8)], ids=["3x1x28x28", "5x4x8x8"])
def test_x0_kernels_bitwise(shape, guided):
    sched, tab, coef = _table()
    tau_dev = sched.device_tables("cuda")[0]
    lo, hi, w = -1.0, 1.0, (2.5 if guided else None)
    for k in (0, 1, S_K - 1):
        x, out, z = _draw(shape, tab[k], guided, w, seed=10 * k + len(shape) + shape[0])
        want, x0 = _cpu_x0_step(x, out, z, tab[k], lo, hi, k, w)
        assert (x0 < lo).any() and (x0 > hi).any() and ((x0 > lo) & (x0 < hi)).any()   # both clamps bind, not everywhere
        if k == 0:
            assert want.min() >= lo and want.max() <= hi      # the last step returns the clamped prediction
        t_idx = torch.tensor([k], dtype=torch.int32, device="cuda")
        for tau in (None, tau_dev):
            xd = (torch.cat([x, x]) if guided else x).cuda().contiguous()
            od, zd = out.cuda(), z.cuda()
            keep = [t.clone() for t in (xd, od, zd, coef, tau_dev, t_idx)]
            if guided:      # in place by definition: both halves of x
                check(_call_x0(None, xd, od, zd, coef, tau, t_idx, lo, hi, w=w))
                got = xd[:shape[0]]
                assert torch.equal(xd[shape[0]:], got)
                keep[0] = xd
            else:
                got = torch.empty_like(xd)
                check(_call_x0(got, xd, od, zd, coef, tau, t_idx, lo, hi))
            assert torch.equal(got.cpu(), want), (k, tau is not None, (got.cpu() - want).abs().max().item())
            for t, saved in zip((xd, od, zd, coef, tau_dev, t_idx), keep):    # inputs untouched
                assert torch.equal(t, saved)
            if not guided:      # in place: x_out == x
                check(_call_x0(xd, xd, od, zd, coef, tau, t_idx, lo, hi))
                assert torch.equal(xd.cpu(), want)
            # no noise tensor at all: the update without the noise term
            xn = (torch.cat([x, x]) if guided else x).cuda().contiguous()
            check(_call_x0(xn, xn, od, None, coef, tau, t_idx, lo, hi, w=w))
            assert torch.equal(xn[:shape[0]].cpu(), _cpu_x0_step(x, out, None, tab[k], lo, hi, k, w)[0])
            # in-kernel noise = the tensor form fed the noise the existing Philox update draws under this seed
            zp = _philox_noise(shape, k, tau, seed=11)
            if k > 0:
                assert zp.abs().max() > 0 and (tau is None or not torch.equal(zp, _philox_noise(shape, k, None, 11)))
            else:
                assert not zp.any()
            xa = (torch.cat([x, x]) if guided else x).cuda().contiguous()
            xb = xa.clone()
            check(_call_x0(xa, xa, od, None, coef, tau, t_idx, lo, hi, philox=1, seed=11, w=w))
            check(_call_x0(xb, xb, od, zp, coef, tau, t_idx, lo, hi, w=w))
            assert torch.equal(xa, xb) and torch.isfinite(xa).all()
    # never-binding bounds: the arithmetic of the unclamped form
    x, out, z = _draw(shape, tab[1], guided, w, seed=99)
    t_idx = torch.tensor([1], dtype=torch.int32, device="cuda")
    xd = (torch.cat([x, x]) if guided else x).cuda().contiguous()
    check(_call_x0(xd, xd, out.cuda(), z.cuda(), coef, tau_dev, t_idx, -INF, INF, w=w))
    assert torch.equal(xd[:shape[0]].cpu(), _cpu_x0_step(x, out, z, tab[1], -INF, INF, 1, w)[0])


def test_x0_kernels_bad_arguments():
    _, _, coef = _table()
    x = torch.zeros(8, device="cuda")
    out = torch.zeros(16, device="cuda")
    t_idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = _stream()
    xp, op, cp, kp = x.data_ptr(), out.data_ptr(), coef.data_ptr(), t_idx.data_ptr()
    ok = (xp, xp, op, None, cp, None, kp, 8, -1.0, 1.0, 0, 0, None, st)
    assert lib.tdx_p_sample_step_x0(*ok) == 0
    for i in (0, 1, 2, 4, 6):          # x_out, x, out, coef5, t_idx
        bad = list(ok)
        bad[i] = None
        assert lib.tdx_p_sample_step_x0(*bad) == TDX_E_BADARG, i
    for n in (0, -4, 6, 7):
        assert lib.tdx_p_sample_step_x0(*ok[:7], n, *ok[8:]) == TDX_E_BADARG, n
    for lo, hi in ((1.0, -1.0), (0.0, 0.0), (float("nan"), 1.0), (-1.0, float("nan")), (INF, INF)):
        assert lib.tdx_p_sample_step_x0(*ok[:8], lo, hi, *ok[10:]) == TDX_E_BADARG, (lo, hi)
    okg = (xp, op, None, cp, None, kp, 8, 2.0, -1.0, 1.0, 0, 0, None, st)
    assert lib.tdx_p_sample_step_x0_guided(*okg[:6], 4, *okg[7:]) == 0      # x holds two halves of 4
    for i in (0, 1, 3, 5):             # x, out, coef5, t_idx
        bad = list(okg)
        bad[i] = None
        assert lib.tdx_p_sample_step_x0_guided(*bad) == TDX_E_BADARG, i
    for n in (0, -4, 6):
        assert lib.tdx_p_sample_step_x0_guided(*okg[:6], n, *okg[7:]) == TDX_E_BADARG, n
    for lo, hi in ((1.0, -1.0), (0.0, 0.0), (float("nan"), 1.0)):
        assert lib.tdx_p_sample_step_x0_guided(*okg[:8], lo, hi, *okg[10:]) == TDX_E_BADARG, (lo, hi)
    torch.cuda.synchronize()
    assert not x.any()      # x0 = 0 inside the bounds: the two good calls left zeros


# ---------------------------------------------------------------- 5. fused = separate
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,w", [("uncond", None), ("cond", 2.0), ("laion", 2.0)])
def test_clipped_fused_update_equals_separate_kernel(kind, w, bf16):
    """One clipped step through tdx_unet_eval_step_x0 with the update in final_conv's epilogue, and one with the knob
    sample_fuse without bit 2 (the plain convolution, then tdx_p_sample_step_x0{,_guided}): the same accumulation order,
    the same cfg_eps / p_step_x0 expressions, the same Philox indexing - x and the network's output bit-identical."""
    n, S = 4, 2
    fp = ForwardProcess()
    m = _model(kind, 8).eval()
    if bf16:
        m.set_compute_dtype(torch.bfloat16)
    x_T, zs, y = _inputs(kind, n, 1, seed=2)
    sched = ddim_schedule(fp, timesteps=[200, 700], eta=1.0)
    tau = sched.device_tables("cuda")[0]
    coef = sched.x0_form(fp, "eps", device="cuda")
    assert coef[1, 4] > 0
    rows = 2 * n if w is not None else n
    y2 = y if w is None else torch.cat([y, _null(kind, y)]).contiguous()
    res = {}
    for z in (None, zs[0].cuda().contiguous()):        # in-kernel noise, a noise tensor
        for fused in (True, False):
            x = (torch.cat([x_T, x_T]) if w is not None else x_T).cuda().contiguous()
            counter = torch.tensor([1], dtype=torch.int64, device="cuda")
            t_idx = torch.empty(1, dtype=torch.int32, device="cuda")
            t_vec = torch.empty(rows, dtype=torch.int64, device="cuda")
            out = torch.empty_like(x)
            with tuned(sample_fuse=6 if fused else 2), torch.no_grad():
                m._run_eval_step(x, y2, coef, counter, t_idx, t_vec, out, z=z, philox_seed=9, tau=tau, S=S,
                                 guidance_scale=w, clip=(-1.0, 1.0))
                torch.cuda.synchronize()
            assert counter.item() == 0 and t_idx.item() == 1 and int(t_vec[-1]) == 700
            res[(z is None, fused)] = (x.clone(), out.clone())
        (xf, of), (xs, os_) = res[(z is None, True)], res[(z is None, False)]
        assert torch.isfinite(xf).all()
        assert torch.equal(of, os_) and torch.equal(xf, xs), rel_mse(xf, xs)
        if w is not None:
            assert torch.equal(xf[:n], xf[n:])
    # the step did clamp, and not everywhere: the implied x0 of the network's output, in the kernel's arithmetic
    o = res[(True, True)][1].cpu()
    if w is not None:
        o = o[n:] + torch.tensor(w) * (o[:n] - o[n:])
    p, q = coef[1, 0].cpu(), coef[1, 1].cpu()
    x0 = p * x_T + q * o
    assert (x0.abs() > 1).any() and (x0.abs() < 1).any()
    assert not torch.equal(res[(True, True)][0], res[(False, True)][0])     # the two noise sources differ


# ---------------------------------------------------------------- 6. chains against fp64
CHAINS = [("uncond", None, "eps", 4), ("uncond", None, "v", 5), ("cond", 3.0, "eps", 5), ("laion", None, "eps", 4),
          ("latent", None, "eps", 4), ("transformer", None, "eps", 4)]


@pytest.mark.parametrize("kind,w,prediction,n", CHAINS)
def test_clipped_ddim_chain_against_fp64(kind, w, prediction, n):
    S = 10
    fp = ForwardProcess()
    m = _model(kind, 1)
    x_T, _, y = _inputs(kind, n, 1, seed=11 + n)
    sched = ddim_schedule(fp, steps=S)
    want, clamped, untouched = _clip_chain64(_fp64_forward(kind, 1), kind, fp, sched, x_T, y, -1.0, 1.0, prediction, w)
    print(f"clipped DDIM eta=0 S={S} {kind} w={w} {prediction}: fp64 chain clamped {clamped}, left {untouched} elements")
    assert clamped > 0 and untouched > 0
    assert want.min() >= -1 and want.max() <= 1
    for mode, kw in MODES.items():   # eta = 0 draws no noise: the Philox mode is comparable too
        got = sample_loop(m, fp, "cuda", n, y, x_T=x_T, schedule=sched, guidance_scale=w, prediction=prediction,
                          clip_denoised=True, **kw)
        r = rel_mse(got, want)
        print(f"clipped DDIM eta=0 S={S} {kind} w={w} {prediction} {mode}: relative MSE vs fp64 {r:.3e} "
              f"(bound {CHAIN_TOL * _amp(w):.1e})")
        assert got.shape == x_T.shape and r < CHAIN_TOL * _amp(w), (mode, r)
        assert got.min() >= -1 and got.max() <= 1


@pytest.mark.parametrize("kind,w,prediction,n", [("uncond", None, "eps", 4), ("cond", 3.0, "eps", 5),
                                                 ("cond", None, "v", 4), ("laion", None, "eps", 4)])
def test_clipped_ddpm_chain_against_fp64(kind, w, prediction, n):
    T = 20
    fp = ForwardProcess(num_timesteps=T)
    m = _model(kind, 1)
    x_T, zs, y = _inputs(kind, n, T, seed=5 + n)
    lo, hi = (-1.0, 1.0) if w is None else (-0.75, 0.5)
    want, clamped, untouched = _clip_chain64(_fp64_forward(kind, 1), kind, fp, ddpm_schedule(fp), x_T, y, lo, hi,
                                             prediction, w, zs)
    print(f"clipped DDPM T={T} {kind} w={w} {prediction}: fp64 chain clamped {clamped}, left {untouched} elements")
    assert clamped > 0 and untouched > 0
    for mode in ("eager", "graph"):
        got = sample_loop(m, fp, "cuda", n, y, x_T=x_T, noises=zs, guidance_scale=w, prediction=prediction,
                          clip_denoised=(lo, hi), **MODES[mode])
        r = rel_mse(got, want)
        print(f"clipped DDPM T={T} recorded noise {kind} w={w} {prediction} {mode}: relative MSE vs fp64 {r:.3e} "
              f"(bound {CHAIN_TOL * _amp(w):.1e})")
        assert r < CHAIN_TOL * _amp(w), (mode, r)
        assert got.min() >= lo and got.max() <= hi


@pytest.mark.parametrize("kind,w,prediction", [("uncond", None, "eps"), ("cond", 2.0, "v"), ("laion", 2.0, "eps"),
                                               ("latent", None, "eps")])
def test_clipped_philox_graph_equals_eager(kind, w, prediction):
    """In-kernel noise: the graph mode (device counter, sampling tables, fused epilogue, a tail graph) against the eager
    chain on the direct time path - the tolerance of that pairing in tests/test_gpu_ddim.py (the table mode reassociates
    one projection sum) -, and bit for bit with the tables off."""
    n, S = 4, 13
    assert S % GRAPH_STEPS
    fp = ForwardProcess()
    m = _model(kind, 4)
    x_T, _, y = _inputs(kind, n, 1, seed=S)
    sched = ddim_schedule(fp, steps=S, eta=0.5)
    assert float(sched.coef[1:, 2].min()) > 0
    kw = dict(x_T=x_T, schedule=sched, guidance_scale=w, prediction=prediction, clip_denoised=True, philox_seed=4)
    pe = sample_loop(m, fp, "cuda", n, y, **kw)
    pt = sample_loop(m, fp, "cuda", n, y, use_graph=True, **kw)
    with tuned(sample_tables=0):
        pg = sample_loop(m, fp, "cuda", n, y, use_graph=True, **kw)
    assert torch.isfinite(pe).all() and pe.min() >= -1 and pe.max() <= 1
    assert torch.equal(pg, pe)
    r = rel_mse(pt, pe)
    print(f"clipped graph + Philox vs eager + Philox {kind} w={w} {prediction} S={S}: relative MSE {r:.3e}")
    assert r < 1e-10
    other = sample_loop(m, fp, "cuda", n, y, use_graph=True, **{**kw, "philox_seed": 5})
    assert rel_mse(other, pe) > 1e-4      # the comparison can tell one noise stream from another


# ---------------------------------------------------------------- 7. range
@pytest.mark.parametrize("clip", [True, (-0.5, 0.25)], ids=repr)
@pytest.mark.parametrize("kind,w", [("uncond", None), ("cond", 3.0)])
def test_returned_samples_lie_in_the_range(kind, w, clip):
    n = 5
    lo, hi = (-1.0, 1.0) if clip is True else clip
    fp = ForwardProcess()
    m = _model(kind, 3)
    x_T, zs, y = _inputs(kind, n, 1000, seed=17)
    sched = ddim_schedule(fp, steps=7, eta=0.7)
    fp20 = ForwardProcess(num_timesteps=20)
    for mode, kw in MODES.items():
        noise = {} if "philox_seed" in kw else dict(noises=zs)
        for got in (sample_loop(m, fp, "cuda", n, y, x_T=x_T, schedule=sched, guidance_scale=w, clip_denoised=clip,
                                **noise, **kw),
                    sample_loop(m, fp20, "cuda", n, y, x_T=x_T, guidance_scale=w, clip_denoised=clip, **noise, **kw)):
            assert got.shape == x_T.shape and torch.isfinite(got).all()
            assert got.min().item() >= lo and got.max().item() <= hi, (mode, got.min().item(), got.max().item())
    free = sample_loop(m, fp20, "cuda", n, y, x_T=x_T, guidance_scale=w, noises=zs)
    assert free.min().item() < lo and free.max().item() > hi              # and the unclipped chain leaves the range


# ---------------------------------------------------------------- 8. never-binding bounds
@pytest.mark.parametrize("kind,w,prediction", [("uncond", None, "eps"), ("uncond", None, "v"), ("cond", 3.0, "eps"),
                                               ("transformer", None, "eps")])
def test_infinite_bounds_reproduce_the_unclipped_chain(kind, w, prediction):
    n = 4
    fp = ForwardProcess()
    fp20 = ForwardProcess(num_timesteps=20)
    m = _model(kind, 5)
    x_T, zs, y = _inputs(kind, n, 1000, seed=23)
    sched = ddim_schedule(fp, steps=10, eta=0.5)
    for name, f, kw in (("DDIM graph + Philox", fp, dict(schedule=sched, use_graph=True, philox_seed=3)),
                        ("DDIM eager + Philox", fp, dict(schedule=sched, philox_seed=3)),
                        ("DDIM recorded graph", fp, dict(schedule=sched, noises=zs, use_graph=True)),
                        ("DDPM T=20 recorded", fp20, dict(noises=zs)),
                        ("DDPM T=20 graph + Philox", fp20, dict(use_graph=True, philox_seed=3))):
        base = dict(x_T=x_T, guidance_scale=w, prediction=prediction, **kw)
        plain = sample_loop(m, f, "cuda", n, y, **base)
        got = sample_loop(m, f, "cuda", n, y, clip_denoised=(-INF, INF), **base)
        r = rel_mse(got, plain)
        print(f"(-inf, inf) vs unclipped {kind} w={w} {prediction} {name}: relative MSE {r:.3e}")
        assert torch.isfinite(got).all() and r < 1e-8, (name, r)
        clipped = sample_loop(m, f, "cuda", n, y, clip_denoised=True, **base)
        assert rel_mse(clipped, plain) > 1e-4      # the comparison can tell a clipped chain from an unclipped one


# ---------------------------------------------------------------- 9. the defaults are the path as it was
def test_defaults_are_the_path_as_it_was(monkeypatch):
    from tiny_diffusion_amd import conditional_diffusion as C
    from tiny_diffusion_amd import diffusion as D

    calls = []
    spy_entries(monkeypatch, lib, ("tdx_p_sample_step_x0", "tdx_p_sample_step_x0_guided", "tdx_p_sample_update",
                                   "tdx_unet_eval_step_update"), calls)
    n = 3
    fp = ForwardProcess(num_timesteps=20)
    for kind, mod, w in (("uncond", D, None), ("cond", C, 2.0)):
        m = _model(kind, 2)
        x_T, zs, y = _inputs(kind, n, 20, seed=4)
        cond = dict(n_samples=n) if kind == "uncond" else dict(n_samples=n, y=y, guidance_scale=w)
        for kw in (dict(x_T=x_T, noises=zs), dict(x_T=x_T, noises=zs, use_graph=True),
                   dict(x_T=x_T, use_graph=True, philox_seed=3), dict()):
            outs = []
            for extra in ({}, dict(clip_denoised=None), dict(clip_denoised=False)):
                torch.manual_seed(77)   # the default mode draws from torch's generators
                outs.append((mod.sample(m, fp, "cuda", **cond, **kw, **extra),
                             mod.ddim_sample(m, fp, "cuda", **cond, steps=6, eta=0.4, **kw, **extra)))
            for o in outs[1:]:
                assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]), (kind, w, list(kw))
        assert calls and not [c for c in calls if "[x0" in c or "step_x0" in c]      # eps-form updates only
        calls.clear()
        g = ",guided" if w is not None else ""
        # and the spies do see a clipped call: the one-call step in graph + Philox mode, the separate kernel otherwise
        mod.ddim_sample(m, fp, "cuda", **cond, steps=3, x_T=x_T, use_graph=True, philox_seed=3, clip_denoised=True)
        assert calls == ["tdx_unet_eval_step_update[x0,sched" + g + "]"] * 4, calls     # one warm-up step, three captured
        calls.clear()
        mod.ddim_sample(m, fp, "cuda", **cond, steps=3, x_T=x_T, noises=zs, clip_denoised=True)
        assert calls == ["tdx_p_sample_update[x0,sched" + g + "]"] * 3, calls
        calls.clear()


# ---------------------------------------------------------------- 10. no stale state
@pytest.mark.parametrize("kind,w", [("uncond", None), ("cond", 2.0)])
def test_no_stale_state_between_clipped_and_unclipped_calls(kind, w):
    n = 4
    fp = ForwardProcess()
    m = _model(kind, 6)
    x_T, _, y = _inputs(kind, n, 1, seed=8)
    sched = ddim_schedule(fp, steps=12, eta=0.3)
    kw = dict(x_T=x_T, schedule=sched, guidance_scale=w, use_graph=True, philox_seed=3)   # sampling tables are on
    first = sample_loop(m, fp, "cuda", n, y, clip_denoised=True, **kw)
    second = sample_loop(m, fp, "cuda", n, y, **kw)
    third = sample_loop(m, fp, "cuda", n, y, clip_denoised=True, **kw)
    fourth = sample_loop(m, fp, "cuda", n, y, clip_denoised=(-0.5, 0.25), **kw)
    assert torch.equal(third, first)
    assert torch.equal(second, sample_loop(_model(kind, 6), fp, "cuda", n, y, **kw))
    assert torch.equal(first, sample_loop(_model(kind, 6), fp, "cuda", n, y, clip_denoised=True, **kw))
    assert torch.equal(fourth, sample_loop(_model(kind, 6), fp, "cuda", n, y, clip_denoised=(-0.5, 0.25), **kw))
    assert not torch.equal(first, second) and not torch.equal(first, fourth)
    assert first.abs().max() <= 1 and second.abs().max() > 1 and fourth.max() <= 0.25 and fourth.min() >= -0.5
