"""The training objective on the device: ``tdx_q_sample_target[_philox]`` (the v target written by the q_sample launch)
and ``tdx_mse_loss_grad_weighted`` (a per-timestep loss weight) against the entries they stand in for and against CPU
fp32 / fp64 restatements, ``TrainStep(prediction="v", loss_weighting="min_snr")`` against the existing forward and
backward around a ``d_out`` built with torch operations, the defaults against the step as it was, the captured step
against the eager one, and v-model sampling against an fp64 chain in x0 form.

The bitwise comparisons hold because the build has fp contraction off and every product / sum of the new kernels is
rounded on its own: a CPU tensor expression with one operation per rounding is the same arithmetic."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oracle import ref_laion as RLA  # noqa: E402
from oracle.weights import make_state_dict, make_state_dict_laion  # noqa: E402
from parity_helpers import rel_mse  # noqa: E402

from tiny_diffusion_amd._lib import check, lib  # noqa: E402
from tiny_diffusion_amd.schedule import (ForwardProcess, ddim_sample_loop, ddim_schedule, ddpm_schedule,  # noqa: E402
                                         loss_weights, sample_loop)

TDX_E_BADARG, TDX_E_SHAPE = -1, -2
T = 1000
CHAIN_TOL = 1e-8    # the project's chain tolerance (test_gpu_ddim.py: relative MSE against fp64)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _scratch():
    return torch.empty(lib.tdx_mse_scratch_bytes(), dtype=torch.uint8, device="cuda")


# ------------------------------------------------------------------ tdx_q_sample_target
# (3, 1x28x28): the MNIST sample, 588 float4 - three blocks of 256 lanes, the last partly filled; (2, 4x8x8): a sample
# boundary inside a block; (5, 20): the latent MLP's rows, five float4 each
Q_SHAPES = [(3, (1, 28, 28)), (2, (4, 8, 8)), (5, (20,))]


@functools.lru_cache(maxsize=None)
def _q_data(B, shape):
    """x0, noise, t (0 and T - 1 among them) on the CPU, shared and never written."""
    g = torch.Generator().manual_seed(B * 100 + len(shape))
    x0 = torch.rand(B, *shape, generator=g) * 2 - 1
    noise = torch.randn(B, *shape, generator=g)
    t = torch.randint(0, T, (B,), generator=g)
    t[0], t[-1] = 0, T - 1
    return x0, noise, t


def _v_cpu(fp, x0, noise, t):
    """v = sqrt_ac[t] noise - sqrt_1mac[t] x0 in CPU fp32: two products and one difference, each rounded once."""
    sa = torch.sqrt(fp.alphas_cumprod)[t].view(-1, *([1] * (x0.dim() - 1)))
    s1 = torch.sqrt(1.0 - fp.alphas_cumprod)[t].view(-1, *([1] * (x0.dim() - 1)))
    p, q = sa * noise, s1 * x0
    return p - q


def _q_target(fp, x0, noise, t, target, kind):
    sa, s1, _ = fp.tables("cuda")
    B = x0.shape[0]
    x_t = torch.full_like(x0, float("nan"))
    check(lib.tdx_q_sample_target(x0.data_ptr(), noise.data_ptr(), t.data_ptr(), sa.data_ptr(), s1.data_ptr(),
                                  x_t.data_ptr(), target.data_ptr(), B, x0.numel() // B, kind, _st()), "tdx_q_sample_target")
    return x_t


@pytest.mark.parametrize("B,shape", Q_SHAPES)
def test_q_sample_target_bitwise(B, shape):
    fp = ForwardProcess()
    x0c, nc, tc = _q_data(B, shape)
    x0, noise, t = x0c.cuda(), nc.cuda(), tc.cuda()
    want_xt, _ = fp.q_sample("cuda", x0, t, noise=noise)       # tdx_q_sample
    want_v = _v_cpu(fp, x0c, nc, tc)
    assert not torch.equal(want_v, nc)
    for kind, want in ((0, nc), (1, want_v)):
        target = torch.full_like(x0, float("nan"))
        x_t = _q_target(fp, x0, noise, t, target, kind)
        assert torch.equal(x_t, want_xt), (kind, "x_t")
        assert torch.equal(target.cpu(), want), (kind, "target")
        assert torch.equal(noise.cpu(), nc) and torch.equal(x0.cpu(), x0c)     # inputs untouched
        inplace = noise.clone()
        x_t = _q_target(fp, x0, inplace, t, inplace, kind)      # target == noise
        assert torch.equal(x_t, want_xt), (kind, "x_t in place")
        assert torch.equal(inplace.cpu(), want), (kind, "target in place")
    # the Python wrapper: a noise handed in is kept, the result is the same
    x_t, v = fp.q_sample_target("cuda", x0, t, noise=noise, prediction="v")
    assert torch.equal(x_t, want_xt) and torch.equal(v.cpu(), want_v) and torch.equal(noise.cpu(), nc)
    x_t, e = fp.q_sample_target("cuda", x0, t, noise=noise, prediction="eps")
    assert torch.equal(x_t, want_xt) and torch.equal(e.cpu(), nc)


@pytest.mark.parametrize("B,shape", Q_SHAPES)
def test_q_sample_target_philox_bitwise(B, shape):
    fp = ForwardProcess()
    x0c, _, tc = _q_data(B, shape)
    x0, t = x0c.cuda(), tc.cuda()
    seed, offset = 1234, 7
    want_xt, noise = fp.q_sample_philox(x0, t, seed, offset)    # tdx_q_sample_philox
    nc = noise.cpu()
    assert torch.isfinite(nc).all() and nc.std() > 0.5
    for pred, want in (("eps", nc), ("v", _v_cpu(fp, x0c, nc, tc))):
        x_t, target = fp.q_sample_target_philox(x0, t, seed, offset, prediction=pred)
        assert torch.equal(x_t, want_xt), pred
        assert torch.equal(target.cpu(), want), pred
    other, _ = fp.q_sample_target_philox(x0, t, seed, offset + 1, prediction="v")
    assert not torch.equal(other, want_xt)


# ------------------------------------------------------------------ tdx_mse_loss_grad_weighted
# The grid is min(ceil(n / 1024), 512) blocks of 256 lanes, so a lane makes about four grid-stride iterations at every
# size.  3 x 784 = 2352: three blocks, lanes cross sample boundaries.  200 x 784 = 156 800 (more than 512 x 256 elements):
# 154 blocks, many samples per lane.  700 x 784 = 548 800 > 512 x 1024: the block cap applies and lanes iterate further.
M_SIZES = [(3, 784), (200, 784), (700, 784)]
GSCALES = (1.0, 0.5)


@functools.lru_cache(maxsize=None)
def _m_data(B, per):
    gen = torch.Generator().manual_seed(B + per)
    a = torch.randn(B, per, generator=gen)
    b = torch.randn(B, per, generator=gen)
    a[0, :5] = b[0, :5]       # exact zeros in the difference
    t = torch.randint(0, T, (B,), generator=gen)
    t[0], t[1], t[-1] = 0, 130, T - 1      # SNR 1e4, SNR near gamma = 5 (the largest min-SNR weights), SNR 4e-5
    return a, b, t


def _weighted(a, b, t, w, gscale, want_grad=True):
    B, per = a.shape
    loss = torch.full((1,), float("nan"), device="cuda")
    d_a = torch.full_like(a, float("nan")) if want_grad else None
    check(lib.tdx_mse_loss_grad_weighted(a.data_ptr(), b.data_ptr(), t.data_ptr(), w.data_ptr(), loss.data_ptr(),
                                         None if d_a is None else d_a.data_ptr(), gscale, B, per,
                                         _scratch().data_ptr(), _st()), "tdx_mse_loss_grad_weighted")
    return loss, d_a


@pytest.mark.parametrize("B,per", M_SIZES)
def test_weighted_loss_with_ones_is_the_existing_entry(B, per):
    ac, bc, tc = _m_data(B, per)
    a, b, t = ac.cuda(), bc.cuda(), tc.cuda()
    ones = torch.ones(T, device="cuda")
    for gscale in GSCALES:
        want_loss = torch.full((1,), float("nan"), device="cuda")
        want_d = torch.full_like(a, float("nan"))
        check(lib.tdx_mse_loss_grad(a.data_ptr(), b.data_ptr(), want_loss.data_ptr(), want_d.data_ptr(), gscale,
                                    a.numel(), _scratch().data_ptr(), _st()), "tdx_mse_loss_grad")
        loss, d_a = _weighted(a, b, t, ones, gscale)
        assert torch.isfinite(want_d).all()
        assert torch.equal(loss, want_loss), gscale
        assert torch.equal(d_a, want_d), gscale
        loss2, none = _weighted(a, b, t, ones, gscale, want_grad=False)      # d_a = NULL
        assert none is None and torch.equal(loss2, want_loss)


@pytest.mark.parametrize("B,per", M_SIZES)
@pytest.mark.parametrize("prediction", ["eps", "v"])
def test_weighted_loss_min_snr_against_cpu(B, per, prediction):
    fp = ForwardProcess()
    ac, bc, tc = _m_data(B, per)
    a, b, t = ac.cuda(), bc.cuda(), tc.cuda()
    wc = loss_weights(fp, prediction, "min_snr")
    assert wc[tc].min() < 0.1 and wc[tc].max() > 0.5       # the weights really differ over the batch
    w = wc.cuda()
    n = B * per
    want64 = (wc[tc].double().view(B, 1) * (ac.double() - bc.double()) ** 2).sum().item() / n
    for gscale in GSCALES:
        loss, d_a = _weighted(a, b, t, w, gscale)
        # k_b = fl(fl(2 gscale / n) * w[t_b]), d_a = fl(fl(a - b) * k_b): fp32 on the CPU, one operation per rounding
        scale = (torch.tensor(2.0, dtype=torch.float32) * torch.tensor(gscale, dtype=torch.float32)) \
            / torch.tensor(float(n), dtype=torch.float32)
        k = (scale * wc[tc]).view(B, 1)
        d = ac - bc
        want_d = d * k
        assert torch.equal(d_a.cpu(), want_d), (gscale, (d_a.cpu() - want_d).abs().max().item())
        rel = abs(loss.item() - want64) / want64
        print(f"weighted loss B={B} {prediction} gscale={gscale}: {loss.item():.9g} vs fp64 {want64:.9g}, rel {rel:.2e}")
        assert rel < 1e-6, rel
        loss2, _ = _weighted(a, b, t, w, gscale, want_grad=False)
        assert torch.equal(loss2, loss)
    # a user table: weight 0 removes a sample from loss and gradient
    tab = torch.ones(T)
    tab[tc[1]] = 0.0
    keep = (tab[tc] != 0).double().view(B, 1)
    loss, d_a = _weighted(a, b, t, tab.cuda(), 1.0)
    assert torch.equal(d_a[1], torch.zeros_like(d_a[1])) and d_a[0].abs().max() > 0
    want = (keep * (ac.double() - bc.double()) ** 2).sum().item() / n
    assert abs(loss.item() - want) / want < 1e-6


def test_new_entries_refuse_bad_arguments():
    fp = ForwardProcess()
    sa, s1, _ = fp.tables("cuda")
    x0c, nc, tc = _q_data(3, (1, 28, 28))
    x0, noise, t = x0c.cuda(), nc.cuda(), tc.cuda()
    x_t, target = torch.full_like(x0, 7.0), torch.full_like(x0, 7.0)
    ptrs = [x0.data_ptr(), noise.data_ptr(), t.data_ptr(), sa.data_ptr(), s1.data_ptr(), x_t.data_ptr(), target.data_ptr()]
    for i in range(7):
        bad = list(ptrs)
        bad[i] = None
        assert lib.tdx_q_sample_target(*bad, 3, 784, 1, _st()) == TDX_E_BADARG, i
    pp = ptrs[:1] + ptrs[2:]     # the Philox form has no noise input
    for i in range(6):
        bad = list(pp)
        bad[i] = None
        assert lib.tdx_q_sample_target_philox(*bad, 3, 784, 1, 1, 0, _st()) == TDX_E_BADARG, i
    for kind in (-1, 2, 7):
        assert lib.tdx_q_sample_target(*ptrs, 3, 784, kind, _st()) == TDX_E_BADARG
        assert lib.tdx_q_sample_target_philox(*pp, 3, 784, kind, 1, 0, _st()) == TDX_E_BADARG
    for batch, per, code in ((0, 784, TDX_E_BADARG), (3, 0, TDX_E_BADARG), (-1, 784, TDX_E_BADARG), (3, 783, TDX_E_SHAPE),
                             (3, 782, TDX_E_SHAPE)):
        assert lib.tdx_q_sample_target(*ptrs, batch, per, 1, _st()) == code, (batch, per)
        assert lib.tdx_q_sample_target_philox(*pp, batch, per, 1, 1, 0, _st()) == code, (batch, per)

    ac, bc, tm = _m_data(3, 784)
    a, b, tm = ac.cuda(), bc.cuda(), tm.cuda()
    w = torch.ones(T, device="cuda")
    loss, d_a, scratch = torch.full((1,), 7.0, device="cuda"), torch.full_like(a, 7.0), _scratch()
    mp = [a.data_ptr(), b.data_ptr(), tm.data_ptr(), w.data_ptr(), loss.data_ptr(), d_a.data_ptr()]
    for i in range(5):      # d_a (index 5) may be NULL
        bad = list(mp)
        bad[i] = None
        assert lib.tdx_mse_loss_grad_weighted(*bad, 1.0, 3, 784, scratch.data_ptr(), _st()) == TDX_E_BADARG, i
    assert lib.tdx_mse_loss_grad_weighted(*mp, 1.0, 3, 784, None, _st()) == TDX_E_BADARG
    for batch, per in ((0, 784), (3, 0), (-3, 784), (3, -1)):
        assert lib.tdx_mse_loss_grad_weighted(*mp, 1.0, batch, per, scratch.data_ptr(), _st()) == TDX_E_BADARG
    torch.cuda.synchronize()
    for buf in (x_t, target, loss, d_a):       # a refused call launches nothing
        assert torch.equal(buf, torch.full_like(buf, 7.0))
    assert torch.equal(noise.cpu(), nc)


# ------------------------------------------------------------------ TrainStep
def _model(kind, seed=0):
    if kind == "uncond":
        from tiny_diffusion_amd.diffusion import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict(seed, False), strict=True)
    elif kind == "cond":
        from tiny_diffusion_amd.conditional_diffusion import NoiseModel
        m = NoiseModel()
        m.load_state_dict(make_state_dict(seed, True), strict=True)
    else:
        from tiny_diffusion_amd.conditional_diffusion_laion import NoiseModel
        m = NoiseModel(time_dim=768)
        m.load_state_dict(make_state_dict_laion(seed), strict=True)
    return m.cuda()


SHAPES = {"uncond": (1, 28, 28), "cond": (1, 28, 28), "laion": (4, 32, 32)}   # 32: the smallest side the LAION UNet takes


def _batch(kind, B, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = (torch.rand(B, *SHAPES[kind], generator=g) * 2 - 1).cuda()
    noise = torch.randn(B, *SHAPES[kind], generator=g).cuda()
    t = torch.randint(0, T, (B,), generator=g)
    t[0], t[1] = 3, 130            # SNR far above gamma = 5 (a small weight) and near it (the largest weights)
    if B > 2:
        t[-1] = T - 1              # the noisiest
    y = None if kind == "uncond" else (torch.randn(B, 768, generator=g) if kind == "laion"
                                        else torch.randint(0, 10, (B,), generator=g)).cuda()
    return x0, noise, t.cuda(), y


@pytest.mark.parametrize("kind,B,bf16", [("cond", 4, False), ("laion", 2, False), ("cond", 4, True)])
def test_train_step_v_min_snr_against_existing_forward_and_backward(kind, B, bf16):
    """The step's gradient against the same launches issued by hand on a second model - the existing forward, a
    ``d_out`` from torch operations, the existing backward: expected bit-equal (the same kernels on the same inputs;
    the new ones only produce ``x_t``, the target and ``d_out``, each checked bitwise above)."""
    from tiny_diffusion_amd.train import TrainStep
    from tiny_diffusion_amd.unet import MODE_TRAIN

    fp = ForwardProcess()
    x0, noise, t, y = _batch(kind, B, 17)
    models = [_model(kind, 3).train() for _ in range(2)]
    if bf16:
        for m in models:
            m.set_compute_dtype(torch.bfloat16)
    m1, m2 = models
    step = TrainStep(m1, fp, lr=1e-3, prediction="v", loss_weighting="min_snr")
    assert step._w_table is not None and step._w_table.is_cuda and step._w_table.shape == (T,)
    assert torch.equal(step._w_table.cpu(), loss_weights(fp, "v", "min_snr", 5.0))
    loss = step.step(x0, y, t=t, noise=noise).clone()
    grad1 = step.flat_grad.clone()

    x_t, target = fp.q_sample_target("cuda", x0, t, noise=noise, prediction="v")
    out, plan, _ = m2._run_forward(x_t, t, y, mode=MODE_TRAIN)
    n = out.numel()
    w = step._w_table[t]
    scale = torch.tensor(2.0, dtype=torch.float32, device="cuda") / torch.tensor(float(n), dtype=torch.float32, device="cuda")
    k = (scale * w).view(B, 1, 1, 1)
    d = out - target
    d_out = d * k
    flat2, views2 = m2._grad_buffers(torch.device("cuda", torch.cuda.current_device()))
    m2._run_backward(plan, d_out, views2)
    torch.cuda.synchronize()
    assert torch.isfinite(grad1).all() and grad1.abs().max() > 0
    diff = (grad1 - flat2).abs().max().item()
    print(f"TrainStep v/min_snr {kind} B={B} bf16={bf16}: max |grad - hand-issued grad| = {diff:.3e}")
    assert torch.equal(grad1, flat2), diff
    want = (w.double().view(B, 1, 1, 1) * (out.double() - target.double()) ** 2).sum().item() / n
    rel = abs(loss.item() - want) / want
    print(f"  returned loss {loss.item():.9g} vs fp64 {want:.9g}: rel {rel:.2e}")
    assert rel < 1e-6, rel
    # and the unweighted v loss / the weighted eps loss are other numbers: both keywords took effect
    plain = ((out.double() - target.double()) ** 2).mean().item()
    assert abs(plain - want) > 1e-3 * want
    assert not torch.equal(target, noise)


def _steps(model, x0, y, ts, noises, **kw):
    from tiny_diffusion_amd.train import TrainStep

    step = TrainStep(model, ForwardProcess(), lr=1e-3, **kw)
    losses = [step.step(x0, y, t=t, noise=e).item() for t, e in zip(ts, noises)]
    return step, losses


def test_defaults_are_the_step_as_it_was(monkeypatch):
    """Omitted keywords, explicit defaults: the same parameters after two steps, no table, and the new entries are
    never called.  eps with a table of ones goes through the weighted entry and still lands on the same bits."""
    B = 4
    x0, _, _, y = _batch("cond", B, 5)
    g = torch.Generator().manual_seed(6)
    ts = [torch.randint(0, T, (B,), generator=g).cuda() for _ in range(2)]
    noises = [torch.randn(B, 1, 28, 28, generator=g).cuda() for _ in range(2)]
    calls = []
    for name in ("tdx_q_sample_target", "tdx_q_sample_target_philox", "tdx_mse_loss_grad_weighted"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    omitted, l0 = _steps(_model("cond", 1).train(), x0, y, ts, noises)
    assert omitted._w_table is None and omitted._w_cpu is None and omitted.prediction == "eps"
    explicit, l1 = _steps(_model("cond", 1).train(), x0, y, ts, noises, prediction="eps", loss_weighting=None,
                          snr_gamma=5.0)
    assert explicit._w_table is None and explicit._w_cpu is None
    assert not calls
    assert l0 == l1 and torch.equal(omitted.flat_param, explicit.flat_param)
    ones, l2 = _steps(_model("cond", 1).train(), x0, y, ts, noises, loss_weighting=torch.ones(T))
    assert calls == ["tdx_mse_loss_grad_weighted"] * 2
    assert l2 == l0 and torch.equal(ones.flat_param, omitted.flat_param)
    # set_objective() on a step built with the other objective gives the default step back, and forth again
    from tiny_diffusion_amd.train import TrainStep
    sw = TrainStep(_model("cond", 1).train(), ForwardProcess(), lr=1e-3, prediction="v", loss_weighting="min_snr")
    assert sw._w_table is not None
    sw.set_objective()
    assert sw._w_table is None and sw.prediction == "eps" and sw.loss_weighting is None
    calls.clear()
    assert [sw.step(x0, y, t=t, noise=e).item() for t, e in zip(ts, noises)] == l0 and not calls
    assert torch.equal(sw.flat_param, omitted.flat_param)
    sw.set_objective("v", "min_snr")
    sw.step(x0, y, t=ts[0], noise=noises[0])
    assert calls == ["tdx_q_sample_target", "tdx_mse_loss_grad_weighted"] and sw._w_table is not None
    with pytest.raises(ValueError, match="prediction"):
        sw.set_objective("x0")
    assert sw.prediction == "v"
    # Philox noise: the v step draws the noise of the eps step (same key), so its x_t - and its first forward - agree
    pe = _steps(_model("cond", 1).train(), x0, y, ts[:1], [None], philox_seed=9)[0]
    calls.clear()
    pv = _steps(_model("cond", 1).train(), x0, y, ts[:1], [None], philox_seed=9, prediction="v")[0]
    assert calls == ["tdx_q_sample_target_philox"]
    assert not torch.equal(pe.flat_param, pv.flat_param) and torch.isfinite(pv.flat_param).all()


def test_captured_step_is_the_eager_step():
    """``use_graph=True`` with both keywords: t is drawn inside the graph and the weight is looked up by the loss kernel
    from the device table, so replays need nothing refreshed.  Three steps (eager warm-up, capture + replay, replay)
    against three eager steps under the same torch seeds, parameters bit for bit.  lr and the betas are powers of two /
    dyadic so that the step scalars of the two paths (C floats in the eager step, a device tensor filled from Python
    doubles in the captured one) are the same numbers - with lr = 1e-3 they differ in the last bit, which
    tests/test_gpu_unet.py::test_train_step_graph_capture_three_streams documents for the step as it was."""
    from tiny_diffusion_amd.train import TrainStep

    B = 8
    x0, _, _, y = _batch("cond", B, 23)
    out = []
    for use_graph in (False, True):
        m = _model("cond", 2).train()
        step = TrainStep(m, ForwardProcess(), lr=2.0 ** -10, betas=(0.5, 0.75), use_graph=use_graph, prediction="v",
                         loss_weighting="min_snr")
        torch.manual_seed(3)
        torch.cuda.manual_seed(3)
        rec = []
        for _ in range(3):
            loss = step.step(x0, y).item()
            rec.append((loss, step.flat_param.clone()))
        assert (step._graph is not None) == use_graph
        out.append(rec)
    eager, graph = out
    assert not torch.equal(eager[2][1], eager[1][1]) and not torch.equal(eager[1][1], eager[0][1])
    for k in range(3):
        diff = (eager[k][1] - graph[k][1]).abs().max().item()
        print(f"captured v/min_snr step {k}: loss {graph[k][0]:.6g} (eager {eager[k][0]:.6g}), max |dp| {diff:.3e}")
    for k in range(3):
        assert eager[k][0] == graph[k][0], k
        assert torch.equal(eager[k][1], graph[k][1]), k


# ------------------------------------------------------------------ sampling a v-model
NUM_CLASSES = 10
MODES = {"eager": dict(use_graph=False), "graph": dict(use_graph=True), "philox": dict(use_graph=True, philox_seed=7)}


def _fp64_forward(kind, seed):
    """fwd(x, t, y) in double; a label -1 (cond) is an appended zero row of the class embedding, a zero text
    embedding (laion) is the null condition as it stands."""
    if kind == "laion":
        sd = make_state_dict_laion(seed)
    else:
        sd = make_state_dict(seed, kind == "cond")
        if kind == "cond":
            w = sd["class_embedding.weight"]
            sd["class_embedding.weight"] = torch.cat([w, torch.zeros(1, w.shape[1], dtype=w.dtype)])
    p, b = R.split_state(sd)
    p = {k: v.double() for k, v in p.items()}

    def fwd(x, t, y):
        bb = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in b.items()}
        if kind == "laion":
            return RLA.unet_forward(p, bb, x, t, y.cpu().double(), training=False)
        if y is not None:
            y = y.cpu()
            y = torch.where(y < 0, torch.full_like(y, NUM_CLASSES), y)
        return R.unet_forward(p, bb, x, t, y, training=False)
    return fwd


@torch.no_grad()
def _v_chain64(fwd, kind, fp, taus, eta, x_T, y, w=None, zs=None):
    """The reverse chain of a v-model in x0 form, fp64 state (Song et al. 2021 eq. 12 with x0 = sa x - s1 v and
    eps = sa v + s1 x); ``w``: classifier-free guidance on v; zs[t] is the noise of the step at timestep t."""
    acp = fp.alphas_cumprod.double()
    x = x_T.double()
    n = x.shape[0]
    for k in reversed(range(len(taus))):
        t = taus[k]
        ab = acp[t].item()
        ab_prev = acp[taus[k - 1]].item() if k > 0 else 1.0
        tt = torch.full((n,), t, dtype=torch.long)
        if w is None:
            v = fwd(x, tt, y)
        else:
            null = torch.zeros_like(y) if kind == "laion" else torch.full_like(y, -1)
            o = fwd(torch.cat([x, x]), torch.cat([tt, tt]), torch.cat([y, null]))
            v = o[n:] + w * (o[:n] - o[n:])
        sa, s1 = math.sqrt(ab), math.sqrt(1 - ab)
        x0, eps = sa * x - s1 * v, sa * v + s1 * x
        sigma = eta * math.sqrt((1 - ab_prev) / (1 - ab)) * math.sqrt(1 - ab / ab_prev)
        x = math.sqrt(ab_prev) * x0 + math.sqrt(max(0.0, 1 - ab_prev - sigma ** 2)) * eps
        if k > 0 and sigma > 0:
            x = x + sigma * zs[t].double()
    return x


@pytest.mark.parametrize("kind,w", [("uncond", None), ("cond", 2.0), ("laion", None)])
def test_ddim_v_against_fp64(kind, w):
    n, S = 2, 10
    fp = ForwardProcess()
    m = _model(kind, 1)
    g = torch.Generator().manual_seed(11)
    x_T = torch.randn(n, *SHAPES[kind], generator=g)
    y = None if kind == "uncond" else (torch.randn(n, 768, generator=g) if kind == "laion"
                                        else torch.randint(0, NUM_CLASSES, (n,), generator=g)).cuda()
    taus = ddim_schedule(fp, steps=S).timesteps.tolist()
    want = _v_chain64(_fp64_forward(kind, 1), kind, fp, taus, 0.0, x_T, y, w)
    kw = {} if w is None else dict(guidance_scale=w)
    eps_chain = ddim_sample_loop(m, fp, "cuda", n, y, steps=S, x_T=x_T, **kw)
    for mode, mkw in MODES.items():
        got = ddim_sample_loop(m, fp, "cuda", n, y, steps=S, x_T=x_T, prediction="v", **kw, **mkw)
        r = rel_mse(got, want)
        print(f"DDIM v-prediction {kind} w={w} S={S} {mode}: relative MSE vs fp64 {r:.3e}")
        assert torch.isfinite(got).all()
        assert r < CHAIN_TOL, (mode, r)
        assert rel_mse(got, eps_chain) > 1e-3      # the same outputs read as eps give another sample


def test_ddpm_v_recorded_noise_graph_equals_eager():
    n, T20 = 2, 20
    fp = ForwardProcess(num_timesteps=T20)
    m = _model("uncond", 2)
    g = torch.Generator().manual_seed(5)
    x_T = torch.randn(n, 1, 28, 28, generator=g)
    zs = torch.randn(T20, n, 1, 28, 28, generator=g)
    eager = sample_loop(m, fp, "cuda", n, None, x_T=x_T, noises=zs, prediction="v")
    graph = sample_loop(m, fp, "cuda", n, None, x_T=x_T, noises=zs, prediction="v", use_graph=True)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, graph)
    assert torch.equal(eager, sample_loop(m, fp, "cuda", n, None, x_T=x_T, noises=zs,
                                          schedule=ddpm_schedule(fp).for_prediction(fp, "v")))
    assert not torch.equal(eager, sample_loop(m, fp, "cuda", n, None, x_T=x_T, noises=zs))
    # the module wrappers pass the keyword through
    from tiny_diffusion_amd.diffusion import ddim_sample, sample
    assert torch.equal(sample(m, fp, "cuda", n_samples=n, x_T=x_T, noises=zs, prediction="v"), eager)
    a = ddim_sample(m, fp, "cuda", n_samples=n, x_T=x_T, steps=5, prediction="v")
    assert torch.equal(a, sample_loop(m, fp, "cuda", n, None, x_T=x_T,
                                      schedule=ddim_schedule(fp, steps=5).for_prediction(fp, "v")))
    with pytest.raises(ValueError, match="prediction"):
        sample(m, fp, "cuda", n_samples=n, prediction="x0")
