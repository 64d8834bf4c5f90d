"""Transformer training, host side (no GPU): the new C entries are declared, listed and exported; the restatement of
the training step (tests/transformer_train_helpers.py) equals the CPU oracle in fp64, its Adam is torch's, it
reproduces the vectors of the reference's own ``NoiseModel`` + ``torch.optim.Adam`` (tests/golden/
transformer_train_B16.npz, tools/make_golden_transformer_train.py), its fp32 form stays well inside the parameter
bounds the GPU test uses, and ``TransformerTrainStep``'s argument errors come before any device work."""
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

import transformer_train_helpers as H
from oracle import ref_transformer as RT
from oracle.weights import make_state_dict_transformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tdx_transformer_train_workspace_floats", "tdx_transformer_loss_grads")
MAX_DIFF, LOOSE_SHARE = 2.1e-3, 5e-3     # test_gpu_latent.py::test_latent_train_step's two parameter bounds


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "transformer_train_B16.npz"))


@pytest.fixture(scope="module")
def inputs(golden_dir, fixture):
    src = np.load(os.path.join(golden_dir, "transformer_B16.npz"))
    z_t, t, y, noise = (torch.from_numpy(src[k]) for k in ("z_t", "t", "y", "noise"))
    pert = torch.from_numpy(fixture["pert"])
    return [(z_t + float(fixture["pert_scale"]) * pert[k], t, y, noise) for k in range(3)]


@pytest.fixture(scope="module")
def runs(inputs):
    """The three fixture steps in fp64 and fp32, computed once."""
    sd = make_state_dict_transformer(0)
    return {dt: H.train_steps(sd, inputs, dtype=dt, lr=1e-3) for dt in (torch.float64, torch.float32)}


def test_new_symbols_declared_listed_and_exported():
    import ctypes as C

    import tiny_diffusion_amd._lib as L
    import tiny_diffusion_amd.diffusion_transformer as DT

    hdr = open(os.path.join(ROOT, "include", "tdx.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS, name
        assert getattr(L.lib, name).argtypes is not None, name
    assert L.lib.tdx_version() == 400   # the ABI only grows
    assert "TransformerTrainStep" in DT.__all__
    # sizes are host arithmetic; the shape limits answer before anything is launched
    ws = lambda *a: L.lib.tdx_transformer_train_workspace_floats(C.byref(DT._TShape(*a)))   # noqa: E731
    B, Ld, D, L_ = 128, 20, 256, 4
    n = ws(B, Ld, D, 4, L_, 10, 0.05, 1e-5)
    assert n >= B * D * (L_ * 14 + 8)       # per block: 6 (B, D) and 2 (B, 4 D) activations
    for bad in ((B, Ld, 96, 4, L_, 10, 0.05, 1e-5), (B, Ld, 1088, 4, L_, 10, 0.05, 1e-5), (B, Ld, 256, 3, L_, 10, 0.05, 1e-5),
                (0, Ld, D, 4, L_, 10, 0.05, 1e-5), (B, Ld, D, 4, L_, 10, 1.0, 1e-5)):
        assert ws(*bad) == 0, bad
        s = DT._TShape(*bad)
        one = C.c_void_p(16)    # never dereferenced: the shape is refused first
        assert L.lib.tdx_transformer_loss_grads(C.byref(s), one, None, one, one, one, one, None, 0, 0, 0, None, 1.0, one,
                                                None, one, None) == -2
    assert ws(3, 7, 1024, 8, 1, 10, 0.0, 1e-5) > 0


def test_restatement_equals_the_oracle_in_fp64(inputs):
    sd = make_state_dict_transformer(0)
    z_t, t, y, noise = inputs[0]
    loss, eps, g = H.loss_grads(sd, z_t, t, y, noise, dtype=torch.float64)
    loss_o, eps_o, g_o = RT.train_step_grads(sd, z_t, t, noise, y, dtype=torch.float64)
    assert abs(float(loss) - float(loss_o)) <= 1e-12 * float(loss_o)
    assert float((eps - eps_o).norm()) <= 1e-12 * float(eps_o.norm())
    assert list(g) == list(g_o) == list(sd)
    for k in sd:
        assert float((g[k] - g_o[k]).norm()) <= 1e-12 * float(g_o[k].norm()), k
        if k.endswith("in_proj_weight") or k.endswith("in_proj_bias"):
            n = g[k].shape[0] // 3
            assert float(g[k][:2 * n].abs().max()) == 0.0 and float(g_o[k][:2 * n].abs().max()) == 0.0
    # all-ones masks are no masks, and a weight table of ones is the plain mean
    ones = []
    for _ in range(4):
        ones += [torch.ones(16, 4, dtype=torch.float64)] + [torch.ones(16, 256, dtype=torch.float64)] * 3
    loss1, eps1, _ = H.loss_grads(sd, z_t, t, y, noise, masks=ones, w_table=torch.ones(1000))
    assert torch.equal(eps1, eps) and abs(float(loss1) - float(loss)) <= 1e-14 * float(loss)


def test_helper_adam_is_torch_adam():
    g = torch.Generator().manual_seed(3)
    p0 = OrderedDict(a=torch.randn(7, 5, generator=g, dtype=torch.float64), b=torch.randn(11, generator=g, dtype=torch.float64))
    grads = [OrderedDict((k, torch.randn(v.shape, generator=g, dtype=torch.float64)) for k, v in p0.items()) for _ in range(4)]
    mine = H.Adam(p0, lr=1e-3)
    ref = [v.clone().requires_grad_(True) for v in p0.values()]
    opt = torch.optim.Adam(ref, lr=1e-3)
    for gr in grads:
        mine.step(gr)
        for r, gk in zip(ref, gr.values()):
            r.grad = gk.clone()
        opt.step()
    for r, v in zip(ref, mine.p.values()):
        assert torch.allclose(r.detach(), v, rtol=1e-13, atol=1e-15)
    # clipping: clip_grad_norm_'s coefficient
    mine = H.Adam(p0, lr=1e-3, max_grad_norm=0.5)
    ref = [v.clone().requires_grad_(True) for v in p0.values()]
    opt = torch.optim.Adam(ref, lr=1e-3)
    for r, gk in zip(ref, grads[0].values()):
        r.grad = gk.clone()
    torch.nn.utils.clip_grad_norm_(ref, 0.5)
    opt.step()
    mine.step(grads[0])
    for r, v in zip(ref, mine.p.values()):
        assert torch.allclose(r.detach(), v, rtol=1e-13, atol=1e-15)
    # the average: e += (1 - d_k)(p - e), d_k = min(decay, (1 + k) / (10 + k))
    from tiny_diffusion_amd.train import ema_decay_at

    mine = H.Adam(p0, lr=1e-2, ema_decay=0.999, ema_warmup=True)
    e = p0["a"].clone()
    for k, gr in enumerate(grads):
        mine.step(gr)
        e = e + (1.0 - ema_decay_at(k, 0.999, True)) * (mine.p["a"] - e)
    assert torch.allclose(mine.ema["a"], e, rtol=1e-14, atol=0)


def test_restatement_reproduces_the_reference_fixture(fixture, inputs, runs):
    sd = make_state_dict_transformer(0)
    losses, opt = runs[torch.float32]
    assert np.allclose(losses, fixture["losses"], rtol=2e-5, atol=0), (losses, fixture["losses"])
    _, _, g = H.loss_grads(sd, *inputs[0], dtype=torch.float32)
    diffs = []
    for k in sd:
        kk = k.replace(".", "__")
        gn = float(fixture["gnorm__" + kk])
        assert abs(g[k].double().norm().item() - gn) <= 2e-3 * gn + 1e-12, k     # test_gpu_transformer.py's bound
        head = torch.from_numpy(fixture["phead__" + kk])
        diffs.append((opt.p[k].reshape(-1)[: head.numel()] - head).abs())
    diffs = torch.cat(diffs)
    assert diffs.max().item() <= MAX_DIFF and (diffs > 1e-5).float().mean().item() <= LOOSE_SHARE


def test_fp32_restatement_stays_inside_the_parameter_bounds(runs):
    """Three Adam steps at lr 1e-3 move every element by up to 3e-3, and Adam's first steps are sign-like (m / sqrt(v)
    ~ +-1), so a gradient element whose fp32 rounding error is comparable to its size moves its parameter by a visible
    fraction of lr: that is what MAX_DIFF allows for.  Measured here (printed): max 7.2e-4, at most a share of 3.9e-4 of
    the elements of the worst tensor off by more than 1e-5."""
    sd = make_state_dict_transformer(0)
    l64, o64 = runs[torch.float64]
    l32, o32 = runs[torch.float32]
    assert np.allclose(l32, l64, rtol=2e-5, atol=0)     # the project's loss bound; measured 1e-7, 3.8e-6, 3.3e-6
    worst, worst_share = 0.0, 0.0
    for k in sd:
        diff = (o32.p[k].double() - o64.p[k]).abs()
        worst, worst_share = max(worst, diff.max().item()), max(worst_share, (diff > 1e-5).double().mean().item())
        if k.endswith("in_proj_weight") or k.endswith("in_proj_bias"):
            n = sd[k].shape[0] // 3
            assert torch.equal(o32.p[k][:2 * n], sd[k][:2 * n]), k      # Q / K rows: zero gradient, bit-unchanged
    print(f"fp32 vs fp64 restatement after 3 steps: max {worst:.3g}, worst share above 1e-5 {worst_share:.3g}")
    assert worst <= MAX_DIFF / 2 and worst_share <= LOOSE_SHARE / 2      # room to spare: half of each bound


def test_validation_errors_come_before_any_device_work():
    from tiny_diffusion_amd import _lib
    from tiny_diffusion_amd.diffusion_transformer import ForwardProcess, NoiseModel, TransformerTrainStep

    m = NoiseModel(time_dim=64, num_layers=1)   # on the CPU: every ValueError must come before the device is looked at
    fp = ForwardProcess()
    for kw in (dict(lr="1e-3"), dict(lr=None), dict(lr=True), dict(betas=(0.9, "x")), dict(betas=(0.9,)), dict(betas=0.9),
               dict(betas=(0.9, 1.0)), dict(eps=None), dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0),
               dict(prediction="x0"), dict(loss_weighting="snr"), dict(loss_weighting=torch.ones(7)),
               dict(snr_gamma=0.0), dict(ema_decay=1.5), dict(ema_decay=True), dict(ema_warmup=True),
               dict(philox_seed=-1), dict(philox_seed=1.5), dict(dropout_seed=-1), dict(dropout_seed=2 ** 64),
               dict(dropout_seed=True)):
        with pytest.raises(ValueError):
            TransformerTrainStep(m, fp, **kw)
    with pytest.raises(ValueError):
        TransformerTrainStep(torch.nn.Linear(2, 2), fp)
    with pytest.raises(ValueError):
        TransformerTrainStep(m, None)
    with pytest.raises(TypeError):
        TransformerTrainStep(m, fp, cond_drop_prob=0.1)      # this model has no null class
    with pytest.raises(_lib.TdxError, match="CUDA"):
        TransformerTrainStep(m, fp)                          # valid arguments, CPU module: no fallback
    assert m.pos_encoding.device.type == "cpu" and m.input_proj.weight.shape == (64, 20)   # and nothing was touched
    assert issubclass(_lib.TdxError, RuntimeError) and not issubclass(_lib.TdxError, ValueError)
