"""Every dispatch branch of csrc/mlp.hip against fp64: the BatchNorm1d+ReLU kernels are chosen by the
batch size (register variants <2> <8> <16> <64> up to 32 / 128 / 256 / 1024 rows, then the three-sweep pair), LayerNorm
by N / 64, and the row ops of the transformer model run at more than one block.  The GEMM's load paths are covered by
the linear tests of tests/test_gpu_latent.py (_lin_cases).  Helpers and gates are those of test_gpu_latent.py and
test_gpu_transformer.py, unchanged."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import test_gpu_latent as TL  # noqa: E402
import test_gpu_transformer as TT  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from oracle import ref_latent as RL  # noqa: E402
from oracle import ref_transformer as RT  # noqa: E402
from oracle.weights import make_state_dict_latent, make_state_dict_transformer  # noqa: E402

BN_EPS = 1e-5
# BatchNorm module of unit u (csrc/mlp.hip LU[]) and the Linear in front of it
UNIT_BN = ("enc1.1", "enc1.4", "enc2.1", "enc2.4", "enc3.1", "enc3.4", "bottleneck.1", "dec3.1", "dec3.4", "dec2.1",
           "dec2.4", "dec1.1", "dec1.4")
# units whose activation lands in a concat buffer: unit -> (buffer, its width, first column, time projection added)
CAT_ROUTE = {1: ("cat1", 512, 256, None), 3: ("cat2", 256, 128, None), 5: ("cat3", 128, 64, None),
             6: ("cat3", 128, 0, "t1"), 8: ("cat2", 256, 0, "t2"), 10: ("cat1", 512, 0, "t3")}


def _latent_inputs(B):
    g = torch.Generator().manual_seed(31 + B)
    z = torch.randn(B, 20, generator=g)
    noise = torch.randn(B, 20, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    y = torch.randint(0, 10, (B,), generator=g)
    return z, noise, t, y


def _buffer_failures(model, b32, b64):
    """running_mean / running_var of the model against the fp64 oracle's buffers after the same step.  Distance: largest
    absolute difference over the buffer's largest magnitude; bound: 8 x the fp32 oracle's own distance on the same
    buffer (the factor of DESIGN.md 3.11), floor 1e-6.  num_batches_tracked must equal the oracle's (advanced once)."""
    bad = []
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            if int(v) != int(b64[k]):
                bad.append((k, int(v), int(b64[k])))
        elif "running_" in k:
            ref = b64[k].double()
            scale = ref.abs().max().item()
            err = (v.double().cpu() - ref).abs().max().item() / scale
            err32 = (b32[k].double() - ref).abs().max().item() / scale
            if not err <= max(8.0 * err32, 1e-6):
                bad.append((k, f"gpu {err:.2e}", f"cpu32 {err32:.2e}"))
    return bad


@pytest.mark.parametrize("B,training", [(33, True), (128, True), (129, True), (256, True), (257, True), (1024, True),
                                        (1025, True), (128, False), (257, False), (1025, False)])
def test_latent_step_vs_fp64_at_every_bn1d_variant(B, training):
    """One full step (forward, MSE, backward) at both sides of every bn1d_relu_{fwd,bwd} threshold: <8> at 33 and 128
    (128 is the batch of the benchmark's latent leg), <16> at 129 and 256, <64> at 257 and 1024, the three-sweep kernels
    at 1025; train mode, and eval mode with grad enabled (training = 0: running statistics normalise, and the Linear
    biases have the gradient s1 * gamma * rstd instead of zero - _grad_precision_failures excludes none there)."""
    sd = make_state_dict_latent(2)
    z, noise, t, y = _latent_inputs(B)
    m = TL.build(2)
    m.train(training)
    eps = m(z.cuda(), t.cuda(), y.cuda())
    loss = F.mse_loss(eps, noise.cuda())
    loss.backward()
    loss_ref, _, g32, b32 = RL.train_step_grads(sd, z, t, noise, y, training=training)
    _, eps64, g64, b64 = RL.train_step_grads(sd, z, t, noise, y, training=training, dtype=torch.float64)
    assert abs(loss.item() - loss_ref.item()) < 2e-5 * loss_ref.item()
    r = TL.rel_mse(eps.detach(), eps64)
    assert r < TL.REL_MSE_TOL, (B, training, r)
    bad = TL._grad_precision_failures({k: p.grad for k, p in m.named_parameters()}, g32, g64, training)
    assert not bad, (B, training, bad)
    bad = _buffer_failures(m, b32, b64)   # (eval mode: nothing may have moved)
    assert not bad, (B, training, bad)


def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def _bn_from_y(Y, gamma, beta, dtype):
    """mean | rstd | scale | shift of train-mode BatchNorm1d from the pre-activations Y, in `dtype` on the CPU."""
    Y, gamma, beta = Y.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean = Y.mean(0)
    rstd = 1.0 / torch.sqrt(Y.var(0, unbiased=False) + BN_EPS)
    scale = gamma * rstd
    return {"mean": mean, "rstd": rstd, "scale": scale, "shift": beta - mean * scale}


@pytest.mark.parametrize("B", [32, 33, 130, 257, 1025])
def test_latent_bn1d_units_from_their_own_input(B):
    """After a train-mode forward, every unit's scale | shift | mean | rstd ("ss{u}"), the running statistics it left
    behind (0.9 old + 0.1 batch, the variance unbiased) and, for the six units that write into the concat buffers, its
    activation relu(Y scale + shift) (+ t_k), recomputed in fp64 from the GPU's OWN Y{u}: no error of an earlier layer
    enters, so the gate is one kernel's rounding.  Bound: 8 x the distance of the same
    formulas in fp32 on the CPU (torch) from fp64, floor one fp32 ulp of the quantity's largest magnitude; outputs
    whose fp64 pre-ReLU value is within 1e-6 of zero are left out (under 0.1 % of them).  One B per kernel variant:
    <2> 32, <8> 33, <16> 130, <64> 257, three-sweep 1025.  Both column blocks of every concat buffer are checked, which
    pins ldo and the column offsets."""
    sd = make_state_dict_latent(2)
    z, _, t, y = _latent_inputs(B)
    m = TL.build(2)
    m.train()
    with torch.no_grad():
        m(z.cuda(), t.cuda(), y.cuda())
    plan = m._plan(B, torch.device("cuda", torch.cuda.current_device()))
    state = m.state_dict()
    grab = lambda name: plan.tensor(name).clone().cpu()   # noqa: E731
    cats = {name: grab(name).view(B, w) for name, w in (("cat1", 512), ("cat2", 256), ("cat3", 128))}
    tp = {name: grab(name).view(B, w) for name, w in (("t1", 64), ("t2", 128), ("t3", 256))}
    worst = {"gpu": 0.0, "cpu": 0.0}
    bad, skipped, total = [], 0, 0

    def gate(what, got, r32, r64, keep=None):
        e_gpu, e_cpu = (got.double() - r64).abs(), (r32.double() - r64).abs()
        if keep is not None:
            e_gpu, e_cpu = e_gpu[keep], e_cpu[keep]
        floor = _ulp32(r64.abs().max().item())
        g_, c_ = e_gpu.max().item(), e_cpu.max().item()
        worst["gpu"], worst["cpu"] = max(worst["gpu"], g_ / floor), max(worst["cpu"], c_ / floor)
        if not g_ <= max(8.0 * c_, floor):
            bad.append((what, f"gpu {g_:.3e}", f"cpu32 {c_:.3e}", f"ulp {floor:.3e}"))

    for u, bn in enumerate(UNIT_BN):
        N = sd[f"{bn}.weight"].numel()
        Y = grab(f"Y{u}").view(B, N)
        ss = grab(f"ss{u}").view(4, N)
        got = {"scale": ss[0], "shift": ss[1], "mean": ss[2], "rstd": ss[3]}
        r64 = _bn_from_y(Y, sd[f"{bn}.weight"], sd[f"{bn}.bias"], torch.float64)
        r32 = _bn_from_y(Y, sd[f"{bn}.weight"], sd[f"{bn}.bias"], torch.float32)
        for k in ("mean", "rstd", "scale", "shift"):
            gate(f"ss{u}.{k}", got[k], r32[k], r64[k])
        for dt, r in ((torch.float32, r32), (torch.float64, r64)):
            Yd = Y.to(dt)
            r["running_mean"] = 0.9 * sd[f"{bn}.running_mean"].to(dt) + 0.1 * Yd.mean(0)
            r["running_var"] = 0.9 * sd[f"{bn}.running_var"].to(dt) + 0.1 * Yd.var(0, unbiased=True)
        for k in ("running_mean", "running_var"):
            gate(f"{bn}.{k}", state[f"{bn}.{k}"].cpu(), r32[k], r64[k])
        if u in CAT_ROUTE:
            buf, _, c0, tk = CAT_ROUTE[u]
            pre64 = Y.double() * r64["scale"] + r64["shift"]
            o64 = torch.relu(pre64) + (tp[tk].double() if tk else 0.0)
            o32 = torch.relu(Y * r32["scale"] + r32["shift"]) + (tp[tk] if tk else 0.0)
            keep = pre64.abs() > 1e-6
            skipped += int((~keep).sum())
            total += keep.numel()
            gate(f"{buf}[:, {c0}:{c0 + N}] (unit {u})", cats[buf][:, c0:c0 + N], o32, o64, keep)
    print(f"bn1d units at B={B}: worst distance from fp64 in ulps of the largest magnitude: "
          f"gpu {worst['gpu']:.2f}, cpu fp32 {worst['cpu']:.2f}; {skipped} of {total} outputs at the ReLU kink left out")
    assert not bad, (B, bad)
    assert skipped < 1e-3 * total


def test_latent_forward_at_the_batch_limit():
    """B = 4096, the largest batch tdx_latent_forward takes (three-sweep BatchNorm kernels, 128 row tiles per GEMM):
    train-mode forward against fp64 and the running statistics as above, then the INFER forward (BatchNorm folded into
    the GEMM epilogue) on the statistics that step left behind.  No gradient gate here: the fp32 restatement's own
    median gradient distance from fp64 is 2.6e-4 at this size, a hundred times that of the other sizes, so a gate
    calibrated on it would show nothing."""
    B = 4096
    sd = make_state_dict_latent(2)
    z, _, t, y = _latent_inputs(B)
    p, b32 = R.split_state(sd)
    p64 = {k: v.double() for k, v in p.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in b32.items()}
    m = TL.build(2)
    m.train()
    with torch.no_grad():
        got = m(z.cuda(), t.cuda(), y.cuda())
        RL.noise_forward(p, b32, z, t, y, training=True)
        ref = RL.noise_forward(p64, b64, z.double(), t, y, training=True)
    r = TL.rel_mse(got, ref)
    assert r < TL.REL_MSE_TOL, r
    bad = _buffer_failures(m, b32, b64)
    assert not bad, bad
    m.eval()
    with torch.no_grad():
        got = m(z.cuda(), t.cuda(), y.cuda())
        ref = RL.noise_forward(p64, b64, z.double(), t, y, training=False)
    r = TL.rel_mse(got, ref)
    assert r < TL.REL_MSE_TOL, r


def test_latent_batch_over_the_limit_is_refused():
    """B = 4097 raises and leaves the model usable: a B = 8 forward afterwards still matches fp64, and the refused
    call moved no running statistic."""
    from tiny_diffusion_amd._lib import TdxError

    sd = make_state_dict_latent(2)
    m = TL.build(2)
    m.train()
    z, _, t, y = _latent_inputs(4097)
    with pytest.raises(TdxError):
        with torch.no_grad():
            m(z.cuda(), t.cuda(), y.cuda())
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    m.eval()
    p, b = R.split_state(sd)
    with torch.no_grad():
        got = m(z[:8].cuda(), t[:8].cuda(), y[:8].cuda())
        ref = RL.noise_forward({k: v.double() for k, v in p.items()},
                               {k: (v.double() if v.is_floating_point() else v) for k, v in b.items()},
                               z[:8].double(), t[:8], y[:8], training=False)
    assert TL.rel_mse(got, ref) < TL.REL_MSE_TOL


# ------------------------------------------------------------------------------------------------ LayerNorm
def _layer_norm_case(M, N, seed):
    from tiny_diffusion_amd import ops

    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, N, generator=g).cuda().requires_grad_(True)
    w = (1 + 0.1 * torch.randn(N, generator=g)).cuda().requires_grad_(True)
    b = (0.1 * torch.randn(N, generator=g)).cuda().requires_grad_(True)
    gy = torch.randn(M, N, generator=g).cuda()
    out = ops.layer_norm(x, w, b)
    out.backward(gy)
    xd, wd, bd = (u.detach().double().requires_grad_(True) for u in (x, w, b))
    ref = F.layer_norm(xd, (N,), wd, bd)
    ref.backward(gy.double())
    assert torch.allclose(out.double(), ref, rtol=1e-5, atol=1e-5)       # the tolerances of test_rowwise_ops_vs_torch
    for a, r in ((x, xd), (w, wd), (b, bd)):
        assert torch.allclose(a.grad.double(), r.grad, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("N", [64 * k for k in range(1, 17)])
def test_layernorm_every_width_of_the_contract(N):
    """include/tdx.h: N % 64 == 0, N <= 1024 - one instantiation per N / 64; M = 5 is a full block of four rows and a
    partial one."""
    _layer_norm_case(5, N, N)


@pytest.mark.parametrize("N", [192, 512])
@pytest.mark.parametrize("M", [1, 4, 1027])
def test_layernorm_row_counts(M, N):
    """a single row, exactly one block, and 257 blocks with a partial last one (dgamma / dbeta sum 1027 rows)."""
    _layer_norm_case(M, N, 1000 * M + N)


@pytest.mark.parametrize("N", [1088, 100])
def test_layernorm_outside_the_contract_raises(N):
    from tiny_diffusion_amd import ops
    from tiny_diffusion_amd._lib import TdxError

    with pytest.raises(TdxError):
        ops.layer_norm(torch.randn(5, N).cuda(), torch.ones(N).cuda(), torch.zeros(N).cuda())


def test_layernorm_with_a_large_common_offset():
    """x = 50 + randn: a one-pass variance E[x^2] - E[x]^2 loses 2500 : 1 of its digits here, the two-pass form of the
    kernel does not.  Bound: 8 x the distance of torch's fp32 CPU F.layer_norm from fp64 on the same input."""
    from tiny_diffusion_amd import ops

    g = torch.Generator().manual_seed(50)
    M, N = 37, 320
    x = 50 + torch.randn(M, N, generator=g)
    w = 1 + 0.1 * torch.randn(N, generator=g)
    b = 0.1 * torch.randn(N, generator=g)
    ref = F.layer_norm(x.double(), (N,), w.double(), b.double())
    e_cpu = (F.layer_norm(x, (N,), w, b).double() - ref).abs().max().item()
    got = ops.layer_norm(x.cuda(), w.cuda(), b.cuda()).cpu()
    e_gpu = (got.double() - ref).abs().max().item()
    print(f"layer_norm(50 + randn): distance from fp64 gpu {e_gpu:.3e}, torch fp32 cpu {e_cpu:.3e}")
    assert e_gpu <= 8.0 * e_cpu, (e_gpu, e_cpu)


# ------------------------------------------------------------------------------------------------ transformer model
def _transformer_vs_fp64(m_eval, m_train, sd, B, D):
    """eval eps_hat (rel. MSE < 1e-10) and dropout = 0 train gradients (err <= max(10 err32, 1e-4)) against
    oracle/ref_transformer.py in fp64: the two gates of test_transformer_forward_and_backward_match_reference_golden."""
    L = m_eval.latent_dim
    g = torch.Generator().manual_seed(77 + B)
    z = torch.randn(B, L, generator=g)
    noise = torch.randn(B, L, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    y = torch.randint(0, 10, (B,), generator=g)
    m_eval.eval()
    with torch.no_grad():
        eps = m_eval(z.cuda(), t.cuda(), y.cuda())
        ref = RT.noise_forward({k: v.double() for k, v in sd.items()}, z.double(), t, y)
    assert eps.shape == (B, L) and TT.rel_mse(eps, ref) < 1e-10, (B, TT.rel_mse(eps, ref))
    m_train.train()
    loss = F.mse_loss(m_train(z.cuda(), t.cuda(), y.cuda()), noise.cuda())
    loss.backward()
    _, _, g32 = RT.train_step_grads(sd, z, t, noise, y)
    _, _, g64 = RT.train_step_grads(sd, z, t, noise, y, dtype=torch.float64)
    for k, p in m_train.named_parameters():
        got = p.grad.detach().cpu()
        n64 = g64[k].norm().item()
        err = (got.double() - g64[k]).norm().item() / max(n64, 1e-30)
        err32 = (g32[k].double() - g64[k]).norm().item() / max(n64, 1e-30)
        assert err <= max(10 * err32, 1e-4), (B, k, err, err32)
        if k.endswith("attention.in_proj_weight"):
            assert float(got[:2 * D].abs().max()) == 0.0   # Q, K: exactly zero, as in the reference


@pytest.mark.parametrize("B", [1, 37, 130])
def test_transformer_vs_oracle_odd_batches(B):
    """The default model at a single row, at two ragged 32-row GEMM tiles and at five (the golden vectors are B = 16)."""
    _transformer_vs_fp64(TT.build(0), TT.build(0, dropout=0.0), make_state_dict_transformer(0), B, 256)


def test_transformer_time_dim_and_latent_dim_constructor_arguments():
    """NoiseModel(time_dim=192, latent_dim=10): a LayerNorm width off the powers of two (N / 64 = 3) and Linear layers
    whose row strides (10, and 1 for the time input) are no multiple of 4, i.e. the GEMM's scalar loads; the module's
    own default initialisation."""
    from tiny_diffusion_amd.diffusion_transformer import NoiseModel

    torch.manual_seed(5)
    m = NoiseModel(time_dim=192, latent_dim=10, dropout=0.0)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.cuda()
    _transformer_vs_fp64(m, m, sd, 37, 192)


# ------------------------------------------------------------------------------------------------ row ops
def test_embedding_bwd_many_rows_and_an_absent_class():
    from tiny_diffusion_amd import ops

    g = torch.Generator().manual_seed(11)
    M, N, absent = 300, 256, 4
    idx = torch.randint(0, 9, (M,), generator=g)
    idx = idx + (idx >= absent).long()          # 10 classes, class 4 never drawn
    assert set(idx.tolist()) == set(range(10)) - {absent}
    E = torch.randn(10, N, generator=g).cuda().requires_grad_(True)
    gy = torch.randn(M, N, generator=g)
    e = ops.embedding(E, idx.cuda())
    assert torch.equal(e, E.detach()[idx.cuda()])
    e.backward(gy.cuda())
    want = torch.zeros(10, N, dtype=torch.float64).index_add_(0, idx, gy.double())
    assert torch.allclose(E.grad.double().cpu(), want, rtol=2e-5, atol=2e-5)
    assert float(E.grad[absent].abs().max()) == 0.0


def test_add_broadcast_row_over_many_blocks():
    """tdx_add with a period of 130 over 1000 rows (508 blocks, the period no multiple of the block) is one rounded fp32
    addition per element: bit-equal to torch.  The row's gradient is a column sum of 1000 fp32 terms of size ~1, whose
    natural scale is its largest column: 2e-5 of that (the relative tolerance of the Linear tests, whose bias
    gradient is the same kernel)."""
    from tiny_diffusion_amd import ops

    g = torch.Generator().manual_seed(12)
    M, N = 1000, 130
    a = torch.randn(M, N, generator=g).cuda().requires_grad_(True)
    row = torch.randn(N, generator=g).cuda().requires_grad_(True)
    gy = torch.randn(M, N, generator=g)
    s = ops.add(a, row)
    assert torch.equal(s.detach().cpu(), a.detach().cpu() + row.detach().cpu())
    s.backward(gy.cuda())
    assert torch.equal(a.grad.cpu(), gy)
    want = gy.double().sum(0)
    err = (row.grad.double().cpu() - want).abs().max().item()
    assert err <= 2e-5 * want.abs().max().item(), (err, want.abs().max().item())


@pytest.mark.parametrize("group", [1, 64])
def test_dropout_backward_reuses_the_forward_mask(group):
    from tiny_diffusion_amd import ops

    g = torch.Generator().manual_seed(13)
    n, p = 4096 * 256 + 3, 0.05
    x = (0.5 + torch.rand(n, generator=g)).cuda().requires_grad_(True)    # no zeros: out == 0 <=> dropped
    gy = (0.5 + torch.rand(n, generator=g)).cuda()
    o = ops.dropout(x, p, group, 1234, 7)
    o.backward(gy)
    kept = o.detach() != 0
    assert 0.94 < kept.float().mean().item() < 0.96
    assert torch.equal(x.grad != 0, kept)
    scale = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))    # float32(1 / (1 - p)), as the kernel forms it
    assert float(scale) == float(np.float32(1.0 / (1.0 - p)))
    assert torch.equal(x.grad[kept], (gy * scale.cuda())[kept])
