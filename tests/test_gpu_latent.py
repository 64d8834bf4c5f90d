"""GPU parity of the latent-space DDPM (latent_diffusion.py:16-154, 308-347,
vae.py:37-62) against vectors produced by the reference's own classes
(tests/golden/latent_B32.npz, tools/make_golden.py) and against the CPU oracle
(oracle/ref_latent.py).  Tolerances (fp32): eps_hat relative MSE <= 1e-10; gradients as close
to the fp64 gradient as the fp32 CPU oracle is."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ref_cpu as R  # noqa: E402
from oracle import ref_latent as RL  # noqa: E402
from oracle.weights import make_state_dict_latent, make_state_dict_vae  # noqa: E402

REL_MSE_TOL = 1e-10
ZERO_GRAD = ("time_embedding.2.bias", "time_proj1.bias", "time_proj2.bias", "time_proj3.bias", "initial_fc.bias")


def rel_mse(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b) ** 2).mean().item() / max((b**2).mean().item(), 1e-30)


def is_zero_grad(key):
    """exactly-zero true gradient under train-mode BatchNorm (see tests/test_oracle_latent.py)."""
    stage, idx, kind = (key.split(".") + ["", ""])[:3]
    return key in ZERO_GRAD or (kind == "bias" and idx in ("0", "3") and stage[:3] in ("enc", "dec", "bot"))


def build(seed=0):
    from tiny_diffusion_amd.latent_diffusion import NoiseModel

    m = NoiseModel()
    m.load_state_dict(make_state_dict_latent(seed), strict=True)
    return m.cuda()


def build_vae(seed=0):
    from tiny_diffusion_amd.latent_diffusion import VAE, VAEConfig

    v = VAE(VAEConfig())
    v.load_state_dict(make_state_dict_vae(seed), strict=True)
    return v.cuda()


def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "latent_B32.npz"))


def _lin_cases(extra=()):
    """(M, N, K, act, ldx, ldo, off).  The first block keeps its ids: ldx = K + 12, ldo = N + 8 and torch-aligned bases
    (every operand on the 16-byte load of stage_load / load4, K tails at chunk ends only).  The second block is the rest
    of load4's dispatch: ld % 4 != 0 (four guarded scalar loads, rows that start at every alignment), a K tail INSIDE a
    4-group of the vector path (c + 3 < C fails next to random padding), and ld % 4 == 0 with every base one float into
    its allocation (off = 1: scalar path by the pointer test alone)."""
    old = [(1, 20, 512, 0), (37, 400, 784, 1), (130, 784, 400, 2), (16, 512, 20, 1), (128, 64, 64, 0)] + list(extra)
    cases = [pytest.param(M, N, K, act, K + 12, N + 8, 0, id=f"{M}-{N}-{K}-{act}") for M, N, K, act in old]
    new = [(3, 36, 50, 1, 50, 37, 0), (33, 5, 36, 0, 39, 7, 0), (130, 130, 130, 2, 131, 133, 0),
           (16, 64, 258, 1, 258, 66, 0), (8, 32, 130, 0, 132, 36, 0), (16, 64, 256, 2, 260, 72, 1)]
    return cases + [pytest.param(*c, id="-".join(map(str, c[:4])) + f"-ld{c[4]}-{c[5]}-off{c[6]}") for c in new]


class _Block:
    """A (rows, ld) matrix that starts `off` floats into a CUDA allocation of its own, with `off` guard floats before
    and one behind it.  Outputs (src None) are filled with 7.0, guards included; inputs carry NaN guards, so a kernel
    that reads one float outside the block poisons its result."""

    def __init__(self, rows, ld, off, src=None):
        n = rows * ld
        flat = torch.full((off + n + 1,), 7.0 if src is None else float("nan"))
        if src is not None:
            flat[off:off + n] = src.reshape(-1)
        self.flat = flat.cuda()
        self.m = self.flat[off:off + n].view(rows, ld)
        self.off, self.n = off, n
        assert self.m.data_ptr() % 16 == (4 * off) % 16

    def ptr(self):
        return self.m.data_ptr()

    def guards_untouched(self):
        return bool((self.flat[:self.off] == 7.0).all()) and float(self.flat[self.off + self.n]) == 7.0


@pytest.mark.parametrize("M,N,K,act,ldx,ldo,off", _lin_cases())
def test_linear_fwd_bwd_vs_torch(M, N, K, act, ldx, ldo, off):
    """tdx_linear_fwd / tdx_linear_bwd with row strides, ragged tiles and K tails; both load paths of the GEMM (see
    _lin_cases); nothing outside the M x N / M x K / N x K / N results is written."""
    from tiny_diffusion_amd._lib import lib, check

    g = torch.Generator().manual_seed(M * 7 + N)
    xb = _Block(M, ldx, off, torch.randn(M, ldx, generator=g))
    w = _Block(N, K, off, torch.randn(N, K, generator=g) / K**0.5)
    b = torch.randn(N, generator=g).cuda()
    ob = _Block(M, ldo, off)
    check(lib.tdx_linear_fwd(xb.ptr(), ldx, w.ptr(), b.data_ptr(), ob.ptr(), ldo, M, N, K, act, None), "fwd")
    x = xb.m[:, :K]
    ref = F.linear(x.double(), w.m.double(), b.double())
    ref = torch.relu(ref) if act == 1 else torch.sigmoid(ref) if act == 2 else ref
    assert torch.allclose(ob.m[:, :N].double(), ref, rtol=2e-5, atol=2e-5)
    assert bool((ob.m[:, N:] == 7.0).all())  # the padding columns are not touched
    assert ob.guards_untouched()
    gyb = _Block(M, ldo, off, torch.randn(M, ldo, generator=g))
    gx, dw, db = _Block(M, ldx, off), _Block(N, K, off), _Block(1, N, 0)
    check(lib.tdx_linear_bwd(gyb.ptr(), ldo, xb.ptr(), ldx, w.ptr(), gx.ptr(), ldx, dw.ptr(),
                             db.ptr(), M, N, K, None), "bwd")
    gy = gyb.m[:, :N].double()
    assert torch.allclose(dw.m.double(), gy.t() @ x.double(), rtol=2e-5, atol=2e-5)
    assert torch.allclose(db.m[0].double(), gy.sum(0), rtol=2e-5, atol=2e-5)
    assert torch.allclose(gx.m[:, :K].double(), gy @ w.m.double(), rtol=2e-5, atol=2e-5)
    assert bool((gx.m[:, K:] == 7.0).all())
    assert gx.guards_untouched() and dw.guards_untouched() and db.guards_untouched()


@pytest.mark.parametrize("M,N,K,act,ldx,ldo,off", _lin_cases(extra=[(32, 512, 512, 1)]))
def test_linear_bf16_mode_same_arithmetic_on_the_host(M, N, K, act, ldx, ldo, off):
    """tdx_linear_{fwd,bwd}_prec with TDX_PREC_BF16 (gemm_bf16_kernel: operands rounded to bf16, v_mfma_f32_32x32x16_bf16,
    fp32 accumulation) against the SAME arithmetic on the host - operands rounded to bf16 (nearest even), exact
    products, fp64 sums: what is left is fp32 accumulation order (<= 2e-5); row strides, ragged tiles, K tails and both
    load paths as in the fp32 test (_lin_cases); TDX_PREC_F32 through the same entry equals tdx_linear_fwd bit for bit."""
    from tiny_diffusion_amd._lib import lib, check

    r16 = lambda v: v.to(torch.bfloat16).double()   # noqa: E731
    g = torch.Generator().manual_seed(M * 11 + N)
    xb = _Block(M, ldx, off, torch.randn(M, ldx, generator=g))
    w = _Block(N, K, off, torch.randn(N, K, generator=g) / K**0.5)
    b = torch.randn(N, generator=g).cuda()
    ob = _Block(M, ldo, off)
    check(lib.tdx_linear_fwd_prec(xb.ptr(), ldx, w.ptr(), b.data_ptr(), ob.ptr(), ldo, M, N, K, act, 1, None))
    x = xb.m[:, :K]
    ref = r16(x) @ r16(w.m).t() + b.double()
    ref = torch.relu(ref) if act == 1 else torch.sigmoid(ref) if act == 2 else ref
    assert torch.allclose(ob.m[:, :N].double(), ref, rtol=2e-5, atol=2e-5)
    assert bool((ob.m[:, N:] == 7.0).all())
    assert ob.guards_untouched()
    exact = F.linear(x.double(), w.m.double(), b.double())   # and it IS a different arithmetic from fp32
    exact = torch.relu(exact) if act == 1 else torch.sigmoid(exact) if act == 2 else exact
    if K >= 64:
        assert (ob.m[:, :N].double() - exact).abs().max() > 1e-4
    gyb = _Block(M, ldo, off, torch.randn(M, ldo, generator=g))
    gx, dw, db = _Block(M, ldx, off), _Block(N, K, off), _Block(1, N, 0)
    check(lib.tdx_linear_bwd_prec(gyb.ptr(), ldo, xb.ptr(), ldx, w.ptr(), gx.ptr(), ldx, dw.ptr(),
                                  db.ptr(), M, N, K, 1, None))
    gy = gyb.m[:, :N]
    assert torch.allclose(dw.m.double(), r16(gy).t() @ r16(x), rtol=2e-5, atol=2e-5)
    assert torch.allclose(db.m[0].double(), gy.double().sum(0), rtol=2e-5, atol=2e-5)      # bias gradient: plain fp32 sum
    assert torch.allclose(gx.m[:, :K].double(), r16(gy) @ r16(w.m), rtol=2e-5, atol=2e-5)
    assert bool((gx.m[:, K:] == 7.0).all())
    assert gx.guards_untouched() and dw.guards_untouched() and db.guards_untouched()
    o32a, o32b = _Block(M, ldo, off), _Block(M, ldo, off)
    check(lib.tdx_linear_fwd_prec(xb.ptr(), ldx, w.ptr(), b.data_ptr(), o32a.ptr(), ldo, M, N, K, act, 0, None))
    check(lib.tdx_linear_fwd(xb.ptr(), ldx, w.ptr(), b.data_ptr(), o32b.ptr(), ldo, M, N, K, act, None))
    assert torch.equal(o32a.m[:, :N], o32b.m[:, :N])


def test_latent_bf16_mode_against_reference_autocast_yardstick(golden_dir):
    """BASELINE.json configs[3] (latent_diffusion.py in bf16): model.set_compute_dtype(torch.bfloat16) runs the Linear
    layers of the latent noise model on the bf16 MFMA (fp32 accumulation, fp32 BatchNorm1d and time path).  Gate
    (tests/parity_helpers.py::AutocastYardstick, BF16_K = 1): no further from the reference's fp32 vectors than the
    REFERENCE's own module is under torch.autocast(bfloat16) on the same inputs (latent_diffusion.py:16-128;
    tests/golden/bf16_autocast.npz) - eps_hat MSE in train and eval mode, worst and median gradient cosine, loss; then
    the T = 10 reverse chain and one TrainStep in bf16 mode; and back to fp32 bit for bit."""
    from parity_helpers import AutocastYardstick
    from tiny_diffusion_amd.latent_diffusion import ForwardProcess, sample
    from tiny_diffusion_amd.train import TrainStep

    d = golden(golden_dir)
    yard = AutocastYardstick("latent_B32", skip=is_zero_grad)
    z_t, t, y = (torch.from_numpy(d[k]).cuda() for k in ("z_t", "t", "y"))
    noise = torch.from_numpy(d["noise"])
    sd = make_state_dict_latent(0)
    _, _, g32, _ = RL.train_step_grads(sd, z_t.cpu(), t.cpu(), noise, y.cpu())
    m = build(0).train()
    assert m.compute_dtype == torch.float32
    m.set_compute_dtype(torch.bfloat16)
    assert m.compute_dtype == torch.bfloat16
    eps = m(z_t, t, y)
    loss = F.mse_loss(eps, noise.cuda())
    loss.backward()
    ref = torch.from_numpy(d["eps_train"]).double()
    mse = ((eps.detach().cpu().double() - ref) ** 2).mean().item()
    assert mse > 1e-9, "bf16 mode produced the fp32 result: the precision switch did nothing"
    cos = []
    for k, p in m.named_parameters():
        if is_zero_grad(k):
            continue
        a, b = p.grad.double().reshape(-1).cpu(), g32[k].double().reshape(-1)
        cos.append(((a @ b / (a.norm() * b.norm())).item(), k))
    cos.sort()
    yard.check("latent B32 train", eps_mse=mse, cos_sorted=cos, loss=loss.item(), loss_ref=float(d["loss_train"]))
    m2 = build(0).eval().set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        e2 = m2(z_t, t, y)
    ref2 = torch.from_numpy(d["eps_eval"]).double()
    yard.check("latent B32 eval", eps_mse=((e2.cpu().double() - ref2) ** 2).mean().item(), eval_mode=True)
    # reverse chain (graph replay) in bf16 mode against the reference's fp32 chain
    T, n = int(d["chain_T"]), d["chain_z_T"].shape[0]
    v = build_vae(0)
    img = sample(v, m2, ForwardProcess(num_timesteps=T), "cuda", n_samples=n, y=y[:n].cpu(), x_T=torch.from_numpy(d["chain_z_T"]),
                 noises=torch.from_numpy(d["chain_zs"]), use_graph=True)
    fin = torch.from_numpy(d["chain_img"]).double()
    relc = ((img.cpu().double() - fin) ** 2).mean().item() / (fin ** 2).mean().item()
    print(f"latent bf16 chain T={T}: relative MSE of the decoded images {relc:.3e}")
    assert torch.isfinite(img).all() and relc < 1e-2
    # four optimisation steps in both modes from the same weights and the same noise: the loss curves stay together (5 %:
    # at B = 32 and lr = 1e-3 four Adam steps amplify the forward's 1e-4 differences to a few per cent: measured 3.6 %)
    losses = {}
    for dt in (torch.float32, torch.bfloat16):
        mm = build(0).train().set_compute_dtype(dt)
        ts = TrainStep(mm, ForwardProcess(), lr=1e-3, philox_seed=3)
        losses[dt] = [float(ts.step(torch.from_numpy(d["z0"]).cuda(), y=y, t=t)) for _ in range(4)]
    a, b = losses[torch.float32], losses[torch.bfloat16]
    print("latent train steps fp32", a, "bf16", b)
    assert all(abs(p - q) <= 0.05 * abs(p) for p, q in zip(a, b)) and b[-1] < b[0]
    # and back
    m.set_compute_dtype(torch.float32)
    m.load_state_dict(sd); m.train()
    with torch.no_grad():
        e32 = m(z_t, t, y)
    assert rel_mse(e32, torch.from_numpy(d["eps_train"])) < REL_MSE_TOL


def test_vae_matches_reference_golden(golden_dir):
    d = golden(golden_dir)
    v = build_vae(0)
    x = torch.from_numpy(d["x_img"]).cuda()
    mu, logvar = v.encode(x)
    assert torch.allclose(mu.cpu(), torch.from_numpy(d["mu"]), rtol=2e-5, atol=2e-6)
    assert torch.allclose(logvar.cpu(), torch.from_numpy(d["logvar"]), rtol=2e-5, atol=2e-6)
    z0 = v.reparameterize(mu, logvar, eps=torch.from_numpy(d["eps_vae"]).cuda())
    assert torch.allclose(z0.cpu(), torch.from_numpy(d["z0"]), rtol=2e-5, atol=2e-6)
    dec = v.decode(torch.from_numpy(d["z0"]).cuda())
    assert torch.allclose(dec.cpu(), torch.from_numpy(d["dec"]), rtol=2e-5, atol=2e-6)
    torch.manual_seed(3)
    rec, mu2, lv2 = v(x.view(-1, 1, 28, 28))      # forward(): view(-1, 784) -> encode -> reparameterize -> decode
    assert rec.shape == (32, 784) and torch.equal(mu2, mu) and float(rec.min()) >= 0 and float(rec.max()) <= 1
    with pytest.raises(Exception):
        v.encode(torch.zeros(2, 784))  # CPU tensor: no fallback


def test_latent_module_contract():
    from tiny_diffusion_amd.latent_diffusion import ForwardProcess, NoiseModel, sample

    m = NoiseModel(time_dim=256, num_classes=10, latent_dim=20)
    ref = make_state_dict_latent(0)
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    for k in ref:
        assert tuple(sd[k].shape) == tuple(ref[k].shape) and sd[k].dtype == ref[k].dtype, k
    with pytest.raises(ValueError):
        NoiseModel(latent_dim=32)
    m, v = m.cuda(), build_vae()
    fp = ForwardProcess(num_timesteps=2)
    with pytest.raises(ValueError):
        sample(v, m, fp, "cuda", n_samples=4)
    with pytest.raises(ValueError):
        sample(v, m, fp, "cuda", n_samples=4, y=torch.zeros(3, dtype=torch.long))
    with pytest.raises(Exception):
        m(torch.randn(2, 20), torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long))
    torch.manual_seed(1)
    img = sample(v, m, fp, "cuda", n_samples=4, y=torch.tensor([1, 2, 3, 4]))
    assert img.shape == (4, 1, 28, 28) and m.training is False and torch.isfinite(img).all()
    # q_sample on (B,20) draws its own noise and returns it (latent_diffusion.py:143-154)
    z0 = torch.randn(6, 20).cuda()
    t = torch.tensor([0, 999, 5, 500, 10, 100]).cuda()
    z_t, eps = ForwardProcess().q_sample("cuda", z0, t)
    want = RL.q_sample(R.Schedule(), z0.cpu(), t.cpu(), eps.cpu())
    assert torch.equal(z_t.cpu(), want)


def test_latent_forward_matches_reference_golden(golden_dir):
    d = golden(golden_dir)
    z_t, t, y = (torch.from_numpy(d[k]).cuda() for k in ("z_t", "t", "y"))
    noise = torch.from_numpy(d["noise"]).cuda()
    for mode in ("train", "eval"):
        m = build(0)
        m.train(mode == "train")
        ref = torch.from_numpy(d[f"eps_{mode}"])
        with torch.no_grad():
            eps = m(z_t, t, y)
        assert eps.shape == (32, 20) and eps.dtype == torch.float32
        r = rel_mse(eps, ref)
        assert r < REL_MSE_TOL, f"{mode}: relative MSE {r:.3e}"
        loss = F.mse_loss(eps, noise).item()
        assert abs(loss - float(d[f"loss_{mode}"])) <= 2e-5 * abs(float(d[f"loss_{mode}"]))
        if mode == "train":
            for k, v in m.state_dict().items():
                if "running_" in k:
                    assert torch.allclose(v.cpu(), torch.from_numpy(d["buf__" + k.replace(".", "__")]),
                                          rtol=2e-5, atol=2e-5), k
                if "num_batches" in k:
                    assert int(v) == 2
        else:
            eps2 = m(z_t, t, y)  # eval + grad enabled (unfused path)
            assert eps2.requires_grad and rel_mse(eps2.detach(), ref) < REL_MSE_TOL


def test_latent_forward_vs_oracle_odd_batches():
    for B, modes in ((1, (False,)), (3, (True, False)), (130, (True, False))):
        sd = make_state_dict_latent(1)
        m = build(1)
        g = torch.Generator().manual_seed(B)
        z = torch.randn(B, 20, generator=g)
        t = torch.randint(0, 1000, (B,), generator=g); t[0] = 999
        y = torch.randint(0, 10, (B,), generator=g)
        for training in modes:
            m.train(training)
            p, b = R.split_state(sd)
            p64 = {k: v.double() for k, v in p.items()}
            b64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in b.items()}
            with torch.no_grad():
                ref = RL.noise_forward(p, b, z, t, y, training=training)
                ref64 = RL.noise_forward(p64, b64, z.double(), t, y, training=training)
                got = m(z.cuda(), t.cuda(), y.cuda())
            # batch statistics over 3 rows leave some features with var << eps, where 1/sqrt(var+eps)
            # multiplies fp32 rounding noise by ~300: calibrate on the fp32 oracle's own distance
            # from the fp64 evaluation
            tol = max(1e-10, 20.0 * rel_mse(ref, ref64))
            assert rel_mse(got, ref64) < tol, (B, training, rel_mse(got, ref64), tol)
            m.load_state_dict(sd)


def _grad_precision_failures(got, g32, g64, training, k_factor=10.0, floor=1e-4):
    errs_cpu = {k: (g32[k].double() - g64[k]).norm().item() / max(g64[k].norm().item(), 1e-30) for k in g64}
    usable = [e for k, e in errs_cpu.items() if not (training and is_zero_grad(k))]
    med = float(np.median(usable))
    bad = []
    for k, g in got.items():
        if training and is_zero_grad(k):
            continue
        n64 = g64[k].norm().item()
        err = (g.detach().double().cpu() - g64[k]).norm().item() / max(n64, 1e-30)
        tol = max(k_factor * errs_cpu[k], k_factor * med, floor)
        if not err <= tol:
            bad.append((k, f"gpu {err:.2e}", f"cpu32 {errs_cpu[k]:.2e}", f"tol {tol:.2e}"))
    return bad


def test_latent_backward_matches_reference_golden(golden_dir):
    """loss.backward() + Adam step through the module (latent_diffusion.py:214-222)."""
    d = golden(golden_dir)
    m = build(0)
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    z_t, t, y, noise = (torch.from_numpy(d[k]) for k in ("z_t", "t", "y", "noise"))
    loss = F.mse_loss(m(z_t.cuda(), t.cuda(), y.cuda()), noise.cuda())
    opt.zero_grad()
    loss.backward()
    assert abs(loss.item() - float(d["loss_train"])) <= 2e-5 * float(d["loss_train"])
    bad = []
    for k, p in m.named_parameters():
        kk = k.replace(".", "__")
        got = p.grad.detach().contiguous().view(-1).cpu()
        gn = float(d[f"gnorm__{kk}"])
        if is_zero_grad(k):
            wn = float(d[f"gnorm__{kk.replace('bias', 'weight')}"])
            if not got.double().norm().item() <= 2e-5 * wn:
                bad.append((k, "zero-grad bias", got.double().norm().item(), wn))
            continue
        head = torch.from_numpy(d[f"ghead__{kk}"])
        e_norm = abs(got.double().norm().item() - gn) / gn
        rms = gn / np.sqrt(got.numel())
        e_head = (got[: head.numel()] - head).abs().max().item() / max(head.abs().max().item(), rms)
        if e_norm > 2e-3 or e_head > 3e-2:
            bad.append((k, e_norm, e_head))
    assert not bad, bad
    sd0 = make_state_dict_latent(0)
    _, _, g32, _ = RL.train_step_grads(sd0, z_t, t, noise, y)
    _, _, g64, _ = RL.train_step_grads(sd0, z_t, t, noise, y, dtype=torch.float64)
    bad = _grad_precision_failures({k: p.grad for k, p in m.named_parameters()}, g32, g64, True)
    assert not bad, bad
    opt.step()
    for k, p in m.named_parameters():
        if is_zero_grad(k):
            continue
        kk = k.replace(".", "__")
        head = torch.from_numpy(d[f"adam_head__{kk}"])
        got = p.detach().contiguous().view(-1)[: head.numel()].cpu()
        ghead = torch.from_numpy(d[f"ghead__{kk}"])[: head.numel()].abs()
        tol = torch.where(ghead > 1e-5, torch.tensor(2e-6), torch.tensor(1.05e-3))
        assert bool(((got - head).abs() <= tol).all()), k


def test_latent_backward_vs_oracle_full_tensors():
    for B, training in ((5, True), (130, True), (7, False)):
        sd = make_state_dict_latent(2)
        g = torch.Generator().manual_seed(31 + B)
        z = torch.randn(B, 20, generator=g)
        noise = torch.randn(B, 20, generator=g)
        t = torch.randint(0, 1000, (B,), generator=g)
        y = torch.randint(0, 10, (B,), generator=g)
        m = build(2)
        m.train(training)
        loss = F.mse_loss(m(z.cuda(), t.cuda(), y.cuda()), noise.cuda())
        loss.backward()
        loss_ref, _, g32, _ = RL.train_step_grads(sd, z, t, noise, y, training=training)
        _, _, g64, _ = RL.train_step_grads(sd, z, t, noise, y, training=training, dtype=torch.float64)
        assert abs(loss.item() - loss_ref.item()) < 2e-5 * loss_ref.item()
        bad = _grad_precision_failures({k: p.grad for k, p in m.named_parameters()}, g32, g64, training)
        assert not bad, (B, training, bad)


@pytest.mark.parametrize("use_graph", [False, True])
def test_latent_sample_chain_recorded_noise(golden_dir, use_graph):
    from tiny_diffusion_amd.latent_diffusion import ForwardProcess, sample
    from tiny_diffusion_amd.schedule import sample_loop

    d = golden(golden_dir)
    m, v = build(0), build_vae(0)
    m.train()
    T = int(d["chain_T"])
    fp = ForwardProcess(num_timesteps=T)
    y = torch.from_numpy(d["y"])[:4]
    kw = dict(x_T=torch.from_numpy(d["chain_z_T"]), noises=torch.from_numpy(d["chain_zs"]), use_graph=use_graph)
    z = sample_loop(m, fp, "cuda", 4, y, **kw)
    assert rel_mse(z, torch.from_numpy(d["chain_final"])) < 1e-9
    img = sample(v, m, fp, "cuda", n_samples=4, y=y, **kw)
    assert img.shape == (4, 1, 28, 28)
    assert torch.allclose(img.cpu(), torch.from_numpy(d["chain_img"]), rtol=1e-4, atol=1e-5)


def test_latent_train_step():
    """TrainStep on latents: vae.encode -> reparameterize -> q_sample -> fwd -> mse -> bwd -> Adam
    (latent_diffusion.py:199-222) against the module + torch.optim.Adam."""
    from tiny_diffusion_amd.latent_diffusion import ForwardProcess
    from tiny_diffusion_amd.train import TrainStep

    fp = ForwardProcess()
    v = build_vae(0)
    m, ref = build(3), build(3)
    m.train(); ref.train()
    ts = TrainStep(m, fp, lr=1e-3)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(8)
    x = (torch.rand(16, 1, 28, 28, generator=g) * 2 - 1).cuda()
    mu, logvar = v.encode(x.view(-1, 784))
    z0 = v.reparameterize(mu, logvar, eps=torch.randn(16, 20, generator=g).cuda())
    noise = torch.randn(16, 20, generator=g).cuda()
    t = torch.randint(0, 1000, (16,), generator=g).cuda()
    y = torch.randint(0, 10, (16,), generator=g).cuda()
    loss = ts.step(z0, y, t=t, noise=noise)
    z_t, _ = fp.q_sample("cuda", z0, t, noise=noise)
    l2 = F.mse_loss(ref(z_t, t, y), noise)
    opt.zero_grad(); l2.backward(); opt.step()
    assert abs(float(loss) - l2.item()) <= 2e-6 * abs(l2.item())
    for (k, a), (_, b) in zip(m.named_parameters(), ref.named_parameters()):
        if is_zero_grad(k):
            continue
        diff = (a - b).abs()
        assert diff.max().item() <= 2.1e-3, k
        assert (diff > 1e-5).float().mean().item() <= 5e-3, (k, (diff > 1e-5).float().mean().item())
