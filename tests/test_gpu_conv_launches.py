"""Every 3x3 convolution launch of the benchmarked workloads, run as the plan runs it, against an fp64 reference of
the same operation.

The launch table is built from the library, not written by hand: the 13 conv/BN units of the MNIST UNet at 28x28 and
of the LAION UNet at 32x32 and 64x64 (shapes from the model's modules and the plan's own tensors), the training
algorithm of every role at the per-GPU batch bench.py times (tdx_conv3x3_train_algo) and the sampling algorithm at
n = 16 / 64 (tdx_conv3x3_infer_algo).  Each distinct launch runs through the public entry the plan uses, with the
plan's flags, and is gated three ways:

  (a) norm-wise: ||got - ref|| / ||ref|| within the bounds of tests/test_gpu_ops.py (direct 2e-6 / 3e-6 where that
      file has 3e-6, Winograd 1e-5);
  (b) per element: |got - ref| / (u sqrt(K) (|x| * |w|)), the error over that element's magnitude-sum (the same fp64
      reference on absolute values), u = 2^-24, K the length of the dot product - catches one wrong tile or one
      missing K-stage of one workgroup, which moves (a) very little on a 25 M-element tensor;
  (c) Winograd error budget: where a Winograd kernel runs, the direct kernel runs on the same operands too, and the
      Winograd norm-wise error may be at most K_WINO times the direct one.

Plus the launches the B = 256 table does not reach: the compact / XCD-grouped workgroup mapping boundary (63, 64 and
65 tile blocks, the last one ragged), a ragged 7x7 launch in the grouped mapping, and the weight gradient's chunk at its
1024-tile cap with a ragged last chunk."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
B_TRAIN = 256                 # per-GPU batch of the benchmarked training step (bench.py)
N_SAMPLE = (16, 64)           # sampling batches: the reverse process's default and bench.py's larger one
ROLES = ("fwd", "dgrad", "wgrad")

# (a) the existing norm-wise bounds (tests/test_gpu_ops.py): not loosened here
REL_DIRECT = {"fwd": 2e-6, "dgrad": 2e-6, "wgrad": 3e-6, "infer": 3e-6}
REL_WINO = 1e-5

# (b) per-element bound, in units of u sqrt(K) (|x| * |w|).  Probabilistic rounding-error analysis (Higham & Mary 2019):
# a K-term fp32 dot product is within lambda sqrt(K) u sum|x_i w_i| of the exact one except with probability
# ~2 K exp(-lambda^2 / 2) per element; over ~1e10 (element, rounding) pairs of this module lambda = 9 leaves that
# below 1e-7.  The Winograd kernels accumulate the same products in transformed form: the F(2x2, 3x3) transforms grow
# the magnitude-sum of a 1-D output by at most 8/3 for operands of equal size ((8/3)^2 ~ 7 -> 8 in 2-D), and the sums
# they round are shorter (cin terms instead of 9 cin for forward / input gradient, tiles instead of pixels for the
# weight gradient: sqrt(K) is 2-3x too large for them), so lambda x 8 / 2 = 36, plus a third for the transforms' own
# (not accumulated) roundings: 48.
ELEM_DIRECT = 9.0
ELEM_WINO = 48.0

# (c) Winograd / direct norm-wise error.  In the independent-rounding model a sum's error grows with the square root of
# the roundings each product carries and linearly with the operands' RMS: a Winograd product carries two extra
# rounded additions per operand (B^T d B; G g G^T or A e A^T, whose halvings are exact) and two in the output transform,
# 1 + 6 = 7 roundings against 1 (sqrt 7 = 2.6), on operands whose RMS the transforms grow by at most 1.5 -> 4.
K_WINO = {"fwd": 4.0, "dgrad": 4.0, "wgrad": 4.0, "infer": 4.0}


@pytest.fixture(scope="module")
def tdx():
    import tiny_diffusion_amd._lib as L

    assert torch.cuda.is_available()
    return L


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------- reference
def conv_ref64(x, w, bias=None):
    """fp64 3x3 / pad 1 convolution on the device as nine shifted GEMMs: x NHWC [B, H, W, cin], w [cout, cin, 3, 3]."""
    B, H, W, _ = x.shape
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    w = w.double()
    out = torch.zeros(B, H, W, w.shape[0], dtype=torch.float64, device=x.device)
    for kh in range(3):
        for kw in range(3):
            out += torch.matmul(xp[:, kh:kh + H, kw:kw + W, :], w[:, :, kh, kw].t())
    if bias is not None:
        out += bias.double()
    return out


def dgrad_ref64(dy, w):
    """dL/dx of conv_ref64 for dL/dy = dy (NHWC): the convolution with the flipped, transposed filter."""
    return conv_ref64(dy, w.flip(2, 3).transpose(0, 1))


def wgrad_ref64(x, dy):
    """dL/dw [cout, cin, 3, 3] of conv_ref64 for dL/dy = dy: nine GEMMs over the pixels."""
    B, H, W, cin = x.shape
    cout = dy.shape[-1]
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    g = dy.double().reshape(-1, cout).t()
    dw = torch.empty(cout, cin, 3, 3, dtype=torch.float64, device=x.device)
    for kh in range(3):
        for kw in range(3):
            dw[:, :, kh, kw] = g @ xp[:, kh:kh + H, kw:kw + W, :].reshape(-1, cin)
    return dw


def test_reference_helpers_against_cpu_conv2d():
    """The device fp64 helpers are the convolution, its input gradient and its weight gradient (CPU F.conv2d in fp64)."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 5, 7, 6, generator=g, dtype=torch.float64)
    w = torch.randn(4, 6, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(4, generator=g, dtype=torch.float64)
    dy = torch.randn(3, 5, 7, 4, generator=g, dtype=torch.float64)
    xc = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wc = w.clone().requires_grad_(True)
    y = F.conv2d(xc, wc, b, padding=1)
    y.backward(dy.permute(0, 3, 1, 2))
    d = torch.device("cuda")
    got = conv_ref64(x.to(d), w.to(d), b.to(d)).cpu()
    assert torch.allclose(got, y.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(dgrad_ref64(dy.to(d), w.to(d)).cpu(), xc.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(wgrad_ref64(x.to(d), dy.to(d)).cpu(), wc.grad, rtol=1e-12, atol=1e-12)


def rel_err(got, ref):
    got, ref = got.double(), ref.double()
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-300)).item()


def elem_ratio(got, ref, mag, K):
    """max over elements of |got - ref| / (u sqrt(K) mag); an element whose magnitude-sum is 0 must be exactly 0."""
    err = (got.double() - ref).abs()
    den = U * math.sqrt(K) * mag
    zero = den == 0
    if bool((err[zero] > 0).any()):
        return float("inf")
    return (err[~zero] / den[~zero]).max().item()


# ---------------------------------------------------------------------------------------------------------- the table
def model_units(kind, hw):
    """(cin as stored, cin of the reference weight, cout, H) of the 13 conv/BN units of one network, from the model's
    modules (channels) and the plan's own tensors (map sizes; the stored width of the first unit's input)."""
    from tiny_diffusion_amd import unet as UN

    if kind == UN.KIND_MNIST:
        from tiny_diffusion_amd.diffusion import NoiseModel
        model = NoiseModel()
    else:
        from tiny_diffusion_amd.conditional_diffusion_laion import NoiseModel
        model = NoiseModel()
    arch = model._arch
    plan = UN._Plan(1, 0, torch.device("cuda"), kind, 0 if hw == arch.in_shape[1] else hw)
    out = []
    for i, (stage, idx) in enumerate(UN._UNIT_PREFIX):
        conv = getattr(model, stage)[idx]
        assert isinstance(conv, torch.nn.Conv2d) and conv.kernel_size == (3, 3) and conv.padding == (1, 1)
        cin, cout = conv.in_channels, conv.out_channels
        H = math.isqrt(plan.tensor(f"Y{i}").numel() // cout)
        assert H * H * cout == plan.tensor(f"Y{i}").numel()
        stored = cin
        if i == 0:   # the first unit reads x0 (initial_conv's output), stored at the plan's width
            stored = plan.tensor("x0").numel() // (H * H)
        out.append((stored, cin, cout, H))
    del plan
    assert len(out) == 13
    return out


def launch_table(lib):
    """Distinct launches [(B, H, cin, cin_real, cout, role, algo, models)] of the benchmarked workloads."""
    from tiny_diffusion_amd import unet as UN

    nets = [("mnist28", UN.KIND_MNIST, 28, True), ("laion32", UN.KIND_LAION, 32, True), ("laion64", UN.KIND_LAION, 64, False)]
    table = {}
    for name, kind, hw, sampled in nets:
        units = model_units(kind, hw)
        for cin, cin_real, cout, H in units:
            for r, role in enumerate(ROLES):
                algo = "wino" if lib.tdx_conv3x3_train_algo(B_TRAIN, H, H, cin, cout, r) else "direct"
                table.setdefault((B_TRAIN, H, cin, cin_real, cout, role, algo), []).append(name)
            if sampled:
                for n in N_SAMPLE:
                    algo = "wino" if lib.tdx_conv3x3_infer_algo(n, H, H, cin, cout) else "direct"
                    table.setdefault((n, H, cin, cin_real, cout, "infer", algo), []).append(f"{name}/n{n}")
    return [k + (v,) for k, v in table.items()]


def tile_blocks(B, H):
    return -(-B * ((H + 1) // 2) ** 2 // 64)


def test_launch_table_covers_the_kernels(tdx):
    """The table reaches every kernel family and the XCD-grouped Winograd mapping with a padded grid."""
    table = launch_table(tdx.lib)
    kinds = {(e[5], e[6]) for e in table}
    for need in (("fwd", "wino"), ("dgrad", "wino"), ("wgrad", "wino"), ("infer", "wino"), ("infer", "direct")):
        assert need in kinds, need
    assert any(e[6] == "direct" and e[5] != "infer" for e in table)
    grouped = [e for e in table if e[6] == "wino" and e[5] in ("fwd", "dgrad") and tile_blocks(e[0], e[1]) >= 64]
    assert any(tile_blocks(e[0], e[1]) % 8 for e in grouped), "no grouped launch pads its grid"


# ---------------------------------------------------------------------------------------------------------- launches
class Operands:
    """Random operands of one (B, H, cin, cout) on the device; input channels >= cin_real are zero (the padded x0)."""

    def __init__(self, B, H, cin, cin_real, cout, seed):
        d = torch.device("cuda")
        g = torch.Generator(device=d).manual_seed(seed)
        self.B, self.H, self.cin, self.cout = B, H, cin, cout
        self.x = torch.randn(B, H, H, cin, generator=g, device=d)
        self.w = torch.randn(cout, cin, 3, 3, generator=g, device=d) * (2.0 / (9 * cin_real)) ** 0.5
        if cin_real < cin:
            self.x[..., cin_real:] = 0
            self.w[:, cin_real:] = 0
        self.b = torch.randn(cout, generator=g, device=d) * 0.1
        self.dy = torch.randn(B, H, H, cout, generator=g, device=d)
        self.osc = torch.randn(cout, generator=g, device=d)
        self.osh = torch.randn(cout, generator=g, device=d) * 0.3
        self._packs = {}

    def pack(self, tdx, which):
        if not self._packs:
            c = self.cout * 9 * self.cin
            wf, wg = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
            tdx.check(tdx.lib.tdx_pack_conv3x3(p(self.w), p(wf), p(wg), self.cout, self.cin, stream()))
            uf, ug = (torch.full((self.cout * self.cin * 16,), float("nan"), device="cuda") for _ in range(2))
            tdx.check(tdx.lib.tdx_pack_conv3x3_wino(p(self.w), p(uf), p(ug), self.cout, self.cin, stream()))
            self._packs = dict(wf=wf, wg=wg, uf=uf, ug=ug)
        return self._packs[which]


def run_fwd(tdx, o, algo):
    """Training forward with the BatchNorm statistics epilogue; returns (y, merged per-channel mean, biased var)."""
    lib, B, H, cin, cout = tdx.lib, o.B, o.H, o.cin, o.cout
    out = torch.full((B, H, H, cout), float("nan"), device="cuda")
    if algo == "wino":
        tiles, rows = lib.tdx_conv3x3_wino_stat_tiles(B, H, H), lib.tdx_conv3x3_wino_stat_tile_rows(B, H, H)
        stats = torch.full((tiles, 2, cout), float("nan"), device="cuda")
        tdx.check(lib.tdx_conv3x3_fwd_wino(p(o.x), p(o.pack(tdx, "uf")), p(o.b), p(out), B, H, H, cin, cout, 4, None, None,
                                           p(stats), stream()))
    else:
        tiles, rows = lib.tdx_conv3x3_stat_tiles(B, H, H, cin, cout), lib.tdx_conv3x3_stat_tile_rows(B, H, H, cin, cout)
        stats = torch.full((tiles, 2, cout), float("nan"), device="cuda")
        need = lib.tdx_conv3x3_train_scratch_floats(B, H, H, cin, cout)
        scratch = torch.full((max(need, 1),), float("nan"), device="cuda")
        tdx.check(lib.tdx_conv3x3_fwd_train(p(o.x), p(o.pack(tdx, "wf")), p(o.b), p(out), B, H, H, cin, cout, 4, p(stats),
                                            p(scratch), need, stream()))
    n = B * H * H
    assert (tiles - 1) * rows < n <= tiles * rows
    sd = stats.double()
    counts = torch.full((tiles,), float(rows), dtype=torch.float64, device="cuda")
    counts[-1] = n - (tiles - 1) * rows
    S, Q = sd[:, 0].sum(0), sd[:, 1].sum(0)
    mean = S / n
    var = (Q + (sd[:, 0] ** 2 / counts[:, None]).sum(0) - S * S / n) / n
    return out, mean, var


def run_dgrad(tdx, o, algo):
    lib, B, H, cin, cout = tdx.lib, o.B, o.H, o.cin, o.cout
    gin = torch.full((B, H, H, cin), float("nan"), device="cuda")
    if algo == "wino":   # the forward entry on the mirrored, channel-swapped pack
        tdx.check(lib.tdx_conv3x3_fwd_wino(p(o.dy), p(o.pack(tdx, "ug")), None, p(gin), B, H, H, cout, cin, 0, None, None,
                                           None, stream()))
    else:
        need = lib.tdx_conv3x3_train_scratch_floats(B, H, H, cout, cin)
        scratch = torch.full((max(need, 1),), float("nan"), device="cuda")
        tdx.check(lib.tdx_conv3x3_fwd_train(p(o.dy), p(o.pack(tdx, "wg")), None, p(gin), B, H, H, cout, cin, 0, None,
                                            p(scratch), need, stream()))
    return gin


def run_wgrad(tdx, o, algo):
    lib, B, H, cin, cout = tdx.lib, o.B, o.H, o.cin, o.cout
    if algo == "wino":
        splits = lib.tdx_conv3x3_wgrad_wino_splits(B, H, H, cin, cout)
        slabs = torch.full((splits, cout, 9, cin), float("nan"), device="cuda")
        tdx.check(lib.tdx_conv3x3_wgrad_wino(p(o.x), p(o.dy), p(slabs), B, H, H, cin, cout, stream()))
    else:
        splits = lib.tdx_conv3x3_wgrad_splits(B, H, H, cin, cout)
        slabs = torch.full((splits, cout, 9, cin), float("nan"), device="cuda")
        tdx.check(lib.tdx_conv3x3_wgrad(p(o.x), p(o.dy), p(slabs), B, H, H, cin, cout, 0, None, None, stream()))
    dw = torch.full((cout, cin, 3, 3), float("nan"), device="cuda")
    tdx.check(lib.tdx_conv3x3_wgrad_reduce(p(slabs), p(dw), splits, cout, cin, stream()))
    return dw


def run_infer(tdx, o, algo, ample):
    """Sampling forward, relu((conv + b) * osc + osh): K split as far as an ample scratch lets the plan go, or unsplit."""
    lib, B, H, cin, cout = tdx.lib, o.B, o.H, o.cin, o.cout
    out = torch.full((B, H, H, cout), float("nan"), device="cuda")
    if algo == "wino":
        scratch = torch.full(((cin // 8) * B * H * H * cout,), float("nan"), device="cuda") if ample else None
        tdx.check(lib.tdx_conv3x3_fwd_wino_infer(p(o.x), p(o.pack(tdx, "uf")), p(o.b), p(out), B, H, H, cin, cout, p(o.osc),
                                                 p(o.osh), p(scratch), 0 if scratch is None else scratch.numel(), stream()))
    elif ample:
        need = lib.tdx_conv3x3_splitk_scratch_floats(B, H, H, cin, cout)
        scratch = torch.full((max(need, 1),), float("nan"), device="cuda")
        tdx.check(lib.tdx_conv3x3_fwd_splitk(p(o.x), p(o.pack(tdx, "wf")), p(o.b), p(out), B, H, H, cin, cout, 2, None, None,
                                             p(o.osc), p(o.osh), p(scratch), need, stream()))
    else:
        tdx.check(lib.tdx_conv3x3_fwd(p(o.x), p(o.pack(tdx, "wf")), p(o.b), p(out), B, H, H, cin, cout, 2, None, None,
                                      p(o.osc), p(o.osh), None, stream()))
    return out


def check_launch(tdx, B, H, cin, cin_real, cout, role, algo, seed=0):
    """Runs one launch (and, for a Winograd launch, the direct kernel on the same operands); returns (row, failures)."""
    o = Operands(B, H, cin, cin_real, cout, seed)
    fails = []
    if role in ("fwd", "infer"):
        ref = conv_ref64(o.x, o.w, o.b)
        mag = conv_ref64(o.x.abs(), o.w.abs(), o.b.abs())
        K = 9 * cin
    elif role == "dgrad":
        ref, mag, K = dgrad_ref64(o.dy, o.w), dgrad_ref64(o.dy.abs(), o.w.abs()), 9 * cout
    else:
        ref, mag, K = wgrad_ref64(o.x, o.dy), wgrad_ref64(o.x.abs(), o.dy.abs()), B * H * H
    if role == "infer":   # relu is 1-Lipschitz: the bound of the affine map's output holds after it
        sc, sh = o.osc.double(), o.osh.double()
        ref = torch.relu(ref * sc + sh)
        mag = mag * sc.abs() + sh.abs()

    def run(a):
        if role == "fwd":
            y, mean, var = run_fwd(tdx, o, a)
            flat = ref.reshape(-1, cout)
            if not torch.allclose(mean, flat.mean(0), rtol=1e-4, atol=1e-5):
                fails.append(f"{a} batch mean")
            if not torch.allclose(var, flat.var(0, unbiased=False), rtol=1e-4, atol=1e-6):
                fails.append(f"{a} batch variance")
            return y
        if role == "dgrad":
            return run_dgrad(tdx, o, a)
        if role == "wgrad":
            d1 = run_wgrad(tdx, o, a)
            if not torch.equal(d1, run_wgrad(tdx, o, a)):
                fails.append(f"{a} wgrad not reproducible")
            return d1
        y1, y2 = run_infer(tdx, o, a, True), run_infer(tdx, o, a, True)
        if not torch.equal(y1, y2):
            fails.append(f"{a} split inference not bitwise reproducible")
        y0 = run_infer(tdx, o, a, False)
        e0 = rel_err(y0, ref)
        if not e0 < (REL_WINO if a == "wino" else REL_DIRECT["infer"]):
            fails.append(f"{a} unsplit inference rel err {e0:.2e}")
        return y1

    got = run(algo)
    torch.cuda.synchronize()
    e = rel_err(got, ref)
    r = elem_ratio(got, ref, mag, K)
    rel_gate = REL_WINO if algo == "wino" else REL_DIRECT[role]
    elem_gate = ELEM_WINO if algo == "wino" else ELEM_DIRECT
    if not e < rel_gate:
        fails.append(f"rel err {e:.2e} >= {rel_gate:.0e}")
    if not r <= elem_gate:
        fails.append(f"per-element ratio {r:.3g} > {elem_gate:g}")
    wd = None
    if algo == "wino":
        gd = run("direct")
        ed = rel_err(gd, ref)
        rd = elem_ratio(gd, ref, mag, K)
        wd = e / max(ed, 1e-300)
        if not ed < REL_DIRECT[role]:
            fails.append(f"direct twin rel err {ed:.2e}")
        if not rd <= ELEM_DIRECT:
            fails.append(f"direct twin per-element ratio {rd:.3g}")
        if not wd <= K_WINO[role]:
            fails.append(f"winograd / direct {wd:.2f} > K_WINO {K_WINO[role]:g}")
    row = (f"{B:4d} {H:3d} {cin:5d} {cout:5d} {role:6s} {algo:6s} blocks {tile_blocks(B, H):5d}  rel {e:.2e}  "
           f"elem {r:6.3f}  wino/direct {'-' if wd is None else f'{wd:.2f}':>5s}")
    return row, fails


def run_table(tdx, entries):
    failures = []
    print(f"\n{'B':>4s} {'H':>3s} {'cin':>5s} {'cout':>5s} role   algo")
    for i, (B, H, cin, cin_real, cout, role, algo, tag) in enumerate(entries):
        row, fails = check_launch(tdx, B, H, cin, cin_real, cout, role, algo, seed=i)
        print(f"{row}  {tag}{'  FAIL ' + '; '.join(fails) if fails else ''}", flush=True)
        failures += [(B, H, cin, cout, role, algo, f) for f in fails]
    return failures


def test_every_launch_of_the_benchmarked_workloads(tdx):
    """Every distinct 3x3 convolution launch of the B = 256 training step (MNIST, LAION 32x32 and 64x64) and of the
    n = 16 / 64 reverse step (MNIST, LAION 32x32), as the plan runs it, against fp64."""
    table = launch_table(tdx.lib)
    failures = run_table(tdx, [e[:7] + (",".join(e[7]),) for e in table])
    assert not failures, failures


def test_edge_launches(tdx):
    """The launches the B = 256 table does not reach: 63 / 64 / 65 tile blocks around the compact / XCD-grouped mapping
    boundary (65: ragged last block), a ragged 7x7 launch in the grouped mapping (66 blocks of four whole images, the
    last with one), and the Winograd weight gradient with its pixel chunk at the 1024-tile cap (wino_wgrad_target = 1:
    one split per channel tile wanted, so the cap decides; 2156 and 1120 tiles -> a ragged last chunk)."""
    lib = tdx.lib
    entries = []
    for B, H, cin, cout in ((252, 8, 64, 128), (256, 8, 128, 64), (257, 8, 64, 64), (261, 7, 64, 128)):
        assert lib.tdx_conv3x3_wino_ok(B, H, H, cin, cout) and lib.tdx_conv3x3_wino_ok(B, H, H, cout, cin)
        for role in ("fwd", "dgrad", "infer"):
            entries.append((B, H, cin, cin, cout, role, "wino", f"{tile_blocks(B, H)} tile blocks"))
    assert sorted({tile_blocks(e[0], e[1]) for e in entries}) == [63, 64, 65, 66]
    default_target = 512
    try:
        tdx.check(lib.tdx_tune_set(b"wino_wgrad_target", 1))
        for B, H, cin, cout in ((11, 28, 64, 128), (70, 7, 64, 64)):
            nt = B * ((H + 1) // 2) ** 2
            assert lib.tdx_conv3x3_wgrad_wino_splits(B, H, H, cin, cout) == -(-nt // 1024) and nt % 1024
            entries.append((B, H, cin, cin, cout, "wgrad", "wino", f"{nt} tiles in chunks of 1024"))
        failures = run_table(tdx, entries)
    finally:
        tdx.check(lib.tdx_tune_set(b"wino_wgrad_target", default_target))
    assert lib.tdx_conv3x3_wgrad_wino_splits(256, 28, 28, 64, 128) == 251   # the default plan is back
    assert not failures, failures
