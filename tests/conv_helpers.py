"""Shared pieces of the kernel-level 3x3 convolution tests: the fp64 references (convolution, input gradient, weight
gradient - plain torch, on whatever device their operands live), the error measures, the gates, guarded output buffers
and the launch wrappers of the fp32 entries, all on (B, H, W) maps with H and W independent.

Used by tests/test_gpu_conv_launches.py (square maps: every launch of the benchmarked workloads), by
tests/test_gpu_conv_nonsquare.py (H != W) and by tests/test_conv_refs_host.py (the references themselves, no GPU)."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24

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

TDX_E_SHAPE = -2
GUARD = 64   # elements behind every guarded buffer

# The (B, H, W) maps of tests/test_gpu_conv_nonsquare.py, per kernel family (why each: that module's docstring);
# tests/test_conv_refs_host.py shows that an H / W exchange moves the reference of every one of them.
WINO_SHAPES = [(3, 6, 10), (9, 6, 10), (5, 8, 7), (5, 7, 8), (9, 3, 7), (5, 1, 16)]
WINO_REFUSED = [(2, 14, 7), (2, 5, 6)]
DIRECT_SHAPES = [(3, 6, 10), (5, 8, 7), (5, 7, 8), (2, 5, 12), (7, 4, 3)]
DIRECT_WIDE = (2, 4, 6)            # 256 -> 256 and 512 -> 512: the weight-gradient tiles 64 -> 128 does not reach
DIRECT_WGRAD_NARROW = [(6, 4, 2), (9, 8, 1), (7, 2, 5), (5, 1, 16)]   # 32 / W rows >= 3 H, or H < 4: the row carry
BF16_SHAPES = [(8, 4, 8), (4, 8, 7), (4, 7, 8), (1, 8, 96), (1, 96, 8)]
BF16_BN_SHAPE = (4, 6, 10)
EDGE_SMALL = [(3, 6, 5), (2, 9, 4), (2, 4, 9), (5, 7, 8)]
EDGE_LARGE = [(33, 40, 50), (66, 40, 50), (263, 40, 50)]
EDGE_PAIRS = [(1, 64), (4, 32)]    # (thin channels, real fat channels): MNIST | LAION latents


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------- reference
def conv_ref64(x, w, bias=None):
    """fp64 3x3 / pad 1 convolution as nine shifted GEMMs: x NHWC [B, H, W, cin], w [cout, cin, 3, 3]."""
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


def exchanged(fn, *nhwc):
    """fn on the same buffers read as (B, W, H, C) maps - what a kernel that exchanged H and W would compute - with a
    map-shaped result read back as (B, H, W, C)."""
    B, H, W, _ = nhwc[0].shape
    out = fn(*[t.contiguous().reshape(B, W, H, t.shape[-1]) for t in nhwc])
    return out.reshape(B, H, W, out.shape[-1]) if out.shape[:3] == (B, W, H) else out


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


def tile_blocks(B, H, W=None):
    """Winograd workgroups along the tiles: 64 tiles of 2x2 outputs each."""
    W = H if W is None else W
    return -(-B * ((H + 1) // 2) * ((W + 1) // 2) // 64)


# ---------------------------------------------------------------------------------------------------------- guards
class Guards:
    """NaN-filled output buffers with GUARD more NaN elements behind each; intact() after the launches."""

    def __init__(self):
        self.bufs = []

    def new(self, shape, dtype=torch.float32):
        n = math.prod(shape)
        buf = torch.full((n + GUARD,), float("nan"), dtype=dtype, device="cuda")
        self.bufs.append((buf, n))
        return buf[:n].view(shape)

    def intact(self):
        torch.cuda.synchronize()
        ok = all(bool(torch.isnan(buf[n:]).all()) for buf, n in self.bufs)
        self.bufs = []
        return ok


def new_out(guards, shape, dtype=torch.float32):
    if guards is not None:
        return guards.new(shape, dtype)
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device="cuda")


# ---------------------------------------------------------------------------------------------------------- launches
class Operands:
    """Random operands of one (B, H, W, cin, cout) on the device (W = H when not given); input channels >= cin_real are
    zero (the padded x0)."""

    def __init__(self, B, H, cin, cin_real, cout, seed, W=None, device="cuda", fenced=False):
        W = H if W is None else W
        d = torch.device(device)
        g = torch.Generator(device=d).manual_seed(seed)
        self.B, self.H, self.W, self.cin, self.cout = B, H, W, cin, cout
        self._fences = []
        self.x = torch.randn(B, H, W, cin, generator=g, device=d)
        self.w = torch.randn(cout, cin, 3, 3, generator=g, device=d) * (2.0 / (9 * cin_real)) ** 0.5
        if cin_real < cin:
            self.x[..., cin_real:] = 0
            self.w[:, cin_real:] = 0
        self.b = torch.randn(cout, generator=g, device=d) * 0.1
        self.dy = torch.randn(B, H, W, cout, generator=g, device=d)
        self.osc = torch.randn(cout, generator=g, device=d)
        self.osh = torch.randn(cout, generator=g, device=d) * 0.3
        self._packs = {}
        if fenced:   # the same values, with (W + 2) pixels of NaN in front of and behind each activation tensor
            self.x, self.dy = self._fence(self.x), self._fence(self.dy)

    def _fence(self, t):
        """t inside a NaN-filled buffer: a kernel that reads in front of or behind its input - and uses what it read,
        be it times zero - returns NaN."""
        pad = -(-(self.W + 2) * t.shape[-1] // 64) * 64   # whole 256-byte lines: the tensor keeps its alignment
        buf = torch.full((t.numel() + 2 * pad,), float("nan"), device=t.device)
        view = buf[pad:pad + t.numel()].view(t.shape)
        view.copy_(t)
        self._fences.append(buf)
        return view

    def pack(self, tdx, which):
        if not self._packs:
            c = self.cout * 9 * self.cin
            wf, wg = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
            tdx.check(tdx.lib.tdx_pack_conv3x3(p(self.w), p(wf), p(wg), self.cout, self.cin, stream()))
            uf, ug = (torch.full((self.cout * self.cin * 16,), float("nan"), device="cuda") for _ in range(2))
            tdx.check(tdx.lib.tdx_pack_conv3x3_wino(p(self.w), p(uf), p(ug), self.cout, self.cin, stream()))
            self._packs = dict(wf=wf, wg=wg, uf=uf, ug=ug)
        return self._packs[which]


class EdgeOperands:
    """Random operands of the two boundary convolutions on one (B, H, W) map: ct thin channels (the model's input /
    output, NCHW) and 64 stored fat channels (channels-last) of which cf are real for initial_conv."""

    def __init__(self, B, H, W, ct, cf, seed, device="cuda"):
        d = torch.device(device)
        g = torch.Generator(device=d).manual_seed(seed)
        self.B, self.H, self.W, self.ct, self.cf = B, H, W, ct, cf
        self.x = torch.randn(B, ct, H, W, generator=g, device=d)              # initial_conv's input
        self.w_init = torch.randn(cf, ct, 3, 3, generator=g, device=d) * 0.3
        self.b_init = torch.randn(cf, generator=g, device=d) * 0.1
        self.g_fat = torch.randn(B, H, W, 64, generator=g, device=d)          # gradient of initial_conv's stored output
        self.fat = torch.randn(B, H, W, 64, generator=g, device=d)            # final_conv's input
        self.w_fin = torch.randn(ct, 64, 3, 3, generator=g, device=d) * 0.05
        self.b_fin = torch.randn(ct, generator=g, device=d) * 0.1
        self.g_thin = torch.randn(B, ct, H, W, generator=g, device=d)         # gradient of final_conv's output

    @property
    def x_nhwc(self):
        return self.x.permute(0, 2, 3, 1).contiguous()

    @property
    def g_thin_nhwc(self):
        return self.g_thin.permute(0, 2, 3, 1).contiguous()


def merge_stats(stats, tiles, rows, n):
    """Per-channel mean and biased variance of n rows from [tiles][2][C] partials (sum, M2 about the tile mean) over
    tiles of `rows` rows, the last one ragged (Chan's merge, in fp64)."""
    assert (tiles - 1) * rows < n <= tiles * rows
    sd = stats.double()
    counts = torch.full((tiles,), float(rows), dtype=torch.float64, device=stats.device)
    counts[-1] = n - (tiles - 1) * rows
    S, Q = sd[:, 0].sum(0), sd[:, 1].sum(0)
    mean = S / n
    var = (Q + (sd[:, 0] ** 2 / counts[:, None]).sum(0) - S * S / n) / n
    return mean, var


def run_fwd(tdx, o, algo, guards=None):
    """Training forward with the BatchNorm statistics epilogue; returns (y, merged per-channel mean, biased var)."""
    lib, B, H, W, cin, cout = tdx.lib, o.B, o.H, o.W, o.cin, o.cout
    out = new_out(guards, (B, H, W, cout))
    if algo == "wino":
        tiles, rows = lib.tdx_conv3x3_wino_stat_tiles(B, H, W), lib.tdx_conv3x3_wino_stat_tile_rows(B, H, W)
        stats = new_out(guards, (tiles, 2, cout))
        tdx.check(lib.tdx_conv3x3_fwd_wino(p(o.x), p(o.pack(tdx, "uf")), p(o.b), p(out), B, H, W, cin, cout, 4, None, None,
                                           p(stats), stream()))
    else:
        tiles, rows = lib.tdx_conv3x3_stat_tiles(B, H, W, cin, cout), lib.tdx_conv3x3_stat_tile_rows(B, H, W, cin, cout)
        stats = new_out(guards, (tiles, 2, cout))
        need = lib.tdx_conv3x3_train_scratch_floats(B, H, W, cin, cout)
        scratch = torch.full((max(need, 1),), float("nan"), device="cuda")
        tdx.check(lib.tdx_conv3x3_fwd_train(p(o.x), p(o.pack(tdx, "wf")), p(o.b), p(out), B, H, W, cin, cout, 4, p(stats),
                                            p(scratch), need, stream()))
    mean, var = merge_stats(stats, tiles, rows, B * H * W)
    return out, mean, var


def run_dgrad(tdx, o, algo, guards=None):
    lib, B, H, W, cin, cout = tdx.lib, o.B, o.H, o.W, o.cin, o.cout
    gin = new_out(guards, (B, H, W, cin))
    if algo == "wino":   # the forward entry on the mirrored, channel-swapped pack
        tdx.check(lib.tdx_conv3x3_fwd_wino(p(o.dy), p(o.pack(tdx, "ug")), None, p(gin), B, H, W, cout, cin, 0, None, None,
                                           None, stream()))
    else:
        need = lib.tdx_conv3x3_train_scratch_floats(B, H, W, cout, cin)
        scratch = torch.full((max(need, 1),), float("nan"), device="cuda")
        tdx.check(lib.tdx_conv3x3_fwd_train(p(o.dy), p(o.pack(tdx, "wg")), None, p(gin), B, H, W, cout, cin, 0, None,
                                            p(scratch), need, stream()))
    return gin


def run_wgrad(tdx, o, algo, guards=None):
    lib, B, H, W, cin, cout = tdx.lib, o.B, o.H, o.W, o.cin, o.cout
    if algo == "wino":
        splits = lib.tdx_conv3x3_wgrad_wino_splits(B, H, W, cin, cout)
        slabs = new_out(guards, (splits, cout, 9, cin))
        tdx.check(lib.tdx_conv3x3_wgrad_wino(p(o.x), p(o.dy), p(slabs), B, H, W, cin, cout, stream()))
    else:
        splits = lib.tdx_conv3x3_wgrad_splits(B, H, W, cin, cout)
        slabs = new_out(guards, (splits, cout, 9, cin))
        tdx.check(lib.tdx_conv3x3_wgrad(p(o.x), p(o.dy), p(slabs), B, H, W, cin, cout, 0, None, None, stream()))
    dw = new_out(guards, (cout, cin, 3, 3))
    tdx.check(lib.tdx_conv3x3_wgrad_reduce(p(slabs), p(dw), splits, cout, cin, stream()))
    return dw


def run_infer(tdx, o, algo, ample, guards=None):
    """Sampling forward, relu((conv + b) * osc + osh): K split as far as an ample scratch lets the plan go, or unsplit."""
    lib, B, H, W, cin, cout = tdx.lib, o.B, o.H, o.W, o.cin, o.cout
    out = new_out(guards, (B, H, W, cout))
    if algo == "wino":
        scratch = torch.full(((cin // 8) * B * H * W * cout,), float("nan"), device="cuda") if ample else None
        tdx.check(lib.tdx_conv3x3_fwd_wino_infer(p(o.x), p(o.pack(tdx, "uf")), p(o.b), p(out), B, H, W, cin, cout, p(o.osc),
                                                 p(o.osh), p(scratch), 0 if scratch is None else scratch.numel(), stream()))
    elif ample:
        need = lib.tdx_conv3x3_splitk_scratch_floats(B, H, W, cin, cout)
        scratch = torch.full((max(need, 1),), float("nan"), device="cuda")
        tdx.check(lib.tdx_conv3x3_fwd_splitk(p(o.x), p(o.pack(tdx, "wf")), p(o.b), p(out), B, H, W, cin, cout, 2, None, None,
                                             p(o.osc), p(o.osh), p(scratch), need, stream()))
    else:
        tdx.check(lib.tdx_conv3x3_fwd(p(o.x), p(o.pack(tdx, "wf")), p(o.b), p(out), B, H, W, cin, cout, 2, None, None,
                                      p(o.osc), p(o.osh), None, stream()))
    return out


def role_reference(o, role):
    """(fp64 reference, magnitude-sum, K) of one role on the operands o."""
    if role in ("fwd", "infer"):
        ref = conv_ref64(o.x, o.w, o.b)
        mag = conv_ref64(o.x.abs(), o.w.abs(), o.b.abs())
        K = 9 * o.cin
    elif role == "dgrad":
        ref, mag, K = dgrad_ref64(o.dy, o.w), dgrad_ref64(o.dy.abs(), o.w.abs()), 9 * o.cout
    else:
        ref, mag, K = wgrad_ref64(o.x, o.dy), wgrad_ref64(o.x.abs(), o.dy.abs()), o.B * o.H * o.W
    if role == "infer":   # relu is 1-Lipschitz: the bound of the affine map's output holds after it
        sc, sh = o.osc.double(), o.osh.double()
        ref = torch.relu(ref * sc + sh)
        mag = mag * sc.abs() + sh.abs()
    return ref, mag, K


def check_launch(tdx, B, H, cin, cin_real, cout, role, algo, seed=0, W=None, guards=None, fenced=False):
    """Runs one launch (and, for a Winograd launch, the direct kernel on the same operands); returns (row, failures)."""
    o = Operands(B, H, cin, cin_real, cout, seed, W, fenced=fenced)
    fails = []
    ref, mag, K = role_reference(o, role)

    def run(a):
        if role == "fwd":
            y, mean, var = run_fwd(tdx, o, a, guards)
            flat = ref.reshape(-1, cout)
            if not torch.allclose(mean, flat.mean(0), rtol=1e-4, atol=1e-5):
                fails.append(f"{a} batch mean")
            if not torch.allclose(var, flat.var(0, unbiased=False), rtol=1e-4, atol=1e-6):
                fails.append(f"{a} batch variance")
            return y
        if role == "dgrad":
            return run_dgrad(tdx, o, a, guards)
        if role == "wgrad":
            d1 = run_wgrad(tdx, o, a, guards)
            if not torch.equal(d1, run_wgrad(tdx, o, a, guards)):
                fails.append(f"{a} wgrad not reproducible")
            return d1
        y1, y2 = run_infer(tdx, o, a, True, guards), run_infer(tdx, o, a, True, guards)
        if not torch.equal(y1, y2):
            fails.append(f"{a} split inference not bitwise reproducible")
        y0 = run_infer(tdx, o, a, False, guards)
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
    if guards is not None and not guards.intact():
        fails.append("guard region written")
    shape = f"{H:3d}" if W is None else f"{H:3d}x{W:<3d}"
    row = (f"{B:4d} {shape} {cin:5d} {cout:5d} {role:6s} {algo:6s} blocks {tile_blocks(B, H, W):5d}  rel {e:.2e}  "
           f"elem {r:6.3f}  wino/direct {'-' if wd is None else f'{wd:.2f}':>5s}")
    return row, fails
