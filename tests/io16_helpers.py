"""References, bounds, builders and a host model of the dispatch for the bf16-storage (`io16`) instantiations of
csrc/bn.hip, csrc/spatial.hip and csrc/edge_conv.hip and for the kernels that emit BatchNorm-backward partial sums
(DESIGN.md 3.23).  Built on tests/spatial_helpers.py (S) and tests/conv_helpers.py (CH): the fp64 references and the
fp32 bounds are THEIRS, evaluated on the operands the kernel reads - bf16 values widened exactly, fp32 parameters.  Plain
module, no fixtures: tests/test_io16_refs_host.py checks it on the CPU, tests/test_gpu_io16_dispatch.py holds the
kernels against it.

fp32 outputs (dgamma, dbeta, dbias, partial sums, pixel sums, thin tensors, dw / db) keep the per-element bound of their
fp32 tests, 9 u sqrt(K) x magnitude-sum with K counted on the kernel.  A bf16 output with fp64 reference `ref` and
fp32 bound `b` must lie in [RNE_bf16(ref - b), RNE_bf16(ref + b)]: rounding is monotone, so a correctly rounded fp32
result always passes, and where both ends round to the same bf16 value the comparison is bit for bit.  No new constant."""
import math

import torch

import conv_helpers as CH
import spatial_helpers as S
from oracle import ref_cpu as R

U, LAM = S.U, S.LAM
TDX_E_BADARG, TDX_E_SHAPE = -1, -2
UNDECIDED_CAP_TRAIN_G = 0.20    # share of elements whose interval spans more than one bf16 value: train-mode BN g'
UNDECIDED_CAP = 0.05            # every other bf16 output

# constants of the sources that decide a branch (test_io16_refs_host.py pins each against the source text)
APPLY16_CAP = 8192              # bn_relu_apply16_kernel: workgroups of 256 threads, eight channels per thread
PRODUCER_CAP = 2048             # TDX_BNBWD_MAX_PRODUCER_BLOCKS: the two sum-emitting producers
PLAIN_CAP = S.EW_GRID_CAP       # 4096: the plain max-pool / resize kernels
BNBWD_FUSED_DEFAULT = 6         # knob bnbwd_fused: bit 1 (2) the resize adjoint, bit 2 (4) the max-pool backward
KNOB_RESIZE, KNOB_POOL = 2, 4


# ------------------------------------------------------------------------------------------------ bf16 arithmetic
def to16(t):
    """fp32 -> bf16 storage, round to nearest even (what st4 / st1 of csrc/io16.h do)."""
    return t.to(torch.bfloat16)


def r16(t):
    """fp32 values rounded to bf16 and widened again: a bf16-representable fp32 tensor."""
    return t.to(torch.bfloat16).float()


def trunc16(t):
    """fp32 -> bf16 by TRUNCATION of the low 16 bits (the defect the interval must catch), widened again."""
    bits = t.contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32)


def is16(t):
    return bool(torch.equal(r16(t), t))


def rne16_64(x):
    """fp64 -> nearest bf16 value (ties to even), returned in fp64: rounded ONCE from the fp64 value, not through fp32.
    bf16 has 8 significant bits: the quantum of x in [2^(e-1), 2^e) is 2^(e-8), 2^-133 below the normal range."""
    m, e = torch.frexp(x)
    q = torch.exp2((e.clamp_min(-125) - 8).double())
    return torch.round(x / q) * q


def interval16(ref, bound):
    lo, hi = rne16_64(ref - bound), rne16_64(ref + bound)
    return lo, hi


def undecided_share(ref, bound):
    lo, hi = interval16(ref, bound)
    return float((lo != hi).double().mean())


def outside16(got, ref, bound):
    """Number of elements of the bf16 (or widened) tensor `got` outside [RNE(ref - b), RNE(ref + b)]; NaN is outside."""
    lo, hi = interval16(ref, bound)
    g = got.double()
    return int((~((g >= lo) & (g <= hi))).sum())


def ratio16(got, ref, bound):
    """For the printed figure only: max |got - ref| / (b + half a bf16 spacing at ref)."""
    m, e = torch.frexp(ref)
    half = torch.exp2((e.clamp_min(-125) - 9).double())
    r = (got.double() - ref).abs() / (bound + half)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ BatchNorm
def bn_operands16(rows, C, seed, device, big_mean=False):
    """S.bn_operands with y and g bf16-representable and the ReLU decidable AFTER the rounding (S.nudge_relu(bf16))."""
    d = S.bn_operands(rows, C, seed, device, big_mean)
    d["y"] = S.nudge_relu(d["y"], d["scale"], d["shift"], bf16=True)
    d["g"] = r16(d["g"])
    assert is16(d["y"]) and is16(d["g"]) and S.relu_decidable(d["y"], d["scale"], d["shift"])
    return d


def bn_apply_ref16(y, scale, shift):
    """S.bn_relu_fwd_ref with the bound set to 0 where the ReLU is closed: it is decidable (asserted by the builder), so
    the kernel's fma has the sign of the exact pre-activation and stores exactly 0 there."""
    ref, b = S.bn_relu_fwd_ref(y, scale, shift)
    return ref, torch.where(ref > 0, b, torch.zeros_like(b))


def host_partials(d, nblk, seed):
    """A caller-made partial [nblk][2][C] in fp32: the exact per-channel sums of (g, y) spread over nblk blocks with
    random shares 1 / nblk (1 + randn / 2).  What it sums to is whatever its fp32 entries sum to: the reference reads
    THEM (bn_from_partials_ref), so nothing a kernel wrote feeds a reference."""
    g, y = d["g"].double(), d["y"].double()
    pre = y * d["scale"].double() + d["shift"].double()
    gz = torch.where(pre > 0, g, torch.zeros_like(g))
    xh = (y - d["mean"].double()) * d["rstd"].double()
    tot = torch.stack([gz.sum(0), (gz * xh).sum(0)])                       # (2, C)
    gen = torch.Generator(device=g.device).manual_seed(seed)
    share = (1 + 0.5 * torch.randn(nblk, 2, g.shape[1], device=g.device, generator=gen).double()) / nblk
    return (share * tot).float().contiguous()


def bn_from_partials_ref(g, y, partial, scale, shift, mean, rstd, gamma, training):
    """tdx_bn_relu_bwd_from_partials in fp64 from its operands -> {name: (reference, bound)}.  The kernel adds the
    blocks in double (no fp32 rounding) and casts: dbeta, dgamma carry 1 rounding against sum |partial|.  g' in train
    mode carries the nine roundings of the apply pass (gamma rstd, the two casts of the means, xhat two, xhat m2, two
    differences, the product: S.bn_relu_bwd_ref's K + 13 less the K + 4 of sums that here are exact), eval one; dbias
    in eval mode is one product in double and a cast: 1."""
    g, y, p = g.double(), y.double(), partial.double()
    N = g.shape[0]
    s1, s2 = p[:, 0].sum(0), p[:, 1].sum(0)
    a1, a2 = p[:, 0].abs().sum(0), p[:, 1].abs().sum(0)
    pre = y * scale.double() + shift.double()
    gz = torch.where(pre > 0, g, torch.zeros_like(g))
    xh = (y - mean.double()) * rstd.double()
    out = {"dbeta": (s1, LAM * U * a1), "dgamma": (s2, LAM * U * a2)}
    if training:
        k1 = gamma.double() * rstd.double()
        out["g"] = (k1 * (gz - s1 / N - xh * s2 / N),
                    LAM * U * math.sqrt(9) * k1.abs() * (gz.abs() + a1 / N + xh.abs() * a2 / N))
        out["dbias"] = (torch.zeros_like(s1), torch.zeros_like(s1))
    else:
        out["g"] = (gz * scale.double(), LAM * U * (gz * scale.double()).abs())
        out["dbias"] = (s1 * scale.double(), LAM * U * a1 * scale.double().abs())
    return out


# ------------------------------------------------------------------------------------------------ producers
def partial_sums_ref(g_ref, b_g, y, scale, shift, mean, rstd, K):
    """The two per-channel sums a producer emits for the gradient it writes, in fp64: sum gz and sum gz xhat over every
    element, gz = g_ref where relu(y scale + shift) is open, xhat = (y - mean) rstd -> {name: (reference, bound)}.
    K: fp32 additions behind one channel's sum in one workgroup (elements one thread accumulates + rgroups); the
    second sum has 3 more roundings (xhat two, the product).  b_g: the per-element bound of the fp32 gradient the sums
    are formed from (before it is rounded for the store); it is carried in as sum b_g and sum b_g |xhat|."""
    C = y.shape[-1]
    g, yy = g_ref.reshape(-1, C), y.double().reshape(-1, C)
    bg = b_g.reshape(-1, C) if torch.is_tensor(b_g) else torch.zeros_like(g)
    pre = yy * scale.double() + shift.double()
    opn = pre > 0
    gz = torch.where(opn, g, torch.zeros_like(g))
    bz = torch.where(opn, bg, torch.zeros_like(g))
    xh = (yy - mean.double()) * rstd.double()
    return {"s1": (gz.sum(0), LAM * U * math.sqrt(K) * gz.abs().sum(0) + bz.sum(0)),
            "s2": ((gz * xh).sum(0), LAM * U * math.sqrt(K + 3) * (gz * xh).abs().sum(0) + (bz * xh.abs()).sum(0))}


def partial_totals(partial, nblk):
    """Sum over the blocks of a producer's partial [nblk][2][C], added in fp64 -> (s1, s2) per channel."""
    p = partial[:nblk].double()
    return p[:, 0].sum(0), p[:, 1].sum(0)


def width_ok(C):
    return S.bn_bwd_width_ok(C)


def pool_producer_plan(B, H, W, C, knob=BNBWD_FUSED_DEFAULT, scale_given=True, partial_given=True):
    """Host model of tdx_maxpool2_ceil_bwd_bn: which kernel runs, its grid, the trips of its grid-stride loop, and K of
    the emitted sums (a thread adds up to 4 positions of one window per trip, a workgroup adds its rgroups threads)."""
    n = B * ((H + 1) // 2) * ((W + 1) // 2) * (C // 4)
    why = None
    if not partial_given:
        why = "partial == NULL"
    elif not knob & KNOB_POOL:
        why = "knob bit 2 off"
    elif not scale_given:
        why = "scale == NULL"
    elif not width_ok(C):
        why = "width"
    cap = PLAIN_CAP if why else PRODUCER_CAP
    grid = max(1, min(-(-n // 256), cap))
    trips = -(-n // (grid * 256))
    plan = {"branch": "plain" if why else "producer", "why": why, "grid": grid, "trips": trips, "nblk": 0 if why else grid}
    if not why:
        plan["K"] = 4 * trips + 256 // (C // 4)
    return plan


def resize_producer_plan(B, Hi, Wi, Ho, Wo, C, knob=BNBWD_FUSED_DEFAULT, partial_given=True):
    """Host model of tdx_bilinear_ac_bwd_bn on top of S.adjoint_branch: "rejected", the plain adjoint (with the reason
    of the fall-back) or the producer form of the row kernel; rows a workgroup owns; K of the emitted sums (a thread adds
    ceil(Wi C / 4 / 256) elements per row)."""
    branch = S.adjoint_branch(Hi, Wi, Ho, Wo)
    if branch == "rejected":
        return {"branch": "rejected", "nblk": 0}
    why = None
    if not partial_given:
        why = "partial == NULL"
    elif not knob & KNOB_RESIZE:
        why = "knob bit 1 off"
    elif branch == "generic":
        why = "Hi or Wi > 64"
    elif not width_ok(C):
        why = "width"
    if why:
        return {"branch": "plain:" + branch, "why": why, "nblk": 0}
    rows = B * Hi
    grid = min(rows, PRODUCER_CAP)
    per_wg = -(-rows // grid)
    return {"branch": "producer:" + branch, "why": None, "grid": grid, "nblk": grid, "rows_per_wg": per_wg,
            "K": per_wg * -(-(Wi * (C // 4)) // 256) + 256 // (C // 4)}


def apply16_plan(rows, C):
    """tdx_bn_apply_relu_fwd_io with io16: refused unless C % 8 == 0; grid and trips of bn_relu_apply16_kernel."""
    if C % 8:
        return {"branch": "refused"}
    n8 = rows * C // 8
    grid = min(-(-n8 // 256), APPLY16_CAP)
    return {"branch": "apply16", "grid": grid, "trips": -(-n8 // (grid * 256))}


def bwd_apply_trips(rows, C):
    """Trips of bn_bwd_apply_kernel's stride loop (cap S.BN_BWD_APPLY_CAP workgroups of 256 quads)."""
    n4 = rows * C // 4
    return -(-n4 // (min(-(-n4 // 256), S.BN_BWD_APPLY_CAP) * 256))


def finalize_trips(nblk):
    """Trips of the 256-wide block loop of bn_bwd_finalize_kernel for its busiest thread."""
    return -(-nblk // 256)


# ------------------------------------------------------------------------------------------------ max-pool
def pool_inputs16(B, H, W, C, seed, device, bn):
    """S.maxpool_inputs, asserted exact in bf16 (dyadic, at most 5 significant bits: so is skip + g)."""
    y, sc, sh, go, skip = S.maxpool_inputs(B, H, W, C, seed, device, bn)
    assert is16(y) and is16(go) and is16(skip)
    return y, sc, sh, go, skip


def pool_bn_stats(C, seed, device):
    """bn_mean, bn_rstd of the unit whose sums the max-pool producer emits: any fp32 values (xhat then rounds)."""
    gen = torch.Generator(device=device).manual_seed(seed)
    return 0.1 * torch.randn(C, device=device, generator=gen), 0.5 + torch.rand(C, device=device, generator=gen)


# ------------------------------------------------------------------------------------------------ resize
def resize_inputs16(B, Hi, Wi, Ho, Wo, C, seed, device):
    """S.resize_inputs with y and g bf16-representable, the ReLU decidable after the rounding; plus the pre-BN output
    bn_y (B, Hi, Wi, C) and the statistics of the unit whose gradient the adjoint writes (the producer form)."""
    d = S.resize_inputs(B, Hi, Wi, Ho, Wo, C, seed, device)
    d["y"] = S.nudge_relu(d["y"], d["scale"], d["shift"], bf16=True)
    d["g"] = r16(d["g"])
    gen = torch.Generator(device=device).manual_seed(seed + 1)
    d["mean"] = 0.2 * torch.randn(C, device=device, generator=gen)
    d["rstd"] = 0.5 + torch.rand(C, device=device, generator=gen)
    return d


def resize_from(a, mag, K, Ho, Wo):
    """The align_corners resize (R.bilinear_ac: the kernel's fp32 coordinates) of the fp64 tensor `a`, channels last,
    and LAM u sqrt(K) x the same resize of its magnitude."""
    with torch.device(a.device):
        ref = S.nhwc(R.bilinear_ac(S.nchw(a), (Ho, Wo)))
        m = S.nhwc(R.bilinear_ac(S.nchw(mag), (Ho, Wo)))
    return ref, LAM * U * math.sqrt(K) * m


def defer_operands(B, H, W, C, splits, seed, device, with_bias=True):
    """A deferred split-K source: `splits` fp32 slabs (B, H, W, C) a slab of B H W C + 64 floats apart, bias, scale,
    shift; the ReLU of (bias + sum partial) scale + shift decidable: an offender's first slab is moved."""
    gen = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=gen)   # noqa: E731
    slab = B * H * W * C + 64
    buf = torch.full((splits * slab,), float("nan"), device=device)
    parts = [buf[s * slab:s * slab + B * H * W * C].view(B, H, W, C) for s in range(splits)]
    for p_ in parts:
        p_.copy_(rn(B, H, W, C))
    bias = 0.3 * rn(C) if with_bias else None
    scale = (0.5 + torch.rand(C, device=device, generator=gen)) * torch.where(rn(C) < 0, -1.0, 1.0)
    shift = 0.2 * rn(C)
    for _ in range(4):
        pre, thr, _ = defer_margin(parts, bias, scale, shift)
        bad = ~(pre.abs() > thr)
        if not bool(bad.any()):
            break
        step = 64.0 * thr / scale.double().abs() * torch.where(pre >= 0, 1.0, -1.0) * torch.sign(scale.double())
        parts[0].copy_(torch.where(bad, (parts[0].double() + step).float(), parts[0]))
    pre, thr, _ = defer_margin(parts, bias, scale, shift)
    assert bool((pre.abs() > thr).all())
    return {"buf": buf, "parts": parts, "slab": slab, "bias": bias, "scale": scale, "shift": shift}


def defer_margin(parts, bias, scale, shift):
    """fp64 pre-activation of a deferred source, the threshold below which its sign is not decided (splits additions
    and one fma, each within u of the magnitude-sum: 8 u (splits + 1) mag), and the magnitude-sum itself."""
    v = sum(p_.double() for p_ in parts)
    a = sum(p_.double().abs() for p_ in parts)
    if bias is not None:
        v, a = v + bias.double(), a + bias.double().abs()
    mag = a * scale.double().abs() + shift.double().abs()
    return v * scale.double() + shift.double(), 8.0 * U * (len(parts) + 1) * mag, mag


def pair_ref(a, defer, b, b_addend, Ho, Wo):
    """tdx_bilinear_pair_fwd_io in fp64 -> (reference, bound), channels [0, Ca) | [Ca, Ca + Cb).  Source A plain: K = 4
    (S.resize_fwd_ref); deferred: + splits additions (the bias leads the sum) + the fma.  Source B: K = 4 + 1 with an
    addend."""
    if defer is None:
        ra, ba = S.resize_fwd_ref(a, None, None, None, Ho, Wo)
    else:
        pre, _, mag = defer_margin(defer["parts"], defer["bias"], defer["scale"], defer["shift"])
        ra, ba = resize_from(torch.relu(pre), torch.where(pre > 0, mag, torch.zeros_like(mag)),
                             4 + len(defer["parts"]) + 1, Ho, Wo)
    if b is None:
        return ra, ba
    rb, bb = S.resize_fwd_ref(b, None, None, b_addend, Ho, Wo)
    return torch.cat([ra, rb], -1), torch.cat([ba, bb], -1)


# ------------------------------------------------------------------------------------------------ pixel sum
def pixel_sum_ref(g, C):
    """out[b][c] = sum over pixels of g (B, HW, C) in fp64 and its bound: a thread adds every rgroups-th pixel, the
    workgroup adds its rgroups threads: K = ceil(HW / rgroups) + rgroups."""
    rgroups = 256 // (C // 4)
    HW = g.shape[1]
    K = -(-HW // rgroups) + rgroups
    return g.double().sum(1), LAM * U * math.sqrt(K) * g.double().abs().sum(1)


def pixel_sum_hw(C):
    rgroups = 256 // (C // 4)
    return sorted({1, rgroups - 1, rgroups + 1, 784} - {0})


# ------------------------------------------------------------------------------------------------ boundary convolutions
def edge_operands16(B, H, W, ct, cf, seed, device="cuda"):
    """CH.EdgeOperands with the two fat tensors the kernels READ (g_fat, fat) bf16-representable."""
    e = CH.EdgeOperands(B, H, W, ct, cf, seed, device)
    e.g_fat, e.fat = r16(e.g_fat), r16(e.fat)
    return e


def edge_refs(e):
    """fp64 reference, magnitude-sum and K of every output of the five boundary-convolution entries (the gates of
    tests/test_gpu_conv_nonsquare.py: forwards K = 9 cin, input gradients 9 x the stored channels, dw / db B H W).
    Fat outputs are channels-last (the initial forward's over its cf real channels), thin ones NCHW."""
    x, g0 = e.x_nhwc, e.g_fat[..., :e.cf]
    gt = e.g_thin_nhwc
    n = e.B * e.H * e.W
    nchw = lambda t: t.permute(0, 3, 1, 2)   # noqa: E731
    return {
        "init_fwd": (CH.conv_ref64(x, e.w_init, e.b_init), CH.conv_ref64(x.abs(), e.w_init.abs(), e.b_init.abs()), 9 * e.ct),
        "init_dw": (CH.wgrad_ref64(x, g0), CH.wgrad_ref64(x.abs(), g0.abs()), n),
        "init_db": (g0.double().sum((0, 1, 2)), g0.double().abs().sum((0, 1, 2)), n),
        "init_gx": (nchw(CH.dgrad_ref64(g0, e.w_init)), nchw(CH.dgrad_ref64(g0.abs(), e.w_init.abs())), 9 * 64),
        "fin_fwd": (nchw(CH.conv_ref64(e.fat, e.w_fin, e.b_fin)),
                    nchw(CH.conv_ref64(e.fat.abs(), e.w_fin.abs(), e.b_fin.abs())), 9 * 64),
        "fin_gin": (CH.dgrad_ref64(gt, e.w_fin), CH.dgrad_ref64(gt.abs(), e.w_fin.abs()), 9 * e.ct),
        "fin_dw": (CH.wgrad_ref64(e.fat, gt), CH.wgrad_ref64(e.fat.abs(), gt.abs()), n),
        "fin_db": (gt.double().sum((0, 1, 2)), gt.double().abs().sum((0, 1, 2)), n),
    }


EDGE_REL = {"init_fwd": 2e-6, "init_dw": 3e-6, "init_db": 3e-6, "init_gx": 2e-6, "fin_fwd": 2e-6, "fin_gin": 3e-6,
            "fin_dw": 3e-6, "fin_db": 3e-6}      # the norm-wise gates of the fp32 tests, for the fp32 outputs
EDGE_FAT_OUT = ("init_fwd", "fin_gin")            # bf16 in io16 mode: the interval check


def edge_bound(mag, K):
    return CH.ELEM_DIRECT * U * math.sqrt(K) * mag


# ------------------------------------------------------------------------------------------------ the cases
# BatchNorm: (C, rows) at rows = rpb + 1 of the floor regime (two blocks, the second of one row), plus the shapes the
# undecided shares of the issue were measured on
BN_WIDTHS = (4, 64, 1024)


def bn_two_block_rows(C):
    return S.bn_bwd_plan(1, C)["rpb"] + 1


BN_SHARE_CASES = [(4, 513, False), (64, 4100, True), (64, 65, False), (1024, 9, False)]   # (C, rows, big_mean)
BN_APPLY_BIG = (8, 524289)             # rows C / 4 = 1 048 578 > 4096 x 256: the apply pass's second trip
APPLY16_CASES = [(1, 8), (3, 8), (5, 1024)]
APPLY16_BIG = (2097160, 8)             # rows C / 8 = 2 097 160 > 8192 x 256
FROM_PARTIALS_NBLK = (1, 255, 256, 257, 2048)
FROM_PARTIALS_SHAPE = (37, 64)         # rows, C
POOL_SHAPES = [(1, 1), (1, 5), (5, 1), (5, 4), (7, 7), (13, 32)]
POOL_PRODUCER_WIDTHS = (4, 64, 1024)
POOL_PRODUCER_BIG = (262100, 3, 3, 4)  # B Ho Wo C / 4 = 1 048 400 = 2 x 2048 x 256 - 176: nearly every thread takes two trips
RESIZE_FWD_PAIRS = [(4, 7, 8, 8), (32, 16, 28, 28), (5, 8, 1, 1)]
RESIZE_BWD_CASES = {(4, 7, 8, 8): "rows-batched", (3, 2, 7, 6): "rows-batched", (2, 3, 7, 8): "rows-loop",
                    (65, 3, 66, 6): "generic"}
RESIZE_PRODUCER_SHAPES = [(4, 7, 8, 8), (2, 3, 7, 8)]     # rows-batched, rows-loop
RESIZE_PRODUCER_MANY_ROWS = (1500, 2, 3, 4, 5, 4)          # B, Hi, Wi, Ho, Wo, C: B Hi = 3000 > 2048
# (Ca, Cb, (Ha, Wa), (Hb, Wb), (Ho, Wo)): sources of different sizes
PAIR_CASES = [(64, 64, (4, 7), (8, 5), (8, 8)), (4, 128, (3, 2), (5, 6), (7, 6)), (64, 0, (5, 8), (1, 1), (7, 11))]   # (not 5 -> 9: outputs at exact midpoints of two bf16 values are ties)
PIXEL_WIDTHS = (4, 64, 1024)
PIXEL_REFUSED = (12, 6, 2048)
