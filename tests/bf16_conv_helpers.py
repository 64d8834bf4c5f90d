"""References, operands, gates, cases and a host model of the dispatch for the bf16 MFMA convolution kernels of
csrc/conv3x3_bf16.hip.  Built on tests/conv_helpers.py (CH: the fp64 references, elem_ratio,
ELEM_DIRECT, Guards) and tests/io16_helpers.py (H: rne16_64, interval16, outside16, undecided_share, UNDECIDED_CAP).
Plain module, no fixtures, no GPU: tests/test_bf16_conv_refs_host.py checks it on the CPU,
tests/test_gpu_bf16_conv_dispatch.py holds the kernels against it.

Every reference is fp64 on the operands the kernel reads: bf16 values widened exactly, the bf16-rounded weight, fp32
bias / scale / shift; the IN_BN operand is relu(fma(x, scale, shift)) in fp32 rounded once to bf16, padding 0 after it.

Two operand regimes per case:
  exact     small integers (scales +-{0.5, 1, 2}): every product and every partial sum in any order is a multiple of 1/4
            below 2^22, so fp32 accumulation is exact whatever the tiling, split or MFMA order.  fp32 outputs must
            torch.equal the fp64 reference, bf16 outputs must equal rne16_64(ref); no tolerance, no element left out.
            Only M2 is inexact (the tile mean is a quotient): LAM u sqrt(rows) x sum((v - mean)^2).
  rounding  relu(N(0,1)) activations, N(1,1) sqrt(2 / (9 cin)) weights: fp32 outputs within CH.ELEM_DIRECT u sqrt(K) x
            magnitude-sum, bf16 outputs inside [RNE(ref - b), RNE(ref + b)] with b that bound.  One-signed operands keep
            |ref| near the magnitude-sum, which is what keeps the share of undecided bf16 elements under H.UNDECIDED_CAP."""
import functools
import math

import torch

import conv_helpers as CH
import io16_helpers as H

U, LAM = H.U, H.LAM
REGIMES = ("exact", "rounding")
FLAG_IN_BN, FLAG_INFER, FLAG_STATS = 1, 2, 4
STAT_ROWS = 128                 # tdx_conv3x3_bf16_stat_tile_rows()

# constants of the sources that decide a branch (tests/test_bf16_conv_refs_host.py pins each against the source text)
THIN_WROWS = 448                # conv3x3_bf16_thin_kernel: rows of its LDS window
RING_ROWS = 256                 # M % 256 == 0: the ring and the thin kernel
RING_MAX_CIN = 1024
WGRAD9_MAX_W = 95               # nine-tap ring of <= 7 blocks
WGRAD9_MIN_SLOTS = 8            # (H + 1)(W + 1) >= 8: pos_of shifts a slot by 8 samples
KNOB_DEFAULTS = {"bf16_ring": 0, "bf16_thin": 3, "bf16_wgrad_swz": 1, "bf16_wgrad9": 1, "wgrad9_wgs": 0,
                 "wgrad_target": 2048, "wgrad_target_big": 1024}
EPIS = ("EPI_PLAIN", "EPI_STATS", "EPI_BNRELU")
FLAGS = (0, FLAG_STATS, FLAG_INFER)


# ------------------------------------------------------------------------------------------------ host model
def thin_window_fits(Hh, W):
    """thin_window_fits of the source: the largest slot window of any 256-pixel tile plus its halo -> (fits, rows)."""
    PW, HW = W + 1, Hh * W
    PP = (Hh + 1) * PW

    def slot_of(p):
        n, r = divmod(p, HW)
        oh, ow = divmod(r, W)
        return n * PP + oh * PW + ow

    worst = 0
    for j in range(HW):
        m0 = RING_ROWS * j
        worst = max(worst, slot_of(m0 + 255) - slot_of(m0) + 1 + 2 * (PW + 1))
        if (m0 + RING_ROWS) % HW == 0:
            break
    return worst <= THIN_WROWS, worst


def _b(x):
    return "true" if x else "false"


def fwd_kernel(shape, in_bn, flags, io16, knobs=None):
    """The instantiation tdx_conv3x3_fwd_bf16_io launches for (B, H, W, cin, cout) (channels as passed to the entry)."""
    B, Hh, W, cin, cout = shape
    k = dict(KNOB_DEFAULTS, **(knobs or {}))
    M = B * Hh * W
    epi = EPIS[2] if flags & FLAG_INFER else EPIS[1] if flags & FLAG_STATS else EPIS[0]
    thin = k["bf16_thin"]
    if (io16 and not in_bn and M % RING_ROWS == 0 and thin_window_fits(Hh, W)[0]
            and ((thin >= 1 and cout == 64) or (thin >= 2 and cin == 64) or thin >= 3)):
        return f"conv3x3_bf16_thin_kernel<{epi}>"
    if io16 and k["bf16_ring"] and M % RING_ROWS == 0 and cin <= RING_MAX_CIN:
        return f"conv3x3_bf16_ring_kernel<{128 if cout % 128 == 0 else 64}, {_b(in_bn)}, {epi}>"
    return f"conv3x3_bf16_kernel<128, {128 if cout % 128 == 0 else 64}, {_b(in_bn)}, {epi}, {_b(io16)}>"


def wgrad_plan(M, cin, cout, knobs=None):
    """pick_wgrad(M, cin, cout, bf16 = true) of csrc/conv3x3.hip -> (bm, bn, splits, chunk)."""
    k = dict(KNOB_DEFAULTS, **(knobs or {}))
    bm = 128 if cout % 128 == 0 else 64
    bn = 128 if cin % 128 == 0 else 64
    tiles = (cout // bm) * (cin // bn) * 9
    target = k["wgrad_target_big"] if (bm == 128 and bn == 128 and k["wgrad_target_big"] > 0) else k["wgrad_target"]
    s = (target + tiles - 1) // tiles
    if k["wgrad9_wgs"] > 0:
        s = k["wgrad9_wgs"] // ((cout // 64) * (cin // 64))
    s = max(1, min(s, (M + 255) // 256))
    chunk = (-(-M // s) + 31) // 32 * 32
    return bm, bn, -(-M // chunk), chunk


def wgrad9_geometry(W):
    """HALOB and NB of conv3x3_wgrad9_bf16_kernel: the block-aligned halo and the blocks one K-tile reads past its own."""
    PW = W + 1
    halob = (PW + 1 + 63) // 64 * 64
    return halob, (halob + 64 + PW) // 64


def wgrad_kernel(shape, in_bn, io16, knobs=None):
    B, Hh, W, cin, cout = shape
    k = dict(KNOB_DEFAULTS, **(knobs or {}))
    if io16 and k["bf16_wgrad9"] and W <= WGRAD9_MAX_W and (Hh + 1) * (W + 1) >= WGRAD9_MIN_SLOTS:
        return f"conv3x3_wgrad9_bf16_kernel<{_b(in_bn)}>"
    bm, bn, _, _ = wgrad_plan(B * Hh * W, cin, cout, knobs)
    if io16 and k["bf16_wgrad_swz"]:
        return f"conv3x3_wgrad_bf16s_kernel<{bm}, {bn}, {_b(in_bn)}>"
    return f"conv3x3_wgrad_bf16_kernel<{bm}, {bn}, {_b(in_bn)}, {_b(io16)}>"


def all_instantiations():
    """Every instantiation launch_bf16, launch_bf16_ring, launch_bf16_thin, launch_wgrad_bf16, launch_wgrad_bf16s and
    launch_wgrad9_bf16 can launch."""
    tf = ("false", "true")
    out = [f"conv3x3_bf16_kernel<128, {bn}, {i}, {e}, {io}>" for bn in (128, 64) for i in tf for e in EPIS for io in tf]
    out += [f"conv3x3_bf16_ring_kernel<{bn}, {i}, {e}>" for bn in (128, 64) for i in tf for e in EPIS]
    out += [f"conv3x3_bf16_thin_kernel<{e}>" for e in EPIS]
    tiles = ((128, 128), (128, 64), (64, 128), (64, 64))
    out += [f"conv3x3_wgrad_bf16_kernel<{bm}, {bn}, {i}, {io}>" for bm, bn in tiles for i in tf for io in tf]
    out += [f"conv3x3_wgrad_bf16s_kernel<{bm}, {bn}, {i}>" for bm, bn in tiles for i in tf]
    out += [f"conv3x3_wgrad9_bf16_kernel<{i}>" for i in tf]
    return out


# ------------------------------------------------------------------------------------------------ the cases
RING = {"bf16_ring": 1, "bf16_thin": 0}
# forward / input gradient: name -> (shape (B, H, W, cin, cout), knobs, io16 values, in_bn values, family of the forward)
FWD_CASES = {
    "k128-ragged": ((3, 5, 7, 64, 64), {}, (0, 1), (0, 1), "k128"),          # one ragged tile, 9 K-tiles (odd)
    "k128-two-tiles": ((5, 5, 7, 128, 128), {}, (0, 1), (0, 1), "k128"),     # full + ragged tile, 18 K-tiles, 128-wide
    "k128-nine-tiles": ((9, 11, 11, 64, 192), {}, (0, 1), (0, 1), "k128"),   # second group of eight; three column tiles
    "k128-144-ktiles": ((2, 8, 8, 1024, 64), {}, (0, 1), (0, 1), "k128"),
    "k128-m256": ((4, 8, 8, 64, 128), {"bf16_thin": 0}, (1,), (0, 1), "k128"),   # M % 256 == 0, kept on this kernel
    "ring-64": ((4, 8, 8, 64, 64), RING, (1,), (0, 1), "ring"),
    "ring-128": ((8, 8, 8, 128, 128), RING, (1,), (0, 1), "ring"),
    "ring-cin1024": ((4, 8, 8, 1024, 64), RING, (1,), (0, 1), "ring"),       # last cin it takes
    "ring-cin1088": ((4, 8, 8, 1088, 64), RING, (1,), (0, 1), "k128"),       # one step past the gate
    "thin-448": ((32, 2, 12, 64, 64), {}, (1,), (0,), "thin"),               # window exactly 448 rows
    "thin-449": ((64, 2, 10, 64, 64), {}, (1,), (0,), "k128"),               # 449 rows: refused
    "thin-16-samples": ((16, 4, 4, 128, 192), {}, (1,), (0,), "thin"),       # channel-block loop, 3 workgroups per window
    "thin-phases": ((64, 6, 6, 64, 64), {}, (1,), (0,), "thin"),             # tiles start at every phase of a sample
    "thin-16x16": ((1, 16, 16, 64, 128), {}, (1,), (0,), "thin"),
    "thin-level1": ((16, 4, 4, 128, 192), {"bf16_thin": 1}, (1,), (0,), "k128"),
    "thin-level2": ((16, 4, 4, 128, 192), {"bf16_thin": 2}, (1,), (0,), "k128"),
}
RING_TWIN = {"bf16_ring": 0, "bf16_thin": 0}    # ring-cin1088 must equal its result under these knobs bit for bit

WGRAD_KNOBS = {"default": {}, "per-tap": {"bf16_wgrad9": 0}, "round2": {"bf16_wgrad9": 0, "bf16_wgrad_swz": 0},
               "wgs256": {"wgrad9_wgs": 256}}
WGRAD_PAIRS = [(3, 5, 7, 64, 64), (3, 5, 7, 128, 128), (3, 5, 7, 128, 64), (3, 5, 7, 64, 128)]   # M = 105
WGRAD_FP32 = list(WGRAD_PAIRS)                                                # io16 = 0: the per-tap kernel's four tiles
WGRAD_IO16 = WGRAD_PAIRS + [(2, 4, 5, 64, 64),      # M = 40: fewer pixels than one K-tile
                            (9, 11, 11, 64, 64),    # several chunks, the last one ragged
                            (5, 21, 21, 64, 64),    # nine chunks: the chunk index passes the group of eight
                            (16, 4, 4, 64, 128)]    # 2.5 samples per 64-slot tile
WGRAD_RING = [(1, 3, 62, 64, 64), (1, 3, 63, 64, 64), (1, 2, 95, 64, 64), (1, 2, 96, 64, 64)]   # nine-tap ring geometry
WGRAD_TINY = [(70, 1, 1, 64, 64), (40, 1, 2, 64, 64), (40, 2, 1, 64, 64), (30, 2, 2, 64, 64), (20, 1, 7, 64, 64),
              (9, 3, 3, 64, 64)]
WGRAD_TINY_KNOBS = ("default", "per-tap")
PACK_SHAPES = [(64, 128), (192, 64)]               # (cout, cin)


def wgrad_runs():
    """Every (shape, io16, knob-set name) of the weight-gradient tests."""
    runs = [(s, 0, "default") for s in WGRAD_FP32]
    runs += [(s, 1, k) for k in WGRAD_KNOBS for s in WGRAD_IO16]
    runs += [(s, 1, "default") for s in WGRAD_RING]
    runs += [(s, 1, k) for k in WGRAD_TINY_KNOBS for s in WGRAD_TINY]
    return runs


def fwd_launches(name):
    """Every launch of one forward case -> [(role, shape as passed, in_bn, flags, io16)]: the forward with flags plain /
    statistics / inference epilogue x in_bn x io16, and the input gradient (the plain launch on dy, channels swapped)."""
    (B, Hh, W, cin, cout), _, io16s, in_bns, _ = FWD_CASES[name]
    out = [("fwd", (B, Hh, W, cin, cout), i, f | (FLAG_IN_BN if i else 0), io) for io in io16s for i in in_bns for f in FLAGS]
    return out + [("dgrad", (B, Hh, W, cout, cin), 0, 0, io) for io in io16s]


def reached():
    """instantiation -> the first case that reaches it, over every launch of every case (the 3.26 table)."""
    seen = {}
    for name in FWD_CASES:
        knobs = FWD_CASES[name][1]
        for role, shape, in_bn, flags, io16 in fwd_launches(name):
            seen.setdefault(fwd_kernel(shape, in_bn, flags, io16, knobs), f"{name} {role} io16={io16}")
    for shape, io16, kn in wgrad_runs():
        for in_bn in (0, 1):
            seen.setdefault(wgrad_kernel(shape, in_bn, io16, WGRAD_KNOBS[kn]),
                            "wgrad " + "x".join(map(str, shape)) + f" io16={io16} {kn}")
    return seen


def design_table():
    """The rows of the DESIGN.md 3.26 table, one per instantiation, from the model."""
    seen = reached()
    return [f"| `{inst}` | {seen.get(inst, 'NOT REACHED')} |" for inst in all_instantiations()]


# ------------------------------------------------------------------------------------------------ operands
def seed_of(shape, regime):
    return H.S.case_seed(*shape, REGIMES.index(regime))


@functools.lru_cache(maxsize=None)
def operands(shape, regime):
    """CPU operands of one (B, H, W, cin, cout): x, dy channels-last and bf16-representable, w [cout, cin, 3, 3] as the pack
    entry takes it (fp32), wr its bf16 rounding, bias, in_scale / in_shift, out_scale / out_shift."""
    B, Hh, W, cin, cout = shape
    g = torch.Generator().manual_seed(seed_of(shape, regime))
    if regime == "exact":
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()   # noqa: E731
        sc = lambda n: torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=g)] * (   # noqa: E731
            1.0 - 2.0 * torch.randint(0, 2, (n,), generator=g).float())
        d = {"x": ri(-4, 4, B, Hh, W, cin), "dy": ri(-4, 4, B, Hh, W, cout), "w": ri(-4, 4, cout, cin, 3, 3),
             "b": ri(-4, 4, cout), "isc": sc(cin), "ish": ri(-3, 3, cin), "osc": sc(cout), "osh": ri(-3, 3, cout)}
    else:
        rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
        d = {"x": H.r16(torch.relu(rn(B, Hh, W, cin))), "dy": H.r16(torch.relu(rn(B, Hh, W, cout))),
             "w": (1.0 + rn(cout, cin, 3, 3)) * (2.0 / (9 * cin)) ** 0.5, "b": rn(cout) * 0.1,
             "isc": torch.rand(cin, generator=g) + 0.5, "ish": rn(cin) * 0.3,
             "osc": torch.rand(cout, generator=g) + 0.5, "osh": rn(cout) * 0.3}
    d["wr"] = H.r16(d["w"])
    assert H.is16(d["x"]) and H.is16(d["dy"])
    return d


def staged(d, in_bn):
    """The A operand the kernel multiplies: x, or relu(fma(x, scale, shift)) in fp32 rounded once to bf16."""
    if not in_bn:
        return d["x"]
    return H.r16(torch.relu(torch.addcmul(d["ish"], d["x"], d["isc"])))


# ------------------------------------------------------------------------------------------------ references
def fp32_bound(mag, K):
    return CH.ELEM_DIRECT * U * math.sqrt(K) * mag


def infer_ref(v, b, osc, osh):
    """The inference epilogue relu(v out_scale + out_shift) before its ReLU, and the fp32 bound carried through the fma:
    |out_scale| b + 2 u (|out_scale v| + |out_shift|).  The ReLU is applied to both ends of the interval."""
    sc, sh = osc.double(), osh.double()
    pre = v * sc + sh
    return pre, sc.abs() * b + 2 * U * ((sc * v).abs() + sh.abs())


def tile_stats(v, b=None):
    """Per 128-row tile and channel of the unrounded v [M, C]: rows, sum, M2 about the tile mean, and their bounds.
    b = None (exact regime): the sum is exact, M2 within LAM u sqrt(rows) M2.  b = the per-element fp32 bound of v
    (rounding regime): the sum carries sum b + LAM u sqrt(rows) sum |v|; M2 = sum (v - mean)^2 moves by at most
    2 sum |v - mean| (b + b_sum / rows) to first order, plus its own LAM u sqrt(rows) M2."""
    M, C = v.shape
    tiles = -(-M // STAT_ROWS)
    s, m2, bs, bm = (torch.empty(tiles, C, dtype=torch.float64) for _ in range(4))
    for t in range(tiles):
        blk = v[t * STAT_ROWS:(t + 1) * STAT_ROWS]
        rows = blk.shape[0]
        dev = blk - blk.mean(0)
        s[t], m2[t] = blk.sum(0), dev.pow(2).sum(0)
        bm[t] = LAM * U * math.sqrt(rows) * m2[t]
        if b is None:
            bs[t] = 0
        else:
            bb = b[t * STAT_ROWS:(t + 1) * STAT_ROWS]
            bs[t] = bb.sum(0) + LAM * U * math.sqrt(rows) * blk.abs().sum(0)
            bm[t] += 2 * (dev.abs() * (bb + bs[t] / rows)).sum(0)
    return {"sum": s, "m2": m2, "b_sum": bs, "b_m2": bm}


@functools.lru_cache(maxsize=None)
def fwd_refs(shape, regime, in_bn):
    """Forward references of one case: conv + bias (ref, mag, K), the epilogue's pre-activation and bound, tile statistics."""
    d = operands(shape, regime)
    a = staged(d, in_bn)
    ref = CH.conv_ref64(a, d["wr"], d["b"])
    mag = CH.conv_ref64(a.abs(), d["wr"].abs(), d["b"].abs())
    K = 9 * shape[3]
    b = fp32_bound(mag, K)
    pre, b_inf = infer_ref(ref, b, d["osc"], d["osh"])
    mag_inf = mag * d["osc"].double().abs() + d["osh"].double().abs()
    C = shape[4]
    st = tile_stats(ref.reshape(-1, C), None if regime == "exact" else b.reshape(-1, C))
    return {"ref": ref, "mag": mag, "K": K, "b": b, "pre": pre, "b_inf": b_inf, "mag_inf": mag_inf, "stats": st}


@functools.lru_cache(maxsize=None)
def dgrad_refs(shape, regime):
    d = operands(shape, regime)
    ref, mag, K = CH.dgrad_ref64(d["dy"], d["wr"]), CH.dgrad_ref64(d["dy"].abs(), d["wr"].abs()), 9 * shape[4]
    return {"ref": ref, "mag": mag, "K": K, "b": fp32_bound(mag, K)}


@functools.lru_cache(maxsize=None)
def wgrad_refs(shape, regime, in_bn):
    d = operands(shape, regime)
    a = staged(d, in_bn)
    return {"ref": CH.wgrad_ref64(a, d["dy"]), "mag": CH.wgrad_ref64(a.abs(), d["dy"].abs()), "K": shape[0] * shape[1] * shape[2]}


# ------------------------------------------------------------------------------------------------ gates
def interval16_relu(pre, b):
    """[RNE(relu(pre - b)), RNE(relu(pre + b))]: rounding keeps sign and zero, so the ReLU commutes with it."""
    lo, hi = H.interval16(pre, b)
    return lo.clamp_min(0), hi.clamp_min(0)


def undecided(ref, b, relu=False):
    lo, hi = interval16_relu(ref, b) if relu else H.interval16(ref, b)
    return float((lo != hi).double().mean())


def held(got, regime, ref, b, mag, K, relu=False):
    """-> (passes, figure) of one output `got` (fp32 or bf16 tensor) against its reference; relu: ref is the epilogue's
    pre-activation and b its carried bound.  exact: equality with the fp64 reference (fp32) / with rne16_64 of it
    (bf16), figure = mismatching elements.  rounding: elem_ratio <= ELEM_DIRECT (fp32; behind the ReLU, which is
    1-Lipschitz, |got - relu(pre)| / b in the same units) / no element outside the interval (bf16), figure = worst
    ratio in units of the bound."""
    g = got.detach().double().cpu()
    want = ref.clamp_min(0) if relu else ref
    is16 = got.dtype == torch.bfloat16
    if regime == "exact":
        want = H.rne16_64(want) if is16 else want.float().double()
        bad = int((~(g == want)).sum())
        return bad == 0, bad
    if is16:
        if relu:
            lo, hi = interval16_relu(ref, b)
            out = int((~((g >= lo) & (g <= hi))).sum())
        else:
            out = H.outside16(g, ref, b)
        return out == 0, H.ratio16(g, want, b)
    if relu:
        if bool(torch.isnan(g).any()) or bool(((g - want).abs()[b == 0] > 0).any()):
            return False, float("inf")
        r = float(((g - want).abs() / b.clamp_min(1e-300)).max()) * CH.ELEM_DIRECT
    else:
        r = CH.elem_ratio(g, ref, mag, K)
    return (r <= CH.ELEM_DIRECT and not bool(torch.isnan(g).any())), r


def stats_held(got, st, regime):
    """got [tiles, 2, C] (sum, M2) against tile_stats -> (passes, worst sum figure, worst M2 figure); figures are
    |error| / bound (exact sums: mismatching elements)."""
    g = got.detach().double().cpu()
    if bool(torch.isnan(g).any()):
        return False, float("inf"), float("inf")
    es, em = (g[:, 0] - st["sum"]).abs(), (g[:, 1] - st["m2"]).abs()
    fm = float((em / st["b_m2"].clamp_min(1e-300)).max()) if bool((em > 0).any()) else 0.0
    if regime == "exact":
        fs = int((g[:, 0] != st["sum"].float().double()).sum())
        return fs == 0 and bool((em <= st["b_m2"]).all()), fs, fm
    fs = float((es / st["b_sum"].clamp_min(1e-300)).max())
    return bool((es <= st["b_sum"]).all()) and bool((em <= st["b_m2"]).all()), fs, fm


def pack_refs(w):
    """tdx_pack_conv3x3_bf16 on w [cout, cin, 3, 3]: the forward pack [cout][9][cin] and the mirrored input-gradient pack
    [cin][8 - tap][cout], both rounded to bf16 (nearest even)."""
    cout, cin = w.shape[:2]
    wf = w.permute(0, 2, 3, 1).reshape(cout, 9, cin)
    wd = wf.flip(1).permute(2, 1, 0)
    return wf.bfloat16().contiguous(), wd.bfloat16().contiguous()
