"""fp64 references, error bounds, input builders and a host model of the dispatch of csrc/time_embed.hip (DESIGN.md
3.20).  Plain module, no fixtures: tests/test_time_path_refs_host.py checks it against torch on the CPU,
tests/test_gpu_time_path_dispatch.py holds the kernels against it.

Every reference is one STAGE of the path, computed from the operands the kernel of that stage reads (for the GPU test:
the device's own fp32 `pre`, `emb`, `g_emb`, `g_h`), so an error in one kernel shows in that kernel's outputs only.
A stage is a function of a dtype: evaluated in fp64 it is the reference, on absolute values the magnitude-sum, in fp32
the CPU restatement that the host test holds against the same bounds.

Bounds.  u = 2^-24; |got - ref| <= LAM u sqrt(K) mag (+ the two terms below), the model of tests/spatial_helpers.py;
K, the count of fp32 roundings behind one output, is read off the kernel and stated where each bound is formed.
Nothing here was fitted to a kernel's output.
  * SiLU is x / (1 + expf(-x)): expf (1 ulp = 2 u), the sum and the quotient, K_SILU = 4, relative to |silu(x)|.
  * SiLU' is s (1 + x (1 - s)), s = 1 / (1 + expf(-x)).  s carries 4 u; 1 - s is exact (Sterbenz) or rounded once, so
    x (1 - s) is off by at most 4 u |x| s-relative; the product and the two sums add 4 more.  All of it is within
    K_DSILU = 8 roundings of the magnitude s (1 + |x|), which replaces |silu'(x)| in every magnitude-sum.
  * Underflow.  For x < -87.3 the sigmoid s < 2^-126 is denormal or flushed, and below -88.72 expf(-x) overflows and
    both functions return 0; the true values there are at most (1 + |x|) 2^-126.  The relative model says nothing about
    them (mag itself is ~1e-38), so every sum over SiLU or SiLU' terms gets the absolute term
    (terms) 2^-126 (1 + max|pre|) x (the largest cofactors), `underflow()`.
  * Sinusoid.  The angle is t f_j, f_j = expf(-logf(1e4) j / (half - 1)): logf, the product and the quotient put
    3 u |arg| on the argument of expf (|arg| <= 9.22), expf adds 2 u and t f one more: the angle is off by at most
    (3 |arg| + 3) u |t f|, and so is its sine or cosine; sinf / cosf add 2 ulp = 4 u of their own.  At t = 0 the angle
    is exactly 0 and sin 0 = 0, cos 0 = 1 are exact: the bound is 0 there.  At t = 999, j = 0 this is 1.8e-4, the
    1.5e-4 of tests/test_gpu_laion.py's sinusoid check at the same place."""
import math

import torch

U = 2.0 ** -24
LAM = 9.0
TINY = 2.0 ** -126
K_SILU = 4
K_DSILU = 8
TDX_E_BADARG = -1
TDX_E_SHAPE = -2
PART_PROJ, PART_MID, PART_L1 = 1, 2, 4

# constants of csrc/time_embed.hip that decide a branch (test_time_path_refs_host.py pins what follows from them, so a
# change there shows up as a failed expectation)
ROW_WIDTHS = (256, 512, 768, 1024)   # td_fast: multiples of 256 up to 1024 take linear_rows_kernel<R = td / 256>
ROW_OUT_BLOCK = 64                   # ... if the output width is a multiple of 64 (one workgroup = 64 output rows)
ROW_NB = 4                           # samples per workgroup of the row kernels; the sample index is clamped to B - 1
L1_COLS, L1_SLICES = 32, 8           # time_l1_bwd_kernel: 32 columns x 8 interleaved slices of the batch
LABEL_TRIP = 256                     # class_emb_bwd_kernel: labels per LDS trip
TD_MAX = 4096
TD_MIN = {0: 1, 1: 4}
FUSED_TD = 256                       # kind 0 at this width: time_emb_kernel + time_proj_kernel
PROJ = {0: (128, 256, 512), 1: (64, 128, 256)}
NUM_CLASSES = 10

# slots of the TDX_P_* parameter table (include/tdx.h) that the path reads
SLOT = {"w1": 0, "b1": 1, "w2": 2, "b2": 3, "E": 4, "pw0": 61, "pb0": 62, "pw1": 63, "pb1": 64, "pw2": 65, "pb2": 66}
SLOT_COUNT = 67
SLOT_NAMES = {"w1": "time_embedding.0.weight", "b1": "time_embedding.0.bias", "w2": "time_embedding.2.weight",
              "b2": "time_embedding.2.bias", "E": "class_embedding.weight", "pw0": "time_proj1.weight",
              "pb0": "time_proj1.bias", "pw1": "time_proj2.weight", "pb1": "time_proj2.bias",
              "pw2": "time_proj3.weight", "pb2": "time_proj3.bias"}


def case_seed(*xs):
    s = 17
    for x in xs:
        s = (s * 1000003 + int(x) + 7) % (2 ** 31 - 1)
    return s


def elem_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound; where the bound is 0 the element must be exact.  NaN / inf count as
    inf."""
    err = (got.double() - ref).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    zero = bound == 0
    if bool((err[zero] > 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / bound[~zero]).max())


# ------------------------------------------------------------------------------------------------ the case list
# (kind, time_dim, batch, labels): labels "none" | "labels" | "null" (labels of which some are negative) for kind 0,
# "text" for kind 1.  Every width has a small batch and one with B % 4 != 0; the large batches go with 256 and 100.
K0_SHAPES = [(1, 1), (1, 5), (33, 2), (33, 7), (64, 3), (64, 9), (100, 5), (100, 8), (100, 37), (100, 257), (100, 600),
             (255, 2), (255, 7), (256, 1), (256, 2), (256, 3), (256, 5), (256, 7), (256, 8), (256, 9), (256, 37),
             (256, 257), (256, 600), (257, 3), (257, 5), (512, 2), (512, 9), (768, 3), (768, 8), (1024, 5), (1024, 8),
             (1024, 9), (1280, 1), (1280, 7), (4096, 3)]
K0_NULL_SHAPES = [(256, 5), (256, 37), (100, 5), (100, 257), (512, 9), (33, 7)]
K1_SHAPES = [(4, 1), (4, 5), (5, 2), (5, 7), (100, 5), (100, 8), (100, 37), (100, 257), (256, 3), (256, 8), (256, 37),
             (256, 600), (512, 2), (512, 9), (768, 5), (768, 8), (768, 300), (1024, 3), (1024, 9), (1280, 2),
             (1280, 7)]
CASES = [(0, td, B, lab) for td, B in K0_SHAPES for lab in ("none", "labels")] \
    + [(0, td, B, "null") for td, B in K0_NULL_SHAPES] + [(1, td, B, "text") for td, B in K1_SHAPES]
REFUSED = [(0, 4097), (0, 0), (1, 3), (1, 4097)]
# the step's order against the one-call backward, bit for bit
PARTS_CASES = [(0, 256, 37, "labels"), (0, 256, 5, "none"), (0, 100, 9, "null"), (1, 768, 5, "text"),
               (1, 100, 7, "text")]
# sampling tables through the module: (kind, time_dim, batch, labels)
TABLE_CASES = [(0, 256, 3, "null"), (0, 256, 3, "none"), (0, 512, 3, "null"), (0, 512, 3, "none"), (0, 100, 3, "null"),
               (0, 100, 3, "none"), (1, 768, 2, "text"), (1, 100, 2, "text")]


def case_id(case):
    return "-".join(str(x) for x in case)


# ------------------------------------------------------------------------------------------------ host model
def td_ok(kind, td):
    return TD_MIN[kind] <= td <= TD_MAX


def linear_kernel(td, out_width, silu):
    """Which kernel linear_rows<IN_SILU> launches for an input width td and an output width out_width."""
    if td in ROW_WIDTHS and out_width % ROW_OUT_BLOCK == 0:
        return f"linear_rows_kernel<R={td // 256},silu={int(silu)}>"
    return f"linear_generic_kernel<silu={int(silu)}>"


def _linear(out, td, width, silu, B, addend=False, null_bias=False):
    k = linear_kernel(td, width, silu)
    out.add(k)
    if k.startswith("linear_rows"):
        if B % ROW_NB:
            out.add("rows:clamped_sample")
        if addend:
            out.add("rows:addend")
        if null_bias:
            out.add("rows:null_bias")
    else:
        if addend:
            out.add("generic:addend")
        if null_bias:
            out.add("generic:null_bias")
        if td % 256 == 0:
            out.add("generic:multiple_of_256")


def branch(kind, td, B, labels="none"):
    """Names of the kernels (and of the branches inside them) that tdx_time_path_fwd followed by tdx_time_path_bwd with
    all parts reaches for one case."""
    assert td_ok(kind, td) and B > 0
    out = set()
    if kind == 0 and td == FUSED_TD:
        out |= {"time_emb_kernel", "time_proj_kernel"}
        if labels == "null":
            out.add("time_emb_kernel:null_label")
    elif kind == 0:
        out.add("time_l1_fwd_kernel")
        _linear(out, td, td, True, B)
        if labels != "none":
            out.add("add_class_emb_kernel")
        for w in PROJ[0]:
            _linear(out, td, w, False, B)
    else:
        out.add("sinusoid_kernel")
        if td % 2:
            out.add("sinusoid_kernel:odd_zero_column")
        _linear(out, td, td, False, B)
        _linear(out, td, td, True, B, addend=True)
        for w in PROJ[1]:
            _linear(out, td, w, False, B)
    out |= {"lin_wgrad_kernel", "lin_dgrad_kernel", "silu_kernel", f"backward:kind{kind}:td={td}"}
    if kind == 0:
        out.add("time_l1_bwd_kernel")
        if td % L1_COLS:
            out.add("time_l1_bwd_kernel:ragged_last_workgroup")
        if B < L1_SLICES:
            out.add("time_l1_bwd_kernel:empty_slices")
        if labels != "none":
            out.add("class_emb_bwd_kernel")
            out.add(f"class_emb_bwd_kernel:trips={-(-B // LABEL_TRIP)}")
    else:
        out.add("silu_bwd_kernel")
    return out


def branch_tables(kind, td, B, labels):
    """tdx_time_tables_build over T rows, tdx_time_tables_cond over B rows and the look-up of a step."""
    out = {"sample_head_kernel"}
    T = 7
    out |= {b for b in branch(kind, td, T, "none") if "bwd" not in b and "grad" not in b and b != "silu_kernel"
            and not b.startswith("backward")}
    if labels != "none":
        if kind == 0:
            out.add("class_rows_kernel")
        for w in PROJ[kind]:
            _linear(out, td, w, False, B, null_bias=True)
    return out


# ------------------------------------------------------------------------------------------------ inputs
def make_operands(kind, td, B, labels, seed=None, device="cpu"):
    """Operands of one case, fp32 / int64 on `device`, initialised as the reference's modules are: Linear and Conv2d
    U(+-1/sqrt(fan_in)) for weight and bias (so time_embedding.0.weight of kind 0 lies in +-1 and |pre| reaches 999),
    Embedding N(0, 1).  t holds 0 and 999 (B = 1: 999 alone); labels hold a repeat, use classes 0..7 of 10 only (8 and
    9 stay absent) and for "null" hold -1 and one other negative value; text rows and the gradients g_tk are N(0, 1)."""
    g = torch.Generator().manual_seed(case_seed(kind, td, B, len(labels)) if seed is None else seed)

    def uni(shape, fan_in):
        return (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in)

    fan1 = 1 if kind == 0 else td
    d = {"w1": uni((td, fan1), fan1), "b1": uni((td,), fan1), "w2": uni((td, td), td), "b2": uni((td,), td)}
    for k, w in enumerate(PROJ[kind]):
        d[f"pw{k}"] = uni((w, td), td)
        d[f"pb{k}"] = uni((w,), td)
        d[f"g{k}"] = torch.randn(B, w, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    t[0] = 999
    if B > 1:
        t[B - 1] = 0
    d["t"] = t
    d["y"] = d["cond"] = d["E"] = None
    if kind == 1:
        d["cond"] = torch.randn(B, td, generator=g)
    elif labels != "none":
        d["E"] = torch.randn(NUM_CLASSES, td, generator=g)
        y = torch.randint(0, 8, (B,), generator=g)
        if B > 1:
            y[1] = y[0]
        if labels == "null":
            assert B >= 3
            y[B - 1] = -1
            y[B // 2] = -7
        d["y"] = y
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ stages
def silu(x):
    return x * torch.sigmoid(x)


def dsilu(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def dsilu_mag(x):
    return torch.sigmoid(x) * (1 + x.abs())


def underflow(terms, pre, *cofactors):
    """The absolute term of a sum of `terms` products of SiLU(pre) or SiLU'(pre) with the given cofactors (module
    docstring): terms x 2^-126 x (1 + max|pre|) x prod max(1, max|cofactor|)."""
    v = terms * TINY * (1.0 + float(pre.abs().max()))
    for c in cofactors:
        v *= max(1.0, float(c.abs().max()))
    return v


def _bound(K, mag, extra=0.0):
    return LAM * U * math.sqrt(K) * mag + extra


def sinusoid_ref(t, td):
    """get_timestep_embedding (conditional_diffusion_laion.py:222-232) with exact frequencies -> (reference, bound)."""
    half = td // 2
    k = torch.arange(half, dtype=torch.float64, device=t.device)
    arg = -math.log(10000.0) * k / (half - 1)
    ang = t.double()[:, None] * torch.exp(arg)[None, :]
    ref = torch.zeros(t.shape[0], td, dtype=torch.float64, device=t.device)
    ref[:, :half], ref[:, half:2 * half] = torch.sin(ang), torch.cos(ang)
    b = (3 * arg.abs() + 3)[None, :] * U * ang.abs() + 4 * U * (t != 0).double()[:, None]
    bound = torch.zeros_like(ref)
    bound[:, :half], bound[:, half:2 * half] = b, b
    return ref, bound


def sinusoid_fp32(t, td):
    """The reference's own fp32 sequence."""
    half = td // 2
    f = torch.exp(torch.arange(half, dtype=torch.float32, device=t.device) * -(math.log(10000) / (half - 1)))
    e = t.float()[:, None] * f[None, :]
    e = torch.cat([torch.sin(e), torch.cos(e)], 1)
    return torch.nn.functional.pad(e, (0, 1)) if td % 2 else e


def _lin(x, w, b, dt, absval):
    c = (lambda v: v.to(dt).abs()) if absval else (lambda v: v.to(dt))
    y = c(x) @ c(w).t()
    return y if b is None else y + c(b)


def pre_stage(kind, d, aux, dt=torch.float64, absval=False):
    """kind 0: fmaf(w1, float(t), b1), one rounding; kind 1: W1 sinusoid + b1 from the given sinusoid."""
    x = d["t"].to(dt)[:, None] if kind == 0 else aux
    return _lin(x, d["w1"], d["b1"], dt, absval)


def pre_ref(kind, d, aux):
    K = 1 if kind == 0 else aux.shape[1] + 1     # one fma | dot of length td and the bias
    return pre_stage(kind, d, aux), _bound(K, pre_stage(kind, d, aux, absval=True))


def addend_of(kind, d, dt):
    """The rows added to the time embedding: E[y] (0 for a negative label), the text rows, or None."""
    if kind == 1:
        return d["cond"].to(dt)
    if d["y"] is None:
        return None
    y = d["y"]
    return d["E"].to(dt)[y.clamp(min=0)] * (y >= 0).to(dt)[:, None]


def emb_stage(kind, d, pre, dt=torch.float64, absval=False):
    h = silu(pre.to(dt))
    e = _lin(h, d["w2"], d["b2"], dt, absval)
    a = addend_of(kind, d, dt)
    return e if a is None else e + (a.abs() if absval else a)


def emb_ref(kind, d, pre):
    """K = td products-and-sums of the dot + the bias + the addend + K_SILU on every term."""
    td = pre.shape[1]
    return emb_stage(kind, d, pre), _bound(td + 2 + K_SILU, emb_stage(kind, d, pre, absval=True),
                                           underflow(td, pre, d["w2"]))


def proj_stage(d, k, emb, dt=torch.float64, absval=False, bias=True):
    return _lin(emb, d[f"pw{k}"], d[f"pb{k}"] if bias else None, dt, absval)


def proj_ref(d, k, emb):
    """K = td + 1: the dot and the bias."""
    return proj_stage(d, k, emb), _bound(emb.shape[1] + 1, proj_stage(d, k, emb, absval=True))


def gemb_stage(kind, d, dt=torch.float64, absval=False, upto=3):
    c = (lambda v: v.to(dt).abs()) if absval else (lambda v: v.to(dt))
    return sum(c(d[f"g{k}"]) @ c(d[f"pw{k}"]) for k in range(upto))


def gemb_ref(kind, d, upto=3):
    """One fma chain over the outputs of the projections 0 .. upto - 1 (lin_dgrad_kernel, accumulating): K = their
    total width."""
    return gemb_stage(kind, d, upto=upto), _bound(sum(PROJ[kind][:upto]), gemb_stage(kind, d, absval=True, upto=upto))


def wgrad_stage(g, x, dt=torch.float64, absval=False):
    c = (lambda v: v.to(dt).abs()) if absval else (lambda v: v.to(dt))
    return c(g).t() @ c(x), c(g).sum(0)


def wgrad_ref(g, x, extra_k=0, extra=0.0):
    """lin_wgrad_kernel: dW[o][j] = sum_n g[n][o] x[n][j], db[o] = sum_n g[n][o]: K = B (+ what x carries)."""
    (dw, db), (mw, mb) = wgrad_stage(g, x), wgrad_stage(g, x, absval=True)
    return (dw, _bound(g.shape[0] + extra_k, mw, extra)), (db, _bound(g.shape[0], mb))


def class_emb_grad_ref(d, g_emb):
    """dE[c] = sum over the samples labelled c, in fp32: K = B.  Absent classes and negative labels: exactly 0."""
    y, g64 = d["y"], g_emb.double()
    onehot = torch.zeros(NUM_CLASSES, y.shape[0], dtype=torch.float64, device=g_emb.device)
    idx = (y >= 0).nonzero().flatten()
    onehot[y[idx], idx] = 1.0
    return onehot @ g64, _bound(y.shape[0], onehot @ g64.abs())


def h_ref(pre):
    r = silu(pre.double())
    return r, _bound(K_SILU, r.abs(), underflow(1, pre))


def gh_stage(kind, d, g_emb, pre, dt=torch.float64, absval=False):
    c = (lambda v: v.to(dt).abs()) if absval else (lambda v: v.to(dt))
    gh = c(g_emb) @ c(d["w2"])
    if kind == 1:                      # silu_bwd_kernel multiplies in place
        gh = gh * (dsilu_mag(pre.to(dt)) if absval else dsilu(pre.to(dt)))
    return gh


def gh_ref(kind, d, g_emb, pre):
    """lin_dgrad_kernel: K = td; kind 1 also takes SiLU' and a product, K_DSILU + 1."""
    td = pre.shape[1]
    K = td + (K_DSILU + 1 if kind == 1 else 0)
    extra = underflow(1, pre, gh_stage(0, d, g_emb, pre, absval=True)) if kind == 1 else 0.0
    return gh_stage(kind, d, g_emb, pre), _bound(K, gh_stage(kind, d, g_emb, pre, absval=True), extra)


def l1_grad_stage(kind, d, g_h, pre, aux, dt=torch.float64, absval=False):
    """kind 0: g_pre = g_h silu'(pre), dW1 = sum_n g_pre t, db1 = sum_n g_pre; kind 1: g_h already is g_pre and the
    first layer is a plain weight gradient against the sinusoid."""
    c = (lambda v: v.to(dt).abs()) if absval else (lambda v: v.to(dt))
    if kind == 1:
        return wgrad_stage(g_h, aux, dt, absval)
    gp = c(g_h) * (dsilu_mag(pre.to(dt)) if absval else dsilu(pre.to(dt)))
    return (gp * c(aux)[:, None]).sum(0)[:, None], gp.sum(0)


def l1_grad_ref(kind, d, g_h, pre, aux):
    """kind 0 (time_l1_bwd_kernel): per term SiLU' (K_DSILU), the product with g_h and the fma with t; B / 8 terms per
    slice and 8 slices: K = B + K_DSILU + 10.  Underflow: B terms x 2^-126 (1 + max|pre|) max|t| max|g_h|."""
    B = g_h.shape[0]
    (dw, db), (mw, mb) = l1_grad_stage(kind, d, g_h, pre, aux), l1_grad_stage(kind, d, g_h, pre, aux, absval=True)
    if kind == 1:
        return (dw, _bound(B, mw)), (db, _bound(B, mb))
    K = B + K_DSILU + 10
    return (dw, _bound(K, mw, underflow(B, pre, aux, g_h))), (db, _bound(K, mb, underflow(B, pre, g_h)))


# ------------------------------------------------------------------------------------------------ whole stages at once
def forward_checks(kind, d, dev_out):
    """{stage: (reference, bound)} of the forward from the operands and the given `aux`, `pre`, `emb` (the device's own,
    or a restatement's)."""
    out = {}
    if kind == 0:
        out["aux"] = (d["t"].double(), torch.zeros(d["t"].shape, dtype=torch.float64, device=d["t"].device))
    else:
        out["aux"] = sinusoid_ref(d["t"], d["w2"].shape[0])
    out["pre"] = pre_ref(kind, d, dev_out["aux"].double())
    out["emb"] = emb_ref(kind, d, dev_out["pre"])
    for k in range(3):
        out[f"t{k + 1}"] = proj_ref(d, k, dev_out["emb"])
    return out


def backward_checks(kind, d, dev):
    """{stage: (reference, bound)} of the backward from the operands, the forward's `aux`, `pre`, `emb` and the given
    scratch blocks `g_emb`, `g_h`."""
    out = {"g_emb": gemb_ref(kind, d)}
    for k in range(3):
        out[f"pw{k}"], out[f"pb{k}"] = wgrad_ref(d[f"g{k}"], dev["emb"])
    if kind == 0 and d["y"] is not None:
        out["E"] = class_emb_grad_ref(d, dev["g_emb"])
    out["h"] = h_ref(dev["pre"])
    td = dev["pre"].shape[1]
    out["w2"], out["b2"] = wgrad_ref(dev["g_emb"], silu(dev["pre"].double()), K_SILU,
                                     underflow(dev["pre"].shape[0], dev["pre"], dev["g_emb"]))
    out["g_h"] = gh_ref(kind, d, dev["g_emb"], dev["pre"])
    out["w1"], out["b1"] = l1_grad_ref(kind, d, dev["g_h"], dev["pre"], dev["aux"])
    assert td == d["w2"].shape[0]
    return out


def restate_fp32(kind, d):
    """The whole path in plain fp32 torch, stage by stage (each stage from the previous fp32 stage): what the bounds
    must admit with room to spare.  -> dict with the forward outputs, the scratch blocks and the gradients."""
    f32 = torch.float32
    td = d["w2"].shape[0]
    r = {"aux": d["t"].float() if kind == 0 else sinusoid_fp32(d["t"], td)}
    r["pre"] = pre_stage(kind, d, r["aux"], f32)
    r["emb"] = emb_stage(kind, d, r["pre"], f32)
    for k in range(3):
        r[f"t{k + 1}"] = proj_stage(d, k, r["emb"], f32)
    r["g_emb"] = gemb_stage(kind, d, f32)
    for k in range(3):
        r[f"pw{k}"], r[f"pb{k}"] = wgrad_stage(d[f"g{k}"], r["emb"], f32)
    if kind == 0 and d["y"] is not None:
        e = torch.zeros(NUM_CLASSES, td)     # an fp32 sum in sample order
        for n, c in enumerate(d["y"].tolist()):
            if c >= 0:
                e[c] += r["g_emb"][n]
        r["E"] = e
    r["h"] = silu(r["pre"])
    r["w2"], r["b2"] = wgrad_stage(r["g_emb"], r["h"], f32)
    r["g_h"] = gh_stage(kind, d, r["g_emb"], r["pre"], f32)
    r["w1"], r["b1"] = l1_grad_stage(kind, d, r["g_h"], r["pre"], r["aux"], f32)
    return r


def stage_ratios(kind, d, r):
    """Worst |r - reference| / bound per stage for a run r (the device's or a restatement's) whose every stage is held
    against the reference formed from r's own earlier stages."""
    checks = dict(forward_checks(kind, d, r))
    checks.update(backward_checks(kind, d, r))
    return {k: elem_ratio(r[k].reshape(ref.shape), ref, bound) for k, (ref, bound) in checks.items()}


# ------------------------------------------------------------------------------------------------ composed path (autograd)
def composed_autograd(kind, d):
    """The path as the reference's modules compose it, in fp64 with torch autograd -> (outputs, gradients)."""
    td = d["w2"].shape[0]
    P = {k: d[k].double().requires_grad_(True) for k in SLOT if d.get(k) is not None}
    if kind == 0:
        x = d["t"].double()[:, None]
    else:
        x = sinusoid_ref(d["t"], td)[0]
    pre = x @ P["w1"].t() + P["b1"]
    emb = torch.nn.functional.silu(pre) @ P["w2"].t() + P["b2"]
    if kind == 1:
        emb = emb + d["cond"].double()
    elif d["y"] is not None:
        keep = d["y"] >= 0
        emb = emb + torch.nn.functional.embedding(d["y"].clamp(min=0), P["E"]) * keep.double()[:, None]
    outs = [emb @ P[f"pw{k}"].t() + P[f"pb{k}"] for k in range(3)]
    sum((o * d[f"g{k}"].double()).sum() for k, o in enumerate(outs)).backward()
    return {"aux": x, "pre": pre.detach(), "emb": emb.detach(), "t1": outs[0].detach(), "t2": outs[1].detach(),
            "t3": outs[2].detach()}, {k: v.grad for k, v in P.items()}


def chained_fp64(kind, d):
    """The stage references chained in fp64 (each stage fed the previous reference): must equal composed_autograd."""
    td = d["w2"].shape[0]
    r = {"aux": d["t"].double() if kind == 0 else sinusoid_ref(d["t"], td)[0]}
    r["pre"] = pre_stage(kind, d, r["aux"])
    r["emb"] = emb_stage(kind, d, r["pre"])
    for k in range(3):
        r[f"t{k + 1}"] = proj_stage(d, k, r["emb"])
    r["g_emb"] = gemb_stage(kind, d)
    for k in range(3):
        r[f"pw{k}"], r[f"pb{k}"] = wgrad_stage(d[f"g{k}"], r["emb"])
    if kind == 0 and d["y"] is not None:
        r["E"] = class_emb_grad_ref(d, r["g_emb"])[0]
    r["w2"], r["b2"] = wgrad_stage(r["g_emb"], silu(r["pre"]))
    r["g_h"] = gh_stage(kind, d, r["g_emb"], r["pre"])
    r["w1"], r["b1"] = l1_grad_stage(kind, d, r["g_h"], r["pre"], r["aux"])
    return r


# ------------------------------------------------------------------------------------------------ sampling tables
SILU_LIP = 1.1    # max |silu'| = 1.0998


def table_rows_ref(kind, d, t_rows, k):
    """What a table-mode step leaves in the projection slot k: tab_k[t] + tabc_k[b] = (W_k MLP(t) + b_k) + W_k c_b, in
    fp64 from t (the table's intermediate rows are not visible to a caller) -> (reference, bound).  The bound is the
    stage bound of the two-term form, K = td + 1 over |W_k| |MLP(t)| + |b_k| + |W_k| |c_b| (plus the one sum of the two
    rows), and the stage bounds of the rows behind it carried forward: the sinusoid's through |W1|, pre's through SiLU
    (Lipschitz 1.1) and |W2|, emb's through |W_k|."""
    dd = dict(d, t=t_rows, y=None, cond=None)
    td = d["w2"].shape[0]
    kk = 0 if kind == 0 else 1
    aux, b_aux = (t_rows.double(), None) if kind == 0 else sinusoid_ref(t_rows, td)
    pre, b_pre = pre_ref(kk, dd, aux)
    if b_aux is not None:
        b_pre = b_pre + b_aux @ d["w1"].double().abs().t()
    emb = _lin(silu(pre), d["w2"], d["b2"], torch.float64, False)
    m_emb = _lin(silu(pre), d["w2"], d["b2"], torch.float64, True)
    b_emb = _bound(td + 1 + K_SILU, m_emb, underflow(td, pre, d["w2"])) + (SILU_LIP * b_pre) @ d["w2"].double().abs().t()
    c = addend_of(kind, d, torch.float64)
    W = d[f"pw{k}"].double()
    ref = emb @ W.t() + d[f"pb{k}"].double()
    mag = m_emb @ W.abs().t() + d[f"pb{k}"].double().abs()
    if c is not None:
        ref = ref + c @ W.t()
        mag = mag + c.abs() @ W.abs().t()
    return ref, _bound(td + 2, mag) + b_emb @ W.abs().t()


# ------------------------------------------------------------------------------------------------ planted extremes
EXTREMES = (88.0, -88.0, 104.0, -104.0, 999.0, -999.0, 87.5, -87.5)


def plant_extremes(kind, d, aux):
    """Move b1 so that the pre-activations of sample 0 in the first columns land on +-88, +-104 and +-999 (the edges of
    expf in SiLU and SiLU'; +-87.5 sits in the denormal range of the sigmoid) to fp32 rounding.  aux: float(t) or the
    sinusoid the device computed.  In place."""
    n = min(len(EXTREMES), d["b1"].shape[0])
    x = (d["t"].double()[:, None] if kind == 0 else aux.double())[0]
    cur = d["w1"].double()[:n] @ x
    d["b1"][:n] = (torch.tensor(EXTREMES[:n], dtype=torch.float64, device=cur.device) - cur).float()
    return n
