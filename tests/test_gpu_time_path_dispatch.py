"""Every branch of csrc/time_embed.hip against fp64, per element: the time / class / text path on its
own through tdx_time_path_fwd, tdx_time_path_bwd and tdx_time_path_proj_bwd at both kinds, at widths on both sides of
every dispatch decision (the fused kernels of kind 0 at 256, the row kernels at R = 1 .. 4, the generic kernels at
every other width, 1280 and 4096 among them), at every B % 4, below and across the eight batch slices of the first
layer's backward and over one, two and three label trips; the `parts` protocol of the training step bit for bit; the
sampling tables through the module; and the whole network at two non-default widths.

References, bounds, input builders and the case lists are those of tests/time_path_helpers.py (checked on the CPU by
tests/test_time_path_refs_host.py, which also states which branch each case reaches): every stage in fp64 from the
operands its kernel read - the device's own pre, emb, g_emb, g_h - and |got - ref| <= 9 u sqrt(K) x magnitude-sum per
element, K read off the kernel where each bound is formed.  Every output is pre-filled with NaN and followed by guard
floats.  The norm-wise gate of tests/test_gpu_ops.py::test_time_mlp_fwd_bwd stays where it is."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import time_path_helpers as H  # noqa: E402

DEV = "cuda"
GUARD = 64
NAN = float("nan")
FWD_KEYS = ("aux", "pre", "emb", "t1", "t2", "t3")
GRAD_KEYS = ("w1", "b1", "w2", "b2", "pw0", "pb0", "pw1", "pb1", "pw2", "pb2")
PROJ_KEYS = ("pw0", "pb0", "pw1", "pb1", "pw2", "pb2")


@pytest.fixture(scope="module")
def tdx():
    import tiny_diffusion_amd._lib as L

    assert torch.cuda.is_available()
    return L


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def guarded(shape, fill=NAN):
    """(buffer, view): a tensor of `shape` filled with `fill`, GUARD more elements behind it."""
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), fill, device=DEV)
    return buf, buf[:n].view(shape)


def guards_ok(bufs):
    return all(bool(torch.isnan(b[-GUARD:]).all()) for b in bufs)


def all_nan(t):
    return bool(torch.isnan(t).all())


def ptab(d, src=None):
    """A TDX_P_COUNT table of device pointers with the slots of the time path filled from `src` (default: d)."""
    tab = (C.c_void_p * H.SLOT_COUNT)()
    for k, s in H.SLOT.items():
        v = (src or d).get(k)
        tab[s] = None if v is None else v.data_ptr()
    return tab


def run_fwd(tdx, kind, td, d, B, cond="own", size_td=None):
    """tdx_time_path_fwd into NaN-filled guarded buffers (sized for the width size_td, default td) ->
    (status, {name: view}, [buffers])."""
    sz = td if size_td is None else size_td
    shapes = {"aux": (B,) if kind == 0 else (B, sz), "pre": (B, sz), "emb": (B, sz)}
    shapes.update({f"t{k + 1}": (B, w) for k, w in enumerate(H.PROJ[kind])})
    g = {k: guarded(s) for k, s in shapes.items()}
    c = (d["y"] if kind == 0 else d["cond"]) if cond == "own" else cond
    rc = tdx.lib.tdx_time_path_fwd(kind, td, ptr(d["t"]), ptr(c), ptab(d), *[g[k][1].data_ptr() for k in FWD_KEYS], B,
                                   stream())
    torch.cuda.synchronize()
    return rc, {k: v[1] for k, v in g.items()}, [v[0] for v in g.values()]


def grad_buffers(kind, td, d, B):
    g = {k: guarded(tuple(d[k].shape)) for k in GRAD_KEYS}
    if d["E"] is not None:
        g["E"] = guarded(tuple(d["E"].shape))
    g["scratch"] = guarded((3, B, td))
    return g


def run_bwd(tdx, kind, td, d, B, fwd, parts=7, g=None):
    """tdx_time_path_bwd -> (status, {name: view} with the scratch blocks as g_emb | h | g_h, [buffers])."""
    g = g or grad_buffers(kind, td, d, B)
    views = {k: v[1] for k, v in g.items()}
    rc = tdx.lib.tdx_time_path_bwd(kind, td, parts, ptr(d["y"]), ptab(d), ptab(d, views), ptr(fwd["aux"]),
                                   ptr(fwd["pre"]), ptr(fwd["emb"]), ptr(d["g0"]), ptr(d["g1"]), ptr(d["g2"]),
                                   views["scratch"].data_ptr(), B, H.NUM_CLASSES if d["y"] is not None else 0, stream())
    torch.cuda.synchronize()
    s = views.pop("scratch")
    views.update(g_emb=s[0], h=s[1], g_h=s[2])
    return rc, views, [v[0] for v in g.values()]


def show(what, case, ratios):
    print(what, H.case_id(case), {k: round(v, 3) for k, v in ratios.items()})


# ------------------------------------------------------------------------------------------------ every case, per element
@pytest.mark.parametrize("case", H.CASES, ids=H.case_id)
def test_time_path_fwd_bwd_per_element(tdx, case):
    """Forward (aux, pre, emb, t1..3) and backward (every gradient and the scratch blocks g_emb | h | g_h), each stage
    against fp64 from the operands its kernel read.  A null label's row of emb is the unconditional row bit for bit,
    absent classes and null labels leave exact zeros in dE, a second call on the same operands gives the same bits,
    and at kind 0 width 256 tdx_time_mlp_fwd / _bwd give the bits of the new entries."""
    kind, td, B, lab = case
    d = H.make_operands(kind, td, B, lab, device=DEV)
    rc, fwd, fbufs = run_fwd(tdx, kind, td, d, B)
    assert rc == 0 and guards_ok(fbufs)
    rc, bwd, bbufs = run_bwd(tdx, kind, td, d, B, fwd)
    assert rc == 0 and guards_ok(bbufs)
    r = dict(fwd, **bwd)
    ratios = H.stage_ratios(kind, d, r)
    show("time path", case, ratios)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    if kind == 1 and td % 2:
        assert bool((fwd["aux"][:, -1] == 0).all())
    if d["y"] is not None:
        y = d["y"]
        absent = sorted(set(range(H.NUM_CLASSES)) - set(y.tolist()))
        assert len(absent) >= 2 and bool((bwd["E"][absent] == 0).all())
        if lab == "null":
            rc, un, _ = run_fwd(tdx, kind, td, d, B, cond=None)
            assert rc == 0 and int((y < 0).sum()) == 2
            assert torch.equal(fwd["emb"][y < 0], un["emb"][y < 0]) and torch.equal(fwd["pre"], un["pre"])
            assert not torch.equal(fwd["emb"][y >= 0], un["emb"][y >= 0])
    rc, again, _ = run_bwd(tdx, kind, td, d, B, fwd)
    assert rc == 0 and all(torch.equal(again[k], bwd[k]) for k in bwd), "the backward is not reproducible"
    if kind == 0 and td == H.FUSED_TD:
        out = {k: guarded(tuple(fwd[k].shape))[1] for k in FWD_KEYS[1:]}
        assert tdx.lib.tdx_time_mlp_fwd(ptr(d["t"]), ptr(d["y"]), ptab(d), *[out[k].data_ptr() for k in FWD_KEYS[1:]], B,
                                        stream()) == 0
        torch.cuda.synchronize()
        assert all(torch.equal(out[k], fwd[k]) for k in out)
        g = {k: torch.full_like(v, NAN) for k, v in bwd.items() if k not in ("g_emb", "h", "g_h")}
        scratch = torch.full(((3 * td + 1) * B,), NAN, device=DEV)
        assert tdx.lib.tdx_time_mlp_bwd(ptr(d["t"]), ptr(d["y"]), ptab(d), ptab(d, g), ptr(fwd["pre"]), ptr(fwd["emb"]),
                                        ptr(d["g0"]), ptr(d["g1"]), ptr(d["g2"]), scratch.data_ptr(), B,
                                        H.NUM_CLASSES if d["y"] is not None else 0, stream()) == 0
        torch.cuda.synchronize()
        assert all(torch.equal(g[k], bwd[k]) for k in g)
        assert torch.equal(scratch[:3 * B * td].view(3, B, td), torch.stack([bwd["g_emb"], bwd["h"], bwd["g_h"]]))


# ------------------------------------------------------------------------------------------------ the parts protocol
@pytest.mark.parametrize("case", H.PARTS_CASES, ids=H.case_id)
def test_parts_write_their_own_outputs_and_the_step_order_is_the_one_call_backward(tdx, case):
    """TDX_TIME_PROJ writes the six projection gradients and g_emb, TDX_TIME_MID the middle, TDX_TIME_L1 dW1 and db1
    (kind 0; for kind 1 the first layer belongs to the middle) - every other buffer keeps its NaN.  The training step's
    order proj_bwd(0), (1), (2), MID, L1 equals the single all-parts call bit for bit on every output; after
    proj_bwd(0) alone g_emb is the first projection's term (overwritten, not accumulated into the NaN)."""
    kind, td, B, lab = case
    d = H.make_operands(kind, td, B, lab, device=DEV)
    rc, fwd, _ = run_fwd(tdx, kind, td, d, B)
    assert rc == 0
    rc, full, _ = run_bwd(tdx, kind, td, d, B, fwd)
    assert rc == 0
    mid = {"w2", "b2", "h", "g_h"} | ({"E"} if "E" in full else set()) | ({"w1", "b1"} if kind == 1 else set())
    own = {H.PART_PROJ: set(PROJ_KEYS) | {"g_emb"}, H.PART_MID: mid,
           H.PART_L1: {"w1", "b1"} if kind == 0 else set()}
    for part, keys in own.items():
        g = grad_buffers(kind, td, d, B)
        if part != H.PART_PROJ:          # the later parts read what the earlier ones left in the scratch
            g["scratch"][1][0].copy_(full["g_emb"])
            g["scratch"][1][2].copy_(full["g_h"])
        rc, got, bufs = run_bwd(tdx, kind, td, d, B, fwd, parts=part, g=g)
        assert rc == 0 and guards_ok(bufs)
        for k in full:
            if k in keys:
                assert torch.equal(got[k], full[k]), (part, k)
            elif not (part != H.PART_PROJ and k in ("g_emb", "g_h")):
                assert all_nan(got[k]), (part, k)
    # the step's order
    g = grad_buffers(kind, td, d, B)
    views = {k: v[1] for k, v in g.items()}
    for k in range(3):
        assert tdx.lib.tdx_time_path_proj_bwd(kind, td, k, ptab(d), ptab(d, views), ptr(fwd["emb"]), ptr(d[f"g{k}"]),
                                              views["scratch"].data_ptr(), B, stream()) == 0
        torch.cuda.synchronize()
        ref, bound = H.gemb_ref(kind, d, upto=k + 1)
        assert H.elem_ratio(views["scratch"][0], ref, bound) <= 1.0, k
        assert all_nan(views["scratch"][1:]) and all_nan(views["w2"]) and all_nan(views["w1"])
        for j in range(3):
            assert all_nan(views[f"pw{j}"]) == (j > k) and all_nan(views[f"pb{j}"]) == (j > k)
    for part in (H.PART_MID, H.PART_L1)[:2 if kind == 0 else 1]:
        rc, got, bufs = run_bwd(tdx, kind, td, d, B, fwd, parts=part, g=g)
        assert rc == 0 and guards_ok(bufs)
    for k in full:
        assert torch.equal(got[k], full[k]), k


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_widths_and_arguments_write_nothing(tdx):
    """Widths outside td_ok: TDX_E_SHAPE; a null pointer, batch <= 0, a bad `parts` or k, labels without num_classes, a
    float4-read operand off its 16-byte boundary at a row-kernel width: TDX_E_BADARG - before any launch, every buffer
    keeps its NaN.  The buffers are sized for the refused width all the same."""
    for kind, td in H.REFUSED:
        B, tdb = 2, max(td, 4)
        d = H.make_operands(kind, tdb, B, "labels" if kind == 0 else "text", seed=1, device=DEV)
        rc, fwd, fbufs = run_fwd(tdx, kind, td, d, B, size_td=tdb)
        assert rc == H.TDX_E_SHAPE and all(all_nan(b) for b in fbufs), (kind, td)
        good = fwd
        rc, _, bbufs = run_bwd(tdx, kind, td, d, B, good, g=grad_buffers(kind, tdb, d, B))
        assert rc == H.TDX_E_SHAPE and all(all_nan(b) for b in bbufs), (kind, td)
        g = grad_buffers(kind, tdb, d, B)
        views = {k: v[1] for k, v in g.items()}
        rc = tdx.lib.tdx_time_path_proj_bwd(kind, td, 0, ptab(d), ptab(d, views), ptr(good["emb"]), ptr(d["g0"]),
                                            views["scratch"].data_ptr(), B, stream())
        torch.cuda.synchronize()
        assert rc == H.TDX_E_SHAPE and all(all_nan(v[0]) for v in g.values())
    for kind, lab in ((0, "labels"), (1, "text")):
        td, B = 256, 3
        d = H.make_operands(kind, td, B, lab, device=DEV)
        rc, fwd, _ = run_fwd(tdx, kind, td, d, B)
        assert rc == 0
        for bad in ("t", "w2", "pb2"):
            rc, _, bufs = run_fwd(tdx, kind, td, dict(d, **{bad: None}), B)
            assert rc == H.TDX_E_BADARG and all(all_nan(b) for b in bufs), bad
        # batch <= 0, an unknown kind
        outs = {k: guarded(tuple(fwd[k].shape)) for k in FWD_KEYS}
        c = d["y"] if kind == 0 else d["cond"]
        for k_, b_ in ((kind, 0), (kind, -3), (2, B), (-1, B)):
            rc = tdx.lib.tdx_time_path_fwd(k_, td, ptr(d["t"]), ptr(c), ptab(d), *[outs[k][1].data_ptr() for k in FWD_KEYS],
                                           b_, stream())
            torch.cuda.synchronize()
            assert rc == H.TDX_E_BADARG and all(all_nan(v[0]) for v in outs.values())
        if kind == 1:   # the text rows are not optional
            rc, _, bufs = run_fwd(tdx, kind, td, d, B, cond=None)
            assert rc == H.TDX_E_BADARG and all(all_nan(b) for b in bufs)
        # off a 16-byte boundary: pre, emb (both kinds), the weight rows
        for k in ("pre", "emb"):
            arg = {q: outs[q][1].data_ptr() for q in FWD_KEYS}
            shifted = torch.full((B * td + 1 + GUARD,), NAN, device=DEV)
            arg[k] = shifted.data_ptr() + 4
            rc = tdx.lib.tdx_time_path_fwd(kind, td, ptr(d["t"]), ptr(c), ptab(d), *[arg[q] for q in FWD_KEYS], B, stream())
            torch.cuda.synchronize()
            assert rc == H.TDX_E_BADARG and all_nan(shifted) and all(all_nan(v[0]) for v in outs.values()), k
        w = torch.zeros(td * td + 1, device=DEV)
        rc, _, bufs = run_fwd(tdx, kind, td, dict(d, w2=w[1:].view(td, td)), B)
        assert rc == H.TDX_E_BADARG and all(all_nan(b) for b in bufs)
        # the same at a width of the generic kernels is served: they read scalars
        d2 = H.make_operands(kind, 100, B, lab, device=DEV)
        w = torch.zeros(100 * 100 + 1, device=DEV)
        w[1:].copy_(d2["w2"].flatten())
        rc, f2, _ = run_fwd(tdx, kind, 100, dict(d2, w2=w[1:].view(100, 100)), B)
        rc0, f0, _ = run_fwd(tdx, kind, 100, d2, B)
        assert rc == 0 and rc0 == 0 and torch.equal(f2["emb"], f0["emb"])
        # backward: parts, k, labels without a class count, a null gradient table entry
        for parts in (0, 8, -1, 15):
            rc, _, bufs = run_bwd(tdx, kind, td, d, B, fwd, parts=parts)
            assert rc == H.TDX_E_BADARG and all(all_nan(b) for b in bufs), parts
        g = grad_buffers(kind, td, d, B)
        views = {k: v[1] for k, v in g.items()}
        for k in (-1, 3):
            rc = tdx.lib.tdx_time_path_proj_bwd(kind, td, k, ptab(d), ptab(d, views), ptr(fwd["emb"]), ptr(d["g0"]),
                                                views["scratch"].data_ptr(), B, stream())
            torch.cuda.synchronize()
            assert rc == H.TDX_E_BADARG and all(all_nan(v[0]) for v in g.values())
        rc = tdx.lib.tdx_time_path_bwd(kind, td, 7, ptr(d["y"]), ptab(d), ptab(d, dict(views, w2=None)), ptr(fwd["aux"]),
                                       ptr(fwd["pre"]), ptr(fwd["emb"]), ptr(d["g0"]), ptr(d["g1"]), ptr(d["g2"]),
                                       views["scratch"].data_ptr(), B, H.NUM_CLASSES, stream())
        torch.cuda.synchronize()
        assert rc == H.TDX_E_BADARG and all(all_nan(v[0]) for v in g.values())
        if kind == 0:
            rc = tdx.lib.tdx_time_path_bwd(kind, td, 7, ptr(d["y"]), ptab(d), ptab(d, views), ptr(fwd["aux"]),
                                           ptr(fwd["pre"]), ptr(fwd["emb"]), ptr(d["g0"]), ptr(d["g1"]), ptr(d["g2"]),
                                           views["scratch"].data_ptr(), B, 0, stream())
            torch.cuda.synchronize()
            assert rc == H.TDX_E_BADARG and all(all_nan(v[0]) for v in g.values())


# ------------------------------------------------------------------------------------------------ extremes
@pytest.mark.parametrize("kind,td,B,lab", [(0, 256, 5, "labels"), (0, 100, 5, "labels"), (1, 256, 5, "text"),
                                           (1, 100, 5, "text")])
def test_pre_activations_at_the_edges_of_expf(tdx, kind, td, B, lab):
    """Pre-activations planted at +-88, +-104, +-999 (and +-87.5, where the sigmoid is denormal): the edges of expf in
    SiLU and SiLU'.  Every output is finite and within its bound (whose underflow term is what admits a flushed
    SiLU' there)."""
    d = H.make_operands(kind, td, B, lab, seed=H.case_seed(kind, td, 88), device=DEV)
    rc, fwd, _ = run_fwd(tdx, kind, td, d, B)
    assert rc == 0
    n = H.plant_extremes(kind, d, fwd["aux"])
    rc, fwd, fbufs = run_fwd(tdx, kind, td, d, B)
    assert rc == 0 and guards_ok(fbufs)
    want = torch.tensor(H.EXTREMES[:n], device=DEV)
    assert bool(((fwd["pre"][0, :n] - want).abs() <= 1e-3 * want.abs()).all()), fwd["pre"][0, :n]
    rc, bwd, bbufs = run_bwd(tdx, kind, td, d, B, fwd)
    assert rc == 0 and guards_ok(bbufs)
    r = dict(fwd, **bwd)
    assert all(bool(torch.isfinite(v).all()) for v in r.values())
    ratios = H.stage_ratios(kind, d, r)
    show("extremes", (kind, td, B, lab), ratios)
    assert all(v <= 1.0 for v in ratios.values()), ratios


# ------------------------------------------------------------------------------------------------ sampling tables
def _module(kind, td, labelled):
    from oracle.weights import make_state_dict, make_state_dict_laion

    if kind == 1:
        from tiny_diffusion_amd.conditional_diffusion_laion import NoiseModel
        sd = make_state_dict_laion(6, time_dim=td)
    elif labelled:
        from tiny_diffusion_amd.conditional_diffusion import NoiseModel
        sd = make_state_dict(6, True, time_dim=td)
    else:
        from tiny_diffusion_amd.diffusion import NoiseModel
        sd = make_state_dict(6, False, time_dim=td)
    m = NoiseModel(time_dim=td)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval(), sd


def _operands_of(m, kind, cond):
    """The helper's operand dictionary from a module's own fp32 parameters."""
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    mlp = "time_mlp" if kind == 1 else "time_embedding"
    d = {"w1": sd[f"{mlp}.0.weight"], "b1": sd[f"{mlp}.0.bias"], "w2": sd[f"{mlp}.2.weight"], "b2": sd[f"{mlp}.2.bias"],
         "E": sd.get("class_embedding.weight"), "y": None, "cond": None}
    for k in range(3):
        d[f"pw{k}"] = sd[f"time_proj{k + 1}.weight"].flatten(1).contiguous()
        d[f"pb{k}"] = sd[f"time_proj{k + 1}.bias"]
    if kind == 1:
        d["cond"] = cond
    elif cond is not None:
        d["y"] = cond
    return d


@pytest.mark.parametrize("case", H.TABLE_CASES, ids=H.case_id)
def test_sampling_tables_per_element(tdx, case):
    """After one table-mode reverse step the workspace's t_k rows are tab_k[t] + tabc_k[b] = W_k (MLP(t) + c_b) + b_k
    in fp64 within the bound of the two-term form (time_path_helpers.table_rows_ref), at an odd T = 7 with the counter
    inside the table, at T and at -1 (rows T - 1 and 0), and along a 5-step tau schedule whose rows are built at tau[k]
    (t_vec = tau[k], t_idx = k).  A null label's conditioning row is exactly 0: its t_k equal the unlabelled sample's
    table row bit for bit.  After _drop_sampling_tables the same step's t_k are the bits tdx_time_path_fwd writes for
    the same operands.  The reverse update reads its coefficient row at the raw counter, so the coefficient table here
    sits inside a buffer with a row of padding on either side."""
    from tiny_diffusion_amd.schedule import ForwardProcess, ddim_schedule

    kind, td, B, lab = case
    knob = C.c_int(-1)
    assert tdx.lib.tdx_tune_get(b"sample_tables", C.byref(knob)) == 0 and knob.value == 1
    m, _ = _module(kind, td, lab != "none")
    g = torch.Generator().manual_seed(H.case_seed(*case[:3]))
    shape = (4, 32, 32) if kind == 1 else (1, 28, 28)
    x0 = torch.randn(B, *shape, generator=g).cuda()
    cond = torch.randn(B, td, generator=g).cuda() if kind == 1 else \
        torch.tensor([3, -1, 3], device=DEV) if lab == "null" else None
    d = _operands_of(m, kind, cond)
    plan = lambda: [p for key, p in m._plans.items() if key[1] == B][0]   # noqa: E731
    t_idx = torch.empty(1, dtype=torch.int32, device=DEV)
    t_vec = torch.empty(B, dtype=torch.int64, device=DEV)
    eps = torch.empty_like(x0)

    def step(counter_value, coef, **kw):
        counter = torch.tensor([counter_value], dtype=torch.int64, device=DEV)
        with torch.no_grad():
            m._run_eval_step(x0.clone(), cond, coef, counter, t_idx, t_vec, eps, philox_seed=3, **kw)
        torch.cuda.synchronize()
        return [plan().tensor(f"t{k + 1}").clone().view(B, -1) for k in range(3)], int(counter)

    def check(got, t_rows, what):
        ratios = {}
        for k in range(3):
            ref, bound = H.table_rows_ref(kind, d, t_rows, k)
            ratios[f"t{k + 1}"] = H.elem_ratio(got[k], ref, bound)
        show(f"tables {what}", case, ratios)
        assert all(v <= 1.0 for v in ratios.values()), (what, ratios)

    def direct(t_rows):
        dd = dict(d, t=t_rows)
        rc, fwd, _ = run_fwd(tdx, kind, td, dd, B)
        assert rc == 0
        return [fwd[f"t{k + 1}"] for k in range(3)]

    T = 7
    real = ForwardProcess(num_timesteps=T).tables(DEV)[2]
    padded = torch.zeros(T + 2, real.shape[1], device=DEV)
    padded[1:T + 1] = real
    coef = padded[1:T + 1]
    step(T - 1, coef)                                    # builds the INFER pack
    m._prepare_sampling(x0, cond, T)
    tabled = {}
    for c, row in ((4, 4), (T, T - 1), (-1, 0), (0, 0), (T - 1, T - 1)):
        got, after = step(c, coef)
        assert after == c - 1 and int(t_idx) == c and t_vec.tolist() == [c] * B
        check(got, torch.full((B,), row, device=DEV), f"counter {c}")
        tabled[c] = got
        if lab == "null":     # row 1 carries the null label: the table row alone
            assert all(not torch.equal(got[k][0], got[k][1]) and torch.equal(got[k][0], got[k][2]) for k in range(3))
    m._drop_sampling_tables(x0)
    got, _ = step(4, coef)
    want = direct(torch.full((B,), 4, device=DEV))
    assert all(torch.equal(got[k], want[k]) for k in range(3))
    if lab != "none":
        assert any(not torch.equal(got[k], tabled[4][k]) for k in range(3))   # the tables did split the sum
    else:
        assert all(torch.equal(got[k], tabled[4][k]) for k in range(3))       # no conditioning row: the same sum
    if lab == "null":        # tabc of the null label is exactly 0: its rows are the bits of the label-free direct path
        dd = dict(d, t=torch.full((B,), 4, device=DEV), y=None)
        rc, fwd, _ = run_fwd(tdx, kind, td, dd, B)
        assert rc == 0
        assert all(torch.equal(tabled[4][k][1], fwd[f"t{k + 1}"][1]) for k in range(3))
    # a tau schedule of 5 steps
    sched = ddim_schedule(ForwardProcess(), timesteps=[0, 3, 333, 600, 999], eta=0.5)
    tau, coef5 = sched.device_tables(DEV)
    S = 5
    step(S - 1, coef5, tau=tau, S=S)
    m._prepare_sampling(x0, cond, S, tau=tau)
    for k in (4, 2, 0):
        got, after = step(k, coef5, tau=tau, S=S)
        tk = int(sched.timesteps[k])
        assert after == k - 1 and int(t_idx) == k and t_vec.tolist() == [tk] * B
        check(got, torch.full((B,), tk, device=DEV), f"tau[{k}] = {tk}")
    m._drop_sampling_tables(x0)
    got, _ = step(2, coef5, tau=tau, S=S)
    want = direct(torch.full((B,), int(sched.timesteps[2]), device=DEV))
    assert all(torch.equal(got[k], want[k]) for k in range(3))


# ------------------------------------------------------------------------------------------------ the whole network
def _time_params(grads):
    return {k: v for k, v in grads.items() if k.split(".")[0] in ("time_embedding", "time_mlp", "class_embedding",
                                                                   "time_proj1", "time_proj2", "time_proj3")}


def test_network_time_path_gradients_at_width_512():
    """One train-mode forward + backward through the class-conditional NoiseModel(time_dim=512), B = 5: the wiring of
    the path in csrc/unet.hip (label copy, scratch sizing, the parts issued on the side stream) at a row-kernel width
    with B % 4 != 0.  The gradients of the time-path parameters against the fp64 oracle within 10 x the fp32 oracle's
    own distance (parity_helpers.grad_precision_failures)."""
    from oracle import ref_cpu as R
    from parity_helpers import gpu_pool_routing, gpu_relu_masks, grad_precision_failures

    td, B = 512, 5
    m, sd = _module(0, td, True)
    m.train()
    g = torch.Generator().manual_seed(51)
    x = torch.randn(B, 1, 28, 28, generator=g)
    noise = torch.randn(B, 1, 28, 28, generator=g)
    t = torch.tensor([999, 0, 500, 17, 998])
    y = torch.tensor([3, 3, 0, 9, 1])
    F.mse_loss(m(x.cuda(), t.cuda(), y.cuda()), noise.cuda()).backward()
    args = (sd, x, t, noise, y)
    pidx = gpu_pool_routing(m, B, args, True)
    masks, _ = gpu_relu_masks(m, B, args, True, pool_idx=pidx)
    kw = dict(training=True, pool_idx=pidx, relu_masks=masks)
    _, _, g32, _ = R.train_step_grads(*args, **kw)
    _, _, g64, _ = R.train_step_grads(*args, dtype=torch.float64, **kw)
    got = _time_params({k: p.grad for k, p in m.named_parameters()})
    assert len(got) == 11
    bad = grad_precision_failures(got, g32, g64, True, log=True)
    assert not bad, bad


def test_laion_network_time_path_gradients_at_width_100():
    """The same through the LAION network at time_dim = 100 (generic kernels), B = 2, 32 x 32.  The oracle is given the
    GPU run's max-pool routing and ReLU active sets, each after its tie check: at B = 2 the per-sample offsets t_k sit
    in front of a train-mode BatchNorm that removes their mean, so one near-tied ReLU decided the other way moves the
    gradients of time_proj2 / 3 by several 1e-4 of their norm."""
    from oracle import ref_cpu as R
    from oracle import ref_laion as RL
    from test_gpu_laion import _gpu_pool_routing
    from parity_helpers import UNIT_BN, check_relu_ties, grad_precision_failures

    td, B = 100, 2
    m, sd = _module(1, td, True)
    m.train()
    g = torch.Generator().manual_seed(52)
    x = torch.randn(B, 4, 32, 32, generator=g)
    noise = torch.randn(B, 4, 32, 32, generator=g)
    t = torch.tensor([999, 0])
    cond = torch.randn(B, td, generator=g)
    F.mse_loss(m(x.cuda(), t.cuda(), cond.cuda()), noise.cuda()).backward()
    pidx = _gpu_pool_routing(m, B, sd, x, t, cond)
    # the GPU run's ReLU active sets too (one ReLU input within rounding of 0 decided the other way moves these
    # gradients by more than the gate), after the tie check of parity_helpers.check_relu_ties
    plan = [pl for key, pl in m._plans.items() if key[1] == B][0]
    shapes = [(32, 64), (32, 64), (16, 128), (16, 128), (8, 256), (8, 256), (4, 256), (8, 256), (8, 256), (16, 128),
              (16, 128), (32, 64), (32, 64)]
    masks = {}
    for u, (name, (hw, Cc)) in enumerate(zip(UNIT_BN, shapes)):
        Y, ss = plan.tensor(f"Y{u}").view(B, hw, hw, Cc), plan.tensor(f"ss{u}")
        masks[name] = (torch.addcmul(ss[Cc:2 * Cc], Y, ss[:Cc]).permute(0, 3, 1, 2) > 0).cpu()
    p64, b64 = R.split_state(sd)
    p64 = {k: v.double() for k, v in p64.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in b64.items()}
    taps = {}
    with torch.no_grad():
        RL.unet_forward(p64, b64, x.double(), t, cond.double(), training=True, taps=taps, pool_idx=pidx, relu_masks=masks)
    print("ReLU sets differing from the exact ones:", check_relu_ties(masks, taps))
    kw = dict(pool_idx=pidx, relu_masks=masks)
    _, _, g32, _ = RL.train_step_grads(sd, x, t, noise, cond, **kw)
    _, _, g64, _ = RL.train_step_grads(sd, x, t, noise, cond, dtype=torch.float64, **kw)
    got = _time_params({k: p.grad for k, p in m.named_parameters()})
    assert len(got) == 10
    bad = grad_precision_failures(got, g32, g64, True, log=True)
    assert not bad, bad
