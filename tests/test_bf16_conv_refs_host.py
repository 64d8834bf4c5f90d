"""CPU: the references, operands, gates and the dispatch model of tests/bf16_conv_helpers.py, before any kernel of
csrc/conv3x3_bf16.hip is held against them (tests/test_gpu_bf16_conv_dispatch.py).  The references agree with fp64
F.conv2d + autograd; the exactness premise and the undecided cap hold for every case of the GPU file; the model reaches
every instantiation of the DESIGN.md 3.26 table and its constants match the source; the gates reject six corruptions of
the reference.  Nothing here reads a kernel's output."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import bf16_conv_helpers as BC
import conv_helpers as CH
import io16_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    return open(os.path.join(ROOT, "tiny_diffusion_amd", "csrc", name)).read()


def _fwd_shapes():
    return sorted({BC.FWD_CASES[n][0] for n in BC.FWD_CASES})


def _wgrad_shapes():
    return sorted({s for s, _, _ in BC.wgrad_runs()})


def _fwd_in_bns(shape):
    return sorted({i for n in BC.FWD_CASES if BC.FWD_CASES[n][0] == shape for i in BC.FWD_CASES[n][3]})


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("regime", BC.REGIMES)
@pytest.mark.parametrize("in_bn", [0, 1])
def test_references_agree_with_conv2d_and_autograd(regime, in_bn):
    shape = (3, 5, 7, 64, 64)
    d = BC.operands(shape, regime)
    a = BC.staged(d, in_bn)
    if in_bn:   # one rounding of the fp32 fma; padding is 0 after the transform (conv2d pads the transformed tensor)
        fma64 = torch.relu(d["x"].double() * d["isc"].double() + d["ish"].double())   # exact product, one rounding each
        assert torch.equal(a, fma64.float().bfloat16().float())
        assert H.is16(a) and bool((a >= 0).all())
    an = a.double().permute(0, 3, 1, 2).requires_grad_(True)
    wr = d["wr"].double().requires_grad_(True)
    dy = d["dy"].double().permute(0, 3, 1, 2)
    y = F.conv2d(an, wr, d["b"].double(), padding=1)
    dw, dx = torch.autograd.grad(y, (wr, an), dy)
    nhwc = lambda t: t.permute(0, 2, 3, 1)   # noqa: E731
    fr, dr, wg = BC.fwd_refs(shape, regime, in_bn), BC.dgrad_refs(shape, regime), BC.wgrad_refs(shape, regime, in_bn)
    assert torch.allclose(fr["ref"], nhwc(y.detach()), rtol=1e-12, atol=1e-12)
    assert torch.allclose(wg["ref"], dw, rtol=1e-12, atol=1e-12)
    if not in_bn:
        assert torch.allclose(dr["ref"], nhwc(dx), rtol=1e-12, atol=1e-12)
    assert bool((fr["mag"] >= fr["ref"].abs()).all()) and bool((wg["mag"] >= wg["ref"].abs() - 1e-9).all())
    # statistics: the partials merge (Chan) to the batch mean and variance of conv + bias
    st = fr["stats"]
    flat = fr["ref"].reshape(-1, shape[4])
    mean, var = CH.merge_stats(torch.stack([st["sum"], st["m2"]], 1), st["sum"].shape[0], BC.STAT_ROWS, flat.shape[0])
    assert torch.allclose(mean, flat.mean(0), atol=1e-10) and torch.allclose(var, flat.var(0, unbiased=False), rtol=1e-10)


def test_pack_reference_layouts():
    w = torch.arange(2 * 3 * 9, dtype=torch.float32).reshape(2, 3, 3, 3)
    wf, wd = BC.pack_refs(w)
    for co in range(2):
        for ci in range(3):
            for tap in range(9):
                assert float(wf[co, tap, ci]) == float(w[co, ci, tap // 3, tap % 3])
                assert float(wd[ci, 8 - tap, co]) == float(w[co, ci, tap // 3, tap % 3])
    # the mirrored pack IS the forward pack of the input gradient's filter
    wg = w.flip(2, 3).transpose(0, 1)
    assert torch.equal(wd, BC.pack_refs(wg)[0])


# ------------------------------------------------------------------------------------------------ premises of the regimes
def test_exact_regime_every_sum_is_exact_in_fp32():
    """Operands are multiples of 1/2 (IN_BN: x scale + shift), the epilogue's scale makes multiples of 1/4: with
    4 x magnitude-sum < 2^24 every partial sum in any order is an fp32 value."""
    worst = 0.0
    for shape in _fwd_shapes():
        d = BC.operands(shape, "exact")
        assert bool((d["isc"].abs().log2().frac() == 0).all()) and bool((d["ish"] > 0).any()) and bool((d["osh"] > 0).any())
        for in_bn in _fwd_in_bns(shape):
            r = BC.fwd_refs(shape, "exact", in_bn)
            assert torch.equal(BC.staged(d, in_bn) * 2, (BC.staged(d, in_bn) * 2).round())
            assert torch.equal(r["ref"] * 2, (r["ref"] * 2).round()) and torch.equal(r["pre"] * 4, (r["pre"] * 4).round())
            worst = max(worst, float(r["mag"].max()), float(r["mag_inf"].max()))
            assert torch.equal(r["stats"]["sum"].float().double(), r["stats"]["sum"])
        worst = max(worst, float(BC.dgrad_refs(shape, "exact")["mag"].max()))
    for shape in _wgrad_shapes():
        for in_bn in (0, 1):
            r = BC.wgrad_refs(shape, "exact", in_bn)
            assert torch.equal(r["ref"] * 2, (r["ref"] * 2).round())
            worst = max(worst, float(r["mag"].max()))
    print(f"exact regime: largest magnitude-sum {worst:.0f}")
    assert 4 * worst < 2.0 ** 24


def test_rounding_regime_undecided_share_is_under_the_cap():
    """From the reference alone: the share of bf16 elements whose interval spans more than one bf16 value, for the
    forward, the inference epilogue and the input gradient of every case."""
    worst = {}
    for shape in _fwd_shapes():
        for in_bn in _fwd_in_bns(shape):
            r = BC.fwd_refs(shape, "rounding", in_bn)
            worst[("fwd", shape, in_bn)] = BC.undecided(r["ref"], r["b"])
            worst[("infer", shape, in_bn)] = BC.undecided(r["pre"], r["b_inf"], relu=True)
        g = BC.dgrad_refs(shape, "rounding")
        worst[("dgrad", shape, 0)] = BC.undecided(g["ref"], g["b"])
    for key, share in sorted(worst.items(), key=lambda kv: -kv[1])[:6]:
        print(f"undecided {100 * share:.2f} % {key}")
    assert max(worst.values()) <= H.UNDECIDED_CAP
    # sign-symmetric Gaussian operands would not do: the same bound decides far fewer elements
    gen = torch.Generator().manual_seed(0)
    x = H.r16(torch.randn(2, 8, 8, 1024, generator=gen))
    w = H.r16(torch.randn(64, 1024, 3, 3, generator=gen) * (2.0 / (9 * 1024)) ** 0.5)
    sym = H.undecided_share(CH.conv_ref64(x, w), BC.fp32_bound(CH.conv_ref64(x.abs(), w.abs()), 9 * 1024))
    assert sym > 4 * H.UNDECIDED_CAP


# ------------------------------------------------------------------------------------------------ host model
def test_constants_match_the_source():
    bf, cv, knobs = _src("conv3x3_bf16.hip"), _src("conv3x3.hip"), _src("knobs.h")
    assert f"#define THIN_WROWS {BC.THIN_WROWS}\n" in bf and "return worst <= THIN_WROWS;" in bf
    assert "worst = std::max(worst, slot_of(m0 + 255) - slot_of(m0) + 1 + 2 * (PW + 1));" in bf
    assert "const int m0 = 256 * j;" in bf and "if ((m0 + 256) % HW == 0) break;" in bf
    assert ("if (io16 && !(flags & TDX_CONV_IN_BNRELU) && a.M % 256 == 0 && thin_window_fits(H, W) &&\n"
            "      ((g_knobs.bf16_thin >= 1 && cout == 64) || (g_knobs.bf16_thin >= 2 && cin == 64) || "
            "g_knobs.bf16_thin >= 3)) {") in bf
    assert f"if (io16 && g_knobs.bf16_ring && a.M % {BC.RING_ROWS} == 0 && cin <= {BC.RING_MAX_CIN}) {{" in bf
    assert "return cout % 128 == 0 ? launch_bf16_ring<128>(a, flags, st) : launch_bf16_ring<64>(a, flags, st);" in bf
    assert "return io16 ? launch_bf16<128, 128, true>(a, flags, st) : launch_bf16<128, 128, false>(a, flags, st);" in bf
    assert "return io16 ? launch_bf16<128, 64, true>(a, flags, st) : launch_bf16<128, 64, false>(a, flags, st);" in bf
    assert (f"if (io16 && g_knobs.bf16_wgrad9 && W <= {BC.WGRAD9_MAX_W} && (H + 1) * (W + 1) >= {BC.WGRAD9_MIN_SLOTS}) "
            "return launch_wgrad9_bf16(a, splits, in_bn, st);") in bf
    assert "const int s8 = slot + 8 * PP;" in bf                      # the shift WGRAD9_MIN_SLOTS answers
    assert bf.count("const int HALOB = (PW + 1 + 63) / 64 * 64") == 2 and "NB = (HALOB + 64 + PW) / 64" in bf
    assert "const int NB = (HALOB + 64 + PW) / 64;" in bf
    assert "(g_knobs.bf16_wgrad_swz ? launch_wgrad_bf16s<BM_, BN_>(a, in_bn, st) : launch_wgrad_bf16<BM_, BN_, true>" in bf
    assert f"extern \"C\" int tdx_conv3x3_bf16_stat_tile_rows(void) {{ return {BC.STAT_ROWS}; }}" in bf
    for line in ("c.bm = (cout % 128 == 0) ? 128 : 64;", "c.bn = (cin % 128 == 0) ? 128 : 64;",
                 "int64_t tiles = (int64_t)(cout / c.bm) * (cin / c.bn) * 9;", "int64_t s = (target + tiles - 1) / tiles;",
                 "if (bf16 && g_knobs.wgrad9_wgs > 0) s = g_knobs.wgrad9_wgs / ((int64_t)(cout / 64) * (cin / 64));",
                 "int64_t smax = (M + 255) / 256;", "chunk = (chunk + 31) / 32 * 32;", "s = (M + chunk - 1) / chunk;"):
        assert line in cv, line
    for key, val in BC.KNOB_DEFAULTS.items():
        assert re.search(r"\bint %s = %d;" % (key, val), knobs), key


def test_dispatch_model_names_the_kernel_of_every_case():
    for name, (shape, knobs, io16s, in_bns, family) in BC.FWD_CASES.items():
        want = {"k128": "conv3x3_bf16_kernel<", "ring": "conv3x3_bf16_ring_kernel<", "thin": "conv3x3_bf16_thin_kernel<"}[family]
        for flags in BC.FLAGS:
            assert BC.fwd_kernel(shape, in_bns[-1] if family != "thin" else 0, flags, io16s[-1], knobs).startswith(want), name
    assert BC.thin_window_fits(2, 12) == (True, 448) and BC.thin_window_fits(2, 10) == (False, 449)
    assert all(BC.thin_window_fits(h, w)[0] for h, w in ((4, 4), (6, 6), (16, 16)))
    assert (64 * 6 * 6) % 256 == 0 and len({(256 * j) % 36 for j in range(9)}) == 9       # every phase of a sample
    assert all(BC.FWD_CASES[n][0][0] * BC.FWD_CASES[n][0][1] * BC.FWD_CASES[n][0][2] % 256 == 0
               for n in BC.FWD_CASES if n.startswith(("ring", "thin", "k128-m256")))
    assert BC.fwd_kernel((4, 8, 8, 1024, 64), 0, 0, 1, BC.RING).startswith("conv3x3_bf16_ring_kernel<64")
    assert BC.fwd_kernel((4, 8, 8, 1088, 64), 0, 0, 1, BC.RING) == BC.fwd_kernel((4, 8, 8, 1088, 64), 0, 0, 1, BC.RING_TWIN)
    assert BC.fwd_kernel((4, 8, 8, 64, 128), 0, 0, 1) == "conv3x3_bf16_thin_kernel<EPI_PLAIN>"    # what bf16_thin = 0 avoids
    # K-tiles, row tiles
    assert [9 * s[3] // 64 for s in ((3, 5, 7, 64, 64), (5, 5, 7, 128, 128), (2, 8, 8, 1024, 64))] == [9, 18, 144]
    assert -(-9 * 11 * 11 // 128) == 9 and -(-5 * 5 * 7 // 128) == 2 and 3 * 5 * 7 < 128
    # weight gradient
    for (shape, tile) in zip(BC.WGRAD_PAIRS, ("64, 64", "128, 128", "64, 128", "128, 64")):
        assert BC.wgrad_kernel(shape, 0, 0) == f"conv3x3_wgrad_bf16_kernel<{tile}, false, false>"
        assert BC.wgrad_kernel(shape, 1, 1, BC.WGRAD_KNOBS["per-tap"]) == f"conv3x3_wgrad_bf16s_kernel<{tile}, true>"
        assert BC.wgrad_kernel(shape, 1, 1, BC.WGRAD_KNOBS["round2"]) == f"conv3x3_wgrad_bf16_kernel<{tile}, true, true>"
        assert BC.wgrad_kernel(shape, 0, 1) == BC.wgrad_kernel(shape, 0, 1, BC.WGRAD_KNOBS["wgs256"]) \
            == "conv3x3_wgrad9_bf16_kernel<false>"
    assert BC.wgrad_plan(40, 64, 64)[2:] == (1, 64) and BC.wgrad_plan(9 * 121, 64, 64)[2:] == (5, 224)
    assert 9 * 121 % 224 != 0 and BC.wgrad_plan(5 * 441, 64, 64)[2] == 9
    assert BC.wgrad9_geometry(62) == (64, 2) and BC.wgrad9_geometry(63) == (128, 4) and BC.wgrad9_geometry(95) == (128, 4)
    assert BC.wgrad9_geometry(28) == (64, 2) and 64 / 25 == 2.56                              # 4x4: 25 slots per sample
    assert BC.wgrad_kernel((1, 2, 95, 64, 64), 0, 1).startswith("conv3x3_wgrad9")
    assert BC.wgrad_kernel((1, 2, 96, 64, 64), 0, 1) == "conv3x3_wgrad_bf16s_kernel<64, 64, false>"
    nine = [s for s in BC.WGRAD_TINY if BC.wgrad_kernel(s, 0, 1).startswith("conv3x3_wgrad9")]
    assert nine == [(30, 2, 2, 64, 64), (20, 1, 7, 64, 64), (9, 3, 3, 64, 64)]                 # the others: per-tap


def test_design_table_lists_every_instantiation_with_a_case_that_reaches_it():
    rows = BC.design_table()
    assert len(rows) == len(BC.all_instantiations()) == 65 and not any("NOT REACHED" in r for r in rows)
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 3.26 "):]
    for row in rows:
        assert row in sec, row
    # and the source launches nothing the list does not hold: every kernel template named in a launcher is one of these
    bf = _src("conv3x3_bf16.hip")
    launched = set(re.findall(r"auto kern = (conv3x3_\w+)<", bf))
    assert launched == {r.split("`")[1].split("<")[0] for r in rows}


# ------------------------------------------------------------------------------------------------ power of the gates
def _rejects(got, shape, regime, ref, b, mag, K, bf16, relu=False):
    g = got.float()
    return not BC.held(H.to16(g) if bf16 else g, regime, ref, b, mag, K, relu)[0]


def test_gates_accept_torch_fp32_and_reject_six_corruptions():
    shape = (3, 5, 7, 64, 64)
    B, Hh, W, cin, cout = shape
    verdict = {}
    for regime in BC.REGIMES:
        d = BC.operands(shape, regime)
        r0, r1 = BC.fwd_refs(shape, regime, 0), BC.fwd_refs(shape, regime, 1)
        wg = BC.wgrad_refs(shape, regime, 0)
        nchw = lambda t: t.permute(0, 3, 1, 2)   # noqa: E731
        # torch's own fp32 convolution of the same operands passes every gate, fp32 and rounded to bf16
        y32 = F.conv2d(nchw(d["x"]), d["wr"], d["b"], padding=1).permute(0, 2, 3, 1)
        for bf16 in (False, True):
            assert not _rejects(y32, shape, regime, r0["ref"], r0["b"], r0["mag"], r0["K"], bf16)
            inf32 = torch.relu(y32 * d["osc"] + d["osh"])
            assert not _rejects(inf32, shape, regime, r0["pre"], r0["b_inf"], r0["mag_inf"], r0["K"], bf16, relu=True)
        assert BC.stats_held(torch.stack([r0["stats"]["sum"], r0["stats"]["m2"]], 1).float(), r0["stats"], regime)[0]

        def note(name, rejected):
            verdict.setdefault(name, {})[regime] = bool(rejected)

        # 1. one tap dropped at one border pixel: pixel (0, 0, 0) without its right neighbour (tap kh = 1, kw = 2)
        y = r0["ref"].clone()
        y[0, 0, 0] -= d["wr"][:, :, 1, 2].double() @ d["x"][0, 0, 1].double()
        note("tap", _rejects(y, shape, regime, r0["ref"], r0["b"], r0["mag"], r0["K"], False))
        # 2. H and W exchanged
        y = CH.exchanged(lambda t: CH.conv_ref64(t, d["wr"], d["b"]), d["x"])
        note("exchanged", _rejects(y, shape, regime, r0["ref"], r0["b"], r0["mag"], r0["K"], False))
        # 3. padding left at relu(shift): the transform applied to the padded tensor
        xp = F.pad(nchw(d["x"]), (1, 1, 1, 1))
        ap = H.r16(torch.relu(xp * d["isc"].view(1, -1, 1, 1) + d["ish"].view(1, -1, 1, 1)))
        y = F.conv2d(ap.double(), d["wr"].double(), d["b"].double()).permute(0, 2, 3, 1)
        note("padding", _rejects(y, shape, regime, r1["ref"], r1["b"], r1["mag"], r1["K"], False))
        # 4. one pixel missing from one slab of dw
        dy = d["dy"].clone()
        dy[1, 2, 3] = 0
        note("pixel", _rejects(CH.wgrad_ref64(d["x"], dy), shape, regime, wg["ref"], None, wg["mag"], wg["K"], False))
        # 5. truncation instead of nearest-even in the bf16 store
        t = H.trunc16(r0["ref"].float())
        note("trunc16", not BC.held(H.to16(t), regime, r0["ref"], r0["b"], r0["mag"], r0["K"])[0])
        # 6. statistics taken from the rounded output
        st16 = BC.tile_stats(H.r16(r0["ref"].float()).double().reshape(-1, cout))
        note("stats", not BC.stats_held(torch.stack([st16["sum"], st16["m2"]], 1).float(), r0["stats"], regime)[0])
    print(verdict)
    assert set(verdict) == {"tap", "exchanged", "padding", "pixel", "trunc16", "stats"}
    assert all(any(v.values()) for v in verdict.values()), verdict
    # each regime is needed for something, and the exact regime alone sees the geometry
    assert all(verdict[k]["exact"] for k in ("tap", "exchanged", "padding", "pixel"))
    assert verdict["trunc16"]["rounding"]
