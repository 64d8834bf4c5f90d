"""CPU checks of tests/time_path_helpers.py: the stage references chained in fp64 against torch
autograd over the composed path, the CPU-fp32 restatement of every case of tests/test_gpu_time_path_dispatch.py under
every bound, the input builders, and the host model of the dispatch of csrc/time_embed.hip - which branch each of those
cases is there to reach."""
import os
import re

import pytest
import torch

import time_path_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


AUTOGRAD_CASES = [(0, 256, 37, "none"), (0, 256, 37, "labels"), (0, 100, 5, "null"), (0, 33, 7, "null"),
                  (0, 1, 5, "labels"), (1, 5, 7, "text"), (1, 100, 5, "text"), (1, 768, 5, "text")]


@pytest.mark.parametrize("case", AUTOGRAD_CASES, ids=H.case_id)
def test_stage_references_compose_to_torch_autograd(case):
    """The stage references, each fed the previous one, are the composed path of the reference's modules: outputs and
    every gradient against torch autograd in fp64, both kinds, with and without labels and null labels."""
    kind, td, B, lab = case
    d = H.make_operands(kind, td, B, lab)
    outs, grads = H.composed_autograd(kind, d)
    r = H.chained_fp64(kind, d)
    for k, v in outs.items():
        assert _rel(r[k].reshape(v.shape), v) < 1e-12, k
    for k, g in grads.items():
        assert _rel(r[k].reshape(g.shape), g) < 1e-11, k
    if lab == "null":
        y = d["y"]
        assert (y < 0).sum() == 2 and -1 in y.tolist()
        un = H.chained_fp64(kind, dict(d, y=None))
        assert torch.equal(r["emb"][y < 0], un["emb"][y < 0])          # a null label's row is the unconditional row
        absent = sorted(set(range(H.NUM_CLASSES)) - set(y.tolist()))
        assert absent and bool((r["E"][absent] == 0).all())


@pytest.mark.parametrize("case", H.CASES, ids=H.case_id)
def test_fp32_restatement_is_within_every_bound(case):
    """Plain fp32 torch on the CPU, stage by stage, stays under every bound on every case of the GPU list (with room:
    the worst ratios are recorded in DESIGN.md 3.20), and the builders keep their promises."""
    kind, td, B, lab = case
    d = H.make_operands(kind, td, B, lab)
    t = d["t"].tolist()
    assert 999 in t and (B == 1 or 0 in t)
    if kind == 0:
        assert float(d["w1"].abs().max()) <= 1.0
    if d["y"] is not None and B > 1:
        y = d["y"].tolist()
        assert y[0] == y[1] and len(set(range(H.NUM_CLASSES)) - set(y)) >= 1
    ratios = H.stage_ratios(kind, d, H.restate_fp32(kind, d))
    print("fp32 restatement", case, {k: round(v, 3) for k, v in ratios.items()})
    assert all(v <= 1.0 for v in ratios.values()), ratios


def test_sinusoid_bound_is_exact_at_zero_and_matches_the_laion_gate():
    t = torch.tensor([0, 999, 1, 500])
    for td in (4, 5, 100, 768):
        ref, bound = H.sinusoid_ref(t, td)
        half = td // 2
        assert bool((bound[0] == 0).all()) and bool((ref[0, :half] == 0).all()) and bool((ref[0, half:2 * half] == 1).all())
        if td % 2:
            assert bool((ref[:, -1] == 0).all()) and bool((bound[:, -1] == 0).all())
        assert H.elem_ratio(H.sinusoid_fp32(t, td), ref, bound) <= 1.0
    assert 1.5e-4 <= float(H.sinusoid_ref(t, 768)[1][1].max()) <= 2e-4


def test_underflow_term_covers_flushed_silu_grad():
    """SiLU' of a pre-activation below -87.3 in fp32 against fp64: outside the relative bound, inside the underflow
    term."""
    x = torch.tensor([-87.5, -88.0, -88.8, -95.0, -104.0, -999.0])
    err = (H.dsilu(x).double() - H.dsilu(x.double())).abs()
    assert float(err.max()) <= H.underflow(1, x)
    err = (H.silu(x).double() - H.silu(x.double())).abs()
    assert float(err.max()) <= H.underflow(1, x)


@pytest.mark.parametrize("kind,td,lab", [(0, 256, "null"), (0, 100, "none"), (1, 100, "text"), (1, 768, "text")])
def test_table_reference_is_the_direct_reference(kind, td, lab):
    """table_rows_ref == the chained references at the same t, and its bound admits the fp32 restatement."""
    B = 3
    d = H.make_operands(kind, td, B, lab)
    d["t"] = torch.full((B,), 6)
    r, r32 = H.chained_fp64(kind, d), H.restate_fp32(kind, d)
    for k in range(3):
        ref, bound = H.table_rows_ref(kind, d, d["t"], k)
        assert _rel(ref, r[f"t{k + 1}"]) < 1e-12
        assert H.elem_ratio(r32[f"t{k + 1}"], ref, bound) <= 1.0


# ------------------------------------------------------------------------------------------------ host model
def test_constants_match_the_source():
    src = open(os.path.join(ROOT, "tiny_diffusion_amd", "csrc", "time_embed.hip")).read()
    assert "td % 256 == 0 && td <= 1024" in src and H.ROW_WIDTHS == (256, 512, 768, 1024)
    assert f"O % {H.ROW_OUT_BLOCK}" in src and f"constexpr int NB = {H.ROW_NB};" in src
    assert f"red[2][{H.L1_SLICES}][{H.L1_COLS}]" in src and f"n0 += {H.LABEL_TRIP}" in src
    assert f"td <= {H.TD_MAX}" in src and "kind == 1 ? 4 : 1" in src
    assert "min(n0 + s, B - 1)" in src
    hdr = open(os.path.join(ROOT, "include", "tdx.h")).read()
    enum = re.search(r"TDX_P_TE0_W = 0.*?TDX_P_COUNT", hdr, re.S).group(0)
    assert "TDX_P_UNIT0 + 13 * 4" in enum
    from tiny_diffusion_amd.unet import param_slot_names

    names = param_slot_names(True)
    assert len(names) == H.SLOT_COUNT
    for k, s in H.SLOT.items():
        assert names[s] == H.SLOT_NAMES[k], (k, s, names[s])


def test_dispatch_model():
    assert H.linear_kernel(256, 128, False) == "linear_rows_kernel<R=1,silu=0>"
    assert H.linear_kernel(512, 512, True) == "linear_rows_kernel<R=2,silu=1>"
    assert H.linear_kernel(1024, 64, False) == "linear_rows_kernel<R=4,silu=0>"
    assert H.linear_kernel(1280, 1280, True) == "linear_generic_kernel<silu=1>"
    assert H.linear_kernel(255, 128, False) == H.linear_kernel(4096, 128, False) == "linear_generic_kernel<silu=0>"
    assert "time_emb_kernel" in H.branch(0, 256, 5) and "time_l1_fwd_kernel" not in H.branch(0, 256, 5)
    assert "time_emb_kernel" not in H.branch(1, 256, 5, "text")
    assert not H.td_ok(0, 4097) and not H.td_ok(1, 3) and H.td_ok(0, 1) and H.td_ok(1, 4) and H.td_ok(0, 4096)
    for kind, td in H.REFUSED:
        assert not H.td_ok(kind, td)


def test_every_named_branch_is_reached_by_a_case():
    reached = {}
    for kind, td, B, lab in H.CASES:
        for b in H.branch(kind, td, B, lab):
            reached.setdefault(b, []).append((kind, td, B, lab))
    tables = set()
    for kind, td, B, lab in H.TABLE_CASES:
        tables |= H.branch_tables(kind, td, B, lab)
    need = [f"linear_rows_kernel<R={r},silu={s}>" for r in (1, 2, 3, 4) for s in (0, 1)] + [
        "linear_generic_kernel<silu=0>", "linear_generic_kernel<silu=1>", "generic:multiple_of_256", "generic:addend",
        "rows:clamped_sample", "rows:addend", "time_l1_fwd_kernel", "add_class_emb_kernel", "time_emb_kernel",
        "time_emb_kernel:null_label", "time_proj_kernel", "sinusoid_kernel:odd_zero_column",
        "class_emb_bwd_kernel:trips=1", "class_emb_bwd_kernel:trips=2", "class_emb_bwd_kernel:trips=3",
        "time_l1_bwd_kernel:ragged_last_workgroup", "time_l1_bwd_kernel:empty_slices", "silu_bwd_kernel"]
    need += [f"backward:kind0:td={td}" for td in (1, 33, 64, 100, 255, 256, 257, 512, 768, 1024, 1280, 4096)]
    need += [f"backward:kind1:td={td}" for td in (4, 5, 100, 256, 512, 768, 1024, 1280)]
    missing = [b for b in need if b not in reached]
    assert not missing, missing
    # kind 0 reaches the row kernels with SiLU at every R but 1 (width 256 is the fused kernel), kind 1 at every R
    for r in (2, 3, 4):
        assert any(c[0] == 0 for c in reached[f"linear_rows_kernel<R={r},silu=1>"])
    assert any(c[0] == 1 for c in reached["linear_generic_kernel<silu=0>"])
    assert any(c[0] == 1 and c[1] == 1280 for c in reached["generic:multiple_of_256"])
    # every B % 4, B below and across the 8 slices
    assert {c[2] % 4 for c in reached["rows:clamped_sample"]} == {1, 2, 3}
    assert {1, 2, 3, 5, 7, 8, 9, 37, 257, 600} <= {c[2] for c in H.CASES}
    assert all(B <= 3 for k, td, B, lab in H.CASES if td == 4096)
    for b in ("rows:null_bias", "generic:null_bias", "class_rows_kernel", "sample_head_kernel",
              "linear_rows_kernel<R=1,silu=0>", "linear_rows_kernel<R=2,silu=0>", "linear_rows_kernel<R=3,silu=0>"):
        assert b in tables, b
