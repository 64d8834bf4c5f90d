"""CPU-only guard on the Winograd main loops' instruction mix (tools/wino_loop_census.py compiles conv3x3_wino.hip for
gfx950 and counts one K-stage of each loop).  The row-split forward / input-gradient loops build two transform rows per
wave: at most 64 v_add/sub_f32 and 72 non-MFMA VALU per 64 MFMAs (the fp32 MFMA shares the vector pipe, so every
extra add costs), and no kernel of the file may spill to scratch."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROWS = ("conv3x3_wino_kernel<1,false,true> (fwd, row split)", "conv3x3_wino_kernel<0,false,true> (dgrad, row split)")


@pytest.fixture(scope="module")
def census():
    import wino_loop_census

    return wino_loop_census.run()


@pytest.mark.parametrize("name", ROWS)
def test_row_split_loop(census, name):
    row = census[name]
    assert row is not None, f"{name} not in the object"
    assert row["mfma"] == 64
    assert row["v_add/sub_f32"] <= 64, row
    assert row["valu"] <= 72, row
    assert row["scratch"] == 0, row
    assert row["res"]["scratch"] == "0", row["res"]
    assert int(row["res"]["vgpr"]) <= 256 and int(row["res"]["agpr"]) <= 256, row["res"]


def test_training_kernels_do_not_spill(census):
    for name in ROWS + ("conv3x3_wgrad_wino_kernel",):
        assert census[name]["res"]["scratch"] == "0", (name, census[name]["res"])
