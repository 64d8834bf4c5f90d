"""CPU: the tuning-knob table (csrc/knobs.h, csrc/knobs.hip) through tdx_tune_set / tdx_tune_get / tdx_tune_name and
_lib.tuned.  The three entries touch no device, so nothing here needs a GPU.

DEFAULTS below is the one place outside csrc/knobs.h where the defaults are written: it pins them.  RULES restates, in
plain Python, what each key does to a value it is given."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import tiny_diffusion_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBES = (-5, -1, 0, 1, 2, 3, 4, 7, 8, 9, 255, 256, 257, 100000)


def raw(v, d):
    return v


def boolean(v, d):
    return int(v != 0)


def mask7(v, d):
    return v & 7


def positive(v, d):
    return v if v > 0 else d


def non_negative(v, d):
    return v if v >= 0 else d


def at_least(lo):
    return lambda v, d: v if v > lo else lo


# key: (default, rule)
KNOBS = {
    "conv_tile": (0, raw), "splitk": (1, raw), "splitk_tiles": (260, raw), "splitk_target": (512, raw),
    "streams": (-1, raw), "materialize": (1, raw), "sample_defer_max": (2, raw), "conv_dbg": (0, raw),
    "conv_stamp": (0, raw), "wgrad_small": (1, raw),
    "bf16_storage": (1, boolean), "sample_tables": (1, boolean), "sample_halves": (0, boolean),
    "conv_hybrid": (0, boolean), "splitk_train": (1, boolean), "bf16_materialize": (1, boolean),
    "bf16_ring": (0, boolean), "bf16_wgrad9": (1, boolean), "bf16_wgrad_swz": (1, boolean), "wino": (1, boolean),
    "wino_infer": (1, boolean), "wino_wgrad": (1, boolean), "wino_rows": (1, boolean), "infer_ring": (0, boolean),
    "sample_fuse": (6, mask7), "bnbwd_fused": (6, mask7),
    "conv_min_tiles": (256, positive), "splitk_train_t64": (1024, positive), "splitk_train_target": (1536, positive),
    "wino_wgrad_min_tiles": (1024, positive), "wino_wgrad_target": (512, positive),
    "wino_rows_min_stages": (16, positive), "wgrad_target": (2048, positive),
    "wino_infer_min_units": (700, non_negative), "wino_infer_ovh": (2, non_negative),
    "wino_infer_red": (3, non_negative), "infer_ovh": (4, non_negative), "infer_red": (12, non_negative),
    "wino_min_wgs": (100, at_least(1)), "wgrad_target_big": (1024, at_least(0)), "infer_splits": (0, at_least(0)),
    "wgrad9_wgs": (0, at_least(0)),
    "sample_halves_min": (4, at_least(2)),
    "infer_stages": (4, lambda v, d: 3 if v == 3 else 4),
    "infer_cus": (256, lambda v, d: v if 1 <= v <= 256 else 256),
    "bf16_thin": (3, lambda v, d: 0 if v < 0 else v),
    "stats_epi": (0, boolean),          # bit 3 of conv_dbg
}
DEFAULTS = {k: d for k, (d, _) in KNOBS.items()}


def get(key):
    v = ctypes.c_int(-12345)
    assert L.lib.tdx_tune_get(key.encode(), ctypes.byref(v)) == 0, key
    return v.value


def put(key, value):
    assert L.lib.tdx_tune_set(key.encode(), value) == 0, key


def names():
    out, i = [], 0
    while (nm := L.lib.tdx_tune_name(i)) is not None:
        out.append(nm.decode())
        i += 1
    return out


def snapshot():
    return {k: get(k) for k in names()}


DUMP = ("import ctypes, json, tiny_diffusion_amd._lib as L\n"
        "out, i = {}, 0\n"
        "while (nm := L.lib.tdx_tune_name(i)) is not None:\n"
        "    v = ctypes.c_int(); assert L.lib.tdx_tune_get(nm, ctypes.byref(v)) == 0\n"
        "    out[nm.decode()] = v.value; i += 1\n"
        "print('KNOBS ' + json.dumps(out))\n")


@pytest.fixture(scope="module")
def fresh():
    """Three fresh interpreters, started together: no TDX_TUNE, a TDX_TUNE of two live keys, one naming a retired key."""
    env = {k: v for k, v in os.environ.items() if k != "TDX_TUNE"}
    env["TDX_NO_AUTOBUILD"] = "1"     # the library under test is the one this process loaded
    specs = {"plain": None, "tuned": "wino=0,sample_fuse=5", "retired": "wino=0,time_stage=14"}
    procs = {k: subprocess.Popen([sys.executable, "-c", DUMP], cwd=ROOT, env=dict(env, **({"TDX_TUNE": s} if s else {})),
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k, s in specs.items()}
    return {k: (p.communicate(), p.returncode) for k, p in procs.items()}


def dumped(result):
    (out, err), rc = result
    assert rc == 0, err
    return json.loads(next(ln for ln in out.splitlines() if ln.startswith("KNOBS "))[6:])


def test_enumeration_and_defaults(fresh):
    ks = names()
    assert len(ks) == len(set(ks)) == 47
    assert set(ks) == set(DEFAULTS)
    assert L.lib.tdx_tune_name(-1) is None and L.lib.tdx_tune_name(len(ks)) is None
    assert dumped(fresh["plain"]) == DEFAULTS


def test_env_tuning_reaches_the_table(fresh):
    assert dumped(fresh["tuned"]) == dict(DEFAULTS, wino=0, sample_fuse=5)
    (out, err), rc = fresh["retired"]
    assert rc != 0 and "time_stage" in err and "KNOBS" not in out


@pytest.mark.parametrize("key", [k for k in KNOBS if k != "stats_epi"])
def test_normaliser(key):
    default, rule = KNOBS[key]
    before = snapshot()
    try:
        for v in PROBES:
            put(key, v)
            assert get(key) == rule(v, default), (key, v)
            put(key, get(key))                       # idempotent at every stored value
            assert get(key) == rule(v, default), (key, v)
    finally:
        put(key, before[key])
    assert snapshot() == before


def test_set_of_get_changes_nothing():
    before = snapshot()
    for k in names():
        put(k, get(k))
    assert snapshot() == before


def test_stats_epi_is_bit_3_of_conv_dbg():
    before = snapshot()
    try:
        for dbg in (0, 1, 8, 52, 63, -1):
            put("conv_dbg", dbg)
            assert get("stats_epi") == (dbg >> 3) & 1
            for v in PROBES:
                put("stats_epi", v)
                assert get("stats_epi") == int(v != 0)
                assert get("conv_dbg") == ((dbg | 8) if v else (dbg & ~8)), (dbg, v)
        for v in PROBES:
            put("conv_stamp", v)
            assert get("conv_stamp") == v
    finally:
        put("conv_dbg", before["conv_dbg"])
        put("conv_stamp", before["conv_stamp"])
    assert snapshot() == before


def test_tuned_restores():
    before = snapshot()
    with L.tuned(sample_fuse=2, wino=0, wgrad_target=-3):
        assert (get("sample_fuse"), get("wino"), get("wgrad_target")) == (2, 0, DEFAULTS["wgrad_target"])
        with L.tuned(sample_fuse=5):                  # the same key inside itself
            assert get("sample_fuse") == 5
            with L.tuned():
                assert get("sample_fuse") == 5
        assert get("sample_fuse") == 2
    assert snapshot() == before
    with pytest.raises(ZeroDivisionError):
        with L.tuned(conv_dbg=16, stats_epi=1, infer_stages=3):
            assert (get("conv_dbg"), get("infer_stages")) == (24, 3)
            1 / 0
    assert snapshot() == before
    assert L.tune_get("sample_fuse") == before["sample_fuse"]


def test_unknown_key_raises_before_anything_is_set():
    before = snapshot()
    with pytest.raises(L.TdxError):
        with L.tuned(wino=0, time_stage=14, sample_fuse=1):
            raise AssertionError("the body ran")
    assert snapshot() == before
    with pytest.raises(L.TdxError):
        L.tune_get("no_such_knob")


def test_get_and_set_refuse_null_and_unknown_keys():
    v = ctypes.c_int(77)
    assert L.lib.tdx_tune_get(None, ctypes.byref(v)) != 0
    assert L.lib.tdx_tune_get(b"no_such_knob", ctypes.byref(v)) != 0
    assert L.lib.tdx_tune_get(b"", ctypes.byref(v)) != 0
    assert L.lib.tdx_tune_get(b"wino", None) != 0
    assert v.value == 77
    assert L.lib.tdx_tune_set(None, 1) != 0 and L.lib.tdx_tune_set(b"no_such_knob", 1) != 0
