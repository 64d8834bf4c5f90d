#!/usr/bin/env python3
"""Instruction census of the Winograd kernels' main loops (CPU only: no GPU needed).

Compiles tiny_diffusion_amd/csrc/conv3x3_wino.hip for gfx950 with the project's flags (_build.HIPCC_FLAGS) to device
assembly in a temporary directory, finds each Winograd kernel's innermost main loop (the smallest span between a label
and a branch back to it that holds an MFMA; of a kernel with one copy of its loop per wave role, the smaller) and
prints per-class instruction counts of one iteration, scaled to 64 MFMAs (one K-stage of every kernel), with the
kernel's VGPR / AGPR counts and scratch size.
usage: wino_loop_census.py [path/to/conv3x3_wino.hip]"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tiny_diffusion_amd import _build  # noqa: E402

KERNELS = [("conv3x3_wgrad_wino_kernel", "_Z25conv3x3_wgrad_wino_kernel10WinoWgArgs"),
           ("conv3x3_wino_kernel<1,false,false> (forward, stats)", "_Z19conv3x3_wino_kernelILi1ELb0ELb0EEv8WinoArgs"),
           ("conv3x3_wino_kernel<0,false,false> (input gradient)", "_Z19conv3x3_wino_kernelILi0ELb0ELb0EEv8WinoArgs"),
           ("conv3x3_wino_kernel<1,false,true> (fwd, row split)", "_Z19conv3x3_wino_kernelILi1ELb0ELb1EEv8WinoArgs"),
           ("conv3x3_wino_kernel<0,false,true> (dgrad, row split)", "_Z19conv3x3_wino_kernelILi0ELb0ELb1EEv8WinoArgs")]
CLASSES = ["mfma", "v_add/sub_f32", "other VALU", "accvgpr mov", "SALU", "ds", "buffer", "scratch", "waitcnt/barrier"]


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if re.fullmatch(r"v_(add|sub|subrev)_f32(_e32|_e64)?", op):
        return "v_add/sub_f32"
    if op.startswith("v_accvgpr"):
        return "accvgpr mov"
    if op.startswith("v_"):
        return "other VALU"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith("buffer_"):
        return "buffer"
    if op.startswith(("s_waitcnt", "s_barrier")):
        return "waitcnt/barrier"
    if op.startswith("s_") and not op.startswith(("s_nop", "s_cbranch", "s_branch", "sched_")):
        return "SALU"
    return None


def function_body(asm, sym):
    start = asm.index(f"\n{sym}:")
    end = asm.index(".Lfunc_end", start)
    return asm[start:end]


def innermost_loop(body):
    lines = body.split("\n")
    labels = {}
    best = None
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            labels[m.group(1)] = i
        m = re.match(r"^\s+s_cbranch_\w+\s+(\.LBB\w+)|^\s+s_branch\s+(\.LBB\w+)", ln)
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in labels and any("v_mfma" in x for x in lines[labels[tgt]:i]) and (
                    best is None or i - labels[tgt] < best[1] - best[0]):
                best = (labels[tgt], i)
    return lines[best[0]:best[1] + 1] if best else []


def census(lines):
    n = dict.fromkeys(CLASSES, 0)
    for ln in lines:
        s = ln.strip()
        if not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        c = classify(s.split()[0])
        if c:
            n[c] += 1
        if "buffer_" in s and "off, s[0:3]" in s:   # scratch through the buffer path
            n["scratch"] += 1
    return n


def resources(asm, sym):
    m = re.search(rf"\.name:\s+{re.escape(sym)}\n(.*?)(?=\n  - \.|\Z)", asm, re.S)
    meta = m.group(1) if m else ""
    blk = asm[asm.index(f"\n{sym}:"):]
    get = lambda pat, txt: (re.search(pat, txt) or [None, "?"])[1]  # noqa: E731
    return {"vgpr": get(r"; NumVgprs:\s+(\d+)", blk), "agpr": get(r"; NumAgprs:\s+(\d+)", blk),
            "scratch": get(r"; ScratchSize:\s+(\d+)", blk), "lds_static": get(r"\.group_segment_fixed_size:\s+(\d+)", meta)}


def compile_asm(src):
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "wino.s")
        cmd = [_build._hipcc(), *_build.HIPCC_FLAGS, "--cuda-device-only", "-S", "-I", _build.CSRC, src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError(f"hipcc failed:\n{r.stderr}")
        return open(out).read()


def run(src=None):
    """{kernel name: None (not in the object) or {"lines", the CLASSES per 64 MFMAs, "valu" (non-MFMA VALU per 64
    MFMAs), "res": {"vgpr", "agpr", "scratch", "lds_static"} as strings}}"""
    asm = compile_asm(src or os.path.join(_build.CSRC, "conv3x3_wino.hip"))
    rows = {}
    for name, sym in KERNELS:
        if f"\n{sym}:" not in asm:
            rows[name] = None
            continue
        loop = innermost_loop(function_body(asm, sym))
        n = census(loop)
        k = 64.0 / n["mfma"] if n["mfma"] else 1.0
        row = {c: n[c] * k for c in CLASSES}
        row["valu"] = (n["v_add/sub_f32"] + n["other VALU"]) * k
        row["lines"] = len(loop)
        row["res"] = resources(asm, sym)
        rows[name] = row
    return rows


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_build.CSRC, "conv3x3_wino.hip")
    try:
        rows = run(src)
    except RuntimeError as e:
        sys.exit(str(e))
    print(f"# {os.path.relpath(src, ROOT)}  ({' '.join(_build.HIPCC_FLAGS)})")
    print("# innermost loop, one iteration scaled to 64 MFMAs (one K-stage)")
    print(f"{'kernel':52s} {'lines':>5s} " + " ".join(f"{c:>14s}" for c in CLASSES) + "  VGPR AGPR scratch")
    for name, row in rows.items():
        if row is None:
            print(f"{name:52s} (not found)")
            continue
        print(f"{name:52s} {row['lines']:5d} " + " ".join(f"{row[c]:14.0f}" for c in CLASSES)
              + f"  {row['res']['vgpr']:>4s} {row['res']['agpr']:>4s} {row['res']['scratch']:>7s}")
        print(f"{'':52s} {'':5s}   non-MFMA VALU per 64 MFMAs (add/sub + other): {row['valu']:.0f}")


if __name__ == "__main__":
    main()
