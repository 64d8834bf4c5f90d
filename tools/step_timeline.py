#!/usr/bin/env python3
"""Timeline of ONE training step from a rocprofv3 kernel trace of `python3 bench.py --train-only`:

    python tools/step_timeline.py <..._kernel_trace.csv> [step index, default 10] > profiles/rNN_step_timeline.txt

One line per kernel: start / end / duration in us relative to the end of the previous step's Adam kernel, the
hardware queue (1 = main stream, 2 = weight-gradient stream, 3 = helper stream), C for the MFMA convolutions,
the kernel name and its grid.  The footer sums the convolution kernels by role and lists every interval with no
convolution in flight (what the step pays on top of its GEMMs), then every interval of 3 us or more on the caller's
stream between a kernel's end and the next kernel's start, and their sum (the fork / join operations of the schedule)."""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
adam = [i for i, r in enumerate(rows) if r["Kernel_Name"].startswith("adam") or "adam_clip_kernel" in r["Kernel_Name"]]
k = int(sys.argv[2]) if len(sys.argv) > 2 else 10
a, b = adam[k], adam[k + 1]
seg = rows[a + 1:b + 1]
t0 = int(rows[a]["End_Timestamp"])
queues = {}


def short(n):
    return n.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0][:52]


def isconv(n):
    return "conv3x3_igemm" in n or "conv3x3_wgrad" in n or "conv3x3_bf16" in n or "conv3x3_wino" in n


iv = []
for r in seg:
    s, e = int(r["Start_Timestamp"]) - t0, int(r["End_Timestamp"]) - t0
    q = queues.setdefault(r["Queue_Id"], len(queues) + 1)
    n = r["Kernel_Name"]
    if isconv(n):
        iv.append((s, e, n))
    print(f"{s / 1e3:9.1f} {e / 1e3:9.1f} {(e - s) / 1e3:8.1f}  q{q} {'C' if isconv(n) else ' '} {short(n):52s} "
          f"grid {int(r['Grid_Size_X']) // max(int(r['Workgroup_Size_X']), 1)}x{r['Grid_Size_Y']}")
end = int(seg[-1]["End_Timestamp"]) - t0
print(f"\nstep wall {end / 1e3:.1f} us, {len(seg)} kernels")
for tag, pred in (("forward/dgrad (igemm)", lambda n: "igemm" in n or "conv3x3_bf16_kernel" in n or "conv3x3_bf16_ring" in n or "conv3x3_bf16_thin" in n),
                  ("wgrad", lambda n: "wgrad" in n)):
    print(f"  sum of {tag} kernels: {sum(e - s for s, e, n in iv if pred(n)) / 1e3:.1f} us")
gaps, cur = [], 0
for s, e, _ in sorted(iv):
    if s > cur:
        gaps.append((cur, s))
    cur = max(cur, e)
if cur < end:
    gaps.append((cur, end))
print(f"  no convolution in flight: {sum(e - s for s, e in gaps) / 1e3:.1f} us in {len(gaps)} intervals; the longest:")
for s, e in sorted(gaps, key=lambda g: g[0] - g[1])[:12]:
    inside = [short(r["Kernel_Name"]) for r in seg
              if int(r["Start_Timestamp"]) - t0 < e and int(r["End_Timestamp"]) - t0 > s and not isconv(r["Kernel_Name"])]
    print(f"    {s / 1e3:9.1f} .. {e / 1e3:9.1f} ({(e - s) / 1e3:6.1f} us): {', '.join(dict.fromkeys(inside))}")
# The caller's stream (the queue of the step's first kernel) is the step's dependent chain.  Same-stream boundaries
# with nothing between them show start == previous end; what is left are the event records and stream waits that the
# fork / join schedule puts there (and, between steps, the host).
MIN_GAP = 3000  # ns
main = [(int(r["Start_Timestamp"]) - t0, int(r["End_Timestamp"]) - t0, short(r["Kernel_Name"]))
        for r in seg if queues[r["Queue_Id"]] == 1]
holes, cur, last = [], 0, "(previous step's Adam)"
for s, e, n in main:
    if s - cur >= MIN_GAP:
        holes.append((cur, s, last, n))
    if e > cur:
        cur, last = e, n
print(f"\ncaller's stream: {len(main)} kernels, {len(holes)} intervals >= {MIN_GAP / 1e3:.0f} us between a kernel's end "
      f"and the next kernel's start, {sum(e - s for s, e, _, _ in holes) / 1e3:.1f} us in all:")
for s, e, a, b in holes:
    print(f"    {s / 1e3:9.1f} .. {e / 1e3:9.1f} ({(e - s) / 1e3:6.1f} us): {a} -> {b}")
