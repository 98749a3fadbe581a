"""Packet by packet: a few steady steps of the read step from a rocprofv3 --kernel-trace CSV (clears and counter copies are
kernels of the runtime's own and show up in it), in the format of profiles/step_overhead_after.txt: start / end / duration, the
gap to the latest end of anything before the packet (negative: it started while an earlier packet was still running), queue.
Usage: python tools/step_timeline.py kernel_trace.csv [ANCHOR=k_fused_roles] [occurrence=30] [steps=3]"""
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
anchor = sys.argv[2] if len(sys.argv) > 2 else "k_fused_roles"
occ = int(sys.argv[3]) if len(sys.argv) > 3 else 30
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
idx = [i for i, r in enumerate(rows) if anchor in r["Kernel_Name"]]
if len(idx) <= occ + steps:
    occ = max(0, len(idx) - steps - 1)
i0, i1 = idx[occ], idx[occ + steps]
t0 = int(rows[i0]["Start_Timestamp"])
print("  start us     end us    dur us    gap us  queue  packet   (gap = start - the latest end of anything before it)")
latest = None
for k, r in enumerate(rows[:i1 + 1]):
    s, e = int(r["Start_Timestamp"]) - t0, int(r["End_Timestamp"]) - t0
    if k >= i0 - 3:
        gap = f"{(s - latest) / 1e3:9.1f}" if latest is not None and k > i0 - 3 else " " * 9
        print(f"{s / 1e3:10.1f} {e / 1e3:10.1f} {(e - s) / 1e3:9.1f} {gap}  q{r.get('Queue_Id', '?'):>3}  {r['Kernel_Name'].split('(')[0][-52:]}")
    latest = e if latest is None else max(latest, e)
anchors = [rows[i] for i in idx[occ:occ + steps + 1]]
for a, b in zip(anchors, anchors[1:]):
    sa, ea, sb = int(a["Start_Timestamp"]), int(a["End_Timestamp"]), int(b["Start_Timestamp"])
    print(f"  {anchor}: start to start {(sb - sa) / 1e3:7.1f} us   the next one starts {(ea - sb) / 1e3:+7.1f} us before this one ends (positive: overlap)")
