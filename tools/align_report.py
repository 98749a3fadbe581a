"""Write step with aligned blob offsets (znippy_rounds_set_blob_align) against the packed one, workload by workload, in one
process: sides a1, a16, a128, a4096 are this build's write step at those alignments, each on a rounds table of its own; with
ZN_LIB_B=path/to/libznippy_hip.so (the parent commit's build) sides B1 and B2 are that build's packed write step on two contexts
of its own, loaded the way tools/decode_report.py loads its second side.  All sides run in turn (the order rotates every round),
tables warm; a step is queue + results, by the wall clock with the device idle in front.  B1 against B2 is the A/A of the report:
two copies of one build, whose spread |B1 / B2 - 1| is the margin of the condition
    write step at align 1 <= parent's write step x (1 + spread)
Per alignment the report gives the step, the kernel times, the region size as a fraction of the packed one (the price of the
gaps: at 85 bytes per frame, c2 pays dearly), and the read step and table build time of a row table made from the aligned results.

Usage: [ZN_LIB_B=...] python tools/align_report.py [workloads=c5,c5text,c4store,c2] [rounds=12]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, workloads
from znippy_amd import _build, _lib, hip

names = (sys.argv[1] if len(sys.argv) > 1 else "c5,c5text,c4store,c2").split(",")
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 12
ALIGNS = (1, 16, 128, 4096)

ctx_a = hip.Context(0)
lib_b = os.environ.get("ZN_LIB_B")
ctx_b = []
if lib_b:  # the packed sides from another build of the library
    so_a = _build.SO
    _lib._lib = None
    _build.SO = os.path.abspath(lib_b)
    ctx_b = [hip.Context(0), hip.Context(0)]
    _lib._lib = None
    _build.SO = so_a
print(f"a1 .. a4096 = write step of {os.path.relpath(_lib.lib_path(), ROOT)}   B1, B2 = packed write step of {lib_b if lib_b else '(no second build given)'}   rounds {rounds}")


def step(ctx, rt, d_src, d_blob):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rt.encode_hash_async(d_src, d_blob)
    r = rt.results_lagged(0)
    dt = (time.perf_counter() - t0) * 1e3
    return dt, r, dict(ctx.kernel_times())


def med(x):
    return float(np.median(x))


ok_all = True
for name in names:
    wl = workloads.build(name, torch)
    lens, d_src = wl["lens"], wl["d_src"]
    n, total = len(lens), int(lens.sum())
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    sides = []  # (label, context, table)
    for a in ALIGNS:
        rt = hip.RoundTable(ctx_a, offs, lens, wl["skip"])
        rt.set_blob_align(a)
        sides.append((f"a{a}", ctx_a, rt))
    for k, c in enumerate(ctx_b):
        sides.append((f"B{k + 1}", c, hip.RoundTable(c, offs, lens, wl["skip"])))
    d_blob = torch.zeros(max(rt.blob_bound() for _, _, rt in sides) + 64, dtype=torch.uint8, device="cuda")
    t, kt, last = [[] for _ in sides], [{} for _ in sides], [None] * len(sides)
    for i in range(rounds + 3):
        for j in [(i + k) % len(sides) for k in range(len(sides))]:
            _, ctx, rt = sides[j]
            dt, r, k = step(ctx, rt, d_src, d_blob)
            if i >= 3:
                t[j].append(dt)
                for kn, v in k.items():
                    kt[j].setdefault(kn, []).append(v)
            last[j] = dict(bytes=int(r["blob_bytes"]), bo=r["blob_offset"].copy(), bs=r["blob_size"].copy(), ck=r["checksum"].copy())
    print(f"\n{name}: {wl['name']}  ({n} rounds, {total / 2**20:.0f} MiB in)")
    packed = last[0]["bytes"]
    v1 = med(t[0])
    if ctx_b:
        vb1, vb2 = med(t[len(ALIGNS)]), med(t[len(ALIGNS) + 1])
        spread = abs(vb1 / vb2 - 1.0)
        vb = min(vb1, vb2)
        ok = v1 <= vb * (1.0 + spread)
        ok_all &= ok
        assert last[len(ALIGNS)]["bytes"] == packed and np.array_equal(last[len(ALIGNS)]["bo"], last[0]["bo"]), "align 1 is not the parent's layout"
        print(f"  A/A: parent's packed write step ms (median of {rounds}) B1 {vb1:.4f}  B2 {vb2:.4f}  spread {spread * 100:.2f} %")
        print(f"  align 1 against the parent: {v1:.4f} / {vb:.4f} = {v1 / vb:.3f}  -> {'ok' if ok else 'MISSES'} (<= {1.0 + spread:.4f})")
        print("  parent kernels: " + "  ".join(f"{k} {med(v):.4f}" for k, v in kt[len(ALIGNS)].items()))
    for j, a in enumerate(ALIGNS):
        L = last[j]
        assert np.array_equal(L["bs"], last[0]["bs"]) and np.array_equal(L["ck"], last[0]["ck"]) and (L["bo"] % np.uint64(a) == 0).all()
        print(f"  align {a:4d}: write step {med(t[j]):.4f} ms ({med(t[j]) / v1:.3f} of align 1)  kernel sum {sum(med(v) for v in kt[j].values()):.4f}"
              f"  region {L['bytes']} B = {L['bytes'] / max(packed, 1):.4f} of packed")
        print("              " + "  ".join(f"{k} {med(v):.4f}" for k, v in kt[j].items()))
    # the read side over the aligned regions: row table build, then decode + verify steps
    comp = (1 - wl["skip"]).astype(np.uint8) if wl["skip"] is not None else np.ones(n, np.uint8)
    bitmap = np.packbits(comp.astype(bool), bitorder="little")
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    for j, a in enumerate(ALIGNS):
        _, ctx, rt = sides[j]
        step(ctx, rt, d_src, d_blob)  # the region of this alignment
        L = last[j]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = hip.RowTable(ctx_a, L["bo"], L["bs"], lens, offs, bitmap, L["ck"])
        ctx_a.sync()
        build_ms = (time.perf_counter() - t0) * 1e3
        rd = []
        for i in range(rounds + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows.decode_verify_async(d_blob, d_out, blob_cap=L["bytes"])
            c = rows.results_lagged(0)
            if i >= 3:
                rd.append((time.perf_counter() - t0) * 1e3)
            assert c["corrupt_rows"] == 0 and c["decode_errors"] == 0 and c["verified_bytes"] == total, (name, a, c)
        assert torch.equal(d_out[:total], d_src[:total]), (name, a, "the aligned region does not read back as the source")
        print(f"  align {a:4d}: read step {med(rd):.4f} ms  table_build_ms {build_ms:.3f}")
        rows.close()
    for _, _, rt in sides:
        rt.close()
    del d_blob, d_out, wl, d_src
    torch.cuda.empty_cache()
if ctx_b:
    print("\nalign 1 within the parent's margin on every workload" if ok_all else "\nat least one workload MISSES the parent's margin at align 1")
