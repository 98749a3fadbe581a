"""The read step around its kernels, this build against another build of the library, in one process: the bench's own step —
decode_verify_async + results_lagged(1), two runs in flight, kernel timing level 1 — timed in blocks of pipelined steps by the
wall clock, the sides taking turns (the order rotates every round).  Sides: P1 and P2, two contexts of the other build
(ZN_LIB_B=path/to/libznippy_hip.so — the parent commit's; without it, this build's) whose spread |P1 / P2 - 1| is the margin of
the report; this build with the default ordering and with ZNIPPY_NO_RUN_LANES (every lean run in queue order on the main stream:
the parent's order of stream operations).  Per side: ms per step (median of the rounds), the longest bracketed kernel's time by
its HIP events, and step minus that kernel — except on a side whose runs went to the run lanes, where the events stand on the lane
and the kernel's time includes its wait for CUs the run in front still holds: there the step alone counts, and the line says so
(with the context's lane counters).  c2 is the headline
table (100k x 10 KiB, libzstd -19 frames); the other workloads are this build's own archives and are there to show that nothing
gets slower: each side must stay within the other build's A/A spread.  Table build time (create + the stream drained, median of
the rounds, the sides taking turns) is printed per side under the same rule.

A side's place in the order in which contexts and tables are created moves its step by a few tenths of a percent on the big
workloads (four sides of one build: 0.5 % on c5); `this_first` as the fourth argument creates this build's sides in front of the
other build's, so that a difference that follows the place and not the build shows.

Usage: [ZN_LIB_B=...] python tools/step_overhead_report.py [workloads=c2,c3,c4store,c5] [rounds=9] [steps per block=40] [this_first]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, gen, workloads
from gpu_cases import make_ctx
from znippy_amd import _build, _lib, hip

names = (sys.argv[1] if len(sys.argv) > 1 else "c2,c3,c4store,c5").split(",")
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
block = int(sys.argv[3]) if len(sys.argv) > 3 else 40
this_first = len(sys.argv) > 4 and sys.argv[4] == "this_first"

lib_b = os.environ.get("ZN_LIB_B")
so_a = _build.SO
SIDES = [("P1", None), ("P2", None), ("default", {}), ("no_run_lanes", {"ZNIPPY_NO_RUN_LANES": "1"})]
ctx_t = [make_ctx(env) for _, env in SIDES[2:]] if this_first else []
if lib_b:
    _lib._lib = None
    _build.SO = os.path.abspath(lib_b)
ctx_p = [hip.Context(0), hip.Context(0)]
if lib_b:
    _lib._lib = None
    _build.SO = so_a
ctxs = ctx_p + (ctx_t or [make_ctx(env) for _, env in SIDES[2:]])
made = [2, 3, 0, 1] if this_first else [0, 1, 2, 3]  # the order in which the sides' tables are created
print(f"P1, P2 = {lib_b if lib_b else 'this build'}   the other sides = {os.path.relpath(_lib.lib_path(), ROOT)}   rounds {rounds} x {block} steps"
      f"   created first: {'this build' if this_first else 'P1, P2'}")


def archive(name):
    if name == "c2":  # the headline table (bench.py)
        n, sz = 100_000, 10240
        chunk = gen.text(sz)
        frame = np.frombuffer(workloads.libzstd_compress(chunk, 19), dtype=np.uint8)
        fl = len(frame)
        return dict(d_blobs=torch.from_numpy(np.concatenate([np.tile(frame, n), np.zeros(64, np.uint8)])).cuda(),
                    bo=np.arange(n, dtype=np.uint64) * fl, bs=np.full(n, fl, np.uint64), us=np.full(n, sz, np.uint64),
                    comp=np.ones(n, np.uint8), ck=np.tile(np.frombuffer(ctxs[2].blake3(chunk), dtype=np.uint8), (n, 1)),
                    label="100k x 10 KiB text chunks, libzstd -19 frames")
    wl = workloads.build(name, torch)  # this build's own archive of the configuration
    lens = wl["lens"]
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    rt = hip.RoundTable(ctxs[2], offs, lens, wl["skip"])
    d_blob = torch.zeros(rt.blob_bound() + 64, dtype=torch.uint8, device="cuda")
    enc = rt.encode_hash(wl["d_src"], d_blob)
    enc = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in enc.items()}
    rt.close()
    return dict(d_blobs=d_blob, bo=enc["blob_offset"], bs=enc["blob_size"], us=lens, comp=enc["compressed"], ck=enc["checksum"], label=wl["name"])


def run_block(ctx, rt, d_blobs, d_out, steps, total):
    """`steps` pipelined steps as bench.py queues them -> ms per step."""
    torch.cuda.synchronize(); ctx.sync()
    t0 = time.perf_counter()
    for k in range(steps):
        rt.decode_verify_async(d_blobs, d_out)
        if k:
            c = rt.results_lagged(1)
    c = rt.results_lagged(0)
    dt = (time.perf_counter() - t0) * 1e3 / steps
    assert c["corrupt_rows"] == 0 and c["decode_errors"] == 0 and c["verified_bytes"] == total, c
    return dt


ok_all = True
for name in names:
    A = archive(name)
    total = int(A["us"].sum())
    bitmap = np.packbits(A["comp"].astype(bool), bitorder="little")
    oo = (np.cumsum(A["us"]) - A["us"]).astype(np.uint64)
    rts = [None] * len(ctxs)
    for j in made:
        rts[j] = hip.RowTable(ctxs[j], A["bo"], A["bs"], A["us"], oo, bitmap, A["ck"])
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    build = [[] for _ in ctxs]  # table build time: create + the context's stream drained, the sides taking turns
    for i in range(rounds + 2):
        for j in [(i + k) % len(ctxs) for k in range(len(ctxs))]:
            ctxs[j].sync()
            t0 = time.perf_counter()
            tmp = hip.RowTable(ctxs[j], A["bo"], A["bs"], A["us"], oo, bitmap, A["ck"])
            ctxs[j].sync()
            if i >= 2:
                build[j].append((time.perf_counter() - t0) * 1e3)
            tmp.close()
    level = 1 if name in ("c2", "c2small") else 2  # as bench.py's timed region
    t = [[] for _ in ctxs]
    main = [[] for _ in ctxs]
    def lane_stats(c):  # (a library without the counters — an older build as the other side — has no lanes)
        return c.run_lane_stats() if hasattr(c.L, "znippy_ctx_run_lane_stats") else {}
    lanes0 = [lane_stats(c) for c in ctxs]
    for c in ctxs:
        c.set_kernel_timing(level)
    for i in range(rounds + 2):
        for j in [(i + k) % len(ctxs) for k in range(len(ctxs))]:
            dt = run_block(ctxs[j], rts[j], A["d_blobs"], d_out, block, total)
            if i >= 2:
                t[j].append(dt)
                kt = dict(ctxs[j].kernel_times())  # the block's last run
                main[j].append(max(kt.values()) if kt else float("nan"))
    kall = []
    for j, c in enumerate(ctxs):  # every kernel's time, in untimed runs
        c.set_kernel_timing(2)
        acc = {}
        for _ in range(5):
            rts[j].decode_verify_async(A["d_blobs"], d_out)
            rts[j].results_lagged(0); c.sync()
            for kn, v in c.kernel_times():
                acc.setdefault(kn, []).append(v)
        kall.append({k: float(np.median(v)) for k, v in acc.items()})
    med = [float(np.median(x)) for x in t]
    mk = [float(np.median(x)) for x in main]
    spread = abs(med[0] / med[1] - 1.0)
    base = min(med[0], med[1])
    print(f"\n{name}: {A['label']}  ({len(A['bo'])} rows, {total / 2**20:.0f} MiB decoded)")
    print(f"  A/A of the other build: P1 {med[0]:.4f}  P2 {med[1]:.4f} ms per step  spread {spread * 100:.2f} %")
    for j, (side, _) in enumerate(SIDES):
        verdict = ""
        if j >= 2:
            gain = 1.0 - med[j] / base
            slower = med[j] > max(med[0], med[1]) * (1.0 + spread)
            ok_all &= not slower
            verdict = f"  vs other build {gain * 100:+.2f} %" + ("  beats it by more than 5 x spread" if gain > 5 * spread else "") + ("  SLOWER than its margin" if slower else "")
        lanes = {k: v - lanes0[j][k] for k, v in lane_stats(ctxs[j]).items()}
        if lanes.get("unordered"):  # the bracketed kernel waited for CUs inside its events: no "step - kernel"
            print(f"  {side:15s} step {med[j]:.4f} ms   main kernel {mk[j]:.4f} ms INCLUDING its wait on the lane   lanes {lanes}{verdict}")
        else:
            print(f"  {side:15s} step {med[j]:.4f} ms   main kernel {mk[j]:.4f} ms   step - main kernel {(med[j] - mk[j]) * 1e3:6.1f} us{verdict}")
    bm = [float(np.median(x)) for x in build]
    bspread = abs(bm[0] / bm[1] - 1.0)
    for j, (side, _) in enumerate(SIDES):
        slower = j >= 2 and bm[j] > max(bm[0], bm[1]) * (1.0 + bspread)
        ok_all &= not slower
        print(f"  {side:15s} table_build_ms {bm[j]:.4f}" + (f"  (A/A spread of the other build {bspread * 100:.2f} %)" if j == 1 else "") + ("  SLOWER than its margin" if slower else ""))
    for j in (0, 2):
        print(f"  kernels of {SIDES[j][0]}: " + "  ".join(f"{k} {v:.4f}" for k, v in kall[j].items()))
    for r in rts:
        r.close()
    del A, d_out
    torch.cuda.empty_cache()
print("\nno side slower than the other build's margin" if ok_all else "\nat least one side is SLOWER than the other build's margin")
