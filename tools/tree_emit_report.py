"""Block tree from the write side (znippy_rounds_emit_block_tree) and the sidecar `<archive>.b3t`: what they cost and what they save.

Write step, workload by workload, in one process: side `off` is this build's write step on a table that was never asked, side `on`
the step with emission on — queue, results and the fetch of the tree; with ZN_LIB_B=path/to/libznippy_hip.so (the parent commit's
build) sides B1 and B2 are that build's write step on two contexts of its own, loaded the way tools/align_report.py loads its second
side.  All sides run in turn (another order of the sides every round, through all of them), tables warm; a step is by the wall clock with the device idle in
front.  B1 against B2 is the A/A of the report: two copies of one build, whose spread |B1 / B2 - 1| is the margin of the condition
    write step with emission off <= parent's write step x (1 + spread)
and the kernel-time names of `off` must be the parent's, those of `on` the same plus block_tree_entries.  `r300k` is a table of
2,000 text rounds of 300,001 bytes (three entries each) beside tests/workloads.py's names.

First verified read: two files of 10 MiB (text, own frames; a .jar, stored) written by znippy_compress_dir with
ZNIPPY_HOST_BLOCK_TREE=1 (on 14 CPUs, so that its slice size keeps each file one chunk); on a fresh znippy_archive handle whose context is warm (one unverified read of a small file), the first
znippy_archive_read_range_verified of 4 KiB from the big file, with the sidecar and with it moved away, by the wall clock.  The
host layer does not expose its context's kernel times, so the kernel names of the two first touches come from the same calls made
through hip.RowTable over the same blobs: set_block_tree + read_ranges_verified, and build_block_tree in front of them.

ZN_B_FIRST=1 creates the other build's contexts in front of this build's: a step of 0.4 ms differs by a few tenths of a per cent with
the order in which a process made its contexts, which is the size of the spreads above.

Usage: [ZN_LIB_B=... [ZN_B_FIRST=1]] python tools/tree_emit_report.py [workloads=c3,c4store,r300k] [rounds=8]"""
import itertools
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, gen, gen_gpu, workloads
from znippy_amd import _build, _lib, block_tree, hip, host

names = (sys.argv[1] if len(sys.argv) > 1 else "c3,c4store,r300k").split(",")
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 8

lib_b = os.environ.get("ZN_LIB_B")
b_first = bool(lib_b) and os.environ.get("ZN_B_FIRST", "0") not in ("", "0")
_lib.lib()  # (this build's library is loaded first either way)
ctx_a = ctx_on = None
if not b_first:
    ctx_a, ctx_on = hip.Context(0), hip.Context(0)  # every side has a context of its own, as the parent's two have
ctx_b = []
if lib_b:  # the parent's sides from another build of the library
    so_a = _build.SO
    _lib._lib = None
    _build.SO = os.path.abspath(lib_b)
    ctx_b = [hip.Context(0), hip.Context(0)]
    _lib._lib = None
    _build.SO = so_a
if b_first:
    ctx_a, ctx_on = hip.Context(0), hip.Context(0)
    print("ZN_B_FIRST: the other build's two contexts were created in front of this build's")
print(f"off, on = write step of {os.path.relpath(_lib.lib_path(), ROOT)}   B1, B2 = write step of {lib_b if lib_b else '(no second build given)'}   rounds {rounds}")


def med(x):
    return float(np.median(x))


def build(name):
    if name == "r300k":
        n, ln = 2000, 300_001
        return dict(lens=np.full(n, ln, np.uint64), skip=None, d_src=gen_gpu.text(n * ln), name="2,000 text rounds of 300,001 bytes")
    return workloads.build(name, torch)


def step(ctx, rt, d_src, d_blob, tree):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rt.encode_hash_async(d_src, d_blob)
    r = rt.results_lagged(0)
    t = rt.block_tree(0) if tree else None
    dt = (time.perf_counter() - t0) * 1e3
    return dt, r, t, ctx.kernel_times()


ok_all = True
for name in names:
    wl = build(name)
    lens, d_src = wl["lens"], wl["d_src"]
    n, total = len(lens), int(lens.sum())
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    sides = [("off", ctx_a, hip.RoundTable(ctx_a, offs, lens, wl["skip"]), False), ("on", ctx_on, hip.RoundTable(ctx_on, offs, lens, wl["skip"]), True)]
    sides[1][2].emit_block_tree()
    for k, c in enumerate(ctx_b):
        sides.append((f"B{k + 1}", c, hip.RoundTable(c, offs, lens, wl["skip"]), False))
    d_blob = torch.zeros(max(s[2].blob_bound() for s in sides) + 64, dtype=torch.uint8, device="cuda")
    perms = list(itertools.permutations(range(len(sides))))  # every order in turn: no side always runs behind the same other one
    random.Random(1).shuffle(perms)
    t, kt, order, last, tree = [[] for _ in sides], [{} for _ in sides], [None] * len(sides), [None] * len(sides), None
    for i in range(rounds + 3):
        for j in perms[i % len(perms)]:
            _, ctx, rt, emit = sides[j]
            dt, r, tr, k = step(ctx, rt, d_src, d_blob, emit)
            if i >= 3:
                t[j].append(dt)
                for kn, v in k:
                    kt[j].setdefault(kn, []).append(v)
            order[j] = [kn for kn, _ in k]
            last[j] = dict(bytes=int(r["blob_bytes"]), bs=r["blob_size"].copy(), ck=r["checksum"].copy())
            tree = tr if emit else tree
    n_entries = sides[1][2].block_tree_layout()[0]
    print(f"\n{name}: {wl['name']}  ({n} rounds, {total / 2**20:.0f} MiB in, {n_entries} entries = {32 * n_entries} B of tree beside {16 + 48 * n} B of results)")
    for j in range(1, len(sides)):
        assert last[j]["bytes"] == last[0]["bytes"] and np.array_equal(last[j]["bs"], last[0]["bs"]) and np.array_equal(last[j]["ck"], last[0]["ck"]), "results differ between the sides"
    v_off, v_on = med(t[0]), med(t[1])
    if ctx_b:
        vb1, vb2 = med(t[2]), med(t[3])
        spread = abs(vb1 / vb2 - 1.0)
        vb = min(vb1, vb2)
        ok = v_off <= vb * (1.0 + spread)
        same = order[0] == order[2]
        ok_all &= ok and same
        print(f"  A/A: parent's write step ms (median of {rounds}) B1 {vb1:.4f}  B2 {vb2:.4f}  spread {spread * 100:.2f} %")
        print(f"  emission off against the parent: {v_off:.4f} / {vb:.4f} = {v_off / vb:.3f}  -> {'ok' if ok else 'MISSES'} (<= {1.0 + spread:.4f})")
        print(f"  kernel-time names with emission off {'equal' if same else 'DIFFER from'} the parent's: {' '.join(order[0])}")
        print("  parent kernels: " + "  ".join(f"{k} {med(v):.4f}" for k, v in kt[2].items()))
    added = [k for k in order[1] if k not in order[0]]
    ok_names = added == (["block_tree_entries"] if n_entries else []) and [k for k in order[1] if k in order[0]] == order[0]
    ok_all &= ok_names
    print(f"  emission off: write step {v_off:.4f} ms  kernel sum {sum(med(v) for v in kt[0].values()):.4f}")
    print("                " + "  ".join(f"{k} {med(v):.4f}" for k, v in kt[0].items()))
    print(f"  emission on : write step {v_on:.4f} ms ({v_on / v_off:.3f} of off, tree fetched)  kernel sum {sum(med(v) for v in kt[1].values()):.4f}"
          f"  names added: {added if added else 'none'} -> {'ok' if ok_names else 'UNEXPECTED'}")
    print("                " + "  ".join(f"{k} {med(v):.4f}" for k, v in kt[1].items()))
    if n_entries:  # the tree is the right one: a row table of the results accepts every row's entries
        r = sides[1][2].results_lagged(0)
        comp = (1 - wl["skip"]).astype(np.uint8) if wl["skip"] is not None else np.ones(n, np.uint8)
        rows = hip.RowTable(ctx_on, r["blob_offset"].copy(), r["blob_size"].copy(), lens, offs, np.packbits(comp.astype(bool), bitorder="little"), r["checksum"].copy())
        st = rows.set_block_tree(tree)
        rows.close()
        print(f"  set_block_tree on the results' row table: {int((st == 0).sum())} of {n} rows accepted")
        ok_all &= bool((st == 0).all())
    for s in sides:
        s[2].close()
    del d_blob, wl, d_src
    torch.cuda.empty_cache()

# ---- first verified read on a fresh handle, with and without the sidecar ----
MIB = 1 << 20
mib = gen.pseudo_text(MIB, seed=5)
files = {"big.txt": b"".join(mib[1000 * i:] + mib[:1000 * i] for i in range(10)),
         "big.jar": np.random.default_rng(6).integers(0, 256, 10 * MIB, dtype=np.uint8).tobytes(), "small.txt": gen.text(5000)}
tmp = tempfile.mkdtemp(prefix="tree_emit_report_")
try:
    os.mkdir(os.path.join(tmp, "in"))
    for k, v in files.items():
        with open(os.path.join(tmp, "in", k), "wb") as f:
            f.write(v)
    arc = os.path.join(tmp, "a.znippy")
    os.environ["ZNIPPY_HOST_BLOCK_TREE"] = "1"
    cpus = os.sched_getaffinity(0)
    os.sched_setaffinity(0, sorted(cpus)[:14])  # compress_dir cuts files at 200 MB / (0.9 x CPUs): 13 workers keep 10 MiB in one chunk
    try:
        host.compress_dir(os.path.join(tmp, "in"), arc)
    finally:
        os.sched_setaffinity(0, cpus)
    del os.environ["ZNIPPY_HOST_BLOCK_TREE"]
    side = block_tree.sidecar_path(arc)
    index, _, _ = host.read_index(arc)
    n_rows, entries = block_tree.read_sidecar(side)
    print(f"\nfirst verified read of 4 KiB on a fresh handle ({rounds} handles each); sidecar: {os.path.getsize(side)} B, {entries.shape[0]} entries, {n_rows} rows")
    raw = np.fromfile(arc, dtype=np.uint8)
    for name in ("big.txt", "big.jar"):
        chunks = [r for r in index if r["relative_path"] == name]
        c0 = chunks[0]
        clen = c0["uncompressed_size"] if c0["compressed"] else c0["blob_size"]
        at = min(5 * MIB, clen - 8192) + 777
        res = {}
        for with_side in (True, False):
            if not with_side:
                os.rename(side, side + ".away")
            ms, stats = [], None
            for _ in range(rounds):
                a = host.ZnippyArchive.open(arc)
                a.read_range("small.txt", 0, 100)  # the context and its buffers exist
                t0 = time.perf_counter()
                got = a.read_range_verified(name, at, 4096)
                ms.append((time.perf_counter() - t0) * 1e3)
                assert got == files[name][at:at + 4096]
                stats = a.block_tree_stats()
                a.close()
            if not with_side:
                os.rename(side + ".away", side)
            res[with_side] = med(ms)
            print(f"  {name} ({'own frame' if c0['compressed'] else 'stored'}, first chunk {clen} B): {'with' if with_side else 'without'} sidecar {med(ms):.3f} ms  stats {stats}")
        print(f"  {name}: without / with = {res[False] / res[True]:.2f}")
        # the same two first touches through hip.RowTable, for the kernel-time names
        first = block_tree.layout([r["uncompressed_size"] if r["compressed"] else r["blob_size"] for r in index])[1]
        i0 = index.index(c0)
        one = lambda v: np.array([v], np.uint64)
        d_blobs = torch.from_numpy(np.concatenate([raw[c0["blob_offset"]:c0["blob_offset"] + c0["blob_size"]], np.zeros(64, np.uint8)])).cuda()
        d_out = torch.zeros(4096 + 64, dtype=torch.uint8, device="cuda")
        ck = np.frombuffer(c0["checksum"], np.uint8).copy()
        for with_side in (True, False):
            rows = hip.RowTable(ctx_a, one(0), one(c0["blob_size"]), one(clen), one(0), np.array([1 if c0["compressed"] else 0], np.uint8), ck)
            seen = []
            if with_side:
                tree = entries[int(first[i0]):int(first[i0 + 1])]
            else:
                tree, st = rows.build_block_tree(d_blobs, blob_cap=c0["blob_size"])
                assert (st == 0).all()
                seen += [k for k, _ in ctx_a.kernel_times()]
            assert (rows.set_block_tree(tree) == 0).all()
            seen += [k for k, _ in ctx_a.kernel_times()]
            st, decoded, hashed = rows.read_ranges_verified(d_blobs, [0], [at], [4096], d_out, blob_cap=c0["blob_size"])
            seen += [k for k, _ in ctx_a.kernel_times()]
            rows.close()
            assert st[0] == 0 and d_out[:4096].cpu().numpy().tobytes() == files[name][at:at + 4096]
            building = [k for k in seen if k in ("range_decode_rows", "range_decode_rows_late", "block_tree_cvs")]
            ok_read = (not building) if with_side else True
            ok_all &= ok_read
            print(f"    {'with' if with_side else 'without'} sidecar: decoded {decoded} B, hashed {hashed} B; kernels: {' '.join(seen)}"
                  + (f"  -> {'no decode or build kernel' if ok_read else 'UNEXPECTED: ' + ' '.join(building)}" if with_side else ""))
finally:
    shutil.rmtree(tmp, ignore_errors=True)
print("\nall conditions hold" if ok_all else "\nat least one condition MISSES")
