"""Verified range reads against what a caller had to do for a verified range before them, table by table, in one process.  One range
of `range_bytes` per row at seeded pseudo-random offsets; the sides run in turn (a seeded random order every round, so that no side
always follows the same other side), tables warm and their block trees installed, a call by the wall clock with the device idle in
front:
  C1, C2  znippy_decode_verify_rows of another build of the library (ZN_LIB_B=path/to/libznippy_hip.so — the parent commit's; without
          it, this build's) over the touched rows, on two contexts of its own — the only way to a verified range there: decode and hash
          the whole row, then slice.  Their spread |C1 / C2 - 1| is the A/A margin of the report
  V       this build's znippy_rows_read_ranges_verified
  U       this build's znippy_rows_read_ranges (unverified)
Tables: own — this build's level-19 frames of 10 MiB rows of the c3 text; stored — 8 MiB stored rows (c4store's); libzstd — libzstd
-19 multi-block frames of 1 MiB (another writer's: the whole route, every touched row decoded and hashed whole).  Per side: call
time, per-kernel times, decoded_bytes and hashed_bytes.  The expectation under test: V beats C on own and stored rows by more than
C's A/A spread, and V - U is about the hash of the touched blocks (range_verify_blocks).  Also: what building and installing a
table's block tree costs, once.

Usage: [ZN_LIB_B=...] python tools/verified_range_report.py [rows=64] [range_bytes=4096] [rounds=24]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, gen, gen_gpu, workloads
from znippy_amd import _build, _lib, hip

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 64
range_bytes = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 24

ctx_a = hip.Context(0)
ctx_v = hip.Context(0)
ctx_u = hip.Context(0)
lib_b = os.environ.get("ZN_LIB_B")
if lib_b:
    so_a = _build.SO
    _lib._lib = None
    _build.SO = os.path.abspath(lib_b)
ctx_c = [hip.Context(0), hip.Context(0)]
if lib_b:
    _lib._lib = None
    _build.SO = so_a
print(f"V, U = znippy_rows_read_ranges_verified / znippy_rows_read_ranges of {os.path.relpath(_lib.lib_path(), ROOT)}   C1, C2 = "
      f"znippy_decode_verify_rows of {lib_b if lib_b else 'the same library'}   rows {rows}  range {range_bytes} B  rounds {rounds}")


def encode(d_src, lens, skip=None):
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    ctx_a.set_level(19)
    rt = hip.RoundTable(ctx_a, offs, lens, skip)
    d_blob = torch.zeros(rt.blob_bound() + 64, dtype=torch.uint8, device="cuda")
    enc = rt.encode_hash(d_src, d_blob)
    enc = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in enc.items()}
    rt.close()
    return dict(d_blobs=d_blob, bo=enc["blob_offset"], bs=enc["blob_size"], us=lens, comp=enc["compressed"], ck=enc["checksum"])


def archive(name):
    if name == "own":
        lens = np.full(rows, 10 << 20, np.uint64)
        return dict(encode(gen_gpu.text(int(lens.sum())), lens), label=f"{rows} x 10 MiB rows of the c3 text, this build's level-19 frames")
    if name == "stored":
        lens = np.full(rows, 8 << 20, np.uint64)
        return dict(encode(gen_gpu.random_lcg(int(lens.sum())), lens, np.ones(rows, np.uint8)), label=f"{rows} x 8 MiB stored rows (c4store's)")
    one = gen.pseudo_text(1 << 20, seed=8)
    frame = np.frombuffer(workloads.libzstd_compress(one, 19), np.uint8)
    ck = np.frombuffer(ctx_a.blake3(one), np.uint8)
    return dict(d_blobs=torch.from_numpy(np.concatenate([np.tile(frame, rows), np.zeros(64, np.uint8)])).cuda(),
                bo=np.arange(rows, dtype=np.uint64) * np.uint64(len(frame)), bs=np.full(rows, len(frame), np.uint64),
                us=np.full(rows, 1 << 20, np.uint64), comp=np.ones(rows, np.uint8), ck=np.tile(ck, (rows, 1)),
                label=f"{rows} x 1 MiB rows, libzstd -19 multi-block frames (the whole route)")


def timed(ctx, call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = call()
    return (time.perf_counter() - t0) * 1e3, res, dict(ctx.kernel_times())


def med(d):
    return {k: float(np.median(v)) for k, v in d.items()}


for name in ("own", "stored", "libzstd"):
    A = archive(name)
    n, total = len(A["bo"]), int(A["us"].sum())
    bitmap = np.packbits(A["comp"].astype(bool), bitorder="little")
    oo = (np.cumsum(A["us"]) - A["us"]).astype(np.uint64)
    ck = np.ascontiguousarray(A["ck"], np.uint8).reshape(n, 32)
    ctxs = [ctx_c[0], ctx_c[1], ctx_v, ctx_u]
    rts = [hip.RowTable(c, A["bo"], A["bs"], A["us"], oo, bitmap, ck) for c in ctxs]
    # the block tree: built once from the blobs, installed (and authenticated) once
    t_build, (tree, st), k_build = timed(ctx_v, lambda: rts[2].build_block_tree(A["d_blobs"]))
    assert (st == 0).all(), (name, st)
    t_set, st, k_set = timed(ctx_v, lambda: rts[2].set_block_tree(tree))
    assert (st == 0).all(), (name, st)
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    d_rng = [torch.zeros(n * range_bytes + 64, dtype=torch.uint8, device="cuda") for _ in range(2)]
    rng = np.random.default_rng(12345)
    rr = np.arange(n, dtype=np.uint64)
    rb = rng.integers(0, A["us"].astype(np.int64) - range_bytes, n).astype(np.uint64)
    rl = np.full(n, range_bytes, np.uint64)
    sides = [(ctxs[j], (lambda j=j: rts[j].decode_verify(A["d_blobs"], d_out))) for j in range(2)]
    sides.append((ctx_v, lambda: rts[2].read_ranges_verified(A["d_blobs"], rr, rb, rl, d_rng[0])))
    sides.append((ctx_u, lambda: rts[3].read_ranges(A["d_blobs"], rr, rb, rl, d_rng[1])))
    t, kt = ([], [], [], []), ({}, {}, {}, {})
    work = {}
    order = np.random.default_rng(99)
    for i in range(rounds + 3):
        for j in order.permutation(4):
            dt, res, k = timed(*sides[j])
            if j < 2:
                assert res[0]["decode_errors"] == 0 and res[0]["corrupt_rows"] == 0 and res[0]["verified_bytes"] == total, (name, j, res[0])
            else:
                assert (res[0] == 0).all(), (name, res[0])
                work[j] = res[1:]
            if i >= 3:
                t[j].append(dt)
                for kn, v in k.items():
                    kt[j].setdefault(kn, []).append(v)
    idx = torch.from_numpy((oo + rb).astype(np.int64)).cuda()[:, None] + torch.arange(range_bytes, device="cuda")[None, :]
    for d in d_rng:  # the ranges against the whole-row decode's bytes
        assert torch.equal(d[:n * range_bytes].view(n, range_bytes), d_out[idx]), (name, "the ranges are not the decoded rows' bytes")
    c1, c2, v, u = (float(np.median(x)) for x in t)
    spread = abs(c1 / c2 - 1.0)
    c = min(c1, c2)
    kv, ku = med(kt[2]), med(kt[3])
    print(f"\n{name}: {A['label']}  ({total / 2**20:.0f} MiB decoded and hashed by a whole-row run)")
    print(f"  A/A: parent znippy_decode_verify_rows call ms (median of {rounds}) C1 {c1:.4f}  C2 {c2:.4f}  spread {spread * 100:.2f} %")
    print(f"  znippy_rows_read_ranges_verified {v:.4f} ms  = {v / c:.3f} of the parent's znippy_decode_verify_rows ({c:.4f})  -> "
          f"{'less, by more than the spread' if v < c * (1.0 - spread) else 'NOT less by more than the spread'}")
    print(f"  znippy_rows_read_ranges {u:.4f} ms   verified - unverified {v - u:.4f} ms   range_verify_blocks {kv.get('range_verify_blocks', 0.0):.4f} ms"
          f"   kernel sums {sum(kv.values()):.4f} / {sum(ku.values()):.4f}")
    print(f"  verified: decoded_bytes {work[2][0]}  hashed_bytes {work[2][1]} of {total} ({work[2][1] / total * 100:.2f} %)   unverified: decoded_bytes {work[3][0]}")
    print("  parent decode + verify kernels: " + "  ".join(f"{k} {x:.4f}" for k, x in med(kt[0]).items()))
    print("  verified range kernels: " + "  ".join(f"{k} {x:.4f}" for k, x in kv.items()))
    print("  unverified range kernels: " + "  ".join(f"{k} {x:.4f}" for k, x in ku.items()))
    print(f"  block tree, once: {tree.shape[0]} entries ({tree.nbytes} B)  build call {t_build:.3f} ms (" + "  ".join(f"{k} {x:.4f}" for k, x in k_build.items()) +
          f")  set call {t_set:.3f} ms (" + "  ".join(f"{k} {x:.4f}" for k, x in k_set.items()) + ")")
    for x in rts:
        x.close()
    del A, d_out, d_rng
    torch.cuda.empty_cache()
