"""Range reads against whole-row decodes, table by table, in one process.  One range of `range_bytes` per row at seeded pseudo-random
offsets; the sides run in turn (a seeded random order every round, so that no side always follows the same other side), tables warm,
a call by the wall clock with the device idle in front:
  B1, B2  znippy_decode_rows of another build of the library (ZN_LIB_B=path/to/libznippy_hip.so — the parent commit's; without it,
          this build's) on two contexts of its own: their spread |B1 / B2 - 1| is the A/A margin of the report
  D       this build's znippy_decode_rows over the same rows: must sit inside that margin (nothing it runs was touched)
  R       this build's znippy_rows_read_ranges
Tables: own — this build's level-19 frames of 10 MiB rows of the c3 text; words — the same of non-periodic word soup (every block
entropy-coded); stored — 8 MiB stored rows (c4store's); libzstd — libzstd -19 multi-block frames of 1 MiB (another writer's: the
fallback, every touched row decoded whole).  Per side: call time, per-kernel times, and for R decoded_bytes against the rows' sizes.
Last, the fixed cost: a call of ONE range on the own table.

Usage: [ZN_LIB_B=...] python tools/range_report.py [rows=64] [range_bytes=4096] [rounds=24]"""
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
ctx_r = hip.Context(0)
lib_b = os.environ.get("ZN_LIB_B")
if lib_b:
    so_a = _build.SO
    _lib._lib = None
    _build.SO = os.path.abspath(lib_b)
ctx_b = [hip.Context(0), hip.Context(0)]
if lib_b:
    _lib._lib = None
    _build.SO = so_a
print(f"D, R = znippy_decode_rows / znippy_rows_read_ranges of {os.path.relpath(_lib.lib_path(), ROOT)}   B1, B2 = znippy_decode_rows of "
      f"{lib_b if lib_b else 'the same library'}   rows {rows}  range {range_bytes} B  rounds {rounds}")


def encode(d_src, lens, skip=None):
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    ctx_a.set_level(19)
    rt = hip.RoundTable(ctx_a, offs, lens, skip)
    d_blob = torch.zeros(rt.blob_bound() + 64, dtype=torch.uint8, device="cuda")
    enc = rt.encode_hash(d_src, d_blob)
    enc = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in enc.items()}
    rt.close()
    return dict(d_blobs=d_blob, bo=enc["blob_offset"], bs=enc["blob_size"], us=lens, comp=enc["compressed"])


def archive(name):
    if name == "own":
        lens = np.full(rows, 10 << 20, np.uint64)
        return dict(encode(gen_gpu.text(int(lens.sum())), lens), label=f"{rows} x 10 MiB rows of the c3 text, this build's level-19 frames")
    if name == "words":
        one = torch.from_numpy(np.frombuffer(gen.pseudo_text(10 << 20, seed=7), np.uint8).copy()).cuda()
        lens = np.full(rows, 10 << 20, np.uint64)
        return dict(encode(torch.cat([one.repeat(rows), torch.zeros(64, dtype=torch.uint8, device="cuda")]), lens),
                    label=f"{rows} x 10 MiB rows of word soup, this build's level-19 frames")
    if name == "stored":
        lens = np.full(rows, 8 << 20, np.uint64)
        return dict(encode(gen_gpu.random_lcg(int(lens.sum())), lens, np.ones(rows, np.uint8)), label=f"{rows} x 8 MiB stored rows (c4store's)")
    one = gen.pseudo_text(1 << 20, seed=8)
    frame = np.frombuffer(workloads.libzstd_compress(one, 19), np.uint8)
    return dict(d_blobs=torch.from_numpy(np.concatenate([np.tile(frame, rows), np.zeros(64, np.uint8)])).cuda(),
                bo=np.arange(rows, dtype=np.uint64) * np.uint64(len(frame)), bs=np.full(rows, len(frame), np.uint64),
                us=np.full(rows, 1 << 20, np.uint64), comp=np.ones(rows, np.uint8), label=f"{rows} x 1 MiB rows, libzstd -19 multi-block frames (the fallback)")


def timed(ctx, call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = call()
    return (time.perf_counter() - t0) * 1e3, res, dict(ctx.kernel_times())


def med(d):
    return {k: float(np.median(v)) for k, v in d.items()}


inside_all = True
for name in ("own", "words", "stored", "libzstd"):
    A = archive(name)
    n, total = len(A["bo"]), int(A["us"].sum())
    bitmap = np.packbits(A["comp"].astype(bool), bitorder="little")
    oo = (np.cumsum(A["us"]) - A["us"]).astype(np.uint64)
    ctxs = [ctx_b[0], ctx_b[1], ctx_a, ctx_r]
    rts = [hip.RowTable(c, A["bo"], A["bs"], A["us"], oo, bitmap, None) for c in ctxs]
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    d_rng = torch.zeros(n * range_bytes + 64, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(12345)
    rr = np.arange(n, dtype=np.uint64)
    rb = rng.integers(0, A["us"].astype(np.int64) - range_bytes, n).astype(np.uint64)
    rl = np.full(n, range_bytes, np.uint64)
    sides = [(ctxs[j], (lambda j=j: rts[j].decode(A["d_blobs"], d_out))) for j in range(3)]
    sides.append((ctx_r, lambda: rts[3].read_ranges(A["d_blobs"], rr, rb, rl, d_rng)))
    t, kt = ([], [], [], []), ({}, {}, {}, {})
    decoded = 0
    order = np.random.default_rng(99)
    for i in range(rounds + 3):
        for j in order.permutation(4):
            dt, res, k = timed(*sides[j])
            if j < 3:
                assert res[0]["decode_errors"] == 0 and res[0]["total_written_bytes"] == total, (name, j, res[0])
            else:
                assert (res[0] == 0).all(), (name, res[0])
                decoded = res[1]
            if i >= 3:
                t[j].append(dt)
                for kn, v in k.items():
                    kt[j].setdefault(kn, []).append(v)
    got = d_rng[:n * range_bytes].view(n, range_bytes)        # the ranges against the whole-row decode's bytes
    idx = torch.from_numpy((oo + rb).astype(np.int64)).cuda()[:, None] + torch.arange(range_bytes, device="cuda")[None, :]
    assert torch.equal(got, d_out[idx]), (name, "the ranges are not the decoded rows' bytes")
    b1, b2, d, r = (float(np.median(x)) for x in t)
    spread = abs(b1 / b2 - 1.0)
    b = min(b1, b2)
    inside = abs(d / ((b1 + b2) / 2) - 1.0) <= spread or min(b1, b2) <= d <= max(b1, b2)
    inside_all &= inside
    print(f"\n{name}: {A['label']}  ({total / 2**20:.0f} MiB decoded by a whole-row run)")
    print(f"  A/A: parent znippy_decode_rows call ms (median of {rounds}) B1 {b1:.4f}  B2 {b2:.4f}  spread {spread * 100:.2f} %")
    print(f"  this build's znippy_decode_rows {d:.4f} ms  ratio to the parent's mean {d / ((b1 + b2) / 2):.4f}  -> {'inside the spread' if inside else 'OUTSIDE the spread'}")
    print(f"  znippy_rows_read_ranges {r:.4f} ms  = {r / b:.3f} of the parent's znippy_decode_rows ({b:.4f})  -> "
          f"{'less, by more than the spread' if r < b * (1.0 - spread) else 'NOT less by more than the spread'}")
    print(f"  decoded_bytes {decoded} of {total} ({decoded / total * 100:.2f} %)")
    print("  parent decode kernels: " + "  ".join(f"{k} {v:.4f}" for k, v in med(kt[0]).items()))
    print("  this build's decode kernels: " + "  ".join(f"{k} {v:.4f}" for k, v in med(kt[2]).items()))
    print("  range kernels: " + "  ".join(f"{k} {v:.4f}" for k, v in med(kt[3]).items()) + f"   (sum {sum(med(kt[3]).values()):.4f})")
    if name == "own":  # the fixed cost of a call: one range
        one = []
        for i in range(rounds + 3):
            dt, res, k = timed(ctx_r, lambda: rts[3].read_ranges(A["d_blobs"], rr[:1], rb[:1], rl[:1], d_rng))
            if i >= 3:
                one.append(dt)
        print(f"  one-range call {float(np.median(one)):.4f} ms  kernels: " + "  ".join(f"{k} {v:.4f}" for k, v in k.items()))
    for x in rts:
        x.close()
    del A, d_out, d_rng
    torch.cuda.empty_cache()
print("\nthis build's znippy_decode_rows inside the parent's A/A spread on every table" if inside_all
      else "\nthis build's znippy_decode_rows OUTSIDE the parent's A/A spread on at least one table")
