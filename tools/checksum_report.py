"""Content checksums on the batch path (znippy_ctx_set_batch_checksums) against the serial decoder, and the default path against the
parent build, in one process.  Three workloads, each as libzstd -19 frames WITH a content checksum and as their twins without one
(the same bytes, Content_Checksum bit cleared, trailer dropped):
  text    text_rows x 10 KiB chunks of the image's source text (the shape of the read_text_archive leg)
  one     one 8 MiB frame of the image's shared objects
  binary  binary_MB of such 8 MiB frames
Sides, all warm, run in turn, the order changing every round so that each side follows each other side equally often (a side that always ran
behind the same other side would always find the caches as that one left them); a step is queue + results by the wall clock, device idle in front:
  off, on   the checksummed table on this build, switch off (the serial decoder checks) and on (the checksum stage does)
  A         the twin table on this build, switch off — the default path
  P1, P2    the twin table on another build of the library on two contexts (ZN_LIB_B=path/to/libznippy_hip.so, the parent commit's;
            without it this build's): the A/A of the report, whose spread |P1 / P2 - 1| is the margin of  A <= min(P1, P2) x (1 + spread)
for the decode + verify step and for the decode-only step.  Per-kernel times (medians) of off and on, zstd_batch_checksum among them,
and the stage's counters are printed beside the step times.

Usage: [ZN_LIB_B=...] python tools/checksum_report.py [text_rows=100000] [binary_MB=256] [rounds=8]"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, workloads
from znippy_amd import _build, _lib, hip

text_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
binary_mb = int(sys.argv[2]) if len(sys.argv) > 2 else 256
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 8

ctx_off, ctx_on, ctx_a = hip.Context(0), hip.Context(0), hip.Context(0)
ctx_on.set_batch_checksums(1)
lib_b = os.environ.get("ZN_LIB_B")
if lib_b:  # the parent's sides from another build of the library
    so_a = _build.SO
    _lib._lib = None
    _build.SO = os.path.abspath(lib_b)
ctx_p = [hip.Context(0), hip.Context(0)]
if lib_b:
    _lib._lib = None
    _build.SO = so_a
print(f"off, on, A = {os.path.relpath(_lib.lib_path(), ROOT)}   P1, P2 = {lib_b if lib_b else 'the same library'}   rounds {rounds}")


def twin(frame):
    return frame[:4] + bytes([frame[4] & ~4]) + frame[5:-4]


def frames_of(slices):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda x: workloads.libzstd_compress_adv(x, 19, checksum=True), slices))


def workload(name):
    """-> label, distinct slices, their checksummed frames, row -> slice"""
    if name == "text":
        sz, distinct = 10240, min(4096, text_rows)
        raw = b"".join(workloads.image_corpus("text", distinct * sz + (1 << 20), whole_files=False))
        sl = [raw[i * sz:(i + 1) * sz] for i in range(distinct)]
        return f"{text_rows} x 10 KiB chunks of real text, libzstd -19 frames", sl, frames_of(sl), np.arange(text_rows) % distinct
    n = 1 if name == "one" else max(1, binary_mb // 8)
    raw = b"".join(workloads.image_corpus("binary", n * (8 << 20) + (1 << 20), whole_files=False))
    sl = [raw[i << 23:(i + 1) << 23] for i in range(n)]
    sl = [s for s in sl if len(s) == 8 << 20] or sl[:1]
    return f"{len(sl)} x 8 MiB of shared objects, libzstd -19 frames", sl, frames_of(sl), np.arange(len(sl))


def table(ctx, frames, sl, idx, dig):
    bs = np.array([len(f) for f in frames], np.uint64)[idx]
    us = np.array([len(s) for s in sl], np.uint64)[idx]
    d_blobs = torch.from_numpy(np.frombuffer(b"".join(frames[i] for i in idx) + bytes(64), dtype=np.uint8).copy()).cuda()
    return d_blobs, [hip.RowTable(c, (np.cumsum(bs) - bs).astype(np.uint64), bs, us, (np.cumsum(us) - us).astype(np.uint64), None, dig[idx]) for c in ctx]


def step(ctx, queue, rt):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    queue()
    c = rt.results_lagged(0)
    return (time.perf_counter() - t0) * 1e3, c, dict(ctx.kernel_times())


ok_all = True
for name in ("text", "one", "binary"):
    label, sl, fr, idx = workload(name)
    dig = np.stack([np.frombuffer(ctx_a.blake3(x), dtype=np.uint8) for x in sl])
    total = int(sum(len(sl[i]) for i in idx))
    blobs_ck, (rt_off, rt_on) = table([ctx_off, ctx_on], fr, sl, idx, dig)
    blobs_tw, (rt_a, rt_p1, rt_p2) = table([ctx_a] + ctx_p, [twin(f) for f in fr], sl, idx, dig)
    outs = [torch.zeros(total + 64, dtype=torch.uint8, device="cuda") for _ in range(2)]
    names = ("off", "on", "A", "P1", "P2")
    print(f"\n{name}: {label}  ({len(idx)} rows, {total / 2**20:.0f} MiB decoded)")
    for kind in ("decode + verify", "decode-only"):
        def q(rt, blobs, out):
            return (lambda: rt.decode_verify_async(blobs, out)) if kind == "decode + verify" else (lambda: rt.decode_async(blobs, out))
        sides = [(ctx_off, q(rt_off, blobs_ck, outs[0]), rt_off), (ctx_on, q(rt_on, blobs_ck, outs[1]), rt_on), (ctx_a, q(rt_a, blobs_tw, outs[0]), rt_a),
                 (ctx_p[0], q(rt_p1, blobs_tw, outs[0]), rt_p1), (ctx_p[1], q(rt_p2, blobs_tw, outs[0]), rt_p2)]
        t, kt = [[] for _ in sides], [{} for _ in sides]
        for i in range(rounds + 2):
            for j in [((i + k) * (1 + i % 4)) % len(sides) for k in range(len(sides))]:  # (five sides: every stride is a full turn, and every side follows every other)
                dt, c, k = step(*sides[j])
                assert c["corrupt_rows"] == 0 and c["decode_errors"] == 0, (name, kind, names[j], c)
                if i >= 2:
                    t[j].append(dt)
                    for kn, v in k.items():
                        kt[j].setdefault(kn, []).append(v)
        sides[0][1](); rt_off.results_lagged(0); sides[1][1](); rt_on.results_lagged(0)
        assert torch.equal(outs[0], outs[1]), (name, kind, "the bytes differ between switch off and on")
        stats = rt_on.checksum_stats()
        med = [float(np.median(x)) for x in t]
        km = [{k: float(np.median(v)) for k, v in d.items()} for d in kt]
        spread = abs(med[3] / med[4] - 1.0)
        ok = med[2] <= min(med[3], med[4]) * (1.0 + spread)
        ok_all &= ok
        print(f"  {kind} step ms (median of {rounds}):")
        print(f"    with checksums: switch off {med[0]:.4f}  switch on {med[1]:.4f}  on / off {med[1] / med[0]:.3f}   zstd_batch_checksum {km[1].get('zstd_batch_checksum', float('nan')):.4f}"
              f"   checksum_stats {stats}")
        print(f"    without checksums: this build, switch off {med[2]:.4f}  parent P1 {med[3]:.4f}  P2 {med[4]:.4f}  spread {spread * 100:.2f} %  A / min(P) {med[2] / min(med[3], med[4]):.3f}"
              f"  -> {'ok' if ok else 'MISSES'} (<= {1.0 + spread:.4f})")
        print("    kernels, switch off: " + "  ".join(f"{k} {v:.4f}" for k, v in km[0].items()))
        print("    kernels, switch on:  " + "  ".join(f"{k} {v:.4f}" for k, v in km[1].items()))
    for r in (rt_off, rt_on, rt_a, rt_p1, rt_p2):
        r.close()
    del blobs_ck, blobs_tw, outs
    torch.cuda.empty_cache()
print("\nthe default path is within the parent's margin on every workload" if ok_all else "\nthe default path MISSES the parent's margin on at least one workload")
