"""Decode-only step against the decode + verify step, workload by workload, in one process: side A is this build's decode-only run
(znippy_decode_rows), sides B1 and B2 are the decode + verify run of another build of the library on two contexts of its own
(ZN_LIB_B=path/to/libznippy_hip.so — the parent commit's; without it, this build's own decode + verify run), loaded the way
tools/verify_report.py loads its second side.  The three run in turn (the order rotates every round), tables warm, lean where they
can be; a step is queue + results, by the wall clock with the device idle in front.  B1 against B2 is the A/A of the report: two
copies of the same build, whose spread |B1 / B2 - 1| is the margin of the condition
    decode-only step <= decode + verify step x (1 + spread)
— a decode-only run writes the same bytes and hashes nothing.  Beside decode_small / copy_stored of c2 and c2store the hash's VALU
floor (znippy_measure_blake3_pass_ns, priced the way bench.py prices it) is printed: the goal is a store kernel below it.

Usage: [ZN_LIB_B=...] python tools/decode_report.py [workloads=c2,c2store,c3,c4store,c4codec,text] [rounds=12]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, gen, workloads
from znippy_amd import _build, _lib, hip

names = (sys.argv[1] if len(sys.argv) > 1 else "c2,c2store,c3,c4store,c4codec,text").split(",")
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 12

ctx_a = hip.Context(0)
lib_b = os.environ.get("ZN_LIB_B")
if lib_b:  # the decode + verify sides from another build of the library
    so_a = _build.SO
    _lib._lib = None
    _build.SO = os.path.abspath(lib_b)
ctx_b = [hip.Context(0), hip.Context(0)]
if lib_b:
    _lib._lib = None
    _build.SO = so_a
print(f"A = decode-only run of {os.path.relpath(_lib.lib_path(), ROOT)}   B1, B2 = decode + verify run of {lib_b if lib_b else 'the same library'}   rounds {rounds}")
cus = torch.cuda.get_device_properties(0).multi_processor_count


def archive(name):
    """-> dict(d_blobs, bo, bs, us, comp, ck, label)"""
    if name == "c2":  # the headline table: libzstd level-19 frames of the 10 KiB text chunk (bench.py)
        n, sz = 100_000, 10240
        chunk = gen.text(sz)
        frame = np.frombuffer(workloads.libzstd_compress(chunk, 19), dtype=np.uint8)
        fl = len(frame)
        return dict(d_blobs=torch.from_numpy(np.concatenate([np.tile(frame, n), np.zeros(64, np.uint8)])).cuda(),
                    bo=np.arange(n, dtype=np.uint64) * fl, bs=np.full(n, fl, np.uint64), us=np.full(n, sz, np.uint64),
                    comp=np.ones(n, np.uint8), ck=np.tile(np.frombuffer(ctx_a.blake3(chunk), dtype=np.uint8), (n, 1)),
                    label="100k x 10 KiB text chunks, libzstd -19 frames")
    if name == "text":  # the real-text archive of the --full bench: 100k x 10 KiB chunks of source text, libzstd -19 frames
        from concurrent.futures import ThreadPoolExecutor
        n, sz, distinct = 100_000, 10240, 4096
        raw = b"".join(workloads.image_corpus("text", distinct * sz + (1 << 20), whole_files=False))
        sl = [raw[i * sz:(i + 1) * sz] for i in range(distinct)]
        with ThreadPoolExecutor(16) as ex:
            fr = list(ex.map(lambda x: workloads.libzstd_compress(x, 19), sl))
        idx = np.arange(n) % distinct
        bs = np.array([len(f) for f in fr], np.uint64)[idx]
        dig = np.stack([np.frombuffer(ctx_a.blake3(x), dtype=np.uint8) for x in sl])
        return dict(d_blobs=torch.from_numpy(np.frombuffer(b"".join(fr[i] for i in idx) + bytes(64), dtype=np.uint8).copy()).cuda(),
                    bo=(np.cumsum(bs) - bs).astype(np.uint64), bs=bs, us=np.full(n, sz, np.uint64), comp=np.ones(n, np.uint8), ck=dig[idx],
                    label="100k x 10 KiB chunks of real text, libzstd -19 frames")
    wl = workloads.build(name, torch)  # this build's own archive of the configuration
    lens = wl["lens"]
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    rt = hip.RoundTable(ctx_a, offs, lens, wl["skip"])
    d_blob = torch.zeros(rt.blob_bound() + 64, dtype=torch.uint8, device="cuda")
    enc = rt.encode_hash(wl["d_src"], d_blob)
    enc = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in enc.items()}
    rt.close()
    return dict(d_blobs=d_blob, bo=enc["blob_offset"], bs=enc["blob_size"], us=lens, comp=enc["compressed"], ck=enc["checksum"], label=wl["name"])


def step(ctx, queue, rt):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    queue()
    c = rt.results_lagged(0)
    dt = (time.perf_counter() - t0) * 1e3
    return dt, c, dict(ctx.kernel_times())


ok_all = True
for name in names:
    A = archive(name)
    n, total = len(A["bo"]), int(A["us"].sum())
    bitmap = np.packbits(A["comp"].astype(bool), bitorder="little")
    oo = (np.cumsum(A["us"]) - A["us"]).astype(np.uint64)
    ctxs = [ctx_a] + ctx_b
    rts = [hip.RowTable(c, A["bo"], A["bs"], A["us"], oo, bitmap, A["ck"]) for c in ctxs]
    outs = [torch.zeros(total + 64, dtype=torch.uint8, device="cuda") for _ in range(2)]  # A's, and the one B1 and B2 share
    sides = [(ctx_a, lambda: rts[0].decode_async(A["d_blobs"], outs[0]), rts[0]),
             (ctx_b[0], lambda: rts[1].decode_verify_async(A["d_blobs"], outs[1]), rts[1]),
             (ctx_b[1], lambda: rts[2].decode_verify_async(A["d_blobs"], outs[1]), rts[2])]
    t, kt = ([], [], []), ({}, {}, {})
    for i in range(rounds + 3):
        for j in [(i + k) % 3 for k in range(3)]:
            dt, c, k = step(*sides[j])
            assert c["corrupt_rows"] == 0 and c["decode_errors"] == 0 and c["verified_bytes"] == total, (name, j, c)
            if i >= 3:
                t[j].append(dt)
                for kn, v in k.items():
                    kt[j].setdefault(kn, []).append(v)
    assert torch.equal(outs[0], outs[1]), (name, "the decode-only run's bytes are not the decode + verify run's")
    va, vb1, vb2 = (float(np.median(x)) for x in t)
    ka, kb = ({k: float(np.median(v)) for k, v in kt[j].items()} for j in (0, 1))
    spread = abs(vb1 / vb2 - 1.0)
    vb = min(vb1, vb2)
    ok = va <= vb * (1.0 + spread)
    ok_all &= ok
    print(f"\n{name}: {A['label']}  ({n} rows, {total / 2**20:.0f} MiB decoded)")
    print(f"  A/A: decode + verify step ms (median of {rounds}) B1 {vb1:.4f}  B2 {vb2:.4f}  spread {spread * 100:.2f} %")
    print(f"  step ms (median of {rounds}): decode-only {va:.4f}  decode + verify {vb:.4f}  ratio {va / vb:.3f}  -> {'ok' if ok else 'MISSES'} (<= {1.0 + spread:.4f})")
    print(f"  kernel ms, sum: decode-only {sum(ka.values()):.4f}  decode + verify {sum(kb.values()):.4f}")
    print("  decode-only kernels: " + "  ".join(f"{k} {v:.4f}" for k, v in ka.items()))
    print("  decode + verify kernels: " + "  ".join(f"{k} {v:.4f}" for k, v in kb.items()))
    if name in ("c2", "c2store"):  # the hash's VALU floor (bench.py's pricing: every lane of every pass busy) beside the store kernel
        ns = ctx_a.blake3_pass_ns()
        lens = A["us"]
        leaves, blocks = int(np.maximum((lens + 1023) // 1024, 1).sum()), int(np.maximum((lens + 63) // 64, 1).sum())
        floor = (blocks + leaves - n) / 64.0 / (4 * cus) * ns * 1e-6
        kn = "decode_small" if "decode_small" in ka else "copy_stored"
        v = ka.get(kn, float("nan"))
        print(f"  VALU floor {floor:.4f} ms ({ns:.1f} ns per pass per SIMD, {4 * cus} SIMDs) beside {kn} {v:.4f} ms = {total / v / 1e6:.0f} GB/s written"
              f"  -> {'below the floor' if v < floor else 'NOT below the floor'}")
    for r in rts:
        r.close()
    del A, outs
    torch.cuda.empty_cache()
print("\nevery workload within its margin" if ok_all else "\nat least one workload MISSES its margin")
