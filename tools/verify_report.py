"""Verify-only step against the decode step, workload by workload, in one process: side A is this build's verify run
(znippy_verify_rows), side B the decode run of another build of the library (ZN_LIB_B=path/to/libznippy_hip.so — the parent
commit's; without it, this build's own decode run), loaded the way tools/ab_tree.py loads its second side.  The two run in
turn (the order changes every pair), tables warm, lean where they can be; a step is queue + results, by the wall clock with the
device idle in front.  Condition: a verify run does a subset of a decode run's work, so verify <= decode x 1.02 (twice the
~1 % the interleaved A/B resolves).

Usage: [ZN_LIB_B=...] python tools/verify_report.py [workloads=c2,c3,c4store,c4codec,c5,c2store,text] [pairs=12]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, gen, workloads
from znippy_amd import _build, _lib, hip

names = (sys.argv[1] if len(sys.argv) > 1 else "c2,c3,c4store,c4codec,c5,c2store,text").split(",")
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 12
MARGIN = 1.02

ctx_a = hip.Context(0)
lib_b = os.environ.get("ZN_LIB_B")
if lib_b:  # the decode side from another build of the library
    so_a = _build.SO
    _lib._lib = None
    _build.SO = os.path.abspath(lib_b)
ctx_b = hip.Context(0)
if lib_b:
    _lib._lib = None
    _build.SO = so_a
print(f"A = verify run of {os.path.relpath(_lib.lib_path(), ROOT)}   B = decode run of {lib_b if lib_b else 'the same library'}   pairs {pairs}")
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
    rounds = hip.RoundTable(ctx_a, offs, lens, wl["skip"])
    d_blob = torch.zeros(rounds.blob_bound() + 64, dtype=torch.uint8, device="cuda")
    enc = rounds.encode_hash(wl["d_src"], d_blob)
    enc = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in enc.items()}
    rounds.close()
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
    rt_a = hip.RowTable(ctx_a, A["bo"], A["bs"], A["us"], None, bitmap, A["ck"])
    rt_b = hip.RowTable(ctx_b, A["bo"], A["bs"], A["us"], oo, bitmap, A["ck"])
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    sides = ((ctx_a, lambda: rt_a.verify_async(A["d_blobs"]), rt_a), (ctx_b, lambda: rt_b.decode_verify_async(A["d_blobs"], d_out), rt_b))
    t, kt = ([], []), ({}, {})
    for i in range(pairs + 3):
        for j in ((0, 1) if i % 2 == 0 else (1, 0)):
            dt, c, k = step(*sides[j])
            assert c["corrupt_rows"] == 0 and c["decode_errors"] == 0 and c["verified_bytes"] == total, (name, j, c)
            if i >= 3:
                t[j].append(dt)
                for kn, v in k.items():
                    kt[j].setdefault(kn, []).append(v)
    _, scratch_bytes, _ = rt_a.verify_scratch()
    va, vb = float(np.median(t[0])), float(np.median(t[1]))
    ka, kb = ({k: float(np.median(v)) for k, v in kt[j].items()} for j in (0, 1))
    ok = va <= vb * MARGIN
    ok_all &= ok
    print(f"\n{name}: {A['label']}  ({n} rows, {total / 2**20:.0f} MiB decoded, verify scratch {scratch_bytes / 2**20:.0f} MiB)")
    print(f"  step ms (median of {pairs}): verify {va:.4f}  decode {vb:.4f}  ratio {va / vb:.3f}  -> {'ok' if ok else 'MISSES'} (<= {MARGIN})")
    print(f"  kernel ms, sum: verify {sum(ka.values()):.4f}  decode {sum(kb.values()):.4f}")
    print("  verify kernels: " + "  ".join(f"{k} {v:.4f}" for k, v in ka.items()))
    print("  decode kernels: " + "  ".join(f"{k} {v:.4f}" for k, v in kb.items()))
    if name == "c2":  # the hash's VALU floor beside the role-split kernel (bench.py's pricing: every lane of every pass busy)
        ns = ctx_a.blake3_pass_ns()
        lens = A["us"]
        leaves, blocks = int(np.maximum((lens + 1023) // 1024, 1).sum()), int(np.maximum((lens + 63) // 64, 1).sum())
        floor = (blocks + leaves - n) / 64.0 / (4 * cus) * ns * 1e-6
        print(f"  VALU floor {floor:.4f} ms ({ns:.1f} ns per pass per SIMD, {4 * cus} SIMDs) beside verify_roles {ka.get('verify_roles', float('nan')):.4f} ms "
              f"(decode_verify_roles {kb.get('decode_verify_roles', float('nan')):.4f})")
    if name == "c4store":  # the hash-only rate beside the store path's hash + copy
        h, d = ka.get("blake3_hash_only"), kb.get("blake3_second_pass")
        if h and d:
            print(f"  blake3_hash_only {h:.4f} ms = {total / h / 1e6:.0f} GB/s hashed  beside blake3_second_pass (hash + copy) {d:.4f} ms = {total / d / 1e6:.0f} GB/s")
    rt_a.close(); rt_b.close()
    del A, d_out
    torch.cuda.empty_cache()
print("\nall workloads within the margin" if ok_all else "\nat least one workload MISSES the margin")
