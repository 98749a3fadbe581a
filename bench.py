#!/usr/bin/env python3
"""bench.py — BASELINE.json's headline metric on MI355X.

A "step" = one pass of the hot path over one rank's batch of index rows: decode-or-passthrough
+ BLAKE3 + verify of every row (the body of decompress.rs:L135-190 for the whole row range),
inputs (blob region, index columns) resident in HBM when the timed region starts.  A second
timed loop measures the write side (BLAKE3 + zstd encode of every Round, stream_packer.rs:L217-284).

Workload (config.workload): BASELINE configs[1] — 100,000 x 10,240-byte text chunks
(perf_bench.rs:L133-141).  The headline read leg decodes an archive of **libzstd level-19 frames**
(the nearest stand-in for what the reference's L19 codec hands the decoder; built in the untimed
setup); the archive this build's own encoder writes is decoded as a second, separately reported leg.

Steps are pipelined the way the read loop reports (after the loop, not per row, decompress.rs:L195-221):
step k+1 is queued before step k's counters are read (znippy_rows_results_lagged), so the host's
round trip is not inside a step.

Multi-GPU (one process per GPU, RCCL counter all-reduce per step, no payload exchange):
  --scaling weak    every rank owns a full copy of the workload (default: per-GPU work fixed)
  --scaling strong  ONE archive; the row cursor is split into per-rank ranges balanced by bytes
                    (znippy_amd.sharding.split_rows = decompress.rs:L104,L136 split over ranks)

A plain run sets up, warms up and times the headline read leg only, and prints the result line (metric, value, unit,
higher_is_better, dtype, ms_per_step and the configuration).  --full adds everything else: the oracle parity checks of
the write side, the decoded-bytes check of every read leg before timing, the own-archive and real-text read legs, the
write leg, table-build and single-shot times, per-kernel times, the roofline and the CPU baseline.

--dump-outputs DIR writes what the headline leg's last timed step returned to rank 0 (float32 / float64 .npy):
  counters.npy              the run's counters, COUNTER_KEYS order
  row_status.npy            per-row status (0 = verified)                    \\ all rows, or DUMP_ROWS of them drawn
  row_digests.npy           per-row BLAKE3 digest of the decoded bytes       / with np.random.default_rng(0), sorted
  decoded_bytes_sample.npy  decoded bytes at DUMP_BYTES positions: all of them, or sorted
                            np.random.default_rng(1).integers(0, bytes_per_gpu, DUMP_BYTES)
The inputs are generated from fixed seeds, so two builds run with the same arguments can be compared file for file.

    python bench.py --gpus 1 --steps 20 --warmup 3 [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
COUNTER_KEYS = ("total_chunks", "total_written_bytes", "verified_bytes", "corrupt_bytes", "corrupt_rows", "decode_errors")
DUMP_ROWS = 1 << 17   # --dump-outputs: at most 64 MB in all (digests 16 MiB + status 0.5 MiB + bytes 16 MiB)
DUMP_BYTES = 1 << 22
# A plain run's headline leg starts straight out of the CPU-bound set-up, where a few warm-up steps leave the timed ones
# ~9 % slow (--full times it after the other legs).  So its warm-up steps go on until this many seconds have passed; with
# several ranks it stays W steps, because every rank must run the same number of steps.
WARMUP_MIN_S = 0.25


def measured_traffic(kernel, workload):
    """HBM bytes per launch of `kernel` from the PMC passes recorded under profiles/ (rocprofv3 --pmc
    FETCH_SIZE and --pmc WRITE_SIZE in separate runs, FETCH_SIZE doubled per the gfx950 correction)."""
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
        return d.get(workload, {}).get(kernel)
    except (OSError, ValueError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3,
                    help="untimed steps before the timed ones (a plain one-process run goes on until WARMUP_MIN_S has passed)")
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--archive", choices=("libzstd19", "own"), default=None,
                    help="frames of the headline read leg (default: libzstd19 for c2, own otherwise)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-text-leg", action="store_true", help="skip the read_text_archive leg (non-periodic text frames)")
    ap.add_argument("--headline-only", action="store_true",
                    help="run only the headline read leg and the write leg (a profiler's per-kernel averages then "
                         "describe the headline leg alone: the other read legs launch the same kernels)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline leg: parity checks, the other read legs, the write leg, table-build and "
                         "single-shot times, per-kernel times, roofline, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the headline leg's last timed step's results to DIR/<name>.npy")
    args = ap.parse_args()
    full = args.full

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N")
    # one process per GPU; ZNIPPY_BENCH_BACKEND=gloo lets several ranks share one card to rehearse the N>1 path
    backend = os.environ.get("ZNIPPY_BENCH_BACKEND", "nccl")
    dev = local_rank if backend == "nccl" else local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(dev)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
        else:
            dist.init_process_group(backend)

    import gen
    import workloads
    from oracle import oracle as O  # checker + cpu_baseline leg only
    from znippy_amd import hip
    from znippy_amd.sharding import split_rows

    lay = workloads.layout(args.workload)
    lens, skip = lay["lens"], lay["skip"]
    n = len(lens)
    total_in = int(lens.sum())
    src_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    ctx = hip.Context(dev)
    archive_kind = args.archive or ("libzstd19" if args.workload in ("c2", "c2small") else "own")
    if archive_kind == "libzstd19" and args.workload not in ("c2", "c2small"):
        raise SystemExit("--archive libzstd19 is built for the c2 workloads only (one chunk, compressed once, tiled)")

    # this rank's share of the row cursor / of the Rounds
    if args.scaling == "strong" and world > 1:
        r0, r1 = split_rows(lens, world)[rank]
    else:
        r0, r1 = 0, n
    my_rows = r1 - r0
    my_bytes = int(lens[r0:r1].sum())
    # the staging buffer: the whole workload (weak scaling: every rank owns a copy), or this rank's share of it only
    # (strong scaling: ONE workload, nobody builds bytes that belong to another rank's rows)
    base = int(src_off[r0]) if my_rows else 0
    wl = workloads.build(args.workload, torch, (base, base + my_bytes) if (args.scaling == "strong" and world > 1) else None)
    d_src, base = wl["d_src"], wl["base"]
    rel = (src_off - np.uint64(base)).astype(np.uint64)  # offsets into d_src (meaningful for this rank's rows)

    # ---- write side: this rank's Rounds over the resident staging buffer (a plain run needs it only to make the
    # archive of an "own" headline leg) ----
    archives = {}
    if full or archive_kind == "own":
        t0 = time.perf_counter()
        rounds = hip.RoundTable(ctx, rel[r0:r1], lens[r0:r1], None if skip is None else skip[r0:r1])
        round_table_ms = (time.perf_counter() - t0) * 1e3  # the context's first table: includes its device-memory pools
        # warm = what a context that has built and released a table of this shape before pays (its pools hold the buffers:
        # the host pipelines build and drop one table per hand-off); best of three
        round_table_warm_ms = None
        for _ in range(4 if full else 0):
            t0 = time.perf_counter()
            _rt2 = hip.RoundTable(ctx, rel[r0:r1], lens[r0:r1], None if skip is None else skip[r0:r1])
            dt_ = (time.perf_counter() - t0) * 1e3
            _rt2.close()
            if _ > 0:
                round_table_warm_ms = dt_ if round_table_warm_ms is None else min(round_table_warm_ms, dt_)
        d_blob = torch.zeros(rounds.blob_bound() + 64, dtype=torch.uint8, device="cuda")
        enc = rounds.encode_hash(d_src, d_blob)
        enc = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in enc.items()}
        # parity spot checks against the oracle: digests and frames of a few rounds
        for i in sorted({0, my_rows // 2, my_rows - 1}) if full else ():
            g = r0 + i
            src_i = d_src[int(rel[g]):int(rel[g] + lens[g])].cpu().numpy()
            assert enc["checksum"][i].tobytes() == O.blake3(src_i), "GPU write-side digest != oracle"
            f = d_blob[int(enc["blob_offset"][i]):int(enc["blob_offset"][i] + enc["blob_size"][i])].cpu().numpy()
            if enc["compressed"][i]:
                assert O.zstd_decompress(f.tobytes()) == src_i.tobytes(), "GPU frame does not decode on the oracle"
            else:
                assert f.tobytes() == src_i.tobytes()

        # ---- the archives the read legs decode ----
        own = dict(d_blobs=d_blob, bo=enc["blob_offset"], bs=enc["blob_size"], comp=enc["compressed"], ck=enc["checksum"],
                   label="gpu-encoded (this build's zstd frames)")
        archives["own"] = own
    if archive_kind == "libzstd19":
        sz = int(lens[0])
        chunk = gen.text(sz)
        frame = np.frombuffer(workloads.libzstd_compress(chunk, 19), dtype=np.uint8)  # every C2 chunk is this chunk (system libzstd)
        fl = len(frame)
        archives["libzstd19"] = dict(
            d_blobs=torch.from_numpy(np.concatenate([np.tile(frame, my_rows), np.zeros(64, np.uint8)])).cuda(),
            bo=np.arange(my_rows, dtype=np.uint64) * fl, bs=np.full(my_rows, fl, np.uint64),
            comp=np.ones(my_rows, np.uint8), ck=np.tile(np.frombuffer(O.blake3(chunk), dtype=np.uint8), (my_rows, 1)),
            label=f"libzstd level-19 frames ({fl} B per 10 KiB chunk; stand-in for the reference's L19 codec output)")
    my_lens = lens[r0:r1]
    out_off = (src_off[r0:r1] - src_off[r0]).astype(np.uint64)
    d_out = torch.zeros(my_bytes + 64, dtype=torch.uint8, device="cuda")
    d_src_mine = d_src[int(rel[r0]):int(rel[r0]) + my_bytes] if my_rows else d_src[:0]

    def cpu_read_loop(A, rows, out_offsets, lens_, nbytes):
        """The oracle's read loop (libzstd decode + scalar C BLAKE3 per row, decompress.rs:L135-190) on the host cores: best of
        three passes over the same rows (the first pass pays thread start-up and page faults of the output buffer)."""
        cores = len(os.sched_getaffinity(0))
        threads = max(1, int(np.ceil(0.9 * cores)))  # common_config.rs:L34 rule on what we can see
        host_blobs = A["d_blobs"].cpu().numpy()
        bitmap = np.packbits(A["comp"].astype(bool), bitorder="little")
        host_out = np.zeros(nbytes, dtype=np.uint8)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            st, _c = O.decompress_rows(host_blobs, A["bo"], A["bs"], lens_, out_offsets, bitmap, A["ck"], 0, rows,
                                       out=host_out, n_threads=threads, use_libzstd=O.have_libzstd())
            dt = time.perf_counter() - t0
            assert st["verified_bytes"] == nbytes
            best = dt if best is None else min(best, dt)
        return dict(value=round(nbytes / 2**20 / best, 1), unit="MB/s", cores=threads, kind="port",
                    sample=f"all {rows} rows of the same archive, best of 3 passes: oracle read loop (libzstd decode + scalar C "
                           f"BLAKE3, not SIMD), {threads} threads of {cores} visible cores")

    def text_archive(rows, chunk):
        """BASELINE configs[1]'s shape with REAL text in place of the 45-byte phrase: `rows` chunks of `chunk` bytes cut from
        source text found in the image (seeded word soup where the image has none), libzstd level-19 frames — Huffman
        literals, described FSE tables, ~800 sequences per chunk: nothing the periodic-shape recogniser can take.
        4,096 distinct chunks, tiled; every row owns its own copy of its frame in the blob region."""
        from concurrent.futures import ThreadPoolExecutor
        distinct = min(rows, 4096)
        raw = b"".join(workloads.image_corpus("text", distinct * chunk + (1 << 20), whole_files=False))
        if len(raw) < distinct * chunk:
            raw += gen.pseudo_text(distinct * chunk - len(raw), seed=11)
        sl = [raw[i * chunk:(i + 1) * chunk] for i in range(distinct)]
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:  # (libzstd releases the GIL inside ctypes calls)
            fr = list(ex.map(lambda x: workloads.libzstd_compress(x, 19), sl))
        idx = np.arange(rows) % distinct
        fl = np.array([len(f) for f in fr], np.uint64)
        bs_ = fl[idx]
        bo_ = np.concatenate([[0], np.cumsum(bs_)[:-1]]).astype(np.uint64)
        blob = np.frombuffer(b"".join(fr[i] for i in idx) + bytes(64), dtype=np.uint8)
        dig = np.stack([np.frombuffer(O.blake3(x), dtype=np.uint8) for x in sl])
        src_t = torch.from_numpy(np.frombuffer(b"".join(sl), dtype=np.uint8).copy()).cuda().view(distinct, chunk)
        return dict(d_blobs=torch.from_numpy(blob.copy()).cuda(), bo=bo_, bs=bs_, comp=np.ones(rows, np.uint8), ck=dig[idx],
                    label=f"libzstd level-19 frames of real text chunks ({distinct} distinct, mean {float(fl.mean()):.0f} B per {chunk} B chunk)",
                    src=src_t, idx=torch.from_numpy(idx).cuda(), distinct=distinct)

    def make_rows(a):
        t0 = time.perf_counter()
        rt = hip.RowTable(ctx, a["bo"], a["bs"], my_lens, out_off, np.packbits(a["comp"].astype(bool), bitorder="little"), a["ck"])
        first = (time.perf_counter() - t0) * 1e3
        bm = np.packbits(a["comp"].astype(bool), bitorder="little")
        warm = None  # further tables of the same archive, each released before the next: the pools hold the buffers; best of three
        for k in range(4 if full else 0):
            t0 = time.perf_counter()
            rt2 = hip.RowTable(ctx, a["bo"], a["bs"], my_lens, out_off, bm, a["ck"])
            dt_ = (time.perf_counter() - t0) * 1e3
            rt2.close()
            if k > 0:
                warm = dt_ if warm is None else min(warm, dt_)
        return rt, (first, warm)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    cvec = torch.zeros(8, dtype=torch.int64, device="cuda")
    hvec = torch.zeros(8, dtype=torch.int64).pin_memory() if world > 1 else None
    comm_stream = torch.cuda.Stream() if world > 1 else None  # the reduce never sits in front of the next pass

    def reduce_counters(counters):
        """The only cross-GPU traffic: one small all-reduce of the counters (RCCL over xGMI), on its own stream."""
        if world > 1:
            comm_stream.synchronize()  # the previous step's reduce is done with hvec / cvec
            for i, k in enumerate(COUNTER_KEYS):
                hvec[i] = counters[k]
            with torch.cuda.stream(comm_stream):
                cvec.copy_(hvec, non_blocking=True)
                dist.all_reduce(cvec)

    class ReadLeg:
        def __init__(self, a):
            self.a = a
            self.rows, self.table_ms = make_rows(a)
            self.pending = 0
            self.last = None
            self.bad_steps = 0  # steps whose counters were not "every byte verified" (checked on the host, off the GPU's path)

        def _take(self, c):
            self.last = c
            if c["corrupt_rows"] or c["decode_errors"] or c["verified_bytes"] != my_bytes:
                self.bad_steps += 1
            reduce_counters(c)

        def step(self):  # queue run k+1, then read run k
            self.rows.decode_verify_async(self.a["d_blobs"], d_out)
            if self.pending:
                self._take(self.rows.results_lagged(1))
            self.pending = 1

        def drain(self):
            if self.pending:
                self._take(self.rows.results_lagged(0))
                self.pending = 0

    class WriteLeg:
        def __init__(self):
            self.pending = 0
            self.last = None

        def step(self):
            rounds.encode_hash_async(d_src, d_blob)
            if self.pending:
                self.last = rounds.results_lagged(1)
            self.pending = 1

        def drain(self):
            if self.pending:
                self.last = rounds.results_lagged(0)
                self.pending = 0

    # HIP events in the timed region: around the dominant read kernels (decode_verify_*) for the small-row workloads —
    # a pair around every one of the step's near-empty follow-up launches costs the stream ~30 us of markers per step
    # (tools/ab_ktime.sh) — around every kernel otherwise (the dominant kernel of c3/c4store/c5 is not a decode_verify_* one)
    timed_level = 1 if args.workload in ("c2", "c2small") else 2

    def timed(leg, steps, warmup, after=None):
        ctx.set_kernel_timing(timed_level)
        t0, k = time.perf_counter(), 0
        while k < warmup or (not full and world == 1 and time.perf_counter() - t0 < WARMUP_MIN_S):
            leg.step()
            k += 1
        leg.drain()
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            leg.step()
        leg.drain()
        barrier()
        dt = time.perf_counter() - t0
        if after is not None:  # before any further step overwrites what the last timed step returned
            after(leg)
        # per-kernel durations (HIP events the library records around each launch on its own streams): read back in
        # a few extra, untimed steps so that the event queries are not part of the timed region
        ktimes = {}
        ctx.set_kernel_timing(2)
        for _ in range(min(steps, 10) if full else 0):
            leg.step()
            leg.drain()
            for name, ms in ctx.kernel_times():
                ktimes.setdefault(name, []).append(ms)
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()), {k: float(np.mean(v)) for k, v in ktimes.items()}

    def dump_outputs(leg):
        """--dump-outputs: the results the headline leg's last timed step handed this rank (see the module docstring)."""
        if args.dump_outputs is None or rank != 0:
            return
        os.makedirs(args.dump_outputs, exist_ok=True)
        _c, _corrupt, status = leg.rows.results()
        rows = np.arange(my_rows) if my_rows <= DUMP_ROWS else np.sort(
            np.random.default_rng(0).choice(my_rows, DUMP_ROWS, replace=False))
        pos = np.arange(my_bytes) if my_bytes <= DUMP_BYTES else np.sort(
            np.random.default_rng(1).integers(0, my_bytes, DUMP_BYTES))
        sample = d_out[torch.from_numpy(pos.astype(np.int64)).to(d_out.device)].cpu().numpy()
        for name, a in (("counters", np.array([leg.last[k] for k in COUNTER_KEYS], np.float64)),
                        ("row_status", status[rows].astype(np.float32)),
                        ("row_digests", leg.rows.digests()[rows].astype(np.float32)),
                        ("decoded_bytes_sample", sample.astype(np.float32))):
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a)

    # ---- read side (the headline) ----
    if args.headline_only or not full:
        args.no_text_leg = True
        archives = {archive_kind: archives[archive_kind]}
    legs = {k: ReadLeg(a) for k, a in archives.items()}
    for k, leg in legs.items() if full else ():  # correctness of each archive's decode before anything is timed
        d_out.zero_()
        leg.step()
        leg.drain()
        c = leg.last
        assert c["corrupt_rows"] == 0 and c["decode_errors"] == 0 and c["verified_bytes"] == my_bytes, (k, c)
        assert torch.equal(d_out[:my_bytes], d_src_mine), f"decoded bytes differ from the source ({k})"
    head = legs[archive_kind]
    text = None
    if args.workload in ("c2", "c2small") and not args.no_text_leg:
        text = text_archive(my_rows, int(lens[0]))
        archives["text"] = text
        tleg = ReadLeg(text)
        d_out.zero_()
        tleg.step(); tleg.drain()
        c = tleg.last
        assert c["corrupt_rows"] == 0 and c["decode_errors"] == 0 and c["verified_bytes"] == my_bytes, ("text", c)
        got = d_out[:my_bytes].view(my_rows, int(lens[0]))
        for lo_ in range(0, my_rows, text["distinct"]):  # every row's bytes against its chunk
            hi_ = min(lo_ + text["distinct"], my_rows)
            assert torch.equal(got[lo_:hi_], text["src"][:hi_ - lo_]), "decoded text rows differ from the source"
        legs["text"] = tleg
    # Order of the legs: the secondary read leg (own-encoder archive) first, the headline leg after it.  Each leg has
    # exactly W warmup + K timed steps; whichever runs first comes straight out of the CPU-bound set-up and measures
    # ~4 % slow with W = 3 (the two archives decode at the same speed when their runs are interleaved in one process,
    # tools/ab_frames.py: 0.475 vs 0.480 ms) — the sustained rate is the one that describes the path.
    dt_own, k_own = timed(legs["own"], args.steps, args.warmup) if archive_kind != "own" and "own" in legs else (None, None)
    dt_read, k_read = timed(head, args.steps, args.warmup, after=dump_outputs)
    if dt_own is None:
        dt_own, k_own = dt_read, k_read
    dt_write, k_write = timed(WriteLeg(), args.steps, args.warmup) if full else (None, None)
    dt_text, k_text = timed(legs["text"], args.steps, args.warmup) if text is not None else (None, None)
    # single shot (an archive is decoded once): table construction + ONE run + its results, blobs resident, index columns
    # in host memory as the reader leaves them; best of three
    def single_shot_read(a):
        bm = np.packbits(a["comp"].astype(bool), bitorder="little")
        best = None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rt_ = hip.RowTable(ctx, a["bo"], a["bs"], my_lens, out_off, bm, a["ck"])
            c_, _corrupt, _status = rt_.decode_verify(a["d_blobs"], d_out)
            dt_ = (time.perf_counter() - t0) * 1e3
            rt_.close()
            assert c_["corrupt_rows"] == 0 and c_["verified_bytes"] == my_bytes
            best = dt_ if best is None else min(best, dt_)
        return best

    def single_shot_write():
        best = None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rd_ = hip.RoundTable(ctx, rel[r0:r1], lens[r0:r1], None if skip is None else skip[r0:r1])
            e_ = rd_.encode_hash(d_src, d_blob)
            dt_ = (time.perf_counter() - t0) * 1e3
            rd_.close()
            assert int(e_["blob_size"].sum()) > 0
            best = dt_ if best is None else min(best, dt_)
        return best
    ctx.set_kernel_timing(timed_level)  # as in the timed steps (the kernel-time collection above brackets every kernel)
    ss_read = None if args.headline_only or not full else single_shot_read(archives[archive_kind])
    ss_write = single_shot_write() if full else None
    for k, leg in legs.items():  # every step of every read leg (warmup, timed, kernel-time collection) verified every byte
        assert leg.bad_steps == 0, f"{leg.bad_steps} steps of the {k} read leg did not verify"

    total_bytes = total_in * world if args.scaling == "weak" else total_in
    mbps = lambda dt: total_bytes / 2**20 / (dt / args.steps)

    if rank == 0:
        # roofline of the dominant read-side kernel, algorithmic bytes per launch (read each
        # blob byte, write each output byte, the index columns)
        A = archives[archive_kind]
        blob_bytes = int(A["bs"].sum())
        path_alg = blob_bytes + my_bytes + 57 * my_rows
        alg = {
            "decode_verify_fused": path_alg,             # one launch does the whole path for small rows
            "decode_verify_roles": path_alg,
            "zstd_decode_general": path_alg,
            "zstd_decode_blocks": path_alg,              # block items: same bytes, one work item per block
            "decode_verify_fused_blocks": path_alg,      # block items written + hashed in one go
            "blake3_second_pass": my_bytes + 32 * my_rows + (0 if skip is None else my_bytes),  # read (+ copy on the store path)
        }
        # (a launch that only waits for CUs while the other stream's kernel runs — the general decoder with nothing
        # routed to it — is not a candidate: its interval measures its neighbour)
        idle = {"zstd_decode_general"} if "decode_verify_fused_blocks" in k_read else set()
        dom = max((k for k in k_read if k in alg and k not in idle), key=lambda k: k_read[k]) if k_read else None
        roofline = None
        if dom:
            ach = alg[dom] / (k_read[dom] * 1e-3) / 1e9
            path_ms = sum(k_read.values())
            roofline = dict(bound="hbm", kernel=dom, achieved=round(ach, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                            frac=round(ach / HBM_PEAK_GBS, 4), traffic=None,
                            kernel_ms={k: round(v, 4) for k, v in k_read.items()},
                            path_achieved=round(path_alg / (path_ms * 1e-3) / 1e9, 1),
                            path_frac=round(path_alg / (path_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4))
            tr = measured_traffic(dom, args.workload)
            if tr is not None:
                roofline["traffic"] = tr
            # What actually limits the kernel: the HBM roofline is what `frac` is priced against, but
            # a decompress+VERIFY pass hashes every output byte, and BLAKE3 is integer VALU work.  Its floor =
            # (64-lane compress passes the step needs per SIMD) x (measured ns per pass per SIMD with nothing else
            # running).  Passes = (leaf block compressions + parent nodes) / 64 — every lane of every pass busy, the
            # bound no lane packing can beat.
            try:
                ns_pass = ctx.blake3_pass_ns()
                leaves = int(np.maximum((my_lens + 1023) // 1024, 1).sum())
                blocks = int(np.maximum((my_lens + 63) // 64, 1).sum())      # 64-byte compressions of the leaves
                passes = (blocks + (leaves - my_rows)) / 64.0                # + one per parent node; every lane busy
                floor_ms = passes / 1024.0 * ns_pass * 1e-6
                roofline["limiter"] = "valu"
                # what the 0.40 target is to be read against: the fraction of the HBM roofline the step would reach if the
                # dominant kernel ran AT the integer-VALU floor of its BLAKE3 passes (nothing but the hash, every lane busy)
                roofline["ceiling_frac"] = round(alg[dom] / (floor_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                roofline["valu"] = dict(floor_ms=round(floor_ms, 4), frac_of_floor=round(floor_ms / k_read[dom], 4),
                                        ns_per_pass_per_simd=round(ns_pass, 1), passes_per_step=round(passes, 0),
                                        note="BLAKE3 compress passes (64 lanes) per step / 1024 SIMDs x measured ns per pass")
            except Exception as e:  # the hook is diagnostic: never fail the bench over it
                roofline["valu"] = dict(error=str(e))
        cpu = None
        if full and not args.no_cpu_baseline and world == 1:
            cpu = cpu_read_loop(A, my_rows, out_off, my_lens, my_bytes)
        text_leg = None
        if text is not None:
            t_blob = int(text["bs"].sum())
            t_alg = t_blob + my_bytes + 57 * my_rows  # every blob byte read, every output byte written, the index columns
            t_ms = dt_text / args.steps * 1e3
            stage = {k: v for k, v in k_text.items() if k.startswith("zstd_batch_")}
            t_dom = max(stage, key=stage.get) if stage else None
            text_leg = {"archive": text["label"], "MBps": round(mbps(dt_text), 1), "GBps": round(total_bytes / (dt_text / args.steps) / 1e9, 2),
                        "ms_per_step": round(t_ms, 4), "blob_bytes_per_gpu": t_blob,
                        "kernel_ms": {k: round(v, 4) for k, v in k_text.items()},
                        "roofline": dict(bound="hbm", kernel=t_dom, achieved=round(t_alg / (t_ms * 1e-3) / 1e9, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                                         frac=round(t_alg / (t_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), traffic=None,
                                         note="the leg is a chain of six kernels (scan, tables, Huffman streams, sequences, execute, hash): "
                                              "achieved = algorithmic bytes / step time; `kernel` = the longest of them; limiter: serial "
                                              "entropy chains (lane = block), not memory"),
                        "cpu_baseline": cpu_read_loop(text, my_rows, out_off, my_lens, my_bytes) if (not args.no_cpu_baseline and world == 1) else None}
        line = {
            "metric": "decompress MB/s (uncompressed) + compress MB/s, 100k x 10KB archive",
            "value": round(mbps(dt_read), 1), "unit": "MB/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt_read / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "u8",
            "data": "synthetic",
            "config": {"workload": wl["name"], "rows_per_gpu": my_rows, "chunk_bytes": int(lens[0]),
                       "bytes_per_gpu": my_bytes, "blob_bytes_per_gpu": blob_bytes, "archive": A["label"],
                       "parallelism": f"row-cursor ranges x{world}",
                       "pipelining": "step k+1 queued before step k's counters are read (two runs in flight)"},
        }
        if full:
            line.update({
                "read_own_archive": {"archive": own["label"], "MBps": round(mbps(dt_own), 1),
                                     "ms_per_step": round(dt_own / args.steps * 1e3, 4),
                                     "blob_bytes_per_gpu": int(own["bs"].sum()),
                                     "kernel_ms": {k: round(v, 4) for k, v in k_own.items()}},
                "compress_level": int(ctx.level),  # CONFIG.compression_level = 19 unless ZNIPPY_LEVEL says otherwise: the higher effort tier
                "compress_MBps": round(mbps(dt_write), 1),
                "compress_ms_per_step": round(dt_write / args.steps * 1e3, 4),
                "compress_kernel_ms": {k: round(v, 4) for k, v in k_write.items()},
                "table_build_ms": {"row_table": round(head.table_ms[1], 3), "round_table": round(round_table_warm_ms, 3),
                                   "row_table_first": round(head.table_ms[0], 3), "round_table_first": round(round_table_ms, 3),
                                   "note": "host passes + H2D of the index columns / Rounds (the encoder plan is built on the device), outside the timed steps; best of three with the context's pools warm (a table of this shape was built and released before); *_first = the context's first table (its memory pools are created)"},
                "single_shot_ms": {"read": None if ss_read is None else round(ss_read, 3), "write": round(ss_write, 3),
                                   "note": "table construction + one run + its results (synchronous), blobs / staging buffer resident, index columns / Rounds in host memory; best of three"},
                "read_text_archive": text_leg,
                "roofline": roofline, "cpu_baseline": cpu,
            })
        print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
