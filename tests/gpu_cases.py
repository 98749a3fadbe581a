"""Builders and run bodies the GPU test modules share (not a test module: pytest does not collect it, so a test module
that imports from here does not collect another module's tests a second time).  Archives are built by the oracle's
write loop or by the container's libzstd; every run goes through the C ABI (znippy_amd.hip)."""
import glob
import os

import numpy as np

import gen
import workloads


def make_ctx(env):
    """A context created with `env` set in the environment (switches are read at context creation), the environment
    restored afterwards."""
    from znippy_amd import hip
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return hip.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ---- own archives (the oracle's write loop) -------------------------------------------------------------------------

def build_archive(oracle, entries, level=19, skip=None):
    """entries: list of bytes; returns dict of index columns + blob region (oracle write loop)."""
    src = np.frombuffer(b"".join(entries) + b"\0" * 16, dtype=np.uint8)
    lens = np.array([len(e) for e in entries], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    skip = np.zeros(len(entries), dtype=np.uint8) if skip is None else np.asarray(skip, dtype=np.uint8)
    r = oracle.compress_rounds(src, offs, lens, skip, level=level, n_threads=1)
    r["usize"] = lens
    r["out_off"] = offs
    r["src"] = src
    return r


def run_gpu(gpu_ctx, arch, pad_blobs=0, rt=None):
    """One run of `arch` on a table of gpu_ctx (a new one, or `rt` again): counters, corrupt list, status, bytes, table."""
    import torch
    from znippy_amd import hip
    blobs = np.concatenate([np.zeros(pad_blobs, np.uint8), arch["blobs"], np.zeros(32, np.uint8)])
    d_blobs = torch.from_numpy(blobs).cuda()
    total = int(arch["usize"].sum())
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    bitmap = np.packbits(arch["compressed"].astype(bool), bitorder="little")
    if rt is None:
        rt = hip.RowTable(gpu_ctx, arch["blob_offset"] + np.uint64(pad_blobs), arch["blob_size"], arch["usize"],
                          arch["out_off"], bitmap, arch["checksum"])
    counters, corrupt, status = rt.decode_verify(d_blobs, d_out)
    return counters, corrupt, status, d_out.cpu().numpy()[:total], rt


def oracle_rows(oracle, arch, extent=None, fill=0):
    """The oracle's read loop over the whole archive: (counters, corrupt list, output bytes).  extent / fill: size and
    initial value of the output image, for archives whose rows do not lie back to back from 0."""
    n = len(arch["usize"])
    bitmap = np.packbits(arch["compressed"].astype(bool), bitorder="little")
    want_out = np.full(int(arch["usize"].sum()) if extent is None else int(extent), fill, dtype=np.uint8)
    want, want_corrupt = oracle.decompress_rows(arch["blobs"], arch["blob_offset"], arch["blob_size"], arch["usize"],
                                                arch["out_off"], bitmap, arch["checksum"], 0, n, out=want_out)
    return want, want_corrupt, want_out


def random_archive(oracle, seed, n_rows=2500):
    """Randomised archive — whole-leaf and ragged rows, text / binary / word-soup / incompressible / empty, stored and
    compressed, runs of equal rows and single ones, three big rows, ~1 in 40 rows damaged (one bit of the blob)."""
    rng = np.random.default_rng(1000 + seed)
    entries, skip = [], []
    while len(entries) < n_rows:
        kind = int(rng.integers(0, 8))
        run = int(rng.integers(1, 30)) if rng.random() < 0.5 else 1
        n = int(rng.choice([0, 1, 1023, 1024, 1025, 4096, 10240, 10240, 10240, 20480, 30720, 65536, int(rng.integers(2, 50000))]))
        if kind <= 1: e = gen.text(n)
        elif kind == 2: e = gen.binary(n)
        elif kind == 3: e = gen.pseudo_text(min(n, 20000), seed=len(entries))
        elif kind == 4: e = gen.incompressible(len(entries), min(n, 30000))
        elif kind == 5: e = bytes(n)
        else: e = gen.text(n)
        for _ in range(run):
            entries.append(e)
            skip.append(1 if kind == 4 and len(entries) % 3 == 0 else 0)
    for big, sk in ((gen.text(700_000), 0), (gen.incompressible(9, 400_000), 1), (gen.pseudo_text(300_000, seed=5), 0)):
        at = int(rng.integers(0, len(entries)))
        entries.insert(at, big); skip.insert(at, sk)
    arch = build_archive(oracle, entries, level=3, skip=skip)
    n = len(entries)
    blobs = arch["blobs"].copy()
    for i in rng.choice(n, size=n // 40, replace=False):       # damage: one byte somewhere in the row's blob
        if arch["blob_size"][i] > 0:
            at = int(arch["blob_offset"][i]) + int(rng.integers(0, int(arch["blob_size"][i])))
            blobs[at] ^= 1 << int(rng.integers(0, 8))
    arch["blobs"] = blobs
    return arch


def check_random_archive_run(arch, want, want_corrupt, want_out, counters, corrupt, status, out, rt, rep):
    """One run of a random archive against the oracle's read loop: counters, verdicts, sampled bytes, digests."""
    n = len(arch["usize"])
    assert counters == want, (rep, counters, want)
    assert sorted(int(x) for x in corrupt) == sorted(int(x) for x in want_corrupt), rep
    okrows = status >= 0
    assert int((~okrows).sum()) == want["decode_errors"]
    for i in np.nonzero(okrows)[0][:: max(1, n // 400)]:    # bytes of a sample of the decoded rows (all digests below)
        a, b = int(arch["out_off"][i]), int(arch["out_off"][i] + arch["usize"][i])
        assert np.array_equal(out[a:b], want_out[a:b]), (rep, int(i))
    good = okrows.copy(); good[[int(x) for x in want_corrupt]] = False
    assert np.array_equal(rt.digests()[good], arch["checksum"][good]), rep


def mixed_archive_entries():
    """Compressed text/binary/pseudo-text rows of ragged sizes, stored (skip) rows, empty rows, a multi-block frame of
    > 64 leaves, a big stored row."""
    rng = np.random.default_rng(11)
    entries, skip = [], []
    for i in range(300):
        kind = i % 6
        n = int(rng.integers(0, 40000))
        if kind == 0: e = gen.text(n)
        elif kind == 1: e = gen.binary(n)
        elif kind == 2: e = gen.pseudo_text(n, seed=i)
        elif kind == 3: e = gen.incompressible(i, n)
        elif kind == 4: e = b""
        else: e = gen.pseudo_text(n * 4, seed=i)
        entries.append(e)
        skip.append(1 if kind == 3 and i % 2 else 0)
    entries.append(gen.pseudo_text(2 << 20, seed=77))   # multi-block frame, > 64 leaves
    skip.append(0)
    entries.append(gen.incompressible(5, 3 << 20))      # big stored row
    skip.append(1)
    return entries, skip


def random_round_entries(seed, n_rounds=500):
    """Randomised Round tables: every kind of content, block-boundary sizes, runs of equal rounds, some on the store path."""
    rng = np.random.default_rng(seed)
    entries, skip = [], []
    while len(entries) < n_rounds:
        kind = int(rng.integers(0, 7))
        run = int(rng.integers(1, 12)) if rng.random() < 0.4 else 1
        n = int(rng.choice([0, 1, 63, 1024, 4096, 10240, 10240, 16384, 16385, 20480, 131072, 131073, int(rng.integers(2, 300000))]))
        if kind <= 1: e = gen.text(n)
        elif kind == 2: e = gen.binary(n)
        elif kind == 3: e = gen.pseudo_text(min(n, 60000), seed=len(entries) + seed * 1000)
        elif kind == 4: e = gen.incompressible(len(entries) + seed, min(n, 200000))
        elif kind == 5: e = bytes(n)
        else: e = (gen.pseudo_text(min(n, 30000) // 2 + 1, seed=seed) + gen.incompressible(seed, min(n, 30000) // 2))[:n]
        for _ in range(run):
            entries.append(e); skip.append(1 if kind == 4 and len(entries) % 4 == 0 else 0)
    return entries, skip


# ---- foreign frames (the container's libzstd) -----------------------------------------------------------------------

def py_corpus(cap):
    """Real text: python sources of the image, in sorted order (deterministic on a given image)."""
    out, tot = [], 0
    for f in sorted(glob.glob("/usr/lib/python3.10/*.py")):
        try:
            b = open(f, "rb").read()
        except OSError:
            continue
        out.append(b)
        tot += len(b)
        if tot >= cap:
            break
    data = b"".join(out)
    if len(data) < cap:  # a bare image: fall back to the seeded word stream
        data += gen.pseudo_text(cap - len(data), seed=5)
    return data[:cap]


def mixed(n, seed):
    """Text with incompressible and constant stretches: raw and RLE blocks between compressed ones."""
    rng = np.random.default_rng(seed)
    parts, tot = [], 0
    while tot < n:
        k = int(rng.integers(0, 4))
        m = int(rng.integers(20000, 400000))
        if k == 0:
            p = rng.integers(0, 256, size=m, dtype=np.uint8).tobytes()
        elif k == 1:
            p = bytes([int(rng.integers(0, 256))]) * m
        else:
            p = gen.pseudo_text(m, seed=int(rng.integers(0, 1 << 30)))
        parts.append(p)
        tot += m
    return b"".join(parts)[:n]


def foreign_archive(oracle, entries, level):
    frames = [workloads.libzstd_compress(e, level) for e in entries]
    bs = np.array([len(f) for f in frames], np.uint64)
    bo = np.concatenate([[0], np.cumsum(bs)[:-1]]).astype(np.uint64)
    us = np.array([len(e) for e in entries], np.uint64)
    oo = np.concatenate([[0], np.cumsum(us)[:-1]]).astype(np.uint64)
    ck = np.stack([np.frombuffer(oracle.blake3(e), dtype=np.uint8) for e in entries])
    blobs = np.frombuffer(b"".join(frames) + bytes(64), dtype=np.uint8)
    return dict(blobs=blobs, bo=bo, bs=bs, us=us, oo=oo, ck=ck, frames=frames)


def run_foreign(ctx, A):
    import torch
    from znippy_amd import hip
    d_blobs = torch.from_numpy(A["blobs"].copy()).cuda()
    total = int(A["us"].sum())
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    rt = hip.RowTable(ctx, A["bo"], A["bs"], A["us"], A["oo"], None, A["ck"])
    first = None
    for rep in range(3):  # the work lists of the two-phase path are filled in a different order every run: every run must agree
        d_out.zero_()
        c, corrupt, status = rt.decode_verify(d_blobs, d_out)
        got = (dict(c), sorted(int(x) for x in corrupt), status.copy(), rt.digests()[status >= 0].copy(), d_out.cpu().numpy()[:total].copy())
        if first is None:
            first = got
        else:
            assert got[0] == first[0] and got[1] == first[1] and (got[2] == first[2]).all(), rep
            assert (got[3] == first[3]).all() and (got[4] == first[4]).all(), rep
    return c, corrupt, status, first[4], dict(ctx.kernel_times())


def frame_table(oracle, entries, frames):
    bs = np.array([len(f) for f in frames], np.uint64)
    bo = np.concatenate([[0], np.cumsum(bs)[:-1]]).astype(np.uint64)
    us = np.array([len(e) for e in entries], np.uint64)
    oo = np.concatenate([[0], np.cumsum(us)[:-1]]).astype(np.uint64)
    dig = {}
    for e in entries:
        if e not in dig:
            dig[e] = np.frombuffer(oracle.blake3(e), dtype=np.uint8)
    ck = np.stack([dig[e] for e in entries])
    blobs = np.frombuffer(b"".join(frames) + bytes(64), dtype=np.uint8)
    return dict(blobs=blobs, bo=bo, bs=bs, us=us, oo=oo, ck=ck)


def decode_table(ctx, A, reps=2, full=False):
    """full: the corrupt list and the digests of the last run are returned too."""
    import torch
    from znippy_amd import hip
    d_blobs = torch.from_numpy(A["blobs"].copy()).cuda()
    total = int(A["us"].sum())
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    rt = hip.RowTable(ctx, A["bo"], A["bs"], A["us"], A["oo"], None, A["ck"])
    outs, lists = [], []
    for _ in range(reps):  # work lists are filled in a different order every run: every run must agree
        d_out.zero_()
        c, corrupt, status = rt.decode_verify(d_blobs, d_out)
        outs.append((dict(c), status.copy(), d_out[:total].cpu().numpy().copy()))
        lists.append(sorted(int(x) for x in corrupt))
    for o in outs[1:]:
        assert o[0] == outs[0][0] and (o[1] == outs[0][1]).all() and (o[2] == outs[0][2]).all()
    res = outs[0] + (rt.foreign_stats(), dict(ctx.kernel_times()))
    if full:
        assert all(x == lists[0] for x in lists[1:])
        res += (lists[0], rt.digests().copy())
    return res


# ---- mutated frames -------------------------------------------------------------------------------------------------

def random_mutants(frame: bytes, rng, count):
    out = []
    n = len(frame)
    for i in range(count):
        b = bytearray(frame)
        kind = i % 5
        if kind == 0:                      # single bit flip
            p = int(rng.integers(0, n)); b[p] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:                    # random byte
            p = int(rng.integers(0, n)); b[p] = int(rng.integers(0, 256))
        elif kind == 2:                    # truncate
            b = b[:int(rng.integers(1, n))]
        elif kind == 3:                    # burst of 4 random bytes
            p = int(rng.integers(0, max(n - 4, 1)))
            for k in range(min(4, n - p)):
                b[p + k] = int(rng.integers(0, 256))
        else:                              # swap two bytes
            p, q = int(rng.integers(0, n)), int(rng.integers(0, n)); b[p], b[q] = b[q], b[p]
        out.append(bytes(b))
    return out


def fuzz_run(gpu_ctx, oracle, bases, per_base, seed, min_ok, min_rej, mutants=None):
    import torch
    from znippy_amd import hip
    rng = np.random.default_rng(seed)
    _m = mutants or random_mutants
    frames, sizes, originals = [], [], []
    for data, lvl in bases:
        f = oracle.libzstd_compress(data, lvl)
        g = gpu_ctx.compress(data)                       # this build's own frames too
        for base in (f, g):
            frames.append(base); sizes.append(len(data)); originals.append(data)   # the intact frame as control
            for m in _m(base, rng, per_base):
                frames.append(m); sizes.append(len(data)); originals.append(data)
    n = len(frames)
    bs = np.array([len(f) for f in frames], dtype=np.uint64)
    bo = np.concatenate([[0], np.cumsum(bs)[:-1]]).astype(np.uint64)
    us = np.array(sizes, dtype=np.uint64)
    oo = np.concatenate([[0], np.cumsum(us)[:-1]]).astype(np.uint64)
    ck = np.stack([np.frombuffer(oracle.blake3(d), dtype=np.uint8) for d in originals])
    d_blobs = torch.from_numpy(np.frombuffer(b"".join(frames) + bytes(64), dtype=np.uint8).copy()).cuda()
    d_out = torch.zeros(int(us.sum()) + 64, dtype=torch.uint8, device="cuda")
    rt = hip.RowTable(gpu_ctx, bo, bs, us, oo, None, ck)
    counters, corrupt, status = rt.decode_verify(d_blobs, d_out)
    out = d_out.cpu().numpy()
    corrupt = set(int(x) for x in corrupt)
    n_ok = n_rej = n_flagged = 0
    for i in range(n):
        try:
            want = oracle.zstd_decompress(frames[i], cap=sizes[i])
            oracle_ok = len(want) == sizes[i]
        except ValueError:
            oracle_ok = False
        got = out[int(oo[i]):int(oo[i] + us[i])].tobytes()
        if oracle_ok:
            assert status[i] == 0, (i, status[i])
            assert got == want, i
            assert (i in corrupt) == (want != originals[i]), i       # verify flags exactly the changed contents
            n_ok += 1
        elif status[i] < 0:
            n_rej += 1
        else:
            assert i in corrupt or got == originals[i], i            # never "verified" with wrong bytes
            n_flagged += 1
    assert counters["total_chunks"] == n and counters["decode_errors"] == int((status < 0).sum())
    assert n_ok >= min_ok and n_rej >= min_rej, (n_ok, n_rej)
    print(f"mutants: {n} rows, oracle-accepted {n_ok}, rejected by both {n_rej}, gpu-decoded-but-flagged {n_flagged}")


# ---- the small cases several modules run (oracle side: build once per module) -----------------------------------------

def random_case(oracle):
    arch = random_archive(oracle, seed=4, n_rows=900)
    return arch, oracle_rows(oracle, arch)


def mixed_case(oracle):
    entries, skip = mixed_archive_entries()
    arch = build_archive(oracle, entries, level=3, skip=skip)
    return arch, oracle_rows(oracle, arch)


def foreign_case(oracle):
    """libzstd -19 frames of real text: 10 KiB ones (batch path), 64-256 KiB ones and one above 256 KiB (resolve path),
    three of them damaged."""
    data = py_corpus(3 << 20)
    entries = [data[i * 10240:(i + 1) * 10240] for i in range(160)]
    entries += [data[2_000_000:2_000_000 + n] for n in (65_537, 100_000, 180_000, 262_143)] + [data[1_700_000:1_700_000 + 300_001]]
    frames = [workloads.libzstd_compress(e, 19) for e in entries]
    A = frame_table(oracle, entries, frames)
    blobs = A["blobs"].copy()
    rng = np.random.default_rng(8)
    for i in (17, 161, 164):
        blobs[int(A["bo"][i]) + int(rng.integers(8, int(A["bs"][i]) - 4))] ^= 0x5A
    A["blobs"] = blobs
    arch = dict(blobs=blobs, blob_offset=A["bo"], blob_size=A["bs"], usize=A["us"], out_off=A["oo"], checksum=A["ck"],
                compressed=np.ones(len(entries), np.uint8))
    return arch, oracle_rows(oracle, arch)


def store_case(oracle):
    """No compressed row: ragged rows, 64-leaf rows, a 64-leaf row queued beside a big row's first slice (both 64-leaf
    units of different kinds), odd output offsets, one damaged row."""
    rng = np.random.default_rng(31)
    sizes = [65536, 200_000, 65536, 65536, 65537, 3 * 65536, 65536, (1 << 20) + 1] + [int(x) for x in rng.integers(0, 30000, 120)]
    sizes += [10240] * 40 + [0, 1, 15, 16, 17, 1023, 1024, 1025]
    rows = [gen.incompressible(900 + i, n) for i, n in enumerate(sizes)]
    out_off, pos = [], 5
    for n in sizes:
        out_off.append(pos)
        pos += n + 3                                  # odd offsets, 3 guard bytes between rows
    blobs = np.frombuffer(b"".join(rows) + bytes(64), dtype=np.uint8).copy()
    bs = np.array(sizes, dtype=np.uint64)
    bo = (np.cumsum(bs) - bs).astype(np.uint64)
    ck = np.stack([np.frombuffer(oracle.blake3(d), dtype=np.uint8) for d in rows])
    bad_row = 9
    blobs[int(bo[bad_row]) + 7] ^= 0x10
    total = pos + 64
    want = np.full(total, 0xA5, np.uint8)
    for i, o in enumerate(out_off):
        want[o:o + sizes[i]] = blobs[int(bo[i]):int(bo[i]) + sizes[i]]
    return dict(blobs=blobs, bo=bo, bs=bs, oo=np.array(out_off, np.uint64), ck=ck, total=total, want=want, bad_row=bad_row,
                sizes=sizes)


def write_case(oracle):
    entries, skip = random_round_entries(seed=3, n_rounds=160)
    return entries, skip, [oracle.blake3(e) for e in entries]


def ragged_rounds():
    """(offsets, sizes, staging bytes): many rounds of ragged sizes at unaligned offsets in one staging buffer — several chunks
    per wave, big-unit slices, the merge kernel."""
    rng = np.random.default_rng(5)
    sizes = [0, 1, 5, 64, 1000, 1024, 1025, 4096, 10240, 10240, 10240, 33333, 65536, 65537, 70000, 300000,
             0, 2, 1 << 20, 3, 999, 5 << 20, 17, 64 * 1024 * 3 + 5] + [int(x) for x in rng.integers(0, 20000, 400)]
    offs, pos = [], 3
    for s in sizes:
        offs.append(pos)
        pos += s + int(rng.integers(0, 7))
    return offs, sizes, np.frombuffer(gen.incompressible(99, pos + 16), dtype=np.uint8)


def periodic(period, n, seed):
    rng = np.random.default_rng(seed)
    p = rng.integers(32, 127, size=period, dtype=np.uint8).tobytes()
    return (p * (n // period + 1))[:n]


BLK = 128 * 1024


def big_rows_entries():
    """Big rows for this library's own encoder: blocks that are 'literals + one periodic match' or raw (the fused block
    kernel), short last blocks, a mixed frame, entropy-coded blocks (block items), two small rows."""
    return [
        periodic(45, 8 * BLK, 1),                      # whole blocks, all recognised
        periodic(7, 3 * BLK + 12345, 2),               # short last block
        periodic(600, 2 * BLK + 1, 3),
        gen.incompressible(4, 4 * BLK),                # raw blocks
        gen.incompressible(5, 2 * BLK + 999),
        periodic(13, BLK, 6) + gen.incompressible(7, BLK) + gen.pseudo_text(BLK, seed=8) + periodic(200, BLK + 77, 9),  # mixed frame
        gen.pseudo_text(3 * BLK + 5, seed=10),         # entropy-coded blocks: not for the fused kernel
        periodic(1, 5 * BLK, 11),
        gen.text(10240), gen.text(70000),
    ]


def periodic_rows_entries():
    """A cut of test_periodic_rows_every_period_and_alignment's rows: every period class the recognised-row path of the
    fused kernel tells apart, whole-leaf and ragged sizes, back to back (so every output alignment), text rows behind."""
    rng = np.random.default_rng(5)
    entries = []
    for i, period in enumerate(list(range(1, 33)) + [45, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 400, 511, 600]):
        n = int(rng.integers(1, 40)) * 1024 if i % 3 else int(rng.integers(70, 40000))
        entries.append(periodic(period, n, i))
    return entries + [gen.text(10240)] * 16 + [gen.text(10239), gen.text(10241), gen.text(65536), gen.text(65), gen.text(64)]


# ---- far placement: the same rows with offsets beyond 4 GiB ------------------------------------------------------------

FAR_LINE = 1 << 32


def place(offsets, sizes, mode, k=None):
    """The shift to add to an offset column so that its rows lie around the 4 GiB line: "above" — every row above it
    (line + 64 KiB); "straddle" — the line falls inside row k, near its middle (rows in front of k below it, rows behind k
    above); "start_at_line" — row k begins at the line when its offset is a multiple of 128, else within 127 bytes
    behind it.  One shift for the whole column, a multiple of 128: rows keep their distances and their alignment class."""
    if mode == "above":
        return FAR_LINE + (64 << 10)
    off, n = int(offsets[k]), int(sizes[k])
    assert off + n < FAR_LINE
    if mode == "straddle":
        assert n >= 256, "the row is too short to hold the line after rounding"
        return (FAR_LINE - off - n // 2) // 128 * 128
    if mode == "start_at_line":
        return -((off - FAR_LINE) // 128) * 128
    raise ValueError(mode)
