"""Opt-in aligned blob offsets on the write side (znippy_rounds_set_blob_align): every payload starts at a multiple of a power
of two, the gaps are zero, nothing at or beyond blob_bytes is written and the payloads are those of the packed run.  The tables
are the smallest shapes that reach each code path of the pad pass, the scan and the two gathers: A lane-per-piece gather with the
hash inside the encoder and more than 256 pieces; B store-heavy (the hash kernel copies the stored rounds, the gather owns the
gaps) with stored rounds around the 16-byte, 4 KiB and 64 KiB piece borders, at an aligned and at an odd base; C wave-per-piece
gather, rounds of several blocks, without and with the cross-block window; D the device decides what is stored; E the hash on
the auxiliary stream beside the encoder; F encoded rounds of 4, 5 and 66 blocks: the pad pass sums a round of up to 4 pieces in
its own lane and a longer one with the whole wave, 64 pieces per step.  Expected values are the oracle's (BLAKE3, an independent zstd decoder) and the
recurrence of the header's contract."""
import ctypes as C

import numpy as np
import pytest

import gen
from gpu_cases import FAR_LINE as T

pytestmark = pytest.mark.gpu

ALIGNS = (1, 16, 128, 4096)
GUARD = 0xA5
TAIL = 8192  # guard bytes behind blob_bound
BLK = 128 * 1024  # one encoder block = one piece of an encoded round


class Table:
    def __init__(self, oracle, entries, skip=None, store_inc=False, window_log=0):
        self.entries = entries
        self.n = len(entries)
        self.skip = np.zeros(self.n, np.uint8) if skip is None else np.asarray(skip, np.uint8)
        self.store_inc, self.window_log = store_inc, window_log
        self.lens = np.array([len(e) for e in entries], np.uint64)
        self.offs = (np.cumsum(self.lens) - self.lens).astype(np.uint64)
        self.src = np.frombuffer(b"".join(entries) + bytes(64), np.uint8).copy()
        self.digests = np.stack([np.frombuffer(oracle.blake3(e), np.uint8) for e in entries])
        self._dev = None
        self.packed = None  # the run of a table on which the setter was never called: (offsets, sizes, compressed, region)

    def d_src(self):
        import torch
        if self._dev is None:
            self._dev = torch.from_numpy(self.src).cuda()
        return self._dev

    def rounds(self, ctx):
        from znippy_amd import hip
        rt = hip.RoundTable(ctx, self.offs, self.lens, self.skip if self.skip.any() else None)
        if self.store_inc:
            rt.set_store_incompressible(True)
        return rt


SMALL_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 100, 255, 256, 257, 511, 512, 513, 1000, 2047, 4095, 4096, 4097, 7000, 10240]
STORED_LENS = [0, 1, 15, 16, 17, 4095, 4096, 4097, 65535, 65536, 65537, 200003]


def _build(name, oracle):
    if name == "A":
        return Table(oracle, [gen.pseudo_text(SMALL_LENS[i % len(SMALL_LENS)], seed=i) if i % 3 else gen.text(SMALL_LENS[i % len(SMALL_LENS)])
                              for i in range(300)])
    if name == "B":
        entries, skip = [], []
        for i, n in enumerate(STORED_LENS):
            entries += [gen.incompressible(20 + i, n), gen.text(300 + 7 * i)]
            skip += [1, 0]
        return Table(oracle, entries, skip)
    if name in ("C", "Cw"):
        return Table(oracle, [gen.pseudo_text(131072, seed=1), gen.pseudo_text(131073, seed=2), gen.pseudo_text(300000, seed=3)],
                     window_log=17 if name == "Cw" else 0)
    if name == "D":
        return Table(oracle, [gen.incompressible(1, 1), gen.text(10240), gen.incompressible(2, 100), gen.pseudo_text(50000, seed=4),
                              gen.incompressible(3, 5000), gen.text(300), gen.incompressible(4, 70000), b"", gen.incompressible(5, 200003),
                              gen.incompressible(6, 140000), gen.text(17)], store_inc=True)
    if name == "F":
        return Table(oracle, [gen.text(4 * BLK), gen.text(4 * BLK + 1), gen.text(65 * BLK + 5), gen.pseudo_text(1000, seed=9)])
    if name == "E":
        entries = [gen.pseudo_text(20000 + 6001 * i, seed=30 + i) for i in range(20)]
        skip = [0] * 20
        for at, n in ((3, 1000), (9, 65537), (15, 17)):
            entries.insert(at, gen.incompressible(40 + at, n))
            skip.insert(at, 1)
        return Table(oracle, entries, skip)
    raise KeyError(name)


@pytest.fixture(scope="module")
def tables(oracle):
    built = {}

    def get(name):
        if name not in built:
            built[name] = _build(name, oracle)
        return built[name]
    return get


class Window:
    """The session's context at level 19 with the table's window, as it was afterwards."""

    def __init__(self, ctx, window_log):
        self.ctx, self.window_log = ctx, window_log

    def __enter__(self):
        self.old = (self.ctx.level, self.ctx.window_log)
        self.ctx.set_level(19)
        self.ctx.set_window_log(self.window_log)

    def __exit__(self, *exc):
        self.ctx.set_level(self.old[0])
        self.ctx.set_window_log(self.old[1])


def round_up(v, a):
    return (int(v) + a - 1) // a * a


def check_layout(oracle, t, a, bo, bs, comp, ck, nbytes, region, what, payloads=True):
    """region: host bytes from the base on, beyond blob_bytes; everything the contract says about one run."""
    bo, bs = [int(x) for x in bo], [int(x) for x in bs]
    assert bo[0] == 0, what
    for i in range(t.n - 1):
        assert bo[i + 1] == round_up(bo[i] + bs[i], a), (what, i, bo[i], bs[i], bo[i + 1])
    assert all(o % a == 0 for o in bo), what
    assert nbytes == bo[-1] + bs[-1], (what, nbytes)
    assert np.array_equal(ck, t.digests), what
    gap = np.ones(nbytes, bool)
    for i, e in enumerate(t.entries):
        gap[bo[i]:bo[i] + bs[i]] = False
        if not payloads:
            continue
        f = region[bo[i]:bo[i] + bs[i]].tobytes()
        if comp[i]:
            assert oracle.libzstd_decompress(f, max(len(e), 1)) == e, (what, i, len(e))
        else:
            assert f == e, (what, i, len(e))
    assert not region[:nbytes][gap].any(), (what, "a gap byte is not zero")
    tail = region[nbytes:]
    assert (tail == GUARD).all(), (what, "byte written at or beyond blob_bytes", nbytes + int((tail != GUARD).nonzero()[0][0]))


def run_aligned(ctx, t, a, shift=0, set_it=True, cap=None):
    """One run on a new table into a region prefilled with the guard value, blob_cap = blob_bound() unless given.
    Returns (offsets, sizes, compressed, digests, blob_bytes, region on the host, bound, kernel names)."""
    import torch
    rt = t.rounds(ctx)
    if set_it:
        rt.set_blob_align(a)
        assert rt.blob_align() == a
    bound = rt.blob_bound()
    buf = torch.full((shift + bound + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
    d_blob = buf[shift:]
    assert (d_blob.data_ptr() - shift) % 256 == 0
    try:
        enc = rt.encode_hash(t.d_src(), d_blob, blob_cap=bound if cap is None else cap)
        out = (enc["blob_offset"].copy(), enc["blob_size"].copy(), enc["compressed"].copy(), enc["checksum"].copy(),
               int(enc["blob_bytes"]), d_blob.cpu().numpy(), bound, set(dict(ctx.kernel_times())))
    finally:
        rt.close()
    return out


def packed_run(ctx, t):
    if t.packed is None:
        bo, bs, comp, ck, nbytes, region, bound, names = run_aligned(ctx, t, 1, set_it=False)
        assert "round_pad" not in names
        assert np.array_equal(bo, np.cumsum(bs) - bs) and nbytes == int(bs.sum())
        t.packed = (bo, bs, comp, region[:nbytes].copy(), bound)
    return t.packed


CASES = [("A", 0), ("B", 0), ("B", 1), ("C", 0), ("Cw", 0), ("D", 0), ("E", 0), ("F", 0)]


@pytest.mark.parametrize("a", ALIGNS)
@pytest.mark.parametrize("name,shift", CASES, ids=[f"{n}+{s}" if s else n for n, s in CASES])
def test_aligned_layout(gpu_ctx, oracle, tables, name, shift, a):
    t = tables(name)
    with Window(gpu_ctx, t.window_log):
        pbo, pbs, pcomp, pregion, pbound = packed_run(gpu_ctx, t)
        bo, bs, comp, ck, nbytes, region, bound, names = run_aligned(gpu_ctx, t, a, shift)
    what = f"table {name} align {a} shift {shift}"
    print(f"ALIGN {what}: blob_bytes {nbytes} (packed {len(pregion)}), bound {bound}; kernels {sorted(names)}")
    assert bound == pbound + (t.n - 1) * (a - 1), what
    assert nbytes <= bound, what
    assert ("round_pad" in names) == (a > 1), (what, sorted(names))
    check_layout(oracle, t, a, bo, bs, comp, ck, nbytes, region, what)
    # frames do not depend on the alignment: every payload is the packed run's
    assert np.array_equal(bs, pbs) and np.array_equal(comp, pcomp), what
    for i in range(t.n):
        assert np.array_equal(region[int(bo[i]):int(bo[i] + bs[i])], pregion[int(pbo[i]):int(pbo[i] + pbs[i])]), (what, i)
    if a == 1:  # the setter with 1 is the table on which it was never called
        assert np.array_equal(bo, pbo) and nbytes == len(pregion) and np.array_equal(region[:nbytes], pregion), what
    if name == "D":
        assert not comp[[4, 6, 8, 9]].any() and comp[[1, 3]].all(), (what, comp.tolist())  # the device stored the incompressible rounds


def test_two_runs_in_flight_keep_their_own_alignment(gpu_ctx, oracle, tables):
    import torch
    for name in ("A", "B"):
        t = tables(name)
        with Window(gpu_ctx, 0):
            rt = t.rounds(gpu_ctx)
            rt.set_blob_align(4096)
            cap = rt.blob_bound()
            bufs = [torch.full((cap + TAIL,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(2)]
            rt.set_blob_align(16)
            rt.encode_hash_async(t.d_src(), bufs[0], blob_cap=cap)
            rt.set_blob_align(4096)  # the queued run keeps 16
            rt.encode_hash_async(t.d_src(), bufs[1], blob_cap=cap)
            rt.set_blob_align(1)     # neither run sees this
            older = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in rt.results_lagged(1).items()}
            newer = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in rt.results_lagged(0).items()}
            rt.close()
        for a, r, buf in ((16, older, bufs[0]), (4096, newer, bufs[1])):
            check_layout(oracle, t, a, r["blob_offset"], r["blob_size"], r["compressed"], r["checksum"], int(r["blob_bytes"]),
                         buf.cpu().numpy(), f"table {name} in flight align {a}")


@pytest.mark.parametrize("name", ["A", "B", "C", "E"])
def test_region_one_byte_short(gpu_ctx, oracle, tables, name):
    """blob_cap one below what a good run reports: the packed path's error, nothing written at or behind blob_cap."""
    from znippy_amd._lib import E_DST_SMALL, ZnippyError
    t = tables(name)
    for a in (1, 128, 4096):
        with Window(gpu_ctx, 0):
            nbytes = run_aligned(gpu_ctx, t, a)[4]
            import torch
            rt = t.rounds(gpu_ctx)
            rt.set_blob_align(a)
            buf = torch.full((nbytes - 1 + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
            with pytest.raises(ZnippyError) as ei:
                rt.encode_hash(t.d_src(), buf, blob_cap=nbytes - 1)
            rt.close()
        assert ei.value.code == E_DST_SMALL, (name, a)
        assert bool((buf[nbytes - 1:] == GUARD).all()), (name, a, "byte written behind blob_cap")


@pytest.mark.parametrize("a", [16, 4096])
def test_round_trip_through_the_read_side(gpu_ctx, oracle, tables, a):
    """A row table built from the aligned results, with the region's size declared: decode + verify, verify-only and decode-only."""
    import torch
    from znippy_amd import hip
    for name in ("B", "E"):
        t = tables(name)
        with Window(gpu_ctx, 0):
            bo, bs, comp, ck, nbytes, region, _, _ = run_aligned(gpu_ctx, t, a)
        total = int(t.lens.sum())
        d_blobs = torch.from_numpy(np.concatenate([region[:nbytes], np.zeros(64, np.uint8)])).cuda()
        rows = hip.RowTable(gpu_ctx, bo, bs, t.lens, t.offs, np.packbits(comp.astype(bool), bitorder="little"), ck)
        want = dict(total_chunks=t.n, total_written_bytes=total, verified_bytes=total, corrupt_bytes=0, corrupt_rows=0, decode_errors=0)
        d_out = torch.full((total + 64,), GUARD, dtype=torch.uint8, device="cuda")
        c, corrupt, status = rows.decode_verify(d_blobs, d_out, out_cap=total, blob_cap=nbytes)
        assert c == want and len(corrupt) == 0 and (status == 0).all(), (name, a, c)
        assert d_out[:total].cpu().numpy().tobytes() == b"".join(t.entries) and bool((d_out[total:] == GUARD).all())
        assert np.array_equal(rows.digests(), t.digests)
        c, corrupt, status = rows.verify(d_blobs, blob_cap=nbytes)
        assert c == want and len(corrupt) == 0 and (status == 0).all(), (name, a, c)
        d_out.fill_(GUARD)
        c, status = rows.decode(d_blobs, d_out, out_cap=total, blob_cap=nbytes)
        assert c == want and (status == 0).all(), (name, a, c)
        assert d_out[:total].cpu().numpy().tobytes() == b"".join(t.entries)
        rows.close()


def test_invalid_arguments(gpu_ctx, tables):
    from znippy_amd import _lib, hip
    from znippy_amd._lib import E_INVAL, ZnippyError
    t = tables("E")
    rt = t.rounds(gpu_ctx)
    assert rt.blob_align() == 1
    packed = rt.blob_bound()
    rt.set_blob_align(128)
    for bad in (0, 3, 8192, 4097, 1 << 31):
        with pytest.raises(ZnippyError) as ei:
            rt.set_blob_align(bad)
        assert ei.value.code == E_INVAL, bad
        assert rt.blob_align() == 128 and rt.blob_bound() == packed + (t.n - 1) * 127, bad
    for a in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        rt.set_blob_align(a)
        assert rt.blob_align() == a and rt.blob_bound() == packed + (t.n - 1) * (a - 1)
    rt.close()
    L = _lib.lib()
    assert L.znippy_rounds_set_blob_align(None, 16) == E_INVAL and L.znippy_rounds_blob_align(None) == 1
    # a closed context (destroyed while a table keeps it alive): the setter is refused and changes nothing
    h = C.c_void_p()
    assert L.znippy_ctx_create(0, None, C.byref(h)) == 0
    one = np.array([0], np.uint64), np.array([100], np.uint64)
    r = C.c_void_p()
    assert L.znippy_rounds_create(h, _lib.np_ptr(one[0]), _lib.np_ptr(one[1]), None, 1, C.byref(r)) == 0
    assert L.znippy_rounds_set_blob_align(r, 64) == 0
    L.znippy_ctx_destroy(h)
    assert L.znippy_rounds_set_blob_align(r, 16) == E_INVAL and L.znippy_rounds_blob_align(r) == 64
    L.znippy_rounds_destroy(r)


FILL = 64 << 20


def test_aligned_offsets_cross_the_4_gib_line(gpu_ctx, oracle, tables):
    """By the method of test_gpu_far.py: 64 store-path rounds over one 64 MiB slice push table E's aligned payloads across the
    4 GiB line of a big region.  An offset cut to 32 bits would land in the first filler's copy, which is compared whole."""
    import torch
    from znippy_amd import hip
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip(f"the far region needs 6 GiB of free device memory, {free >> 20} MiB are free")
    t, a = tables("E"), 4096
    X = 200003  # the fillers end this far below the line, at an odd address
    filler = np.random.default_rng(78).integers(0, 256, FILL, dtype=np.uint8)
    d_src = torch.from_numpy(np.concatenate([filler, t.src])).cuda()
    ln = np.concatenate([np.full(63, FILL, np.uint64), [np.uint64(FILL - X)], t.lens]).astype(np.uint64)
    so = np.concatenate([np.zeros(64, np.uint64), t.offs + np.uint64(FILL)]).astype(np.uint64)
    sk = np.concatenate([np.ones(64, np.uint8), t.skip])
    far = torch.empty(T + (96 << 20), dtype=torch.uint8, device="cuda")
    far[T - FILL:].fill_(GUARD)
    with Window(gpu_ctx, 0):
        pbo, pbs, pcomp, pregion, _ = packed_run(gpu_ctx, t)
        rt = hip.RoundTable(gpu_ctx, so, ln, sk)
        rt.set_blob_align(a)
        assert rt.blob_bound() <= far.numel()
        enc = rt.encode_hash(d_src, far)
        bo, bs, ck, nbytes = enc["blob_offset"].copy(), enc["blob_size"].copy(), enc["checksum"].copy(), int(enc["blob_bytes"])
        rt.close()
    bo, bs = [int(x) for x in bo], [int(x) for x in bs]
    assert bs == [int(x) for x in ln[:64]] + [int(x) for x in pbs]
    assert bo[0] == 0 and all(bo[i + 1] == round_up(bo[i] + bs[i], a) for i in range(len(bo) - 1))
    assert nbytes == bo[-1] + bs[-1] and bo[64] == round_up(T - X, a) < T < bo[-1]
    whole, cut = oracle.blake3(filler.tobytes()), oracle.blake3(filler[:FILL - X].tobytes())
    assert all(ck[i].tobytes() == whole for i in range(63)) and ck[63].tobytes() == cut
    assert np.array_equal(ck[64:], t.digests)
    for i in range(63):
        assert torch.equal(far[i * FILL:(i + 1) * FILL], d_src[:FILL]), i   # (i = 0: where an offset cut to 32 bits lands)
    assert torch.equal(far[63 * FILL:T - X], d_src[:FILL - X])
    assert not far[T - X:bo[64]].any(), "gap behind the fillers"
    d_packed = torch.from_numpy(pregion).cuda()
    for i in range(t.n):
        k = 64 + i
        assert torch.equal(far[bo[k]:bo[k] + bs[k]], d_packed[int(pbo[i]):int(pbo[i] + pbs[i])]), i
        if i + 1 < t.n:
            assert not far[bo[k] + bs[k]:bo[k + 1]].any(), ("gap", i)
    assert bool((far[nbytes:] == GUARD).all()), "bytes behind blob_bytes were written"
    print(f"ALIGN far: table E from {bo[64]} to {nbytes}, line at {T}")
    del far
    torch.cuda.empty_cache()


def test_python_pipelines_on_the_gpu_backend(gpu_ctx, tmp_path):
    """compress_stream / compress_dir with blob_align on the product backend: aligned offsets in the index, zero gaps, and the
    archive reads back; the backend is left packing as before."""
    from znippy_amd import index as ix
    from znippy_amd.backend import default_backend
    from znippy_amd.decompress import decompress_archive
    from znippy_amd.slot_packer import compress_dir
    from znippy_amd.stream_packer import ArchiveEntry, compress_stream
    files = {f"t/{i}.txt": gen.pseudo_text(500 + 977 * i, seed=i) for i in range(10)}
    files.update({"s.jar": gen.incompressible(1, 70001), "empty": b"", "z.txt": gen.text(100)})
    b = default_backend()
    try:
        c = compress_stream(tmp_path / "a", False, backend=b, blob_align=4096)
        for k, v in files.items():
            c.sender().send(ArchiveEntry(k, v))
        c.finish()
        assert b.blob_align == 4096
        (tmp_path / "in" / "t").mkdir(parents=True)
        for k, v in files.items():
            (tmp_path / "in" / k).write_bytes(v)
        compress_dir(tmp_path / "in", tmp_path / "d", backend=b, blob_align=128)
        for name, a in (("a", 4096), ("d", 128)):
            p = tmp_path / f"{name}.znippy"
            _, batches = ix.read_znippy_index(str(p))
            rows = sorted((o, s) for bt in batches for o, s in zip(bt.column(5).to_pylist(), bt.column(6).to_pylist()))
            assert len(rows) == len(files) and all(o % a == 0 for o, _ in rows)
            raw = np.frombuffer(p.read_bytes(), np.uint8)
            gap = np.ones(rows[-1][0] + rows[-1][1], bool)
            for o, s in rows:
                gap[o:o + s] = False
            assert gap.any() and not raw[:len(gap)][gap].any(), name
            rep = decompress_archive(p, True, tmp_path / f"out_{name}", backend=b)
            assert (rep.total_files, rep.corrupt_files) == (len(files), 0)
            for k, v in files.items():
                assert (tmp_path / f"out_{name}" / k).read_bytes() == v, (name, k)
        compress_stream(tmp_path / "p", False, backend=b).finish()   # the default resets the backend
        assert b.blob_align == 1
    finally:
        b.set_blob_align(1)
