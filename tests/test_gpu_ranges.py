"""Byte ranges of rows (znippy_rows_read_ranges): a read that decodes only the 128 KiB blocks a range overlaps.

The bytes of every case are compared with the source slices; what the call decoded is compared with a figure worked out
from the geometry alone (decoded_bytes: the content size of every block decoded on its own, uncompressed_size of every row
decoded whole, nothing for stored rows) — that figure, not a timing, shows which route a row took.  Output regions carry a
sentinel around and between the destinations, so a byte written outside a destination shows."""
import ctypes as C

import numpy as np
import pytest

import gen
import zstd_synth as zs
from gpu_cases import foreign_archive, mixed
from range_checks import (BLK, HIGH_BASE, ROW_SIZES, SENTINEL, boundary_ranges, expected_decoded, own_frames, read_and_check, sentinel,
                          table_of, to_dev)

pytestmark = pytest.mark.gpu

# ---- 1. block boundaries on own frames (and 8: the same with a far base) ----------------------------------------------------

@pytest.fixture(scope="module")
def own_rows():
    rows = [gen.pseudo_text(n, seed=40 + i) for i, n in enumerate(ROW_SIZES[:-1])] + [mixed(ROW_SIZES[-1], seed=9)]
    return rows, {level: own_frames(level, rows) for level in (3, 19)}


@pytest.mark.parametrize("level", [3, 19])
@pytest.mark.parametrize("base", [0, HIGH_BASE], ids=["base0", "far_base"])
def test_block_boundaries_on_own_frames(gpu_ctx, own_rows, level, base):
    rows, frames = own_rows
    rt, d_blobs, _ = table_of(gpu_ctx, frames[level], rows, base=base)
    ranges = boundary_ranges(ROW_SIZES)
    want = expected_decoded(ranges, ROW_SIZES)
    assert want == 5_000 + 131_072 + 131_073 + 262_145 + 300_001   # every block of every row is touched, each counted once
    kw = dict(blob_base=base)
    read_and_check(rt, d_blobs, rows, ranges, ("in order", level), want_decoded=want, **kw)
    shuffled = [ranges[i] for i in np.random.default_rng(level).permutation(len(ranges))]
    read_and_check(rt, d_blobs, rows, shuffled, ("shuffled", level), guard=1, want_decoded=want, **kw)
    read_and_check(rt, d_blobs, rows, shuffled, ("shuffled, packed", level), guard=64, packed=True, want_decoded=want, **kw)
    names = dict(gpu_ctx.kernel_times())
    assert {"range_scan", "range_decode_blocks", "range_decode_rows", "range_copy"} <= set(names), sorted(names)
    # only what a range overlaps: one block of the 300,001-byte row, the ragged last one
    few = [(4, 300_000, 1), (4, 262_144, 5), (2, 131_072, 1), (0, 17, 3)]
    read_and_check(rt, d_blobs, rows, few, ("few", level), want_decoded=(300_001 - 2 * BLK) + 1 + 5_000, **kw)
    rt.close()


# ---- 2. work saved -------------------------------------------------------------------------------------------------------------

def test_one_range_decodes_one_or_two_blocks(gpu_ctx):
    row = gen.pseudo_text(1 << 20, seed=77)
    rt, d_blobs, _ = table_of(gpu_ctx, own_frames(19, [row]), [row])
    read_and_check(rt, d_blobs, [row], [(0, 3 * BLK + 1000, 4096)], "inside block 3", want_decoded=131_072)
    read_and_check(rt, d_blobs, [row], [(0, 4 * BLK - 2048, 4096)], "blocks 3 and 4", want_decoded=262_144)
    names = set(dict(gpu_ctx.kernel_times()))
    assert "range_decode_rows" not in names and "range_decode_blocks" in names, sorted(names)
    rt.close()


# ---- 3. the gather at every alignment --------------------------------------------------------------------------------------

def test_gather_alignment_on_stored_rows(gpu_ctx):
    from znippy_amd import hip
    LENS = [1, 15, 16, 17, 63, 129, 4097]
    blob = np.frombuffer(gen.incompressible(5, 80_003), np.uint8)
    bo, bs = np.array([0, 40_003], np.uint64), np.array([40_000, 40_000], np.uint64)
    rt = hip.RowTable(gpu_ctx, bo, bs, bs, None, np.zeros(1, np.uint8), None)
    d_blobs = to_dev(blob)
    assert d_blobs.data_ptr() % 16 == 0
    rr, rb, rl, ro, cur, used = [], [], [], [], 5, set()
    for s in range(16):
        for d in range(16):
            row = (s + d) & 1
            begin = 16 * (7 + d) + (s - int(bo[row])) % 16
            n = LENS[(s * 16 + d) % 7]
            cur += (d - cur) % 16 or 16                    # a gap of 1..16 sentinel bytes in front of every destination
            rr.append(row); rb.append(begin); rl.append(n); ro.append(cur)
            assert (int(bo[row]) + begin) % 16 == s and cur % 16 == d
            used.add(n)
            cur += n
    assert used == set(LENS)
    region = sentinel(cur + 64)
    assert region.data_ptr() % 16 == 0
    status, decoded = rt.read_ranges(d_blobs, rr, rb, rl, region, out_offsets=ro)
    assert (status == 0).all() and decoded == 0
    want = np.full(cur + 64, SENTINEL, np.uint8)
    for row, begin, n, at in zip(rr, rb, rl, ro):
        a = int(bo[row]) + begin
        want[at:at + n] = blob[a:a + n]
    got = region.cpu().numpy()
    assert np.array_equal(got, want), int(np.nonzero(got != want)[0][0])
    assert set(dict(gpu_ctx.kernel_times())) == {"range_copy"}
    rt.close()


# ---- 4. fallbacks return the same bytes -----------------------------------------------------------------------------------

def fallback_ranges(sizes):
    out = []
    for row, L in enumerate(sizes):
        out += [(row, 0, 1), (row, L - 1, 1), (row, 131_071, 2), (row, 140_000, 4097), (row, L, 0)]
    return out


def test_fallback_foreign_frames(gpu_ctx, oracle):
    rows = [gen.pseudo_text(300_001, seed=3), gen.pseudo_text(200_000, seed=4), gen.pseudo_text(150_000, seed=5)]
    A = foreign_archive(oracle, rows, 19)
    from znippy_amd import hip
    rt = hip.RowTable(gpu_ctx, A["bo"], A["bs"], A["us"], A["oo"], None, A["ck"])
    d_blobs = to_dev(A["blobs"])
    ranges = fallback_ranges([300_001, 200_000])           # row 2 is not touched
    read_and_check(rt, d_blobs, rows, ranges, "libzstd -19", want_decoded=500_001)
    rt.close()


def test_fallback_window_frames(gpu_ctx):
    part = gen.incompressible(8, 100_000)
    rows = [part * 3, gen.pseudo_text(50_000, seed=6) * 6]
    frames = own_frames(19, rows, window_log=17)
    plain = own_frames(19, rows)
    assert all(len(f) < len(p) for f, p in zip(frames, plain))   # smaller than with the window off: blocks reach into the ones before
    rt, d_blobs, _ = table_of(gpu_ctx, frames, rows)
    read_and_check(rt, d_blobs, rows, fallback_ranges([300_000, 300_000]), "window 17", want_decoded=600_000)
    rt.close()


def synth_frames():
    """Two frames in this encoder's plain style — raw literals, predefined tables, 128 KiB of content per block, a closing empty raw
    block — whose second block needs the first: a match reaching into it / a repeat code as its first sequence."""
    lits0 = gen.pseudo_text(70_000, seed=11)
    b0 = zs.Comp(lits0, [(70_000, BLK - 70_000, 3 + 4_321)], lit=dict(type="raw"))
    lits1 = gen.pseudo_text(BLK - 50_000, seed=12)
    reach = zs.Comp(lits1, [(100, 50_000, 3 + 5_100)], lit=dict(type="raw"))      # 5,000 bytes into block 0
    repeat = zs.Comp(lits1, [(100, 50_000, 1)], lit=dict(type="raw"))             # the distance block 0's last sequence used
    out = []
    for b1 in (reach, repeat):
        content = zs.execute([b0, b1])
        assert len(content) == 2 * BLK
        out.append((content, zs.write_frame([b0, b1], content=content, empty_last=True)))
    return out


def test_fallback_block_that_needs_history(gpu_ctx, oracle):
    cases = synth_frames()
    for content, frame in cases:
        assert oracle.zstd_decompress(frame, cap=len(content)) == content       # a valid frame, by the oracle's decoder
    rows, frames = [c for c, _ in cases], [f for _, f in cases]
    rt, d_blobs, _ = table_of(gpu_ctx, frames, rows)
    # block 0 alone decodes from a clean state: 128 KiB, nothing whole
    read_and_check(rt, d_blobs, rows, [(0, 1_000, 4096), (1, 70_500, 100)], "block 0", want_decoded=2 * BLK)
    assert "range_decode_rows" not in dict(gpu_ctx.kernel_times())
    # block 1 does not.  decoded_bytes is the evidence for both halves: 2 x 128 KiB above with no whole-row pass means the scan accepted the
    # frames and block 0 decoded on its own; two whole rows here means the block decoder flagged block 1 and the rows went to the late pass
    read_and_check(rt, d_blobs, rows, [(0, BLK + 50, 4096), (0, 5, 9), (1, BLK + 50, 4096), (1, 2 * BLK - 1, 1)], "block 1", want_decoded=4 * BLK)
    assert "range_decode_rows_late" in dict(gpu_ctx.kernel_times())
    rt.close()


# ---- 5. damage ---------------------------------------------------------------------------------------------------------------

def block_payloads(frame):
    """[(offset of the payload, bytes)] of the blocks of a single-segment frame."""
    fhd = frame[4]
    single, fcs_flag = (fhd >> 5) & 1, fhd >> 6
    pos = 5 + (0 if single else 1) + (single if fcs_flag == 0 else 1 << fcs_flag)
    out = []
    while True:
        bh = int.from_bytes(frame[pos:pos + 3], "little")
        size = 1 if (bh >> 1) & 3 == 1 else bh >> 3
        out.append((pos + 3, size))
        pos += 3 + size
        if bh & 1:
            return out


def test_damage_outside_the_needed_blocks(gpu_ctx):
    from znippy_amd import hip
    row = gen.pseudo_text(4 * BLK, seed=21)
    (frame,) = own_frames(19, [row])
    blocks = block_payloads(frame)
    assert len(blocks) == 5 and blocks[4][1] == 0           # four blocks and the closing empty one
    bad = bytearray(frame)
    bad[blocks[3][0] + blocks[3][1] // 2] ^= 0x5A
    blobs = bytes(bad) + frame
    bo = np.array([0, len(frame)], np.uint64)
    bs = np.array([len(frame), len(frame) - 1], np.uint64)  # row 1: the clean frame, cut by one byte
    us = np.array([4 * BLK, 4 * BLK], np.uint64)
    oo = np.array([0, 4 * BLK], np.uint64)
    d_blobs = to_dev(blobs)
    fresh = hip.RowTable(gpu_ctx, bo, bs, us, oo, None, None)
    d_full = sentinel(8 * BLK + 64)
    _, st_whole = fresh.decode(d_blobs, d_full)
    st_whole = st_whole.copy()
    whole = d_full.cpu().numpy()
    fresh.close()
    assert st_whole[1] < 0
    rt = hip.RowTable(gpu_ctx, bo, bs, us, None, None, None)
    region = sentinel(9000)
    status, decoded = rt.read_ranges(d_blobs, [0, 1], [BLK - 5000, 100], [4097, 300], region, out_offsets=[3, 4500])
    assert list(status) == [0, st_whole[1]], (status, st_whole)
    got = region.cpu().numpy()
    want = np.full(9000, SENTINEL, np.uint8)
    want[3:3 + 4097] = np.frombuffer(row[BLK - 5000:BLK - 5000 + 4097], np.uint8)
    assert np.array_equal(got, want) and decoded == BLK
    # a range inside the damaged block: the whole-row decode's verdict, and its bytes where it has one
    region = sentinel(5000)
    status, _ = rt.read_ranges(d_blobs, [0], [3 * BLK + 10], [4097], region, out_offsets=[1])
    assert status[0] == st_whole[0], (status, st_whole)
    got = region.cpu().numpy()
    assert got[0] == SENTINEL and bool((got[4098:] == SENTINEL).all())
    if st_whole[0] == 0:
        assert np.array_equal(got[1:4098], whole[3 * BLK + 10:3 * BLK + 10 + 4097])
    else:
        assert bool((got == SENTINEL).all())
    rt.close()


# ---- 6. validation -------------------------------------------------------------------------------------------------------------

def test_validation_on_the_host(gpu_ctx):
    from znippy_amd import _lib, hip
    rows = [gen.pseudo_text(300_001, seed=31), gen.incompressible(2, 1000), gen.pseudo_text(9_000, seed=32)]
    frames = own_frames(3, [rows[0]]) + [rows[1]] + own_frames(3, [rows[2]])
    bs = np.array([len(f) for f in frames], np.uint64)
    bo = (np.cumsum(bs) - bs).astype(np.uint64)
    us = np.array([len(r) for r in rows], np.uint64)
    rt = hip.RowTable(gpu_ctx, bo, bs, us, None, np.packbits(np.array([1, 0, 1], bool), bitorder="little"), None, row_begin=0)
    d_blobs = to_dev(b"".join(frames))
    blob_cap = int(bo[2]) + int(bs[2]) - 1                  # the last row's blob ends one byte outside
    good = [(0, 200_000, 777), (1, 10, 99)]
    cases = [((3, 0, 1), _lib.E_INVAL), ((0, 300_000, 2), _lib.E_INVAL), ((0, 5, (1 << 64) - 3), _lib.E_INVAL),
             ((0, 300_002, 0), _lib.E_INVAL), ((1, 0, 50), _lib.E_DST_SMALL), ((2, 0, 10), _lib.E_CORRUPT)]
    cap = 4000
    for (row, begin, n), code in cases:
        region = sentinel(cap + 64)
        at = cap - 20 if code == _lib.E_DST_SMALL else 2000
        status, decoded = rt.read_ranges(d_blobs, [good[0][0], row, good[1][0]], [good[0][1], begin, good[1][1]], [good[0][2], n, good[1][2]], region,
                                         out_offsets=[1, at, 1000], out_cap=cap, blob_cap=blob_cap)
        assert list(status) == [0, code, 0], ((row, begin, n), status)
        want = np.full(cap + 64, SENTINEL, np.uint8)
        want[1:778] = np.frombuffer(rows[0][200_000:200_777], np.uint8)
        want[1000:1099] = np.frombuffer(rows[1][10:109], np.uint8)
        assert np.array_equal(region.cpu().numpy(), want), (row, begin, n)
        assert decoded == BLK
    # an offset past out_cap with no bytes is still outside; begin == length with no bytes is fine
    region = sentinel(cap)
    status, _ = rt.read_ranges(d_blobs, [1, 1], [1000, 0], [0, 0], region, out_offsets=[cap, cap + 1], out_cap=cap, blob_cap=blob_cap)
    assert list(status) == [0, _lib.E_DST_SMALL] and bool((region == SENTINEL).all().item())
    rt.close()


def test_abi_arguments(gpu_ctx):
    import torch
    from znippy_amd import _lib
    L = _lib.lib()
    E = _lib.E_INVAL
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    raw = gen.incompressible(3, 500)
    d = to_dev(raw)
    out = sentinel(256)
    dp, op = C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr())
    rows = C.c_void_p()
    bitmap = (C.c_uint8 * 1)(0)
    assert L.znippy_rows_create(gpu_ctx.h, u64(0), u64(500), bitmap, u64(500), None, None, 0, 1, C.byref(rows)) == 0
    st = (C.c_int32 * 2)(7, 7)
    dec = C.c_uint64(99)
    call = lambda ctx, t, blobs, rr, rb, rl, n, o: L.znippy_rows_read_ranges(ctx, t, blobs, 0, rr, rb, rl, None, n, o, 256, st, C.byref(dec))
    assert call(None, rows, dp, u64(0), u64(0), u64(4), 1, op) == E
    assert call(gpu_ctx.h, None, dp, u64(0), u64(0), u64(4), 1, op) == E
    assert call(gpu_ctx.h, rows, None, u64(0), u64(0), u64(4), 1, op) == E
    assert call(gpu_ctx.h, rows, dp, None, u64(0), u64(4), 1, op) == E
    assert call(gpu_ctx.h, rows, dp, u64(0), None, u64(4), 1, op) == E
    assert call(gpu_ctx.h, rows, dp, u64(0), u64(0), None, 1, op) == E
    assert call(gpu_ctx.h, rows, dp, u64(0), u64(0), u64(4), 1, None) == E
    assert call(gpu_ctx.h, rows, None, None, None, None, 0, None) == 0 and dec.value == 0       # no ranges
    assert bool((out == SENTINEL).all().item())
    assert call(gpu_ctx.h, rows, dp, u64(0, 0), u64(7, 100), u64(5, 3), 2, op) == 0             # packed, status and decoded_bytes filled
    assert [st[0], st[1]] == [0, 0] and dec.value == 0
    assert out[:8].cpu().numpy().tobytes() == raw[7:12] + raw[100:103] and bool((out[8:] == SENTINEL).all().item())
    assert L.znippy_rows_read_ranges(gpu_ctx.h, rows, dp, 0, u64(0), u64(1), u64(2), u64(40), 1, op, 256, None, None) == 0   # both optional
    assert out[40:42].cpu().numpy().tobytes() == raw[1:3]
    other = C.c_void_p()
    assert L.znippy_ctx_create(0, None, C.byref(other)) == 0
    assert call(other, rows, dp, u64(0), u64(0), u64(4), 1, op) == E                            # a table of another context
    t2 = C.c_void_p()
    assert L.znippy_rows_create(other, u64(0), u64(500), bitmap, u64(500), None, None, 0, 1, C.byref(t2)) == 0
    L.znippy_ctx_destroy(other)                                                                  # closed, kept alive by its table
    assert call(other, t2, dp, u64(0), u64(0), u64(4), 1, op) == E
    L.znippy_rows_destroy(t2)
    L.znippy_rows_destroy(rows)
    torch.cuda.synchronize()


# ---- 7. not a run --------------------------------------------------------------------------------------------------------------

def test_not_a_run(gpu_ctx, oracle):
    import torch
    rows = [gen.pseudo_text(300_001, seed=51), gen.incompressible(9, 70_000), gen.text(10_240), gen.pseudo_text(2 * BLK, seed=52)]
    comp = [1, 0, 1, 1]
    frames = [f if c else r for f, r, c in zip(own_frames(19, rows), rows, comp)]
    ck = np.stack([np.frombuffer(oracle.blake3(r), np.uint8) for r in rows])
    ck[2] ^= 1                                              # one checksum mismatch, so that the corrupt list has an entry
    total = sum(len(r) for r in rows)
    ranges = [(0, 250_000, 4097), (3, 131_000, 200), (1, 5, 777), (2, 100, 100)]

    def sequence(with_ranges):
        rt, d_blobs, _ = table_of(gpu_ctx, frames, rows, comp=comp, checksum=ck)
        outs = [sentinel(total + 64) for _ in range(2)]
        rt.decode_verify_async(d_blobs, outs[0])
        if with_ranges:
            read_and_check(rt, d_blobs, rows, ranges, "between two runs")
        rt.decode_verify_async(d_blobs, outs[1])
        a = rt.results_lagged(1)
        if with_ranges:
            read_and_check(rt, d_blobs, rows, ranges, "between a run and its results")
        b, corrupt, status = rt.results()
        res = (a, b, list(corrupt), status.copy(), rt.digests().copy(), outs[0].cpu().numpy(), outs[1].cpu().numpy())
        if with_ranges:
            read_and_check(rt, d_blobs, rows, ranges, "behind the runs")
        v = rt.verify(d_blobs)
        res += (v[0], list(v[1]), v[2].copy(), rt.digests().copy())
        rt.close()
        return res

    plain, mixed_in = sequence(False), sequence(True)
    assert plain[0]["corrupt_rows"] == 1 and plain[2] == [2]
    for k, (x, y) in enumerate(zip(plain, mixed_in)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, k
    # tables without out_offset / without checksum
    for kw in (dict(out_offset=False, checksum=ck), dict(out_offset=True, checksum=None), dict(out_offset=False, checksum=None)):
        rt, d_blobs, _ = table_of(gpu_ctx, frames, rows, comp=comp, **kw)
        read_and_check(rt, d_blobs, rows, ranges, kw, want_decoded=expected_decoded(ranges, [len(r) for r in rows], comp))
        rt.close()
    torch.cuda.synchronize()
