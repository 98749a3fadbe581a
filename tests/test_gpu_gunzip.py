"""znippy_gunzip_batch: whole gzip files inflated on the device, members and flush segments in parallel, against Python's
gzip.decompress and the piece model of tests/gz_model.py.  One batch per test; every source starts at an odd offset, every room has
guard bytes in front of and behind it, and the guards are compared after every batch."""
import ctypes as C
import gzip
import zlib

import numpy as np
import pytest

import gen
import gz_model as M
from gunzip_checks import (E_CHECKSUM, E_CORRUPT, E_DST_SMALL, E_INVAL, E_UNSUPPORTED, GUARD, OK, bgzf, check_valid, flushed, gz, run_batch,
                           single_members)

pytestmark = pytest.mark.gpu


# ---- 1. single members ---------------------------------------------------------------------------------------------------------

def test_single_members(gpu_ctx):
    items = single_members()
    for s in items:
        # (the empty file of level 0 is one final stored block, 01 00 00 FF FF: a flush candidate in front of its trailer that the default seg_min drops)
        assert M.candidates(s, M.SEG_MIN_DEFAULT) == ([], False), "the fixture is meant to have no kept candidate behind byte 0"
    want, segments, names = check_valid(gpu_ctx, items)
    assert segments == [1] * len(items)
    assert names == ["gunzip_scan", "gunzip_single", "gunzip_crc"], names   # one decode pass per item


# ---- 2. members ----------------------------------------------------------------------------------------------------------------

def test_members(gpu_ctx):
    three = gz(gen.text(5000)) + gz(b"") + gz(gen.pseudo_text(9000, seed=5), 9)
    five = bgzf(gen.pseudo_text(5 * 3000, seed=8), 3000)
    assert len(five) > 28 and gzip.decompress(five) == gen.pseudo_text(5 * 3000, seed=8)
    items = [three, five, three + bytes(7), gz(b"a") + bytes(7) + gz(b"b") + bytes(64) + gz(b"c") + bytes(129)]
    want, segments, names = check_valid(gpu_ctx, items, seg_min=1)
    assert [w[1:] for w in want] == [(3, 3), (6, 6), (3, 3), (3, 3)]
    assert "gunzip_probe" in names and "gunzip_inflate" in names and "gunzip_crc" in names, names


# ---- 3. flush points -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("make", [gen.text, lambda n: gen.pseudo_text(n, seed=21)], ids=["phrase", "words"])
def test_full_flush(gpu_ctx, make):
    t = make(200_000)
    f = flushed([t[i:i + 40_000] for i in range(0, 200_000, 40_000)], zlib.Z_FULL_FLUSH)
    want, segments, names = check_valid(gpu_ctx, [f], seg_min=1)
    assert segments == [5]
    assert "gunzip_probe" in names and "gunzip_inflate" in names, names
    _, fewer, _ = check_valid(gpu_ctx, [f])                      # the default seg_min: the same bytes from fewer or as many pieces
    assert 1 <= fewer[0] <= 5


def test_sync_flush_joins(gpu_ctx):
    half = gen.incompressible(3, 4096)
    twice = flushed([half, half], zlib.Z_SYNC_FLUSH)             # the second copy is matches into the first
    t = gen.pseudo_text(80_000, seed=4)
    mixed = flushed([t[:20_000], t[20_000:40_000], t[40_000:60_000], t[60_000:]], [zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH])
    phrase = gen.text(9000)
    # two sync flushes in a row: an empty piece that is independent, and behind it one that reaches through it
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    gap = c.compress(phrase[:4000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(phrase[4000:]) + c.flush()
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    gap2 = c.compress(phrase[:4000]) + c.flush(zlib.Z_SYNC_FLUSH) + b"\x00\x00\x00\xff\xff" + c.compress(phrase[4000:]) + c.flush()
    want, segments, names = check_valid(gpu_ctx, [twice, mixed, gap, gap2], seg_min=1)
    assert segments[0] == 1 and segments[1] == 3 and segments[3] == 1, segments


# ---- 4. false candidates -------------------------------------------------------------------------------------------------------

def test_false_candidates(gpu_ctx):
    # stored data that holds the flush pattern followed by bytes that parse as a block header (a final fixed block: 03 00), by a
    # stored block header, and member magic with a plausible header behind it
    inner = gz(b"not a member of the file")
    data = (gen.text(300) + b"\x00\x00\xff\xff\x03\x00" + gen.text(100) + b"\x00\x00\xff\xff\x00\x05\x00\xfa\xffhello" + b"\x1f\x8b\x08\x00" + bytes(6) +
            gen.text(50) + inner + b"\x00\x00\xff\xff" + gen.text(77))
    stored = gz(data, 0)
    assert stored.count(b"\x00\x00\xff\xff") >= 3 and stored.count(b"\x1f\x8b\x08") >= 3
    # ... and the same bytes as the first of two members, and inside a compressed member next to a true flush point
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    mixed = c.compress(gen.text(5000)) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(gen.incompressible(5, 600) + data) + c.flush()
    items = [stored, stored + gz(gen.text(100)), mixed]
    want, segments, names = check_valid(gpu_ctx, items, seg_min=1)
    assert [w[1] for w in want] == [1, 2, 1]
    assert "gunzip_probe" in names
    # candidates that outnumber the item's slice of the list (16 + len / 256): the item is decoded by one wave, member by member
    many = gz((b"\x00\x00\xff\xff" + b"\x1f\x8b\x08") * 400, 0) + gz(gen.text(300)) + gz(b"")
    assert M.candidates(many, 1)[1]
    want, segments, names = check_valid(gpu_ctx, [many], seg_min=1)
    assert want[0][1:] == (3, 1) and names == ["gunzip_scan", "gunzip_single", "gunzip_crc"], names


# ---- 5. statuses ---------------------------------------------------------------------------------------------------------------

def test_statuses(gpu_ctx):
    t = gen.pseudo_text(30_000, seed=2)
    good = flushed([t[:10_000], t[10_000:20_000], t[20_000:]], zlib.Z_FULL_FLUSH)
    small = gz(gen.text(500))
    flush_at = good.index(b"\x00\x00\xff\xff") + 4
    flip = lambda s, at: s[:at] + bytes([s[at] ^ 0x10]) + s[at + 1:]   # noqa: E731
    method9, reserved = bytearray(small), bytearray(small)
    method9[2] = 9
    reserved[3] |= 0x20
    G, S = 30_000, 500                                                                             # the contents' sizes
    cases = [
        (good, OK, G), (small, OK, S),
        (flip(good, len(good) - 8), E_CHECKSUM, G), (flip(small, len(small) - 6), E_CHECKSUM, S),        # CRC
        (flip(good, len(good) - 3), E_CHECKSUM, G), (flip(small, len(small) - 1), E_CHECKSUM, S),        # ISIZE
        (good[:7], E_CORRUPT, G), (small[:3], E_CORRUPT, S),                                             # inside the header
        (good[:len(good) // 2], E_CORRUPT, G), (small[:len(small) - 12], E_CORRUPT, S),                  # inside the stream
        (good[:flush_at], E_CORRUPT, G), (good[:flush_at + 1], E_CORRUPT, G),                            # at a flush point
        (good[:-3], E_CORRUPT, G), (small[:-8], E_CORRUPT, S), (small[:-1], E_CORRUPT, S),               # inside the trailer
        (good + b"x", E_CORRUPT, G), (small + b"x", E_CORRUPT, S), (small + bytes(5) + b"x", E_CORRUPT, S),
        (good + small[:9], E_CORRUPT, G + S), (small + b"\x1f\x8b\x09", E_UNSUPPORTED, S),
        (bytes(method9), E_UNSUPPORTED, S), (bytes(reserved), E_UNSUPPORTED, S),
        (good + bytes(method9), E_UNSUPPORTED, G + S), (good + flip(small, len(small) - 1), E_CHECKSUM, G + S),
        (good, OK, G), (small, OK, S),
    ]
    items, rooms = [c[0] for c in cases], [c[2] for c in cases]
    status, got, members, segments, names = run_batch(gpu_ctx, items, rooms, seg_min=1)
    assert status == [c[1] for c in cases], status
    for s, st, g in zip(items, status, got):
        assert g == (gzip.decompress(s) if st == OK else b"")
    for s, st in zip(items, status):                                       # the arbiter refuses what the device refuses,
        if st != OK and s != bytes(reserved):                              # but for the one deviation: reserved flag bits
            with pytest.raises((OSError, EOFError, zlib.error)):
                gzip.decompress(s)
    # rooms one byte short beside rooms that fit; a room with slack
    items = [good, small, good, small, good + small, small]
    rooms = [29_999, 499, 30_000, 500, 30_499, 777]
    status, got, members, segments, names = run_batch(gpu_ctx, items, rooms, seg_min=1)
    assert status == [E_DST_SMALL, E_DST_SMALL, OK, OK, E_DST_SMALL, OK], status
    assert got[2] == t and got[3] == gen.text(500) and got[5] == gen.text(500) and members[2:4] == [1, 1] and segments[2:4] == [3, 1]


def test_host_validation_and_call_rules(gpu_ctx):
    import torch
    from znippy_amd import _lib
    L = _lib.lib()
    s = gz(gen.text(1000))
    d_src = torch.from_numpy(np.frombuffer(bytes(7) + s, np.uint8).copy()).cuda()
    d_out = torch.full((4096,), GUARD, dtype=torch.uint8, device="cuda")
    big = (1 << 64) - 4
    src_off = [7, 7, big, 7, 7, 7, 7]
    src_len = [len(s), len(s) + 1, 8, len(s), len(s), 1 << 32, len(s)]
    out_off = [0, 1000, 1000, 4096 - 999, big, 1000, 2000]
    status, _, ln, _, _ = gpu_ctx.gunzip_batch(d_src, src_off, src_len, d_out, [1000] * 7, out_off=out_off)
    assert list(status) == [OK, E_INVAL, E_INVAL, E_DST_SMALL, E_DST_SMALL, E_INVAL, OK]    # past src_cap, overflowing, past out_cap
    assert list(ln) == [1000, 0, 0, 0, 0, 0, 1000]
    img = d_out.cpu().numpy()
    assert img[:1000].tobytes() == gen.text(1000) and img[2000:3000].tobytes() == gen.text(1000) and (img[1000:2000] == GUARD).all() and (img[3000:] == GUARD).all()
    # sizes of 4 GiB and more are refused before any kernel (the regions only have to be declared that big); an item of no bytes is
    # no member and no content, as for the arbiter
    status, _, ln, mem, _ = gpu_ctx.gunzip_batch(d_src, [0, 0, 7], [1 << 32, 8, 0], d_out, [8, 1 << 32, 5], out_off=[0, 0, 0], src_cap=1 << 33, out_cap=1 << 33)
    assert list(status) == [E_UNSUPPORTED, E_UNSUPPORTED, OK] and list(ln) == [0, 0, 0] and gzip.decompress(b"") == b""
    # rooms packed back to back when no offsets are given
    status, off, ln, _, _ = gpu_ctx.gunzip_batch(d_src, [7, 7], [len(s), len(s)], d_out, [1000, 1000])
    assert list(status) == [OK, OK] and list(off) == [0, 1000] and d_out[:2000].cpu().numpy().tobytes() == gen.text(1000) * 2
    # n == 0, NULL arguments, n too large
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)   # noqa: E731
    st = (C.c_int32 * 1)(99)
    ol = u64(99)
    sp, op = C.c_void_p(d_src.data_ptr()), C.c_void_p(d_out.data_ptr())

    def call(h, dsrc, so, sl, dout, room, out_len, n):
        return L.znippy_gunzip_batch(h, dsrc, d_src.numel(), so, sl, n, dout, d_out.numel(), None, room, 0, out_len, st, None, None)
    assert call(gpu_ctx.h, None, None, None, None, None, None, 0) == OK
    assert call(gpu_ctx.h, sp, u64(7), u64(len(s)), op, u64(1000), ol, 1) == OK and st[0] == OK and ol[0] == 1000
    for args in [(None, u64(7), u64(len(s)), op, u64(1000), ol), (sp, None, u64(len(s)), op, u64(1000), ol), (sp, u64(7), None, op, u64(1000), ol),
                 (sp, u64(7), u64(len(s)), None, u64(1000), ol), (sp, u64(7), u64(len(s)), op, None, ol), (sp, u64(7), u64(len(s)), op, u64(1000), None)]:
        assert call(gpu_ctx.h, *args, 1) == E_INVAL
    assert call(None, sp, u64(7), u64(len(s)), op, u64(1000), ol, 1) == E_INVAL
    assert call(gpu_ctx.h, sp, u64(7), u64(len(s)), op, u64(1000), ol, (1 << 32) - 16) == E_INVAL


# ---- 6. every single-bit mutant around the places that steer the chain ----------------------------------------------------------

def test_single_bit_mutants(gpu_ctx):
    t = gen.pseudo_text(21_000, seed=13)
    first = flushed([t[:5000], t[5000:10_000], t[10_000:15_000]], zlib.Z_FULL_FLUSH)
    f = first + gz(t[15_000:])
    assert 4000 <= len(f) <= 8000, len(f)
    flushes = [i + 4 for i in range(len(first)) if first[i:i + 4] == b"\x00\x00\xff\xff"]
    assert len(flushes) == 2
    where = set(range(48)) | set(range(len(f) - 16, len(f)))
    for p in flushes + [len(first)]:
        where |= set(range(p - 8, p + 8))
    items = []
    for at in sorted(where):
        for bit in range(8):
            items.append(f[:at] + bytes([f[at] ^ (1 << bit)]) + f[at + 1:])
    room = 4 * len(f)
    status, got, members, segments, names = run_batch(gpu_ctx, items + [f], [room] * (len(items) + 1), seg_min=1)
    assert status[-1] == OK and got[-1] == t and (members[-1], segments[-1]) == (2, 4)
    seen = set()
    for i, s in enumerate(items):
        want = M.outcome(s, room)
        seen.add(want[0])
        if want[0] == "ok":
            assert status[i] == OK and got[i] == want[1], (i, status[i])
        elif want[0] == "dst":
            assert status[i] == E_DST_SMALL, (i, status[i])
        elif want[0] == "unsup":
            assert status[i] == E_UNSUPPORTED, (i, status[i])
        else:
            assert status[i] != OK, i
    assert {"ok", "unsup", "bad"} <= seen, seen   # (flips of MTIME, XFL and OS change nothing; of FLG's reserved bits and the method: unsup)


# ---- 7. not a run --------------------------------------------------------------------------------------------------------------

def test_not_a_run(gpu_ctx, oracle):
    from test_gpu_ranges import own_frames, sentinel, table_of
    rows = [gen.pseudo_text(300_001, seed=51), gen.incompressible(9, 70_000), gen.text(10_240)]
    comp = [1, 0, 1]
    frames = [f if c else r for f, r, c in zip(own_frames(19, rows), rows, comp)]
    ck = np.stack([np.frombuffer(oracle.blake3(r), np.uint8) for r in rows])
    ck[2] ^= 1                                                  # one mismatch, so that the corrupt list has an entry
    total = sum(len(r) for r in rows)
    t = gen.text(50_000)
    items = [flushed([t[:25_000], t[25_000:]], zlib.Z_FULL_FLUSH), gz(gen.text(100))]

    def sequence(mixed_in):
        rt, d_blobs, _ = table_of(gpu_ctx, frames, rows, comp=comp, checksum=ck)
        out = sentinel(total + 64)
        rt.decode_verify_async(d_blobs, out)
        if mixed_in:
            status, got, members, segments, names = run_batch(gpu_ctx, items, [50_000, 100], seg_min=1)
            assert status == [OK, OK] and got == [t, gen.text(100)] and segments == [2, 1]
            assert names == ["gunzip_scan", "gunzip_probe", "gunzip_single", "gunzip_inflate", "gunzip_crc"], names
        counters, corrupt, status = rt.results()
        res = (counters, list(corrupt), status.copy(), rt.digests().copy(), out.cpu().numpy())
        rt.close()
        return res
    plain, mixed = sequence(False), sequence(True)
    assert plain[0]["corrupt_rows"] == 1 and plain[1] == [2]
    for k, (x, y) in enumerate(zip(plain, mixed)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, k
