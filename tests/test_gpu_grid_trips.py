"""Past one grid.  The batch decoders launch min(n, 65536) workgroups and loop with += gridDim.x, so with more than 65,536 jobs a
workgroup takes a second job on the LDS the first one left: probability or Huffman tables, the input window, CRC tables.  Every
test here runs 65,536 + 64 items in one call; items j and j + 65,536 (j < 64) share a workgroup and differ in every way that reuse
could leak — other properties, a failed job then a clean one, another check, a long job then a tiny one —, in both orders.  The
distinct files are built and put to their CPU arbiter once; every status and every byte of all items is compared, and the guards
with them."""
import zlib

import pytest

import gen
import gunzip_checks as GZ
import gz_model
import inflate_checks as IC
import lzma_build as L
import targz_checks as TC
import targz_model
import xz_build as X
import xz_cases as K
from deflate_build import classify, deflate
from test_tar_rules_cpu import make_tar
from unxz_checks import E_CORRUPT, OK, arbiter, run_batch

pytestmark = pytest.mark.gpu

GRID = 65536
PAIRS = 64


def lay_out(pairs, filler):
    """GRID + PAIRS items: item j is pairs[j % len][0] and item GRID + j its partner, both orders in turn; the filler between them"""
    both = pairs + [(b, a) for a, b in pairs]
    first = [both[j % len(both)][0] for j in range(PAIRS)]
    second = [both[j % len(both)][1] for j in range(PAIRS)]
    return first + [filler[j % len(filler)] for j in range(GRID - PAIRS)] + second


def test_unxz_second_trip(gpu_ctx):
    """more than 65,536 tail ranges, decode jobs and check jobs in one znippy_unxz_batch call"""
    t = gen.pseudo_text(24_000, seed=21)
    lits = lambda s: [("lit", c) for c in s]
    bad_ops = lits(t[:300]) + [("match", 200, 100), ("rep", 0, 50)] + lits(t[300:340]) + [("match", 492, 9), ("lit", 1)]   # (490 bytes are there)
    bad = K.scripted_file(L.Writer(lc=4, lp=0, pb=4).lzma(bad_ops))[0]
    pairs = [(X.xz([t[:3000]], lc=4, lp=0, pb=0, check=X.CHECK_CRC32), X.xz([t[3000:6000]], lc=0, lp=4, pb=4, check=X.CHECK_CRC32)),
             (bad, X.xz([t[6000:6400]], check=X.CHECK_CRC32)),
             (X.xz([t[7000:7700]], check=X.CHECK_CRC32), X.xz([t[7700:8400]], check=X.CHECK_CRC64)),
             (X.xz([t[4000:]], check=X.CHECK_CRC64), X.xz([b"z"], check=X.CHECK_CRC64)),
             (X.xz([t[:2000]], lc=0, lp=0, pb=0), X.xz([t[2000:4000]], lc=3, lp=1, pb=2))]
    filler = [X.xz([t[k:k + 1 + 5 * k]], check=(X.CHECK_CRC32, X.CHECK_CRC64)[k & 1]) for k in range(7)]
    want = {f: arbiter(f) for f in [f for p in pairs for f in p] + filler}
    assert [f for f, w in want.items() if w is None] == [bad]
    items = lay_out(pairs, filler)
    assert len(items) == GRID + PAIRS
    rooms = [len(want[f]) if want[f] is not None else 600 for f in items]
    status, got, streams, blocks, unverified, names = run_batch(gpu_ctx, items, rooms)
    assert names == ["unxz_tail", "unxz_decode", "unxz_check"], names
    wrong = [(i, st) for i, (f, st, g) in enumerate(zip(items, status, got)) if (st, g) != ((OK, want[f]) if f is not bad else (E_CORRUPT, b""))]
    assert not wrong, (len(wrong), wrong[:10])
    clean = [int(f is not bad) for f in items]       # (a failed item reports no streams and no blocks)
    assert streams == clean and blocks == clean and unverified == [0] * len(items)
    assert E_CORRUPT in status[:PAIRS] and E_CORRUPT in status[GRID:]       # a failed job in front of a clean one, and behind one


def corrupt_deflate(data, level=9):
    """`data` deflated and flushed, then a block of the reserved type 3: zlib hands out all of `data` and refuses the next byte, so no
    other verdict (a room too small, a sum that differs) can come first"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    bad = c.compress(data) + c.flush(zlib.Z_FULL_FLUSH) + b"\x07"
    d = zlib.decompressobj(-15)
    with pytest.raises(zlib.error):
        d.decompress(bad)
    return bad


def test_inflate_second_trip(gpu_ctx):
    """more than 65,536 items in one znippy_inflate_batch call: k_inflate and k_inflate_crc"""
    t = gen.pseudo_text(24_000, seed=22)
    dyn = deflate(t[:5000], 9)
    assert dyn[0] & 6 == 4                                  # a dynamic block
    pairs = [(("dynamic", dyn, 5000), ("stored", deflate(t[5000:5300], 0), 300)),
             (("corrupt", corrupt_deflate(t[:5000]), 5000), ("dynamic 2", deflate(t[6000:9000], 6), 3000)),
             (("long", deflate(t, 6), len(t)), ("one byte", deflate(b"q"), 1)),
             (("fixed", deflate(b"abcabcabc"), 9), ("empty", deflate(b""), 0))]
    filler = [(f"filler {k}", deflate(t[k:k + 1 + 9 * k], (0, 6)[k & 1]), 1 + 9 * k) for k in range(7)]
    status = IC.check(gpu_ctx, lay_out(pairs, filler))      # zlib's verdict, bytes and CRC for every item
    assert len(status) == GRID + PAIRS and IC.E_CORRUPT in list(status[:PAIRS]) and IC.E_CORRUPT in list(status[GRID:])


def test_gunzip_second_trip(gpu_ctx):
    """more than 65,536 tiny gzip files in one znippy_gunzip_batch call: the scan, the single-wave decoder and the CRC launch"""
    t = gen.pseudo_text(24_000, seed=23)
    good = GZ.gz(t[:5000], 9)
    bad = good[:10] + corrupt_deflate(t[:5000]) + good[-8:]
    sum_bad = good[:-8] + bytes([good[-8] ^ 1]) + good[-7:]
    pairs = [(good, GZ.gz(t[5000:5300], 0)), (bad, GZ.gz(t[6000:9000], 6)), (GZ.gz(t, 6), GZ.gz(b"q")), (sum_bad, GZ.gz(b"abcabcabc"))]
    filler = [GZ.gz(t[k:k + 1 + 9 * k], (0, 6)[k & 1]) for k in range(7)]
    want = {f: gz_model.expect(f) for f in [f for p in pairs for f in p] + filler if f not in (bad, sum_bad)}
    refused = {bad: GZ.E_CORRUPT, sum_bad: GZ.E_CHECKSUM}
    items = lay_out(pairs, filler)
    rooms = [len(want[f][0]) if f in want else 5000 for f in items]
    status, got, members, segments, names = GZ.run_batch(gpu_ctx, items, rooms)
    wrong = [(i, st) for i, (f, st, g, m, s) in enumerate(zip(items, status, got, members, segments))
             if (st, g, m, s) != ((OK, want[f][0], want[f][1], want[f][2]) if f in want else (refused[f], b"", 0, 0))]
    assert not wrong, (len(wrong), wrong[:10])
    assert "gunzip_scan" in names and len(items) == GRID + PAIRS


def test_targz_find_second_trip(gpu_ctx):
    """more than 65,536 tiny archives in one znippy_targz_find_batch call: k_targz_find and the gather"""
    scan_cap = 4096
    toml = b"[package]\nname = \"pkg\"\n"
    tar = lambda members: TC.gz(make_tar("ustar", members))
    first = tar([("p/Cargo.toml", toml * 3), ("p/a.rs", b"fn a() {}\n" * 40)])
    last = tar([("p/a.rs", gen.incompressible(7, 700)), ("p/Cargo.toml", toml)])
    absent = tar([("p/a.rs", b"fn a() {}\n")])
    bad = last[:10] + corrupt_deflate(make_tar("ustar", [("p/a.rs", gen.incompressible(7, 700)), ("p/Cargo.toml", toml)])[:1024]) + last[-8:]
    pairs = [(first, last), (absent, first), (bad, last)]
    filler = [tar([("p/Cargo.toml", toml[:1 + 3 * k])]) for k in range(7)]
    want = {f: targz_model.find(f, 1, b"", b"Cargo.toml", scan_cap) for f in [f for p in pairs for f in p] + filler}
    assert [want[f][0] for f in (first, last)] == [0, 0] and want[absent][0] != 0 and want[bad][0] == TC.M.E_CORRUPT
    items = lay_out(pairs, filler)
    status, got, scanned = TC.run_batch(gpu_ctx, items, b"Cargo.toml", scan_cap=scan_cap)
    wrong = [(i, st, want[f][0]) for i, (f, st, g) in enumerate(zip(items, status, got)) if (st, g) != (want[f][0], want[f][1])]
    assert not wrong, (len(wrong), wrong[:10])
    assert all(want[f][2] <= sc <= want[f][2] + 65535 + 258 for f, st, sc in zip(items, status, scanned) if st == 0)
    assert len(items) == GRID + PAIRS
