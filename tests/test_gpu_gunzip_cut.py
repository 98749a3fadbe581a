"""znippy_gunzip_batch with the cut at block starts (znippy_ctx_set_gunzip_cut): the contract is equivalence — status, out_len,
members and, for status 0, the bytes must be those of the switch off, on valid, damaged and adversarial files, with gzip.decompress
as the arbiter —, and the model of tests/gz_cut_model.py says what the search counts and how many pieces a cut file has.  A context
of its own carries the switch, so the session's shared context is never touched."""
import ctypes as C
import gzip
import os
import zlib

import numpy as np
import pytest

import deflate_build as D
import gen
import gz_cut_model as CM
import gz_model as M
from gpu_cases import make_ctx
from gunzip_checks import E_CORRUPT, E_DST_SMALL, E_INVAL, E_UNSUPPORTED, OK, flushed, gz, run_batch, with_header

pytestmark = pytest.mark.gpu

LL = D.huffman_lengths([1] * 286)      # complete codes over every symbol: any literal, length and distance can be written
DD = D.huffman_lengths([1] * 30)


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = make_ctx({"ZNIPPY_GZ_CUT": "0"})
    yield c
    c.close()


def both(ctx, cut, items, rooms, seg_min=0):
    """one batch with the switch off and on: status, content and members must be the same.  Returns (the results with it on, the
    segments with it off, stats, kernel names with it on)"""
    ctx.set_gunzip_cut(0)
    off = run_batch(ctx, items, rooms, seg_min)
    assert ctx.gunzip_cut_stats() == [0] * 8 and "gunzip_find" not in off[4]
    ctx.set_gunzip_cut(cut)
    try:
        on = run_batch(ctx, items, rooms, seg_min)
        stats = ctx.gunzip_cut_stats()
    finally:
        ctx.set_gunzip_cut(0)
    assert on[:3] == off[:3]
    return on, off[3], stats, on[4]


def check_stats(stats, items, cut):
    want = CM.expect_stats(items, cut)
    assert tuple(stats[:3]) == want, (stats, want, cut)
    return want


def check_segments(items, cut, segments, off_segments, stats, seg_min=0):
    """every item is a valid file: its segments are the model's, and the counters add up.  Returns the positions landed on"""
    landed, pieces = [], 0
    for i, s in enumerate(items):
        e = CM.expect_cut(s, cut, seg_min)
        if e is None:
            assert segments[i] == off_segments[i], i
        else:
            assert segments[i] == e[1], (i, segments[i], e[1])
            landed += e[2]
            pieces += e[1]
    assert stats[3] == len(landed) and stats[4] + stats[5] == pieces, (stats, len(landed), pieces)
    return landed


def member(blocks):
    """blocks: (kind, ops or data, final) -> a gzip member and its content"""
    bw = D.Bits()
    for kind, ops, final in blocks:
        if kind == "dyn":
            D.dynamic_block(bw, LL, DD, ops, final=final)
        elif kind == "fixed":
            D.fixed_block(bw, ops, final=final)
        else:
            D.stored_block(bw, ops, final=final)
    s = bw.bytes()
    try:
        content = zlib.decompress(s, -15)
    except zlib.error:
        return D.gz_member(s, b""), None
    return D.gz_member(s, content), content


def lits(n, seed):
    return list(gen.incompressible(seed, n))


# ---- 1. the corpus: every block kind, every bit offset ---------------------------------------------------------------------------

def test_corpus(ctx):
    import random
    items, contents = [], []
    for _, s, content, _ in D.corpus():
        items.append(D.gz_member(s, content))
        contents.append(content)
    rng = random.Random(7)
    for k in range(12):                                           # seeded encodings of every block kind, longer than the corpus's
        content = D.TEXT[1000 * k:1000 * k + 20_000 + 777 * k]
        s, _ = D.encode(content, rng, flush_p=0.1)
        items.append(D.gz_member(s, content))
        contents.append(content)
    (status, got, members, segments, _), off_seg, stats, names = both(ctx, 64, items, [len(c) for c in contents])
    assert status == [OK] * len(items) and got == contents and got == [gzip.decompress(s) for s in items]
    assert names[:2] == ["gunzip_scan", "gunzip_find"] and "gunzip_decode" in names, names
    check_stats(stats, items, 64)
    landed = check_segments(items, 64, segments, off_seg, stats)
    assert len(landed) > 100 and {p & 7 for p in landed} == set(range(8)), "the cuts taken cover every bit offset"
    assert stats[4] > 0 and stats[5] > 0 and stats[6] > 0 and stats[7] == 1


# ---- 2. the window's edge ------------------------------------------------------------------------------------------------------------

def test_window_edge(ctx):
    good, content = member([("dyn", lits(32768, 1), 0), ("dyn", [("m", 258, 32768)], 0), ("fixed", [65], 1)])
    assert content is not None and len(content) == 32768 + 259 and content[32768:32768 + 258] == content[:258]
    bad, none = member([("dyn", lits(32767, 1), 0), ("dyn", [("m", 258, 32768)], 0), ("fixed", [65], 1)])   # one byte too far back
    assert none is None
    (status, got, _, segments, _), _, stats, _ = both(ctx, 64, [good, bad, good], [len(content)] * 3)
    assert status == [OK, E_CORRUPT, OK] and got[0] == content and got[2] == content
    assert segments[0] == 2 and stats[4] == 2, (segments, stats)   # the match's block starts a marker piece, in both good files


# ---- 3. chain depth --------------------------------------------------------------------------------------------------------------

def test_chain_depth(ctx):
    blocks = [("dyn", lits(100, 2), 0)] + [("dyn", [("m", 100, 100)], 0)] * 40 + [("fixed", [], 1)]
    f, content = member(blocks)
    assert content == bytes(lits(100, 2)) * 41
    (status, got, _, segments, _), off_seg, stats, _ = both(ctx, 64, [f], [len(content)])
    assert status == [OK] and got == [content]
    landed = check_segments([f], 64, segments, off_seg, stats)
    assert len(landed) >= 40 and stats[4] >= 40 and stats[6] >= 4000   # every block a piece of 100 markers, 32 KiB windows spanning them all


# ---- 4. markers copied inside a piece ------------------------------------------------------------------------------------------------

def test_markers_copied_inside_a_piece(ctx):
    ops = [("m", 200, 900), ("m", 258, 50)] + lits(32_400, 4) + [("m", 258, 32768), ("m", 30, 7)] + lits(500, 5) + [("m", 258, 33_000 - 400)]
    f, content = member([("dyn", lits(1000, 3), 0), ("dyn", ops, 0), ("fixed", [66, 67], 1)])
    assert content is not None and len(content) > 1000 + 32768 + 500
    (status, got, _, segments, _), off_seg, stats, _ = both(ctx, 64, [f], [len(content)])
    assert status == [OK] and got == [content]
    check_segments([f], 64, segments, off_seg, stats)
    assert segments[0] == 2 and stats[6] >= 200 + 258 + 258           # markers in the head (apply) and in the last 32 KiB (tails)


# ---- 5. false candidates -------------------------------------------------------------------------------------------------------

def test_false_candidates(ctx):
    # a valid non-final dynamic block, copied byte for byte into a stored block's data, into FEXTRA and into FNAME: the copies pass
    # the header test (byte-aligned: the original's bit offset inside its first byte is kept) and are no block starts
    t = gen.pseudo_text(400_000, seed=31)
    raw = zlib.compressobj(6, zlib.DEFLATED, -15)
    stream = raw.compress(t) + raw.flush()
    first = next(p for p in CM.true_starts(stream) if p > 0)
    b = CM.Bits(stream)
    end = CM.dynamic_header(b, first + 3)[2]
    piece = stream[first >> 3:(end >> 3) + 64]
    name = piece.replace(b"\0", b"\x01")                          # (FNAME ends at the first zero byte; what is left may or may not pass)
    stored = gz(gen.text(200) + piece + gen.text(300) + piece, 0)
    items = [stored,
             with_header(t, 4, extra=piece[:60000]),
             with_header(t, 8, name=name),
             stored + gz(t)]
    rooms = [len(gzip.decompress(s)) for s in items]
    (status, got, members, segments, _), off_seg, stats, names = both(ctx, 64, items, rooms, seg_min=1)
    assert status == [OK] * 4 and got == [gzip.decompress(s) for s in items] and members == [1, 1, 1, 2]
    tested, passed, kept = check_stats(stats, items, 64)
    true = 3 * len(CM.true_starts(stream))                        # items 1, 2 and 3 hold the real stream once each
    assert passed >= true + 2 + 1 + 2, (passed, true)             # ... and the copies pass as well: 2 + 1 + 2 at the least
    assert stats[1] > stats[3] and stats[3] >= 2, stats           # candidates nobody lands on; items 1 and 2 are cut at the true ones
    assert segments[1] == CM.expect_cut(items[1], 64, 1)[1] >= 2
    assert segments[3] == CM.expect_cut(items[3], 64, 1)[1] > off_seg[3]   # two members, the second cut at its block starts


# ---- 6. mixtures ---------------------------------------------------------------------------------------------------------------

def test_mixtures_and_unsearched_items(ctx):
    text = gen.pseudo_text(400_000, seed=31)
    big = gz(text)                                                 # about 80 KB, a block every 30 KB or so
    small = [gz(gen.text(n)) for n in (0, 1, 500, 3000)]
    t2 = gen.pseudo_text(300_000, seed=32)
    sync = D.gz_member(D.flushed_stream(t2, 40_000, [zlib.Z_SYNC_FLUSH]), t2)     # pigz-like
    full = flushed([t2[i:i + 75_000] for i in range(0, 300_000, 75_000)], zlib.Z_FULL_FLUSH)
    items = [big] + small + [sync, full, big + small[2] + big]
    rooms = [len(gzip.decompress(s)) for s in items]
    assert len(CM.true_starts(big[10:-8])) >= 2
    seen = []
    for cut in (64, 1000, 4096, 16384, 65536):
        (status, got, _, segments, _), off_seg, stats, names = both(ctx, cut, items, rooms, seg_min=1)
        assert status == [OK] * len(items) and got[0] == text
        seen.append(check_stats(stats, items, cut))
        assert stats[0] == 8 * sum(len(s) for s in items if len(s) >= 2 * cut)
        check_segments(items, cut, segments, off_seg, stats, seg_min=1)
        assert all(a >= b for a, b in zip(segments, off_seg)), (cut, segments, off_seg)   # no file loses a cut point it has with the switch off
        if cut <= 16384:
            assert segments[0] >= 2 and off_seg[0] == 1 and segments[5] > off_seg[5], (cut, segments, off_seg)   # the pigz-like file: pieces that reach back no longer join
            assert segments[7] > off_seg[7] == 3                   # several members: each cut at its own block starts
    # the same positions pass whatever the grid; a coarser grid keeps fewer of them
    assert seen[0][1] == seen[1][1] and seen[0][2] >= seen[1][2] >= seen[2][2] >= seen[3][2] >= 1
    # items below 2 * cut are not searched: no launch, no count
    (status, _, _, segments, _), off_seg, stats, names = both(ctx, 1 << 20, small + [sync], rooms[1:6], seg_min=1)
    assert status == [OK] * 5 and stats == [0] * 8 and "gunzip_find" not in names and segments == off_seg


# ---- 7. damage -----------------------------------------------------------------------------------------------------------------

def test_damage(ctx):
    t = gen.pseudo_text(400_000, seed=13)
    f = gz(t)                                                      # one member, three blocks: cut at the second with the switch on
    starts = [80 + p for p in CM.true_starts(f[10:-8])]
    where = list(range(10, 30)) + list(range(len(f) - 10, len(f)))
    for p in starts[1:]:
        where += list(range((p >> 3) - 2, (p >> 3) + 12))          # around a block header the chain lands on
    items = [f[:at] + bytes([f[at] ^ (1 << bit)]) + f[at + 1:] for at in where for bit in (0, 3, 7)]
    items += [f[:n] for n in (130, 200, len(f) // 2, (starts[1] >> 3) + 5, len(f) - 9, len(f) - 1)]     # truncations
    room = len(t) + 100
    (status, got, _, segments, _), _, stats, _ = both(ctx, 64, items + [f], [room] * (len(items) + 1))
    assert status[-1] == OK and got[-1] == t and segments[-1] >= 2 and stats[0] == 8 * sum(len(s) for s in items + [f])
    seen = set()
    for i, s in enumerate(items):
        want = M.outcome(s, room)
        seen.add(want[0])
        if want[0] == "ok":
            assert status[i] == OK and got[i] == want[1], i
        elif want[0] == "dst":
            assert status[i] == E_DST_SMALL, i
        elif want[0] == "unsup":
            assert status[i] == E_UNSUPPORTED, i
        else:
            assert status[i] != OK, i
    assert {"ok", "bad"} <= seen
    # rooms one byte short, a room that ends inside a later piece, a room that fits
    (status, got, _, _, _), _, _, _ = both(ctx, 64, [f, f, f], [len(t) - 1, 250_000, len(t)])
    assert status == [E_DST_SMALL, E_DST_SMALL, OK] and got[2] == t


# ---- 8. the scratch budget -------------------------------------------------------------------------------------------------------

def test_budget(ctx):
    t = gen.pseudo_text(3 << 20, seed=81)
    f = gz(t)
    old = os.environ.get("ZNIPPY_GZ_CUT_SCRATCH_MB")
    os.environ["ZNIPPY_GZ_CUT_SCRATCH_MB"] = "1"                   # (read per call)
    try:
        (status, got, _, segments, _), _, stats, names = both(ctx, 16384, [f], [len(t)])
    finally:
        if old is None:
            del os.environ["ZNIPPY_GZ_CUT_SCRATCH_MB"]
        else:
            os.environ["ZNIPPY_GZ_CUT_SCRATCH_MB"] = old
    assert status == [OK] and got == [t] and segments[0] > 10
    assert stats[7] > 1 and stats[4] == segments[0] - 1 and stats[5] == 1, stats
    assert names.count("gunzip_decode") == names.count("gunzip_tails") == names.count("gunzip_apply") == stats[7]   # one of each per pass
    # a piece whose symbols alone exceed the budget joins the run in front of it: 2,100 matches of 258 bytes are 541,800 symbols
    f, content = member([("dyn", lits(1000, 6), 0), ("dyn", [("m", 258, 1000)] * 2100, 0), ("fixed", [65], 1)])
    assert content is not None and len(content) - 1001 > (1 << 20) // 2 and CM.expect_cut(f, 64)[1] == 2
    (status, got, _, segments, _), _, stats, _ = both(ctx, 64, [f], [len(content)])
    assert status == [OK] and got == [content] and segments == [2] and stats[3:6] == [1, 1, 1]
    os.environ["ZNIPPY_GZ_CUT_SCRATCH_MB"] = "1"
    try:
        (status, got, _, segments, _), _, stats, _ = both(ctx, 64, [f], [len(content)])
    finally:
        if old is None:
            del os.environ["ZNIPPY_GZ_CUT_SCRATCH_MB"]
        else:
            os.environ["ZNIPPY_GZ_CUT_SCRATCH_MB"] = old
    assert status == [OK] and got == [content] and segments == [1] and stats[3:7] == [0, 0, 1, 0], (segments, stats)


# ---- 9. the setter -------------------------------------------------------------------------------------------------------------

def test_setter_rules(ctx):
    from znippy_amd import _lib
    from znippy_amd._lib import ZnippyError
    L = _lib.lib()
    assert ctx.gunzip_cut == 0
    for v in (64, 65, 16384, 1 << 30, 0):
        ctx.set_gunzip_cut(v)
        assert ctx.gunzip_cut == v
    ctx.set_gunzip_cut(4096)
    for bad in (1, 63, (1 << 30) + 1, 1 << 40, (1 << 64) - 1):
        with pytest.raises(ZnippyError) as e:
            ctx.set_gunzip_cut(bad)
        assert e.value.code == E_INVAL and ctx.gunzip_cut == 4096
    ctx.set_gunzip_cut(0)
    assert L.znippy_ctx_set_gunzip_cut(None, 64) == E_INVAL and L.znippy_ctx_gunzip_cut(None) == 0
    assert L.znippy_ctx_gunzip_cut_stats(None, (C.c_uint64 * 8)()) == E_INVAL and L.znippy_ctx_gunzip_cut_stats(ctx.h, None) == E_INVAL
    # the environment sets the initial value of a new context; what is no valid value there is ignored
    for env, want in (("4096", 4096), ("64", 64), (str(1 << 30), 1 << 30), ("0", 0), ("63", 0), ("abc", 0), ("-64", 0), ("64k", 0), ("", 0),
                      (str((1 << 30) + 1), 0)):
        c = make_ctx({"ZNIPPY_GZ_CUT": env})
        try:
            assert c.gunzip_cut == want, env
        finally:
            c.close()
    # a context the environment switched on searches without being told to, and says so
    c = make_ctx({"ZNIPPY_GZ_CUT": "64"})
    try:
        s = gz(gen.pseudo_text(5000, seed=3))
        status, got, _, _, names = run_batch(c, [s], [5000])
        assert len(s) >= 128 and status == [OK] and got == [gen.pseudo_text(5000, seed=3)] and "gunzip_find" in names and c.gunzip_cut_stats()[0] == 8 * len(s)
        # the backend hands the setting through
        from znippy_amd.backend import HipBackend
        be = HipBackend(ctx=c)
        be.set_gunzip_cut(128)
        assert be.gunzip_cut == 128 and c.gunzip_cut == 128 and len(be.gunzip_cut_stats()) == 8
    finally:
        c.close()


def test_not_a_run(ctx, oracle):
    from test_gpu_ranges import own_frames, sentinel, table_of
    rows = [gen.pseudo_text(300_001, seed=51), gen.incompressible(9, 70_000), gen.text(10_240)]
    comp = [1, 0, 1]
    frames = [f if c else r for f, r, c in zip(own_frames(19, rows), rows, comp)]
    ck = np.stack([np.frombuffer(oracle.blake3(r), np.uint8) for r in rows])
    ck[2] ^= 1
    total = sum(len(r) for r in rows)
    t = gen.pseudo_text(400_000, seed=31)
    items = [gz(t), gz(gen.text(100))]

    def sequence(mixed_in):
        rt, d_blobs, _ = table_of(ctx, frames, rows, comp=comp, checksum=ck)
        out = sentinel(total + 64)
        rt.decode_verify_async(d_blobs, out)
        if mixed_in:
            ctx.set_gunzip_cut(64)
            try:
                status, got, members, segments, names = run_batch(ctx, items, [400_000, 100], seg_min=1)
            finally:
                ctx.set_gunzip_cut(0)
            assert status == [OK, OK] and got == [t, gen.text(100)]
            assert names[:2] == ["gunzip_scan", "gunzip_find"] and "gunzip_crc" in names, names
        counters, corrupt, status = rt.results()
        res = (counters, list(corrupt), status.copy(), rt.digests().copy(), out.cpu().numpy())
        rt.close()
        return res
    plain, mixed = sequence(False), sequence(True)
    assert plain[0]["corrupt_rows"] == 1 and plain[1] == [2]
    for k, (x, y) in enumerate(zip(plain, mixed)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, k
