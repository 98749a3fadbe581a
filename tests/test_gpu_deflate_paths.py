"""The streams of tests/deflate_build.py through every place the DEFLATE decoder of csrc/inflate_dev.h is instantiated: k_inflate,
k_gunzip_single (the first member and the members behind it), k_gunzip_probe (a member, and a piece behind a flush point),
k_gunzip_inflate (a run seated at any byte of the file) and k_targz_find.  The batches, the guard bytes and the comparisons are
those of test_gpu_inflate.py, test_gpu_gunzip.py and test_gpu_targz.py; the arbiters are zlib, gzip.decompress, gz_model and
targz_model, never the code under test.  tests/test_deflate_build_cpu.py shows without a GPU that the corpus holds the shapes it is
run for.  Every test is one or a few batches of small items."""
import random
import zlib

import pytest

import deflate_build as B
import gen
import gz_model as M
import targz_model as TM
import test_gpu_gunzip as TG
import test_gpu_inflate as TI
import test_gpu_targz as TT
from test_tar_rules_cpu import make_tar

pytestmark = pytest.mark.gpu

OK, E_UNSUPPORTED, E_CHECKSUM = 0, -6, -7
SINGLE_PASS = ["gunzip_scan", "gunzip_single", "gunzip_crc"]
# a first member of stored pattern soup: more candidates than any item's slice of the list holds (16 + len / 256)
SOUP = TG.gz((b"\x00\x00\xff\xff" + b"\x1f\x8b\x08") * 400, 0)


def inflated(stream):
    d = zlib.decompressobj(-15)
    out = d.decompress(stream)
    assert d.eof and d.unused_data == b""
    return out


def members():
    return [B.gz_member(s, content) for _, s, content, _ in B.corpus()]


# ---- a. k_inflate --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["packed", "reversed"])
def test_inflate_the_corpus(gpu_ctx, layout):
    cases = [(what, s, len(content)) for what, s, content, _ in B.corpus()]
    TI.check(gpu_ctx, cases, layout, accept_only=True)


# ---- b. gunzip, the single pass ------------------------------------------------------------------------------------------------

def test_gunzip_single_pass_first_member(gpu_ctx):
    items = [B.gz_member(s, content) for _, s, content, rec in B.corpus() if 0 not in rec.stored]
    assert len(items) >= 60
    for f in items:
        assert M.candidates(f, 1) == ([], False), "a stream without an empty stored block is meant to have no candidate"
    want, segments, names = TG.check_valid(gpu_ctx, items, seg_min=1)
    assert segments == [1] * len(items) and names == SINGLE_PASS, names


def test_gunzip_single_pass_members_behind_the_first(gpu_ctx):
    items = [SOUP + m for m in members()]
    for f in items:
        assert M.candidates(f, 1)[1], "the soup is meant to overflow the candidate list"
    want, segments, names = TG.check_valid(gpu_ctx, items, seg_min=1)
    assert all(w[1:] == (2, 1) for w in want) and names == SINGLE_PASS, names


# ---- c. gunzip, the probe and the piece decode ---------------------------------------------------------------------------------

def test_gunzip_probed_corpus(gpu_ctx):
    items = members()
    want, segments, names = TG.check_valid(gpu_ctx, items, seg_min=1)
    assert "gunzip_probe" in names and "gunzip_inflate" in names, names
    assert segments.count(1) >= 1 and max(segments) >= 3
    # files of 5 - 10 members, some with zero padding behind a member
    rng = random.Random(5)
    files, at = [], 0
    while at < len(items):
        k = rng.randint(5, 10)
        files.append(b"".join(m + bytes(rng.choice((0, 0, 1, 63, 64, 65))) for m in items[at:at + k]))
        at += k
    want, segments, names = TG.check_valid(gpu_ctx, files, seg_min=1)
    assert all(5 <= w[1] <= 10 for w in want[:-1]) and sum(w[1] for w in want) == len(items)
    assert "gunzip_probe" in names and "gunzip_inflate" in names, names


def test_hand_built_cases_as_pieces_behind_a_flush_point(gpu_ctx):
    """table_corner_cases and the small block_kind_cases behind a non-final fixed block of literals and an empty stored block: the
    case is a piece that the probe reads with REACH and the decoder with the StopAt hook.  Their matches stay inside them; the
    258-byte matches at distances 1 - 259 are then built once more with their source bytes in front of the flush point, so that the
    piece reaches back and joins."""
    prefix = b"a piece in front of the flush point. " * 3
    pre = B.Bits()
    B.fixed_block(pre, list(prefix), final=0)
    B.stored_block(pre, b"", final=0)
    items, alone = [], []
    for what, s, n in B.table_corner_cases() + [c for c in B.block_kind_cases() if c[2] <= 40_000]:
        st, body = B.classify(s, n)
        assert st == OK, what
        items.append(B.gz_member(pre.bytes() + s, prefix + body))
        alone.append(True)
    rnd = gen.incompressible(11, 300)
    for dist in (1, 2, 3, 63, 64, 65, 257, 258, 259):
        bw = B.Bits()
        B.fixed_block(bw, list(rnd[:dist]), final=0)
        B.stored_block(bw, b"", final=0)
        B.fixed_block(bw, [("m", 258, dist)])
        items.append(B.gz_member(bw.bytes(), inflated(bw.bytes())))
        alone.append(False)
    want, segments, names = TG.check_valid(gpu_ctx, items, seg_min=1)
    for sg, a in zip(segments, alone):
        assert sg >= 2 if a else sg == 1, (segments, alone)
    assert "gunzip_probe" in names and "gunzip_inflate" in names, names


# ---- d. window reloads from a run's first byte ---------------------------------------------------------------------------------

RELOADS = ((2035, 2076), (4090, 4136))    # literals in front of the stored block: it moves over the first two reloads of the window


def literal_text():
    text = bytes(b & 0x7F for b in B.TEXT[:4200])           # literals below 144: 8-bit codes
    pre = B.Bits()
    B.fixed_block(pre, list(text), final=0, eob=False)
    return text, pre


def test_stored_blocks_around_the_window_reloads_of_a_member(gpu_ctx):
    """test_short_stored_blocks_at_every_byte_around_the_window_reloads of test_gpu_inflate.py as gzip members: the window of
    k_gunzip_single and of the probe starts at the member's first DEFLATE byte, ten bytes into the source, not at byte 0."""
    text, pre = literal_text()
    tail = list(b"behind the stored block " * 3)
    single, probed = [], []
    for lo, hi in RELOADS:
        for p in range(lo, hi):
            for short in (b"", b"x", b"short"):
                bw = B.Bits()
                bw.b = pre.b[:3 + 8 * p] + [0] * 7        # P literals and the end-of-block code
                B.stored_block(bw, short, final=0)
                B.fixed_block(bw, tail)
                (single if short else probed).append(B.gz_member(bw.bytes(), text[:p] + short + bytes(tail)))
    for f in single:
        assert M.candidates(f, 1) == ([], False)
    want, segments, names = TG.check_valid(gpu_ctx, single, seg_min=1)
    assert names == SINGLE_PASS, names
    want, segments, names = TG.check_valid(gpu_ctx, probed, seg_min=1)
    assert segments == [2] * len(probed) and "gunzip_probe" in names and "gunzip_inflate" in names, names


@pytest.mark.parametrize("p0", [5, 1000])
def test_stored_blocks_around_the_window_reloads_of_a_piece(gpu_ctx, p0):
    """P0 literals, an empty stored block, Q literals, a stored block of 0, 1 or 5 bytes, a fixed tail: the second piece's window
    starts at the flush point, and Q moves the stored block byte by byte over the places it is loaded anew at."""
    text, pre = literal_text()
    tail = list(b"behind the stored block " * 3)
    items = []
    for lo, hi in ((2030, 2081), (4085, 4141)):
        for q in range(lo, hi):
            for short in (b"", b"x", b"short"):
                bw = B.Bits()
                bw.b = pre.b[:3 + 8 * p0] + [0] * 7
                B.stored_block(bw, b"", final=0)
                bw.b += pre.b[:3 + 8 * q] + [0] * 7
                B.stored_block(bw, short, final=0)
                B.fixed_block(bw, tail)
                items.append(B.gz_member(bw.bytes(), text[:p0] + text[:q] + short + bytes(tail)))
    want, segments, names = TG.check_valid(gpu_ctx, items, seg_min=1)
    assert set(segments) == {2, 3} and "gunzip_probe" in names and "gunzip_inflate" in names, names


# ---- e. targz ------------------------------------------------------------------------------------------------------------------

def crate_tars():
    cargo = ("pkg-1.0/Cargo.toml", b"[package]\nname = \"pkg\"\n" * 9)
    noise = gen.incompressible(5, 3000)
    return [make_tar("gnu", [cargo, ("pkg-1.0/src/lib.rs", gen.pseudo_text(700, seed=11))]),
            make_tar("gnu", [("pkg-1.0/noise.bin", noise), cargo]),
            make_tar("gnu", [("pkg-1.0/noise.bin", noise[:700]), ("pkg-1.0/README", b"nothing")])]


def test_targz_random_encodings(gpu_ctx):
    items = []
    for k, tar in enumerate(crate_tars()):
        for seed in range(6):
            s, _ = B.encode(tar, random.Random(100 * k + seed))
            items.append(B.gz_member(s, tar))
    want, status, scanned = TT.check(gpu_ctx, items, b"/Cargo.toml")
    assert status == [0] * 12 + [TM.E_NOENT] * 6, status


def test_targz_every_cut_of_a_random_encoding(gpu_ctx):
    tar = crate_tars()[0]
    s, rec = B.encode(tar, random.Random(7), flush_p=0.5)
    full = B.gz_member(s, tar)
    assert {k for k, _ in rec.blocks} == {B.STORED, B.FIXED, B.DYNAMIC} and len(full) < 8000, (rec.blocks, len(full))
    # what zlib fed one byte at a time hands out, from one pass over the stream: after byte j it has produced cum[j + 1] bytes
    d, out, cum = zlib.decompressobj(-15), b"", [0]
    for j in range(len(s)):
        out += d.decompress(s[j:j + 1])
        cum.append(len(out))
    assert d.eof and out == tar
    items = [full[:k] for k in range(len(full) + 1)]
    prefix = [None if k < 10 else (out, "end", full[10 + len(s):k]) if k >= 10 + len(s) else (out[:cum[k - 10]], "input", b"") for k in range(len(full) + 1)]
    assert TM.inflate_prefix(items[500][10:]) == prefix[500] and TM.inflate_prefix(items[-3][10:]) == prefix[-3]
    scan = 16 << 10                                              # (the tar has 10 KiB: the scratch of the batch stays small)
    for whole in (0, 1):
        want = [TM.find(f, whole, b"", b"/Cargo.toml", scan, inflated=p) for f, p in zip(items, prefix)]
        status, got, _ = TT.run_batch(gpu_ctx, items, b"/Cargo.toml", whole=[whole] * len(items), scan_cap=scan)
        assert [(st, g) for st, g in zip(status, got)] == [(w[0], w[1]) for w in want]
        other = TM.E_CORRUPT if whole else TM.E_MORE
        first_ok = status.index(0)
        assert status[:first_ok] == [other] * first_ok and status[first_ok:] == [0] * (len(items) - first_ok)


# ---- f. damage through gunzip --------------------------------------------------------------------------------------------------

def test_damaged_streams_as_members(gpu_ctx):
    """rejection_cases and every cut of the two truncation streams, each as a member with a plain header and eight bytes of trailer:
    alone, and as the second member behind a clean member with two full flushes.  gzip.decompress refuses every one of them."""
    trunc, _, _ = B.truncation_cases()
    t = gen.pseudo_text(6000, seed=2)
    clean = TG.flushed([t[:2000], t[2000:4000], t[4000:]], zlib.Z_FULL_FLUSH)
    assert M.expect(clean, 1) == (t, 1, 3)
    items, rooms, damaged = [], [], []
    for k, (what, s, n) in enumerate(B.rejection_cases() + trunc):
        m = B.gz_member(s, bytes(n))
        for f, room in ((m, n + 300), (clean + m, len(t) + n + 300)):
            assert M.outcome(f, room)[0] == "bad", what
            items.append(f); rooms.append(room); damaged.append(True)
        if k % 8 == 0:
            items.append(clean); rooms.append(len(t)); damaged.append(False)
    status, got, mem, segments, names = TG.run_batch(gpu_ctx, items, rooms, seg_min=1)
    for i, bad in enumerate(damaged):
        if bad:
            assert status[i] != OK and got[i] == b"", (i, status[i])
        else:
            assert status[i] == OK and got[i] == t and (mem[i], segments[i]) == (1, 3), (i, status[i])


def test_gunzip_every_cut(gpu_ctx):
    t = gen.pseudo_text(1400, seed=6)
    first = TG.flushed([t[:400], t[400:800], t[800:1100]], zlib.Z_FULL_FLUSH)
    f = first + TG.gz(t[1100:])
    assert len(f) < 1000 and M.expect(f, 1) == (t, 2, 4), (len(f), M.expect(f, 1)[1:])
    items = [f[:k] for k in range(len(f) + 1)]
    want = [M.outcome(s, len(t)) for s in items]
    assert [k for k, w in enumerate(want) if w[0] == "ok"] == [0, len(first), len(f)]
    status, got, mem, segments, names = TG.run_batch(gpu_ctx, items, [len(t)] * len(items), seg_min=1)
    for k, w in enumerate(want):
        if w[0] == "ok":
            assert status[k] == OK and got[k] == w[1], (k, status[k])
        else:
            assert w[0] == "bad" and status[k] != OK and got[k] == b"", (k, w[0], status[k])


# ---- g. small gunzip edges -----------------------------------------------------------------------------------------------------

def test_crc_of_members_behind_the_first_at_many_lengths(gpu_ctx):
    """k_gunzip_single folds the CRC-32 of every member behind the first itself (wave_crc): 64 lanes, each a segment of the content"""
    noise = gen.incompressible(21, 70_000)
    small = SOUP + b"".join(TG.gz(noise[n:2 * n], 1 + n % 9) for n in range(201))
    big = SOUP + b"".join(TG.gz(noise[:n], 6) for n in (4095, 4096, 4097, 70_000))
    bad = bytearray(SOUP + TG.gz(noise[:100]) + TG.gz(noise[:133]) + TG.gz(noise[:7]))
    at = len(SOUP) + len(TG.gz(noise[:100])) + len(TG.gz(noise[:133])) - 8
    bad[at] ^= 1                                                  # the CRC-32 in the trailer of the third member
    bad = bytes(bad)
    for f in (small, big, bad):
        assert M.candidates(f, 1)[1]
    want, segments, names = TG.check_valid(gpu_ctx, [small, big], seg_min=1)
    assert [w[1:] for w in want] == [(202, 1), (5, 1)] and names == SINGLE_PASS, names
    assert M.outcome(bad, 4096) == ("bad",)
    status, got, _, _, names = TG.run_batch(gpu_ctx, [bad, small], [4096, len(want[0][0])], seg_min=1)
    assert status == [E_CHECKSUM, OK] and got[1] == want[0][0] and names == SINGLE_PASS, (status, names)


def stored_file_with_candidates(over):
    """a level-0 file whose raw candidate count is 16 + len // 256 + over"""
    for k in range(8, 64):
        for fill in range(0, 256, 5):
            f = TG.gz(b"\x1f\x8b\x08" * k + b"a" * (1000 + fill), 0)
            if len(M.candidates(f, 1)[0]) == 16 + len(f) // 256 + over:
                return f
    raise AssertionError("no such file")


def test_candidate_list_exactly_full_and_one_over(gpu_ctx):
    full, over = stored_file_with_candidates(0), stored_file_with_candidates(1)
    assert not M.candidates(full, 1)[1] and M.candidates(over, 1)[1]
    want, segments, names = TG.check_valid(gpu_ctx, [full], seg_min=1)
    assert "gunzip_probe" in names and "gunzip_single" not in names, names
    want, segments, names = TG.check_valid(gpu_ctx, [over], seg_min=1)
    assert names == SINGLE_PASS, names


def test_tiny_items(gpu_ctx):
    a = TG.gz(b"tiny") + TG.gz(b"")
    items = [a[:k] for k in range(25)] + [(b"\x00\x00\xff\xff" + a)[:k] for k in range(25)] + [(b"\x1f\x8b\x08\xe0" + a[4:])[:k] for k in range(25)]
    want = [M.outcome(s, 16) for s in items]
    assert want[0] == ("ok", b"") and want[len(TG.gz(b"tiny"))] == ("ok", b"tiny") and [w[0] for w in want].count("ok") == 4 and [w[0] for w in want].count("unsup") == 21
    status, got, _, _, _ = TG.run_batch(gpu_ctx, items, [16] * len(items), seg_min=1)
    for k, w in enumerate(want):
        if w[0] == "ok":
            assert status[k] == OK and got[k] == w[1], (k, status[k])
        else:
            assert status[k] != OK and got[k] == b"" and (w[0] != "unsup" or status[k] == E_UNSUPPORTED), (k, w[0], status[k])


def test_stored_data_that_ends_like_a_flush(gpu_ctx):
    """00 00 FF FF as the last bytes of a non-empty stored block: a true block boundary that is also a candidate"""
    items = []
    for dist in (3, 60):                                         # the match of the last block stays inside its piece, or reaches back
        bw = B.Bits()
        B.fixed_block(bw, list(b"in front of the stored block. " * 4), final=0)
        B.stored_block(bw, b"stored data that ends like a flush\x00\x00\xff\xff", final=0)
        B.fixed_block(bw, list(b" and behind it") + [("m", 25, dist)])
        items.append(B.gz_member(bw.bytes(), inflated(bw.bytes())))
    # the 65,535-byte block of a level-0 file, and the same block between two Huffman pieces
    t = gen.pseudo_text(9000, seed=31)
    data = gen.incompressible(41, 65_531) + b"\x00\x00\xff\xff"
    c = zlib.compressobj(0, zlib.DEFLATED, 31, 9)               # (memory level 9: stored blocks of the maximum 65,535)
    level0 = c.compress(data + t[:3000]) + c.flush()
    assert level0[10:15] == b"\x00\xff\xff\x00\x00" and level0[15 + 65_531:15 + 65_535] == b"\x00\x00\xff\xff"
    items.append(level0)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    s = c.compress(t[:5000]) + c.flush(zlib.Z_FULL_FLUSH) + b"\x00\xff\xff\x00\x00" + data + B.deflate(t[5000:], 9)
    items.append(B.gz_member(s, t[:5000] + data + t[5000:]))
    want, segments, names = TG.check_valid(gpu_ctx, items, seg_min=1)
    assert segments[0] == 2 and segments[1] == 1 and segments[2] >= 2 and segments[3] == 3, segments
    assert "gunzip_probe" in names and "gunzip_inflate" in names, names


def test_empty_level_0_member_between_members(gpu_ctx):
    empty = TG.gz(b"", 0)
    assert empty[10:15] == b"\x01\x00\x00\xff\xff"
    f = TG.gz(gen.text(3000)) + empty + TG.gz(gen.pseudo_text(2000, seed=3), 9)
    want, segments, names = TG.check_valid(gpu_ctx, [f, empty + empty, empty + TG.gz(b"x")], seg_min=1)
    assert [w[1] for w in want] == [3, 2, 2]


# ---- h. beyond 4 GiB -----------------------------------------------------------------------------------------------------------

def test_gunzip_sources_and_rooms_beyond_4_gib(gpu_ctx):
    import numpy as np
    import torch
    T = 1 << 32
    size = T + (1 << 20)
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * size:
        pytest.skip(f"two regions of 4 GiB + 1 MiB need {3 * size >> 20} MiB of free device memory, {free >> 20} MiB are free")
    d_src = torch.empty(size, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(size, dtype=torch.uint8, device="cuda")
    text = B.TEXT
    datas = [text[:40_000], text[40_000:140_000], text[150_000:150_900], text[200_000:260_000]]
    files = [TG.flushed([d[at:at + len(d) // 3 + 1] for at in range(0, len(d), len(d) // 3 + 1)], zlib.Z_FULL_FLUSH) for d in datas]
    want = [M.expect(f, 1) for f in files]
    assert [w[1:] for w in want] == [(1, 3)] * 4 and len(files[0]) > 2002 and max(len(f) for f in files) < 150_000
    # source / room: across the line / above it, above / across, above / above, above / above
    src_off = [T - 1001, T + 300_001, T + 500_001, T + 700_001]
    out_off = [T + 700_000, T - 30_000, T + 100_000, T + 400_001]
    W = 64

    def windows(o, k):
        """the guard windows of a room: around it, and where offsets cut to 32 bits would put its bytes above the line"""
        return [(o - W, o), (o + k, o + k + W), (max(max(o, T) - T - W, 0), o + k - T + W)]
    for f, o in zip(files, src_off):
        d_src[o:o + len(f)] = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()
    for d, o in zip(datas, out_off):
        for lo, hi in windows(o, len(d)):
            d_out[lo:hi] = TG.GUARD
    status, off, ln, mem, segments = gpu_ctx.gunzip_batch(d_src, src_off, [len(f) for f in files], d_out, [len(d) for d in datas], out_off=out_off, seg_min=1)
    assert list(status) == [OK] * 4 and [int(x) for x in ln] == [len(d) for d in datas] and list(mem) == [1] * 4 and list(segments) == [3] * 4
    for d, o in zip(datas, out_off):
        assert d_out[o:o + len(d)].cpu().numpy().tobytes() == d
        for lo, hi in windows(o, len(d)):
            assert (d_out[lo:hi] == TG.GUARD).all().item(), (o, lo)
    del d_src, d_out
    torch.cuda.empty_cache()

