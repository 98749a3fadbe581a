"""znippy_bunzip2_batch on the device: whole bzip2 files, every case compared byte for byte with Python's bz2.decompress (the arbiter
for everything it accepts), statuses with the model of bz_model.py.  Sources at odd offsets and guard bytes around every room
(bunzip2_checks.py)."""
import bz2
import ctypes as C
import os

import numpy as np
import pytest

import bz_build as B
import bz_model as M
import gen
from bunzip2_checks import (E_CHECKSUM, E_CORRUPT, E_DST_SMALL, E_INVAL, E_NOMEM, E_UNSUPPORTED, GUARD, OK, check_valid, measure, run_batch)

pytestmark = pytest.mark.gpu


def bz(data, level=1):
    return bz2.compress(data, level)


@pytest.fixture(scope="module")
def text3():
    """250,000 bytes of text at level 1: three blocks, whose magics start at different bits of a byte"""
    data = gen.pseudo_text(250_000)
    s = bz(data)
    where = M.magic_positions(s)
    assert len(where) == 3 and len({p % 8 for p in where}) > 1, where
    return s, data


def false_candidates():
    """A block whose 256 symbols all have 8-bit codes: its data bits are its symbols as bytes, and among them stand the six bytes of
    the block magic and those of the end magic.  -> (stream of that block and a plain one, content)"""
    fill = [7, 200, 3, 3, 90, 2, 250, 31]
    symbols = fill + [0x31, 0x41, 0x59, 0x26, 0x53, 0x59] + fill[::-1] + [0x17, 0x72, 0x45, 0x38, 0x50, 0x90] + fill + [0x31, 0x41, 0x59, 0x26, 0x53, 0x59, 9]
    blk, content = B.accepted_block(list(range(1, 255)), symbols)
    assert set(blk.tables[0]) == {8}
    tail = gen.text(900)
    return B.stream([blk, B.block_fields(tail)]), content + tail


# ---- 1. valid files --------------------------------------------------------------------------------------------------------------

def test_blocks_at_any_bit(gpu_ctx, text3):
    s, data = text3
    want, streams, blocks, names = check_valid(gpu_ctx, [s, bz(b""), bz(b"x")])
    assert (streams, blocks) == ([1, 1, 1], [3, 0, 1]) and len(bz(b"")) == 14
    assert names[:5] == ["bunzip2_scan", "bunzip2_decode", "bunzip2_walk", "bunzip2_expand", "bunzip2_crc"], names


def test_run_length_edges(gpu_ctx):
    contents = [b"a" * 4, b"a" * 5, b"a" * 255, b"a" * 256, b"a" * 259 + b"b", b"aaaa\x00" * 30000, b"aaaa" + b"\x04" + b"\x04" * 3, b"\x04" * 8 + b"\x04",
                b"\xfb" * 300, b"x" + b"\xfb" * (255 + 255 + 3) + b"y",   # 255 of 0xFB: four of them, the count 0xFB, and 0xFB again
                bytes(1_000_000)]
    items = [bz(c) for c in contents]
    assert len(items[-1]) == 48
    want, streams, blocks, _ = check_valid(gpu_ctx, items)
    # (a block holds 100,000 bytes behind the first run-length step, which turns the million zeros into 19,608: one block, 48 bytes)
    assert blocks == [len(M.magic_positions(s)) for s in items] and blocks[-1] == 1 and want[-1] == contents[-1]


def test_periodic_blocks(gpu_ctx):
    check_valid(gpu_ctx, [bz(b"ab" * 5000), bz(b"abcab" * 20000), bz(b"ab" * 5000 + b"c")])


def test_byte_values_and_sizes(gpu_ctx):
    big = gen.pseudo_text(1_000_000, seed=4)
    items = [bz(bytes(range(256)) * 40), bz(b"\xff" * 1000), bz(b"\x00"), bz(gen.incompressible(3, 120_000)), bz(big, 9)]
    want, streams, blocks, _ = check_valid(gpu_ctx, items)
    assert blocks[-1] == 2 and blocks[3] == 2   # (900,000 bytes in the first block of the level-9 stream: the largest tt)


def test_hand_built_blocks(gpu_ctx):
    data = gen.text(700)
    items = [B.stream([B.block_fields(data, n_groups=g)]) for g in (2, 6)]
    b = B.block_fields(data)                      # a code of length 20, on a symbol the block does not use
    alpha = len(b.used) + 2
    lens = B.flat_lens(alpha)
    lens[min(set(range(2, alpha - 1)) - set(b.symbols))] = 20
    b.tables = [list(lens), list(lens)]
    items.append(B.stream([b]))
    b = B.block_fields(data)                      # more selectors than 18002
    b.n_selectors = 18010
    items.append(B.stream([b]))
    for orig in (0, None):                        # origPtr 0 and n - 1: any origPtr below n names a content
        used = list(range(65, 75))
        symbols = [3, 4, 2, 9, 0, 7, 5, 5, 1, 8, 6, 2]
        n = len(symbols) - 2 + 1 + 2               # (a byte per symbol; the RUNA stands for one, the RUNB for two)
        blk, content = B.block_from_symbols(used, symbols, 0 if orig == 0 else n - 1)
        with pytest.raises(IndexError):
            B.block_from_symbols(used, symbols, n)
        items.append(B.stream([blk]))
    # several blocks of different shapes in one stream, at level 9
    items.append(B.stream([B.block_fields(gen.text(300)), B.block_fields(b"z" * 600), B.block_fields(gen.binary(500))], level=9))
    for s in items:
        assert M.walk(s)[0] == OK
    usable = [s for s in items if accepted(s)]
    assert len(usable) >= len(items) - 2          # (libbz2 refuses a hand-made content that ends inside a run of four)
    check_valid(gpu_ctx, usable)
    status, got, _, _, _ = run_batch(gpu_ctx, items, [2000] * len(items))
    assert status == [OK] * len(items) and got == [M.walk(s)[1] for s in items]


def accepted(s):
    try:
        bz2.decompress(s)
        return True
    except (OSError, ValueError):
        return False


def test_streams_and_rests(gpu_ctx, text3):
    s, data = text3
    one, two = bz(gen.text(5000)), bz(gen.binary(3000))
    items = [one + two + bz(b"") + one, one + b"\0" * 9, one + b"BZ" + two, b"", one + b"not bzip2 at all", s + two, b""]
    want, streams, blocks, _ = check_valid(gpu_ctx, items)
    assert streams == [4, 1, 1, 0, 1, 2, 0] and blocks == [3, 1, 1, 0, 1, 4, 0]


def test_false_candidates(gpu_ctx):
    s, content = false_candidates()
    assert bz2.decompress(s) == content
    rest = bytes([0]) + bytes.fromhex("314159265359") + b"junk" + bytes.fromhex("177245385090") + bytes.fromhex("314159265359") + bytes(40)
    plain = bz(gen.text(2000))
    items = [s, plain + rest, s + rest]
    for it in items:
        assert len(M.magic_positions(it)) > M.walk(it)[3]
    want, streams, blocks, _ = check_valid(gpu_ctx, items)
    assert blocks == [2, 1, 2] and [len(M.magic_positions(it)) for it in items] == [4, 3, 6]


# ---- 2. statuses -----------------------------------------------------------------------------------------------------------------

def damaged():
    """-> [(name, item, expected status or None for "whatever the model says")]"""
    a, b = gen.text(1200), gen.binary(800)
    s = B.stream([B.block_fields(a), B.block_fields(b)])
    recs = M.walk(s)[4]
    assert bz2.decompress(s) == a + b and len(recs) == 2
    out = [("cut in the header", s[:3], E_CORRUPT), ("cut in a block", s[:recs[0][1] // 16], E_CORRUPT),
           ("cut between blocks", s[:recs[1][0] // 8], E_CORRUPT), ("cut in the second magic", s[:recs[1][0] // 8 + 3], E_CORRUPT),
           ("cut in the trailer", s[:-2], E_CORRUPT), ("cut in the end magic", s[:-7], E_CORRUPT),
           ("block CRC", B.flip(s, 32 + 48 + 5), E_CHECKSUM), ("combined CRC", B.flip(s, 8 * (len(s) - 3)), E_CHECKSUM),
           ("huffman data", B.flip(s, recs[0][1] - 300), None), ("huffman data 2", B.flip(s, recs[1][1] - 41), None)]

    def one(name, want=E_CORRUPT, **fields):
        blk = B.block_fields(a)
        for k, v in fields.items():
            setattr(blk, k, v)
        out.append((name, B.stream([blk]), want))
    n = len(B.rle1(a))
    one("origPtr = n", orig=n)
    one("origPtr huge", orig=(1 << 24) - 1)
    one("nGroups 1", n_groups=1)
    one("nGroups 7", n_groups=7)
    one("nSelectors 0", n_selectors=0)
    one("selector index = nGroups", selectors=[2] * 40, raw_symbol_bits=[(0, 8)])
    one("few selectors", n_selectors=3)
    one("length 0", start_lens=[0, 5])
    one("length 21", start_lens=[21, 5])
    alpha = len(B.block_fields(a).used) + 2
    one("over-subscribed", tables=[[1] * alpha, [1] * alpha], raw_symbol_bits=[(0, 8)])
    flat = B.flat_lens(alpha)
    assert alpha < 1 << flat[0]
    one("no such code", raw_symbol_bits=[(0, flat[0]), ((1 << flat[0]) - 1, flat[0])])
    one("randomised", want=E_UNSUPPORTED, randomised=1)
    out.append(("run beyond the level", B.stream([B.Block([65], [B.RUNB] * 17 + [2], 0, 0)]), E_CORRUPT))
    out.append(("run within level 9", B.stream([B.Block([0], [B.RUNB] * 17 + [2], 0, 0)], level=9), E_CHECKSUM))
    out.append(("run beyond any level", B.stream([B.Block([65], [B.RUNB] * 21 + [2], 0, 0)], level=9), E_CORRUPT))
    out.append(("no symbols", B.stream([B.Block([65], [2], 0, 0)]), E_CORRUPT))
    out.append(("no used byte", B.stream([B.Block([], [1], 0, 0, tables=[[1, 1], [1, 1]])]), E_CORRUPT))
    out.append(("neither magic", B.stream([B.block_fields(a)], end_magic=0x177245385091), E_CORRUPT))
    out.append(("BZh0", B.stream([B.block_fields(a)], head=b"BZh0"), E_CORRUPT))
    out.append(("BZx1", B.stream([B.block_fields(a)], head=b"BZx1"), E_CORRUPT))
    good = bz(a)
    out.append(("damaged second stream", good + B.flip(good, 300), None))
    out.append(("second stream cut", good + good[:40], E_CORRUPT))
    out.append(("second stream BZh0", good + b"BZh0" + good[4:], E_CORRUPT))
    return out, a, b


def test_statuses(gpu_ctx):
    cases, a, b = damaged()
    good = bz(a)
    room = 400_000
    items = [good] + [c[1] for c in cases] + [good, good]
    rooms = [room] * (len(items) - 2) + [len(a) - 1, len(a)]
    status, got, streams, blocks, _ = run_batch(gpu_ctx, items, rooms)
    assert (status[0], got[0]) == (OK, a) and (status[-1], got[-1]) == (OK, a) and status[-2] == E_DST_SMALL
    seen = set()
    for i, (name, item, want) in enumerate(cases, 1):
        model = M.expect(item, room)
        assert want is None or model[0] == want, (name, model[0], want)
        assert status[i] == model[0] and got[i] == model[1] and (streams[i], blocks[i]) == model[2:], (name, status[i], model[0])
        seen.add(model[0])
    assert {E_CORRUPT, E_CHECKSUM, E_UNSUPPORTED} <= seen
    # the stated deviation: the arbiter drops a damaged later stream without a word
    name, item, _ = cases[[c[0] for c in cases].index("damaged second stream")]
    assert bz2.decompress(item) == a and M.expect(item, room)[0] != OK


def test_header_bit_flips(gpu_ctx):
    """a status test: every flip of the first 200 bits of the block header gives the model's verdict, and no guard changes"""
    data = gen.text(2000)
    s = bz(data)
    items, want = [], []
    for bit in range(32, 232):
        f = B.flip(s, bit)
        try:
            want.append(M.expect(f, len(data) + 500))
            items.append(f)
        except M.Undecided:
            pass
    assert len(items) >= 196
    status, got, streams, blocks, _ = run_batch(gpu_ctx, items + [s], [len(data) + 500] * (len(items) + 1))
    assert (status[-1], got[-1]) == (OK, data)
    for i, w in enumerate(want):
        assert (status[i], got[i], streams[i], blocks[i]) == w, (i, status[i], w[0])
    assert {E_CORRUPT, E_CHECKSUM, E_UNSUPPORTED} <= {w[0] for w in want}


# ---- 3. what must not change a result --------------------------------------------------------------------------------------------

def test_slot_cap(gpu_ctx, text3):
    s, data = text3
    fc, content = false_candidates()
    bad = B.flip(s, M.walk(s)[4][1][0] + 48 + 3)          # the second block's CRC
    items = [s, fc, bz(bytes(300_000)), bad, s + fc]
    rooms = [len(data), len(content), 300_000, len(data), len(data) + len(content)]
    base = run_batch(gpu_ctx, items, rooms)
    assert base[0] == [OK, OK, OK, E_CHECKSUM, OK] and base[1][0] == data and base[1][1] == content and base[1][4] == data + content
    for cap in (1, 2):
        assert run_batch(gpu_ctx, items, rooms, slot_cap=cap)[:4] == base[:4], cap
        assert measure(gpu_ctx, items, slot_cap=cap)[1] == [len(data), len(content), 300_000, len(data), len(data) + len(content)]


def test_split_spacing(gpu_ctx, text3):
    s, data = text3
    items = [s, bz(b"abcab" * 20000), bz(bytes(range(256)) * 40), bz(b"q")]
    base = run_batch(gpu_ctx, items, [len(bz2.decompress(i)) for i in items])
    assert base[0] == [OK] * 4
    old = os.environ.get("ZNIPPY_BZ_SPLIT")
    try:
        for split in ("64", "1", "1000000", "4000000000"):
            os.environ["ZNIPPY_BZ_SPLIT"] = split
            assert run_batch(gpu_ctx, items, [len(g) for g in base[1]])[:4] == base[:4], split
    finally:
        if old is None:
            del os.environ["ZNIPPY_BZ_SPLIT"]
        else:
            os.environ["ZNIPPY_BZ_SPLIT"] = old


def test_scratch_budget(gpu_ctx):
    import torch
    s = bz(gen.text(1000))
    d_src = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda()
    old = os.environ.get("ZNIPPY_BZ_SCRATCH_MB")
    try:
        os.environ["ZNIPPY_BZ_SCRATCH_MB"] = "5"       # less than one slot
        with pytest.raises(Exception) as e:
            gpu_ctx.bunzip2_sizes(d_src, [0], [len(s)])
        assert getattr(e.value, "code", None) == E_NOMEM
        os.environ["ZNIPPY_BZ_SCRATCH_MB"] = "6"       # one slot
        assert [list(x) for x in gpu_ctx.bunzip2_sizes(d_src, [0], [len(s)])[:2]] == [[OK], [1000]]
    finally:
        if old is None:
            del os.environ["ZNIPPY_BZ_SCRATCH_MB"]
        else:
            os.environ["ZNIPPY_BZ_SCRATCH_MB"] = old


def test_measure_mode(gpu_ctx, text3):
    import torch
    s, data = text3
    cases, a, b = damaged()
    items = [s, bz(b""), b"", bz(bytes(1_000_000)), bz(a) + bz(b)] + [c[1] for c in cases]
    dummy = torch.full((4096,), GUARD, dtype=torch.uint8, device="cuda")
    status, sizes, streams, blocks, names = measure(gpu_ctx, items)
    assert (dummy.cpu().numpy() == GUARD).all()
    assert "bunzip2_expand" not in names and "bunzip2_crc" not in names and "bunzip2_decode" in names
    assert status[:5] == [OK] * 5 and sizes[:5] == [len(data), 0, 0, 1_000_000, len(a) + len(b)] and streams[:5] == [1, 1, 0, 1, 2]
    for i, (name, item, _) in enumerate(cases, 5):
        st, content, n_streams, n_blocks, _ = M.walk(item)
        if st == E_CHECKSUM:    # no CRC is checked: the length of what is there
            assert status[i] == OK and sizes[i] > 0, name
        else:
            assert (status[i], sizes[i]) == (st, len(content)), (name, status[i], st)


def test_host_validation_and_call_rules(gpu_ctx):
    import torch
    from znippy_amd import _lib
    L = _lib.lib()
    t = gen.text(1000)
    s = bz(t)
    d_src = torch.from_numpy(np.frombuffer(bytes(7) + s, np.uint8).copy()).cuda()
    d_out = torch.full((4096,), GUARD, dtype=torch.uint8, device="cuda")
    big = (1 << 64) - 4
    src_off = [7, 7, big, 7, 7, 7, 7]
    src_len = [len(s), len(s) + 1, 8, len(s), len(s), 1 << 32, len(s)]
    out_off = [0, 1000, 1000, 4096 - 999, big, 1000, 2000]
    status, _, ln, _, _ = gpu_ctx.bunzip2_batch(d_src, src_off, src_len, d_out, [1000] * 7, out_off=out_off)
    assert list(status) == [OK, E_INVAL, E_INVAL, E_DST_SMALL, E_DST_SMALL, E_INVAL, OK]    # past src_cap, overflowing, past out_cap
    assert list(ln) == [1000, 0, 0, 0, 0, 0, 1000]
    img = d_out.cpu().numpy()
    assert img[:1000].tobytes() == t and img[2000:3000].tobytes() == t and (img[1000:2000] == GUARD).all() and (img[3000:] == GUARD).all()
    # sizes of 4 GiB and more are refused before any kernel; an item of no bytes is no stream and no content
    status, _, ln, streams, _ = gpu_ctx.bunzip2_batch(d_src, [0, 0, 7], [1 << 32, 8, 0], d_out, [8, 1 << 32, 5], out_off=[0, 0, 0], src_cap=1 << 33, out_cap=1 << 33)
    assert list(status) == [E_UNSUPPORTED, E_UNSUPPORTED, OK] and list(ln) == [0, 0, 0] and list(streams) == [0, 0, 0]
    # rooms packed back to back when no offsets are given
    status, off, ln, _, _ = gpu_ctx.bunzip2_batch(d_src, [7, 7], [len(s), len(s)], d_out, [1000, 1000])
    assert list(status) == [OK, OK] and list(off) == [0, 1000] and d_out[:2000].cpu().numpy().tobytes() == t * 2
    # n == 0, NULL arguments, n too large
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)   # noqa: E731
    st = (C.c_int32 * 1)(99)
    ol = u64(99)
    sp, op = C.c_void_p(d_src.data_ptr()), C.c_void_p(d_out.data_ptr())

    def call(h, dsrc, so, sl, dout, room, out_len, n, out_cap=d_out.numel()):
        return L.znippy_bunzip2_batch(h, dsrc, d_src.numel(), so, sl, n, dout, out_cap, None, room, 0, out_len, st, None, None)
    assert call(gpu_ctx.h, None, None, None, None, None, None, 0) == OK
    assert call(gpu_ctx.h, sp, u64(7), u64(len(s)), op, u64(1000), ol, 1) == OK and st[0] == OK and ol[0] == 1000
    for args in [(None, u64(7), u64(len(s)), op, u64(1000), ol), (sp, None, u64(len(s)), op, u64(1000), ol), (sp, u64(7), None, op, u64(1000), ol),
                 (sp, u64(7), u64(len(s)), None, u64(1000), ol), (sp, u64(7), u64(len(s)), op, None, ol), (sp, u64(7), u64(len(s)), op, u64(1000), None)]:
        assert call(gpu_ctx.h, *args, 1) == E_INVAL
    assert call(None, sp, u64(7), u64(len(s)), op, u64(1000), ol, 1) == E_INVAL
    assert call(gpu_ctx.h, sp, u64(7), u64(len(s)), op, u64(1000), ol, (1 << 32) - 16) == E_INVAL
    # measure mode: no buffer and no capacity; the rooms are not read
    ol[0] = 99
    assert call(gpu_ctx.h, sp, u64(7), u64(len(s)), None, None, ol, 1, out_cap=0) == OK and st[0] == OK and ol[0] == 1000


def test_not_a_run(gpu_ctx, oracle, text3):
    from test_gpu_ranges import own_frames, sentinel, table_of
    rows = [gen.pseudo_text(300_001, seed=51), gen.incompressible(9, 70_000), gen.text(10_240)]
    comp = [1, 0, 1]
    frames = [f if c else r for f, r, c in zip(own_frames(19, rows), rows, comp)]
    ck = np.stack([np.frombuffer(oracle.blake3(r), np.uint8) for r in rows])
    ck[2] ^= 1                                                  # one mismatch, so that the corrupt list has an entry
    total = sum(len(r) for r in rows)
    s, data = text3
    items = [s, bz(gen.text(100))]

    def sequence(mixed_in):
        rt, d_blobs, _ = table_of(gpu_ctx, frames, rows, comp=comp, checksum=ck)
        out = sentinel(total + 64)
        rt.decode_verify_async(d_blobs, out)
        if mixed_in:
            status, got, streams, blocks, names = run_batch(gpu_ctx, items, [len(data), 100])
            assert status == [OK, OK] and got == [data, gen.text(100)] and blocks == [3, 1]
            assert names == ["bunzip2_scan", "bunzip2_decode", "bunzip2_walk", "bunzip2_expand", "bunzip2_crc"], names
        counters, corrupt, status = rt.results()
        res = (counters, list(corrupt), status.copy(), rt.digests().copy(), out.cpu().numpy())
        rt.close()
        return res
    plain, mixed = sequence(False), sequence(True)
    assert plain[0]["corrupt_rows"] == 1 and plain[1] == [2]
    for k, (x, y) in enumerate(zip(plain, mixed)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, k
