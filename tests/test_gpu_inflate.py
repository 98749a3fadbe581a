"""znippy_inflate_batch: raw DEFLATE streams decoded on the device, against Python's zlib as arbiter.
Every batch goes through one call; sources start at odd offsets; 0xA5 guard bytes stand around the destinations and are checked
afterwards.  Hand-built streams come from the small bit writer of tests/deflate_build.py, and every one of them is first shown to
zlib, which must accept or reject it as the case intends.  The expected status of any stream with expected length n is what zlib
makes of it:
  raises / does not reach eof / eof with fewer than n bytes -> ZNIPPY_E_CORRUPT;  an (n+1)-th byte -> ZNIPPY_E_DST_SMALL;
  eof with exactly n bytes -> 0 and zlib's bytes."""
import ctypes as C
import zlib

import numpy as np
import pytest

import gen
from deflate_build import (TEXT, Bits, block_kind_cases, classify, deflate, fixed_block, flushed_stream, rejection_cases, stored_block,
                           table_corner_cases, truncation_cases)
from inflate_checks import E_CHECKSUM, E_CORRUPT, E_DST_SMALL, E_INVAL, E_UNSUPPORTED, GUARD, OK, check, run_batch

pytestmark = pytest.mark.gpu


def mutant_streams():
    return [(deflate(TEXT[:200], 6, zlib.Z_FIXED), 200), (deflate(TEXT[:3000], 9), 3000), (deflate(TEXT[5000:5100], 0), 100),
            (deflate(TEXT[:600], 6, zlib.Z_HUFFMAN_ONLY), 600)]


def all_mutants():
    out = []
    for s, n in mutant_streams():
        for bit in range(8 * len(s)):
            m = bytearray(s)
            m[bit >> 3] ^= 1 << (bit & 7)
            out.append((bytes(m), n))
    return out


# ---- 1. every block kind -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["packed", "reversed"])
def test_every_block_kind(gpu_ctx, layout):
    cases = block_kind_cases()
    assert deflate(bytes(70000), 0)[:5] == bytes([0, 0xFF, 0xFF, 0, 0])          # level 0: a first stored block of the maximum 65,535
    check(gpu_ctx, cases, layout, accept_only=True)


# ---- 2. table corners ----------------------------------------------------------------------------------------------------------

def test_table_corners(gpu_ctx):
    check(gpu_ctx, table_corner_cases(), "reversed", accept_only=True)


# ---- 3. rejections -------------------------------------------------------------------------------------------------------------

def test_rejections_between_clean_items(gpu_ctx):
    bad = rejection_cases()
    for what, s, n in bad:
        assert classify(s, n)[0] == E_CORRUPT, f"zlib does not reject the fixture: {what}"
    trunc, (fixed, nf), (dyn, nd) = truncation_cases()
    for what, s, n in trunc:
        assert classify(s, n)[0] == E_CORRUPT, what
    clean = [("clean fixed", fixed, nf), ("clean dynamic", dyn, nd), ("clean stored", deflate(TEXT[:300], 0), 300)]
    cases = []
    for k, c in enumerate(bad + trunc):
        cases += [c, clean[k % 3]]
    status = check(gpu_ctx, cases, "reversed")
    assert (status[0::2] == E_CORRUPT).all() and (status[1::2] == OK).all()


# ---- 4. every single-bit mutant ------------------------------------------------------------------------------------------------

def test_every_single_bit_mutant(gpu_ctx):
    muts = all_mutants()
    want = [classify(s, n) for s, n in muts]
    counts = {k: sum(1 for st, _ in want if st == k) for k in (E_CORRUPT, E_DST_SMALL, OK)}
    print("mutants", len(muts), counts)
    assert len(muts) == sum(8 * len(s) for s, _ in mutant_streams()) and sum(counts.values()) == len(muts)
    status, crc, got = run_batch(gpu_ctx, muts, "reversed", gap=5)
    wrong = [(i, int(status[i]), st) for i, (st, _) in enumerate(want) if status[i] != st]
    assert not wrong, (len(wrong), wrong[:10])
    for i, (st, ref) in enumerate(want):
        if st == OK:
            assert got[i] == ref and int(crc[i]) == zlib.crc32(ref), i


# ---- 5. methods and CRC --------------------------------------------------------------------------------------------------------

def test_methods_and_crc(gpu_ctx):
    a, b = TEXT[:4000], TEXT[4000:4777]
    items = [(deflate(a), len(a)), (deflate(b), len(b)), (a, len(a)), (b, len(b) + 1), (deflate(a), len(a)), (b, len(b))]
    method = [8, 8, 0, 0, 12, 0]
    crcs = [zlib.crc32(a), zlib.crc32(b) ^ 0x8000, zlib.crc32(a), 0, 0, zlib.crc32(b) ^ 1]
    status, crc, got = run_batch(gpu_ctx, items, "reversed", crc32=crcs, method=method)
    assert list(status) == [OK, E_CHECKSUM, OK, E_CORRUPT, E_UNSUPPORTED, E_CHECKSUM]
    assert got[0] == a and got[2] == a
    assert [int(crc[i]) for i in (0, 1, 2, 5)] == [zlib.crc32(a), zlib.crc32(b), zlib.crc32(a), zlib.crc32(b)]   # a mismatch returns the computed value
    status, crc, got = run_batch(gpu_ctx, items[:3], "packed", crc32=None, method=None)                       # method NULL: every item is DEFLATE
    assert list(status) == [OK, OK, classify(a, len(a))[0]] and status[2] != OK and int(crc[1]) == zlib.crc32(b)


# ---- 6. host validation and the call's rules -----------------------------------------------------------------------------------

def test_host_validation_and_call_rules(gpu_ctx):
    import torch
    from znippy_amd import _lib
    L = _lib.lib()
    s = deflate(TEXT[:1000])
    d_src = torch.from_numpy(np.frombuffer(bytes(7) + s, np.uint8).copy()).cuda()
    d_out = torch.full((4096,), GUARD, dtype=torch.uint8, device="cuda")
    big = (1 << 64) - 4
    src_off = [7, 7, big, 7, 7, 7, 7]
    src_len = [len(s), len(s) + 1, 8, len(s), len(s), 1 << 32, len(s)]
    out_off = [0, 1000, 1000, 4096 - 999, big, 1000, 2000]
    out_len = [1000, 1000, 1000, 1000, 1000, 1000, 1000]
    status, _ = gpu_ctx.inflate_batch(d_src, src_off, src_len, d_out, out_len, out_off=out_off)
    assert list(status) == [OK, E_INVAL, E_INVAL, E_DST_SMALL, E_DST_SMALL, E_INVAL, OK]    # past src_cap, overflowing, past out_cap
    img = d_out.cpu().numpy()
    assert img[:1000].tobytes() == TEXT[:1000] and img[2000:3000].tobytes() == TEXT[:1000] and (img[1000:2000] == GUARD).all() and (img[3000:] == GUARD).all()
    # sizes of 4 GiB and more are refused before any kernel (the regions only have to be declared that big)
    status, _ = gpu_ctx.inflate_batch(d_src, [0, 0], [1 << 32, 8], d_out, [8, 1 << 32], out_off=[0, 0], src_cap=1 << 33, out_cap=1 << 33)
    assert list(status) == [E_UNSUPPORTED, E_UNSUPPORTED]
    # n == 0, NULL arguments, n too large, a closed context
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)   # noqa: E731
    st = (C.c_int32 * 1)(99)
    sp, op = C.c_void_p(d_src.data_ptr()), C.c_void_p(d_out.data_ptr())

    def call(h, dsrc, so, sl, dout, ol, n):
        return L.znippy_inflate_batch(h, dsrc, d_src.numel(), so, sl, None, dout, d_out.numel(), None, ol, None, n, st, None)
    assert call(gpu_ctx.h, None, None, None, None, None, 0) == OK
    assert call(gpu_ctx.h, sp, u64(7), u64(len(s)), op, u64(1000), 1) == OK and st[0] == OK
    for args in [(None, u64(7), u64(len(s)), op, u64(1000)), (sp, None, u64(len(s)), op, u64(1000)), (sp, u64(7), None, op, u64(1000)),
                 (sp, u64(7), u64(len(s)), None, u64(1000)), (sp, u64(7), u64(len(s)), op, None)]:
        assert call(gpu_ctx.h, *args, 1) == E_INVAL
    assert call(None, sp, u64(7), u64(len(s)), op, u64(1000), 1) == E_INVAL
    assert call(gpu_ctx.h, sp, u64(7), u64(len(s)), op, u64(1000), (1 << 32) - 16) == E_INVAL
    other = C.c_void_p()
    assert L.znippy_ctx_create(0, None, C.byref(other)) == 0
    t = C.c_void_p()
    bitmap = (C.c_uint8 * 1)(0)
    assert L.znippy_rows_create(other, u64(0), u64(500), bitmap, u64(500), None, None, 0, 1, C.byref(t)) == 0
    L.znippy_ctx_destroy(other)                                # closed, kept alive by its table
    assert call(other, sp, u64(7), u64(len(s)), op, u64(1000), 1) == E_INVAL
    L.znippy_rows_destroy(t)
    torch.cuda.synchronize()


def test_not_a_run_and_kernel_times(gpu_ctx, oracle):
    from test_gpu_ranges import own_frames, sentinel, table_of
    rows = [gen.pseudo_text(300_001, seed=51), gen.incompressible(9, 70_000), gen.text(10_240)]
    comp = [1, 0, 1]
    frames = [f if c else r for f, r, c in zip(own_frames(19, rows), rows, comp)]
    ck = np.stack([np.frombuffer(oracle.blake3(r), np.uint8) for r in rows])
    ck[2] ^= 1                                                  # one mismatch, so that the corrupt list has an entry
    total = sum(len(r) for r in rows)
    items = [(deflate(TEXT[:3000]), 3000), (deflate(TEXT[:100]) + b"trailing bytes", 100)]

    def sequence(mixed_in):
        rt, d_blobs, _ = table_of(gpu_ctx, frames, rows, comp=comp, checksum=ck)
        out = sentinel(total + 64)
        rt.decode_verify_async(d_blobs, out)
        if mixed_in:
            status, crc, got = run_batch(gpu_ctx, items)
            assert list(status) == [OK, OK] and got[0] == TEXT[:3000] and got[1] == TEXT[:100]   # (bytes behind the final block are ignored)
            names = [k for k, _ in gpu_ctx.kernel_times()]
            assert names == ["inflate", "inflate_crc"], names
        counters, corrupt, status = rt.results()
        res = (counters, list(corrupt), status.copy(), rt.digests().copy(), out.cpu().numpy())
        rt.close()
        return res
    plain, mixed = sequence(False), sequence(True)
    assert plain[0]["corrupt_rows"] == 1 and plain[1] == [2]
    for k, (x, y) in enumerate(zip(plain, mixed)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, k


# ---- 7. size and count ---------------------------------------------------------------------------------------------------------

def test_one_big_entry_and_many_small_ones(gpu_ctx):
    big = gen.pseudo_text(3 << 20, seed=3)
    check(gpu_ctx, [("3 MiB", deflate(big, 6), len(big))], "reversed", accept_only=True)
    small = [(f"entry {i}", deflate(TEXT[37 * i:37 * i + 4096], 6), 4096) for i in range(2000)]
    check(gpu_ctx, small, "packed", accept_only=True)


# ---- 8. beyond 4 GiB -----------------------------------------------------------------------------------------------------------

def test_sources_and_destinations_beyond_4_gib(gpu_ctx):
    import torch
    T = 1 << 32
    size = T + (1 << 20)
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * size:
        pytest.skip(f"two regions of 4 GiB + 1 MiB need {3 * size >> 20} MiB of free device memory, {free >> 20} MiB are free")
    d_src = torch.empty(size, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(size, dtype=torch.uint8, device="cuda")
    datas = [TEXT[:40_000], TEXT[40_000:140_000], TEXT[150_000:150_900], TEXT[200_000:260_000]]
    streams = [deflate(d, 6) for d in datas]
    assert len(streams[0]) > 2002
    # source / destination: across the line, above it, below it (destination above), above it (destination across)
    src_off = [T - 1001, T + 300_001, 12_345, T + 500_001]
    out_off = [T + 700_000, T + 100_000, T + 600_001, T - 30_000]
    W = 64

    def windows(o, k):
        """the guard windows of a destination: around it, and where offsets cut to 32 bits would put its bytes above the line"""
        return [(o - W, o), (o + k, o + k + W), (max(max(o, T) - T - W, 0), o + k - T + W)]
    for s, o in zip(streams, src_off):
        d_src[o:o + len(s)] = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda()
    for d, o in zip(datas, out_off):
        for lo, hi in windows(o, len(d)):
            d_out[lo:hi] = GUARD
    status, crc = gpu_ctx.inflate_batch(d_src, src_off, [len(s) for s in streams], d_out, [len(d) for d in datas], out_off=out_off,
                                        crc32=[zlib.crc32(d) for d in datas])
    assert list(status) == [OK] * 4
    for d, o, c in zip(datas, out_off, crc):
        assert d_out[o:o + len(d)].cpu().numpy().tobytes() == d and int(c) == zlib.crc32(d)
        for lo, hi in windows(o, len(d)):
            assert (d_out[lo:hi] == GUARD).all().item(), (o, lo)
    del d_src, d_out
    torch.cuda.empty_cache()


# ---- 9. stored blocks in the middle of a stream: flush points ------------------------------------------------------------------

def test_flush_points_all_over_the_input_window(gpu_ctx):
    """Z_SYNC_FLUSH and Z_FULL_FLUSH write an empty stored block wherever they are asked to: behind a Huffman block, at any byte
    of the stream — also where the decoder's 2 KiB input window has just been loaded anew while the bit buffer still held bytes from
    in front of it, so that the stored block sets the read position back in front of the window.  Streams of several window lengths
    with flushes every 50 to 3,000 bytes; then one flush behind P literal-only bytes for every P of a range in which the empty
    block moves byte by byte across the first two places the window is reloaded at (near stream offsets 2,057 and 4,100)."""
    cases = []
    for piece, kinds in [(50, [zlib.Z_SYNC_FLUSH]), (97, [zlib.Z_FULL_FLUSH]), (211, [zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH]), (500, [zlib.Z_SYNC_FLUSH]),
                         (1301, [zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH]), (3000, [zlib.Z_SYNC_FLUSH])]:
        for k in range(4):
            d = TEXT[10_000 * k:10_000 * k + 40_000 + 13 * k]
            s = flushed_stream(d, piece + k, kinds, 6 if k % 2 else 9)
            assert len(s) > 4 * 2048
            cases.append((f"flush every {piece + k}", s, len(d)))
    for p in range(2600, 7400, 7):
        d = TEXT[:p + 300]
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        s = c.compress(d[:p]) + c.flush(zlib.Z_SYNC_FLUSH if p % 2 else zlib.Z_FULL_FLUSH) + c.compress(d[p:]) + c.flush()
        cases.append((f"one flush behind {p} bytes", s, len(d)))
    check(gpu_ctx, cases, "reversed", accept_only=True)


def test_short_stored_blocks_at_every_byte_around_the_window_reloads(gpu_ctx):
    """Hand-built: a fixed block of P literals (8 bits each), a stored block of 0, 1 or 5 bytes, a final fixed block.  The stored
    block's header begins at bit 10 + 8 P of the stream: P sweeps it byte by byte over stream offsets 2,036 – 2,076 and 4,091 –
    4,136, around the first two places at which the decoder loads its input window anew."""
    text = bytes(b & 0x7F for b in TEXT[:4200])           # literals below 144: 8-bit codes
    pre = Bits()
    fixed_block(pre, list(text), final=0, eob=False)
    tail = list(b"behind the stored block " * 3)
    cases = []
    for lo, hi in ((2035, 2076), (4090, 4136)):
        for p in range(lo, hi):
            for short in (b"", b"x", b"short"):
                bw = Bits()
                bw.b = pre.b[:3 + 8 * p] + [0] * 7        # P literals and the end-of-block code
                stored_block(bw, short, final=0)
                fixed_block(bw, tail)
                cases.append((f"{len(short)} stored bytes behind {p} literals", bw.bytes(), p + len(short) + len(tail)))
    check(gpu_ctx, cases, "packed", accept_only=True)
