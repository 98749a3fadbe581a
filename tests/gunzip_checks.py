"""Builders of gzip files, one znippy_gunzip_batch call and its checker, shared by the test modules that run whole gzip files (not a
test module: pytest does not collect it).  Every source starts at an odd offset, every room has guard bytes in front of and behind it,
and the guards are compared after every batch."""
import gzip
import io
import struct
import zlib

import numpy as np

import gen
import gz_model as M

GUARD = 0xA5
GAP = 37
OK, E_INVAL, E_DST_SMALL, E_CORRUPT, E_UNSUPPORTED, E_CHECKSUM = 0, -1, -4, -5, -6, -7


def gz(content, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(content) + c.flush()


def flushed(chunks, modes, level=6):
    """one member; modes[i] (or the one mode) is the flush between chunk i and chunk i + 1"""
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    out = b""
    for i, ch in enumerate(chunks):
        out += c.compress(ch)
        if i + 1 < len(chunks):
            out += c.flush(modes[i] if isinstance(modes, (list, tuple)) else modes)
    return out + c.flush()


def with_header(content, flg, extra=b"", name=b"", comment=b"", level=6):
    """a member with a hand-built header: FEXTRA 4, FNAME 8, FCOMMENT 16, FHCRC 2 (two bytes that nobody verifies)"""
    raw = zlib.compressobj(level, zlib.DEFLATED, -15)
    h = b"\x1f\x8b\x08" + bytes([flg]) + bytes(4) + b"\x00\xff"
    if flg & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        h += name + b"\0"
    if flg & 16:
        h += comment + b"\0"
    if flg & 2:
        h += b"\x12\x34"
    return h + raw.compress(content) + raw.flush() + struct.pack("<II", zlib.crc32(content), len(content) & 0xFFFFFFFF)


def run_batch(ctx, items, rooms, seg_min=0, src_cap=None):
    """items: files (bytes); rooms: bytes each may produce.  Returns (status, contents, members, segments, kernel names); asserts that
    every byte of the output buffer outside the produced contents of clean items and the rooms of failed ones still holds the guard."""
    import torch
    src_off, pos = [], 1
    for s in items:
        src_off.append(pos)
        pos = (pos + len(s)) | 1                   # every source starts at an odd offset
    src = np.full(pos + 64, 0x5A, np.uint8)
    for s, o in zip(items, src_off):
        src[o:o + len(s)] = np.frombuffer(s, np.uint8)
    d_src = torch.from_numpy(src).cuda()
    out_off, at = [], GAP
    for r in rooms:
        out_off.append(at)
        at += r + GAP
    d_out = torch.full((at,), GUARD, dtype=torch.uint8, device="cuda")
    status, off, ln, members, segments = ctx.gunzip_batch(d_src, src_off, [len(s) for s in items], d_out, rooms, out_off=out_off, seg_min=seg_min,
                                                           src_cap=src_cap)
    names = [k for k, _ in ctx.kernel_times()]
    img = d_out.cpu().numpy()
    got, clean = [], np.ones(at, bool)
    for st, o, r, k in zip(status, out_off, rooms, ln):
        assert int(k) <= r and (st == 0 or int(k) == 0), (st, k, r)
        got.append(img[o:o + int(k)].tobytes())
        clean[o:o + (int(k) if st == 0 else r)] = False   # (inside the room of a failed item the bytes are unspecified)
    assert (img[clean] == GUARD).all(), "a byte outside the rooms was written"
    return [int(x) for x in status], got, [int(x) for x in members], [int(x) for x in segments], names


def check_valid(ctx, items, seg_min=0, slack=0):
    """every item is a valid file in a room of exactly its content (+ slack): content, members and segments are the model's"""
    want = [M.expect(s, seg_min) for s in items]
    status, got, members, segments, names = run_batch(ctx, items, [len(w[0]) + slack for w in want], seg_min)
    for i, (w, st, g, m, sg) in enumerate(zip(want, status, got, members, segments)):
        assert st == OK and g == w[0], (i, st, len(g), len(w[0]))
        assert (m, sg) == (w[1], w[2]), (i, m, sg, w[1:])
    return want, segments, names


def single_members():
    items = [gz(gen.text(n), level) for n in (0, 1, 63, 64, 65, 70_000) for level in (0, 1, 9)]
    b = io.BytesIO()
    with gzip.GzipFile("access.log", "wb", compresslevel=6, fileobj=b, mtime=0) as g:
        g.write(gen.text(3000))
    items.append(b.getvalue())
    t = gen.text(777)
    items += [with_header(t, 4, extra=b"AB\x03\x00xyz"), with_header(t, 16, comment=b"a comment"), with_header(t, 2),
              with_header(t, 4 | 8 | 16 | 2, extra=b"", name=b"n", comment=b"")]
    return items


def bgzf(content, size):
    out = b""
    for at in range(0, len(content), size):
        part = content[at:at + size]
        raw = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = raw.compress(part) + raw.flush()
        bsize = 12 + 6 + len(body) + 8 - 1
        out += with_header(part, 4, extra=b"BC\x02\x00" + struct.pack("<H", bsize))
    return out + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
