"""One znippy_unxz_batch call and its checker, shared by the test modules that run whole xz files (not a test module).  Every source
starts at an odd offset, every room has guard bytes in front of and behind it, and the guards are compared after every batch."""
import lzma

import numpy as np

GUARD = 0xA5
GAP = 37
OK, E_INVAL, E_NOMEM, E_DST_SMALL, E_CORRUPT, E_UNSUPPORTED, E_CHECKSUM = 0, -1, -3, -4, -5, -6, -7


def pack_sources(items):
    src_off, pos = [], 1
    for s in items:
        src_off.append(pos)
        pos = (pos + len(s)) | 1                   # every source starts at an odd offset
    src = np.full(pos + 64, 0x5A, np.uint8)
    for s, o in zip(items, src_off):
        src[o:o + len(s)] = np.frombuffer(s, np.uint8)
    return src, src_off


def run_batch(ctx, items, rooms, src_cap=None):
    """items: files (bytes); rooms: bytes each may produce.  Returns (status, contents, streams, blocks, unverified, kernel names);
    asserts that every byte of the output buffer outside the produced contents of clean items and the rooms of failed ones still
    holds the guard."""
    import torch
    src, src_off = pack_sources(items)
    d_src = torch.from_numpy(src).cuda()
    out_off, at = [], GAP
    for r in rooms:
        out_off.append(at)
        at += r + GAP
    d_out = torch.full((at,), GUARD, dtype=torch.uint8, device="cuda")
    status, off, ln, streams, blocks, unverified = ctx.unxz_batch(d_src, src_off, [len(s) for s in items], d_out, rooms, out_off=out_off, src_cap=src_cap)
    names = [k for k, _ in ctx.kernel_times()]
    img = d_out.cpu().numpy()
    got, clean = [], np.ones(at, bool)
    for st, o, r, k in zip(status, out_off, rooms, ln):
        assert int(k) <= r and (st == 0 or int(k) == 0), (st, k, r)
        got.append(img[o:o + int(k)].tobytes())
        clean[o:o + (int(k) if st == 0 else r)] = False   # (inside the room of a failed item the bytes are unspecified)
    assert (img[clean] == GUARD).all(), "a byte outside the rooms was written"
    return [int(x) for x in status], got, [int(x) for x in streams], [int(x) for x in blocks], [int(x) for x in unverified], names


def measure(ctx, items):
    """measure mode -> (status, sizes, streams, blocks, unverified, kernel names)"""
    import torch
    src, src_off = pack_sources(items)
    d_src = torch.from_numpy(src).cuda()
    status, ln, streams, blocks, unverified = ctx.unxz_sizes(d_src, src_off, [len(s) for s in items])
    names = [k for k, _ in ctx.kernel_times()]
    return [int(x) for x in status], [int(x) for x in ln], [int(x) for x in streams], [int(x) for x in blocks], [int(x) for x in unverified], names


def arbiter(item):
    """What lzma.decompress makes of the whole item, or None where it refuses it."""
    try:
        return lzma.decompress(item)
    except (lzma.LZMAError, EOFError):
        return None


def check_valid(ctx, items, want, slack=0, liblzma=True):
    """every item is a valid file whose content is want[i], in a room of exactly that (+ slack).  liblzma: lzma.decompress must give the
    same (False for the items it reads differently: stream padding, see the header).  Measure mode must report the same sizes and
    counts as the full call."""
    if liblzma:
        for i, (s, w) in enumerate(zip(items, want)):
            assert (lzma.decompress(s) if s else b"") == w, i
    status, got, streams, blocks, unverified, names = run_batch(ctx, items, [len(w) + slack for w in want])
    for i, (w, st, g) in enumerate(zip(want, status, got)):
        assert st == OK and g == w, (i, st, len(g), len(w))
    m = measure(ctx, items)
    assert m[:5] == ([OK] * len(items), [len(w) for w in want], streams, blocks, unverified) and set(m[5]) <= {"unxz_tail"}, m
    return streams, blocks, unverified, names
