"""One znippy_inflate_batch call and its checker, shared by the test modules that run raw DEFLATE streams (not a test module: pytest
does not collect it).  Sources start at odd offsets; 0xA5 guard bytes stand around the destinations and are checked after the call."""
import zlib

import numpy as np

from deflate_build import classify

OK, E_INVAL, E_DST_SMALL, E_CORRUPT, E_UNSUPPORTED, E_CHECKSUM = 0, -1, -4, -5, -6, -7
GUARD = 0xA5


def run_batch(ctx, items, layout="packed", crc32=None, method=None, gap=37):
    """items: (stream, expected length).  layout: "packed" (out_off NULL), "reversed" (explicit offsets, the last item first, a guard
    gap in front of every destination).  Returns (status, crc_out, list of produced bytes); asserts that every byte outside the
    destinations still holds the guard value."""
    import torch
    n = len(items)
    src_off, pos = [], 1
    for s, _ in items:
        src_off.append(pos)
        pos = (pos + len(s)) | 1                  # every source starts at an odd offset
    src = np.full(pos + 64, 0x5A, np.uint8)
    for (s, _), o in zip(items, src_off):
        src[o:o + len(s)] = np.frombuffer(s, np.uint8)
    lens = [k for _, k in items]
    if layout == "packed":
        out_off, total = None, sum(lens) + gap
        offs = np.cumsum([0] + lens[:-1]) if n else np.zeros(0)
    else:
        offs, at = [0] * n, 0
        for i in reversed(range(n)):
            at += gap
            offs[i] = at
            at += lens[i]
        total = at + gap
        out_off = offs
    d_src = torch.from_numpy(src).cuda()
    d_out = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    status, crc = ctx.inflate_batch(d_src, src_off, [len(s) for s, _ in items], d_out, lens, out_off=out_off, crc32=crc32, method=method)
    img = d_out.cpu().numpy()
    outside = np.ones(total, bool)
    got = []
    for o, k in zip(offs, lens):
        outside[int(o):int(o) + k] = False
        got.append(img[int(o):int(o) + k].tobytes())
    assert (img[outside] == GUARD).all(), "a byte outside the destinations was written"
    return status, crc, got


def check(ctx, cases, layout="packed", accept_only=False):
    """cases: (what, stream, n).  Every status is zlib's verdict; every clean item has zlib's bytes and CRC."""
    want = [classify(s, n) for _, s, n in cases]
    if accept_only:
        for (what, _, _), (st, _) in zip(cases, want):
            assert st == OK, f"zlib itself does not accept the fixture: {what}"
    status, crc, got = run_batch(ctx, [(s, n) for _, s, n in cases], layout)
    for i, ((what, _, n), (st, ref)) in enumerate(zip(cases, want)):
        assert status[i] == st, (what, int(status[i]), st)
        if st == OK:
            assert got[i] == ref, what
            assert int(crc[i]) == zlib.crc32(ref), what
    return status
