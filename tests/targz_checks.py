"""Builders of gzip-compressed tars, one znippy_targz_find_batch call and its checker, shared by the test modules that look for tar
members (not a test module: pytest does not collect it)."""
import gzip
import io

import numpy as np

import gen
import targz_model as M
from test_tar_rules_cpu import LONG, LONGER, make_tar, standard

GUARD = 0xA5
SCAN = 8 << 20


def gz(tar, level=6, name=None):
    b = io.BytesIO()
    with gzip.GzipFile(name or "", "wb", compresslevel=level, fileobj=b, mtime=0) as g:
        g.write(tar)
    return b.getvalue()


def run_batch(ctx, items, suffix, prefix=b"", whole=None, scan_cap=SCAN, out_cap=None, gap=41):
    """items: gzip files (bytes).  Returns (status, list of member bytes, scanned); asserts that d_out outside the packed members and
    the guard bytes around it still hold the guard value, and that the members are packed back to back in array order."""
    import torch
    src_off, pos = [], 1
    for s in items:
        src_off.append(pos)
        pos = (pos + len(s)) | 1                  # every source starts at an odd offset
    src = np.full(pos + 64, 0x5A, np.uint8)
    for s, o in zip(items, src_off):
        src[o:o + len(s)] = np.frombuffer(s, np.uint8)
    d_src = torch.from_numpy(src).cuda()
    if out_cap is None:
        out_cap = sum(len(s) for s in items) * 4 + 4096
    d_buf = torch.full((gap + out_cap + gap,), GUARD, dtype=torch.uint8, device="cuda")
    d_out = d_buf[gap:gap + out_cap]
    status, off, ln, scanned = ctx.targz_find_batch(d_src, src_off, [len(s) for s in items], d_out, suffix, prefix=prefix, whole=whole, scan_cap=scan_cap,
                                                    out_cap=out_cap)
    img = d_buf.cpu().numpy()
    got, at = [], 0
    for st, o, k in zip(status, off, ln):
        if st == 0:
            assert int(o) == at, "members are not packed back to back"
            got.append(img[gap + at:gap + at + int(k)].tobytes())
            at += int(k)
        else:
            assert (int(o), int(k)) == (0, 0)
            got.append(b"")
    assert at <= out_cap and (img[:gap] == GUARD).all() and (img[gap + at:] == GUARD).all(), "a byte outside the packed members was written"
    return [int(x) for x in status], got, [int(x) for x in scanned]


def check(ctx, items, suffix, prefix=b"", whole=None, scan_cap=SCAN):
    want = [M.find(s, 1 if whole is None else whole[i], prefix, suffix, scan_cap) for i, s in enumerate(items)]
    status, got, scanned = run_batch(ctx, items, suffix, prefix, whole, scan_cap)
    for i, (w, st, g, sc) in enumerate(zip(want, status, got, scanned)):
        assert (st, g) == (w[0], w[1]), (i, st, w[0], len(g), len(w[1]))
        if st == 0:
            assert w[2] <= sc <= w[2] + 65535 + 258, (i, sc, w[2])   # (one stored block, one match beyond the member's end)
    return want, status, scanned


def valid_tars():
    tars = [standard(fmt, where) for fmt in ("ustar", "gnu", "pax") for where in ("first", "last", "absent")]
    for fmt in ("ustar", "gnu", "pax"):
        tars.append(make_tar(fmt, [("pkg-1.0/a.txt", b"a"), (LONG, b"long name")] + ([(LONGER, b"longer name")] if fmt != "ustar" else []) +
                             [("pkg-1.0/z.txt", b"zz")]))
    # incompressible bodies: headers in the middle of a 64-literal gather.  Long runs: a 258-byte match overshoots the walk's need
    noise = gen.incompressible(5, 3001)
    tars.append(make_tar("gnu", [("pkg-1.0/noise.bin", noise), ("pkg-1.0/Cargo.toml", noise[:777]), ("pkg-1.0/more.bin", noise[:1500])]))
    tars.append(make_tar("gnu", [("pkg-1.0/zeros.bin", bytes(70001)), ("pkg-1.0/Cargo.toml", b"\0" * 300 + b"x" * 300), ("pkg-1.0/zeros2.bin", bytes(5000))]))
    tars.append(make_tar("gnu", []))
    return tars
