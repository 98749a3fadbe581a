"""What the range-read test modules share (not a test module: pytest does not collect it): device buffers with a sentinel, this
library's own frames, tables of frames laid back to back, the decoded-bytes figure worked out from the geometry, and the two checkers
— one call over a list of ranges, exact bytes, the sentinel everywhere else — for znippy_rows_read_ranges and its verified form."""
import numpy as np

from gpu_cases import make_ctx

BLK = 128 * 1024
SENTINEL = 0xA5
HIGH_BASE = (1 << 40) + 12345
ROW_SIZES = [5_000, 131_072, 131_073, 262_145, 300_001]


def to_dev(a, extra=64):
    import torch
    return torch.from_numpy(np.concatenate([np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray)) else a, np.zeros(extra, np.uint8)])).cuda()


def sentinel(n):
    import torch
    return torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")


def own_frames(level, rows, window_log=0):
    """This library's frames of `rows` at `level` (one znippy_compress each, on a context of its own)."""
    ctx = make_ctx({})
    ctx.set_level(level)
    if window_log:
        ctx.set_window_log(window_log)
    frames = [ctx.compress(r) for r in rows]
    ctx.close()
    return frames


def table_of(ctx, frames, rows, comp=None, out_offset=True, checksum=None, base=0):
    """(table, device blobs, columns) of frames laid back to back."""
    from znippy_amd import hip
    bs = np.array([len(f) for f in frames], np.uint64)
    bo = (np.cumsum(bs) - bs).astype(np.uint64)
    us = np.array([len(r) for r in rows], np.uint64)
    oo = (np.cumsum(us) - us).astype(np.uint64)
    comp = np.ones(len(rows), np.uint8) if comp is None else np.asarray(comp, np.uint8)
    rt = hip.RowTable(ctx, bo + np.uint64(base), bs, us, oo if out_offset else None, np.packbits(comp.astype(bool), bitorder="little"), checksum)
    return rt, to_dev(b"".join(frames)), dict(bo=bo, bs=bs, us=us, oo=oo, comp=comp)


def expected_decoded(ranges, sizes, comp=None):
    """From the geometry alone: per distinct (row, block) a range with bytes overlaps, the block's content size; rows of one block whole."""
    seen = set()
    for row, begin, n in ranges:
        if n == 0 or (comp is not None and not comp[row]):
            continue
        if sizes[row] <= BLK:
            seen.add((row, -1))
        else:
            for k in range(begin // BLK, (begin + n - 1) // BLK + 1):
                seen.add((row, k))
    return sum(sizes[row] if k < 0 else min(BLK, sizes[row] - k * BLK) for row, k in seen)


def boundary_ranges(sizes):
    out = []
    for row, L in enumerate(sizes):
        out += [(row, 0, 1), (row, 0, L), (row, L - 1, 1), (row, L, 0), (row, 0, 0), (row, 10, 1001), (row, 500, 1001)]   # the last two overlap
        if L >= 131_073:
            out += [(row, 131_071, 2), (row, 131_072, 1)]
        if L > 141_000:
            out += [(row, 140_000, 777)]                   # inside block 1
        if L >= 262_145:
            out += [(row, 100_000, 262_145 - 100_000)]     # blocks 0-2
    return out


def read_and_check(rt, d_blobs, rows, ranges, tag, guard=37, packed=False, want_decoded=None, **kw):
    """One call over `ranges` [(row, begin, len)], destinations back to back behind `guard` sentinel bytes: exact bytes, the
    sentinel everywhere else, status 0; returns decoded_bytes."""
    lens = np.array([n for _, _, n in ranges], np.uint64)
    at = (np.cumsum(lens) - lens).astype(np.uint64)
    total = int(lens.sum())
    region = sentinel(guard + total + 101)
    if packed:
        status, decoded = rt.read_ranges(d_blobs, [r for r, _, _ in ranges], [b for _, b, _ in ranges], lens, region[guard:], out_cap=total, **kw)
    else:
        status, decoded = rt.read_ranges(d_blobs, [r for r, _, _ in ranges], [b for _, b, _ in ranges], lens, region,
                                         out_offsets=at + np.uint64(guard), **kw)
    assert (status == 0).all(), (tag, status)
    want = np.full(guard + total + 101, SENTINEL, np.uint8)
    for (row, begin, n), a in zip(ranges, at):
        want[guard + int(a):guard + int(a) + n] = np.frombuffer(rows[row][begin:begin + n], np.uint8)
    got = region.cpu().numpy()
    if not np.array_equal(got, want):
        bad = int(np.nonzero(got != want)[0][0])
        k = int(np.searchsorted(at + np.uint64(guard), bad, side="right")) - 1
        raise AssertionError((tag, "first differing byte", bad, "range", ranges[k] if k >= 0 else None))
    if want_decoded is not None:
        assert decoded == want_decoded, (tag, decoded, want_decoded)
    return decoded


def verified_and_check(rt, d_blobs, rows, ranges, tag, guard=37, packed=False, want=None, **kw):
    """read_and_check for the verified call: exact bytes, the sentinel everywhere else, status 0; (decoded, hashed)."""
    lens = np.array([n for _, _, n in ranges], np.uint64)
    at = (np.cumsum(lens) - lens).astype(np.uint64)
    total = int(lens.sum())
    region = sentinel(guard + total + 101)
    rr, rb = [r for r, _, _ in ranges], [b for _, b, _ in ranges]
    if packed:
        status, decoded, hashed = rt.read_ranges_verified(d_blobs, rr, rb, lens, region[guard:], out_cap=total, **kw)
    else:
        status, decoded, hashed = rt.read_ranges_verified(d_blobs, rr, rb, lens, region, out_offsets=at + np.uint64(guard), **kw)
    assert (status == 0).all(), (tag, status)
    expect = np.full(guard + total + 101, SENTINEL, np.uint8)
    for (row, begin, n), a in zip(ranges, at):
        expect[guard + int(a):guard + int(a) + n] = np.frombuffer(rows[row][begin:begin + n], np.uint8)
    got = region.cpu().numpy()
    if not np.array_equal(got, expect):
        raise AssertionError((tag, "first differing byte", int(np.nonzero(got != expect)[0][0])))
    if want is not None:
        assert (decoded, hashed) == want, (tag, decoded, hashed, want)
    return decoded, hashed
