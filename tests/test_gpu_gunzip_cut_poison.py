"""znippy_gunzip_batch with the block-start search on, on contexts created with ZNIPPY_POISON: both allocations of the call are filled
with one byte first, and bytes, statuses, members, segments and the search's counters must be what a clean context gives — nothing
the call reads may be something it has not written (the slots and the count of passing positions are set by memsets of the call)."""
import gzip
import zlib

import pytest

import deflate_build as D
import gen
from gpu_cases import make_ctx
from gunzip_checks import flushed, gz, run_batch

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xA5, 0xFF)


@pytest.fixture(scope="module")
def batches():
    t = gen.pseudo_text(200_000, seed=71)
    valid = [gz(t), flushed([t[:50_000], t[50_000:120_000]], zlib.Z_SYNC_FLUSH), gz(gen.text(300)), gz(b""), gz(t[:90_000], 1) + gz(t[90_000:], 9)]
    valid += [D.gz_member(s, c) for _, s, c, _ in D.corpus()[::9]]
    rooms = [len(gzip.decompress(s)) for s in valid]
    big = valid[0]
    flip = big[:len(big) // 3] + bytes([big[len(big) // 3] ^ 0x20]) + big[len(big) // 3 + 1:]
    bad = [big, flip, big[:len(big) // 2], big[:-1], big + b"x", big]
    return valid, rooms, bad, [200_000] * 5 + [199_999]


def run_all(ctx, batches):
    valid, rooms, bad, bad_rooms = batches
    out = []
    for cut in (64, 4096):
        ctx.set_gunzip_cut(cut)
        for items, r in ((valid, rooms), (bad, bad_rooms)):
            status, got, members, segments, names = run_batch(ctx, items, r, seg_min=1)
            assert "gunzip_find" in names
            # (inside the room of a failed item the bytes are unspecified: run_batch reports no content for it)
            out.append((status, got, members, segments, ctx.gunzip_cut_stats()))
    return out


def test_poisoned_contexts_agree(batches):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = make_ctx({"ZNIPPY_GZ_CUT": "0"})
    try:
        clean = run_all(ctx, batches)
    finally:
        ctx.close()
    assert clean[0][0] == [0] * len(batches[0]) and clean[0][1][0] == gen.pseudo_text(200_000, seed=71)
    assert clean[1][0][0] == 0 and clean[1][0][-1] == -4 and all(s != 0 for s in clean[1][0][1:5])
    assert clean[0][4][1] > 0 and clean[0][4][2] > 0
    for fill in FILLS:
        ctx = make_ctx({"ZNIPPY_POISON": f"{fill:#04x}", "ZNIPPY_GZ_CUT": "0"})
        try:
            for _ in range(2):   # (the second round runs on recycled buffers)
                assert run_all(ctx, batches) == clean, hex(fill)
        finally:
            ctx.close()
