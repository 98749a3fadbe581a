"""znippy_bunzip2_batch on contexts created with ZNIPPY_POISON: every scratch buffer the call takes (the lists, the slots) is filled
with one byte first, and a valid batch and a status batch must give what a clean context gives — nothing the call reads may be
something it has not written."""
import bz2

import pytest

import bz_model as M
import gen
from bunzip2_checks import OK, measure, run_batch
from gpu_cases import make_ctx
from test_gpu_bunzip2 import damaged, false_candidates

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xA5, 0xFF)


@pytest.fixture(scope="module")
def batches():
    fc, content = false_candidates()
    valid = [bz2.compress(gen.pseudo_text(250_000), 1), fc, bz2.compress(b"abcab" * 20000, 1), bz2.compress(bytes(300_000), 1), b"", bz2.compress(b"", 9)]
    cases, a, b = damaged()
    status = [bz2.compress(a, 1)] + [c[1] for c in cases] + [bz2.compress(b, 1)]
    return valid, [len(bz2.decompress(s)) if s else 0 for s in valid], status


def run_all(ctx, batches):
    valid, rooms, status = batches
    out = []
    for cap in (0, 1):   # one pass, and a slot used again and again
        out.append(run_batch(ctx, valid, rooms, slot_cap=cap)[:4])
        out.append(run_batch(ctx, status, [400_000] * len(status), slot_cap=cap)[:4])
        out.append(measure(ctx, valid + status, slot_cap=cap)[:4])
    return out


def test_poisoned_contexts_agree(gpu_ctx, batches):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    clean = run_all(gpu_ctx, batches)
    assert clean[0][0] == [OK] * len(batches[0]) and clean[0][1][0] == gen.pseudo_text(250_000)
    assert clean[1][0][1:-1] == [M.expect(s, 400_000)[0] for s in batches[2][1:-1]]
    for fill in FILLS:
        ctx = make_ctx({"ZNIPPY_POISON": f"{fill:#04x}"})
        try:
            for _ in range(2):   # (the second round runs on recycled buffers)
                assert run_all(ctx, batches) == clean, hex(fill)
        finally:
            ctx.close()
