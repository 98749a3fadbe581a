"""znippy_tar_list_batch on contexts created with ZNIPPY_POISON: every buffer the call takes (the per-block lists, the staging lists,
the gather's pieces) is filled with one byte first, and a valid batch and a status batch must give what a clean context gives —
nothing the call reads may be something it has not written."""
import pytest

from gpu_cases import make_ctx
from tar_list_checks import expect, run_batch
from test_gpu_tar_list import false_candidates, status_tars
from test_tar_list_cpu import valid_tars
from test_tar_rules_cpu import small

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xA5, 0xFF)


@pytest.fixture(scope="module")
def batches():
    data = small()
    valid = list(valid_tars().values()) + false_candidates()
    status = status_tars() + [data[:k] for k in range(0, len(data), 37)]
    return valid, status


def run_all(ctx, batches):
    valid, status = batches
    return [run_batch(ctx, valid), run_batch(ctx, status), run_batch(ctx, valid, b"pkg-1.0/", b".rs", contents=False), run_batch(ctx, valid + status, measure=True)]


def test_poisoned_contexts_agree(gpu_ctx, batches):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    clean = run_all(gpu_ctx, batches)
    assert clean[0] == expect(batches[0]) and clean[1] == expect(batches[1])
    for fill in FILLS:
        ctx = make_ctx({"ZNIPPY_POISON": f"{fill:#04x}"})
        try:
            for _ in range(2):   # (the second round runs on recycled buffers)
                assert run_all(ctx, batches) == clean, hex(fill)
        finally:
            ctx.close()
