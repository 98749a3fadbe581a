"""znippy_unxz_batch on contexts created with ZNIPPY_POISON: every scratch buffer the call takes (the tail stage's lists and staging
buffer, the job lists) is filled with one byte first, and a valid batch and a status batch must give what a clean context gives —
nothing the call reads may be something it has not written."""
import pytest

import xz_cases as K
from gpu_cases import make_ctx
from unxz_checks import OK, measure, run_batch

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xA5, 0xFF)


@pytest.fixture(scope="module")
def batches():
    valid = [(c[1], c[2]) for c in K.small_shapes()] + [(c[1], c[2]) for c in K.containers()] + [(c[1], c[2]) for c in K.scripted()]
    valid += [K.literal_runs()[:2]] + [(c[1], c[2]) for c in K.window_edges()]
    cases, good, content = K.damaged()
    status = [good] + [c[1] for c in cases] + [good]
    return [v[0] for v in valid], [len(v[1]) for v in valid], [v[1] for v in valid], status, len(content) + 8


def run_all(ctx, batches):
    valid, rooms, contents, status, room = batches
    return [run_batch(ctx, valid, rooms)[:5], run_batch(ctx, status, [room] * len(status))[:5], measure(ctx, valid + status)[:5]]


def test_poisoned_contexts_agree(gpu_ctx, batches):
    clean = run_all(gpu_ctx, batches)
    assert clean[0][0] == [OK] * len(batches[0]) and clean[0][1] == batches[2]
    assert clean[1][0][1:-1] == [c[2] for c in K.damaged()[0]]
    for fill in FILLS:
        ctx = make_ctx({"ZNIPPY_POISON": f"{fill:#04x}"})
        try:
            for _ in range(2):   # (the second round runs on recycled buffers)
                assert run_all(ctx, batches) == clean, hex(fill)
        finally:
            ctx.close()
