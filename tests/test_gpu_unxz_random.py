"""znippy_unxz_batch on the device against the random scripts (tests/lzma_random.py), the deterministic sweeps and the check-less
mutants (tests/xz_cases.py).  tests/test_lzma_random_cpu.py and tests/test_xz_build_cpu.py hold every file against liblzma and
assert what they cover; here the device must give the same bytes and verdicts.  Sources at odd offsets, guard bytes around every
room, measure mode agreeing with the full call (unxz_checks.py)."""
import pytest

import lzma_random as R
import xz_cases as K
from unxz_checks import E_CHECKSUM, E_CORRUPT, OK, arbiter, check_valid, run_batch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("part", range(3))
def test_random_scripts(gpu_ctx, part):
    """the corpus in three batches; check_valid puts every file to lzma.decompress again"""
    cases = R.corpus()[part::3]
    streams, blocks, unverified, names = check_valid(gpu_ctx, [c[1] for c in cases], [c[2] for c in cases])
    assert blocks == [1] * len(cases) and unverified == [0] * len(cases)


def test_match_geometry(gpu_ctx):
    cases = K.match_geometry()
    streams, blocks, unverified, names = check_valid(gpu_ctx, [c[1] for c in cases], [c[2] for c in cases])
    assert blocks == [c[3] for c in cases]


def test_literal_runs(gpu_ctx):
    f, content, cases = K.literal_runs()
    streams, blocks, unverified, names = check_valid(gpu_ctx, [f], [content])
    assert blocks == [len(cases)]


def test_window_edges(gpu_ctx):
    cases = K.window_edges()
    assert cases[-1][0] == "check field at 248"     # the batch ends with the block that ends where its window does
    check_valid(gpu_ctx, [c[1] for c in cases], [c[2] for c in cases])


def test_check_lengths(gpu_ctx):
    cases = K.check_lengths()
    streams, blocks, unverified, names = check_valid(gpu_ctx, [c[1] for c in cases], [c[2] for c in cases])
    assert blocks == [len(K.CHECK_LENGTHS)] * 2 and unverified == [0, 0] and "unxz_check" in names


def test_check_damage(gpu_ctx):
    """a content byte or a check byte changed: the decoder is content, the check kernel is not"""
    cases = K.check_damage()
    good = K.check_lengths()[0]
    items = [good[1]] + [c[1] for c in cases] + [good[1]]
    status, got, *_ = run_batch(gpu_ctx, items, [len(good[2])] + [c[2] for c in cases] + [len(good[2])])
    assert status[0] == OK and status[-1] == OK and got[0] == good[2] and got[-1] == good[2]
    wrong = [(c[0], st) for c, st in zip(cases, status[1:-1]) if st != E_CHECKSUM]
    assert not wrong, wrong


def test_mutants_without_a_check(gpu_ctx):
    """every single-bit mutant of the LZMA2 bytes of a file with check id 0: nothing but the decoder judges them.  E_CORRUPT exactly
    where liblzma refuses, liblzma's bytes where it accepts"""
    f, content, at, n = K.nocheck_base()
    items = K.nocheck_mutants()
    want = [arbiter(m) for m in items]
    status, got, streams, blocks, unverified, names = run_batch(gpu_ctx, [f] + items, [len(content) + 16] * (len(items) + 1))
    assert (status[0], got[0], unverified[0]) == (OK, content, 1)
    wrong = [(i, st) for i, (st, g, w, u) in enumerate(zip(status[1:], got[1:], want, unverified[1:]))
             if ((st, g) != (E_CORRUPT, b"") if w is None else (st, g, u) != (OK, w, 1))]
    assert not wrong, (len(wrong), wrong[:20])
    assert 10 <= sum(w is not None for w in want) < len(items) / 5 and E_CHECKSUM not in status
