"""The scripted input builder (tests/enc_inputs.py) and the corpus made with it (tests/enc_edge_cases.py), checked on the CPU: what
the GPU tests of test_gpu_encoder_edges.py conclude from a frame's trace rests on the inputs holding exactly the repeats their
scripts plant.

  * no 4-gram occurs twice in a plain stream, at the alphabets and skews the corpus uses;
  * in every case's buffer, by brute force, every 4-gram that occurs twice lies wholly inside a planted copy with its source at the
    planted distance (overlapping copies are exempt inside their own span);
  * a plain greedy longest-match parse (64 KiB window, matches of 4 bytes and more) of every case's round gives back exactly the
    round's script: the planted copies are the only ones, and each is as long as planted, no byte more at either end.  Cases that
    plant a copy no such parser can give back say so (exact_parse False: a distance of 65,537);
  * the corpus builds in seconds (measured: 4.2 s; the test holds it below 60)."""
import time

import numpy as np
import pytest

import enc_inputs as E

T0 = time.time()
import enc_edge_cases as K  # noqa: E402

CASES = {c.name: c for c in K.cases()}
BUILD_SECONDS = time.time() - T0


@pytest.mark.parametrize("alpha,skew,n", [(16, 0.0, 60000), (64, 1.0, 100000), (256, 1.2, 131072), (256, 2.0, 40000)])
def test_stream_has_no_repeat(alpha, skew, n):
    st = {}
    d = E.no_repeat_stream(n, bytes(range(alpha)), E.zipf(alpha, skew), 3, st)
    assert len(d) == n and E.check_invariant(d, []) == []
    cnt = np.bincount(np.frombuffer(d, np.uint8), minlength=256)
    assert (cnt > 0).sum() == alpha                                           # every symbol present
    print(alpha, skew, n, st, "top share", cnt.max() / n)


def test_stream_steps_back_when_nothing_is_allowed():
    backs = 0
    for seed in range(20):                                                    # 2 symbols: 16 4-grams, 19 bytes at the very most
        st = {}
        d = E.no_repeat_stream(16 + 3, b"ab", None, seed, st)
        assert len(d) == 19 and E.check_invariant(d, []) == []
        backs += st["back"]
    assert backs > 0
    with pytest.raises(E.BuildError):
        E.no_repeat_stream(40, b"ab", None, 1)


def test_a_planted_copy_has_its_guards():
    b = E.build([(100, 20, 80), (0, 12, 64), (5, 300, 3), (9, 6, 430)], tail=30, seed=4)
    assert E.check_invariant(b.data, b.plants) == []
    assert E.greedy_parse(b.data) == ([(100, 20, 80), (0, 12, 64), (5, 300, 3), (9, 6, 430)], 30)
    bad = bytearray(b.data)
    bad[120] = bad[40]                                                        # the byte behind the first copy continues its source
    assert E.greedy_parse(bytes(bad))[0][0] == (100, 21, 80) and E.check_invariant(bytes(bad), b.plants) != []


def test_corpus_builds_in_seconds():
    print(f"corpus: {len(CASES)} cases, {sum(c.n for c in CASES.values())} bytes in rounds, built in {BUILD_SECONDS:.1f} s")
    assert BUILD_SECONDS < 60 and len(CASES) == len(K.cases())


@pytest.mark.parametrize("name", list(CASES))
def test_only_the_planted_copies_repeat(name):
    c = CASES[name]
    assert E.check_invariant(c.buf, c.plants) == []


@pytest.mark.parametrize("name", list(CASES))
def test_greedy_parse_gives_the_script_back(name):
    c = CASES[name]
    got, tail = E.greedy_parse(c.data)
    if c.exact_parse:
        assert got == [tuple(s) for s in c.script] and tail == c.tail
    else:
        assert sum(s[0] + s[1] for s in got) + tail == c.n
    assert sum(s[0] + s[1] for s in c.script) + c.tail == c.n
