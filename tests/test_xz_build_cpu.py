"""liblzma (through Python's lzma module) against everything tests/xz_build.py and tests/lzma_build.py assemble: it is the arbiter of
every hand-built case the GPU tests run.  Valid files must decode to the bytes the builders claim; damaged files must be refused,
apart from the stated deviations (bytes behind a stream that lzma.decompress drops, filters this project does not decode)."""
import lzma

import pytest

import lzma_build as L
import xz_build as X
import xz_cases as K
from unxz_checks import arbiter


def test_builder_equals_the_library_on_an_empty_stream():
    assert X.stream([], X.CHECK_CRC64) == lzma.compress(b"")
    assert X.crc64(b"123456789") == 0x995DC9BBDF1939FA and [X.check_size(i) for i in (0, 1, 3, 4, 6, 7, 10, 15)] == [0, 4, 4, 8, 8, 16, 32, 64]
    assert [X.dict_bytes(X.dict_prop(d)) for d in (4096, 4097, 1 << 20, 3 << 20)] == [4096, 6144, 1 << 20, 3 << 20]


@pytest.mark.parametrize("check", [X.CHECK_NONE, X.CHECK_CRC32, X.CHECK_CRC64, X.CHECK_SHA256])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_blocks_and_checks(check, n):
    parts = [bytes([65 + i]) * (100 * i) + b"tail" for i in range(n)]
    for sizes in (False, True):
        assert lzma.decompress(X.xz(parts, check=check, header_sizes=sizes)) == b"".join(parts)
    assert lzma.decompress(X.xz([parts[0], b""] + parts[1:], check=check)) == b"".join(parts)


def test_valid_cases():
    for name, f, content in K.small_shapes():
        assert (lzma.decompress(f) if f else b"") == content, name
    for name, f, content, kinds in K.chunk_shapes():
        assert lzma.decompress(f) == content, name
    for name, f, content, streams, blocks, unverified, same in K.containers():
        if same:
            assert lzma.decompress(f) == content, name
        elif same is False:   # the stated deviation: what stands behind stream padding is dropped
            assert content.startswith(lzma.decompress(f)) and lzma.decompress(f) != content, name
        else:                 # padding behind the last stream: lzma.decompress refuses what the xz tool reads
            assert arbiter(f) is None, name


def test_chunk_kinds():
    kinds = {name: k for name, _, _, k in K.chunk_shapes()}
    k = kinds["300 KB of text"]
    assert k[0] >= 0xE0 and len(k) >= 4 and all(0x80 <= c < 0xA0 for c in k[1:-1]) and k[-1] == 0, k
    k = kinds["random bytes then text"]
    assert k[0] == 1 and 2 in k and any(0xC0 <= c < 0xE0 for c in k), k
    k = kinds["two raw streams in one block"]
    assert k[0] >= 0xE0 and sum(c >= 0xE0 for c in k) == 2, k
    k = kinds["2 MiB + 1 of a phrase"]
    assert len(k) == 3 and k[0] == 0xE0 | 0x1F and k[1] & 0x1F == 0, k   # a chunk of exactly 2 MiB, then one byte


def test_scripted_cases():
    cases = {name: (f, content, w) for name, f, content, w in K.scripted()}
    assert len(cases) == 5
    for name, (f, content, w) in cases.items():
        assert lzma.decompress(f) == content, name
    assert cases["a literal in all 12 states"][2].lit_states == set(range(12))
    assert cases["carries through runs of 0xFF"][2].carry_run >= 2
    w = cases["rep1-3 and short rep"][2]
    assert {7, 8, 10, 11} <= set(w.states)
    assert len(cases["every distance slot"][1]) - 7 == 65536 + sum(2 * (3 + s % 5) for s in range(32))


def test_distance_limits():
    """What liblzma makes of a match that reaches exactly as far as it may and one byte further: the bytes since the dictionary
    reset, and the declared dictionary size (4 KiB; liblzma's buffer is not larger than that)."""
    lits = [("lit", 65 + i % 26) for i in range(5000)]
    for dist, prop, ok in ((5000, X.dict_prop(8192), True), (5001, X.dict_prop(8192), False), (4096, 0, True), (4097, 0, False)):
        f, content = K.scripted_file(L.Writer().lzma(lits + [("match", dist, 5)]), prop=prop)
        assert (arbiter(f) == content) == ok and (ok or arbiter(f) is None), (dist, prop)


def test_what_may_follow_an_uncompressed_chunk():
    """liblzma's rule, found with hand-built chunk sequences: an uncompressed chunk changes neither the LZMA state nor what the next
    chunk has to bring.  Behind 0x01 (dictionary reset) an LZMA chunk must bring properties; behind 0x02 it may go on without any
    reset, with the probabilities, the state and rep0-3 it had, and its matches reach into the uncompressed bytes."""
    lits = lambda s: [("lit", c) for c in s]
    head = lits(b"abcdefgh") + [("match", 3, 4)]
    for control in (0x80, 0xA0, 0xC0, 0xE0):
        ops = lits(b"XY") if control == 0xE0 else [("lit", 0x58), ("rep", 0, 3), ("match", 14, 6), ("lit", 0x59)]   # (0xE0 empties the dictionary)
        f, content = K.scripted_file(L.Writer().lzma(head).stored(b"0123456789", False).lzma(ops, control=control))
        assert arbiter(f) == content, hex(control)
    for control, ok in ((0x80, False), (0xA0, False), (0xC0, True)):
        f, content = K.scripted_file(L.Writer().stored(b"0123456789", True).lzma(lits(b"XY") + [("match", 5, 4)], control=control))
        assert (arbiter(f) == content) == ok and (ok or arbiter(f) is None), hex(control)


def test_damaged_cases_are_refused():
    cases, good, content = K.damaged()
    assert lzma.decompress(good) == content
    for name, f, status, refused, walk in cases:
        assert status != 0, name
        got = arbiter(f)
        if refused:
            assert got is None, name
        else:
            # the deviations.  Bytes behind the last stream: lzma.decompress drops them when they fail as a stream of their own and
            # refuses them when they are too few to tell.  Filters this project does not decode: liblzma reads the file.
            assert got in (None, content), name


def test_mutant_base():
    f, content = K.mutant_base()
    assert 250 <= len(f) <= 400 and lzma.decompress(f) == content and len(K.mutants()) == 8 * len(f)


# ---- the deterministic sweeps -------------------------------------------------------------------------------------------------------

def test_match_geometry_sweep():
    cases = K.match_geometry()
    assert [c[0] for c in cases] == ["lc 3", "lc 4"]
    for name, f, content, blocks in cases:
        assert lzma.decompress(f) == content, name
        assert blocks == sum(len(K.match_lengths(d)) for d in K.MATCH_DISTANCES) >= 23 * 8
    assert K.match_lengths(1) == [2, 3, 258, 259, 272, 273] and K.match_lengths(64) == [2, 3, 63, 64, 65, 127, 128, 129, 258, 259, 272, 273]
    assert K.match_lengths(274) == [2, 3, 258, 259, 272, 273] and K.match_lengths(200)[2:5] == [199, 200, 201]


def test_literal_run_sweep():
    f, content, cases = K.literal_runs()
    assert lzma.decompress(f) == content
    assert set(cases) == {(k, how) for k in K.LITERAL_RUNS for how in K.RUN_FOLLOWERS} - {(0, "b")}
    assert {62, 63, 64, 65, 127, 128, 129} <= set(K.LITERAL_RUNS)


def test_window_edge_sweep():
    """every case puts what it names where it says, by the model of the decoder's input window"""
    cases = K.window_edges()
    for name, f, content, block, what, at, want in cases:
        assert lzma.decompress(f) == content, name
        offs = K.window_offsets(block)
        assert offs[at] == want, (name, offs[at], want)
        raw_at = len(block.header)
        if what == "control":   # the header, the property byte and the five start bytes follow the control byte
            c, _, off, n = X.chunks_of(block.raw)[1]
            assert c == 0xC0 and raw_at + off == at and [offs[at + i] for i in range(11)] == [(want + i) % 256 for i in range(11)]
        elif what == "last":
            c, _, off, n = X.chunks_of(block.raw)[1]
            assert raw_at + off + n - 1 == at and block.raw[at - raw_at + 1] == 0
        else:
            assert len(block.check_bytes) == 8 and [offs[at + i] for i in range(8)] == [(want + i) % 256 for i in range(8)]
    got = {(what, want) for _, _, _, _, what, _, want in cases}
    assert got >= {("control", r) for r in range(245, 256)} | {("control", 0)} | {("last", r) for r in (255, 0, 1)}
    assert got >= {("check", r % 256) for r in range(248, 257)}
    assert cases[-1][4:] == ("check", cases[-1][5], 248)     # the last item's block ends where the window does


def test_check_length_sweep():
    for name, f, content in K.check_lengths():
        assert lzma.decompress(f) == content and len(content) == sum(K.CHECK_LENGTHS), name
    assert set(range(521)) | {65535, 65536, 65537} == set(K.CHECK_LENGTHS)
    damage = K.check_damage()
    assert len(damage) == 2 * (1 + 4 * 3) + 5 * (4 + 8)
    for name, f, room in damage:
        assert arbiter(f) is None, name


def test_mutants_without_a_check():
    """liblzma's verdict on every single-bit mutant of the LZMA2 bytes of a file without a check: the GPU test asks for the same"""
    f, content, at, n = K.nocheck_base()
    assert 120 <= len(f) <= 180 and lzma.decompress(f) == content and f[at + n - 1] == 0 and f[at] == 0xE0
    kinds = [c[0] for c in X.chunks_of(f[at:at + n])]
    assert kinds == [0xE0, 2, 0x80, 0]
    mutants = K.nocheck_mutants()
    verdicts = [arbiter(m) for m in mutants]
    accepted = [v for v in verdicts if v is not None]
    assert len(mutants) == 8 * n and 10 <= len(accepted) < len(mutants) / 5, (len(mutants), len(accepted))
    assert all(len(v) == len(content) for v in accepted)
