"""liblzma (through Python's lzma module) against the random scripts of tests/lzma_random.py, and what their corpus covers.  The
coverage figures are conditions, not measurements: the seeds and the corpus size are chosen so that the generator alone meets them,
and they are asserted so that a later edit cannot hollow the corpus out.  tests/test_gpu_unxz_random.py runs the same files on the
device."""
import lzma

import lzma_random as R
import xz_build as X

OP_KINDS = ("lit", "match", "rep0", "rep1", "rep2", "rep3", "shortrep")


def union(attr):
    out = set()
    for _, _, _, w in R.corpus():
        out |= getattr(w, attr)
    return out


def test_every_file_decodes_to_the_writers_content():
    corpus = R.corpus()
    assert len(corpus) == R.CORPUS >= 100
    for seed, f, content, w in corpus:
        assert lzma.decompress(f) == content, seed
        assert len(content) < 70_000 or seed % 40 == 20, (seed, len(content))   # (a wave decodes some 2.7 MB/s)


def test_the_generator_is_deterministic():
    a, b = R.script(5), R.script(5)
    assert a.out() == b.out() and a.out() != R.script(6).out()


def test_legal_chunk_sequences():
    pairs = R.legal_pairs()
    assert len(pairs) == 34
    assert {b for a, b in pairs if a == 1} == {0xE0, 0xC0, 1, 2}                      # behind a dictionary reset: properties or no LZMA
    assert all((a, b) in pairs for a in R.LZMA_KINDS + (2,) for b in R.KINDS)
    got = set()
    for _, _, _, w in R.corpus():
        kinds = [c[0] for c in w.chunks]
        assert kinds[0] in (0xE0, 1) and len(kinds) >= 3
        got |= set(zip(kinds, kinds[1:]))
    assert got == pairs, sorted(pairs - got)


def test_every_operation_in_every_state():
    """all seven kinds are reachable from all twelve states (a state says what the last operations were, not what may follow)"""
    got = union("op_states")
    missing = [(k, s) for k in OP_KINDS for s in range(12) if (k, s) not in got]
    assert not missing, missing


def test_every_length_class_at_every_pos_state():
    got = union("len_ps")
    missing = [(which, cls, ps) for which in ("match", "rep") for cls in range(3) for ps in range(16) if (which, cls, ps, 4) not in got]
    assert not missing, missing
    assert {pb for _, _, _, pb in got} == set(range(5))


def test_every_distance_slot_and_align_value():
    assert union("slots") >= set(range(36))      # (slots 33 and above need the 256 KiB lead-in of the "far" scripts)
    assert union("aligns") == set(range(16))


def test_every_property_triple_and_dictionary():
    ws = [w for _, _, _, w in R.corpus()]
    assert {c[3:] for w in ws for c in w.chunks if c[0] >= 0x80} == set(R.PROPS)
    small = [w for w in ws if w.prop == 0]
    assert len(small) == R.CORPUS // 4 and X.dict_bytes(0) == 4096
    assert sum(w.exact_dict for w in small) >= 3 and all(w.exact_dict == 0 for w in ws if w.prop)
    assert any(len({c[3:] for c in w.chunks if c[0] >= 0x80}) > 1 for w in ws)     # properties that change inside a block


def test_dictionary_resets_at_every_residue():
    """an LZMA chunk whose dictionary starts r bytes past a multiple of 16: positions count from there, under pb = 4 and under lp = 4"""
    for which in (5, 4):   # the index of pb, of lp in a chunk record
        got = {c[2] % 16 for _, _, _, w in R.corpus() for c in w.chunks if c[0] >= 0x80 and c[which] == 4}
        assert got >= set(range(1, 16)), (which, sorted(set(range(16)) - got))


def test_matched_literals_hit_and_miss():
    assert union("matched_lits") == {"eq", 0, 1, 2, 3, 4, 5, 6, 7}
