"""The corpus of tests/deflate_build.py proves itself without a GPU: zlib decodes every stream to its content, the builders' own
records show that the shapes the corpus exists for are in it, and the gunzip model accepts every stream as a gzip member and cuts
some of them into pieces.  These are conditions on the inputs of tests/test_gpu_deflate_paths.py: where one fails, the generator is
steered (a shape forced into a stream), the condition is not loosened."""
import time
import zlib

import deflate_build as B
import gz_model as M


def test_huffman_lengths():
    assert B.huffman_lengths([0, 0, 0]) == [0, 0, 0]
    assert B.huffman_lengths([0, 5, 0]) == [0, 1, 0]                       # one used symbol: one 1-bit code
    assert B.huffman_lengths([1, 1, 2, 4]) == [3, 3, 2, 1]
    for n, ratio, limit in [(19, 3.0, 7), (30, 2.0, 15), (286, 1.3, 15), (286, 1.0, 15), (2, 9.0, 15)]:
        lens = B.huffman_lengths([ratio ** -k for k in range(n)], limit)
        assert max(lens) <= limit and min(lens) >= 1
        assert sum(2 ** (limit - x) for x in lens) == 2 ** limit, (n, ratio)  # complete: the Kraft sum is exactly 1
        assert ratio == 1.0 or all(a <= b for a, b in zip(lens, lens[1:]))    # a lighter symbol never has the shorter code


def test_zlib_decodes_every_corpus_stream_to_its_content():
    t = time.time()
    corpus = B.corpus()
    print(f"corpus: {len(corpus)} streams, {sum(len(s) for _, s, _, _ in corpus)} bytes for {sum(len(c) for _, _, c, _ in corpus)} bytes of content, "
          f"built in {time.time() - t:.2f} s")
    assert len(corpus) >= 150 + len(B.SWEEP_SEEDS)
    for what, s, content, _ in corpus:
        d = zlib.decompressobj(-15)
        out = d.decompress(s)
        assert d.eof and d.unused_data == b"" and out == content, what
    assert sum(1 for _, s, _, _ in corpus if len(s) > 3 * 2048) >= 4
    assert any(not content for _, _, content, _ in corpus)


def test_corpus_coverage():
    r = B.corpus_record()
    print("length symbol    :", " ".join(f"{257 + i:>4}" for i in range(29)))
    print("  codes <= 10 bit:", " ".join(f"{x:>4}" for x in r.len_short))
    print("  longer codes   :", " ".join(f"{x:>4}" for x in r.len_long))
    print("distance symbol  :", " ".join(f"{i:>4}" for i in range(30)))
    print("  codes <= 9 bit :", " ".join(f"{x:>4}" for x in r.dist_short))
    print("  longer codes   :", " ".join(f"{x:>4}" for x in r.dist_long))
    phases = {(k, p): 0 for k in (B.STORED, B.FIXED, B.DYNAMIC) for p in range(8)}
    for kp in r.blocks:
        phases[kp] += 1
    for k, name in ((B.STORED, "stored "), (B.FIXED, "fixed  "), (B.DYNAMIC, "dynamic")):
        print(f"{name} block headers at bit 0 - 7:", [phases[(k, p)] for p in range(8)])
    print(f"stored lengths {min(r.stored)} - {max(r.stored)}; {r.flushes} flush points; dynamic blocks without a distance code {r.no_dist}, with a lone one "
          f"{r.lone_dist}; code-length runs across HLIT {r.cross}; 284 + 31: {r.l284_31}")
    assert min(r.len_short) >= 1 and min(r.len_long) >= 1, "a length symbol was never decoded through the primary table, or never through the walk"
    assert min(r.dist_short) >= 1 and min(r.dist_long) >= 1, "a distance symbol was never decoded through the primary table, or never through the walk"
    assert min(phases.values()) >= 1, "a block kind never starts at one of the eight bit phases"
    assert {0, 1} <= set(r.stored) and max(r.stored) >= 1000
    assert r.flushes >= 1 and r.no_dist >= 1 and r.lone_dist >= 1 and r.cross >= 1 and r.l284_31 >= 1
    # the sweep alone reaches every symbol both ways, and a 15-bit distance code exists
    sweep = B.Record()
    for what, _, _, rec in B.corpus():
        if what.startswith("sweep") and "15-bit" not in what:
            sweep.add(rec)
    assert min(sweep.len_short + sweep.len_long + sweep.dist_short + sweep.dist_long) >= 1
    s, content, rec = B.symbol_sweep(3, deep_distance=True)
    assert rec.dist_long[14] >= 1 and rec.dist_long[15] >= 1 and zlib.decompressobj(-15).decompress(s) == content


def test_gunzip_model_accepts_the_corpus_and_cuts_it():
    pieces = []
    for what, s, content, _ in B.corpus():
        got, members, segments = M.expect(B.gz_member(s, content), 1)
        assert got == content and members == 1, what
        pieces.append(segments)
    print("pieces per stream:", {k: pieces.count(k) for k in sorted(set(pieces))})
    # one piece: it decoded alone, or everything joined; three and more: at least one decoded alone behind a flush point.  Joins:
    # a stream with flush points and fewer pieces than flush points + 1
    assert pieces.count(1) >= 1 and max(pieces) >= 3
    joined = [what for (what, _, _, rec), k in zip(B.corpus(), pieces) if rec.flushes and k < 1 + rec.flushes]
    assert joined, "no piece joined its predecessor"
