"""znippy_unxz_batch on the device: whole xz files.  Every case is compared byte for byte with the content its builder knows and with
Python's lzma.decompress wherever that reads the whole item (tests/test_xz_build_cpu.py holds the hand-built ones against it);
damaged files have the status their construction implies.  Sources at odd offsets and guard bytes around every room
(unxz_checks.py)."""
import pytest

import gen
import xz_build as X
import xz_cases as K
from unxz_checks import E_CORRUPT, E_DST_SMALL, E_INVAL, OK, arbiter, check_valid, measure, run_batch

pytestmark = pytest.mark.gpu


# ---- 1. valid small shapes ---------------------------------------------------------------------------------------------------------

def test_small_shapes(gpu_ctx):
    cases = K.small_shapes()
    streams, blocks, unverified, names = check_valid(gpu_ctx, [c[1] for c in cases], [c[2] for c in cases])
    assert streams[:4] == [0, 1, 1, 1] and blocks[:4] == [0, 0, 1, 3] and unverified == [0] * len(cases)
    assert names == ["unxz_tail", "unxz_decode", "unxz_check"], names   # one round: every file is one stream


# ---- 2. chunks -----------------------------------------------------------------------------------------------------------------------

def test_chunk_shapes(gpu_ctx):
    cases = K.chunk_shapes()
    kinds = {c[0]: c[3] for c in cases}
    k = kinds["300 KB of text"]
    assert k[0] >= 0xE0 and len(k) >= 4 and all(0x80 <= c < 0xA0 for c in k[1:-1]), k           # several chunks that reset nothing
    k = kinds["random bytes then text"]
    assert k[0] == 1 and 2 in k and any(0xC0 <= c < 0xE0 for c in k[k.index(2):]), k              # uncompressed, then new properties
    assert sum(c >= 0xE0 for c in kinds["two raw streams in one block"]) == 2                     # a dictionary reset inside the block
    k = kinds["2 MiB + 1 of a phrase"]
    assert len(k) == 3 and k[0] == 0xFF and k[1] & 0x1F == 0, k                                   # a chunk of exactly 2 MiB, then one byte
    check_valid(gpu_ctx, [c[1] for c in cases], [c[2] for c in cases])


# ---- 3. scripted operations -------------------------------------------------------------------------------------------------------

def test_scripted_operations(gpu_ctx):
    cases = K.scripted()
    assert [c[0] for c in cases] == ["length 2, length 273, distance 1", "every distance slot", "rep1-3 and short rep", "a literal in all 12 states",
                                     "carries through runs of 0xFF"]
    assert cases[3][3].lit_states == set(range(12)) and cases[4][3].carry_run >= 2
    check_valid(gpu_ctx, [c[1] for c in cases], [c[2] for c in cases])


def test_what_follows_an_uncompressed_chunk(gpu_ctx):
    """liblzma's rule (test_xz_build_cpu.py finds it): behind 0x02 an LZMA chunk may go on with no reset at all, behind 0x01 it
    must bring properties"""
    import lzma_build as L
    lits = lambda s: [("lit", c) for c in s]
    head = lits(b"abcdefgh") + [("match", 3, 4)]
    items, want = [], []
    for control in (0x80, 0xA0, 0xC0):
        f, content = K.scripted_file(L.Writer().lzma(head).stored(b"0123456789", False).lzma([("lit", 0x58), ("rep", 0, 3), ("match", 14, 6), ("lit", 0x59)],
                                                                                              control=control))
        items.append(f)
        want.append(content)
    f, content = K.scripted_file(L.Writer().stored(b"0123456789", True).lzma(lits(b"XY") + [("match", 5, 4)], control=0xC0))
    check_valid(gpu_ctx, items + [f], want + [content])
    bad = [K.scripted_file(L.Writer().stored(b"0123456789", True).lzma(lits(b"XY") + [("match", 5, 4)], control=c))[0] for c in (0x80, 0xA0)]
    assert all(arbiter(b) is None for b in bad)
    assert run_batch(gpu_ctx, bad, [64, 64])[0] == [E_CORRUPT, E_CORRUPT]


def test_distance_limits(gpu_ctx):
    """a match may reach the first byte behind the dictionary reset and the declared dictionary size, and not a byte further: liblzma
    5.2 draws both lines at the same byte (test_xz_build_cpu.py), so there is no deviation to state"""
    import lzma_build as L
    lits = [("lit", 65 + i % 26) for i in range(5000)]
    items, want = [], []
    for dist, prop, ok in ((5000, X.dict_prop(8192), True), (5001, X.dict_prop(8192), False), (4096, 0, True), (4097, 0, False)):
        f, content = K.scripted_file(L.Writer().lzma(lits + [("match", dist, 5)]), prop=prop)
        assert (arbiter(f) == content) == ok
        items.append(f)
        want.append(content if ok else None)
    status, got, *_ = run_batch(gpu_ctx, items, [5005] * 4)
    assert status == [OK, E_CORRUPT, OK, E_CORRUPT] and [g for g in got if g] == [w for w in want if w]


# ---- 4. containers -------------------------------------------------------------------------------------------------------------------

def test_containers(gpu_ctx):
    cases = K.containers()
    same = [c for c in cases if c[6]]
    streams, blocks, unverified, names = check_valid(gpu_ctx, [c[1] for c in same], [c[2] for c in same])
    assert (streams, blocks, unverified) == ([c[3] for c in same], [c[4] for c in same], [c[5] for c in same])
    # the stated deviation: lzma.decompress drops what stands behind stream padding (or refuses the padding); this call reads it as the xz tool does
    other = [c for c in cases if not c[6]]
    assert len(other) == 3 and all(arbiter(c[1]) != c[2] for c in other)
    streams, blocks, unverified, names = check_valid(gpu_ctx, [c[1] for c in other], [c[2] for c in other], liblzma=False)
    assert (streams, blocks, unverified) == ([c[3] for c in other], [c[4] for c in other], [c[5] for c in other])
    assert names[-2:] == ["unxz_decode", "unxz_check"] and set(names[:-2]) == {"unxz_tail"} and len(names) >= 4, names   # a round per stream


def test_measure_mode_launches_no_decoder(gpu_ctx):
    cases = K.containers()
    status, sizes, streams, blocks, unverified, names = measure(gpu_ctx, [c[1] for c in cases] + [b""])
    assert status == [OK] * (len(cases) + 1) and sizes == [len(c[2]) for c in cases] + [0] and set(names) == {"unxz_tail"}
    assert measure(gpu_ctx, [b"", b""])[5] == []


def test_a_long_index_takes_a_round_of_its_own(gpu_ctx):
    parts = [bytes([i & 255, i >> 8]) for i in range(700)]      # 700 blocks: an index of some 2 KiB, more than the tail read
    f = X.xz(parts, check=X.CHECK_CRC32)
    streams, blocks, unverified, names = check_valid(gpu_ctx, [f, X.xz([b"neighbour"])], [b"".join(parts), b"neighbour"])
    assert blocks == [700, 1] and names.count("unxz_tail") == 2, names   # the tail with the first 12 bytes, then the index


# ---- 5. damaged input ----------------------------------------------------------------------------------------------------------------

def test_damaged_files(gpu_ctx):
    cases, good, content = K.damaged()
    items = [good] + [c[1] for c in cases] + [good]
    status, got, *_ = run_batch(gpu_ctx, items, [len(content) + 8] * len(items))
    assert status[0] == OK and status[-1] == OK and got[0] == content and got[-1] == content
    wrong = [(c[0], st, c[2]) for c, st in zip(cases, status[1:-1]) if st != c[2]]
    assert not wrong, wrong
    # measure mode sees the container alone: what the walk finds, it reports; a damaged block goes unseen
    m = measure(gpu_ctx, items)
    wrong = [(c[0], st) for c, st in zip(cases, m[0][1:-1]) if st != (c[2] if c[4] else OK)]
    assert not wrong and set(m[5]) == {"unxz_tail"}, wrong


# ---- 6. mutants ------------------------------------------------------------------------------------------------------------------------

def test_every_single_bit_mutant(gpu_ctx):
    f, content = K.mutant_base()
    items = K.mutants()
    want = [arbiter(m) for m in items]
    # mutants that only touch bytes the two stated deviations cover (what stands behind stream padding): a flipped bit inside the
    # one stream of this file is never one of them
    excluded = []
    assert excluded == []
    status, got, *_ = run_batch(gpu_ctx, items, [len(content) + 16] * len(items))
    wrong = [(i, st) for i, (st, g, w) in enumerate(zip(status, got, want)) if (w is None) != (st != OK) or (w is not None and g != w)]
    assert not wrong, wrong[:20]
    assert sum(w is not None for w in want) < len(items) // 20   # (nearly every mutant is refused)


# ---- 7. rooms and measure mode -----------------------------------------------------------------------------------------------------------

def test_a_room_one_byte_short(gpu_ctx):
    t = gen.pseudo_text(5000, seed=5)
    a, b, c = X.xz([t[:2000], t[2000:3000]]), X.xz([t[:3000], t[3000:]], check=X.CHECK_CRC32), X.xz([t[::-1]])
    status, got, *_ = run_batch(gpu_ctx, [a, b, c], [3000, 4999, 5000])
    assert status == [OK, E_DST_SMALL, OK] and got[0] == t[:3000] and got[2] == t[::-1]
    status, got, *_ = run_batch(gpu_ctx, [a, b, c], [3000, 5001, 5000])
    assert status == [OK, OK, OK] and got[1] == t


def test_arguments(gpu_ctx):
    import numpy as np
    import torch
    f = X.xz([b"hello"])
    d_src = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()
    d_out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    st, off, ln, *_ = gpu_ctx.unxz_batch(d_src, [0, 8, 0], [len(f), len(f), len(f)], d_out, [5, 5, 5], out_off=[0, 8, 62])
    assert list(st) == [OK, E_INVAL, E_DST_SMALL] and bytes(d_out[:5].cpu().numpy()) == b"hello"   # a source beyond src_cap, a room beyond out_cap
    st, *_ = gpu_ctx.unxz_batch(d_src, [], [], d_out, [])
    assert len(st) == 0
