"""The xz files of the unxz tests (not a test module): generated and hand-built valid files with their content, damaged files with
the status their construction implies.  tests/test_xz_build_cpu.py holds every one of them against liblzma; the GPU tests run them."""
import functools
import random

import gen
import lzma_build as L
import xz_build as X
from unxz_checks import E_CHECKSUM, E_CORRUPT, E_UNSUPPORTED

PROP_1M = X.dict_prop(1 << 20)
PHRASE = b"All work and no play makes Jack a dull boy. "


def scripted_file(writer, check=X.CHECK_CRC32, prop=PROP_1M):
    raw, content = writer.out()
    return X.stream([X.Block(content, check, raw=raw, prop=prop)], check), content


@functools.lru_cache(None)
def small_shapes():
    """[(name, file, content)]"""
    t, s = gen.pseudo_text(60_000), gen.text(1500)
    cases = [("an empty item", b"", b""), ("an empty stream", X.stream([], X.CHECK_CRC64), b""), ("one byte", X.xz([b"x"]), b"x"),
             ("an empty block between two", X.xz([s, b"", s[::-1]]), s + s[::-1])]
    assert len(cases[1][1]) == 32
    for p in range(10):
        cases.append((f"preset {p}", X.xz([t], check=X.CHECK_CRC32, preset=p, dict_size=1 << 20), t))
    for lc, lp, pb in ((0, 0, 0), (4, 0, 4), (0, 4, 0), (3, 0, 2)):
        cases.append((f"lc/lp/pb {lc}/{lp}/{pb}", X.xz([t[:20_000]], lc=lc, lp=lp, pb=pb), t[:20_000]))
    cases.append(("dictionary 4 KiB", X.xz([t], dict_size=4096), t))
    return cases


@functools.lru_cache(None)
def chunk_shapes():
    """[(name, file, content, control bytes of the chunks)]"""
    t = _words(300_000, 3)
    out = []

    def add(name, content, raw=None, prop=None):
        b = X.Block(content, X.CHECK_CRC32, raw=raw, prop=prop, dict_size=1 << 20)
        out.append((name, X.stream([b], X.CHECK_CRC32), content, [c[0] for c in X.chunks_of(b.raw)]))

    add("300 KB of text", t)
    add("random bytes then text", gen.incompressible(5, 140_000) + t[:50_000])
    a, b = t[:30_000], t[10_001:45_000]
    ra, prop = X.raw_lzma2(a, dict_size=1 << 20)
    rb, _ = X.raw_lzma2(b, dict_size=1 << 20)
    add("two raw streams in one block", a + b, ra[:-1] + rb, prop)
    add("2 MiB + 1 of a phrase", (PHRASE * ((1 << 21) // len(PHRASE) + 2))[:(1 << 21) + 1])
    return out


def _words(n, seed):
    """text of a large vocabulary: it compresses to about half, so 300 KB of it are several LZMA chunks"""
    r = random.Random(seed)
    vocab = ["".join(r.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(r.randrange(2, 10))) for _ in range(20_000)]
    out, size = [], 0
    while size < n:
        out.append(r.choice(vocab))
        size += len(out[-1]) + 1
    return " ".join(out).encode()[:n]


def _filler(n, seed):
    r = random.Random(seed)
    return bytes(r.randrange(256) for _ in range(n))


@functools.lru_cache(None)
def scripted():
    """[(name, file, content, writer)]"""
    out = []

    def add(name, w):
        f, content = scripted_file(w)
        out.append((name, f, content, w))

    lits = lambda s: [("lit", c) for c in s]
    add("length 2, length 273, distance 1",
        L.Writer().lzma(lits(b"abcdefgh") + [("match", 8, 2), ("lit", 0x21), ("match", 1, 273), ("match", 3, 273), ("lit", 0x7A), ("match", 1, 2)]))
    # every distance slot a history of 64 KiB reaches: the slot's least and greatest distance, and the distance equal to the bytes produced
    w = L.Writer().stored(_filler(65536, 1), True)
    ops, made = [], 65536
    for slot in range(0, 2 * 16):
        lo = slot if slot < 4 else (2 | (slot & 1)) << ((slot >> 1) - 1)
        hi = lo if slot < 4 else lo + (1 << ((slot >> 1) - 1)) - 1
        for d in (lo, hi):
            ops += [("match", d + 1, 2 + slot % 5), ("lit", slot)]
            made += 3 + slot % 5
    ops.append(("match", made, 7))   # (0-based made - 1: slot 32)
    assert L.dist_slot(made - 1) == 32
    add("every distance slot", w.lzma(ops, control=0xC0))
    add("rep1-3 and short rep",
        L.Writer().lzma(lits(b"0123456789abcdefghijklmnopqrstuvwxyz") +
                        [("match", 5, 3), ("match", 11, 4), ("match", 17, 5), ("match", 23, 6), ("rep", 3, 4), ("rep", 2, 9), ("rep", 1, 20), ("rep", 0, 2),
                         ("shortrep",), ("lit", 0x41), ("rep", 3, 273), ("shortrep",), ("shortrep",), ("rep", 1, 2), ("lit", 0x42)]))
    m, r, sr = ("match", 4, 3), ("rep", 0, 3), ("shortrep",)
    w = L.Writer().lzma(lits(b"wxyz") + [m] + lits(b"abc") + [m, m] + lits(b"d") + [m, r] + lits(b"e") + [r] + lits(b"fgh") + [sr] + lits(b"ijk") +
                        lits(b"l") + [r] + lits(b"m") + [sr] + lits(b"n") + [m, sr] + lits(b"o"))
    add("a literal in all 12 states", w)
    # long carries: random operations until a carry has gone through a run of two pending 0xFF bytes
    for seed in range(200):
        rnd = random.Random(seed)
        w, ops = L.Writer(lc=0, lp=0, pb=0), [("lit", 7)]
        n = 1
        while n < 3000:
            if rnd.random() < 0.7:
                ops.append(("lit", rnd.randrange(256)))
                n += 1
            else:
                k = rnd.randrange(2, 12)
                ops.append(("match", rnd.randrange(1, n + 1), k))
                n += k
        w.lzma(ops)
        if w.carry_run >= 2:
            add("carries through runs of 0xFF", w)
            break
    return out


@functools.lru_cache(None)
def containers():
    """[(name, file, content, streams, blocks, unverified, lzma.decompress reads it the same way: True, False where it drops what
    stands behind stream padding, None where it refuses the file)]"""
    t = gen.pseudo_text(9_000, seed=7)
    six = [t[i * 1500:(i + 1) * 1500 - i] for i in range(6)]
    a, b = X.xz(six[:2], check=X.CHECK_CRC32), X.xz(six[2:5], check=X.CHECK_CRC64, header_sizes=True)
    ca, cb = b"".join(six[:2]), b"".join(six[2:5])
    return [("6 blocks", X.xz(six), b"".join(six), 1, 6, 0, True),
            ("6 blocks with header sizes", X.xz(six, header_sizes=True), b"".join(six), 1, 6, 0, True),
            ("two streams, two checks", a + b, ca + cb, 2, 5, 0, True),
            ("two streams, padding between", a + bytes(8) + b, ca + cb, 2, 5, 0, False),
            ("two streams, padding behind", a + b + bytes(4), ca + cb, 2, 5, 0, None),
            ("two streams, padding between and behind", b + bytes(4) + a + bytes(12), cb + ca, 2, 5, 0, False),
            ("an empty stream between two", a + X.stream([], 0) + b, ca + cb, 3, 5, 0, True),
            ("SHA-256", X.xz(six[:3], check=X.CHECK_SHA256), b"".join(six[:3]), 1, 3, 3, True),
            ("no check", X.xz(six[:2], check=X.CHECK_NONE), b"".join(six[:2]), 1, 2, 2, True),
            ("a reserved check id", X.xz(six[:1], check=2), six[0], 1, 1, 1, True),
            ("CRC32 then none", a + X.xz(six[5:], check=X.CHECK_NONE), ca + six[5], 2, 3, 1, True)]


def _one(raw, content=b"", prop=PROP_1M, check=X.CHECK_CRC32, **kw):
    return X.stream([X.Block(content, check, raw=raw, prop=prop, **kw)], check)


@functools.lru_cache(None)
def damaged():
    """[(name, file, status, liblzma refuses it too, the container walk alone finds it)], the undamaged file and its content"""
    ta, tb = gen.text(700), gen.pseudo_text(900, seed=9)
    CK = X.CHECK_CRC64
    ba, bb = X.Block(ta, CK, header_sizes=True), X.Block(tb, CK)
    recs = [(ba.unpadded, ba.uncomp), (bb.unpadded, bb.uncomp)]
    good = X.stream([ba, bb], CK)
    ix = X.index(recs)
    out = []
    walk = [True]

    def add(name, f, status, refused=True):
        out.append((name, f, status, refused, walk[0]))

    def flip(f, at, bit=0):
        return f[:at] + bytes([f[at] ^ (1 << bit)]) + f[at + 1:]

    st = lambda **kw: X.stream([ba, bb], CK, **kw)
    # ---- the container
    add("footer magic", good[:-1] + b"X", E_CORRUPT)
    add("footer CRC32", flip(good, len(good) - 8), E_CORRUPT)
    add("header magic", b"\xfe" + good[1:], E_CORRUPT)
    add("header CRC32", flip(good, 8), E_CORRUPT)
    add("stream padding that is not zero", good + b"\x00\x00\x00\x01", E_CORRUPT, False)      # (deviation: liblzma drops it)
    add("stream padding of three bytes", good + bytes(3), E_CORRUPT, False)                     # (likewise)
    add("garbage behind the stream", good + b"garbage!", E_CORRUPT, False)                      # (likewise)
    add("stream padding in front", bytes(4) + good, E_CORRUPT)
    add("nothing but padding", bytes(64), E_CORRUPT)
    add("a VLI of 10 bytes", st(index_bytes=X.index([(b"\x80" * 9 + b"\x01", ba.uncomp), recs[1]])), E_CORRUPT)
    add("a VLI with a trailing zero byte", st(index_bytes=X.index([(bytes([ba.unpadded & 0x7F | 0x80, ba.unpadded >> 7 | 0x80, 0]), ba.uncomp), recs[1]])), E_CORRUPT)
    add("an unpadded size of 4", X.stream([], CK, records=[(4, 0)]), E_CORRUPT)
    add("a record count beyond the index", st(index_bytes=X.index(recs, count=1000)), E_CORRUPT)
    add("a record count of 2^62", st(index_bytes=X.index(recs, count=1 << 62)), E_CORRUPT)
    add("a record too few", st(index_bytes=X.index(recs, count=1)), E_CORRUPT)
    add("unpadded sizes that do not add up", st(records=[(ba.unpadded + 4, ba.uncomp), recs[1]]), E_CORRUPT)
    add("unpadded sizes beyond the item", st(records=[((1 << 63) - 4, ba.uncomp), ((1 << 63) - 4, bb.uncomp)]), E_CORRUPT)
    add("header and footer flags differ", st(header=X.stream_header(X.CHECK_CRC32)), E_CORRUPT)
    add("index indicator", st(index_bytes=X.index(recs, indicator=1)), E_CORRUPT)
    add("index padding that is not zero", st(index_bytes=X.index(recs, padding=b"\x01" * (-len(ix) % 4 or 4))), E_CORRUPT)
    add("index CRC32", st(index_bytes=X.index(recs, crc=5)), E_CORRUPT)
    add("a backward size beyond the item", st(footer=X.stream_footer(len(ix), CK, backward=0xFFFF)), E_CORRUPT)
    add("a backward size one too small", st(footer=X.stream_footer(len(ix) - 4, CK)), E_CORRUPT)
    add("a reserved stream flag bit", st(header=X.stream_header(CK, flag0=1), footer=X.stream_footer(len(ix), CK, flag0=1)), E_UNSUPPORTED)
    add("a reserved bit beside the check id", st(header=X.stream_header(CK | 0x10), footer=X.stream_footer(len(ix), CK | 0x10)), E_UNSUPPORTED)
    add("content of 4 GiB", st(records=[(ba.unpadded, 1 << 32), recs[1]]), E_UNSUPPORTED)
    add("content that adds up to 2^64", st(records=[(ba.unpadded, (1 << 63) - 1), (bb.unpadded, (1 << 63) - 1)]), E_UNSUPPORTED)
    for k in range(97, len(good), 97):
        add(f"cut at byte {k}", good[:k], E_CORRUPT)
    # ---- the blocks
    walk[0] = False
    blk =lambda **kw: X.stream([ba, X.Block(tb, CK, **kw)], CK)
    add("a check field that differs", blk(check_bytes=bytes(8)), E_CHECKSUM)
    add("the index claims a byte more", st(records=[recs[0], (bb.unpadded, bb.uncomp + 1)]), E_CORRUPT)
    add("the index claims a byte less", st(records=[recs[0], (bb.unpadded, bb.uncomp - 1)]), E_CORRUPT)
    add("the header's compressed size differs", blk(header=X.block_header(bb.prop, len(bb.raw) + 1, None)), E_CORRUPT)
    add("the header's uncompressed size differs", blk(header=X.block_header(bb.prop, None, len(tb) - 1)), E_CORRUPT)
    add("block header CRC32", blk(header=X.block_header(bb.prop, crc=1)), E_CORRUPT)
    add("block header padding that is not zero", blk(header=X.block_header(bb.prop, padding=b"\x00\x01")), E_CORRUPT)
    add("block header size byte 0", blk(header=X.block_header(bb.prop, size_byte=0)), E_CORRUPT)
    add("a reserved block flag", blk(header=X.block_header(bb.prop, flags=0x04)), E_UNSUPPORTED)
    add("a dictionary byte of 41", blk(header=X.block_header(41)), E_UNSUPPORTED)
    add("a BCJ filter", blk(header=X.block_header(filters=[(X.X86_ID, b""), (X.LZMA2_ID, bytes([bb.prop]))])), E_UNSUPPORTED, False)
    add("a delta filter", blk(header=X.block_header(filters=[(X.DELTA_ID, b"\x00"), (X.LZMA2_ID, bytes([bb.prop]))])), E_UNSUPPORTED, False)
    add("an unknown filter", blk(header=X.block_header(filters=[(0x4000, b"")])), E_UNSUPPORTED)
    add("block padding that is not zero", X.stream([ba, _bad_padding(CK)], CK), E_CORRUPT)
    add("an end byte in front of the block's end", blk(raw=bb.raw + b"\x00", prop=bb.prop), E_CORRUPT)
    lits = lambda s: [("lit", c) for c in s]
    W = L.Writer
    add("a distance one beyond the bytes produced", scripted_file(W().lzma(lits(b"abcd") + [("match", 5, 3)]))[0], E_CORRUPT)
    add("an end marker inside a chunk", scripted_file(W().lzma(lits(b"abcd") + [("eopm",), ("lit", 1)]))[0], E_CORRUPT)
    add("control byte 0x03", _one(b"\x03\x00\x00a\x00", b"a"), E_CORRUPT)
    add("a first chunk of 0x80", scripted_file(W().lzma(lits(b"abcd"), control=0x80))[0], E_CORRUPT)
    add("a first chunk of 0x02", scripted_file(W().stored(b"abcd", False))[0], E_CORRUPT)
    add("no properties behind a dictionary reset", scripted_file(W().stored(b"abcd", True).lzma(lits(b"efgh"), control=0xA0))[0], E_CORRUPT)
    add("lc + lp = 5", scripted_file(W().lzma(lits(b"abcd"), props=(2 * 5 + 2) * 9 + 3))[0], E_CORRUPT)
    add("a property byte of 225", scripted_file(W().lzma(lits(b"abcd"), props=225))[0], E_CORRUPT)
    ops = lits(b"abcdabcd") + [("match", 4, 30)]
    c = len(W().lzma(ops).raw) - 6
    add("a chunk one byte shorter than it says", scripted_file(W().lzma(ops, csize=c + 1))[0], E_CORRUPT)
    add("a chunk one byte longer than it says", scripted_file(W().lzma(ops, csize=c - 1))[0], E_CORRUPT)
    add("a chunk that says a byte more than it holds", scripted_file(W().lzma(ops, usize=39).stored(b"z", False))[0], E_CORRUPT)
    add("a match across the chunk's end", scripted_file(W().lzma(ops, usize=37).stored(b"z", False))[0], E_CORRUPT)
    add("a nonzero first byte of the range coder", _one(*_rc_first()), E_CORRUPT)
    return out, good, ta + tb


def _bad_padding(check):
    for k in range(8):   # (a content whose block needs padding)
        b = X.Block(gen.pseudo_text(900 + k, seed=9), check)
        n = -(len(b.header) + len(b.raw)) % 4
        if n:
            return X.Block(b.content, check, padding=bytes(n - 1) + b"\x01")
    raise AssertionError("no block with padding")


def _rc_first():
    raw, content = L.Writer().lzma([("lit", c) for c in b"abcdefgh"]).out()
    return raw[:6] + b"\x01" + raw[7:], content


@functools.lru_cache(None)
def mutant_base():
    """A file of about 300 bytes with two blocks, one with the sizes in its header, and its content"""
    a, b = gen.text(230), gen.pseudo_text(260, seed=11)
    f = X.stream([X.Block(a, X.CHECK_CRC32, header_sizes=True), X.Block(b, X.CHECK_CRC32)], X.CHECK_CRC32)
    return f, a + b


def mutants():
    f, _ = mutant_base()
    return [f[:i // 8] + bytes([f[i // 8] ^ (1 << (i % 8))]) + f[i // 8 + 1:] for i in range(8 * len(f))]


# ---- deterministic sweeps: every case a small block of its own ---------------------------------------------------------------------

MATCH_DISTANCES = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 272, 273, 274)
LITERAL_RUNS = (0, 1, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 191, 192, 193)
RUN_FOLLOWERS = ("a", "b", "c", "d", "e")


def match_lengths(dist):
    want = (2, 3, dist - 1, dist, dist + 1, 2 * dist - 1, 2 * dist, 2 * dist + 1, 258, 259, 272, 273)
    return sorted({min(max(n, 2), 273) for n in want})


def _blocks_file(writers, check=X.CHECK_CRC32, prop=PROP_1M):
    outs = [w.out() for w in writers]
    return X.stream([X.Block(content, check, raw=raw, prop=prop) for raw, content in outs], check), b"".join(c for _, c in outs)


def _match_byte(w):
    return w.hist[-w.reps[0] - 1]


def _geometry_ops(w, rnd, lead, dist, length, bit):
    """(a generator: the Writer draws one operation at a time, so w.hist holds the bytes produced so far)"""
    for _ in range(lead):
        yield ("lit", rnd.randrange(256))
    yield ("match", dist, length)
    yield ("lit", _match_byte(w))               # matched mode: the byte the match would go on with
    yield ("rep", 0, length)
    yield ("lit", _match_byte(w) ^ (1 << bit))  # matched mode: it leaves the match byte at `bit`
    yield ("rep", 0, length)
    yield ("shortrep",)
    yield ("lit", rnd.randrange(256))


@functools.lru_cache(None)
def match_geometry():
    """[(name, file, content, blocks)], once with lc = 3 and once with lc = 4 (lp = 0).  A block is random literals that cover the
    distance, the match, the literal the match would go on with, the same distance and length again as a rep0, a literal that differs
    from the match byte, the rep0 once more, a short rep and a literal behind it: four times the byte at rep0 and the last byte behind
    an overlapping or plain copy decide which probabilities the next symbol takes."""
    out = []
    for lc in (3, 4):
        rnd, writers = random.Random(lc), []
        for dist in MATCH_DISTANCES:
            for k, length in enumerate(match_lengths(dist)):
                w = L.Writer(lc=lc, lp=0, pb=2)
                writers.append(w.lzma(_geometry_ops(w, rnd, dist + k % 3, dist, length, (k + dist) % 8)))
        f, content = _blocks_file(writers)
        out.append((f"lc {lc}", f, content, len(writers)))
    return out


def _run_head(rnd, k):
    """three literals and a match, which stores them, then the k literals"""
    return [("lit", c) for c in b"xyz"] + [("match", 2, 3)] + [("lit", rnd.randrange(256)) for _ in range(k)]


def _matched_lit(w, flip):
    yield ("lit", _match_byte(w) ^ flip)
    yield ("shortrep",)
    yield ("lit", _match_byte(w))
    yield ("lit", 0x2E)


@functools.lru_cache(None)
def literal_runs():
    """(file, content, [(k, follower)]): k literals behind the last store of the 64-literal buffer, followed by
    a  a match of distance 1;
    b  a match of distance k, whose source are the literals themselves (k > 0);
    c  the chunk's end and a 0x80 chunk that opens with a match of distance k (1 for k = 0);
    d  the chunk's end, a 0x02 chunk and a 0x80 chunk that opens with a literal — in matched mode for k = 0, the only run that leaves
       the state at 7 or above —, a short rep and a literal that is in matched mode for every k;
    e  a match of distance k (1 for k = 0) and the chunk's end, a 0x02 chunk and a 0x80 chunk that opens with a matched-mode literal."""
    rnd, writers, cases = random.Random(64), [], []
    for k in LITERAL_RUNS:
        for how in RUN_FOLLOWERS:
            w, head, d = L.Writer(), _run_head(rnd, k), max(k, 1)
            if how == "a":
                w.lzma(head + [("match", 1, 5), ("lit", 0x41)])
            elif how == "b":
                if k == 0:
                    continue
                w.lzma(head + [("match", k, min(k + 2, 273)), ("lit", 0x42)])
            elif how == "c":
                w.lzma(head).lzma([("match", d, 4), ("lit", 0x43)], control=0x80)
            elif how == "d":
                w.lzma(head).stored(b"-0123-", False).lzma(_matched_lit(w, 0x10), control=0x80)
            else:
                w.lzma(head + [("match", d, 3)]).stored(b"-4567-", False).lzma(_matched_lit(w, 1 << k % 8), control=0x80)
            writers.append(w)
            cases.append((k, how))
    f, content = _blocks_file(writers)
    return f, content, cases


def window_offsets(block):
    """A model of the decoder's 256-byte input window (unxz.hip, XzIn): {offset in the block: offset in the window when that byte is
    read}.  The window is loaded at the block's start and again whenever a byte 256 or more past its base is asked for; the bytes of
    an uncompressed chunk are copied, not read, so a long one moves the base to the control byte behind it."""
    reads, at = [], len(block.header)
    for c, _, off, n in X.chunks_of(block.raw):
        reads += range(at + off, at + off + (3 if c in (1, 2) else n))
    end = at + len(block.raw)
    reads += range(end, end + len(block.padding) + min(8, len(block.check_bytes)))
    out, base = {}, 0
    for q in reads:
        if q - base >= 256:
            base = q
        out[q] = q - base
    return out


def _edge_block(n_lead, n_lits, check):
    """an uncompressed chunk of n_lead bytes (its last byte is fixed, so the LZMA chunk behind it does not depend on n_lead), then
    an LZMA chunk with properties: n_lits random literals and a match"""
    lead = random.Random(n_lead).randbytes(n_lead - 1) + b"\x55"
    rnd = random.Random(7)
    w = L.Writer().stored(lead, True).lzma([("lit", rnd.randrange(256)) for _ in range(n_lits)] + [("match", 3, 4)], control=0xC0)
    raw, content = w.out()
    return X.Block(content, check, raw=raw, prop=PROP_1M)


@functools.lru_cache(None)
def window_edges():
    """[(name, file, content, block, what, block offset of it, offset in the window it is meant to have)].  The control byte of an
    LZMA chunk at window offsets 245..260, so that the header, the property byte and the five bytes that start the range coder each
    lie across a reload; a chunk's last byte at 255, 0 and 1; the eight bytes of a CRC64 at 248..256 (248: the field, and with it
    the block, ends exactly where the window does — the last item)."""
    out = []

    def add(name, b, check, what, at, want):
        out.append((name, X.stream([b], check), b.content, b, what, at, want))

    for r in range(245, 261):
        b = _edge_block(r - 15, 20, X.CHECK_CRC32)       # 12 bytes of block header, 3 of the uncompressed chunk's
        add(f"control byte at {r}", b, X.CHECK_CRC32, "control", r, r if r < 256 else 0)   # (beyond 256 the uncompressed chunk moves the base there)
    for r in (255, 0, 1):
        size = len(_edge_block(1, 300, X.CHECK_CRC32).raw) - 1 - 4        # the LZMA chunk with its header
        n = (r - (15 + size - 1)) % 256 or 256
        assert n <= 240, n                                               # (no jump: the bases stay multiples of 256)
        b = _edge_block(n, 300, X.CHECK_CRC32)
        add(f"last byte of a chunk at {r}", b, X.CHECK_CRC32, "last", 15 + n + size - 1, r)
    for r in (256, 255, 254, 253, 252, 251, 250, 249, 248):
        for n_lits in range(190, 300):
            size = len(_edge_block(1, n_lits, X.CHECK_CRC64).raw) - 4
            fits = [n for n in range(256, 260) if (-(-(15 + n + size) // 4) * 4 - (15 + n)) % 256 == r % 256]
            if fits:
                break
        b = _edge_block(fits[0], n_lits, X.CHECK_CRC64)
        add(f"check field at {r}", b, X.CHECK_CRC64, "check", len(b.header) + len(b.raw) + len(b.padding), r % 256)
    return out


def stored_raw(data):
    """`data` as uncompressed LZMA2 chunks, the end byte included"""
    out = b""
    for at in range(0, len(data), 65536):
        part = data[at:at + 65536]
        out += bytes([2 if at else 1, (len(part) - 1) >> 8, (len(part) - 1) & 255]) + part
    return out + b"\x00"


CHECK_LENGTHS = tuple(range(521)) + (65535, 65536, 65537)
CHECK_DAMAGE_LENGTHS = (1, 255, 256, 257, 513)


@functools.lru_cache(None)
def check_lengths():
    """[(name, file, content)]: a block of uncompressed chunks for every content length of CHECK_LENGTHS, once under CRC32 and once
    under CRC64: the check kernel cuts a block into 256 segments, most of them empty below 256 bytes"""
    rnd, out = random.Random(256), []
    parts = [rnd.randbytes(n) for n in CHECK_LENGTHS]
    for check, name in ((X.CHECK_CRC32, "CRC32"), (X.CHECK_CRC64, "CRC64")):
        out.append((name, X.stream([X.Block(p, check, raw=stored_raw(p), prop=0) for p in parts], check), b"".join(parts)))
    return out


@functools.lru_cache(None)
def check_damage():
    """[(name, file, room)]: blocks of CHECK_DAMAGE_LENGTHS bytes whose check no longer fits: one content byte flipped at the first,
    the middle and the last position with the check field kept, and one bit flipped in each byte of the check field"""
    rnd, out = random.Random(257), []
    for check, name in ((X.CHECK_CRC32, "CRC32"), (X.CHECK_CRC64, "CRC64")):
        for n in CHECK_DAMAGE_LENGTHS:
            p = rnd.randbytes(n)
            field = X.check_field(check, p)
            for at in sorted({0, n // 2, n - 1}):
                q = p[:at] + bytes([p[at] ^ 0xFF]) + p[at + 1:]
                out.append((f"{name}, {n} bytes, content byte {at}", X.stream([X.Block(q, check, raw=stored_raw(q), prop=0, check_bytes=field)], check), n))
            for at in range(len(field)):
                bad = field[:at] + bytes([field[at] ^ (1 << (at + n) % 8)]) + field[at + 1:]
                out.append((f"{name}, {n} bytes, check byte {at}", X.stream([X.Block(p, check, raw=stored_raw(p), prop=0, check_bytes=bad)], check), n))
    return out


# ---- mutants of a file without a check: the verdict is the decoder's alone ----------------------------------------------------------

@functools.lru_cache(None)
def nocheck_base():
    """(file, content, offset of the LZMA2 bytes in the file, their count): every kind of operation, and a 0x02 chunk between two
    LZMA chunks"""
    lits = lambda s: [("lit", c) for c in s]
    w = L.Writer()
    w.lzma(lits(b"The quick brown fox ") + [("match", 4, 3), ("match", 11, 5), ("match", 2, 2), ("match", 17, 9)] + lits(b"jumps") +
           [("rep", 0, 4), ("shortrep",), ("lit", 0x6F), ("rep", 1, 3), ("rep", 2, 12), ("rep", 3, 2)] + lits(b" over"))
    w.stored(b"the lazy", False)
    w.lzma(lits(b" dog") + [("rep", 1, 5), ("shortrep",), ("match", 30, 20), ("lit", 0x2E), ("rep", 3, 6), ("rep", 2, 3), ("lit", 0x0A)], control=0x80)
    f, content = scripted_file(w, check=X.CHECK_NONE)
    raw = w.out()[0]
    return f, content, f.index(raw), len(raw)


def nocheck_mutants():
    f, _, at, n = nocheck_base()
    return [f[:i // 8] + bytes([f[i // 8] ^ (1 << (i % 8))]) + f[i // 8 + 1:] for i in range(8 * at, 8 * (at + n))]
