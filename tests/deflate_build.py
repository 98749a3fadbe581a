"""Builders of DEFLATE (RFC 1951) streams for the tests of every decoder path: a bit writer, the codes of the RFC, the hand-built
cases of tests/test_gpu_inflate.py, a randomised encoder that writes what zlib's compressor never writes, a sweep over every
length and distance symbol, and the corpus made of them.  Not a test file.  Python's zlib is the arbiter of every stream built here
(tests/test_deflate_build_cpu.py shows the corpus to it, and checks from the builders' own records that the shapes the corpus is
there for occur in it)."""
import functools
import heapq
import random
import struct
import zlib

import numpy as np

import gen

OK, E_DST_SMALL, E_CORRUPT = 0, -4, -5


# ---- the arbiter ---------------------------------------------------------------------------------------------------------------

def classify(data, n):
    """(expected status, expected bytes or None) of stream `data` with expected length n, from zlib's raw inflate"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(data), n + 1)
    except zlib.error:
        return E_CORRUPT, None
    if len(out) > n:
        return E_DST_SMALL, None
    if not d.eof or len(out) < n:
        return E_CORRUPT, None
    return OK, out


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


# ---- a bit writer and RFC 1951's codes -----------------------------------------------------------------------------------------

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
PLAIN_CL = [4] * 13 + [5] * 6          # a complete code over all 19 code-length symbols


class Bits:
    def __init__(self):
        self.b = []

    def put(self, v, n):                # a value, least significant bit first
        self.b += [(v >> i) & 1 for i in range(n)]

    def code(self, c):                  # a Huffman code (value, length), most significant bit first
        v, n = c
        self.b += [(v >> i) & 1 for i in reversed(range(n))]

    def align(self):
        self.b += [0] * (-len(self.b) % 8)

    def raw(self, data):
        assert len(self.b) % 8 == 0
        for x in data:
            self.put(x, 8)

    def bytes(self):
        return np.packbits(np.array(self.b, np.uint8), bitorder="little").tobytes()


def canon(lens):
    """symbol -> (code, length) of the canonical code with these lengths (complete or not)"""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def put_ops(bw, ops, ll, dd, eob=True):
    """ops: ints (literals), ('m', length, distance), ('ll', symbol) a bare literal/length symbol, ('sym', symbol, extra value,
    distance symbol, extra value) a match given by its symbols"""
    for op in ops:
        if isinstance(op, int):
            bw.code(ll[op])
        elif op[0] == "ll":
            bw.code(ll[op[1]])
        elif op[0] == "sym":
            _, ls, lx, ds, dx = op
            bw.code(ll[ls]); bw.put(lx, LEXT[ls - 257] if ls <= 285 else 0)
            bw.code(dd[ds]); bw.put(dx, DEXT[ds] if ds < 30 else 0)
        else:
            _, length, dist = op
            i = max(k for k in range(29) if LBASE[k] <= length and (k == 28 or length < 258))
            bw.code(ll[257 + i]); bw.put(length - LBASE[i], LEXT[i])
            j = max(k for k in range(30) if DBASE[k] <= dist)
            bw.code(dd[j]); bw.put(dist - DBASE[j], DEXT[j])
    if eob:
        bw.code(ll[256])


def fixed_block(bw, ops, final=1, eob=True):
    bw.put(final, 1); bw.put(1, 2)
    put_ops(bw, ops, canon(FIXED_LL), canon(FIXED_D), eob)


def stored_block(bw, data, final=1, nlen=None):
    bw.put(final, 1); bw.put(0, 2); bw.align()
    bw.put(len(data), 16); bw.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    bw.raw(data)


def dynamic_block(bw, ll_lens, d_lens, ops, final=1, cl_lens=None, cl_syms=None, hlit=None, hdist=None, body=True, eob=True):
    """cl_syms: the code-length symbols as (symbol, extra value) pairs; None: every length as a symbol of its own"""
    cl_lens = PLAIN_CL if cl_lens is None else cl_lens
    if cl_syms is None:
        cl_syms = [(n, 0) for n in list(ll_lens) + list(d_lens)]
    bw.put(final, 1); bw.put(2, 2)
    bw.put((len(ll_lens) if hlit is None else hlit) - 257, 5)
    bw.put((len(d_lens) if hdist is None else hdist) - 1, 5)
    bw.put(19 - 4, 4)
    for s in CL_ORDER:
        bw.put(cl_lens[s], 3)
    cc = canon(cl_lens)
    for s, x in cl_syms:
        bw.code(cc[s])
        bw.put(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
    if body:
        put_ops(bw, ops, canon(ll_lens), canon(d_lens), eob)


def ll_lens_for(pairs, n=257):
    lens = [0] * n
    for s, k in pairs:
        lens[s] = k
    return lens


TEXT = gen.pseudo_text(300_000, seed=7)


# ---- cases ---------------------------------------------------------------------------------------------------------------------

def block_kind_cases():
    rnd = np.random.default_rng(11).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    cases = [("empty", bytes([3, 0]), 0), ("one byte", deflate(b"Z"), 1),
             ("stored 70000", deflate((rnd * 3)[:70000], 0), 70000),
             ("fixed text", deflate(TEXT[:5000], 6, zlib.Z_FIXED), 5000),
             ("level 9 text", deflate(TEXT, 9), len(TEXT)),
             ("rle zeros", deflate(bytes(300_000), 6, zlib.Z_RLE), 300_000),
             ("huffman only", deflate(TEXT[:20000], 6, zlib.Z_HUFFMAN_ONLY), 20000)]
    bw = Bits()
    stored_block(bw, b"", final=0)
    fixed_block(bw, list(b"behind an empty stored block"))
    cases.append(("empty stored block first", bw.bytes(), 28))
    for dist in (1, 2, 3, 63, 64, 65, 257, 258, 259, 32768):
        bw = Bits()
        head = rnd if dist == 32768 else rnd[:dist]
        if dist == 32768:
            stored_block(bw, head, final=0)
            fixed_block(bw, [("m", 258, dist)])
        else:
            fixed_block(bw, list(head) + [("m", 258, dist)])
        cases.append((f"match 258 at distance {dist}", bw.bytes(), len(head) + 258))
    return cases


def table_corner_cases():
    cases = []
    # literal/length codes of 15 bits, and a lone distance code of length 1
    ll = ll_lens_for([(97 + k, k + 1) for k in range(13)] + [(257, 14), (110, 15), (256, 15)], 258)
    bw = Bits()
    dynamic_block(bw, ll, [1], list(b"abcdefghijklmnnmlkjihgfedcba") + [("m", 3, 1)] * 3 + [110])
    cases.append(("15-bit codes, lone distance code", bw.bytes(), 28 + 9 + 1))
    # HLIT 286 with HDIST 30
    bw = Bits()
    dynamic_block(bw, [8] * 226 + [9] * 60, [4] * 2 + [5] * 28, list(b"all 286 and all 30") + [("m", 258, 18), ("m", 100, 3), 255, 0])
    cases.append(("HLIT 286, HDIST 30", bw.bytes(), 18 + 258 + 100 + 2))
    # a code-16 repeat that crosses from the literal/length lengths into the distance lengths: 120 zeros, 1, 2, 134 zeros, a 4 for
    # symbol 256, then "repeat it" 6 times — symbols 257, 258, 259 and the first three distance codes — and 13 more distance codes
    ll = ll_lens_for([(120, 1), (121, 2), (256, 4), (257, 4), (258, 4), (259, 4)], 260)
    syms = [(18, 120 - 11), (1, 0), (2, 0), (18, 134 - 11), (4, 0), (16, 6 - 3), (16, 6 - 3), (16, 6 - 3), (4, 0)]
    bw = Bits()
    dynamic_block(bw, ll, [4] * 16, [120, 121, 120, 120, ("m", 5, 4), ("m", 3, 7)], cl_syms=syms)
    cases.append(("repeat across the two sets", bw.bytes(), 4 + 5 + 3))
    # a dynamic block holding only end-of-block (its one code has one bit, and there is no distance code), then a fixed block
    bw = Bits()
    dynamic_block(bw, ll_lens_for([(256, 1)]), [0], [], final=0, cl_syms=[(18, 127), (18, 118 - 11), (1, 0), (0, 0)])
    fixed_block(bw, list(b"after nothing"))
    cases.append(("dynamic block of end-of-block only", bw.bytes(), 13))
    # a stored block begun at bit 3 of a byte
    bw = Bits()
    fixed_block(bw, [200], final=0)
    assert len(bw.b) % 8 == 3
    stored_block(bw, b"stored from bit 3")
    cases.append(("stored block at bit 3", bw.bytes(), 1 + 17))
    return cases


def rejection_cases():
    """(what, stream, n): every one must classify as ZNIPPY_E_CORRUPT"""
    out = []

    def add(what, bw, n=10):
        out.append((what, bw.bytes() + bytes(8), n))   # (zeros behind it: the error is the stream's, not a short input's)
    bw = Bits(); bw.put(1, 1); bw.put(3, 2); add("block type 3", bw)
    bw = Bits(); stored_block(bw, b"0123456789", nlen=10); add("LEN is not the complement of NLEN", bw)
    ok_ll = ll_lens_for([(65, 1), (256, 1)])
    for hlit in (287, 288):
        bw = Bits(); dynamic_block(bw, [8] * 224 + [9] * 64, [1, 1], [], hlit=hlit, body=False); add(f"HLIT {hlit}", bw)
    for hdist in (31, 32):
        bw = Bits(); dynamic_block(bw, ok_ll, [1, 1], [], hdist=hdist, body=False); add(f"HDIST {hdist}", bw)
    bw = Bits(); dynamic_block(bw, ok_ll, [1, 1], [], cl_syms=[(16, 0)], body=False); add("code 16 with no previous length", bw)
    bw = Bits(); dynamic_block(bw, ok_ll, [1, 1], [], cl_syms=[(18, 127), (18, 127)], body=False); add("repeat past HLIT + HDIST", bw)
    bw = Bits(); dynamic_block(bw, ok_ll, [1, 1], [], cl_syms=[(18, 127), (18, 107), (1, 0), (1, 0), (17, 0)], body=False); add("zeros past HLIT + HDIST", bw)
    bw = Bits(); dynamic_block(bw, ok_ll, [1, 1], [], cl_lens=[1, 1, 1] + [0] * 16, cl_syms=[], body=False); add("over-subscribed code-length set", bw)
    bw = Bits(); dynamic_block(bw, ok_ll, [1, 1], [], cl_lens=[2, 2, 2] + [0] * 16, cl_syms=[], body=False); add("incomplete code-length set", bw)
    bw = Bits(); dynamic_block(bw, ok_ll, [1, 1], [], cl_lens=[0] * 18 + [1], cl_syms=[], body=False); add("code-length set of one 1-bit code", bw)
    bw = Bits(); dynamic_block(bw, ll_lens_for([(65, 1), (66, 1), (256, 1)]), [1, 1], [], body=False); add("over-subscribed literal/length set", bw)
    bw = Bits(); dynamic_block(bw, ok_ll, [1, 1, 1], [], body=False); add("over-subscribed distance set", bw)
    bw = Bits(); dynamic_block(bw, ll_lens_for([(65, 2), (66, 2), (256, 2)]), [1, 1], [], body=False); add("incomplete literal/length set", bw)
    bw = Bits(); dynamic_block(bw, ok_ll, [2, 2, 2], [], body=False); add("incomplete distance set", bw)
    bw = Bits(); dynamic_block(bw, ll_lens_for([(65, 1), (66, 1)]), [1, 1], [], body=False); add("no end-of-block code", bw)
    # a lone 1-bit literal/length code is allowed; the bit pattern it leaves unused is not
    bw = Bits(); dynamic_block(bw, ll_lens_for([(256, 1)]), [0], [], body=False); bw.put(1, 1); add("unused code of an incomplete set", bw, 0)
    # ... nor is any distance code where the block has none, or the unused one of a lone distance code
    bw = Bits(); dynamic_block(bw, ll_lens_for([(65, 2), (256, 2), (257, 1)], 258), [0], [65, 65, 65, ("ll", 257)], eob=False); bw.put(0, 4); add("a match in a block without distance codes", bw)
    bw = Bits(); dynamic_block(bw, ll_lens_for([(65, 2), (256, 2), (257, 1)], 258), [1], [65, 65, 65, ("ll", 257)], eob=False); bw.put(1, 4); add("unused code of a lone distance code", bw)
    for s in (286, 287):
        bw = Bits(); fixed_block(bw, [65, 66, ("ll", s)]); add(f"literal/length symbol {s}", bw)
    for s in (30, 31):
        bw = Bits(); fixed_block(bw, [65, 66, 67, ("sym", 257, 0, s, 0)]); add(f"distance symbol {s}", bw)
    bw = Bits(); fixed_block(bw, [65, 66, 67, ("m", 3, 4)]); add("distance beyond the bytes produced", bw)
    bw = Bits(); fixed_block(bw, [("m", 3, 1)]); add("a match as the first symbol", bw)
    bw = Bits(); fixed_block(bw, list(b"0123456789"), final=0); out.append(("no final block", bw.bytes(), 10))
    bw = Bits(); fixed_block(bw, list(b"01234")); add("end-of-block short of the expected length", bw)
    return out


def truncation_cases():
    fixed = deflate(TEXT[:150], 6, zlib.Z_FIXED)
    i = 150
    while len(fixed) != 91:        # grow or shrink the input until the stream has the length the case names
        i += 1 if len(fixed) < 91 else -1
        fixed = deflate(TEXT[:i], 6, zlib.Z_FIXED)
        assert 20 < i < 1000
    nf = i
    j = 400
    dyn = deflate(TEXT[1000:1000 + j], 9)
    seen = set()
    while len(dyn) != 260:
        assert j not in seen, "no input of this text deflates to 260 bytes"
        seen.add(j)
        j += 1 if len(dyn) < 260 else -1
        dyn = deflate(TEXT[1000:1000 + j], 9)
    assert dyn[0] & 6 == 4 and fixed[0] & 6 == 2
    return [(f"fixed[:{k}]", fixed[:k], nf) for k in range(len(fixed))] + [(f"dynamic[:{k}]", dyn[:k], j) for k in range(len(dyn))], (fixed, nf), (dyn, j)


def flushed_stream(data, piece, kinds, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """`data` deflated with a flush of kinds[k % len] behind every `piece` bytes: each flush writes an empty stored block"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out = []
    for k, at in enumerate(range(0, len(data), piece)):
        out.append(c.compress(data[at:at + piece]))
        out.append(c.flush(kinds[k % len(kinds)]))
    return b"".join(out) + c.flush()


def gz_member(stream, content):
    """the raw stream as a gzip member: a plain ten-byte header in front, CRC-32 and ISIZE of the content behind"""
    return b"\x1f\x8b\x08\x00" + bytes(4) + b"\x00\xff" + bytes(stream) + struct.pack("<II", zlib.crc32(content), len(content) & 0xFFFFFFFF)


# ---- Huffman code lengths ------------------------------------------------------------------------------------------------------

def huffman_lengths(weights, limit=15):
    """Code lengths of a Huffman code for weights[s] > 0 (0: the symbol has no code), none longer than `limit`: the plain heap
    construction, tried again with flatter weights while the longest code is too long.  Complete by construction; one used symbol
    gets one 1-bit code (the incomplete set RFC 1951 allows)."""
    used = [s for s, w in enumerate(weights) if w > 0]
    lens = [0] * len(weights)
    if len(used) == 1:
        lens[used[0]] = 1
    if len(used) < 2:
        return lens
    w = {s: float(weights[s]) for s in used}
    while True:
        heap = [(w[s], s, (s,)) for s in used]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(depth.values()) <= limit:
            break
        top = max(w.values())
        w = {s: (x / top) ** 0.85 for s, x in w.items()}
    for s in used:
        lens[s] = depth[s]
    return lens


# ---- a randomised encoder ------------------------------------------------------------------------------------------------------

BLOCK_SIZES = (0, 1, 7, 64, 300, 1500, 5000)
STORED, FIXED, DYNAMIC = 0, 1, 2


class Record:
    """what a builder used: blocks = (kind, bit phase of the block header); len_short[i] / len_long[i]: how often length symbol
    257 + i was written through a code of at most 10 bits / a longer one; dist_short / dist_long: the same for distance symbol i and
    9 bits; the stored lengths; flushes = empty non-final stored blocks; dynamic blocks without a distance code and with a lone one;
    code-length runs (16, 17, 18) that cross from the literal/length lengths into the distance lengths; length 258 written as
    symbol 284 with extra value 31."""

    def __init__(self):
        self.blocks, self.stored = [], []
        self.len_short, self.len_long = [0] * 29, [0] * 29
        self.dist_short, self.dist_long = [0] * 30, [0] * 30
        self.flushes = self.no_dist = self.lone_dist = self.cross = self.l284_31 = 0

    def add(self, other):
        self.blocks += other.blocks
        self.stored += other.stored
        for name in ("len_short", "len_long", "dist_short", "dist_long"):
            setattr(self, name, [a + b for a, b in zip(getattr(self, name), getattr(other, name))])
        for name in ("flushes", "no_dist", "lone_dist", "cross", "l284_31"):
            setattr(self, name, getattr(self, name) + getattr(other, name))

    def count_ops(self, ops, ll_lens, d_lens):
        for op in ops:
            if not isinstance(op, int):
                _, ls, lx, ds, dx = op
                (self.len_short if ll_lens[ls] <= 10 else self.len_long)[ls - 257] += 1
                (self.dist_short if d_lens[ds] <= 9 else self.dist_long)[ds] += 1
                self.l284_31 += (ls, lx) == (284, 31)


def match_op(rng, length, dist):
    """('sym', ...) of a match; length 258 is symbol 285 or, as zlib's compressor never writes it, symbol 284 with extra value 31"""
    if length == 258 and rng.random() < 0.5:
        i = 27
    else:
        i = max(k for k in range(29) if LBASE[k] <= length and (k == 28 or length < 258))
    j = max(k for k in range(30) if DBASE[k] <= dist)
    return ("sym", 257 + i, length - LBASE[i], j, dist - DBASE[j])


def _common(c, p, d, most):
    x, y = c[p - d:p - d + most], c[p:p + most]
    if x == y:
        return most
    k = 0
    while x[k] == y[k]:
        k += 1
    return k


def random_parse(content, a, b, rng, match_p=0.5):
    """content[a:b] as literals and matches: at a position, with probability match_p, a few random distances are tried (half of
    them up to 32,768, half up to 300), the longest common run (overlap allowed, at most 258, inside the block) is taken, and a run
    of at least 3 becomes a match of a random length in [3, run]"""
    ops, p = [], a
    while p < b:
        run, dist = 0, 0
        if p and b - p >= 3 and rng.random() < match_p:
            for _ in range(3):
                d = rng.randint(1, min(p, 32768 if rng.random() < 0.5 else 300))
                r = _common(content, p, d, min(258, b - p))
                if r > run:
                    run, dist = r, d
        if run >= 3:
            length = rng.randint(3, run)
            ops.append(match_op(rng, length, dist))
            p += length
        else:
            ops.append(content[p])
            p += 1
    return ops


def code_length_symbols(seq, hlit, rng, rec):
    """the code-length sequence as (symbol, extra value) pairs, with 16 / 17 / 18 runs chosen at random; a run may cross hlit"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        r = 1
        while i + r < n and seq[i + r] == v:
            r += 1
        rep = 0
        if v == 0 and r >= 3 and rng.random() < 0.8:
            if r >= 11 and rng.random() < 0.7:
                rep = rng.randint(11, min(r, 138))
                out.append((18, rep - 11))
            else:
                rep = rng.randint(3, min(r, 10))
                out.append((17, rep - 3))
        elif v and i and seq[i - 1] == v and r >= 3 and rng.random() < 0.8:
            rep = rng.randint(3, min(r, 6))
            out.append((16, rep - 3))
        if rep:
            rec.cross += i < hlit < i + rep
            i += rep
        else:
            out.append((v, 0))
            i += 1
    return out


def write_dynamic(bw, ops, final, rng, rec, ll_lens=None, d_lens=None):
    """a dynamic block of ops.  Codes not given come from huffman_lengths over the symbols used, every weight scaled by a random
    power of 3 between 3^0 and 3^-13 so that used symbols land on long codes, and a few unused symbols with a small weight, whose
    codes nobody uses.  HLIT and HDIST are trimmed to the last code or left at 286 / 30."""
    if ll_lens is None:
        lw, dw = [0.0] * 286, [0.0] * 30
        lw[256] = 1.0
        for op in ops:
            if isinstance(op, int):
                lw[op] += 1
            else:
                lw[op[1]] += 1
                dw[op[3]] += 1

        def scaled(w, extra):
            w = [x * 3.0 ** -rng.randint(0, 13) for x in w]
            low = min(x for x in w if x > 0) if any(w) else 1.0
            for _ in range(extra):
                s = rng.randrange(len(w))
                if w[s] == 0:
                    w[s] = low / 8
            return w
        ll_lens = huffman_lengths(scaled(lw, rng.randint(0, 4)))
        used_d = sum(1 for x in dw if x)
        # no match: no distance code at all, a lone one, or several that nobody uses; one distance symbol: a lone code, or more
        d_lens = huffman_lengths(scaled(dw, rng.choice((0, 0, 1, 3)) if used_d < 2 else rng.randint(0, 3)))
    n_d = sum(1 for x in d_lens if x)
    rec.no_dist += n_d == 0
    rec.lone_dist += n_d == 1
    hlit = 286 if rng.random() < 0.3 else max(257, max(s for s, n in enumerate(ll_lens) if n) + 1)
    hdist = 30 if rng.random() < 0.3 else max([1] + [s + 1 for s, n in enumerate(d_lens) if n])
    ll_lens = (list(ll_lens) + [0] * 286)[:hlit]
    d_lens = (list(d_lens) + [0] * 30)[:hdist]
    cl_syms = code_length_symbols(ll_lens + d_lens, hlit, rng, rec)
    cw = [0.0] * 19
    for s, _ in cl_syms:
        cw[s] += 1
    while sum(1 for x in cw if x) < 2:             # the code-length code has to be complete: two codes at least
        cw[rng.randrange(19)] += 0.1
    rec.blocks.append((DYNAMIC, len(bw.b) % 8))
    rec.count_ops(ops, ll_lens, d_lens)
    dynamic_block(bw, ll_lens, d_lens, ops, final=final, cl_lens=huffman_lengths(cw, 7), cl_syms=cl_syms)


def write_block(bw, kind, content, a, b, final, rng, rec, match_p=0.5):
    if kind == STORED:
        rec.blocks.append((STORED, len(bw.b) % 8))
        rec.stored.append(b - a)
        rec.flushes += a == b and not final
        stored_block(bw, content[a:b], final=final)
        return
    ops = random_parse(content, a, b, rng, match_p)
    if kind == FIXED:
        rec.blocks.append((FIXED, len(bw.b) % 8))
        rec.count_ops(ops, FIXED_LL, FIXED_D)
        fixed_block(bw, ops, final=final)
    else:
        write_dynamic(bw, ops, final, rng, rec)


def encode(content, rng, flush_p=0.25, match_p=0.5, kinds=(STORED, FIXED, DYNAMIC)):
    """`content` as a DEFLATE stream of random blocks (rng: random.Random): sizes from BLOCK_SIZES, kinds from `kinds`, with
    probability flush_p an empty non-final stored block — a flush point — between two blocks, a random parse, random codes; the
    last block of content is final, or a last empty block of a random kind is.  Returns (stream, Record)."""
    bw, rec = Bits(), Record()
    cuts, at = [], 0
    while True:
        end = min(len(content), at + rng.choice(BLOCK_SIZES))
        cuts.append((at, end))
        at = end
        if at == len(content):
            break
    tail = rng.random() < 0.5
    for k, (a, b) in enumerate(cuts):
        if k and rng.random() < flush_p:
            write_block(bw, STORED, content, a, a, 0, rng, rec)
        write_block(bw, rng.choice(kinds), content, a, b, int(k + 1 == len(cuts) and not tail), rng, rec, match_p)
    if tail:
        write_block(bw, rng.choice((STORED, FIXED, DYNAMIC)), content, len(content), len(content), 1, rng, rec)
    return bw.bytes(), rec


# ---- every length and distance symbol ------------------------------------------------------------------------------------------

SWEEP_SEEDS = tuple(range(8))
DEEP_DISTANCE = [k + 1 for k in range(15)] + [15]      # a distance code of lengths 1, 2, ..., 14, 15, 15


def apply_ops(out, ops):
    """the bytes that literals and ('sym', ...) matches add to bytearray `out`"""
    for op in ops:
        if isinstance(op, int):
            out.append(op)
        else:
            _, ls, lx, ds, dx = op
            length, dist = LBASE[ls - 257] + lx, DBASE[ds] + dx
            assert dist <= len(out)
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                out += (bytes(out[-dist:]) * (length // dist + 1))[:length]
    return out


def geometric_lengths(used, n, seed, ratio):
    """code lengths over n symbols for the used ones: weights ratio^-rank, the ranks a permutation that seed // 4 draws and seed % 4
    turns by a quarter, so that over four seeds in a row every symbol is once among the heaviest and once among the lightest"""
    perm = list(range(len(used)))
    random.Random(1000 + seed // 4).shuffle(perm)
    w = [0.0] * n
    for s, r in zip(used, perm):
        w[s] = ratio ** -((r + (seed % 4) * len(used) // 4) % len(used))
    return huffman_lengths(w)


def symbol_sweep(seed, deep_distance=False):
    """One dynamic block: 300 random literals; every length symbol 257 - 285 with extra value 0 and with its maximum; every distance
    symbol 0 - 29 with extra value 0 and with its maximum (matches of 258 fill up until the bytes produced allow the distance).  The
    codes are geometric_lengths of the seed; deep_distance: the hand-set distance code DEEP_DISTANCE over symbols 0 - 15 instead.
    Returns (stream, content, Record)."""
    rng = random.Random(seed)
    ops = [rng.randrange(256) for _ in range(300)]
    out = apply_ops(bytearray(), ops)
    n_dist = 16 if deep_distance else 30

    def add(op):
        ops.append(op)
        apply_ops(out, [op])
    for i in range(29):
        for lx in sorted({0, (1 << LEXT[i]) - 1}):
            ds = rng.randrange(min(n_dist, 16))                 # (distances up to 255 + 127: inside the 300 literals)
            add(("sym", 257 + i, lx, ds, rng.randrange(1 << DEXT[ds])))
    for ds in range(n_dist):
        for dx in sorted({0, (1 << DEXT[ds]) - 1}):
            while len(out) < DBASE[ds] + dx:
                add(("sym", 285, 0, rng.randrange(4), 0))
            add(("sym", 257 + rng.randrange(8), 0, ds, dx))
    ll_used = sorted({op for op in ops if isinstance(op, int)} | {256} | set(range(257, 286)))
    ll_lens = geometric_lengths(ll_used, 286, seed, 1.028)
    d_lens = DEEP_DISTANCE if deep_distance else geometric_lengths(list(range(30)), 30, seed, 1.45)
    bw, rec = Bits(), Record()
    write_dynamic(bw, ops, 1, rng, rec, ll_lens, d_lens)
    return bw.bytes(), bytes(out), rec


# ---- the corpus ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def corpus():
    """[(what, stream, content, Record)], built once per process"""
    out = []
    for seed in SWEEP_SEEDS:
        out.append((f"sweep {seed}",) + symbol_sweep(seed))
    out.append(("sweep, 15-bit distance codes",) + symbol_sweep(3, deep_distance=True))
    rng = random.Random(1951)
    noise = gen.incompressible(17, 4000)
    for k in range(150):
        n = rng.choice((0, 1, 2, 50, 300, 1000, 2500, 4000)) if k % 10 else 0
        n += rng.randrange(1 + n // 3)
        what = k % 5
        if what < 2:
            at = rng.randrange(len(TEXT) - n)
            content = TEXT[at:at + n]
        elif what < 4:
            half = noise[rng.randrange(1000):][:n // 2]
            content = half + half + noise[:n & 1]              # the second half lies at distance n / 2 behind the first
        else:
            content = bytes(n)
        s, rec = encode(content, rng)
        out.append((f"encode {k} ({('text', 'text', 'halves', 'halves', 'zeros')[what]}, {len(content)})", s, content, rec))
    # sources of more than three input windows, nearly all literals
    for k in range(4):
        content = gen.incompressible(30 + k, 6500 + 300 * k)
        s, rec = encode(content, rng, flush_p=(0.0, 0.3)[k & 1], match_p=0.02, kinds=(FIXED, DYNAMIC))
        assert len(s) > 3 * 2048
        out.append((f"long source {k}", s, content, rec))
    return out


def corpus_record():
    total = Record()
    for _, _, _, rec in corpus():
        total.add(rec)
    return total
