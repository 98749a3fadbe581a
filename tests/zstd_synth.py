"""A hand-driven writer of RFC 8878 (Zstandard) frames and a plain reference executor (not a test module: pytest does not
collect it).  Pure Python + numpy, no GPU, no oracle.

A frame is described as a list of blocks:

    Raw(data)                       a Raw_Block
    Rle(byte, n)                    an RLE_Block of n bytes
    Comp(lits, seqs, **choices)     a Compressed_Block: the literal bytes and a list of
                                    (literal_length, match_length, offset_value) -- offset_value is the RFC's
                                    Offset_Value: 1, 2, 3 are the repeat codes, above that it is the distance + 3

`execute(blocks)` turns the description into the decoded bytes with the repeat-offset rules of section 3.1.1.5 written
out in the plainest form; it raises SynthError on a distance of zero or one that reaches before the frame's first byte.
`write_frame(blocks, **choices)` turns the same description into frame bytes; everything the format leaves to an encoder
(header forms, literal formats, table modes, normalised counts, accuracy logs) is an explicit choice.  The named corpus
built from the two is tests/zstd_synth_cases.py."""
import heapq

import numpy as np

BLOCK_MAX = 128 * 1024
MAGIC = b"\x28\xb5\x2f\xfd"

LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512,
           1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387,
                                32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEFAULT = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_DEFAULT = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_DEFAULT = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
DEFAULTS = {"ll": (LL_DEFAULT, 6), "of": (OF_DEFAULT, 5), "ml": (ML_DEFAULT, 6)}
MAX_LOG = {"ll": 9, "of": 8, "ml": 9}
MAX_SYM = {"ll": 35, "of": 31, "ml": 52}


class SynthError(ValueError):
    """The description is not a valid frame (the executor), or a choice cannot be written (the writer)."""


# ---- description ------------------------------------------------------------------------------------------------------

class Raw:
    def __init__(self, data):
        self.data = bytes(data)


class Rle:
    def __init__(self, byte, n):
        self.byte, self.n = byte, n


class Comp:
    """lits: the block's literal bytes; seqs: [(ll, ml, offset_value)].  Choices (None = the plain default):
    lit = dict(type="raw"|"rle"|"huf"|"treeless", fmt=size format 0..3, weights=[...], wdesc="direct"|"fse",
               check=True, lie_regen=None)
    nseq_form = 1 | 2 | 3 (bytes of the sequence count)
    ll / of / ml = "pre" | "rle" | ("fse", normalised counts, accuracy log) | "rep" ("rep-of-nothing": Repeat_Mode
    written although no table came before, an invalid frame)
    modes_reserved = the two reserved bits of Compression_Modes; pad_bits = extra zero bits under the sequence
    bitstream; drop_bits = bits cut off its end (both make the stream invalid)."""

    def __init__(self, lits, seqs, lit=None, nseq_form=None, ll=None, of=None, ml=None, modes_reserved=0, pad_bits=0,
                 drop_bits=0):
        self.lits, self.seqs = bytes(lits), list(seqs)
        self.lit = dict(lit or {})
        self.nseq_form, self.ll, self.of, self.ml = nseq_form, ll, of, ml
        self.modes_reserved, self.pad_bits, self.drop_bits = modes_reserved, pad_bits, drop_bits


# ---- the reference executor -------------------------------------------------------------------------------------------

def execute(blocks):
    """Decoded bytes of the description.  Raises SynthError on a distance of zero or beyond the bytes written so far,
    on literal lengths that sum beyond the literals, and on a block that regenerates more than 128 KiB."""
    out = bytearray()
    rep = [1, 4, 8]
    for b in blocks:
        start = len(out)
        if isinstance(b, Raw):
            out += b.data
        elif isinstance(b, Rle):
            out += bytes([b.byte]) * b.n
        else:
            at = 0
            for ll, ml, ov in b.seqs:
                if at + ll > len(b.lits):
                    raise SynthError("literal lengths sum beyond the literals")
                out += b.lits[at:at + ll]
                at += ll
                if ov > 3:
                    dist = ov - 3
                    rep = [dist, rep[0], rep[1]]
                else:
                    k = ov - 1 + (1 if ll == 0 else 0)      # which entry of the history
                    if k == 0:
                        dist = rep[0]
                    elif k == 1:
                        dist = rep[1]
                        rep = [dist, rep[0], rep[2]]
                    elif k == 2:
                        dist = rep[2]
                        rep = [dist, rep[0], rep[1]]
                    else:
                        dist = rep[0] - 1
                        rep = [dist, rep[0], rep[1]]
                if dist == 0:
                    raise SynthError("a distance of zero")
                if dist > len(out):
                    raise SynthError("a distance beyond the start of the frame")
                if dist >= ml:
                    out += out[len(out) - dist:len(out) - dist + ml]
                else:                                       # the copy reads what it is writing: the period repeats
                    pat = bytes(out[len(out) - dist:])
                    out += (pat * (ml // dist + 1))[:ml]
            out += b.lits[at:]
        if len(out) - start > BLOCK_MAX:
            raise SynthError("a block regenerating more than 128 KiB")
    return bytes(out)


def blocks_of_trace(frame_trace, content):
    """The description (Raw / Rle / Comp with their literals and sequences) of one frame of oracle.zstd_trace's result:
    what `execute` needs to say the frame's bytes again.  content: the trace's decoded bytes (raw and RLE blocks are read
    from it)."""
    out = []
    for b in frame_trace["blocks"]:
        if b["type"] == 0:
            out.append(Raw(content[b["at"]:b["at"] + b["size"]]))
        elif b["type"] == 1:
            out.append(Rle(content[b["at"]], b["size"]))
        else:
            out.append(Comp(b["lits"]["bytes"], [(int(s[0]), int(s[1]), int(s[2])) for s in b["seqs"]]))
    return out


# ---- bit streams ------------------------------------------------------------------------------------------------------

class _Bits:
    """Little-endian bit accumulator: the first field added sits in the lowest bits."""

    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def add(self, v, nbits):
        assert 0 <= v < (1 << nbits) or (nbits == 0 and v == 0), (v, nbits)
        self.acc |= v << self.n
        self.n += nbits
        if self.n >= 512:
            k = self.n // 8
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def bytes(self):
        return bytes(self.buf) + self.acc.to_bytes((self.n + 7) // 8, "little")


def backward_stream(fields, pad_bits=0, drop_bits=0):
    """fields: [(value, nbits)] in the order a decoder READS them (from the end of the stream, most significant bit
    first).  The last field read sits in the lowest bits; a single 1 bit above the first field marks the end."""
    w = _Bits()
    if pad_bits:
        w.add(0, pad_bits)
    drop = drop_bits
    for v, n in reversed(fields):
        if drop >= n:
            drop -= n
            continue
        if drop:
            v, n, drop = v >> drop, n - drop, 0
        w.add(v, n)
    w.add(1, 1)
    return w.bytes()


# ---- FSE --------------------------------------------------------------------------------------------------------------

def _highbit(v):
    return v.bit_length() - 1


def write_ncount(norm, log):
    """The FSE table description (section 4.1.1) of normalised counts (-1 = "less than 1") at an accuracy log."""
    w = _Bits()
    w.add(log - 5, 4)
    remaining = 1 << log
    s = 0
    while remaining > 0 and s < len(norm):
        p = norm[s]
        s += 1
        v = p + 1
        bits = _highbit(remaining + 1) + 1
        threshold = (1 << bits) - 1 - (remaining + 1)
        if v < threshold:
            w.add(v, bits - 1)
        elif v < (1 << (bits - 1)):
            w.add(v, bits)
        else:
            w.add(v + threshold, bits)
        remaining -= abs(p)
        if p == 0:
            z = 0
            while s + z < len(norm) and norm[s + z] == 0:
                z += 1
            s += z
            while z >= 3:
                w.add(3, 2)
                z -= 3
            w.add(z, 2)
    return w.bytes()


class FseTable:
    """The decoding table a decoder builds from normalised counts, and the inverse a writer needs."""

    def __init__(self, norm, log, check=True):
        size = 1 << log
        if check and sum(abs(x) for x in norm) != size:
            raise SynthError("counts do not sum to the table size")
        self.log, self.size, self.norm = log, size, list(norm)
        sym = [0] * size
        high = size
        nxt = {}
        for s, p in enumerate(norm):
            if p == -1:
                high -= 1
                sym[high] = s
                nxt[s] = 1
        self.low_cells = size - high
        step, mask, pos = (size >> 1) + (size >> 3) + 3, size - 1, 0
        for s, p in enumerate(norm):
            if p <= 0:
                continue
            nxt[s] = p
            for _ in range(p):
                sym[pos] = s
                pos = (pos + step) & mask
                while pos >= high:
                    pos = (pos + step) & mask
        self.symbol, self.nbits, self.base = sym, [0] * size, [0] * size
        for i in range(size):
            ns = nxt[sym[i]]
            nxt[sym[i]] += 1
            nb = log - _highbit(ns)
            self.nbits[i], self.base[i] = nb, (ns << nb) - size
        self._inv = {}

    @classmethod
    def rle(cls, sym):
        t = cls.__new__(cls)
        t.log, t.size, t.norm, t.low_cells = 0, 1, None, 0
        t.symbol, t.nbits, t.base, t._inv = [sym], [0], [0], {}
        return t

    def states_of(self, s):
        if self.norm is None:       # an RLE table has one state whatever the code written into it
            return [0]
        return [i for i in range(self.size) if self.symbol[i] == s]

    def prev_state(self, s, nxt):
        """The state that emits symbol s and can move to state nxt: (state, value of the transition bits)."""
        inv = self._inv.get(s)
        if inv is None:
            inv = [-1] * self.size
            for i in self.states_of(s):
                for k in range(self.base[i], self.base[i] + (1 << self.nbits[i])):
                    inv[k] = i
            if not any(x >= 0 for x in inv):
                raise SynthError(f"symbol {s} is not in the table")
            self._inv[s] = inv
        st = inv[nxt]
        assert st >= 0
        return st, nxt - self.base[st]

    def chain(self, symbols):
        """States for a run of symbols decoded by one state variable: ([state per symbol], [(bits value, nbits) of the
        transition after each symbol but the last])."""
        n = len(symbols)
        cand = self.states_of(symbols[-1])
        if not cand:
            raise SynthError(f"symbol {symbols[-1]} is not in the table")
        st = [0] * n
        st[-1] = max(cand, key=lambda i: self.nbits[i])
        tr = [None] * (n - 1)
        for j in range(n - 2, -1, -1):
            st[j], v = self.prev_state(symbols[j], st[j + 1])
            tr[j] = (v, self.nbits[st[j]])
        return st, tr


def spread_norm(used, log, nsym=None, low=()):
    """Normalised counts over symbols 0..max: every symbol of `low` gets -1, the others of `used` share the rest of the
    1 << log cells evenly, the first taking the remainder."""
    used = sorted(set(used) - set(low))
    n = (nsym or (max(list(used) + list(low)) + 1))
    norm = [0] * n
    for s in low:
        norm[s] = -1
    rest = (1 << log) - len(low)
    if not used or rest < len(used):
        raise SynthError("table too small")
    for s in used:
        norm[s] = rest // len(used)
    norm[used[0]] += rest - (rest // len(used)) * len(used)
    return norm


# ---- Huffman ----------------------------------------------------------------------------------------------------------

def huf_weights(data, max_bits=11):
    """Weights (symbol 0 .. the largest one present) of a Huffman code for data, code lengths limited to max_bits."""
    cnt = np.bincount(np.frombuffer(data, np.uint8), minlength=256).tolist()
    syms = [s for s in range(256) if cnt[s]]
    if len(syms) < 2:
        raise SynthError("a Huffman tree needs two symbols")
    shift = 0
    while True:
        heap = [(max(cnt[s] >> shift, 1), s, (s,)) for s in syms]
        heapq.heapify(heap)
        depth = dict.fromkeys(syms, 0)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        mx = max(depth.values())
        if mx <= max_bits:
            break
        shift += 1
    return [mx + 1 - depth[s] if s in depth else 0 for s in range(syms[-1] + 1)]


class HufTree:
    def __init__(self, weights, check=True):
        """weights: symbol 0 .. last present symbol; the last one is not written (the decoder implies it)."""
        self.weights = list(weights)
        total = sum(1 << (w - 1) for w in weights if w)
        self.max_bits = _highbit(total)
        if check:
            if total != 1 << self.max_bits:
                raise SynthError("weights do not sum to a power of two")
            if self.max_bits > 11:
                raise SynthError("a code length above 11")
            part = total - (1 << (weights[-1] - 1))
            left = (1 << self.max_bits) - part
            if weights[-1] == 0 or _highbit(part) + 1 != self.max_bits or left != 1 << (weights[-1] - 1):
                raise SynthError("the last weight is not the implied one")
        self.code = {}
        idx = 0
        for bits in range(self.max_bits, 0, -1):    # longest codes take the lowest table cells, symbols ascending
            for s, w in enumerate(weights):
                if w and self.max_bits + 1 - w == bits:
                    self.code[s] = ((idx >> (self.max_bits - bits)) & ((1 << bits) - 1), bits)
                    idx += 1 << (self.max_bits - bits)

    def stream(self, data):
        return backward_stream([self.code[c] for c in data])

    def describe(self, wdesc="direct", fse=None):
        ws = self.weights[:-1]
        if wdesc == "direct":
            if len(ws) > 128:
                raise SynthError("more than 128 direct weights")
            ws2 = ws + [0] * (len(ws) & 1)
            return bytes([127 + len(ws)]) + bytes((ws2[i] << 4) | ws2[i + 1] for i in range(0, len(ws2), 2))
        if len(ws) < 2:
            raise SynthError("two weights at least for the FSE form")
        if fse is None:
            cnt = np.bincount(ws, minlength=13)
            used = [s for s in range(13) if cnt[s]]
            log = 6 if len(used) > 4 else 5
            norm = [0] * (used[-1] + 1)
            rest = 1 << log
            for s in used:                               # proportional, at least 1
                norm[s] = max(1, int(cnt[s]) * (1 << log) // len(ws))
            while sum(norm) > rest:
                norm[int(np.argmax(norm))] -= 1
            while sum(norm) < rest:
                norm[min(used, key=lambda s: norm[s] / cnt[s])] += 1
        else:
            norm, log = fse
        t = FseTable(norm, log)
        a, ta = t.chain(ws[0::2])
        b, tb = t.chain(ws[1::2])
        fields = [(a[0], log), (b[0], log)]
        for j in range(len(ws) - 2):
            fields.append((ta if j % 2 == 0 else tb)[j // 2])
        # the decoder stops when the transition behind the last-but-one weight runs off the stream: it must want a bit
        last2 = (a, b)[(len(ws) - 2) % 2][-1]
        if t.nbits[last2] == 0:
            raise SynthError("the closing state reads no bits")
        body = write_ncount(norm, log) + backward_stream(fields)
        if len(body) >= 128:
            raise SynthError("FSE-compressed weights of 128 bytes or more")
        return bytes([len(body)]) + body


# ---- the writer -------------------------------------------------------------------------------------------------------

def ll_code(v):
    for c in range(35, -1, -1):
        if v >= LL_BASE[c]:
            return c, v - LL_BASE[c], LL_BITS[c]


def ml_code(v):
    if v < 3:
        raise SynthError("a match shorter than 3")
    for c in range(52, -1, -1):
        if v >= ML_BASE[c]:
            return c, v - ML_BASE[c], ML_BITS[c]


def of_code(v):
    c = _highbit(v)
    return c, v - (1 << c), c


class _State:
    """What a decoder carries from block to block, as far as the writer needs it."""

    def __init__(self):
        self.huf = None
        self.tab = {"ll": None, "of": None, "ml": None}


def _lit_header_plain(typ, fmt, regen):
    if fmt is None:
        fmt = 0 if regen < 32 else (1 if regen < 4096 else 3)
    if fmt in (0, 2):
        if regen >= 32:
            raise SynthError("size format too small")
        return bytes([typ | (fmt << 2) | (regen << 3)])
    if fmt == 1:
        if regen >= 4096:
            raise SynthError("size format too small")
        return (typ | (1 << 2) | (regen << 4)).to_bytes(2, "little")
    return (typ | (3 << 2) | (regen << 4)).to_bytes(3, "little")


def _literals(b, st):
    c = b.lit
    typ = c.get("type", "raw")
    regen = c.get("lie_regen", len(b.lits))
    if typ == "raw":
        return _lit_header_plain(0, c.get("fmt"), regen) + b.lits
    if typ == "rle":
        if b.lits != b.lits[:1] * len(b.lits) or not b.lits:
            raise SynthError("RLE literals are one byte repeated")
        return _lit_header_plain(1, c.get("fmt"), regen) + b.lits[:1]
    if typ == "huf":
        tree = HufTree(c["weights"] if c.get("weights") is not None else huf_weights(b.lits), check=c.get("check", True))
        desc = tree.describe(c.get("wdesc", "direct"), c.get("fse"))
        st.huf = tree
    else:
        if st.huf is None and c.get("tree") is None:
            raise SynthError("treeless literals with no tree before them")
        tree, desc = c.get("tree") or st.huf, b""
    fmt = c.get("fmt")
    if fmt is None:
        fmt = 0 if len(b.lits) < 1024 else (2 if len(b.lits) < 16384 else 3)
    if fmt == 0:
        body = tree.stream(b.lits)
    else:
        n = len(b.lits)
        seg = (n + 3) // 4
        if 3 * seg >= n:
            raise SynthError("too few literals for four streams")
        parts = [tree.stream(b.lits[i * seg:(i + 1) * seg]) for i in range(3)] + [tree.stream(b.lits[3 * seg:])]
        body = b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)
    comp = len(desc) + len(body)
    nb, hl = {0: (10, 3), 1: (10, 3), 2: (14, 4), 3: (18, 5)}[fmt]
    if regen >= 1 << nb or comp >= 1 << nb:
        raise SynthError("size format too small")
    h = (2 if typ == "huf" else 3) | (fmt << 2) | (regen << 4) | (comp << (4 + nb))
    return h.to_bytes(hl, "little") + desc + body


def _nseq(n, form):
    if form is None:
        form = 1 if n < 128 else (2 if n < 0x7F00 else 3)
    if form == 1:
        if n >= 128:
            raise SynthError("count form too small")
        return bytes([n])
    if form == 2:
        if n >= 0x7F00:
            raise SynthError("count form too small")
        return bytes([128 + (n >> 8), n & 255])
    if n < 0x7F00:
        raise SynthError("the 3-byte count starts at 0x7F00")
    return bytes([255]) + (n - 0x7F00).to_bytes(2, "little")


def _table(kind, choice, codes, st):
    """-> (mode, description bytes, table).  No choice: predefined where it has every code, else an even FSE table."""
    dnorm, dlog = DEFAULTS[kind]
    if choice is None:
        if all(c < len(dnorm) for c in codes):
            choice = "pre"
        else:
            choice = ("fse", spread_norm(codes, 5 if len(set(codes)) <= 32 else 6), 5 if len(set(codes)) <= 32 else 6)
    if choice == "pre":
        t = FseTable(dnorm, dlog)
        mode, desc = 0, b""
    elif choice == "rle" or (isinstance(choice, tuple) and choice[0] == "rle"):
        sym = choice[1] if isinstance(choice, tuple) else codes[0]
        t, mode, desc = FseTable.rle(sym), 1, bytes([sym])
    elif choice == "rep":
        if st.tab[kind] is None:
            raise SynthError("Repeat_Mode with no table before it")
        return 3, b"", st.tab[kind]
    elif choice == "rep-of-nothing":        # invalid on purpose: written as if the predefined table were there
        return 3, b"", FseTable(dnorm, dlog)
    else:
        _, norm, log = choice[:3]
        check = choice[3] if len(choice) > 3 else True
        t = FseTable(norm, log, check=check) if check else FseTable(_fixup(norm, log), log)
        mode, desc = 2, write_ncount(norm, log)
    st.tab[kind] = t
    return mode, desc, t


def _fixup(norm, log):
    """A table to encode with when the counts are wrong on purpose: the excess or the shortfall goes to symbol 0."""
    n = list(norm)
    n[0] += (1 << log) - sum(abs(x) for x in n)
    return n


def _compressed(b, st):
    out = bytearray(_literals(b, st))
    n = len(b.seqs)
    out += _nseq(n, b.nseq_form)
    if n == 0:
        return bytes(out)
    lls = [ll_code(s[0]) for s in b.seqs]
    mls = [ml_code(s[1]) for s in b.seqs]
    ofs = [of_code(s[2]) for s in b.seqs]
    tabs = {}
    modes, descs = 0, b""
    for kind, choice, codes, shift in (("ll", b.ll, lls, 6), ("of", b.of, ofs, 4), ("ml", b.ml, mls, 2)):
        m, d, t = _table(kind, choice, [c[0] for c in codes], st)
        modes |= m << shift
        descs += d
        tabs[kind] = t
    out.append(modes | b.modes_reserved)
    out += descs
    sl, tl = tabs["ll"].chain([c[0] for c in lls])
    so, to = tabs["of"].chain([c[0] for c in ofs])
    sm, tm = tabs["ml"].chain([c[0] for c in mls])
    f = [(sl[0], tabs["ll"].log), (so[0], tabs["of"].log), (sm[0], tabs["ml"].log)]
    for i in range(n):
        f.append(ofs[i][1:])
        f.append(mls[i][1:])
        f.append(lls[i][1:])
        if i + 1 < n:
            f.append(tl[i])
            f.append(tm[i])
            f.append(to[i])
    out += backward_stream(f, b.pad_bits, b.drop_bits)
    return bytes(out)


def write_block(b, st, last):
    if isinstance(b, Raw):
        return (last | (len(b.data) << 3)).to_bytes(3, "little") + b.data
    if isinstance(b, Rle):
        return (last | 2 | (b.n << 3)).to_bytes(3, "little") + bytes([b.byte])
    body = _compressed(b, st)
    if len(body) > BLOCK_MAX:
        raise SynthError("a compressed block above 128 KiB")
    return (last | 4 | (len(body) << 3)).to_bytes(3, "little") + body


def xxh64(data, seed=0):
    """XXH64 in plain Python (the content checksum is its low 32 bits)."""
    M = (1 << 64) - 1
    P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & M
    rnd = lambda acc, v: (rotl((acc + v * P2) & M, 31) * P1) & M
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed, (seed - P1) & M]
        words = np.frombuffer(data[:n - n % 32], "<u8").tolist()
        for i in range(0, len(words), 4):
            v = [rnd(v[k], words[i + k]) for k in range(4)]
        p = n - n % 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * P1 + P4) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while p + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(data[p:p + 8], "little")), 27) * P1 + P4) & M
        p += 8
    if p + 4 <= n:
        h = (rotl(h ^ (int.from_bytes(data[p:p + 4], "little") * P1) & M, 23) * P2 + P3) & M
        p += 4
    while p < n:
        h = (rotl(h ^ (data[p] * P5) & M, 11) * P1) & M
        p += 1
    h = ((h ^ (h >> 33)) * P2) & M
    h = ((h ^ (h >> 29)) * P3) & M
    return h ^ (h >> 32)


def write_frame(blocks, content=None, single=True, fcs_bytes=None, window_log=None, did=None, checksum=False,
                skippable=(), reserved=0, fcs_value=None, bad_checksum=False, xxh=None, empty_last=False):
    """Frame bytes of the description.  content: the decoded bytes (for the size field and the checksum; execute(blocks)
    when not given).  single / window_log: Single_Segment or a Window_Descriptor of 1 << window_log.  fcs_bytes: 0, 1, 2,
    4, 8 (None: the smallest the header form allows).  did: None or (field bytes, value).  skippable: payloads of
    skippable frames put in front.  empty_last: close the frame with an empty raw block that carries the last flag."""
    if content is None:
        content = execute(blocks)
    size = len(content) if fcs_value is None else fcs_value
    if fcs_bytes is None:
        fcs_bytes = (1 if size < 256 else (2 if size < 65536 + 256 else 4)) if single else 0
    if (fcs_bytes == 1 and not single) or (fcs_bytes == 0 and single):
        raise SynthError("that size field needs the other header form")
    out = bytearray()
    for i, payload in enumerate(skippable):
        out += (0x184D2A50 + (i & 15)).to_bytes(4, "little") + len(payload).to_bytes(4, "little") + payload
    out += MAGIC
    did_flag = 0 if did is None else {1: 1, 2: 2, 4: 3}[did[0]]
    out.append(({0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes] << 6) | (single << 5) | (reserved << 3) | (checksum << 2) | did_flag)
    if not single:
        out.append((window_log - 10) << 3)
    if did is not None:
        out += did[1].to_bytes(did[0], "little")
    if fcs_bytes == 2:
        if not 256 <= size < 65536 + 256:
            raise SynthError("the 2-byte size field holds 256..65791")
        out += (size - 256).to_bytes(2, "little")
    elif fcs_bytes:
        out += size.to_bytes(fcs_bytes, "little")
    st = _State()
    blocks = list(blocks) + ([Raw(b"")] if empty_last else [])
    for i, b in enumerate(blocks):
        out += write_block(b, st, 1 if i + 1 == len(blocks) else 0)
    if checksum:
        h = (xxh or xxh64)(content) & 0xFFFFFFFF
        out += (h ^ (1 if bad_checksum else 0)).to_bytes(4, "little")
    return bytes(out)
