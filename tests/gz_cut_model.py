"""A model of the block-start search of znippy_gunzip_batch (znippy_ctx_set_gunzip_cut), written from RFC 1951 and independent of
csrc/gz_cut_rules.h (not a test module: pytest does not collect it): the header test at one bit position, a walker that returns the
true block starts of a stream, the grid rule that keeps one candidate per window, and the segments of a file that is cut."""
import functools

import numpy as np

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Bits:
    """data as bits, LSB of byte 0 first; bits past the end read as zero"""

    def __init__(self, data):
        self.data = bytes(data)
        self.nbits = 8 * len(self.data)
        pad = self.data + bytes(16)
        b = np.frombuffer(pad, np.uint8).astype(np.uint64)
        w = np.zeros(len(pad) - 8, np.uint64)
        for k in range(8):
            w |= b[k:k + len(w)] << np.uint64(8 * k)
        self.words = [int(x) for x in w]                  # words[i]: bytes i .. i + 7, little-endian

    def take(self, pos, k):                               # k <= 57
        i = pos >> 3
        if i >= len(self.words):
            return 0
        return (self.words[i] >> (pos & 7)) & ((1 << k) - 1)


def canon(lens):
    """{(length, code read MSB first): symbol} of a canonical code; None if over-subscribed.  Second value: the Kraft sum in units
    of 2^-15"""
    kraft = sum(1 << (15 - l) for l in lens if l)
    if kraft > 1 << 15:
        return None, kraft
    table, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                table[(l, code)] = s
                code += 1
        code <<= 1
    return table, kraft


def read_sym(b, pos, table, longest):
    code = 0
    for l in range(1, longest + 1):
        code = code << 1 | b.take(pos + l - 1, 1)
        if (l, code) in table:
            return table[(l, code)], pos + l
    return None, pos


def dynamic_header(b, pos):
    """the header of a dynamic block whose HLIT field starts at pos -> (literal/length lengths, distance lengths, first bit behind
    the header), or None where a rule of znippy_inflate_batch is broken or the input ends first"""
    hlit, hdist, hclen = b.take(pos, 5) + 257, b.take(pos + 5, 5) + 1, b.take(pos + 10, 4) + 4
    pos += 14
    if hlit > 286 or hdist > 30:
        return None
    cl = [0] * 19
    for i in range(hclen):
        cl[CL_ORDER[i]] = b.take(pos, 3)
        pos += 3
    table, kraft = canon(cl)
    if table is None or kraft != 1 << 15:                 # the code-length code: complete
        return None
    lens = []
    while len(lens) < hlit + hdist:
        sym, pos = read_sym(b, pos, table, 7)
        if sym is None:
            return None
        if sym < 16:
            lens.append(sym)
        elif sym == 16:
            if not lens:
                return None
            lens += [lens[-1]] * (3 + b.take(pos, 2))
            pos += 2
        elif sym == 17:
            lens += [0] * (3 + b.take(pos, 3))
            pos += 3
        else:
            lens += [0] * (11 + b.take(pos, 7))
            pos += 7
        if len(lens) > hlit + hdist:
            return None
    if pos > b.nbits:
        return None
    ll, dd = lens[:hlit], lens[hlit:]
    if ll[256] == 0:
        return None
    for s in (ll, dd):
        table, kraft = canon(s)
        if table is None or (kraft < 1 << 15 and max(s) > 1):
            return None
    return ll, dd, pos


def passes(b, bit):
    """the header test: a non-final dynamic block with a valid header starts at `bit`"""
    if b.take(bit, 1) != 0 or b.take(bit + 1, 2) != 2:
        return False
    return dynamic_header(b, bit + 3) is not None


def quick_positions(data):
    """the bit positions whose first 13 bits can be a non-final dynamic block's (a vectorised filter in front of passes)"""
    bits = np.unpackbits(np.frombuffer(bytes(data), np.uint8), bitorder="little").astype(np.uint32)
    n = len(bits)
    pad = np.concatenate([bits, np.zeros(16, np.uint32)])
    v = np.zeros(n, np.uint32)
    for i in range(13):
        v |= pad[i:i + n] << np.uint32(i)
    ok = ((v & 7) == 4) & (((v >> 3) & 31) <= 29) & (((v >> 8) & 31) <= 29)
    return [int(p) for p in np.nonzero(ok)[0]]


@functools.lru_cache(maxsize=None)
def _passing(data):
    b = Bits(data)
    return tuple(p for p in quick_positions(data) if passes(b, p))


def passing_positions(data):
    """every bit position of `data` that passes the header test, ascending (computed once per file and process)"""
    return list(_passing(bytes(data)))


def block_starts(stream, start_bit=0):
    """walks a valid raw DEFLATE stream -> [(bit position, BFINAL, BTYPE)] of its blocks, and the first bit behind the last"""
    from deflate_build import FIXED_D, FIXED_LL
    b = Bits(stream)
    pos, out = start_bit, []
    while True:
        final, btype = b.take(pos, 1), b.take(pos + 1, 2)
        out.append((pos, final, btype))
        pos += 3
        assert btype != 3 and pos <= b.nbits
        if btype == 0:
            pos = (pos + 7) & ~7
            ln = b.take(pos, 16)
            assert ln == b.take(pos + 16, 16) ^ 0xFFFF
            pos += 32 + 8 * ln
        else:
            if btype == 1:
                ll, dd = FIXED_LL, FIXED_D
            else:
                h = dynamic_header(b, pos)
                assert h is not None, "the walker is for valid streams"
                ll, dd, pos = h
            lt, _ = canon(ll)
            dt, _ = canon(dd)
            while True:
                sym, pos = read_sym(b, pos, lt, 15)
                assert sym is not None
                if sym == 256:
                    break
                if sym > 256:
                    pos += LEXT[sym - 257]
                    d, pos = read_sym(b, pos, dt, 15)
                    assert d is not None and d < 30
                    pos += DEXT[d]
        assert pos <= b.nbits
        if final:
            return out, pos


def true_starts(stream, start_bit=0):
    """the bit positions of the stream's non-final dynamic blocks: what the search must not miss"""
    return [p for p, final, btype in block_starts(stream, start_bit)[0] if not final and btype == 2]


def searched(src_len, cut):
    return cut > 0 and src_len >= 2 * cut


def kept(positions, src_len, cut):
    """the grid rule: {window: the lowest passing bit position of the window} of an item of src_len bytes; windows of cut source
    bytes counted from the item's byte 0; items below 2 * cut bytes are not searched"""
    out = {}
    if searched(src_len, cut):
        for p in sorted(positions):
            out.setdefault((p >> 3) // cut, p)
    return out


def expect_stats(items, cut):
    """(positions tested, positions that pass, candidates kept) of a batch of files"""
    tested = passed = n_kept = 0
    for s in items:
        if searched(len(s), cut):
            pos = passing_positions(s)
            tested += 8 * len(s)
            passed += len(pos)
            n_kept += len(kept(pos, len(s), cut))
    return tested, passed, n_kept


def expect_cut(data, cut, seg_min=0):
    """a valid gzip file with the switch at `cut`: (True, its segments, the bit positions the chain lands on), or None where the file is
    not searched or no block candidate is kept: the call then decodes it as with the switch off.  The chain goes, member by member,
    from block boundary to block boundary of the true stream and lands on every kept candidate that is one — a kept block candidate
    of the search, or a flush candidate the scan keeps (gz_model.candidates); without joins, segments = members + candidates landed
    on, empty pieces included."""
    import gz_model
    if not searched(len(data), cut):
        return None
    k = set(kept(passing_positions(data), len(data), cut).values())
    if not k:
        return None
    scan, overflow = gz_model.candidates(data, seg_min or gz_model.SEG_MIN_DEFAULT)
    assert not overflow
    k |= {8 * p for p, kind in scan if kind == 0}
    members = gz_model.members_of(data)
    landed = []
    for _, start, _, _ in members:
        blocks, _ = block_starts(data[start:])
        landed += [8 * start + p for p, _, _ in blocks[1:] if 8 * start + p in k]
    return True, len(members) + len(landed), sorted(landed)
