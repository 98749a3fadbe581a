"""A plain-Python model of znippy_bunzip2_batch (not a test module): the bzip2 CRC, a block decoder that applies the rules of
include/znippy_hip.h in their order, and the chain over a whole item.  Slow and simple; the tests use it for CRCs, for the records
and statuses they expect, and for the verdict on damaged input."""

OK, E_INVAL, E_NOMEM, E_DST_SMALL, E_CORRUPT, E_UNSUPPORTED, E_CHECKSUM = 0, -1, -3, -4, -5, -6, -7
BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090
MAX_SEL, GROUP = 18002, 50
STEP_BOUND = 3_000_000  # symbols one block may take before the model gives up (Undecided)


class Bad(Exception):
    def __init__(self, status):
        self.status = status


class Undecided(Exception):
    pass


def _table():
    t = []
    for i in range(256):
        c = i << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
        t.append(c)
    return t


_T = _table()


def crc(data, c=0xFFFFFFFF):
    """the bzip2 CRC-32: polynomial 0x04C11DB7, MSB first"""
    for b in data:
        c = ((c << 8) & 0xFFFFFFFF) ^ _T[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


def crc_by_reflection(data):
    """the same value from zlib's CRC: bit-reversed bytes in, bit-reversed result out"""
    import zlib
    rev = bytes(int(f"{b:08b}"[::-1], 2) for b in data)
    return int(f"{zlib.crc32(rev):032b}"[::-1], 2)


def combine(c, block_crc):
    return (((c << 1) | (c >> 31)) & 0xFFFFFFFF) ^ block_crc


class Bits:
    """MSB-first reader; zeros behind the end, `pos` says how far a caller went"""

    def __init__(self, data, pos=0):
        self.v = int.from_bytes(data, "big") if data else 0
        self.n = 8 * len(data)
        self.pos = pos

    def get(self, k):
        p = self.pos
        self.pos += k
        if p + k <= self.n:
            return (self.v >> (self.n - p - k)) & ((1 << k) - 1)
        have = max(self.n - p, 0)
        return ((self.v & ((1 << have) - 1)) << (k - have)) & ((1 << k) - 1)

    def over(self):
        return self.pos > self.n


def magic_positions(data, magic=BLOCK_MAGIC):
    """every bit position where the 48-bit pattern starts"""
    v, n = int.from_bytes(data, "big"), 8 * len(data)
    return [p for p in range(n - 47) if (v >> (n - p - 48)) & 0xFFFFFFFFFFFF == magic]


def decode_block(b, limit):
    """b stands behind a block magic.  -> (crc, orig, bytes in front of the inverse BWT); raises Bad"""
    want = b.get(32)
    if b.get(1):
        raise Bad(E_CORRUPT if b.over() else E_UNSUPPORTED)
    orig = b.get(24)
    in16 = b.get(16)
    seq = []
    for i in range(16):
        if in16 & (0x8000 >> i):
            m = b.get(16)
            seq += [16 * i + j for j in range(16) if m & (0x8000 >> j)]
    if b.over() or not seq:
        raise Bad(E_CORRUPT)
    alpha, eob = len(seq) + 2, len(seq) + 1
    n_groups = b.get(3)
    if not 2 <= n_groups <= 6:
        raise Bad(E_CORRUPT)
    n_sel = b.get(15)
    if n_sel < 1:
        raise Bad(E_CORRUPT)
    sel = []
    for i in range(n_sel):
        j = 0
        while j < n_groups and b.get(1):
            j += 1
        if j >= n_groups or b.over():
            raise Bad(E_CORRUPT)
        if i < MAX_SEL:
            sel.append(j)
    order = list(range(n_groups))
    for i, j in enumerate(sel):
        order.insert(0, order.pop(j))
        sel[i] = order[0]
    tables = []
    for _ in range(n_groups):
        curr = b.get(5)
        lens = []
        for _ in range(alpha):
            while True:
                if not 1 <= curr <= 20:
                    raise Bad(E_CORRUPT)
                if not b.get(1):
                    break
                curr += -1 if b.get(1) else 1
            lens.append(curr)
        if b.over():
            raise Bad(E_CORRUPT)
        tables.append(lens)
    codes = []
    for lens in tables:
        if sum(1 << (20 - l) for l in lens) > 1 << 20:
            raise Bad(E_CORRUPT)  # over-subscribed
        code, d = 0, {}
        for l in range(1, 21):
            for s, sl in enumerate(lens):
                if sl == l:
                    d[(l, code)] = s
                    code += 1
            code <<= 1
        codes.append(d)
    mtf = list(range(256))
    out = bytearray()
    run, weight, steps = 0, 1, 0
    group, left, d = 0, 0, None
    while True:
        steps += 1
        if steps > STEP_BOUND:
            raise Undecided()
        if left == 0:
            if group >= len(sel):
                raise Bad(E_CORRUPT)
            d = codes[sel[group]]
            group += 1
            left = GROUP
        left -= 1
        code, sym = 0, None
        for l in range(1, 21):
            code = code << 1 | b.get(1)
            sym = d.get((l, code))
            if sym is not None:
                break
        if sym is None or b.over():
            raise Bad(E_CORRUPT)
        if sym <= 1:
            run += (sym + 1) * weight
            weight <<= 1
            if run > limit:
                raise Bad(E_CORRUPT)
            continue
        if run:
            if len(out) + run > limit:
                raise Bad(E_CORRUPT)
            out += bytes([seq[mtf[0]]]) * run
            run, weight = 0, 1
        if sym == eob:
            break
        if len(out) >= limit:
            raise Bad(E_CORRUPT)
        mtf.insert(0, mtf.pop(sym - 1))
        out.append(seq[mtf[0]])
    if orig >= len(out):
        raise Bad(E_CORRUPT)
    return want, orig, bytes(out)


def inverse_bwt(ll, orig):
    n = len(ll)
    order = sorted(range(n), key=lambda i: ll[i])  # stable: the successor array
    out = bytearray(n)
    p = order[orig]
    for k in range(n):
        out[k] = ll[p]
        p = order[p]
    return bytes(out)


def unrle1(data):
    out = bytearray()
    run, last = 0, -1
    for v in data:
        if run == 4:
            out += bytes([last]) * v
            run = 0
        else:
            out.append(v)
            if run > 0 and v == last:
                run += 1
            else:
                last, run = v, 1
    return bytes(out)


def block_content(ll, orig):
    return unrle1(inverse_bwt(ll, orig))


def walk(data, room=None):
    """The chain over one item in a room of `room` bytes (None: no limit) -> (status, content, streams, blocks, records).  records: per block (bit position of its magic, bit
    position of the magic behind it, bytes in front of the final run-length step, bytes behind it)."""
    if not data:
        return OK, b"", 0, 0, []
    b = Bits(data)
    content, records = bytearray(), []
    streams = blocks = 0
    sum_bad = False
    at = 0  # byte position of the stream header
    try:
        while True:
            b.pos = 8 * at
            head = b.get(32)
            level = (head & 255) - 0x30
            if b.over() or head >> 8 != 0x425A68 or not 1 <= level <= 9:
                raise Bad(E_CORRUPT)
            comb = 0
            while True:
                start = b.pos
                magic = b.get(48)
                if b.over():
                    raise Bad(E_CORRUPT)
                if magic == BLOCK_MAGIC:
                    want, orig, ll = decode_block(b, level * 100000)
                    piece = block_content(ll, orig)
                    records.append((start, b.pos, len(ll), len(piece)))
                    if room is not None and len(content) + len(piece) > room:
                        raise Bad(E_DST_SMALL)
                    if crc(piece) != want:
                        sum_bad = True
                    content += piece
                    comb = combine(comb, want)
                    blocks += 1
                elif magic == END_MAGIC:
                    break
                else:
                    raise Bad(E_CORRUPT)
            stored = b.get(32)
            if b.over():
                raise Bad(E_CORRUPT)
            if stored != comb:
                sum_bad = True
            streams += 1
            at = (b.pos + 7) // 8
            if data[at:at + 3] != b"BZh":
                break
    except Bad as e:
        return e.status, b"", 0, 0, records
    if sum_bad:
        return E_CHECKSUM, b"", 0, 0, records
    return OK, bytes(content), streams, blocks, records


def expect(data, room=None):
    """-> (status, content, streams, blocks) as znippy_bunzip2_batch reports them for a room of `room` bytes (None: measure mode, where
    no CRC is checked)"""
    status, content, streams, blocks, records = walk(data, room)
    if room is None and status == E_CHECKSUM:
        raise NotImplementedError("measure mode of an item whose only fault is a checksum: ask walk() for the records")
    return status, content, streams, blocks
