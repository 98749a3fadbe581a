"""A bit-level writer of bzip2 streams with every field scriptable (not a test module), in the manner of deflate_build.py: the tests
build the blocks no compressor writes — a chosen number of tables, a code of length 20, more selectors than 18002, a chosen origPtr,
symbols chosen one by one — and the damaged ones.  block_fields() turns content into the fields of one block; Block writes fields,
each of which a test may replace first."""
import bz_model as M

RUNA, RUNB = 0, 1


class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, k):
        assert 0 <= value < 1 << k, (value, k)
        self.v = self.v << k | value
        self.n += k

    def pad(self):
        if self.n % 8:
            self.put(0, 8 - self.n % 8)

    def bytes(self):
        assert self.n % 8 == 0
        return self.v.to_bytes(self.n // 8, "big")


def rle1(data):
    """the first run-length step: runs of 4 .. 255 equal bytes become four of them and a count"""
    out, i = bytearray(), 0
    while i < len(data):
        j = i
        while j < len(data) and data[j] == data[i] and j - i < 255:
            j += 1
        out += data[i:i + min(j - i, 4)]
        if j - i >= 4:
            out.append(j - i - 4)
        i = j
    return bytes(out)


def bwt(s):
    """-> (last column, origPtr), by sorting the rotations (small blocks only)"""
    n = len(s)
    d = s + s
    rot = sorted(range(n), key=lambda i: d[i:i + n])
    return bytes(d[i + n - 1] for i in rot), rot.index(0)


def mtf_symbols(ll, used):
    """bytes in front of the inverse BWT -> the symbols of the block (RUNA/RUNB runs, MTF index + 1) and the end-of-block symbol"""
    mtf = list(used)
    out, zeros = [], 0

    def flush():
        nonlocal zeros
        while zeros > 0:  # bijective base 2, least significant first
            out.append(RUNA if zeros & 1 else RUNB)
            zeros = (zeros - 1) >> 1

    for v in ll:
        k = mtf.index(v)
        if k == 0:
            zeros += 1
        else:
            flush()
            out.append(k + 1)
            mtf.insert(0, mtf.pop(k))
    flush()
    return out + [len(used) + 1]


def flat_lens(alpha):
    """every symbol the same length: the shortest that gives each a code (an incomplete code unless alpha is a power of two)"""
    return [max((alpha - 1).bit_length(), 1)] * alpha


def canonical(lens):
    code, out = 0, [0] * len(lens)
    for l in range(1, 21):
        for s, sl in enumerate(lens):
            if sl == l:
                out[s] = code
                code += 1
        code <<= 1
    return out


class Block:
    """The fields of one block.  Replace any before write(): crc, randomised, orig, used (sorted byte values), n_groups, tables (code
    lengths per table), selectors (a table per group of 50 symbols), n_selectors (the count written; more than len(selectors) repeats
    table 0), symbols, magic.  raw_symbol_bits: (value, bits) pairs written instead of the coded symbols."""

    def __init__(self, used, symbols, orig, crc, n_groups=2, tables=None, selectors=None):
        self.magic = M.BLOCK_MAGIC
        self.crc, self.randomised, self.orig = crc, 0, orig
        self.used, self.symbols = list(used), list(symbols)
        self.n_groups = n_groups
        self.tables = tables if tables is not None else [flat_lens(len(self.used) + 2) for _ in range(n_groups)]
        self.selectors = selectors if selectors is not None else [0] * max((len(self.symbols) + 49) // 50, 1)
        self.n_selectors = None
        self.raw_symbol_bits = None
        self.start_lens = None  # the 5-bit start value of each table (None: its first length)

    def write(self, w):
        w.put(self.magic, 48)
        w.put(self.crc, 32)
        w.put(self.randomised, 1)
        w.put(self.orig, 24)
        rows = [sum(0x8000 >> (v & 15) for v in self.used if v >> 4 == i) for i in range(16)]
        w.put(sum(0x8000 >> i for i in range(16) if rows[i]), 16)
        for r in rows:
            if r:
                w.put(r, 16)
        w.put(self.n_groups, 3)
        n_sel = len(self.selectors) if self.n_selectors is None else self.n_selectors
        w.put(n_sel, 15)
        order = list(range(max(self.n_groups, 6)))
        for i in range(n_sel):
            t = self.selectors[i] if i < len(self.selectors) else 0
            j = order.index(t)
            order.insert(0, order.pop(j))
            w.put((1 << (j + 1)) - 2, j + 1)  # j ones and a zero
        for t, lens in enumerate(self.tables):
            curr = lens[0] if self.start_lens is None else self.start_lens[t]
            w.put(curr, 5)
            for l in lens:
                while curr < l:
                    w.put(2, 2)
                    curr += 1
                while curr > l:
                    w.put(3, 2)
                    curr -= 1
                w.put(0, 1)
        if self.raw_symbol_bits is not None:
            for v, k in self.raw_symbol_bits:
                w.put(v, k)
            return
        codes = [canonical(lens) for lens in self.tables]
        for i, s in enumerate(self.symbols):
            t = self.selectors[i // 50]
            w.put(codes[t][s], self.tables[t][s])


def block_fields(piece, **kw):
    """one block that holds `piece` (content; small: the rotations are sorted naively)"""
    pre = rle1(piece)
    ll, orig = bwt(pre)
    used = sorted(set(ll))
    return Block(used, mtf_symbols(ll, used), orig, M.crc(piece), **kw)


def block_from_symbols(used, symbols, orig, **kw):
    """a block given by its symbols (without the end-of-block symbol, which is added) -> (Block, the content it decodes to)"""
    mtf, ll = list(range(256)), bytearray()
    run, weight = 0, 1
    for s in list(symbols) + [len(used) + 1]:
        if s <= 1:
            run += (s + 1) * weight
            weight <<= 1
            continue
        ll += bytes([used[mtf[0]]]) * run
        run, weight = 0, 1
        if s <= len(used):
            mtf.insert(0, mtf.pop(s - 1))
            ll.append(used[mtf[0]])
    content = M.block_content(bytes(ll), orig)
    return Block(used, list(symbols) + [len(used) + 1], orig, M.crc(content), **kw), content


def accepted_block(used, symbols, **kw):
    """block_from_symbols with the first origPtr whose content Python's bz2 accepts (libbz2 refuses a block that ends in four equal
    bytes without their count, or whose last count reaches past the block)"""
    import bz2
    for orig in range(64):
        try:
            blk, content = block_from_symbols(used, symbols, orig, **kw)
            if bz2.decompress(stream([blk])) == content:
                return blk, content
        except (OSError, ValueError, IndexError):  # (IndexError: origPtr beyond the block)
            pass
    raise AssertionError("no origPtr gives a block that bz2 accepts")


def stream(blocks, level=1, crc=None, head=None, end_magic=M.END_MAGIC):
    """blocks: Block objects.  crc: the combined CRC written (None: folded from the blocks' crc fields)"""
    w = BitWriter()
    for c in (head if head is not None else b"BZh" + bytes([0x30 + level])):
        w.put(c, 8)
    comb = 0
    for b in blocks:
        b.write(w)
        comb = M.combine(comb, b.crc)
    w.put(end_magic, 48)
    w.put(comb if crc is None else crc, 32)
    w.pad()
    return w.bytes()


def flip(data, bit):
    out = bytearray(data)
    out[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(out)
