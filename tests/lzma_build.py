"""A scripted LZMA range encoder: a list of operations — ("lit", byte), ("match", distance, length), ("rep", k, length) with k 0..3,
("shortrep",), ("eopm",) the end marker LZMA2 forbids — is turned into LZMA2 chunks under given lc/lp/pb, with the bytes it stands
for.  It makes no choices: every operation is coded as given, so a test reaches a length, a distance slot, a state or a rep
order by naming it.  A distance beyond the bytes produced is coded too (its copy reads zeros): that is a damaged case.
tests/test_xz_build_cpu.py proves against liblzma that the chunks decode to the bytes claimed."""
import struct

P_IS_MATCH, P_IS_REP, P_REP_G0, P_REP_G1, P_REP_G2, P_REP0_LONG, P_SLOT, P_SPEC, P_ALIGN, P_LEN, P_REPLEN, P_LIT = (
    0, 192, 204, 216, 228, 240, 432, 688, 816, 832, 1346, 1860)
LEN_CHOICE, LEN_CHOICE2, LEN_LOW, LEN_MID, LEN_HIGH = 0, 1, 2, 130, 258


class RangeEncoder:
    def __init__(self):
        self.low, self.range, self.cache, self.cache_size = 0, 0xFFFFFFFF, 0, 1
        self.out = bytearray()
        self.carry_run = 0   # the longest run of pending 0xFF bytes a carry went through

    def shift_low(self):
        if self.low < 0xFF000000 or self.low >= 1 << 32:
            carry = self.low >> 32
            if carry:
                self.carry_run = max(self.carry_run, self.cache_size - 1)
            tmp = self.cache
            while True:
                self.out.append((tmp + carry) & 0xFF)
                tmp = 0xFF
                self.cache_size -= 1
                if self.cache_size == 0:
                    break
            self.cache = (self.low >> 24) & 0xFF
        self.cache_size += 1
        self.low = (self.low & 0x00FFFFFF) << 8

    def norm(self):
        while self.range < 1 << 24:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self.shift_low()

    def bit(self, probs, i, b):
        p = probs[i]
        bound = (self.range >> 11) * p
        if b:
            self.low += bound
            self.range -= bound
            probs[i] = p - (p >> 5)
        else:
            self.range = bound
            probs[i] = p + ((2048 - p) >> 5)
        self.norm()

    def direct(self, v, bits):
        for i in reversed(range(bits)):
            self.range >>= 1
            if (v >> i) & 1:
                self.low += self.range
            self.norm()

    def tree(self, probs, base, bits, v):
        m = 1
        for i in reversed(range(bits)):
            b = (v >> i) & 1
            self.bit(probs, base + m, b)
            m = m << 1 | b

    def rtree(self, probs, base, bits, v):
        m = 1
        for i in range(bits):
            b = (v >> i) & 1
            self.bit(probs, base + m, b)
            m = m << 1 | b

    def flush(self):
        for _ in range(5):
            self.shift_low()


def dist_slot(d):
    """the slot of the 0-based distance d"""
    if d < 4:
        return d
    n = d.bit_length() - 1
    return 2 * n + ((d >> (n - 1)) & 1)


class Writer:
    """LZMA2 chunks, one call per chunk; out() gives (the raw LZMA2 bytes with the end byte, the content)."""

    def __init__(self, lc=3, lp=0, pb=2):
        self.lc, self.lp, self.pb = lc, lp, pb
        self.raw = bytearray()
        self.content = bytearray()
        self.hist = bytearray()   # the bytes since the last dictionary reset
        self.states = []          # the LZMA state in front of every operation
        self.lit_states = set()   # and in front of the literals
        self.carry_run = 0
        # bookkeeping for coverage conditions (tests/test_lzma_random_cpu.py): what the operations coded so far have reached
        self.op_states = set()    # (kind: lit, match, rep0..rep3, shortrep; the state in front of it)
        self.len_ps = set()       # ("match" or "rep", length class 0 / 1 / 2, pos-state, pb)
        self.slots = set()        # distance slots
        self.aligns = set()       # the four align bits of the distances of slot 14 and above
        self.matched_lits = set() # literals coded in matched mode: "eq" (the match byte itself) or the highest bit in which they differ from it
        self.chunks = []          # (control: 0xE0 / 0xC0 / 0xA0 / 0x80 / 1 / 2, content offset, offset of the dictionary's start, lc, lp, pb)
        self.reset_state()

    def reset_state(self):
        self.probs = [1024] * (P_LIT + (0x300 << (self.lc + self.lp)))
        self.state = 0
        self.reps = [0, 0, 0, 0]

    def _len(self, rc, base, ps, length):
        v = length - 2
        self.len_ps.add(("match" if base == P_LEN else "rep", min(v >> 3, 2), ps, self.pb))
        if v < 8:
            rc.bit(self.probs, base + LEN_CHOICE, 0)
            rc.tree(self.probs, base + LEN_LOW + ps * 8, 3, v)
        elif v < 16:
            rc.bit(self.probs, base + LEN_CHOICE, 1)
            rc.bit(self.probs, base + LEN_CHOICE2, 0)
            rc.tree(self.probs, base + LEN_MID + ps * 8, 3, v - 8)
        else:
            rc.bit(self.probs, base + LEN_CHOICE, 1)
            rc.bit(self.probs, base + LEN_CHOICE2, 1)
            rc.tree(self.probs, base + LEN_HIGH, 8, v - 16)

    def _copy(self, dist, length):
        for _ in range(length):
            b = self.hist[-dist] if dist <= len(self.hist) else 0
            self.hist.append(b)
            self.content.append(b)

    def _op(self, rc, op):
        P, st = self.probs, self.state
        ps = len(self.hist) & ((1 << self.pb) - 1)
        self.states.append(st)
        self.op_states.add((op[0] + str(op[1]) if op[0] == "rep" else op[0], st))
        if op[0] == "lit":
            self.lit_states.add(st)
            byte = op[1]
            rc.bit(P, P_IS_MATCH + (st << 4) + ps, 0)
            prev = self.hist[-1] if self.hist else 0
            base = P_LIT + 0x300 * (((len(self.hist) & ((1 << self.lp) - 1)) << self.lc) + (prev >> (8 - self.lc)))
            sym = 1
            if st < 7:
                for i in reversed(range(8)):
                    b = (byte >> i) & 1
                    rc.bit(P, base + sym, b)
                    sym = sym << 1 | b
            else:
                m = self.hist[-self.reps[0] - 1] if self.reps[0] < len(self.hist) else 0
                self.matched_lits.add((m ^ byte).bit_length() - 1 if m != byte else "eq")
                offs = 0x100
                for i in reversed(range(8)):
                    m <<= 1
                    mbit = m & offs
                    b = (byte >> i) & 1
                    rc.bit(P, base + offs + mbit + sym, b)
                    sym = sym << 1 | b
                    offs &= mbit if b else ~mbit
            self.hist.append(byte)
            self.content.append(byte)
            self.state = 0 if st < 4 else st - 3 if st < 10 else st - 6
            return
        rc.bit(P, P_IS_MATCH + (st << 4) + ps, 1)
        if op[0] in ("match", "eopm"):
            d, length = (0xFFFFFFFF, 2) if op[0] == "eopm" else (op[1] - 1, op[2])
            rc.bit(P, P_IS_REP + st, 0)
            self._len(rc, P_LEN, ps, length)
            slot = dist_slot(d)
            if op[0] == "match":
                self.slots.add(slot)
                if slot >= 14:
                    self.aligns.add(d & 15)
            rc.tree(P, P_SLOT + (min(length - 2, 3) << 6), 6, slot)
            if slot >= 4:
                nd = (slot >> 1) - 1
                base = (2 | (slot & 1)) << nd
                if slot < 14:
                    rc.rtree(P, P_SPEC + base - slot - 1, nd, d - base)
                else:
                    rc.direct((d - base) >> 4, nd - 4)
                    rc.rtree(P, P_ALIGN, 4, (d - base) & 15)
            self.reps = [d] + self.reps[:3]
            self.state = 7 if st < 7 else 10
            if op[0] == "match":
                self._copy(d + 1, length)
            return
        rc.bit(P, P_IS_REP + st, 1)
        if op[0] == "shortrep":
            rc.bit(P, P_REP_G0 + st, 0)
            rc.bit(P, P_REP0_LONG + (st << 4) + ps, 0)
            self.state = 9 if st < 7 else 11
            self._copy(self.reps[0] + 1, 1)
            return
        assert op[0] == "rep"
        k, length = op[1], op[2]
        if k == 0:
            rc.bit(P, P_REP_G0 + st, 0)
            rc.bit(P, P_REP0_LONG + (st << 4) + ps, 1)
        else:
            rc.bit(P, P_REP_G0 + st, 1)
            rc.bit(P, P_REP_G1 + st, 0 if k == 1 else 1)
            if k > 1:
                rc.bit(P, P_REP_G2 + st, 0 if k == 2 else 1)
            r = self.reps
            self.reps = [r[k]] + r[:k] + r[k + 1:]
        self._len(rc, P_REPLEN, ps, length)
        self.state = 8 if st < 7 else 11
        self._copy(self.reps[0] + 1, length)

    def lzma(self, ops, control=0xE0, props=None, usize=None, csize=None):
        """One LZMA chunk.  control: 0xE0 dictionary reset + properties + state reset, 0xC0 properties + state reset, 0xA0 state reset,
        0x80 nothing.  props: a property byte other than the writer's.  usize / csize: sizes for the header other than the true ones."""
        if control >= 0xE0:
            self.hist = bytearray()
        if control >= 0xA0:
            self.reset_state()
        rc = RangeEncoder()
        start = len(self.content)
        self.chunks.append((control & 0xE0, start, start - len(self.hist), self.lc, self.lp, self.pb))
        for op in ops:
            self._op(rc, op)
        rc.flush()
        self.carry_run = max(self.carry_run, rc.carry_run)
        u = len(self.content) - start if usize is None else usize
        c = len(rc.out) if csize is None else csize
        assert 1 <= u <= 1 << 21 and 1 <= c <= 1 << 16, (u, c)
        self.raw += bytes([control | (u - 1) >> 16]) + struct.pack(">HH", (u - 1) & 0xFFFF, c - 1)
        if control >= 0xC0:
            self.raw.append((self.pb * 5 + self.lp) * 9 + self.lc if props is None else props)
        self.raw += rc.out
        return self

    def stored(self, data, reset_dict):
        """One uncompressed chunk: control 1 (dictionary reset) or 2."""
        assert 1 <= len(data) <= 1 << 16
        if reset_dict:
            self.hist = bytearray()
        self.chunks.append((1 if reset_dict else 2, len(self.content), len(self.content) - len(self.hist), self.lc, self.lp, self.pb))
        self.raw += bytes([1 if reset_dict else 2]) + struct.pack(">H", len(data) - 1) + data
        self.hist += data
        self.content += data
        return self

    def out(self):
        return bytes(self.raw) + b"\x00", bytes(self.content)
