"""The RFC 8878 table-description rules of znippy_amd/csrc/zstd_rules.h (what every device parser calls: normalised counts, the
spread and the cell rule, symbol meaning, the sequences header walk, the Huffman tree description) as a stand-alone host program
under AddressSanitizer and UBSan.  Descriptions go in on stdin, every field comes back, and a model written here from the RFC's
statements is compared with it field by field.  The writer of tests/zstd_synth.py is the second, independent source: what it
writes must read back as what it was given, and its tables must equal the program's cell by cell.

Every function runs over both storage shapes: flat arrays, and a lane's stripe ([i * 64 + lane]) at lanes 0, 31 and 63 of a
region whose other stripes hold a pattern that must survive.  Regions are heap blocks of exactly the size the device gives
them (64 or 256 counts, 1 << log cells, 256 weights, 16 ranks), so a store past the end is the sanitizer's.  The counts go
through both forward bit readers (FwdR bit by bit, FwdW with a register window).

A rule that is wrong is noticed: with the spread's `pos >= high` step removed from a scratch copy of the header (the first
experiment of tests/test_gpu_synth.py's docstring, against the shared body), test_tables fails on the first table with "less
than 1" symbols (the walk ends on cell 11, not 0: `assert [11] == [0, 0, 2, 20, ...]`) and test_predefined_tables on the
literal-length table (`assert [20, 1] == [0, 1]`); the other four tests pass, none of their cases has such a symbol in play.

Cases: 1,311 count descriptions (13,920 runs over readers, shapes and caps), 600 table runs, the 3 predefined tables in 4 shapes,
147 sequence sections x 8 want masks, 322 Huffman descriptions cut at every length (57,376 runs)."""
import os
import random
import shutil
import subprocess

import pytest

import zstd_synth as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "znippy_amd", "csrc")
E_TRUNC = E_CORRUPT = -5
E_UNSUP = -6

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>
#include "zstd_rules.h"
using namespace zr;

// n entries of T, flat or striped by 64; exactly that large on the heap; the stripes of the other lanes keep a pattern
template <class T, bool STRIPED>
struct Region {
    T *v; size_t n; uint32_t lane;
    static T pat(size_t i) { return (T)(0xA5C3u ^ (i * 2654435761u >> 7)); }
    Region(size_t n_, uint32_t lane_) : n(n_), lane(lane_) { v = (T *)malloc(total() * sizeof(T) + !total()); for (size_t i = 0; i < total(); i++) v[i] = pat(i); }
    ~Region() { free(v); }
    size_t total() const { return STRIPED ? n * 64 : n; }
    std::conditional_t<STRIPED, Stripe<T>, Flat<T>> acc() const { if constexpr (STRIPED) return Stripe<T>{v, lane}; else return Flat<T>{v}; }
    bool clean() const { if (STRIPED) for (size_t i = 0; i < total(); i++) if (i % 64 != lane && v[i] != pat(i)) return false; return true; }
};
// backward bit reader, from the RFC's words (4.1): the last byte's highest set bit closes the stream, bits below bit 0 read as zero
struct BackR {
    const uint8_t *p; int64_t pos;
    bool init(const uint8_t *q, uint32_t n) { if (!n || !q[n - 1]) return false; p = q; pos = (int64_t)n * 8 - (8 - highbit(q[n - 1])); return true; }
    uint32_t read(uint32_t nb) { uint32_t v = 0; for (uint32_t i = 0; i < nb; i++) { const int64_t b = pos - 1 - i; v = (v << 1) | (b >= 0 ? (p[b >> 3] >> (b & 7)) & 1u : 0u); } pos -= nb; return v; }
};
static std::vector<uint8_t> unhex(const char *s) {
    std::vector<uint8_t> o;
    if (s[0] == '-') return o;
    for (; s[0] && s[1]; s += 2) { char b[3] = {s[0], s[1], 0}; o.push_back((uint8_t)strtoul(b, nullptr, 16)); }
    return o;
}
// the description as a heap block of its exact size (a read past it is the sanitizer's)
struct Bytes { uint8_t *p; uint32_t n; Bytes(const std::vector<uint8_t> &v) : n((uint32_t)v.size()) { p = (uint8_t *)malloc(n + !n); if (n) memcpy(p, v.data(), n); } ~Bytes() { free(p); } };

template <class Bits, bool ST>
static void counts(uint32_t lane, int max_log, int max_sym, int cap, const Bytes &d) {
    Region<int16_t, ST> norm((size_t)cap, lane);
    int nsym = 0, log = 0; uint32_t used = 0;
    const int rc = read_ncount<Bits>(d.p, d.n, norm.acc(), max_log, max_sym, cap, &nsym, &log, &used);
    printf("%d %d", rc, (int)norm.clean());
    if (!rc) { printf(" %d %u %d", log, used, nsym); for (int i = 0; i < nsym; i++) printf(" %d", norm.acc().get(i)); }
    printf("\n");
}
// spread + cells of one table: "pos clean" and per cell "symbol nbits next base bits" (base, bits: -1 where the symbol is out of the kind's range)
template <bool ST>
static void table(uint32_t lane, int kind, int log, const std::vector<int> &c) {
    const int nsym = (int)c.size();
    Region<int16_t, ST> norm((size_t)nsym, lane);
    Region<uint16_t, ST> next((size_t)nsym, lane);
    Region<uint8_t, ST> sym((size_t)1 << log, lane);
    for (int i = 0; i < nsym; i++) norm.acc().set(i, c[i]);
    const auto sa = sym.acc();
    const int pos = fse_spread(norm.acc(), next.acc(), nsym, log, [&](uint32_t u, uint32_t s) { sa.set(u, (int)s); });
    printf("%d %d", pos, (int)(norm.clean() && next.clean() && sym.clean()));
    for (int u = 0; pos == 0 && u < (1 << log); u++) {
        const uint32_t s = (uint32_t)sa.get(u);
        const FseCell e = fse_cell(fse_take_state(next.acc(), s), (uint32_t)log);
        if (sym_in_range(kind, s)) { const SymValue v = sym_value(kind, s); printf(" %u %u %u %u %u", s, e.nbits, e.next, v.base, v.bits); }
        else printf(" %u %u %u -1 -1", s, e.nbits, e.next);
    }
    printf("\n");
}
// what the device callers do with the walk, kept to its observable part: the events, and which wanted kinds are in Repeat_Mode
struct Walk {
    std::string ev; uint32_t want, miss; const uint8_t *q;
    bool wanted(int k) const { return (want >> k) & 1; }
    int predefined(int k) { ev += " P" + std::to_string(k); return 0; }
    int rle(int k, uint32_t s) { ev += " R" + std::to_string(k) + ":" + std::to_string(s); return wanted(k) && !sym_in_range(k, s) ? E_CORRUPT : 0; }
    int described(int k, const uint8_t *d, uint32_t n, uint32_t *used) {
        std::vector<int16_t> norm(256);
        int nsym = 0, log = 0;
        const int rc = read_ncount<FwdR>(d, n, Flat<int16_t>{norm.data()}, KIND[k].max_log, KIND[k].max_sym, 256, &nsym, &log, used);
        ev += " D" + std::to_string(k) + ":" + std::to_string(d - q) + ":" + std::to_string(n) + ":" + std::to_string(rc) + ":" + std::to_string(rc ? 0 : log);
        return rc;
    }
    int repeat(int k) { ev += " U" + std::to_string(k); if (wanted(k)) miss |= 1u << k; return 0; }
};
static void header(uint32_t want, const Bytes &d) {
    Walk cb{"", want, 0, d.p};
    uint32_t nseq = 0, at = 0;
    const int rc = seq_header(d.p, d.n, &nseq, &at, cb);
    if (rc) printf("%d%s\n", rc, cb.ev.c_str()); else printf("0 %u %u %u%s\n", nseq, at, cb.miss, cb.ev.c_str());
}
// a Huffman tree description the way huf_read_tree / bx_read_weights compose the rules
template <class Bits, bool ST>
static void tree(uint32_t lane, int cap, const Bytes &d) {
    Region<uint8_t, ST> weights(256, lane);
    Region<uint16_t, ST> rank(16, lane);
    const auto w = weights.acc();
    uint32_t nw = 0, used = 0, maxbits = 0, lastw = 0;
    bool clean = true;
    const int rc = [&]() -> int {
        if (d.n < 1) return E_TRUNC;
        const uint32_t hb = d.p[0];
        if (hb >= 128) { const int r = huf_direct_weights(d.p, d.n, w, &nw, &used); if (r) return r; }
        else {
            if (hb == 0 || 1 + hb > d.n) return E_TRUNC;
            Region<int16_t, ST> norm((size_t)cap, lane);
            int nsym = 0, log = 0; uint32_t hdr = 0;
            int r = read_ncount<Bits>(d.p + 1, hb, norm.acc(), 6, 255, cap, &nsym, &log, &hdr);
            clean = clean && norm.clean();
            if (r) return r;
            Region<uint16_t, ST> next((size_t)nsym, lane), ts((size_t)1 << log, lane), tb((size_t)1 << log, lane), tn((size_t)1 << log, lane);
            const auto sa = ts.acc(), ba = tb.acc(), na = tn.acc();
            if (fse_spread(norm.acc(), next.acc(), nsym, log, [&](uint32_t u, uint32_t s) { sa.set(u, (int)s); }) != 0) return E_CORRUPT;
            for (uint32_t u = 0; u < (1u << log); u++) { const FseCell e = fse_cell(fse_take_state(next.acc(), (uint32_t)sa.get(u)), (uint32_t)log); ba.set(u, (int)e.nbits); na.set(u, (int)e.next); }
            clean = clean && norm.clean() && next.clean() && ts.clean() && tb.clean() && tn.clean();
            if (hdr >= hb) return E_CORRUPT;
            BackR b;
            if (!b.init(d.p + 1 + hdr, hb - hdr)) return E_CORRUPT;
            const auto cell = [&](uint32_t s) { return HufCell{(uint32_t)sa.get(s), (uint32_t)ba.get(s), (uint32_t)na.get(s)}; };
            // (the batch caller, whose scratch holds 64 counts, fetches the other state's cell early; the serial ones do not)
            r = cap == 64 ? huf_walk_weights<true>(b, (uint32_t)log, cell, w, &nw) : huf_walk_weights<false>(b, (uint32_t)log, cell, w, &nw);
            if (r) return r;
            used = 1 + hb;
        }
        int r = huf_limits(w, nw, &maxbits, &lastw);
        if (r) return r;
        w.set(nw, (int)lastw);
        return huf_rank_starts(w, nw + 1, maxbits, rank.acc());
    }();
    printf("%d %d", rc, (int)(clean && weights.clean() && rank.clean()));
    if (!rc) {
        printf(" %u %u %u", used, maxbits, nw + 1);
        for (uint32_t i = 0; i <= nw; i++) printf(" %d", w.get(i));
        for (uint32_t b = 1; b <= maxbits; b++) printf(" %d", rank.acc().get(b));
    }
    printf("\n");
}
template <bool ST>
static void predefined(uint32_t lane, int kind) {  // as init_fused_tables and fse_build_predefined build them
    std::vector<int> c(default_norm(kind), default_norm(kind) + default_nsym(kind));
    table<ST>(lane, kind, KIND[kind].def_log, c);
}

int main() {
    char cmd[8], shape[8], rd[8], hex[1 << 12];
    int lane;
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] == 'K') {  // the constants
            for (int k = 0; k < 3; k++) printf("%d %d %d %d %d ", KIND[k].mode_shift, KIND[k].max_log, KIND[k].max_sym, KIND[k].def_log, default_nsym(k));
            for (volatile int k = 0; k < 3; k = k + 1) printf("%u %d %d %d ", kind_mode_shift(k), kind_max_log(k), kind_max_sym(k), kind_def_log(k));  // the run-time selectors
            for (int k = 0; k < 3; k++) for (int i = 0; i < default_nsym(k); i++) printf("%d ", default_norm(k)[i]);
            for (int k = -1; k < 3; k++) for (uint32_t s = 0; s < 256; s++) printf("%d ", (int)sym_in_range(k, s));
            printf("\n");
            continue;
        }
        if (scanf("%7s %d", shape, &lane) != 2) return 2;
        const bool st = shape[0] == 'S';
        if (cmd[0] == 'N' || cmd[0] == 'H') {
            int max_log = 0, max_sym = 0, cap = 0;
            if (scanf("%7s", rd) != 1) return 2;
            if (cmd[0] == 'N' && scanf("%d %d", &max_log, &max_sym) != 2) return 2;
            if (scanf("%d %4095s", &cap, hex) != 2) return 2;
            const Bytes d(unhex(hex));
            const bool w = rd[0] == 'W';
            if (cmd[0] == 'N') {
                if (st) { if (w) counts<FwdW, true>(lane, max_log, max_sym, cap, d); else counts<FwdR, true>(lane, max_log, max_sym, cap, d); }
                else { if (w) counts<FwdW, false>(lane, max_log, max_sym, cap, d); else counts<FwdR, false>(lane, max_log, max_sym, cap, d); }
            } else {
                if (st) { if (w) tree<FwdW, true>(lane, cap, d); else tree<FwdR, true>(lane, cap, d); }
                else { if (w) tree<FwdW, false>(lane, cap, d); else tree<FwdR, false>(lane, cap, d); }
            }
        } else if (cmd[0] == 'T') {
            int kind, log, n;
            if (scanf("%d %d %d", &kind, &log, &n) != 3) return 2;
            std::vector<int> c((size_t)n);
            for (auto &x : c) if (scanf("%d", &x) != 1) return 2;
            if (st) table<true>(lane, kind, log, c); else table<false>(lane, kind, log, c);
        } else if (cmd[0] == 'D') {
            int kind;
            if (scanf("%d", &kind) != 1) return 2;
            if (st) predefined<true>(lane, kind); else predefined<false>(lane, kind);
        } else if (cmd[0] == 'S') {  // (the walk has no storage: shape and lane carry the want mask)
            if (scanf("%4095s", hex) != 1) return 2;
            header((uint32_t)lane, Bytes(unhex(hex)));
        } else return 2;
    }
    return 0;
}
"""

SHAPES = (("F", 0), ("S", 0), ("S", 31), ("S", 63))
KINDS = (("ll", 9, 35, 6), ("of", 8, 31, 5), ("ml", 9, 52, 6))      # name, Max_Accuracy_Log, largest code, log of the predefined table
SHIFT = (6, 4, 2)
HUF = (6, 255)                                                      # the table of the Huffman weights: log at most 6, any byte a symbol


def hx(b):
    return bytes(b).hex() or "-"


# ---- the model: RFC 8878, restated ------------------------------------------------------------------------------------------

def m_counts(d, max_log, max_sym, cap):
    """4.1.1: 4 bits of accuracy log - 5; then values of variable width until the probabilities sum to 1 << log: a value of
    0..remaining + 1 in highbit(remaining + 1) + 1 bits, the lowest values one bit shorter; value - 1 is the probability (-1 "less
    than 1" takes one cell); a zero is followed by 2-bit repeat counts, 3 meaning another one follows.  The decoder stops storing at
    max_sym + 1 symbols; a symbol the storage cannot hold (index >= cap) is unsupported; bits past the description read as zero
    and make it truncated in the end."""
    if not d:
        return (E_TRUNC,)
    bits, pos = int.from_bytes(d, "little"), 0

    def rd(n):
        nonlocal pos
        pos += n
        return (bits >> (pos - n)) & ((1 << n) - 1)
    log = 5 + rd(4)
    if log > max_log:
        return (E_CORRUPT,)
    remaining, c = 1 << log, []
    while remaining > 0 and len(c) <= max_sym:
        n = (remaining + 1).bit_length()
        short = (1 << n) - 1 - (remaining + 1)                       # this many values fit n - 1 bits
        v = (bits >> pos) & ((1 << (n - 1)) - 1)
        if v < short:
            pos += n - 1
        else:
            v = rd(n)
            if v >= 1 << (n - 1):
                v -= short
        remaining -= abs(v - 1)
        if len(c) >= cap:
            return (E_UNSUP,)
        c.append(v - 1)
        if v - 1 == 0:
            while True:
                r = rd(2)
                for _ in range(r):
                    if len(c) <= max_sym:
                        if len(c) >= cap:
                            return (E_UNSUP,)
                        c.append(0)
                if r != 3:
                    break
    if remaining != 0:
        return (E_CORRUPT,)
    used = (pos + 7) // 8
    if used > len(d):
        return (E_TRUNC,)
    return (0, log, used, len(c), *c)


def m_table(norm, log):
    """4.1.1: "less than 1" symbols take the last cells, one each, in symbol order downwards; the others are spread from cell 0 in
    steps of (size >> 1) + (size >> 3) + 3, skipping those last cells; then cell by cell in ascending order a symbol's cells get the
    state counters count, count + 1, ...: nbits = log - highbit(counter), next-state base = (counter << nbits) - size."""
    size = 1 << log
    cell, high, cnt = [None] * size, size, {}
    for s, p in enumerate(norm):
        if p == -1:
            high -= 1
            cell[high] = s
            cnt[s] = 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, p in enumerate(norm):
        for _ in range(max(p, 0)):
            cell[pos] = s
            pos = (pos + step) % size
            while pos >= high:
                pos = (pos + step) % size
        if p > 0:
            cnt[s] = p
    out = []
    for s in cell:
        nb = log - (cnt[s].bit_length() - 1)
        out.append((s, nb, (cnt[s] << nb) - size))
        cnt[s] += 1
    return pos, out


def m_value(kind, s):
    """3.1.1.3.2.1.1: literal-length and match-length codes by table, offset code N = N extra bits on 1 << N; None past the range."""
    if kind < 0:
        return (s, 0)
    if s > KINDS[kind][2]:
        return None
    return (Z.LL_BASE[s], Z.LL_BITS[s]) if kind == 0 else ((1 << s, s) if kind == 1 else (Z.ML_BASE[s], Z.ML_BITS[s]))


def m_header(d, want):
    """3.1.1.3.2.1: the count in 1, 2 or 3 bytes; nothing follows a count of 0; then the modes byte (LL bits 7-6, OF 5-4, ML 3-2, the
    low two reserved: must be zero) and per kind nothing (predefined, repeat), one byte (RLE) or a description."""
    n = len(d)
    if n < 1:
        return (E_TRUNC, [])
    b0 = d[0]
    if b0 < 128:
        nseq, p = b0, 1
    elif b0 < 255:
        if n < 2:
            return (E_TRUNC, [])
        nseq, p = ((b0 - 128) << 8) + d[1], 2
    else:
        if n < 3:
            return (E_TRUNC, [])
        nseq, p = d[1] + (d[2] << 8) + 0x7F00, 3
    if nseq == 0:
        return (0, nseq, p, 0, [])
    if p >= n:
        return (E_TRUNC, [])
    modes = d[p]
    p += 1
    if modes & 3:
        return (E_CORRUPT, [])
    ev, miss = [], 0
    for k in range(3):
        mode = (modes >> SHIFT[k]) & 3
        if mode == 0:
            ev.append(f"P{k}")
        elif mode == 1:
            if p >= n:
                return (E_TRUNC, ev)
            ev.append(f"R{k}:{d[p]}")
            if (want >> k) & 1 and d[p] > KINDS[k][2]:
                return (E_CORRUPT, ev)
            p += 1
        elif mode == 2:
            r = m_counts(d[p:], KINDS[k][1], KINDS[k][2], 256)
            ev.append(f"D{k}:{p}:{n - p}:{r[0]}:{0 if r[0] else r[1]}")
            if r[0]:
                return (r[0], ev)
            p += r[2]
        else:
            ev.append(f"U{k}")
            miss |= ((want >> k) & 1) << k
    return (0, nseq, p, miss, ev)


def m_back(d):
    """4.1: a backward stream: the highest set bit of the last byte closes it; read from there downwards, most significant bit first."""
    if not d or d[-1] == 0:
        return None
    bits, pos = int.from_bytes(d, "little"), len(d) * 8 - (8 - (d[-1].bit_length() - 1))

    def rd(n):
        nonlocal pos
        pos -= n
        return ((bits << -pos) if pos < 0 else (bits >> pos)) & ((1 << n) - 1)       # below bit 0: zeros
    return rd, lambda: pos


def m_tree(d, cap):
    """4.2.1: a header byte; >= 128: header - 127 weights of 4 bits each; below: that many bytes of FSE-compressed weights (a table
    of log <= 6, two states taking turns until the stream is used up: then the other state's symbol is the last).  At most 255
    weights; weights up to 12; they sum (2^(w - 1)) to a total whose distance to the next power of two is itself a power of two: the
    last symbol's weight; codes of at most 11 bits.  Cells of the table go to the longest codes first."""
    n = len(d)
    if n < 1:
        return (E_TRUNC,)
    hb = d[0]
    if hb >= 128:
        nw = hb - 127
        used = 1 + (nw + 1) // 2
        if used > n:
            return (E_TRUNC,)
        w = [(d[1 + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(nw)]
    else:
        if hb == 0 or 1 + hb > n:
            return (E_TRUNC,)
        r = m_counts(d[1:1 + hb], 6, 255, cap)
        if r[0]:
            return (r[0],)
        log, hdr = r[1], r[2]
        pos, t = m_table(list(r[4:]), log)
        assert pos == 0
        if hdr >= hb:
            return (E_CORRUPT,)
        b = m_back(d[1 + hdr:1 + hb])
        if b is None:
            return (E_CORRUPT,)
        rd, left = b
        st, w, i = [rd(log), rd(log)], [], 0
        while True:
            if len(w) >= 255:
                return (E_CORRUPT,)
            s, nb, nx = t[st[i]]
            w.append(s)
            st[i] = nx + rd(nb)
            if left() < 0:
                if len(w) >= 255:
                    return (E_CORRUPT,)
                w.append(t[st[i ^ 1]][0])
                break
            i ^= 1
        used = 1 + hb
    if any(x > 12 for x in w):
        return (E_CORRUPT,)
    total = sum(1 << (x - 1) for x in w if x)
    if total == 0:
        return (E_CORRUPT,)
    maxbits = total.bit_length()
    rest = (1 << maxbits) - total
    if maxbits > 11 or rest & (rest - 1):
        return (E_CORRUPT,)
    w.append(rest.bit_length())
    start, ranks = 0, {}
    for bits in range(maxbits, 0, -1):
        ranks[bits] = start
        start += sum(1 for x in w if x and maxbits + 1 - x == bits) << (maxbits - bits)
    assert start == 1 << maxbits
    return (0, used, maxbits, len(w), *w, *[ranks[b] for b in range(1, maxbits + 1)])


# ---- the cases --------------------------------------------------------------------------------------------------------------

def count_tables():
    """(kind index or -1 for the Huffman weights, max_log, max_sym, log, norm): valid tables, the smallest that reach each rule."""
    out = []
    for k, (lim_log, lim_sym) in [(i, (K[1], K[2])) for i, K in enumerate(KINDS)] + [(-1, HUF)]:
        top = min(lim_sym, 40)
        for log in range(5, lim_log + 1):
            out.append((k, lim_log, lim_sym, log, Z.spread_norm(range(0, 12), log)))                          # even counts
            out.append((k, lim_log, lim_sym, log, Z.spread_norm([0], log, low=range(1, 20))))                 # mostly "less than 1"
            out.append((k, lim_log, lim_sym, log, Z.spread_norm([0, 4, 9, 16, 24], log, low=(2, 25))))        # zero runs of 3, 4, 6, 7: rep == 3 once and twice
            out.append((k, lim_log, lim_sym, log, Z.spread_norm([3, top], log, low=(1,))))                    # a long run: several rep == 3 in a row
            out.append((k, lim_log, lim_sym, log, Z.spread_norm([0, lim_sym if lim_sym < 64 else 63], log)))  # runs to max_sym exactly
    return out


def test_constants(program):
    v = [int(x) for x in run(program, "K\n")[0].split()]
    assert v[:15] == [x for k, K in enumerate(KINDS) for x in (SHIFT[k], K[1], K[2], K[3], len(Z.DEFAULTS[K[0]][0]))]
    assert v[15:27] == [x for k, K in enumerate(KINDS) for x in (SHIFT[k], K[1], K[2], K[3])]      # kind_mode_shift / _max_log / _max_sym / _def_log
    assert [Z.MAX_LOG[K[0]] for K in KINDS] == [K[1] for K in KINDS]
    v = v[27:]
    assert v[:118] == Z.LL_DEFAULT + Z.OF_DEFAULT + Z.ML_DEFAULT
    want = [1] * 256 + [int(s <= K[2]) for K in KINDS for s in range(256)]
    assert v[118:] == want


def run(program, text):
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-3000:])
    return r.stdout.splitlines()


def check(program, cases):
    """cases: [(command line, expected fields)] -> one process; fields compared one by one behind "rc clean"."""
    lines = run(program, "".join(c + "\n" for c, _ in cases))
    assert len(lines) == len(cases)
    for (c, want), got in zip(cases, lines):
        g = got.split()
        assert g[1] == "1", ("a stripe of another lane was written", c)
        assert [int(g[0])] + [int(x) for x in g[2:]] == list(want), (c[:200], "got", got[:300], "want", want[:40])


def test_counts(program):
    cases, n_desc = [], 0

    def add(d, max_log, max_sym, caps=(256,)):
        nonlocal n_desc
        n_desc += 1
        for cap in caps:
            want = m_counts(d, max_log, max_sym, cap)
            for rd in "RW":
                for sh, lane in SHAPES:
                    cases.append((f"N {sh} {lane} {rd} {max_log} {max_sym} {cap} {hx(d)}", want))
    rng = random.Random(8878)
    for k, max_log, max_sym, log, norm in count_tables():
        d = Z.write_ncount(norm, log)
        got = m_counts(d, max_log, max_sym, 256)
        assert got == (0, log, len(d), len(norm), *norm), (norm, log)             # what the writer wrote reads back
        for cut in range(len(d) + 1):                                              # ... and truncated at every length
            add(d[:cut], max_log, max_sym)
        add(d + b"\xff", max_log, max_sym)                                         # bytes behind it are not its own
    for k, K in enumerate(KINDS):
        add(Z.write_ncount(Z.spread_norm([0, 1], K[1] + 1), K[1] + 1), K[1], K[2])   # one log above the kind's
        past = Z.write_ncount(Z.spread_norm([0, K[2] + 1], 6), 6)                     # one symbol past the alphabet
        assert m_counts(past, K[1], K[2], 256) == (E_CORRUPT,)
        add(past, K[1], K[2])
    add(Z.write_ncount(Z.spread_norm([0, 1], 7), 7), *HUF)
    for last in (62, 63, 64):                                                      # 63, 64, 65 symbols under a cap of 64 and of 256
        d = Z.write_ncount(Z.spread_norm([0, last], 6), 6)
        assert m_counts(d, *HUF, 64)[0] == (E_UNSUP if last == 64 else 0) and m_counts(d, *HUF, 256)[0] == 0
        for cut in range(len(d) + 1):
            add(d[:cut], *HUF, caps=(64, 256))
        if last < 64:                                                              # the same, reached through "less than 1" symbols
            add(Z.write_ncount(Z.spread_norm([0], 6, low=range(1, last + 1)), 6), *HUF, caps=(64, 256))
    for _ in range(400):                                                           # seeded random byte strings
        d = bytes(rng.randrange(256) for _ in range(rng.randrange(1, 24)))
        k = rng.randrange(4)
        add(d, *((KINDS[k][1], KINDS[k][2]) if k < 3 else HUF), caps=(64, 256))
    assert {c[1][0] for c in cases} == {0, E_CORRUPT, E_UNSUP}
    check(program, cases)
    print(f"counts: {n_desc} descriptions, {len(cases)} runs")


def test_tables(program):
    cases = []
    for k, max_log, max_sym, log, norm in count_tables():
        pos, cells = m_table(norm, log)
        assert pos == 0
        t = Z.FseTable(norm, log)                                                 # the writer's table: the second source
        assert [(s, nb, nx) for s, nb, nx in cells] == list(zip(t.symbol, t.nbits, t.base))
        for kind in {k, -1}:
            want = [0]
            for s, nb, nx in cells:
                v = m_value(kind, s)
                want += [s, nb, nx, *(v if v else (-1, -1))]
            for sh, lane in SHAPES:
                cases.append((f"T {sh} {lane} {kind} {log} {len(norm)} " + " ".join(map(str, norm)), want))
    check(program, cases)
    print(f"tables: {len(cases)} runs")


# next, nbits, extra bits, base of every cell of the predefined LL, OF, ML tables, as the parent's host_fse_build (fused_small.hip
# before the rules were shared) produced them
PARENT_PREDEFINED = (
    "0 4 0 0 16 4 0 0 32 5 0 1 0 5 0 3 0 5 0 4 0 5 0 6 0 5 0 7 0 5 0 9 0 5 0 10 0 5 0 12 0 6 0 14 0 5 1 16 0 5 1 20 0 5 1 22 0 5 2 "
    "28 0 5 3 32 0 5 4 48 32 5 6 64 0 5 7 128 0 6 8 256 0 6 10 1024 0 6 12 4096 32 4 0 0 0 4 0 1 0 5 0 2 32 5 0 4 0 5 0 5 32 5 0 7 0 "
    "5 0 8 32 5 0 10 0 5 0 11 0 6 0 13 32 5 1 16 0 5 1 18 32 5 1 22 0 5 2 24 32 5 3 32 0 5 3 40 0 4 6 64 16 4 6 64 32 5 7 128 0 6 9 "
    "512 0 6 11 2048 48 4 0 0 16 4 0 1 32 5 0 2 32 5 0 3 32 5 0 5 32 5 0 6 32 5 0 8 32 5 0 9 32 5 0 11 32 5 0 12 0 6 0 15 32 5 1 18 "
    "32 5 1 20 32 5 2 24 32 5 2 28 32 5 3 40 32 5 4 48 0 6 16 65536 0 6 15 32768 0 6 14 16384 0 6 13 8192",
    "0 5 0 1 0 4 6 64 0 5 9 512 0 5 15 32768 0 5 21 2097152 0 5 3 8 0 4 7 128 0 5 12 4096 0 5 18 262144 0 5 23 8388608 0 5 5 32 0 4 "
    "8 256 0 5 14 16384 0 5 20 1048576 0 5 2 4 16 4 7 128 0 5 11 2048 0 5 17 131072 0 5 22 4194304 0 5 4 16 16 4 8 256 0 5 13 8192 0 "
    "5 19 524288 0 5 1 2 16 4 6 64 0 5 10 1024 0 5 16 65536 0 5 28 268435456 0 5 27 134217728 0 5 26 67108864 0 5 25 33554432 0 5 24 "
    "16777216",
    "0 6 0 3 0 4 0 4 32 5 0 5 0 5 0 6 0 5 0 8 0 5 0 9 0 5 0 11 0 6 0 13 0 6 0 16 0 6 0 19 0 6 0 22 0 6 0 25 0 6 0 28 0 6 0 31 0 6 0 "
    "34 0 6 1 37 0 6 1 41 0 6 2 47 0 6 3 59 0 6 4 83 0 6 7 131 0 6 9 515 16 4 0 4 0 4 0 5 32 5 0 6 0 5 0 7 32 5 0 9 0 5 0 10 0 6 0 "
    "12 0 6 0 15 0 6 0 18 0 6 0 21 0 6 0 24 0 6 0 27 0 6 0 30 0 6 0 33 0 6 1 35 0 6 1 39 0 6 2 43 0 6 3 51 0 6 4 67 0 6 5 99 0 6 8 "
    "259 32 4 0 4 48 4 0 4 16 4 0 5 32 5 0 7 32 5 0 8 32 5 0 10 32 5 0 11 0 6 0 14 0 6 0 17 0 6 0 20 0 6 0 23 0 6 0 26 0 6 0 29 0 6 "
    "0 32 0 6 16 65539 0 6 15 32771 0 6 14 16387 0 6 13 8195 0 6 12 4099 0 6 11 2051 0 6 10 1027")


def test_predefined_tables(program):
    lines = run(program, "".join(f"D {sh} {lane} {k}\n" for k in range(3) for sh, lane in SHAPES))
    for k in range(3):
        parent = [int(x) for x in PARENT_PREDEFINED[k].split()]
        norm, log = Z.DEFAULTS[KINDS[k][0]]
        assert len(parent) == 4 << log
        pos, cells = m_table(norm, log)
        for j in range(len(SHAPES)):
            g = [int(x) for x in lines[k * len(SHAPES) + j].split()]
            assert g[:2] == [0, 1]
            rows = [g[2 + 5 * i:7 + 5 * i] for i in range(1 << log)]              # symbol nbits next base bits
            assert [x for s, nb, nx, base, bits in rows for x in (nx, nb, bits, base)] == parent, KINDS[k][0]
            assert [tuple(r) for r in rows] == [(s, nb, nx, *m_value(k, s)) for s, nb, nx in cells], KINDS[k][0]


def small_desc(k, log=5):
    return Z.write_ncount(Z.spread_norm([0, 1, 2], log), log)


def test_sequences_header(program):
    heads = []
    for n in (0, 127):
        heads.append(Z._nseq(n, 1))
    for n in (128, 0x7EFF):
        heads.append(Z._nseq(n, 2))
    for n in (0x7F00, 0xFFFF + 0x7F00):
        heads.append(Z._nseq(n, 3))
    heads += [Z._nseq(0, 2), Z._nseq(5, 2)]                                        # a count need not use its shortest form
    assert [m_header(h + b"\x00\x80", 7)[1] for h in heads] == [0, 127, 128, 0x7EFF, 0x7F00, 0xFFFF + 0x7F00, 0, 5]
    sections = []
    for h in heads:                                                                # the count forms, cut behind every byte
        full = h + bytes([0]) + b"\x80"
        sections += [full[:c] for c in range(len(full) + 1)]
    for low in (1, 2, 3):                                                          # the reserved bits
        sections.append(b"\x01" + bytes([low]) + b"\x80")
    payload = lambda k, mode: (b"", bytes([3]), small_desc(k), b"")[mode]
    for modes in range(64):                                                        # all 4^3 combinations
        m = [(modes >> 4) & 3, (modes >> 2) & 3, modes & 3]
        sec = b"\x02" + bytes([modes << 2]) + b"".join(payload(k, m[k]) for k in range(3)) + b"\x80"
        sections.append(sec)
        if modes in (0b011001, 0b101010, 0b100110):                               # truncation behind each field
            sections += [sec[:c] for c in range(len(sec))]
    for k, K in enumerate(KINDS):                                                  # an RLE symbol at and above each kind's limit
        for s in (K[2], K[2] + 1, 255):
            sections.append(b"\x01" + bytes([1 << SHIFT[k], s]) + b"\x80")
    sections.append(b"\x01" + bytes([2 << 6]) + Z.write_ncount(Z.spread_norm([0, 1], 10), 10))   # a description that fails
    cases = [(f"S W {want} {hx(sec)}", sec, want) for sec in sections for want in range(8)]
    lines = run(program, "".join(c + "\n" for c, _, _ in cases))
    assert len(lines) == len(cases)
    seen = set()
    for (c, sec, want), got in zip(cases, lines):
        w = m_header(sec, want)
        exp = " ".join(map(str, w[:-1] + tuple(w[-1])))
        assert got.strip() == exp, (c, got, exp)
        seen |= {e[0] for e in w[-1]} | {w[0]}
    assert seen == {0, E_CORRUPT, "P", "R", "D", "U"}
    # the writer's sections read back: count, where the bitstream starts, the modes it chose
    for choice, mode in (("pre", 0), ("rle", 1), (("fse", Z.spread_norm([0, 1, 2], 5), 5), 2)):
        st = Z._State()
        descs = [Z._table(kind, choice, [0, 1, 2], st) for kind in ("ll", "of", "ml")]
        sec = Z._nseq(9, None) + bytes([sum(d[0] << SHIFT[k] for k, d in enumerate(descs))]) + b"".join(d[1] for d in descs)
        w = m_header(sec + b"\x80", 7)
        assert w[:4] == (0, 9, len(sec), 0) and [e[0] for e in w[4]] == ["PRD"[mode]] * 3
    print(f"sequences header: {len(sections)} sections, {len(cases)} runs")


def fse_weights(ws, last):
    """A description of the weights ws (+ the implied last one) in the FSE form, by the writer."""
    return Z.HufTree(list(ws) + [last], check=False).describe("fse")


def test_huffman(program):
    descs = []
    direct = lambda ws: bytes([127 + len(ws)]) + bytes(((ws + [0])[i] << 4) | (ws + [0])[i + 1] for i in range(0, len(ws), 2))
    for ws in ([1], [1, 1], [1] * 127, [1] * 128):                                 # direct weights of 1, 2, 127 and 128 entries
        descs.append(direct(ws))
    descs += [direct([12]), direct([13]), direct([15, 1]),                         # a weight of 12 (its code would have 12 bits) and of 13
              direct([0]), direct([0, 0]),                                         # total zero
              direct([11]), direct([11, 11]),                                      # max bits 11 and 12
              direct([3, 1]), direct([2, 2, 1])]                                   # a remainder that is not a power of two
    assert [m_tree(d, 256)[0] for d in descs[4:]] == [E_CORRUPT] * 5 + [0] + [E_CORRUPT] * 3
    def mix(n):                                                                    # 192 ones among n: total + 64 is a power of two, the last weight is 7
        w = [1, 1, 1, 0] * 64
        for i in (255, 3)[:256 - n]:
            w.pop(i)
        return w
    # an even and an odd number of weights (the stream ends on the first / the second state); 254, 255 and 256 of them
    for ws, last in (([1, 1, 2, 3, 2, 2], 3), ([2, 1, 1, 2, 3, 1, 1], 3), (mix(254), 7), (mix(255), 7), (mix(256), 7)):
        n = len(ws)
        d = fse_weights(ws, last)
        r = m_tree(d, 256)
        assert r[0] == (E_CORRUPT if n == 256 else 0), n
        if n < 256:
            assert r[3] == n + 1 and list(r[4:4 + n + 1]) == ws + [last]              # what the writer wrote reads back
            tree = Z.HufTree(ws + [last])
            firsts = {}
            for s in sorted(tree.code):                                            # the writer's codes: the first cell of every length
                code, bits = tree.code[s]
                firsts.setdefault(bits, code << (tree.max_bits - bits))
            assert all(r[4 + n + 1 + b - 1] == firsts[b] for b in firsts)
        descs.append(d)
    framed = lambda body: bytes([len(body)]) + body
    for syms in ((12, 13), (13, 20)):                                              # weight symbols 13 and 20 (one caller keeps 4 bits of a symbol)
        t = Z.FseTable(Z.spread_norm(syms, 5), 5)
        descs.append(framed(Z.write_ncount(t.norm, 5) + Z.backward_stream([(t.states_of(syms[0])[0], 5), (t.states_of(syms[1])[0], 5)])))
    descs.append(framed(Z.write_ncount(Z.spread_norm([1, 2], 5), 5)))              # counts that use up the section: no stream behind them
    d65 = Z.write_ncount(Z.spread_norm([1, 64], 6), 6)                             # a weight table of 65 symbols: beyond a lane's scratch
    descs.append(framed(d65 + b"\x01"))
    rng = random.Random(421)
    for _ in range(300):
        n = rng.randrange(1, 20)
        descs.append(bytes([rng.choice((n - 1, rng.randrange(128, 140)))]) + bytes(rng.randrange(256) for _ in range(n - 1)))
    cases = []
    for d in descs:
        for cut in ([len(d)] if len(d) > 40 else range(len(d) + 1)):               # every description truncated at every length (the long ones whole)
            for cap in (64, 256):
                want = m_tree(d[:cut], cap)
                for rd in "RW":
                    for sh, lane in SHAPES:
                        cases.append((f"H {sh} {lane} {rd} {cap} {hx(d[:cut])}", want))
    assert {c[1][0] for c in cases} == {0, E_CORRUPT, E_UNSUP}
    check(program, cases)
    print(f"huffman: {len(descs)} descriptions, {len(cases)} runs")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("zstd_rules")
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "rules"
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, str(main), "-o", str(exe)], check=True)
    return str(exe)
