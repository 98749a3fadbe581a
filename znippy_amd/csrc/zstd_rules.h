// The table-description rules of RFC 8878, each stated once: the per-kind constants and code tables, Number_of_Sequences and
// the Symbol_Compression_Modes walk, the FSE normalised counts (4.1.1), the spread of symbols over table cells and a cell's
// nbits / next state, what a sequence symbol means, and the Huffman tree description (4.2.1).  This is what decides what a
// foreign frame may do to LDS; every decoder (zstd_dev.h, zstd_decode.hip, zstd_batch.hip, fused_small.hip's predefined
// tables) calls these bodies and keeps only its own storage and its own parallel algorithm.
// Plain C++: no HIP builtin, no include of the HIP runtime — the qualifiers sit behind ZR_FN, so a host compiler reads the
// same text (tests/test_zstd_rules_cpu.py runs every function under ASan and UBSan against a model).  Storage comes in as
// small accessor objects (get / set by index: Flat for an array, Stripe for a lane's [i * 64 + lane] entries of a wave's
// scratch), the bit reader as a template parameter; everything is forced inline, so an accessor costs its address arithmetic.
#pragma once
#include <stdint.h>

#ifndef ZR_FN
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZR_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define ZR_FN inline __attribute__((always_inline))
#endif
#endif

namespace zr {

constexpr int E_TRUNC = -5, E_CORRUPT = -5, E_UNSUP = -6;

// the three sequence tables, in the order of the modes byte
enum { K_LL = 0, K_OF = 1, K_ML = 2 };
struct KindRule { uint8_t mode_shift, max_log, max_sym, def_log; };  // bits of the modes byte, Max_Accuracy_Log, largest code, log of the predefined table
constexpr KindRule KIND[3] = {{6, 9, 35, 6}, {4, 8, 31, 5}, {2, 9, 52, 6}};
// KIND[kind].field for a kind known only at run time, as selects between immediates (no load from constant memory)
#define ZR_KIND_FIELD(kind, f) ((kind) == K_LL ? KIND[K_LL].f : ((kind) == K_OF ? KIND[K_OF].f : KIND[K_ML].f))
ZR_FN uint32_t kind_mode_shift(int kind) { return ZR_KIND_FIELD(kind, mode_shift); }
ZR_FN int kind_max_log(int kind) { return ZR_KIND_FIELD(kind, max_log); }
ZR_FN int kind_max_sym(int kind) { return ZR_KIND_FIELD(kind, max_sym); }
ZR_FN int kind_def_log(int kind) { return ZR_KIND_FIELD(kind, def_log); }
#undef ZR_KIND_FIELD

// literal-length / match-length codes: value baseline and extra bits (3.1.1.3.2.1.1); predefined distributions (3.1.1.3.2.2)
constexpr uint32_t LL_BASE[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18,
                                  20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048,
                                  4096, 8192, 16384, 32768, 65536};
constexpr uint8_t LL_BITS[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1,
                                 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
constexpr uint32_t ML_BASE[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20,
                                  21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 37,
                                  39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051,
                                  4099, 8195, 16387, 32771, 65539};
constexpr uint8_t ML_BITS[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1,
                                 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11,
                                 12, 13, 14, 15, 16};
constexpr int8_t LL_DEFAULT[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                   2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
constexpr int8_t ML_DEFAULT[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                   1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                   1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
constexpr int8_t OF_DEFAULT[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1,
                                   1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
ZR_FN const int8_t *default_norm(int kind) { return kind == K_LL ? LL_DEFAULT : (kind == K_OF ? OF_DEFAULT : ML_DEFAULT); }
ZR_FN int default_nsym(int kind) { return kind == K_LL ? 36 : (kind == K_OF ? 29 : 53); }

ZR_FN int highbit(uint32_t v) { return 31 - __builtin_clz(v); }  // v != 0

// ---- storage ----------------------------------------------------------------------------------------------------------
template <class T>
struct Flat {  // entry i of an array
    T *p;
    ZR_FN int get(uint32_t i) const { return (int)p[i]; }
    ZR_FN void set(uint32_t i, int v) const { p[i] = (T)v; }
};
template <class T>
struct Stripe {  // a lane's entry i of a wave's scratch: consecutive lanes, consecutive addresses
    T *p;
    uint32_t lane;
    ZR_FN int get(uint32_t i) const { return (int)p[i * 64 + lane]; }
    ZR_FN void set(uint32_t i, int v) const { p[i * 64 + lane] = (T)v; }
};

// ---- forward bit readers (FSE table descriptions); bytes past n read as zero ------------------------------------------------
struct FwdR {  // bit by bit: no state but the position
    const uint8_t *p;
    uint32_t n, bitpos;
    ZR_FN void init(const uint8_t *src, uint32_t len) { p = src; n = len; bitpos = 0; }
    ZR_FN uint32_t peek(uint32_t nb) const {
        uint32_t v = 0;
        for (uint32_t i = 0; i < nb; i++) {
            const uint32_t bp = bitpos + i;
            const uint32_t bit = (bp >> 3) < n ? (p[bp >> 3] >> (bp & 7)) & 1u : 0u;
            v |= bit << i;
        }
        return v;
    }
    ZR_FN uint32_t read(uint32_t nb) { const uint32_t v = peek(nb); bitpos += nb; return v; }
};
struct FwdW {  // with a 64-bit register window
    const uint8_t *p;
    uint32_t n, bitpos, wbit;
    uint64_t win;
    ZR_FN void fill(uint32_t byte) {
        uint64_t v = 0;
        if (byte + 8 <= n) __builtin_memcpy(&v, p + byte, 8);
        else for (uint32_t i = 0; i < 8 && byte + i < n; i++) v |= (uint64_t)p[byte + i] << (8 * i);
        win = v;
        wbit = byte * 8;
    }
    ZR_FN void init(const uint8_t *src, uint32_t len) { p = src; n = len; bitpos = 0; fill(0); }
    ZR_FN uint32_t peek(uint32_t nb) {  // nb <= 25
        if (bitpos + nb > wbit + 64) fill(bitpos >> 3);
        return (uint32_t)(win >> (bitpos - wbit)) & ((1u << nb) - 1u);
    }
    ZR_FN uint32_t read(uint32_t nb) { const uint32_t v = peek(nb); bitpos += nb; return v; }
};

// ---- FSE ----------------------------------------------------------------------------------------------------------------
// Normalised counts (4.1.1) of the description [src, src + n) -> norm[0 .. *nsym); -1 = "less than 1".  At most max_sym + 1
// symbols are read; a symbol at index `cap` or beyond (what the caller's storage holds) answers E_UNSUP.
template <class Bits, class Norm>
ZR_FN int read_ncount(const uint8_t *src, uint32_t n, Norm norm, int max_log, int max_sym, int cap, int *nsym, int *log, uint32_t *consumed) {
    Bits b;
    b.init(src, n);
    if (n == 0) return E_TRUNC;
    const int alog = 5 + (int)b.read(4);
    if (alog > max_log) return E_CORRUPT;
    int remaining = 1 << alog, s = 0;
    while (remaining > 0 && s <= max_sym) {
        const int bits = highbit((uint32_t)remaining + 1) + 1;
        uint32_t val = b.peek((uint32_t)bits);
        const uint32_t lower_mask = (1u << (bits - 1)) - 1, threshold = (1u << bits) - 1 - ((uint32_t)remaining + 1);
        if ((val & lower_mask) < threshold) { b.bitpos += (uint32_t)bits - 1; val &= lower_mask; }  // the small values take one bit less
        else { b.bitpos += (uint32_t)bits; if (val > lower_mask) val -= threshold; }
        const int proba = (int)val - 1;
        remaining -= proba < 0 ? -proba : proba;
        if (s >= cap) return E_UNSUP;
        norm.set((uint32_t)s++, proba);
        if (proba == 0) {
            uint32_t rep = b.read(2);
            for (;;) {
                for (uint32_t i = 0; i < rep && s <= max_sym; i++) { if (s >= cap) return E_UNSUP; norm.set((uint32_t)s++, 0); }
                if (rep == 3) rep = b.read(2); else break;
            }
        }
    }
    if (remaining != 0) return E_CORRUPT;
    if ((b.bitpos + 7) / 8 > n) return E_TRUNC;
    *nsym = s;
    *log = alog;
    *consumed = (b.bitpos + 7) / 8;
    return 0;
}

// Spread of the symbols over the 1 << log cells: put(cell, symbol) for every cell, next[s] = the first state counter of every
// symbol that has cells.  Returns the position the walk ends on: not 0 = the counts do not fill the table (the caller's verdict).
template <class Norm, class Next, class Put>
ZR_FN int fse_spread(Norm norm, Next next, int nsym, int log, Put put) {
    const int size = 1 << log;
    int high = size;
    for (int s = 0; s < nsym; s++)
        if (norm.get((uint32_t)s) == -1) { put((uint32_t)--high, (uint32_t)s); next.set((uint32_t)s, 1); }
    const int step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    int pos = 0;
    for (int s = 0; s < nsym; s++) {
        const int c = norm.get((uint32_t)s);
        if (c <= 0) continue;
        next.set((uint32_t)s, c);
        for (int i = 0; i < c; i++) {
            put((uint32_t)pos, (uint32_t)s);
            do { pos = (pos + step) & mask; } while (pos >= high);
        }
    }
    return pos;
}
// the state counter of the next cell of symbol sym, in cell order
template <class Next>
ZR_FN uint32_t fse_take_state(Next next, uint32_t sym) {
    const uint32_t ns = (uint32_t)next.get(sym);
    next.set(sym, (int)(ns + 1));
    return ns;
}
// a cell from its state counter ns (>= 1): bits to read, and the base of the next state
struct FseCell { uint32_t next, nbits; };
ZR_FN FseCell fse_cell(uint32_t ns, uint32_t log) {
    const uint32_t nb = log - (uint32_t)highbit(ns);
    return FseCell{(ns << nb) - (1u << log), nb};
}

// what symbol sym of a table of kind `kind` stands for: value baseline and extra bits (kind < 0: plain symbols, the Huffman weights)
ZR_FN bool sym_in_range(int kind, uint32_t sym) { return kind < 0 || sym <= (uint32_t)kind_max_sym(kind); }
struct SymValue { uint32_t base, bits; };
ZR_FN SymValue sym_value(int kind, uint32_t sym) {  // sym_in_range(kind, sym)
    if (kind == K_LL) return SymValue{LL_BASE[sym], LL_BITS[sym]};
    if (kind == K_ML) return SymValue{ML_BASE[sym], ML_BITS[sym]};
    if (kind == K_OF) return SymValue{1u << sym, sym};
    return SymValue{sym, 0};
}

// ---- Sequences_Section_Header (3.1.1.3.2.1) of the section [q, q + n) ------------------------------------------------------------
// Number_of_Sequences, then for LL, OF, ML in turn what the modes byte says, told to cb (each answers 0 or an error, which ends
// the walk):  cb.predefined(k)   cb.rle(k, symbol)   cb.described(k, description, bytes available, &bytes used)   cb.repeat(k)
// *bits_at = where the bitstream starts (the end of the count for a section without sequences).
template <class Cb>
ZR_FN int seq_header(const uint8_t *q, uint32_t n, uint32_t *nseq_out, uint32_t *bits_at, Cb &cb) {
    if (n < 1) return E_TRUNC;
    uint32_t p = 0, nseq = 0;
    const uint32_t b0 = q[0];
    if (b0 < 128) { nseq = b0; p = 1; }
    else if (b0 < 255) { if (n < 2) return E_TRUNC; nseq = ((b0 - 128) << 8) + q[1]; p = 2; }
    else { if (n < 3) return E_TRUNC; nseq = q[1] + ((uint32_t)q[2] << 8) + 0x7F00; p = 3; }
    *nseq_out = nseq;
    *bits_at = p;
    if (!nseq) return 0;
    if (p >= n) return E_TRUNC;
    const uint32_t modes = q[p++];
    if (modes & 3) return E_CORRUPT;
    for (int k = 0; k < 3; k++) {
        const uint32_t mode = (modes >> kind_mode_shift(k)) & 3;
        int rc;
        if (mode == 0) rc = cb.predefined(k);
        else if (mode == 1) {
            if (p >= n) return E_TRUNC;
            rc = cb.rle(k, (uint32_t)q[p]);
            p++;
        } else if (mode == 2) {
            uint32_t used = 0;
            rc = cb.described(k, q + p, n - p, &used);
            p += used;
        } else rc = cb.repeat(k);
        if (rc) return rc;
    }
    *bits_at = p;
    return 0;
}

// ---- Huffman tree description (4.2.1) ---------------------------------------------------------------------------------------
// direct form (header byte hb >= 128): hb - 127 weights of 4 bits
template <class W>
ZR_FN int huf_direct_weights(const uint8_t *src, uint32_t n, W w, uint32_t *nw, uint32_t *consumed) {
    const uint32_t num = (uint32_t)src[0] - 127, bytes = (num + 1) / 2;
    if (1 + bytes > n) return E_TRUNC;
    for (uint32_t i = 0; i < num; i++) {
        const uint8_t b = src[1 + i / 2];
        w.set(i, (i & 1) ? (b & 15) : (b >> 4));
    }
    *nw = num;
    *consumed = 1 + bytes;
    return 0;
}
// FSE form: two states take turns over one backward stream b (read(nb), pos = unread bits: below 0 = ran out); tab(state) yields
// the cell {weight, nbits, next}.  A state emits its weight and updates; when the update runs off the stream the other state
// emits the last weight.  At most 255 weights.  EARLY: the other state's cell (the last weight, or the next turn's) is fetched before the
// stream's verdict is in: 2.5 % of k_bx_prep, where 64 lanes walk their LDS stripes at once; a lone lane is 1.6 % of k_zstd_decode faster without.
struct HufCell { uint32_t weight, nbits, next; };
template <bool EARLY, class Bits, class Tab, class W>
ZR_FN int huf_walk_weights(Bits &b, uint32_t log, Tab tab, W w, uint32_t *nw_out) {
    uint32_t cur = b.read(log), other = b.read(log), nw = 0;
    HufCell e = tab(cur);
    for (;;) {
        if (nw >= 255) return E_CORRUPT;
        w.set(nw++, (int)e.weight);
        cur = e.next + b.read(e.nbits);
        HufCell eo = e;
        if (EARLY) eo = tab(other);
        if (b.pos < 0) {
            if (nw >= 255) return E_CORRUPT;
            if (!EARLY) eo = tab(other);
            w.set(nw++, (int)eo.weight);
            break;
        }
        const uint32_t t = cur; cur = other; other = t;
        e = EARLY ? eo : tab(cur);
    }
    *nw_out = nw;
    return 0;
}
// the nw weights that were read -> the longest code's length and the weight of the implied last symbol
template <class W>
ZR_FN int huf_limits(W w, uint32_t nw, uint32_t *maxbits_out, uint32_t *last_weight) {
    uint32_t total = 0;
    for (uint32_t i = 0; i < nw; i++) {
        const uint32_t x = (uint32_t)w.get(i);
        if (x > 12) return E_CORRUPT;
        total += x ? 1u << (x - 1) : 0;
    }
    if (total == 0) return E_CORRUPT;
    const uint32_t maxbits = (uint32_t)highbit(total) + 1;
    if (maxbits > 11) return E_CORRUPT;
    const uint32_t left = (1u << maxbits) - total;
    if (left & (left - 1)) return E_CORRUPT;
    *maxbits_out = maxbits;
    *last_weight = (uint32_t)highbit(left) + 1;
    return 0;
}
// rank[bits] = first cell of the codes of length bits in the 1 << maxbits decoding table, longest codes first (as the table is
// laid out); rank holds 16 entries
template <class W, class Rank>
ZR_FN int huf_rank_starts(W w, uint32_t nsym, uint32_t maxbits, Rank rank) {
    for (uint32_t i = 0; i < 16; i++) rank.set(i, 0);
    for (uint32_t i = 0; i < nsym; i++) {
        const uint32_t x = (uint32_t)w.get(i);
        if (x) rank.set(maxbits + 1 - x, rank.get(maxbits + 1 - x) + 1);  // count per code length
    }
    uint32_t start = 0;
    for (uint32_t bits = maxbits; bits >= 1; bits--) {
        const uint32_t cnt = (uint32_t)rank.get(bits);
        rank.set(bits, (int)start);
        start += cnt << (maxbits - bits);
    }
    return start == (1u << maxbits) ? 0 : E_CORRUPT;
}

}  // namespace zr
