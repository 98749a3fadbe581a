// The block-start test of the gunzip cut search (gunzip.hip: k_gunzip_find), stated once: does a non-final dynamic DEFLATE block
// whose header is valid start at bit `bit` of src[0 .. n)?  The rules are those of dynamic_codes (inflate_dev.h), which are those
// written at znippy_inflate_batch: BFINAL 0, BTYPE 2; HLIT <= 29 and HDIST <= 29 (at most 286 literal/length and 30 distance codes);
// the code-length code complete; a repeat of the previous length never first, no repeat beyond the
// HLIT + HDIST lengths; a code for symbol 256; neither the literal/length nor the distance set over-subscribed, and each complete unless its longest code has
// one bit (or, for distances, there is none); and every bit of the header inside the input.
// A lane tests one bit position on its own, so nothing here is an array: the 19 code-length-code lengths are 57 bits of one word,
// their counts per length 35 bits of another, and of the two big sets only the Kraft sums, the longest lengths and whether symbol
// 256 has a code are kept, which is all the rules ask for.
// Plain C++: no HIP builtin, no include of the HIP runtime — the qualifiers sit behind GZC_FN, so a host compiler reads the same
// text (tests/test_gz_cut_rules_cpu.py runs it over every bit position of real streams against tests/gz_cut_model.py).
#pragma once
#include <stdint.h>

#ifndef GZC_FN
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GZC_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define GZC_FN inline __attribute__((always_inline))
#endif
#endif

namespace gzc {

// the eight bytes from byte `at` on, little-endian; bytes at and past n read as zero
GZC_FN uint64_t load64(const uint8_t *src, uint64_t n, uint64_t at) {
    uint64_t v = 0;
    if (at + 8 <= n) {
        __builtin_memcpy(&v, src + at, 8);
    } else {
        for (uint32_t k = 0; k < 8; k++)
            if (at + k < n) v |= (uint64_t)src[at + k] << (8 * k);
    }
    return v;
}
// at least 57 bits from bit position `bit` on
GZC_FN uint64_t peek(const uint8_t *src, uint64_t n, uint64_t bit) { return load64(src, n, bit >> 3) >> (bit & 7); }

// The first 13 bits: BFINAL 0, BTYPE 2, HLIT <= 29, HDIST <= 29.  About one position in nine passes.
GZC_FN bool quick13(uint32_t bits) { return (bits & 7u) == 4u && ((bits >> 3) & 31u) <= 29u && ((bits >> 8) & 31u) <= 29u; }

constexpr uint8_t CLEN_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
GZC_FN uint32_t clen_order(uint32_t i) {  // (a select chain: no load from constant memory on the device)
    uint32_t v = 0;
    for (uint32_t k = 0; k < 19; k++) v = i == k ? CLEN_ORDER[k] : v;
    return v;
}

// The whole test.  *end_bit (optional): the first bit behind the header, where the block's first symbol starts.
GZC_FN bool block_start(const uint8_t *src, uint64_t n, uint64_t bit, uint64_t *end_bit = nullptr) {
    const uint64_t nbits = n * 8;
    if (bit + 17 > nbits) return false;
    uint64_t w = peek(src, n, bit);
    if (!quick13((uint32_t)w & 0x1FFFu)) return false;
    const uint32_t hlit = (((uint32_t)w >> 3) & 31u) + 257, hdist = (((uint32_t)w >> 8) & 31u) + 1, hclen = (((uint32_t)w >> 13) & 15u) + 4;
    uint64_t pos = bit + 17;
    // the code-length code: lengths by symbol (3 bits each), counts by length (5 bits each)
    uint64_t clens = 0, ccnt = 0;
    for (uint32_t i = 0; i < hclen; i++) {
        if ((i & 15u) == 0) w = peek(src, n, pos + 3 * i);  // (16 lengths are 48 bits)
        const uint64_t l = (w >> (3 * (i & 15u))) & 7u;
        clens |= l << (3 * clen_order(i));
        if (l) ccnt += 1ull << (5 * l);
    }
    pos += 3 * hclen;
    if (pos > nbits) return false;
    uint32_t kraft = 0;
    for (uint32_t l = 1; l <= 7; l++) kraft += (uint32_t)((ccnt >> (5 * l)) & 31u) << (7 - l);
    if (kraft != 128) return false;  // over-subscribed or incomplete
    // the HLIT + HDIST lengths
    const uint32_t total = hlit + hdist;
    uint32_t i = 0, prev = 0, lk = 0, dk = 0, lmax = 0, dmax = 0, has256 = 0;  // Kraft sums in units of 2^-15
    while (i < total) {
        w = peek(src, n, pos);
        // canonical walk over the at most 7 bits of a code
        uint32_t code = 0, first = 0, index = 0, len = 0, rank = 0;
        for (uint32_t l = 1; l <= 7 && !len; l++) {
            code |= (uint32_t)(w >> (l - 1)) & 1u;
            const uint32_t count = (uint32_t)(ccnt >> (5 * l)) & 31u;
            if (code < first + count) {
                len = l;
                rank = code - first;
            }
            index += count;
            first = (first + count) << 1;
            code <<= 1;
        }
        (void)index;
        if (!len) return false;  // (a complete code: cannot happen)
        // the rank-th symbol, in symbol order, among those of this length
        uint32_t sym = 0, seen = 0;
        for (uint32_t s = 0; s < 19; s++) {
            const bool is = ((clens >> (3 * s)) & 7u) == len;
            if (is && seen == rank) sym = s;
            seen += is;
        }
        w >>= len;
        pos += len;
        uint32_t rep = 1, val = sym;
        if (sym == 16) {
            if (i == 0) return false;
            rep = 3 + ((uint32_t)w & 3u);
            val = prev;
            pos += 2;
        } else if (sym == 17) {
            rep = 3 + ((uint32_t)w & 7u);
            val = 0;
            pos += 3;
        } else if (sym == 18) {
            rep = 11 + ((uint32_t)w & 127u);
            val = 0;
            pos += 7;
        }
        if (i + rep > total) return false;
        if (pos > nbits) return false;
        if (val) {
            const uint32_t nl = i >= hlit ? 0u : (hlit - i < rep ? hlit - i : rep), nd = rep - nl;
            const uint32_t unit = 1u << (15 - val);
            lk += nl * unit;
            dk += nd * unit;
            if (nl && val > lmax) lmax = val;
            if (nd && val > dmax) dmax = val;
            if (i <= 256 && 256 < i + rep) has256 = 1;
        }
        prev = val;
        i += rep;
    }
    if (!has256) return false;
    if (lk > 32768u || (lk < 32768u && lmax > 1)) return false;
    if (dk > 32768u || (dk < 32768u && dmax > 1)) return false;
    if (end_bit) *end_bit = pos;
    return true;
}

}  // namespace gzc
