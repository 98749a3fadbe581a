// XXH64 (seed 0: the content checksum of RFC 8878 §3.1.1) cut into the pieces a lane decomposition is built from.
// Plain C++: no HIP builtin, no include of the HIP runtime — the qualifiers sit behind XXL_FN, so a host compiler reads
// the same text (tests/test_xxh64_lanes_cpu.py emulates both decompositions of zstd_batch.hip's checksum stage with it).
//
// The hash walks its input in stripes of 32 bytes.  Stripe i feeds its four 8-byte words to four accumulators, word j to
// accumulator j, and an accumulator's value after stripe i depends on its value after stripe i - 1: four serial chains.
// What one step does to a chain splits in two:
//   xxl_premul  in * P2                          — depends on the input alone: any lane, any time
//   xxl_chain   acc = rotl(acc + pre, 31) * P1   — the chain itself: one add, one rotate, one 64-bit multiply
// Behind the stripes: xxl_merge folds the four accumulators into one value (xxl_short for inputs below 32 bytes, which have
// no stripe), the length is added, the last len & 31 bytes go through xxl_tail (8-, 4- and 1-byte steps), xxl_avalanche ends.
#pragma once
#include <stdint.h>

#ifndef XXL_FN
#if defined(__HIPCC__) || defined(__CUDACC__)
#define XXL_FN __host__ __device__ inline
#else
#define XXL_FN inline
#endif
#endif

namespace xxl {

constexpr uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull, P4 = 0x85EBCA77C2B2AE63ull,
                   P5 = 0x27D4EB2F165667C5ull;
constexpr uint32_t STRIPE = 32;

XXL_FN uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
// little-endian loads from any address (the rows of a table start anywhere)
XXL_FN uint64_t load64(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
XXL_FN uint32_t load32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }

// accumulator j (0..3) before the first stripe
XXL_FN uint64_t acc_init(uint32_t j) { return j == 0 ? P1 + P2 : (j == 1 ? P2 : (j == 2 ? 0ull : 0ull - P1)); }
XXL_FN uint64_t premul(uint64_t in) { return in * P2; }
XXL_FN uint64_t chain(uint64_t acc, uint64_t pre) { return rotl(acc + pre, 31) * P1; }
XXL_FN uint64_t stripe_round(uint64_t acc, uint64_t in) { return chain(acc, premul(in)); }  // the stripe round of one accumulator

XXL_FN uint64_t merge_one(uint64_t h, uint64_t v) { return (h ^ stripe_round(0, v)) * P1 + P4; }
// the four accumulators of an input of >= 32 bytes -> one value (the length is not in it yet)
XXL_FN uint64_t merge(uint64_t v1, uint64_t v2, uint64_t v3, uint64_t v4) {
    uint64_t h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
    h = merge_one(h, v1); h = merge_one(h, v2); h = merge_one(h, v3);
    return merge_one(h, v4);
}
XXL_FN uint64_t short_start() { return P5; }  // in merge's place for an input below 32 bytes

XXL_FN uint64_t tail8(uint64_t h, uint64_t in) { return rotl(h ^ stripe_round(0, in), 27) * P1 + P4; }
XXL_FN uint64_t tail4(uint64_t h, uint32_t in) { return rotl(h ^ ((uint64_t)in * P1), 23) * P2 + P3; }
XXL_FN uint64_t tail1(uint64_t h, uint8_t in) { return rotl(h ^ ((uint64_t)in * P5), 11) * P1; }
// the n < 32 bytes behind the last stripe: reads [q, q + n) and nothing else
XXL_FN uint64_t tail(uint64_t h, const uint8_t *q, uint32_t n) {
    uint32_t i = 0;
    for (; i + 8 <= n; i += 8) h = tail8(h, load64(q + i));
    if (i + 4 <= n) { h = tail4(h, load32(q + i)); i += 4; }
    for (; i < n; i++) h = tail1(h, q[i]);
    return h;
}
XXL_FN uint64_t avalanche(uint64_t h) {
    h ^= h >> 33; h *= P2;
    h ^= h >> 29; h *= P3;
    return h ^ (h >> 32);
}
// everything behind the stripes: v[] = the four accumulators (looked at for len >= 32 only), p / len = the whole input
XXL_FN uint64_t finish(const uint64_t v[4], const uint8_t *p, uint64_t len) {
    uint64_t h = len >= STRIPE ? merge(v[0], v[1], v[2], v[3]) : short_start();
    h += len;
    return avalanche(tail(h, p + (len & ~(uint64_t)(STRIPE - 1)), (uint32_t)(len & (STRIPE - 1))));
}

}  // namespace xxl
