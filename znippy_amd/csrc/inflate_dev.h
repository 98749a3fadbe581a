// The DEFLATE (RFC 1951) stream decoder of one wave, shared by inflate.hip (k_inflate: raw streams of a known length) and targz.hip
// (k_targz_find: a gzip member that is decoded only as far as the tar inside it has to be read).  What the file comment of
// inflate.hip says about tables, input, output and control flow is said about this text.
// The body takes a hook: after every stored block and every symbol that adds bytes it is asked, with the wave-uniform count of
// bytes produced, whether it wants to look at them (due), and if so it is run behind a flush of the gathered literals and a
// wave_mem_sync; a hook that returns non-zero ends the stream loop through its condition.  NoHook is never due and costs nothing.
#pragma once
#include "zstd_dev.h"

namespace zn {

namespace {

constexpr uint32_t LB = 10, DB = 9, CB = 7;  // primary index bits: literal/length, distance, code-length code
constexpr uint32_t IN_WIN = 2048;            // bytes of the input window (+ 16: a refill may start at its last byte)
constexpr uint32_t NO_SYM = 0xFFFFu;
typedef __attribute__((address_space(1))) uint8_t glb8;
constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr int E_CRC = -7;  // ZNIPPY_E_CHECKSUM
// inside the decoder of a hooked stream: the input given ends in front of the bits a decision needs (zlib would ask for more input;
// which status that is depends on whether more input exists).  An unhooked stream has all its input: there it is E_CORRUPT.
constexpr int E_INPUT_END = -100;

struct InflLds {
    uint16_t lt[1u << LB], dt[1u << DB], ct[1u << CB];
    uint16_t lsym[288], dsym[32], csym[32];  // symbols sorted by code
    uint16_t lcnt[16], dcnt[16], ccnt[16];   // codes per length
    uint8_t lens[320];                       // the literal/length and distance code lengths: one sequence
    uint8_t clens[32];
    alignas(16) uint8_t in[IN_WIN + 16];
};

struct Code {
    const uint16_t *tab, *sym, *cnt;
    uint32_t mask;
};

__constant__ uint8_t c_clen_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// Forward bit reader over [src, src + n), through the LDS window.  All members are wave-uniform.
struct BitIn {
    const uint8_t *src;
    uint8_t *win;
    uint64_t n, ip, wbase;  // ip: the next byte to enter the bit buffer (may run past n: zeros)
    uint64_t bb;
    uint32_t bc;

    __device__ __forceinline__ void load_win(uint32_t lane) {
        wbase = ip;
        for (uint32_t j = lane * 16; j < IN_WIN + 16; j += 1024) {
            const uint64_t p = wbase + j;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (p + 16 <= n) {
                __builtin_memcpy(&v, src + p, 16);
            } else if (p < n) {
                uint8_t t[16];
                for (uint32_t k = 0; k < 16; k++) t[k] = p + k < n ? src[p + k] : (uint8_t)0;
                __builtin_memcpy(&v, t, 16);
            }
            *reinterpret_cast<uint4 *>(win + j) = v;
        }
        __syncthreads();
    }
    // at least 56 bits in the buffer afterwards.  The window is loaded anew when the 8 bytes at ip do not lie inside it — behind it,
    // or in front of it: the window starts at the ip of its load, the bit buffer then still holds bits of up to 7 bytes in front
    // of that, and a stored block sets ip back to the first byte the buffer had not used up (plus the block's length, which may be 0)
    __device__ __forceinline__ void refill(uint32_t lane) {
        if (ip < wbase || ip + 8 > wbase + IN_WIN + 16) load_win(lane);
        uint64_t v;
        __builtin_memcpy(&v, win + (uint32_t)(ip - wbase), 8);
        v = uni64(v);
        bb |= v << bc;
        ip += (63 - bc) >> 3;
        bc |= 56;
    }
    __device__ __forceinline__ void drop(uint32_t k) { bb >>= k; bc -= k; }
    __device__ __forceinline__ uint32_t take(uint32_t k) {
        const uint32_t v = (uint32_t)bb & ((1u << k) - 1);
        drop(k);
        return v;
    }
    // more bits consumed than the stream has
    __device__ __forceinline__ bool over() const { return ip * 8 - bc > n * 8; }
    // fewer than k bits are left
    __device__ __forceinline__ bool over_by(uint32_t k) const { return ip * 8 - bc + k > n * 8; }
};

// Canonical decoding tables of `n` code lengths L[0..n) (LDS) by the whole wave.  Returns < 0: over-subscribed (nothing usable was
// built), 0: complete, > 0: incomplete; *maxlen = the longest code (0: no code at all).
__device__ int build_code(const uint8_t *L, uint32_t n, uint16_t *tab, uint32_t pb, uint16_t *sorted, uint16_t *cnt, uint32_t lane, uint32_t *maxlen) {
    for (uint32_t i = lane; i < (1u << pb); i += 64) tab[i] = 0;
    const uint32_t chunks = (n + 63) >> 6;
    uint32_t cntv = 0;  // lane l: codes of length l
    for (uint32_t c = 0; c < chunks; c++) {
        const uint32_t s = c * 64 + lane, l = s < n ? L[s] : 0u;
        for (uint32_t ll = 1; ll <= 15; ll++) {
            const uint32_t k = (uint32_t)__popcll(__ballot(l == ll));
            if (lane == ll) cntv += k;
        }
    }
    if (lane < 16) cnt[lane] = (uint16_t)cntv;
    int left = 1;
    uint32_t code = 0, off = 0, firstv = 0, offv = 0, mx = 0;
    for (uint32_t ll = 1; ll <= 15; ll++) {
        const uint32_t k = rdlane_u(cntv, ll);
        left = left * 2 - (int)k;
        if (left < -(1 << 20)) left = -(1 << 20);
        if (lane == ll) { firstv = code; offv = off; }
        if (k) mx = ll;
        off += k;
        code = (code + k) << 1;
    }
    *maxlen = mx;
    // the running Kraft sum of an over-subscribed set goes below zero at some length and, doubled, never comes back
    if (left < 0) { __syncthreads(); return -1; }
    uint32_t runv = offv;  // lane l: where the next symbol of length l goes in `sorted`
    const uint64_t below = (1ull << lane) - 1;
    for (uint32_t c = 0; c < chunks; c++) {
        const uint32_t s = c * 64 + lane, l = s < n ? L[s] : 0u;
        uint32_t idx = 0;
        for (uint32_t ll = 1; ll <= 15; ll++) {
            const uint64_t m = __ballot(l == ll);
            const uint32_t base = rdlane_u(runv, ll);
            if (l == ll) idx = base + (uint32_t)__popcll(m & below);
            if (lane == ll) runv += (uint32_t)__popcll(m);
        }
        const uint32_t first_l = (uint32_t)__shfl((int)firstv, (int)l), off_l = (uint32_t)__shfl((int)offv, (int)l);
        if (l) {
            sorted[idx] = (uint16_t)s;
            if (l <= pb) {
                const uint32_t cd = first_l + (idx - off_l);
                const uint32_t r = __brev(cd) >> (32 - l);
                const uint16_t e = (uint16_t)(s << 4 | l);
                for (uint32_t k = r; k < (1u << pb); k += 1u << l) tab[k] = e;
            }
        }
    }
    __syncthreads();
    return left > 0 ? 1 : 0;
}

// One symbol from the low bits of `bits` (at least 15 valid or zero-filled): the primary cell, or the canonical walk for a longer
// code and for bits no code matches.  NO_SYM: no code matches.
__device__ __forceinline__ uint32_t decode_sym(const Code &c, uint64_t bits, uint32_t *len) {
    const uint32_t e = uni(c.tab[(uint32_t)bits & c.mask]);
    if (e) {
        *len = e & 15;
        return e >> 4;
    }
    uint32_t code = 0, first = 0, index = 0, sym = NO_SYM, found = 0;
    for (uint32_t l = 1; l <= 15; l++) {
        code |= (uint32_t)(bits >> (l - 1)) & 1u;
        const uint32_t count = uni(c.cnt[l]);
        if (!found && (int)(code - count) < (int)first) {
            sym = uni(c.sym[index + (code - first)]);
            *len = l;
            found = 1;
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return sym;
}

__device__ void fixed_codes(InflLds &S, uint32_t lane) {
    for (uint32_t s = lane; s < 288; s += 64) S.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
    if (lane < 32) S.lens[288 + lane] = 5;
    __syncthreads();
    uint32_t mx;
    (void)build_code(S.lens, 288, S.lt, LB, S.lsym, S.lcnt, lane, &mx);
    (void)build_code(S.lens + 288, 32, S.dt, DB, S.dsym, S.dcnt, lane, &mx);  // symbols 30 and 31 have codes; using one is an error
}

// The header of a dynamic block -> both codes.  0, E_CORRUPT or TR (the input ends inside the header).  As in zlib, a check is made
// once the bits it looks at are there: running out of input comes first.
template <int TR>
__device__ int dynamic_codes(InflLds &S, BitIn &b, uint32_t lane) {
    b.refill(lane);
    const uint32_t hlit = b.take(5) + 257, hdist = b.take(5) + 1, hclen = b.take(4) + 4;
    if (b.over()) return TR;
    if (hlit > 286 || hdist > 30) return E_CORRUPT;
    if (lane < 32) S.clens[lane] = 0;
    __syncthreads();
    for (uint32_t i = 0; i < hclen; i++) {
        if (b.bc < 3) b.refill(lane);
        S.clens[c_clen_order[i]] = (uint8_t)b.take(3);
    }
    __syncthreads();
    if (b.over()) return TR;
    uint32_t mx;
    if (build_code(S.clens, 19, S.ct, CB, S.csym, S.ccnt, lane, &mx) != 0) return E_CORRUPT;  // over-subscribed, or incomplete (always an error here)
    const Code cc = {S.ct, S.csym, S.ccnt, (1u << CB) - 1};
    const uint32_t total = hlit + hdist;
    uint32_t i = 0, prev = 0;
    int st = 0;
    while (i < total && st == 0) {
        b.refill(lane);
        uint32_t l = 0;
        const uint32_t sym = decode_sym(cc, b.bb, &l);
        if (sym == NO_SYM) {
            st = E_CORRUPT;  // (a complete code: cannot happen)
        } else {
            b.drop(l);
            if (sym < 16) {
                S.lens[i] = (uint8_t)sym;
                prev = sym;
                i++;
            } else {
                uint32_t rep, val = 0;
                if (sym == 16) {
                    if (i == 0) st = E_CORRUPT;
                    rep = 3 + b.take(2);
                    val = prev;
                } else if (sym == 17) {
                    rep = 3 + b.take(3);
                } else {
                    rep = 11 + b.take(7);
                }
                if (st == 0) {
                    if (i + rep > total) {
                        st = E_CORRUPT;
                    } else {
                        for (uint32_t k = lane; k < rep; k += 64) S.lens[i + k] = (uint8_t)val;
                        i += rep;
                        prev = val;
                    }
                }
            }
            if (b.over()) st = TR;
        }
    }
    __syncthreads();
    if (st) return st;
    if (uni(S.lens[256]) == 0) return E_CORRUPT;  // no end-of-block code
    int r = build_code(S.lens, hlit, S.lt, LB, S.lsym, S.lcnt, lane, &mx);
    if (r < 0 || (r > 0 && mx > 1)) return E_CORRUPT;  // incomplete is allowed for a single 1-bit code only
    r = build_code(S.lens + hlit, hdist, S.dt, DB, S.dsym, S.dcnt, lane, &mx);
    if (r < 0 || (r > 0 && mx > 1)) return E_CORRUPT;  // (no distance code at all is allowed: a block of literals)
    return 0;
}

struct NoHook {
    static constexpr bool active = false;
    __device__ __forceinline__ bool due(uint32_t) const { return false; }
    __device__ __forceinline__ uint32_t run(const uint8_t *, uint32_t, uint32_t) { return 0; }
};

// The stream behind the bit reader `b` (seated at the first block header, its window not loaded yet) into dst[0 .. out_len).
// *produced = the bytes written.  Returns 0 — the final block ended, or the hook ended the loop —, E_CORRUPT, E_DST or, hooked, E_INPUT_END.
// Unhooked, a symbol that would write past out_len is E_DST in front of its first byte.  Hooked, the part of a match or stored block
// that fits is written and shown to the hook first, and so is the part of a stored block that the input still holds: the hook sees
// every byte the input determines, up to out_len of them.
template <class Hook>
__device__ int inflate_body(InflLds &S, BitIn &b, uint8_t *dst, uint32_t out_len, uint32_t lane, Hook &hook, uint32_t *produced) {
    constexpr int TR = Hook::active ? E_INPUT_END : E_CORRUPT;
    b.load_win(lane);
    const Code lc = {S.lt, S.lsym, S.lcnt, (1u << LB) - 1}, dc = {S.dt, S.dsym, S.dcnt, (1u << DB) - 1};
    int st = 0;
    uint32_t pos = 0;    // bytes produced, the gathered literals included
    uint32_t nlit = 0;   // literals gathered and not stored yet: lane k holds dst[pos - nlit + k]
    uint32_t mylit = 0;
    uint32_t done = 0, fixed_built = 0, stop = 0;
    while (!done && !stop && st == 0) {
        b.refill(lane);
        const uint32_t final_block = b.take(1), type = b.take(2);
        if (b.over()) {
            st = TR;
        } else if (type == 3) {
            st = E_CORRUPT;
        } else if (type == 0) {
            if (lane < nlit) dst[pos - nlit + lane] = (uint8_t)mylit;
            nlit = 0;
            b.drop(b.bc & 7);
            b.refill(lane);
            const uint32_t len = b.take(16), nlen = b.take(16);
            if (b.over()) {
                st = TR;
            } else if (len != (nlen ^ 0xFFFFu)) {
                st = E_CORRUPT;
            } else {
                const uint64_t at = b.ip - (b.bc >> 3);  // the next unread byte (not past src_len: the header was not)
                const uint64_t avail = b.n - at;
                const uint32_t copy = len < avail ? len : (uint32_t)avail;
                if constexpr (!Hook::active) {
                    if (copy > out_len - pos) {
                        st = E_DST;       // zlib would hand out byte out_len + 1 ...
                    } else if (copy < len) {
                        st = E_CORRUPT;   // ... before it runs out of input
                    } else {
                        coop_copy(dst + pos, b.src + at, len, lane, 64);
                        pos += len;
                        b.ip = at + len; b.bb = 0; b.bc = 0;
                        if (final_block) done = 1;
                    }
                } else {
                    const uint32_t room = out_len - pos, part = copy < room ? copy : room;
                    coop_copy(dst + pos, b.src + at, part, lane, 64);
                    pos += part;
                    if (hook.due(pos)) {
                        wave_mem_sync();
                        stop = hook.run(dst, pos, lane);
                    }
                    if (part < copy) {
                        st = E_DST;
                    } else if (copy < len) {
                        st = TR;
                    } else {
                        b.ip = at + len; b.bb = 0; b.bc = 0;
                        if (final_block) done = 1;
                    }
                }
            }
        } else {
            if (type == 1) {
                if (!fixed_built) fixed_codes(S, lane);
                fixed_built = 1;
            } else {
                fixed_built = 0;
                st = dynamic_codes<TR>(S, b, lane);
            }
            uint32_t eob = 0;
            while (!eob && !stop && st == 0) {
                b.refill(lane);  // 56 bits: a length code, its extra bits, a distance code and its extra bits are at most 48
                uint32_t l = 0;
                const uint32_t sym = decode_sym(lc, b.bb, &l);
                if (sym == NO_SYM) {
                    st = b.over_by(1) ? TR : E_CORRUPT;  // (an incomplete code is one 1-bit code: one bit decides)
                } else if (sym < 256) {
                    b.drop(l);
                    if (b.over()) {
                        st = TR;
                    } else if (pos == out_len) {
                        st = E_DST;
                    } else {
                        if (lane == nlit) mylit = sym;
                        nlit++;
                        pos++;
                        if (nlit == 64) {
                            dst[pos - 64 + lane] = (uint8_t)mylit;
                            nlit = 0;
                        }
                        if (hook.due(pos)) {
                            if (lane < nlit) dst[pos - nlit + lane] = (uint8_t)mylit;
                            nlit = 0;
                            wave_mem_sync();
                            stop = hook.run(dst, pos, lane);
                        }
                    }
                } else if (sym == 256) {
                    b.drop(l);
                    if (b.over()) st = TR;
                    else eob = 1;
                } else {
                    b.drop(l);
                    if (b.over()) {
                        st = TR;
                    } else if (sym > 285) {
                        st = E_CORRUPT;
                    } else {
                        const uint32_t i = sym - 257;
                        const uint32_t lx = i < 8 || i == 28 ? 0u : (i - 4) >> 2;
                        const uint32_t len = (i < 8 ? 3 + i : i == 28 ? 258u : 3 + ((4 + (i & 3)) << lx)) + b.take(lx);
                        uint32_t dl = 0;
                        const uint32_t ds = decode_sym(dc, b.bb, &dl);
                        if (ds == NO_SYM) {
                            st = b.over_by(1) ? TR : E_CORRUPT;
                        } else {
                            b.drop(dl);
                            const uint32_t dx = ds < 4 ? 0u : (ds - 2) >> 1;
                            const uint32_t dist = (ds < 4 ? 1 + ds : 1 + ((2 + (ds & 1)) << dx)) + (ds > 29 ? 0u : b.take(dx));
                            if (b.over()) {
                                st = TR;
                            } else if (ds > 29 || dist > pos) {
                                st = E_CORRUPT;
                            } else if (!Hook::active && len > out_len - pos) {
                                st = E_DST;
                            } else {
                                const uint32_t room = out_len - pos, part = len < room ? len : room;  // (unhooked: part == len)
                                if (lane < nlit) dst[pos - nlit + lane] = (uint8_t)mylit;
                                nlit = 0;
                                wave_mem_sync();  // the source bytes are this wave's earlier stores
                                coop_match<1>(dst + pos, dist, part, lane, false, nullptr);
                                pos += part;
                                if (hook.due(pos)) {
                                    wave_mem_sync();
                                    stop = hook.run(dst, pos, lane);
                                }
                                if (part < len) st = E_DST;
                            }
                        }
                    }
                }
            }
            if (st == 0 && !stop && final_block) done = 1;
        }
    }
    if (lane < nlit) dst[pos - nlit + lane] = (uint8_t)mylit;  // (inside the destination whatever the status)
    *produced = pos;
    return st;
}

// CRC-32 arithmetic on the reflected polynomial (k_inflate_crc, and the single pass of gunzip.hip)
__device__ __forceinline__ uint32_t crc_mulmod(uint32_t a, uint32_t b) {  // a * b mod P, reflected (zlib: multmodp)
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = b & 1 ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
__device__ __forceinline__ uint32_t crc_xpow(uint64_t n) {  // x^n mod P
    uint32_t r = 0x80000000u, q = 0x40000000u;
    for (uint32_t i = 0; i < 40; i++) {
        if ((n >> i) & 1) r = crc_mulmod(r, q);
        q = crc_mulmod(q, q);
    }
    return r;
}

// A hook that ends the stream loop once `n` bytes (> 0) exist: the decoder of a piece whose exact byte count is known (gunzip.hip).
struct StopAt {
    static constexpr bool active = true;
    uint32_t n;
    __device__ __forceinline__ bool due(uint32_t pos) const { return pos >= n; }
    __device__ __forceinline__ uint32_t run(const uint8_t *, uint32_t, uint32_t) { return 1; }
};

// The stream behind `b` decoded for its symbols and lengths alone: nothing is written (gunzip.hip: the probe of a candidate start).
// Symbol decoding needs no window, so the count of bytes and the place where the stream ends are those of the real decoder even when
// matches reach in front of the first byte; REACH says whether they may (a piece behind a flush point): then *reach is the longest
// such reach, otherwise a distance beyond the bytes produced is E_CORRUPT as in inflate_body.
// stops[0 .. n_stops): ascending byte positions of b.src.  The loop ends at the first block boundary behind a non-final stored block
// that is one of them (PROBE_BOUNDARY; b.ip is that position), behind the final block (PROBE_FINAL), or when more than `limit` bytes
// would exist (PROBE_LIMIT).  *how is defined when 0 is returned; otherwise E_CORRUPT, or E_INPUT_END where the input ends first.
constexpr uint32_t PROBE_FINAL = 0, PROBE_BOUNDARY = 1, PROBE_LIMIT = 2;
template <bool REACH>
__device__ int probe_body(InflLds &S, BitIn &b, uint64_t limit, const uint32_t *stops, uint32_t n_stops, uint32_t lane, uint64_t *produced, uint32_t *reach,
                          uint32_t *how) {
    constexpr int TR = E_INPUT_END;
    b.load_win(lane);
    const Code lc = {S.lt, S.lsym, S.lcnt, (1u << LB) - 1}, dc = {S.dt, S.dsym, S.dcnt, (1u << DB) - 1};
    int st = 0;
    uint64_t pos = 0;
    uint32_t far = 0, si = 0;
    uint32_t done = 0, fixed_built = 0, stop = 0;
    while (!done && !stop && st == 0) {
        b.refill(lane);
        const uint32_t final_block = b.take(1), type = b.take(2);
        if (b.over()) {
            st = TR;
        } else if (type == 3) {
            st = E_CORRUPT;
        } else if (type == 0) {
            b.drop(b.bc & 7);
            b.refill(lane);
            const uint32_t len = b.take(16), nlen = b.take(16);
            if (b.over()) {
                st = TR;
            } else if (len != (nlen ^ 0xFFFFu)) {
                st = E_CORRUPT;
            } else {
                const uint64_t at = b.ip - (b.bc >> 3);
                const uint64_t avail = b.n - at;
                pos += len < avail ? len : avail;
                if (pos > limit) {
                    stop = PROBE_LIMIT;
                } else if (len > avail) {
                    st = TR;
                } else {
                    b.ip = at + len; b.bb = 0; b.bc = 0;
                    if (final_block) {
                        done = 1;
                    } else {
                        // (the list is walked forward once over the whole stream: the positions only grow)
                        while (si < n_stops && uni(stops[si]) < b.ip) si++;
                        if (si < n_stops && uni(stops[si]) == b.ip) stop = PROBE_BOUNDARY;
                    }
                }
            }
        } else {
            if (type == 1) {
                if (!fixed_built) fixed_codes(S, lane);
                fixed_built = 1;
            } else {
                fixed_built = 0;
                st = dynamic_codes<TR>(S, b, lane);
            }
            uint32_t eob = 0;
            while (!eob && !stop && st == 0) {
                b.refill(lane);
                uint32_t l = 0;
                const uint32_t sym = decode_sym(lc, b.bb, &l);
                if (sym == NO_SYM) {
                    st = b.over_by(1) ? TR : E_CORRUPT;
                } else if (sym < 256) {
                    b.drop(l);
                    if (b.over()) st = TR;
                    else if (++pos > limit) stop = PROBE_LIMIT;
                } else if (sym == 256) {
                    b.drop(l);
                    if (b.over()) st = TR;
                    else eob = 1;
                } else {
                    b.drop(l);
                    if (b.over()) {
                        st = TR;
                    } else if (sym > 285) {
                        st = E_CORRUPT;
                    } else {
                        const uint32_t i = sym - 257;
                        const uint32_t lx = i < 8 || i == 28 ? 0u : (i - 4) >> 2;
                        const uint32_t len = (i < 8 ? 3 + i : i == 28 ? 258u : 3 + ((4 + (i & 3)) << lx)) + b.take(lx);
                        uint32_t dl = 0;
                        const uint32_t ds = decode_sym(dc, b.bb, &dl);
                        if (ds == NO_SYM) {
                            st = b.over_by(1) ? TR : E_CORRUPT;
                        } else {
                            b.drop(dl);
                            const uint32_t dx = ds < 4 ? 0u : (ds - 2) >> 1;
                            const uint32_t dist = (ds < 4 ? 1 + ds : 1 + ((2 + (ds & 1)) << dx)) + (ds > 29 ? 0u : b.take(dx));
                            if (b.over()) {
                                st = TR;
                            } else if (ds > 29 || (!REACH && dist > pos)) {
                                st = E_CORRUPT;
                            } else {
                                if (dist > pos && dist - (uint32_t)pos > far) far = dist - (uint32_t)pos;
                                pos += len;
                                if (pos > limit) stop = PROBE_LIMIT;
                            }
                        }
                    }
                }
            }
            if (st == 0 && !stop && final_block) done = 1;
        }
    }
    *produced = pos;
    *reach = far;
    *how = stop;
    return st;
}

}  // namespace

}  // namespace zn
