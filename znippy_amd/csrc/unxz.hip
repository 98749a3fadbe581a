// Whole xz files (znippy_unxz_batch): every block of every stream of every item decoded straight into its place in the item's room.
// An xz file names each block's compressed and uncompressed size in the index at the end of its stream, so the host
// (host/xz_plan.{h,cc}) knows every block's source range and output offset before a byte is decoded, and all blocks of all items
// are one launch.  Three kernels:
//
//   tail     wave = range: the bytes the host's container walk asks for (stream padding, footer, index, stream header: a few
//            bytes per block) go to a staging buffer that is copied to the host.  One launch per round of the walk.
//   decode   wave = block.  The wave checks and parses its own block header (size byte, CRC32, flags, optional sizes, the filter
//            list: exactly one filter, LZMA2), walks the LZMA2 chunks (xz_chunks) and decodes each LZMA chunk (lzma_run); it
//            records the status, the bytes written, the sizes the header names and the check field.  LZMA is an adaptive range
//            coder: every bit's probability depends on the bits decoded before it, so a block is strictly serial and the wave
//            runs it in wave-uniform control flow: range, code, the LZMA state and rep0..3 are scalars (every value read from
//            LDS or memory goes through readfirstlane), the 11-bit probabilities are 16-bit cells in LDS that all lanes read and
//            write alike.  The lanes differ where bytes move: literals are gathered one per lane and stored 64 at a time,
//            matches and uncompressed chunks are copied by all lanes (coop_match lays an overlapping match down by period
//            doubling), the input comes through a 256-byte LDS window that all lanes fill.
//            The byte at rep0 and the previous byte, which the literal coder needs, never cost a memory round trip of their own: a
//            literal knows the literal before it, and a match loads both (they are bytes that existed before the match: the
//            period of an overlapping match repeats them) together with its own source bytes.
//   check    workgroup = block with check id 1 or 4: CRC32 or CRC64 (ECMA-182, reflected) of the bytes written, 256 segments
//            folded with x^n mod P as k_bunzip2_crc does.  The host compares.
//
//            As built, xz_block, xz_chunks and lzma_run are functions of their own and the state they hand on by reference is kept
//            in scratch memory (112 bytes a lane): the values are wave-uniform, but the compiler branches on them through the exec
//            mask.  Inlining the three removes the scratch (compiled, not yet run on the device).
//
// Occupancy.  A wave's LDS is the probabilities (1,860 + 0x300 << 4 = 14,148 cells, 28,296 bytes: sized for lc + lp = 4 whatever
// the chunk says) and the input window: 28,560 bytes, so a CU's 160 KiB hold five blocks and the 256 CUs 1,280 at a time.
//
// Control flow and bounds.  Every loop of the decoder either consumes a byte of the chunk layer's input, which is bounded by the
// block's compressed size, or produces at least one byte of the chunk's uncompressed size, which is checked against the block's
// output size from the index before the chunk starts.  Input behind the block reads as zeros and the position reached is checked
// afterwards.  A match is checked against the bytes since the last dictionary reset, the dictionary size and the chunk's rest
// before it is copied.  No byte outside [dst, dst + out_len) of the block is written whatever the input holds.
//
// The LZMA step (lzma_run and what it calls) knows nothing of LZMA2 chunks or xz blocks, so an lzip or LZMA-alone call can use it.
// Not done here: BCJ and delta filters, SHA-256, parallelism inside a block.
#include "inflate_dev.h"

namespace zn {

namespace {

constexpr uint32_t XZ_IN_WIN = 256;
// the probability cells of LZMA
constexpr uint32_t P_IS_MATCH = 0, P_IS_REP = 192, P_REP_G0 = 204, P_REP_G1 = 216, P_REP_G2 = 228, P_REP0_LONG = 240, P_SLOT = 432, P_SPEC = 688,
                   P_ALIGN = 816, P_LEN = 832, P_REPLEN = 1346, P_LIT = 1860;
constexpr uint32_t LEN_CHOICE = 0, LEN_CHOICE2 = 1, LEN_LOW = 2, LEN_MID = 130, LEN_HIGH = 258;  // 514 cells
constexpr uint32_t P_TOTAL = P_LIT + (0x300u << 4);
constexpr int E_UNSUPP = -6;  // ZNIPPY_E_UNSUPPORTED

struct XzLds {
    uint16_t p[P_TOTAL];
    alignas(16) uint8_t in[XZ_IN_WIN];
};

// Forward byte reader over [src, src + n) through the LDS window: zeros behind the end, and `pos` says how far a caller went.  All
// members are wave-uniform.
struct XzIn {
    const uint8_t *src;
    uint32_t n, pos, wbase;
    uint8_t *win;
    __device__ __forceinline__ void load(uint32_t lane) {
        wbase = pos;
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t i = wbase + lane * 4 + k;
            if (i >= wbase && i < n) v |= (uint32_t)src[i] << (8 * k);
        }
        __syncthreads();  // (one wave: the reads of the old window are done)
        *reinterpret_cast<uint32_t *>(win + lane * 4) = v;
        __syncthreads();
    }
    __device__ __forceinline__ uint32_t byte(uint32_t lane) {
        if (pos - wbase >= XZ_IN_WIN) load(lane);
        const uint32_t v = uni(win[pos - wbase]);
        pos++;
        return v;
    }
};

// ---- the LZMA step ------------------------------------------------------------------------------------------------------------
struct Lzma {
    uint32_t range, code;
    uint32_t state, rep0, rep1, rep2, rep3;
    uint32_t lc, lp, pb;
    uint32_t prev, mb;  // the last byte written, and the byte at rep0 behind the last match
    uint32_t nlit, mylit;  // literals not stored yet: lane l holds the l-th (mylit is per lane)
};

__device__ __forceinline__ void lzma_reset(XzLds &S, Lzma &z, uint32_t lane) {
    z.state = 0;
    z.rep0 = z.rep1 = z.rep2 = z.rep3 = 0;
    const uint32_t n = P_LIT + (0x300u << (z.lc + z.lp));
    __syncthreads();
    for (uint32_t i = lane; i < n; i += 64) S.p[i] = 1024;
    __syncthreads();
}

__device__ __forceinline__ void rc_norm(XzIn &in, Lzma &z, uint32_t lane) {
    if (z.range < (1u << 24)) {
        z.range <<= 8;
        z.code = z.code << 8 | in.byte(lane);
    }
}
__device__ __forceinline__ uint32_t rc_bit(XzLds &S, XzIn &in, Lzma &z, uint32_t idx, uint32_t lane) {
    rc_norm(in, z, lane);
    const uint32_t p = uni(S.p[idx]);
    const uint32_t bound = (z.range >> 11) * p;
    if (z.code < bound) {
        z.range = bound;
        S.p[idx] = (uint16_t)(p + ((2048 - p) >> 5));
        return 0;
    }
    z.range -= bound;
    z.code -= bound;
    S.p[idx] = (uint16_t)(p - (p >> 5));
    return 1;
}
__device__ __forceinline__ uint32_t rc_tree(XzLds &S, XzIn &in, Lzma &z, uint32_t base, uint32_t bits, uint32_t lane) {
    uint32_t m = 1;
    for (uint32_t i = 0; i < bits; i++) m = m << 1 | rc_bit(S, in, z, base + m, lane);
    return m - (1u << bits);
}
__device__ __forceinline__ uint32_t rc_rtree(XzLds &S, XzIn &in, Lzma &z, uint32_t base, uint32_t bits, uint32_t lane) {
    uint32_t m = 1, r = 0;
    for (uint32_t i = 0; i < bits; i++) {
        const uint32_t b = rc_bit(S, in, z, base + m, lane);
        m = m << 1 | b;
        r |= b << i;
    }
    return r;
}
__device__ __forceinline__ uint32_t rc_direct(XzIn &in, Lzma &z, uint32_t bits, uint32_t lane) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < bits; i++) {
        rc_norm(in, z, lane);
        z.range >>= 1;
        z.code -= z.range;
        const uint32_t t = 0u - (z.code >> 31);
        z.code += z.range & t;
        r = (r << 1) + (t + 1);
    }
    return r;
}
__device__ __forceinline__ uint32_t lzma_len(XzLds &S, XzIn &in, Lzma &z, uint32_t base, uint32_t ps, uint32_t lane) {
    if (!rc_bit(S, in, z, base + LEN_CHOICE, lane)) return 2 + rc_tree(S, in, z, base + LEN_LOW + ps * 8, 3, lane);
    if (!rc_bit(S, in, z, base + LEN_CHOICE2, lane)) return 10 + rc_tree(S, in, z, base + LEN_MID + ps * 8, 3, lane);
    return 18 + rc_tree(S, in, z, base + LEN_HIGH, 8, lane);
}
__device__ __forceinline__ void lzma_flush(Lzma &z, uint8_t *dst, uint32_t pos, uint32_t lane) {
    if (lane < z.nlit) dst[pos - z.nlit + lane] = (uint8_t)z.mylit;
    z.nlit = 0;
}

// One range-coded run: the five bytes that start the coder, symbols until dst[pos .. pos_end) is full, the last normalisation.
// `dict_base` is where the dictionary starts (no match reaches in front of it, and positions count from it), dict_size the most a
// match may reach back.  The caller checks where the input ended up.  Returns 0 or E_CORRUPT; *pos_io says how far it came.
__device__ int lzma_run(XzLds &S, XzIn &in, Lzma &z, uint8_t *dst, uint32_t *pos_io, uint32_t pos_end, uint32_t dict_base, uint32_t dict_size,
                        uint32_t lane) {
    uint32_t pos = *pos_io;
    z.range = 0xFFFFFFFFu;
    z.code = 0;
    const uint32_t first = in.byte(lane);
    for (uint32_t k = 0; k < 4; k++) z.code = z.code << 8 | in.byte(lane);
    int st = first ? E_CORRUPT : 0;
    const uint32_t pmask = (1u << z.pb) - 1, lmask = (1u << z.lp) - 1;
    while (st == 0 && pos < pos_end) {
        const uint32_t posd = pos - dict_base, ps = posd & pmask;
        if (!rc_bit(S, in, z, P_IS_MATCH + (z.state << 4) + ps, lane)) {
            const uint32_t probs = P_LIT + 0x300u * (((posd & lmask) << z.lc) + (z.prev >> (8 - z.lc)));
            uint32_t sym = 1;
            if (z.state < 7) {
                while (sym < 0x100) sym = sym << 1 | rc_bit(S, in, z, probs + sym, lane);
            } else {
                uint32_t m = z.mb, offs = 0x100;
                while (sym < 0x100) {
                    m <<= 1;
                    const uint32_t mbit = m & offs;
                    const uint32_t b = rc_bit(S, in, z, probs + offs + mbit + sym, lane);
                    sym = sym << 1 | b;
                    offs &= b ? mbit : ~mbit;
                }
            }
            z.prev = sym & 0xFF;
            if (lane == z.nlit) z.mylit = z.prev;
            z.nlit++;
            pos++;
            if (z.nlit == 64) lzma_flush(z, dst, pos, lane);
            z.state = z.state < 4 ? 0 : z.state < 10 ? z.state - 3 : z.state - 6;
            continue;
        }
        uint32_t len;
        if (!rc_bit(S, in, z, P_IS_REP + z.state, lane)) {
            z.rep3 = z.rep2;
            z.rep2 = z.rep1;
            z.rep1 = z.rep0;
            len = lzma_len(S, in, z, P_LEN, ps, lane);
            z.state = z.state < 7 ? 7 : 10;
            const uint32_t slot = rc_tree(S, in, z, P_SLOT + ((len < 6 ? len - 2 : 3u) << 6), 6, lane);
            if (slot < 4) {
                z.rep0 = slot;
            } else {
                const uint32_t nd = (slot >> 1) - 1;
                z.rep0 = (2 | (slot & 1)) << nd;
                if (slot < 14) {
                    z.rep0 += rc_rtree(S, in, z, P_SPEC + z.rep0 - slot - 1, nd, lane);
                } else {
                    z.rep0 += rc_direct(in, z, nd - 4, lane) << 4;
                    z.rep0 += rc_rtree(S, in, z, P_ALIGN, 4, lane);
                    if (z.rep0 == 0xFFFFFFFFu) st = E_CORRUPT;  // an end marker: LZMA2 has none
                }
            }
        } else if (!rc_bit(S, in, z, P_REP_G0 + z.state, lane)) {
            if (!rc_bit(S, in, z, P_REP0_LONG + (z.state << 4) + ps, lane)) {
                z.state = z.state < 7 ? 9 : 11;
                len = 1;
            } else {
                len = lzma_len(S, in, z, P_REPLEN, ps, lane);
                z.state = z.state < 7 ? 8 : 11;
            }
        } else {
            uint32_t d;
            if (!rc_bit(S, in, z, P_REP_G1 + z.state, lane)) {
                d = z.rep1;
            } else {
                if (!rc_bit(S, in, z, P_REP_G2 + z.state, lane)) {
                    d = z.rep2;
                } else {
                    d = z.rep3;
                    z.rep3 = z.rep2;
                }
                z.rep2 = z.rep1;
            }
            z.rep1 = z.rep0;
            z.rep0 = d;
            len = lzma_len(S, in, z, P_REPLEN, ps, lane);
            z.state = z.state < 7 ? 8 : 11;
        }
        if (st) break;
        if (z.rep0 >= posd || z.rep0 >= dict_size || len > pos_end - pos) {
            st = E_CORRUPT;
            break;
        }
        // the copy.  The byte the match would go on with and its last byte existed before it (the period of an overlapping match
        // repeats them): both are loaded with the match's own source bytes
        const uint32_t dist = z.rep0 + 1;
        lzma_flush(z, dst, pos, lane);
        wave_mem_sync();  // the source bytes are this wave's earlier stores
        const uint32_t r_next = len < dist ? len : len % dist, r_last = len - 1 < dist ? len - 1 : (len - 1) % dist;
        const uint32_t v_next = dst[pos - dist + r_next], v_last = dst[pos - dist + r_last];
        coop_match<1>(dst + pos, dist, len, lane, false, nullptr);
        z.mb = uni(v_next);
        z.prev = uni(v_last);
        pos += len;
    }
    lzma_flush(z, dst, pos, lane);
    rc_norm(in, z, lane);
    if (st == 0 && z.code != 0) st = E_CORRUPT;
    *pos_io = pos;
    return st;
}

// ---- the LZMA2 chunk layer ------------------------------------------------------------------------------------------------------
// The chunks in [in.pos, comp_end) into dst[0 .. out_len): 0 only if the end byte stands exactly at comp_end and exactly out_len
// bytes were written.  The rules are liblzma's (lzma2_decoder.c): 0x01 and 0xE0.. reset the dictionary and the first chunk must;
// the first LZMA chunk behind a dictionary reset must bring properties; an uncompressed chunk changes neither the LZMA state nor
// what the next chunk must bring.
__device__ int xz_chunks(XzLds &S, XzIn &in, uint32_t comp_end, uint8_t *dst, uint32_t out_len, uint32_t dict_size, uint32_t lane, uint32_t *produced) {
    Lzma z;
    z.state = z.rep0 = z.rep1 = z.rep2 = z.rep3 = 0;
    z.lc = z.lp = z.pb = 0;
    z.prev = z.mb = 0;
    z.nlit = z.mylit = 0;
    uint32_t pos = 0, dict_base = 0;
    bool need_dict = true, need_props = true;
    int st = 0;
    for (;;) {
        if (in.pos >= comp_end) { st = E_CORRUPT; break; }
        const uint32_t ctl = in.byte(lane);
        if (ctl == 0) break;
        if (ctl >= 0xE0 || ctl == 1) {
            need_props = true;
            need_dict = false;
            dict_base = pos;
            z.prev = 0;
        } else if (need_dict) { st = E_CORRUPT; break; }
        if (ctl >= 0x80) {
            uint32_t usize = (ctl & 0x1F) << 16;
            usize += in.byte(lane) << 8;
            usize += in.byte(lane) + 1;
            uint32_t csize = in.byte(lane) << 8;
            csize += in.byte(lane) + 1;
            if (ctl >= 0xC0) {
                uint32_t d = in.byte(lane);
                if (d > 224) { st = E_CORRUPT; break; }
                z.pb = d / 45;
                d -= z.pb * 45;
                z.lp = d / 9;
                z.lc = d - z.lp * 9;
                if (z.lc + z.lp > 4) { st = E_CORRUPT; break; }
                need_props = false;
                lzma_reset(S, z, lane);
            } else if (need_props) {
                st = E_CORRUPT;
                break;
            } else if (ctl >= 0xA0) {
                lzma_reset(S, z, lane);
            }
            if (in.pos > comp_end || csize > comp_end - in.pos || usize > out_len - pos) { st = E_CORRUPT; break; }
            const uint32_t chunk_end = in.pos + csize, pos_end = pos + usize;
            st = lzma_run(S, in, z, dst, &pos, pos_end, dict_base, dict_size, lane);
            if (st == 0 && (in.pos != chunk_end || pos != pos_end)) st = E_CORRUPT;
            if (st) break;
        } else {
            if (ctl > 2) { st = E_CORRUPT; break; }
            uint32_t n = in.byte(lane) << 8;
            n += in.byte(lane) + 1;
            if (in.pos > comp_end || n > comp_end - in.pos || n > out_len - pos) { st = E_CORRUPT; break; }
            const uint8_t *from = in.src + in.pos;
            for (uint32_t i = lane; i < n; i += 64) dst[pos + i] = from[i];
            wave_mem_sync();
            pos += n;
            in.pos += n;
            z.prev = uni(dst[pos - 1]);
            if (!need_props && z.rep0 < pos - dict_base) z.mb = uni(dst[pos - z.rep0 - 1]);
        }
    }
    if (st == 0 && (in.pos != comp_end || pos != out_len)) st = E_CORRUPT;
    *produced = pos;
    return st;
}

// ---- the block ------------------------------------------------------------------------------------------------------------------
// A VLI of the block header, which ends at `limit`: at most 9 bytes, no needless trailing zero byte
__device__ __forceinline__ bool xz_vli(XzIn &in, uint32_t limit, uint32_t lane, uint64_t *v) {
    uint64_t r = 0;
    for (uint32_t i = 0; i < 9; i++) {
        if (in.pos >= limit) return false;
        const uint32_t b = in.byte(lane);
        r |= (uint64_t)(b & 0x7F) << (7 * i);
        if (!(b & 0x80)) {
            *v = r;
            return !(b == 0 && i > 0);
        }
    }
    return false;
}

__device__ int xz_block(XzLds &S, const uint8_t *blk, uint32_t unpadded, uint32_t check, uint8_t *dst, uint32_t out_len, uint32_t lane, XzRec &r) {
    const uint32_t cs = check == 0 ? 0u : 4u << ((check - 1) / 3);
    XzIn in{blk, (unpadded + 3) & ~3u, 0, 0, S.in};
    in.load(lane);
    const uint32_t size_byte = in.byte(lane);
    if (!size_byte) return E_CORRUPT;  // (an index indicator)
    const uint32_t hdr = (size_byte + 1) * 4, limit = hdr - 4;
    r.hdr_size = hdr;
    if (hdr + cs > unpadded) return E_CORRUPT;
    r.comp = unpadded - hdr - cs;
    {   // the header's CRC32 first, as liblzma does: a damaged header is corrupt whatever its fields then say
        uint32_t crc = 0xFFFFFFFFu;
        in.pos = 0;
        for (uint32_t i = 0; i < limit; i++) {
            crc ^= in.byte(lane);
            for (uint32_t k = 0; k < 8; k++) crc = crc & 1 ? (crc >> 1) ^ CRC_POLY : crc >> 1;
        }
        uint32_t stored = 0;
        for (uint32_t k = 0; k < 4; k++) stored |= in.byte(lane) << (8 * k);
        if (stored != ~crc) return E_CORRUPT;
    }
    in.pos = 1;
    const uint32_t flags = in.byte(lane);
    if (flags & 0x3C) return E_UNSUPP;
    if ((flags & 0x40) && !xz_vli(in, limit, lane, &r.hdr_comp)) return E_CORRUPT;
    if ((flags & 0x80) && !xz_vli(in, limit, lane, &r.hdr_uncomp)) return E_CORRUPT;
    const uint32_t n_filters = (flags & 3) + 1;
    bool lzma2 = false;
    uint32_t prop = 0;
    for (uint32_t f = 0; f < n_filters; f++) {
        uint64_t id = 0, psize = 0;
        if (!xz_vli(in, limit, lane, &id) || !xz_vli(in, limit, lane, &psize)) return E_CORRUPT;
        if (psize > limit - in.pos) return E_CORRUPT;
        if (id == 0x21 && psize == 1) {
            lzma2 = true;
            prop = in.byte(lane);
        } else {
            in.pos += (uint32_t)psize;
        }
    }
    while (in.pos < limit)
        if (in.byte(lane)) return E_CORRUPT;
    if (n_filters != 1 || !lzma2 || prop > 40) return E_UNSUPP;  // BCJ, delta, a chain, an unknown filter
    const uint32_t dict_size = prop == 40 ? 0xFFFFFFFFu : (2 | (prop & 1)) << (prop / 2 + 11);
    in.pos = hdr;
    const int st = xz_chunks(S, in, hdr + r.comp, dst, out_len, dict_size, lane, &r.produced);
    if (st) return st;
    while (in.pos & 3)  // block padding
        if (in.byte(lane)) return E_CORRUPT;
    uint32_t w[2] = {0, 0};
    for (uint32_t k = 0; k < 8 && k < cs; k++) w[k >> 2] |= in.byte(lane) << (8 * (k & 3));
    r.check_lo = w[0];
    r.check_hi = w[1];
    return 0;
}

__global__ __launch_bounds__(64) void k_unxz_tail(const XzItem *items, const XzRange *ranges, uint32_t n_ranges, uint8_t *stage) {
    for (uint32_t k = blockIdx.x; k < n_ranges; k += gridDim.x) {
        const XzRange R = ranges[k];
        const uint8_t *from = items[R.item].src + R.off;
        for (uint32_t i = threadIdx.x; i < R.len; i += 64) stage[R.at + i] = from[i];
    }
}

__global__ __launch_bounds__(64) void k_unxz_decode(const XzItem *items, const XzJob *jobs, uint32_t n_jobs, XzRec *recs) {
    __shared__ XzLds S;
    const uint32_t lane = threadIdx.x;
    for (uint32_t j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        const XzJob J = jobs[j];
        const XzItem it = items[J.item];
        XzRec r;
        r.status = 0;
        r.produced = 0;
        r.hdr_comp = r.hdr_uncomp = XZ_ABSENT;
        r.check_lo = r.check_hi = r.hdr_size = r.comp = 0;
        r.status = xz_block(S, it.src + J.src_off, J.unpadded, J.check, it.dst + J.out_off, J.out_len, lane, r);
        if (lane == 0) recs[j] = r;
        __syncthreads();
    }
}

template <typename W>
__device__ __forceinline__ W xz_mulmod(W a, W b, W poly) {  // a * b mod P, reflected
    constexpr uint32_t B = sizeof(W) * 8;
    W p = 0;
    for (uint32_t i = 0; i < B; i++) {
        if (a & ((W)1 << (B - 1 - i))) p ^= b;
        b = b & 1 ? (b >> 1) ^ poly : b >> 1;
    }
    return p;
}
template <typename W>
__device__ __forceinline__ W xz_xpow(uint64_t n, W poly) {  // x^n mod P
    constexpr uint32_t B = sizeof(W) * 8;
    W r = (W)1 << (B - 1), q = (W)1 << (B - 2);
    for (uint32_t i = 0; i < 40; i++) {
        if ((n >> i) & 1) r = xz_mulmod(r, q, poly);
        q = xz_mulmod(q, q, poly);
    }
    return r;
}
// The CRC of p[0 .. len) by 256 threads: 256 segments aligned to the end (k_inflate_crc's split), folded pairwise
template <typename W>
__device__ W xz_crc(const uint8_t *p, uint64_t len, W poly, W *T, W *red, uint32_t tid) {
    {
        W c = tid;
        for (int k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ poly : c >> 1;
        T[tid] = c;
    }
    __syncthreads();
    const uint64_t seg = (len + 255) >> 8;
    int64_t a = (int64_t)len - (int64_t)(256 - tid) * (int64_t)seg, e = a + (int64_t)seg;
    if (a < 0) a = 0;
    if (e < 0) e = 0;
    W crc = ~(W)0;
    for (; a < e; a++) crc = T[(uint32_t)(crc ^ p[a]) & 255] ^ (crc >> 8);
    red[tid] = ~crc;
    __syncthreads();
    W pw = xz_xpow<W>(8 * seg, poly);
    for (uint32_t stride = 1; stride < 256; stride <<= 1) {
        if ((tid & (2 * stride - 1)) == 0) red[tid] = xz_mulmod(pw, red[tid], poly) ^ red[tid + stride];
        __syncthreads();
        pw = xz_mulmod(pw, pw, poly);
    }
    const W out = red[0];
    __syncthreads();
    return out;
}

__global__ __launch_bounds__(256) void k_unxz_check(const XzItem *items, const XzJob *jobs, uint32_t n_jobs, uint64_t *sums) {
    __shared__ uint64_t T[256], red[256];
    const uint32_t tid = threadIdx.x;
    for (uint32_t j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        const XzJob J = jobs[j];
        const uint8_t *p = items[J.item].dst + J.out_off;
        uint64_t sum = 0;
        if (J.check == 1) sum = xz_crc<uint32_t>(p, J.out_len, CRC_POLY, (uint32_t *)T, (uint32_t *)red, tid);
        else if (J.check == 4) sum = xz_crc<uint64_t>(p, J.out_len, 0xC96C5795D7870F42ull, T, red, tid);
        if (tid == 0) sums[j] = sum;
    }
}

}  // namespace

void launch_unxz_tail(const XzItem *items, const XzRange *ranges, uint32_t n_ranges, uint8_t *stage, hipStream_t s) {
    if (n_ranges) hipLaunchKernelGGL(k_unxz_tail, dim3(n_ranges < 65536u ? n_ranges : 65536u), dim3(64), 0, s, items, ranges, n_ranges, stage);
}
void launch_unxz_decode(const XzItem *items, const XzJob *jobs, uint32_t n_jobs, XzRec *recs, hipStream_t s) {
    if (n_jobs) hipLaunchKernelGGL(k_unxz_decode, dim3(n_jobs < 65536u ? n_jobs : 65536u), dim3(64), 0, s, items, jobs, n_jobs, recs);
}
void launch_unxz_check(const XzItem *items, const XzJob *jobs, uint32_t n_jobs, uint64_t *sums, hipStream_t s) {
    if (n_jobs) hipLaunchKernelGGL(k_unxz_check, dim3(n_jobs < 65536u ? n_jobs : 65536u), dim3(256), 0, s, items, jobs, n_jobs, sums);
}

}  // namespace zn
