// Whole bzip2 files (znippy_bunzip2_batch): every block of every stream of every item decoded to the item's room, block CRCs and
// combined CRCs checked.  bzip2 blocks are independent and start at any bit; lbzip2 finds them by their 48-bit magic and so does the
// scan here.  What keeps a magic inside block data or trailing bytes from counting is the host's chain of records
// (host/bz_plan.{h,cc}): a candidate counts only if the block in front of it ended exactly at its bit.  One scan per call, then per
// pass of at most slot_cap blocks four launches, the host's plan between walk and expand:
//
//   scan     wave = 4 KiB of source: every bit position where 0x314159265359 starts is appended to the call's candidate list.
//   decode   wave = job.  A stream-header job reads "BZh" and the level and says which magic follows.  A block job reads the CRC,
//            origPtr, the used-byte map, the selectors and the code lengths, builds canonical tables in LDS and decodes the symbols
//            (Huffman in groups of 50, RUNA/RUNB, MTF) into the slot's byte area; it records the length, where the block ended, the
//            magic there and, behind an end magic, the combined CRC, the byte behind the padding and the three bytes there.  The
//            chain of symbols is serial: lane 0 walks it, the tables and the MTF list in LDS.
//   walk     workgroup = block that decoded.  (a) The successor array tt by a stable counting sort: 32 threads take contiguous slices,
//            their histograms are cnt[byte][slice] in LDS, a prefix over bytes and slices gives every slice its first place per byte,
//            each then scatters its slice.  tt is a permutation whatever the bytes are.  (b) Splitter list ranking: every node whose
//            index is a multiple of the spacing is a splitter, and so is origPtr; a thread walks from a splitter to the next one and
//            records it and the length; one thread walks the splitters from origPtr and gives each sublist its place; the threads
//            walk again and write.  Where the chain closes after L < n steps the first L bytes are walked and the rest repeats them.
//            (c) The final run-length step is parsed for lengths only: a thread's slice starts from the run state at the last
//            position in front of it where two consecutive bytes both differ from their predecessors (that byte starts a run), the
//            slices' expanded lengths are summed to offsets (the slice table) and to the block's out_len.
//   expand   workgroup = landed block: every thread expands its slice to its place in the room, bounded by the block's byte count.
//   crc      workgroup = landed block: the bzip2 CRC-32 (0x04C11DB7, MSB first) of the written bytes.  It is the bit reversal of the
//            zlib CRC over bit-reversed bytes, so the lane split and crc_mulmod / crc_xpow of inflate.hip's k_inflate_crc serve.
//
// Control flow and bounds.  The values that steer a workgroup (a job's status, length, origPtr) are read from one address by all of
// its threads.  The serial decoder consumes input or produces output in every iteration, reads zeros behind the end of the input
// and checks the position it reached; every walk is bounded by the block length in its condition; no loop that holds a barrier is
// left early.  A slot is written only inside its BZ_SLOT_BYTES, a room only inside the landed block's bytes.
//
// Not done here: Huffman decoding in parallel inside a block, randomised blocks, tar members inside .tar.bz2, xz.
#include "inflate_dev.h"

namespace zn {

namespace {

constexpr uint32_t BZ_MAGIC_HI = 0x314159u, BZ_MAGIC_LO = 0x265359u, BZ_END_HI = 0x177245u, BZ_END_LO = 0x385090u;
constexpr uint32_t BZ_MAX_SEL = 18002, BZ_GROUP = 50, BZ_MAX_LEN = 20;
constexpr uint32_t K_HEAD = 0, K_BLOCK = 1, NEXT_BLOCK = 0, NEXT_END = 1;  // bzp::K_*, NEXT_* of host/bz_plan.h
constexpr uint32_t SORT_SLICES = 32;

// MSB-first bit reader over [src, src + nbits / 8): zeros behind the end, and `pos` says how far a caller went
struct BzBits {
    const uint8_t *src;
    uint64_t nbits, pos;
};
__device__ __forceinline__ uint64_t bz_load56(const uint8_t *src, uint64_t n, uint64_t byte) {  // eight bytes from `byte` on, big endian
    uint64_t v = 0;
    if (byte + 8 <= n) {
        __builtin_memcpy(&v, src + byte, 8);
        v = __builtin_bswap64(v);
    } else {
        for (uint32_t k = 0; k < 8; k++) v = v << 8 | (byte + k < n ? src[byte + k] : 0u);
    }
    return v;
}
__device__ __forceinline__ uint32_t bz_peek(const BzBits &b, uint32_t k) {  // 1 <= k <= 32
    const uint64_t v = bz_load56(b.src, b.nbits >> 3, b.pos >> 3);
    return (uint32_t)((v << (b.pos & 7)) >> (64 - k));
}
__device__ __forceinline__ uint32_t bz_get(BzBits &b, uint32_t k) {
    const uint32_t v = bz_peek(b, k);
    b.pos += k;
    return v;
}

struct BzLds {
    uint32_t first[6][BZ_MAX_LEN + 1], count[6][BZ_MAX_LEN + 1], offs[6][BZ_MAX_LEN + 1];  // per length: first code, codes, index into perm
    uint32_t fill[BZ_MAX_LEN + 1];
    uint32_t min_len[6];
    uint16_t perm[6][258];  // symbols sorted by (length, symbol)
    uint8_t len[6][258];
    uint8_t sel[BZ_MAX_SEL];
    uint8_t mtf[256], seq[256];
    uint8_t pos[8];
};

// What stands behind a stream header or a block, at b.pos: into r.next and, behind an end magic, the trailer's fields
__device__ int bz_behind(BzBits &b, BzRec &r) {
    const uint32_t hi = bz_get(b, 24), lo = bz_get(b, 24);
    if (b.pos > b.nbits) return E_CORRUPT;
    if (hi == BZ_MAGIC_HI && lo == BZ_MAGIC_LO) {
        r.next = NEXT_BLOCK;
        return 0;
    }
    if (hi != BZ_END_HI || lo != BZ_END_LO) return E_CORRUPT;  // a block not followed by either magic
    r.next = NEXT_END;
    r.stream_crc = bz_get(b, 32);
    if (b.pos > b.nbits) return E_CORRUPT;
    const uint64_t n = b.nbits >> 3, after = (b.pos + 7) >> 3;
    r.after = after;
    r.tail_len = n - after < 3 ? (uint32_t)(n - after) : 3u;
    r.tail = 0;
    for (uint32_t k = 0; k < r.tail_len; k++) r.tail |= (uint32_t)b.src[after + k] << (8 * k);
    return 0;
}

// One block from behind its magic to its end-of-block symbol, by one lane: bytes[0 .. r.n) and the header's CRC and origPtr
__device__ int bz_block(BzLds &S, BzBits &b, uint8_t *bytes, BzRec &r) {
    r.block_crc = bz_get(b, 32);
    if (bz_get(b, 1)) return b.pos > b.nbits ? E_CORRUPT : -6;  // randomised: ZNIPPY_E_UNSUPPORTED
    r.orig = bz_get(b, 24);
    const uint32_t in16 = bz_get(b, 16);
    uint32_t n_used = 0;
    for (uint32_t i = 0; i < 16; i++) {
        if (in16 & (0x8000u >> i)) {
            const uint32_t m = bz_get(b, 16);
            for (uint32_t j = 0; j < 16; j++)
                if (m & (0x8000u >> j)) S.seq[n_used++] = (uint8_t)(i * 16 + j);
        }
    }
    if (b.pos > b.nbits || n_used == 0) return E_CORRUPT;
    const uint32_t alpha = n_used + 2, eob = n_used + 1;
    const uint32_t n_groups = bz_get(b, 3);
    if (n_groups < 2 || n_groups > 6) return E_CORRUPT;
    const uint32_t n_sel_read = bz_get(b, 15);
    if (n_sel_read < 1) return E_CORRUPT;
    for (uint32_t i = 0; i < n_sel_read; i++) {  // unary MTF indices; those above 18002 are read and discarded, as bzip2 1.0.8 does
        uint32_t j = 0;
        while (j < n_groups && bz_get(b, 1)) j++;
        if (j >= n_groups || b.pos > b.nbits) return E_CORRUPT;
        if (i < BZ_MAX_SEL) S.sel[i] = (uint8_t)j;
    }
    const uint32_t n_sel = n_sel_read < BZ_MAX_SEL ? n_sel_read : BZ_MAX_SEL;
    for (uint32_t g = 0; g < 6; g++) S.pos[g] = (uint8_t)g;
    for (uint32_t i = 0; i < n_sel; i++) {
        uint32_t v = S.sel[i];
        const uint8_t t = S.pos[v];
        for (; v > 0; v--) S.pos[v] = S.pos[v - 1];
        S.pos[0] = t;
        S.sel[i] = t;
    }
    // the delta-coded code lengths; every step of the walk consumes a bit, and zeros behind the input end it
    for (uint32_t t = 0; t < n_groups; t++) {
        uint32_t curr = bz_get(b, 5);
        for (uint32_t i = 0; i < alpha; i++) {
            uint32_t more = 1;
            while (more) {
                if (curr < 1 || curr > BZ_MAX_LEN) return E_CORRUPT;
                if (!bz_get(b, 1)) more = 0;
                else curr += bz_get(b, 1) ? -1 : 1;
            }
            S.len[t][i] = (uint8_t)curr;
        }
        if (b.pos > b.nbits) return E_CORRUPT;
    }
    // canonical tables; a code that claims more than the code space is over-subscribed
    for (uint32_t t = 0; t < n_groups; t++) {
        for (uint32_t l = 0; l <= BZ_MAX_LEN; l++) S.count[t][l] = 0;
        for (uint32_t i = 0; i < alpha; i++) S.count[t][S.len[t][i]]++;
        uint32_t code = 0, idx = 0, kraft = 0, min_len = 0;
        for (uint32_t l = 1; l <= BZ_MAX_LEN; l++) {
            const uint32_t c = S.count[t][l];
            S.first[t][l] = code;
            S.offs[t][l] = idx;
            S.fill[l] = idx;
            code = (code + c) << 1;
            idx += c;
            kraft += c << (BZ_MAX_LEN - l);
            if (c && !min_len) min_len = l;
        }
        if (kraft > (1u << BZ_MAX_LEN)) return E_CORRUPT;
        S.min_len[t] = min_len;
        for (uint32_t i = 0; i < alpha; i++) S.perm[t][S.fill[S.len[t][i]]++] = (uint16_t)i;
    }
    for (uint32_t i = 0; i < 256; i++) S.mtf[i] = (uint8_t)i;

    // the symbols.  Every iteration consumes at least one bit of input; `status` and `done` end the loop through its condition.
    uint32_t n = 0, group = 0, left = 0, t = 0, run = 0, weight = 1, done = 0;
    int status = 0;
    while (!done) {
        if (left == 0) {
            if (group >= n_sel) { status = E_CORRUPT; done = 1; }
            else { t = S.sel[group++]; left = BZ_GROUP; }
        }
        if (!done) {
            left--;
            const uint32_t v = bz_peek(b, BZ_MAX_LEN);
            uint32_t l = S.min_len[t];
            while (l <= BZ_MAX_LEN && (v >> (BZ_MAX_LEN - l)) - S.first[t][l] >= S.count[t][l]) l++;
            if (l > BZ_MAX_LEN) { status = E_CORRUPT; done = 1; }  // a bit pattern no code has
            else {
                b.pos += l;
                const uint32_t sym = S.perm[t][S.offs[t][l] + (v >> (BZ_MAX_LEN - l)) - S.first[t][l]];
                if (b.pos > b.nbits) { status = E_CORRUPT; done = 1; }
                else if (sym <= 1) {  // RUNA, RUNB: weight <= 2^20 while the run stays within a block
                    run += (sym + 1) * weight;
                    weight <<= 1;
                    if (run > BZ_BLOCK_MAX) { status = E_CORRUPT; done = 1; }
                } else {
                    if (run) {
                        const uint8_t uc = S.seq[S.mtf[0]];
                        if (run > BZ_BLOCK_MAX - n) { status = E_CORRUPT; done = 1; }
                        else {
                            for (uint32_t k = 0; k < run; k++) bytes[n + k] = uc;
                            n += run;
                        }
                        run = 0;
                        weight = 1;
                    }
                    if (!done) {
                        if (sym == eob) done = 1;
                        else if (n >= BZ_BLOCK_MAX) { status = E_CORRUPT; done = 1; }
                        else {
                            uint32_t k = sym - 1;
                            const uint8_t at = S.mtf[k];
                            for (; k > 0; k--) S.mtf[k] = S.mtf[k - 1];
                            S.mtf[0] = at;
                            bytes[n++] = S.seq[at];
                        }
                    }
                }
            }
        }
    }
    if (status == 0 && r.orig >= n) status = E_CORRUPT;  // (a block of no symbols among them)
    r.n = n;
    return status;
}

__device__ __forceinline__ bool is_splitter(uint32_t p, uint32_t orig, uint32_t split, bool multi) { return p == orig || (multi && p % split == 0); }

}  // namespace

__global__ __launch_bounds__(64) void k_bunzip2_scan(const BzItem *items, const BzChunk *chunks, uint32_t n_chunks, uint32_t *count, uint64_t *cands, uint32_t cap) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t item = chunks[c].item, off = chunks[c].off;
        const uint8_t *const src = (const uint8_t *)(const glb8 *)(uint64_t)items[item].src;
        const uint64_t n = items[item].src_len;
        for (uint32_t j = 0; j < BZ_SCAN_CHUNK; j += 64) {
            const uint64_t q = (uint64_t)off + j + lane;
            if (q + 6 <= n) {  // (a magic that starts in byte q has its last bit in byte q + 5 or q + 6)
                const uint64_t v = bz_load56(src, n, q);
                for (uint32_t s = 0; s < 8; s++) {
                    const uint64_t m = (v << s) >> 16;
                    if ((uint32_t)(m >> 24) == BZ_MAGIC_HI && (uint32_t)(m & 0xFFFFFFu) == BZ_MAGIC_LO && 8 * q + s + 48 <= 8 * n) {
                        const uint32_t i = atomicAdd(count, 1u);
                        if (i < cap) cands[i] = (uint64_t)item << 36 | (8 * q + s);  // (cap is the bound on all starts, host/bz_plan.h: always true)
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(64) void k_bunzip2_decode(const BzItem *items, const BzJob *jobs, uint32_t n_jobs, BzRec *recs, uint8_t *scratch) {
    __shared__ BzLds S;
    const uint32_t lane = threadIdx.x;
    for (uint32_t j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        __syncthreads();
        if (lane == 0) {
            const BzJob job = jobs[j];
            const uint8_t *const src = (const uint8_t *)(const glb8 *)(uint64_t)items[job.item].src;
            uint8_t *const bytes = (uint8_t *)(glb8 *)(uint64_t)(scratch + (size_t)job.slot * BZ_SLOT_BYTES + BZ_SLOT_BYTES_OFF);
            BzBits b{src, 8 * (uint64_t)items[job.item].src_len, 0};
            BzRec r;
            r.status = 0; r.next = 0; r.end_bit = 0; r.after = 0; r.n = 0; r.level = 0; r.block_crc = 0; r.stream_crc = 0; r.tail = 0; r.tail_len = 0;
            r.out_len = 0; r.orig = 0;
            if (job.kind == K_HEAD) {
                b.pos = 8 * job.pos;
                const uint32_t h = bz_get(b, 32);
                r.level = (h & 255u) - '0';
                if (b.pos > b.nbits || (h >> 8) != 0x425A68u || r.level < 1 || r.level > 9) r.status = E_CORRUPT;
            } else {
                b.pos = job.pos + 48;
                r.status = b.pos > b.nbits ? E_CORRUPT : bz_block(S, b, bytes, r);
            }
            r.end_bit = b.pos;
            if (r.status == 0) r.status = bz_behind(b, r);
            recs[j] = r;
        }
    }
}

__global__ __launch_bounds__(256) void k_bunzip2_walk(const BzJob *jobs, uint32_t n_jobs, BzRec *recs, uint8_t *scratch, uint32_t split_in) {
    __shared__ uint32_t cnt[256 * SORT_SLICES];  // [byte][slice]
    __shared__ uint32_t base[256], sl_len[BZ_SLICES], sl_state[BZ_SLICES];
    __shared__ uint32_t sh_cycle;
    const uint32_t tid = threadIdx.x;
    for (uint32_t j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        __syncthreads();
        // (one value each for the whole workgroup)
        const uint32_t n = recs[j].n, orig = recs[j].orig;
        if (jobs[j].kind == K_BLOCK && recs[j].status == 0 && n >= 1 && n <= BZ_BLOCK_MAX && orig < n) {
            uint8_t *const slot = (uint8_t *)(glb8 *)(uint64_t)(scratch + (size_t)jobs[j].slot * BZ_SLOT_BYTES);
            uint8_t *const bytes = slot + BZ_SLOT_BYTES_OFF;
            uint32_t *const tt = (uint32_t *)(slot + BZ_SLOT_TT_OFF);
            uint8_t *const out = slot + BZ_SLOT_OUT_OFF;
            // (a) tt[j] = successor << 8 | bytes[j], the successors by a stable counting sort of the bytes
            for (uint32_t i = tid; i < 256 * SORT_SLICES; i += 256) cnt[i] = 0;
            __syncthreads();
            const uint32_t s0 = (uint32_t)((uint64_t)n * tid / SORT_SLICES), s1 = (uint32_t)((uint64_t)n * (tid + 1) / SORT_SLICES);
            if (tid < SORT_SLICES)
                for (uint32_t i = s0; i < s1; i++) cnt[bytes[i] * SORT_SLICES + tid]++;
            __syncthreads();
            {
                uint32_t sum = 0;  // thread = byte value: its slices' counts become their first places among the equal bytes
                for (uint32_t s = 0; s < SORT_SLICES; s++) {
                    const uint32_t c = cnt[tid * SORT_SLICES + s];
                    cnt[tid * SORT_SLICES + s] = sum;
                    sum += c;
                }
                base[tid] = sum;
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t sum = 0;
                for (uint32_t v = 0; v < 256; v++) {
                    const uint32_t c = base[v];
                    base[v] = sum;
                    sum += c;
                }
            }
            __syncthreads();
            if (tid < SORT_SLICES)
                for (uint32_t i = s0; i < s1; i++) {
                    const uint32_t v = bytes[i];
                    tt[base[v] + cnt[v * SORT_SLICES + tid]++] = i << 8;  // (a place below n: the counts add up to n)
                }
            __syncthreads();
            for (uint32_t i = tid; i < n; i += 256) tt[i] |= bytes[i];
            __syncthreads();
            // (b) the chain from tt[orig], sublist by sublist.  The byte area is free now: the splitter lists take it.
            const uint32_t split = split_in < BZ_SPLIT_MIN ? BZ_SPLIT_MIN : split_in;
            const bool multi = split < n;
            const uint32_t n_mult = multi ? (n + split - 1) / split : 0, n_spl = n_mult + 1;  // id n_mult: origPtr
            uint32_t *const spl_next = (uint32_t *)bytes, *const spl_len = spl_next + n_spl, *const spl_off = spl_len + n_spl;
            for (uint32_t id = tid; id < n_spl; id += 256) {
                uint32_t p = id == n_mult ? orig : id * split, len = 0;
                uint32_t e = tt[p];
                do {
                    p = e >> 8;
                    e = tt[p];
                    len++;
                } while (!is_splitter(p, orig, split, multi) && len < n);
                spl_next[id] = p == orig || !multi ? n_mult : p / split;
                spl_len[id] = len;
                spl_off[id] = 0xFFFFFFFFu;
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t id = n_mult, at = 0, seen = 0;
                do {
                    spl_off[id] = at;
                    at += spl_len[id];
                    id = spl_next[id];
                    seen++;
                } while (id != n_mult && id < n_spl && seen < n_spl && at < n);
                sh_cycle = at < n ? at : n;
            }
            __syncthreads();
            const uint32_t cycle = sh_cycle;
            for (uint32_t id = tid; id < n_spl; id += 256) {
                const uint32_t at = spl_off[id], len = spl_len[id];
                if (at != 0xFFFFFFFFu) {
                    uint32_t e = tt[id == n_mult ? orig : id * split];
                    for (uint32_t k = 0; k < len && at + k < n; k++) {
                        e = tt[e >> 8];
                        out[at + k] = (uint8_t)e;
                    }
                }
            }
            __syncthreads();
            for (uint32_t k = cycle + tid; k < n; k += 256) out[k] = out[k % cycle];  // (the chain closed early: a periodic block)
            __syncthreads();
            // (c) the final run-length step, lengths only.  State: run (bytes of the current run seen, 4: a count follows) and last.
            {
                const uint32_t a = (uint32_t)((uint64_t)n * tid / BZ_SLICES), e = (uint32_t)((uint64_t)n * (tid + 1) / BZ_SLICES);
                uint32_t run = 0, last = 0, total = 0;
                if (a < e) {
                    uint32_t k = a;  // back to where a byte is known to start a run (or to the block's first byte)
                    while (k >= 2 && !(out[k] != out[k - 1] && out[k - 1] != out[k - 2])) k--;
                    if (k < 2) k = 0;
                    for (; k < a; k++) {
                        const uint32_t v = out[k];
                        if (run == 4) run = 0;
                        else if (run > 0 && v == last) run++;
                        else { last = v; run = 1; }
                    }
                }
                sl_state[tid] = run | last << 8;
                for (uint32_t k = a; k < e; k++) {
                    const uint32_t v = out[k];
                    if (run == 4) { total += v; run = 0; }
                    else {
                        total++;
                        if (run > 0 && v == last) run++;
                        else { last = v; run = 1; }
                    }
                }
                sl_len[tid] = total;
            }
            __syncthreads();
            if (tid == 0) {
                BzSlice *const tab = (BzSlice *)tt;  // (tt is done with)
                uint32_t sum = 0;
                for (uint32_t s = 0; s < BZ_SLICES; s++) {
                    tab[s].off = sum;
                    tab[s].state = sl_state[s];
                    sum += sl_len[s];
                }
                recs[j].out_len = sum;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_bunzip2_expand(const BzItem *items, const BzLand *lands, uint32_t n_lands, const uint8_t *scratch) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t l = blockIdx.x; l < n_lands; l += gridDim.x) {
        const BzLand land = lands[l];
        const uint8_t *const slot = (const uint8_t *)(const glb8 *)(uint64_t)(scratch + (size_t)land.slot * BZ_SLOT_BYTES);
        const uint8_t *const out = slot + BZ_SLOT_OUT_OFF;
        const BzSlice sl = ((const BzSlice *)(slot + BZ_SLOT_TT_OFF))[tid];
        uint8_t *const dst = (uint8_t *)(glb8 *)(uint64_t)(items[land.item].dst + land.out_off);
        const uint32_t n = land.n < BZ_BLOCK_MAX ? land.n : BZ_BLOCK_MAX, lim = land.out_len;
        const uint32_t a = (uint32_t)((uint64_t)n * tid / BZ_SLICES), e = (uint32_t)((uint64_t)n * (tid + 1) / BZ_SLICES);
        uint32_t run = sl.state & 255u, last = sl.state >> 8 & 255u, o = sl.off;
        for (uint32_t k = a; k < e; k++) {
            const uint32_t v = out[k];
            if (run == 4) {
                for (uint32_t c = 0; c < v; c++, o++)
                    if (o < lim) dst[o] = (uint8_t)last;
                run = 0;
            } else {
                if (o < lim) dst[o] = (uint8_t)v;
                o++;
                if (run > 0 && v == last) run++;
                else { last = v; run = 1; }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_bunzip2_crc(const BzItem *items, const BzLand *lands, uint32_t n_lands, uint32_t *crc_out) {
    __shared__ uint32_t T[256], red[256];
    const uint32_t tid = threadIdx.x;
    {
        uint32_t c = tid;
        for (int k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ CRC_POLY : c >> 1;
        T[tid] = c;
    }
    __syncthreads();
    for (uint32_t l = blockIdx.x; l < n_lands; l += gridDim.x) {
        const uint8_t *const p = (const uint8_t *)(const glb8 *)(uint64_t)(items[lands[l].item].dst + lands[l].out_off);
        const uint64_t len = lands[l].out_len;
        const uint64_t seg = (len + 255) >> 8;
        // 256 segments of `seg` bytes, aligned to the END of the block (k_inflate_crc's split); every byte bit-reversed on its way in
        int64_t a = (int64_t)len - (int64_t)(256 - tid) * (int64_t)seg, e = a + (int64_t)seg;
        if (a < 0) a = 0;
        if (e < 0) e = 0;
        uint32_t crc = 0xFFFFFFFFu;
        for (; a < e; a++) crc = T[(crc ^ (__brev((uint32_t)p[a]) >> 24)) & 255] ^ (crc >> 8);
        red[tid] = ~crc;
        __syncthreads();
        uint32_t pw = crc_xpow(8 * seg);
        for (uint32_t stride = 1; stride < 256; stride <<= 1) {
            if ((tid & (2 * stride - 1)) == 0) red[tid] = crc_mulmod(pw, red[tid]) ^ red[tid + stride];
            __syncthreads();
            pw = crc_mulmod(pw, pw);
        }
        if (tid == 0) crc_out[l] = __brev(red[0]);
        __syncthreads();
    }
}

void launch_bunzip2_scan(const BzItem *items, const BzChunk *chunks, uint32_t n_chunks, uint32_t *count, uint64_t *cands, uint32_t cap, hipStream_t s) {
    if (n_chunks) hipLaunchKernelGGL(k_bunzip2_scan, dim3(n_chunks < 65536u ? n_chunks : 65536u), dim3(64), 0, s, items, chunks, n_chunks, count, cands, cap);
}
void launch_bunzip2_decode(const BzItem *items, const BzJob *jobs, uint32_t n_jobs, BzRec *recs, uint8_t *scratch, hipStream_t s) {
    if (n_jobs) hipLaunchKernelGGL(k_bunzip2_decode, dim3(n_jobs < 65536u ? n_jobs : 65536u), dim3(64), 0, s, items, jobs, n_jobs, recs, scratch);
}
void launch_bunzip2_walk(const BzJob *jobs, uint32_t n_jobs, BzRec *recs, uint8_t *scratch, uint32_t split, hipStream_t s) {
    if (n_jobs) hipLaunchKernelGGL(k_bunzip2_walk, dim3(n_jobs < 65536u ? n_jobs : 65536u), dim3(256), 0, s, jobs, n_jobs, recs, scratch, split);
}
void launch_bunzip2_expand(const BzItem *items, const BzLand *lands, uint32_t n_lands, const uint8_t *scratch, hipStream_t s) {
    if (n_lands) hipLaunchKernelGGL(k_bunzip2_expand, dim3(n_lands < 65536u ? n_lands : 65536u), dim3(256), 0, s, items, lands, n_lands, scratch);
}
void launch_bunzip2_crc(const BzItem *items, const BzLand *lands, uint32_t n_lands, uint32_t *crc, hipStream_t s) {
    if (n_lands) hipLaunchKernelGGL(k_bunzip2_crc, dim3(n_lands < 65536u ? n_lands : 65536u), dim3(256), 0, s, items, lands, n_lands, crc);
}

}  // namespace zn
