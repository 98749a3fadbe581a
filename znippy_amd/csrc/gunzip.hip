// Whole gzip files (znippy_gunzip_batch): every member of every item inflated to the item's room, CRC-32 and ISIZE checked.  The
// DEFLATE decoder of inflate_dev.h is one wave per stream and serial; what makes a big file fast is that a file can be cut where its
// writer flushed.  Behind the empty stored block 00 00 FF FF that a flush leaves, symbol decoding needs nothing from before it, and
// gzip members are independent altogether.  Four launches, with the host's plan (host/gz_plan.{h,cc}) between the second and third:
//
//   scan     wave = 4 KiB of source: every position behind 00 00 FF FF (a flush candidate) and every 1F 8B 08 (a member candidate)
//            is appended to its item's list.  The host sorts the list, drops flush candidates closer than seg_min to the one kept
//            before, and gives every kept candidate a wave of the probe.
//   probe    wave = kept candidate.  A member candidate parses its header (tar_rules.h: gzip_header).  The wave then decodes symbols
//            and stored-block lengths and writes nothing (inflate_dev.h: probe_body): it records where it ended — at the first block
//            boundary that is a kept flush candidate behind it, at its member's trailer (whose CRC-32 and ISIZE it reads, with what
//            follows the zero padding behind them), in an error, or beyond the item's room —, the bytes it would produce and the
//            longest reach of a match in front of its first byte.  A candidate the pattern search found inside compressed or stored
//            data decodes garbage up to one of those ends; the room bounds that, and the plan never lands on its record.
//   inflate  wave = run of the plan: the real decoder (inflate_body) from the run's first DEFLATE byte into its final place, ended by
//            a hook once the run's exact byte count exists.
//   crc      inflate.hip's k_inflate_crc over the runs.
//
// An item the scan finds no candidate in (one member, no flush: a crate, an sdist) is not probed: one wave decodes it with the room as
// its limit and checks the trailer and the padding (single); its CRC-32 goes to the crc launch.  The same wave walks an item member by
// member when its candidates overflowed its slice of the list, so that correctness never depends on what the scan could keep; the
// CRC-32 of a member behind the first it folds itself.
// The crc launch takes a member run by run — a long member is many workgroups' work — and the host combines the runs' CRCs
// (gz_plan: crc32_combine) before it compares with the trailer.
// Control flow, bounds and address spaces follow inflate.hip: steering values are wave-uniform, every loop iteration consumes input or
// produces a byte, a failed check sets a status and loops end through their conditions.
//
// With znippy_ctx_set_gunzip_cut further launches run between scan and probe, for the files that have nothing of the above to be cut
// at (host/gz_cut_plan.h has the plan between them; an item they finish is left out of probe, single and inflate):
//   find     lane = bit position of an item of at least 2 * cut source bytes: is it the start of a non-final dynamic block with a
//            valid header (gz_cut_rules.h)?  The lowest passing position of every window of cut source bytes is kept in the window's
//            slot.  Slots and the count of passing positions are set by memsets in front of the launch.
//   probe    wave = kept candidate or byte 0: probe_cut_body, a piece from any bit to the first block that starts at a kept candidate
//   decode   wave = piece: into place (inflate_body), or, where the piece reaches back, into 16-bit symbols (inflate_marks) in which
//            MARK | k stands for byte k of the 32,768 in front of the piece
//   tails    workgroup = an item's pieces of the pass in chain order: the last 32 KiB of each marker piece made bytes
//   apply    lane = symbol: the rest of each marker piece made bytes
//   crc      k_inflate_crc over the pieces
// Who writes what: a record per candidate by the probe; a status per piece and, for a marker piece, its out_len symbols by decode
// (fewer if it fails: tails and apply then read what the scratch held, bounded to the item's room, and the item is decoded again by
// the launches behind); *resolved is set by a memset and added to.
//
// Not done here: xz.  (bzip2 files: bunzip2.hip; listing the members of the tar inside: tar_list.hip.)
#include "gz_cut_rules.h"
#include "inflate_dev.h"
#include "tar_rules.h"

namespace zn {

namespace {

// gzp::K_*, END_*, NEXT_* of host/gz_plan.h
constexpr uint32_t K_MEMBER = 1;
constexpr uint32_t END_BOUNDARY = 0, END_TRAILER = 1, END_ERROR = 2, END_ROOM = 3;
constexpr int32_t NEXT_MEMBER = 0, NEXT_END = 1;

struct Trailer {
    uint32_t crc, isize;
    uint64_t after;  // the first non-zero byte behind the trailer, or n
    int32_t next;    // NEXT_END, NEXT_MEMBER (a member header that gzip_header accepts starts at `after`), or the status of what is there
};

// the header of the member at src[at ..): 0 and *data = its first DEFLATE byte, or the status
__device__ int member_header(const uint8_t *src, uint64_t n, uint64_t at, uint32_t lane, uint64_t *data) {
    uint64_t off = 0;
    int g = 0;
    if (lane == 0) g = tr::gzip_header(tr::MemRd{src + at}, n - at, &off);
    g = (int)uni((uint32_t)g);
    *data = at + uni64(off);
    return g == tr::GZ_OK ? 0 : g == tr::GZ_SHORT ? E_CORRUPT : g;
}

// end: the first byte behind a member's DEFLATE stream (<= n).  0, or E_CORRUPT: the eight bytes are not all there
__device__ int read_trailer(const uint8_t *src, uint64_t n, uint64_t end, uint32_t lane, Trailer *t) {
    if (end > n || n - end < 8) return E_CORRUPT;
    uint32_t v = 0;
    if (lane < 8) v = src[end + lane];
    t->crc = rdlane_u(v, 0) | rdlane_u(v, 1) << 8 | rdlane_u(v, 2) << 16 | rdlane_u(v, 3) << 24;
    t->isize = rdlane_u(v, 4) | rdlane_u(v, 5) << 8 | rdlane_u(v, 6) << 16 | rdlane_u(v, 7) << 24;
    uint64_t at = end + 8;
    uint32_t found = 0;
    while (at < n && !found) {  // (64 bytes of padding per iteration)
        const uint64_t q = at + lane;
        const uint64_t m = __ballot(q < n && src[q] != 0);
        if (m) {
            at += (uint32_t)__ffsll((long long)m) - 1;
            found = 1;
        } else {
            at = n - at < 64 ? n : at + 64;
        }
    }
    at = uni64(at);
    t->after = at;
    if (at == n) {
        t->next = NEXT_END;
    } else {
        uint64_t data;
        const int h = member_header(src, n, at, lane, &data);
        t->next = h == 0 ? NEXT_MEMBER : h;
    }
    return 0;
}

// CRC-32 of p[0 .. len), bytes this wave has stored (behind a wave_mem_sync): k_inflate_crc's scheme with 64 segments
__device__ uint32_t wave_crc(const uint32_t *T, uint32_t *red, const uint8_t *p, uint64_t len, uint32_t lane) {
    const uint64_t seg = (len + 63) >> 6;
    int64_t a = (int64_t)len - (int64_t)(64 - lane) * (int64_t)seg, e = a + (int64_t)seg;
    if (a < 0) a = 0;
    if (e < 0) e = 0;
    uint32_t crc = 0xFFFFFFFFu;
    for (; a < e; a++) crc = T[(crc ^ p[a]) & 255] ^ (crc >> 8);
    __syncthreads();
    red[lane] = ~crc;
    __syncthreads();
    uint32_t pw = crc_xpow(8 * seg);
    for (uint32_t stride = 1; stride < 64; stride <<= 1) {
        if ((lane & (2 * stride - 1)) == 0) red[lane] = crc_mulmod(pw, red[lane]) ^ red[lane + stride];
        __syncthreads();
        pw = crc_mulmod(pw, pw);
    }
    return uni(red[0]);
}

}  // namespace

__global__ __launch_bounds__(64) void k_gunzip_scan(const GzItem *items, const GzScanChunk *chunks, uint32_t n_chunks, uint32_t *count, uint64_t *cands) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t item = chunks[c].item, off = chunks[c].off;
        const uint8_t *const src = (const uint8_t *)(const glb8 *)(uint64_t)items[item].src;
        const uint64_t n = items[item].src_len;
        const uint32_t base = items[item].cand_base, cap = items[item].cand_cap;
        for (uint32_t j = 0; j < GZ_SCAN_CHUNK; j += 64) {
            const uint64_t q = (uint64_t)off + j + lane;
            if (q >= 1 && q < n) {
                // the four bytes in front of q and the three from q on, where they exist
                uint32_t before = 0, after = 0;
                if (q >= 4 && q + 4 <= n) {
                    uint64_t v;
                    __builtin_memcpy(&v, src + q - 4, 8);
                    before = (uint32_t)v;
                    after = (uint32_t)(v >> 32) & 0xFFFFFFu;
                } else {
                    if (q >= 4)
                        for (uint32_t k = 0; k < 4; k++) before |= (uint32_t)src[q - 4 + k] << (8 * k);
                    if (q + 3 <= n)
                        for (uint32_t k = 0; k < 3; k++) after |= (uint32_t)src[q + k] << (8 * k);
                }
                const bool flush = q >= 4 && before == 0xFFFF0000u, member = q + 3 <= n && after == 0x088B1Fu;
                if (flush) {
                    const uint32_t i = atomicAdd(&count[item], 1u);
                    if (i < cap) cands[(uint64_t)base + i] = q << 1;
                }
                if (member) {
                    const uint32_t i = atomicAdd(&count[item], 1u);
                    if (i < cap) cands[(uint64_t)base + i] = q << 1 | K_MEMBER;
                }
            }
        }
    }
}

// The block-start search: wave = FIND_CHUNK source bytes of a searched item, lane = one byte of 64 at a time, whose eight bit
// positions it puts to the 13-bit test one after the other.  About one position in nine passes that; the survivors are gathered in
// LDS, and whenever 64 of them wait every lane takes one through the whole header test, so that the divergent part runs with full
// waves.  A position that passes lowers the slot of its window: the order in which waves and lanes arrive does not matter.
// Every read goes through gzc::load64, which reads no byte at or past n; a slot index is below the item's slot count since the
// position's byte is below n.
__global__ __launch_bounds__(64) void k_gunzip_find(const gzcut::FindItem *items, const gzcut::FindChunk *chunks, uint32_t n_chunks, uint32_t cut,
                                                    unsigned long long *slots, unsigned long long *passed) {
    __shared__ uint64_t queue[128];  // fewer than 64 wait when up to 64 more arrive
    const uint32_t lane = threadIdx.x;
    const uint64_t below = (1ull << lane) - 1;
    uint32_t npass = 0;
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        __syncthreads();
        const uint32_t item = uni(chunks[c].item), off = uni(chunks[c].off);
        const uint8_t *const src = (const uint8_t *)(const glb8 *)uni64((uint64_t)items[item].src);
        const uint64_t n = uni(items[item].src_len);
        unsigned long long *const slot = slots + uni64(items[item].slot_base);
        uint32_t cnt = 0;  // survivors waiting (wave-uniform)
        for (uint32_t j = 0; j < gzcut::FIND_CHUNK && (uint64_t)off + j < n; j += 64) {
            const uint64_t q = (uint64_t)off + j + lane;
            const uint64_t v = q < n ? gzc::load64(src, n, q) : 0;
            for (uint32_t s = 0; s < 8; s++) {
                const bool ok = q < n && gzc::quick13((uint32_t)(v >> s) & 0x1FFFu);
                const uint64_t m = __ballot(ok);
                if (ok) queue[cnt + (uint32_t)__popcll(m & below)] = 8 * q + s;
                cnt += (uint32_t)__popcll(m);
                if (cnt >= 64) {
                    __syncthreads();
                    const uint64_t bit = queue[lane];
                    const uint64_t rest = queue[64 + lane];  // (read by all: only the first cnt - 64 mean anything)
                    __syncthreads();
                    queue[lane] = rest;
                    cnt -= 64;
                    if (gzc::block_start(src, n, bit)) {
                        npass++;
                        atomicMin(&slot[(uint32_t)(bit >> 3) / cut], (unsigned long long)bit);
                    }
                    __syncthreads();
                }
            }
        }
        __syncthreads();
        if (lane < cnt) {
            const uint64_t bit = queue[lane];
            if (gzc::block_start(src, n, bit)) {
                npass++;
                atomicMin(&slot[(uint32_t)(bit >> 3) / cut], (unsigned long long)bit);
            }
        }
    }
    if (npass) atomicAdd(passed, (unsigned long long)npass);
}

// ---- cutting at the block starts found (host/gz_cut_plan.h) ----------------------------------------------------------------------

namespace {

// the bit reader seated at bit position `bit` of src[0 .. n): the bits of the first byte behind it are in the buffer
__device__ void seat(BitIn &b, const uint8_t *src, uint8_t *win, uint64_t n, uint64_t bit) {
    const uint64_t byte = bit >> 3;
    const uint32_t s = (uint32_t)bit & 7u;
    b.src = src; b.win = win; b.n = n; b.bb = 0; b.bc = 0; b.ip = byte;
    if (s) {
        const uint32_t v = uni(byte < n ? (uint32_t)src[byte] : 0u);
        b.ip = byte + 1; b.bb = v >> s; b.bc = 8 - s;  // (1 .. 7 bits: refill's arithmetic holds below 8)
    }
    b.wbase = b.ip;
}

// probe_body (inflate_dev.h) for a piece that may start at any bit and ends at any block boundary: stops[0 .. n_stops) are ascending
// bit positions, and the loop ends in front of the first block behind the piece's first whose header starts at one of them
// (PROBE_BOUNDARY; *end_bit is that position).  reach: matches may reach in front of the first byte (up to 32,768: no distance is longer).
__device__ int probe_cut_body(InflLds &S, BitIn &b, uint64_t limit, const uint64_t *stops, uint32_t n_stops, bool reach_ok, uint32_t lane, uint64_t *produced,
                              uint32_t *reach, uint32_t *how, uint64_t *end_bit) {
    constexpr int TR = E_INPUT_END;
    b.load_win(lane);
    const Code lc = {S.lt, S.lsym, S.lcnt, (1u << LB) - 1}, dc = {S.dt, S.dsym, S.dcnt, (1u << DB) - 1};
    int st = 0;
    uint64_t pos = 0;
    uint32_t far = 0, si = 0, blocks = 0;
    uint32_t done = 0, fixed_built = 0, stop = 0;
    while (!done && !stop && st == 0) {
        b.refill(lane);
        const uint64_t here = b.ip * 8 - b.bc;
        // (the list is walked forward once over the whole piece: the positions only grow)
        while (si < n_stops && uni64(stops[si]) < here) si++;
        if (blocks && si < n_stops && uni64(stops[si]) == here) {
            stop = PROBE_BOUNDARY;
            *end_bit = here;
        } else {
            blocks++;
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
                        if (final_block) done = 1;
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
                                } else if (ds > 29 || (!reach_ok && dist > pos)) {
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
    }
    *produced = pos;
    *reach = far;
    *how = stop;
    return st;
}

// inflate_body for a marker piece: the stream behind `b` into 16-bit symbols sym[0 .. out_len), the piece's exact count, at which the
// loop ends.  A literal or a stored byte is its value; a match copies symbols, markers among them, and where it reaches in front of
// the piece's first symbol it leaves markers: MARK | k for byte k of the 32,768 in front of the piece.  Output i of a match is source
// i mod dist (an overlapping match is its period repeated), and every source lies in front of the match: no lane reads what another
// writes.  No symbol is written at or beyond out_len; anything that would need one is E_CORRUPT (the probe counted these symbols).
__device__ int inflate_marks(InflLds &S, BitIn &b, uint16_t *sym, uint32_t out_len, uint32_t lane, uint32_t *produced) {
    constexpr int TR = E_CORRUPT;
    b.load_win(lane);
    const Code lc = {S.lt, S.lsym, S.lcnt, (1u << LB) - 1}, dc = {S.dt, S.dsym, S.dcnt, (1u << DB) - 1};
    int st = 0;
    uint32_t pos = 0, nlit = 0, mylit = 0;  // lane k holds sym[pos - nlit + k], as in inflate_body
    uint32_t done = 0, fixed_built = 0;
    while (!done && pos < out_len && st == 0) {
        b.refill(lane);
        const uint32_t final_block = b.take(1), type = b.take(2);
        if (b.over()) {
            st = TR;
        } else if (type == 3) {
            st = E_CORRUPT;
        } else if (type == 0) {
            if (lane < nlit) sym[pos - nlit + lane] = (uint16_t)mylit;
            nlit = 0;
            b.drop(b.bc & 7);
            b.refill(lane);
            const uint32_t len = b.take(16), nlen = b.take(16);
            if (b.over()) {
                st = TR;
            } else if (len != (nlen ^ 0xFFFFu)) {
                st = E_CORRUPT;
            } else {
                const uint64_t at = b.ip - (b.bc >> 3);
                if (len > b.n - at || len > out_len - pos) {
                    st = E_CORRUPT;
                } else {
                    for (uint32_t i = lane; i < len; i += 64) sym[pos + i] = b.src[at + i];
                    pos += len;
                    b.ip = at + len; b.bb = 0; b.bc = 0;
                    if (final_block) done = 1;
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
            while (!eob && pos < out_len && st == 0) {
                b.refill(lane);
                uint32_t l = 0;
                const uint32_t s = decode_sym(lc, b.bb, &l);
                if (s == NO_SYM) {
                    st = E_CORRUPT;
                } else if (s < 256) {
                    b.drop(l);
                    if (b.over()) {
                        st = TR;
                    } else {
                        if (lane == nlit) mylit = s;
                        nlit++;
                        pos++;
                        if (nlit == 64) {
                            sym[pos - 64 + lane] = (uint16_t)mylit;
                            nlit = 0;
                        }
                    }
                } else if (s == 256) {
                    b.drop(l);
                    if (b.over()) st = TR;
                    else eob = 1;
                } else {
                    b.drop(l);
                    if (b.over()) {
                        st = TR;
                    } else if (s > 285) {
                        st = E_CORRUPT;
                    } else {
                        const uint32_t i = s - 257;
                        const uint32_t lx = i < 8 || i == 28 ? 0u : (i - 4) >> 2;
                        const uint32_t len = (i < 8 ? 3 + i : i == 28 ? 258u : 3 + ((4 + (i & 3)) << lx)) + b.take(lx);
                        uint32_t dl = 0;
                        const uint32_t ds = decode_sym(dc, b.bb, &dl);
                        if (ds == NO_SYM) {
                            st = E_CORRUPT;
                        } else {
                            b.drop(dl);
                            const uint32_t dx = ds < 4 ? 0u : (ds - 2) >> 1;
                            const uint32_t dist = (ds < 4 ? 1 + ds : 1 + ((2 + (ds & 1)) << dx)) + (ds > 29 ? 0u : b.take(dx));
                            if (b.over()) {
                                st = TR;
                            } else if (ds > 29 || len > out_len - pos) {  // (dist <= 32,768: a marker names every byte it can reach)
                                st = E_CORRUPT;
                            } else {
                                if (lane < nlit) sym[pos - nlit + lane] = (uint16_t)mylit;
                                nlit = 0;
                                wave_mem_sync();  // the source symbols are this wave's earlier stores
                                for (uint32_t k = lane; k < len; k += 64) {
                                    const uint32_t j = dist >= len ? k : k % dist;
                                    const int32_t p = (int32_t)pos - (int32_t)dist + (int32_t)j;  // (below pos; at least -32,768)
                                    sym[pos + k] = p < 0 ? (uint16_t)(gzcut::MARK | (uint32_t)((int32_t)gzcut::WINDOW + p)) : sym[p];
                                }
                                pos += len;
                            }
                        }
                    }
                }
            }
            if (st == 0 && eob && final_block) done = 1;
        }
    }
    if (lane < nlit) sym[pos - nlit + lane] = (uint16_t)mylit;  // (below out_len: pos is)
    *produced = pos;
    return st;
}

// a symbol of a marker piece whose first byte is dst[off] -> its byte; a marker that names a byte in front of the room reads as 0
// (the plan refuses a reach beyond the room's first byte: only symbols of a piece that failed can say so)
__device__ __forceinline__ uint32_t cut_byte(const uint8_t *dst, uint32_t off, uint32_t v, uint32_t *n_marks) {
    if (!(v & gzcut::MARK)) return v & 255u;
    (*n_marks)++;
    const int64_t at = (int64_t)off - (int64_t)gzcut::WINDOW + (int64_t)(v & 0x7FFFu);  // (below off)
    return at >= 0 ? (uint32_t)dst[at] : 0u;
}

}  // namespace

__global__ __launch_bounds__(64) void k_gunzip_cut_probe(const GzItem *items, const gzcut::CutCand *cands, uint32_t n_cands, const uint64_t *stops,
                                                         gzcut::CutRec *recs) {
    __shared__ InflLds S;
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < n_cands; c += gridDim.x) {
        __syncthreads();
        const uint32_t item = uni(cands[c].item), first = uni(cands[c].first), stop0 = uni(cands[c].stop0), stop1 = uni(cands[c].stop1);
        const uint8_t *const src = (const uint8_t *)(const glb8 *)uni64((uint64_t)items[item].src);
        const uint64_t n = uni(items[item].src_len), room = uni(items[item].room);
        gzcut::CutRec r;
        r.start_bit = uni64(cands[c].bit); r.end_bit = 0; r.out = 0; r.end_kind = END_ERROR; r.status = 0; r.reach = 0; r.crc = 0; r.isize = 0; r.next = 0;
        if (first) {
            uint64_t data = 0;
            r.status = r.start_bit >> 3 < n ? member_header(src, n, r.start_bit >> 3, lane, &data) : E_CORRUPT;
            r.start_bit = data * 8;
        }
        if (r.status == 0) {
            BitIn b;
            seat(b, src, S.in, n, r.start_bit);
            uint32_t how = 0;
            const uint64_t *const st = (const uint64_t *)(const __attribute__((address_space(1))) uint64_t *)(uint64_t)(stops + stop0);
            const int rc = probe_cut_body(S, b, room, st, stop1 - stop0, !first, lane, &r.out, &r.reach, &how, &r.end_bit);
            if (rc != 0) {
                r.status = E_CORRUPT;
            } else if (how == PROBE_LIMIT) {
                r.end_kind = END_ROOM;
            } else if (how == PROBE_BOUNDARY) {
                r.end_kind = END_BOUNDARY;
            } else {
                Trailer t;
                if (read_trailer(src, n, b.ip - (b.bc >> 3), lane, &t) != 0) {
                    r.status = E_CORRUPT;
                } else {
                    r.end_kind = END_TRAILER;
                    r.end_bit = t.after * 8; r.crc = t.crc; r.isize = t.isize; r.next = t.next;
                }
            }
        }
        if (lane == 0) recs[c] = r;
    }
}

// wave = piece: a marker piece into its symbols of the pass's scratch, any other into its place
__global__ __launch_bounds__(64) void k_gunzip_cut_decode(const GzItem *items, const gzcut::CutPiece *pieces, uint32_t n_pieces, uint16_t *scratch, int32_t *status) {
    __shared__ InflLds S;
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = blockIdx.x; k < n_pieces; k += gridDim.x) {
        __syncthreads();
        const uint32_t item = uni(pieces[k].item), marker = uni(pieces[k].marker), out_len = uni(pieces[k].out_len);
        int st = 0;
        uint32_t pos = 0;
        if (out_len) {
            const uint8_t *const src = (const uint8_t *)(const glb8 *)uni64((uint64_t)items[item].src);
            BitIn b;
            seat(b, src, S.in, uni(items[item].src_len), uni64(pieces[k].start_bit));
            if (marker) {
                uint16_t *const sym = (uint16_t *)(__attribute__((address_space(1))) uint16_t *)uni64((uint64_t)(scratch + pieces[k].sym_off));
                st = inflate_marks(S, b, sym, out_len, lane, &pos);
            } else {
                uint8_t *const dst = (uint8_t *)(glb8 *)uni64((uint64_t)(items[item].dst + pieces[k].out_off));
                StopAt hook{out_len};
                st = inflate_body(S, b, dst, out_len, lane, hook, &pos);
            }
        }
        if (lane == 0) status[k] = st == 0 && pos == out_len ? 0 : E_CORRUPT;
    }
}

// workgroup = the pieces of one item in this pass, in chain order: the last 32 KiB of every marker piece become bytes in their final
// place.  A marker names a byte in front of the piece, which is final: it lies in the last 32 KiB of the pieces in front — made final
// by this loop one iteration earlier, by the decode launch (a piece decoded into place) or by an earlier pass.  The only serial loop
// is this one, inside one workgroup and bounded by the piece count; no workgroup waits for another.
__global__ __launch_bounds__(256) void k_gunzip_cut_tails(const GzItem *items, const gzcut::CutPiece *pieces, const gzcut::CutGroup *groups, uint32_t n_groups,
                                                          const uint16_t *scratch, unsigned long long *resolved) {
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const uint32_t p0 = groups[g].piece0, p1 = groups[g].piece1;
        for (uint32_t p = p0; p < p1; p++) {
            if (pieces[p].marker) {
                uint32_t marks = 0;
                uint8_t *const dst = items[pieces[p].item].dst;
                const uint16_t *const sym = scratch + pieces[p].sym_off;
                const uint32_t off = pieces[p].out_off, len = pieces[p].out_len;
                for (uint32_t t = (len > gzcut::WINDOW ? len - gzcut::WINDOW : 0u) + threadIdx.x; t < len; t += 256)
                    dst[(uint64_t)off + t] = (uint8_t)cut_byte(dst, off, sym[t], &marks);
                if (marks) atomicAdd(&resolved[p], (unsigned long long)marks);
            }
            __threadfence();
            __syncthreads();
        }
    }
}

// every symbol of every marker piece in front of its last 32 KiB becomes a byte, a lane per symbol; blockIdx.y takes a slice of the piece
__global__ __launch_bounds__(256) void k_gunzip_cut_apply(const GzItem *items, const gzcut::CutPiece *pieces, uint32_t n_pieces, const uint16_t *scratch,
                                                          unsigned long long *resolved) {
    for (uint32_t p = blockIdx.x; p < n_pieces; p += gridDim.x) {
        if (!pieces[p].marker || pieces[p].out_len <= gzcut::WINDOW) continue;
        uint32_t marks = 0;
        uint8_t *const dst = items[pieces[p].item].dst;
        const uint16_t *const sym = scratch + pieces[p].sym_off;
        const uint32_t off = pieces[p].out_off, head = pieces[p].out_len - gzcut::WINDOW;
        for (uint32_t t = blockIdx.y * 256 + threadIdx.x; t < head; t += gridDim.y * 256)
            dst[(uint64_t)off + t] = (uint8_t)cut_byte(dst, off, sym[t], &marks);
        if (marks) atomicAdd(&resolved[p], (unsigned long long)marks);
    }
}

__global__ __launch_bounds__(64) void k_gunzip_probe(const GzItem *items, const GzCand *cands, uint32_t n_cands, const uint32_t *stops, GzProbe *recs) {
    __shared__ InflLds S;
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < n_cands; c += gridDim.x) {
        __syncthreads();
        const uint32_t item = uni(cands[c].item), pos = uni(cands[c].pos), kind = uni(cands[c].kind);
        const uint32_t stop0 = uni(cands[c].stop0), stop1 = uni(cands[c].stop1);
        const uint8_t *const src = (const uint8_t *)(const glb8 *)uni64((uint64_t)items[item].src);
        const uint64_t n = uni(items[item].src_len), room = uni(items[item].room);
        GzProbe r;
        r.data_start = pos; r.end_kind = END_ERROR; r.end_pos = 0; r.status = 0; r.out = 0; r.reach = 0; r.crc = 0; r.isize = 0; r.next = 0;
        uint64_t data = pos;
        if (kind == K_MEMBER) r.status = member_header(src, n, pos, lane, &data);
        if (r.status == 0) {
            r.data_start = (uint32_t)data;
            BitIn b;
            b.src = src; b.win = S.in; b.n = n; b.ip = data; b.bb = 0; b.bc = 0; b.wbase = data;
            uint32_t how = 0;
            const uint32_t *const st = (const uint32_t *)(const __attribute__((address_space(1))) uint32_t *)(uint64_t)(stops + stop0);
            const int rc = kind == K_MEMBER ? probe_body<false>(S, b, room, st, stop1 - stop0, lane, &r.out, &r.reach, &how)
                                            : probe_body<true>(S, b, room, st, stop1 - stop0, lane, &r.out, &r.reach, &how);
            if (rc != 0) {
                r.status = E_CORRUPT;  // (input that ends early is damage: the item is the whole file)
            } else if (how == PROBE_LIMIT) {
                r.end_kind = END_ROOM;
            } else if (how == PROBE_BOUNDARY) {
                r.end_kind = END_BOUNDARY;
                r.end_pos = (uint32_t)b.ip;
            } else {
                Trailer t;
                if (read_trailer(src, n, b.ip - (b.bc >> 3), lane, &t) != 0) {
                    r.status = E_CORRUPT;
                } else {
                    r.end_kind = END_TRAILER;
                    r.end_pos = (uint32_t)t.after; r.crc = t.crc; r.isize = t.isize; r.next = t.next;
                }
            }
        }
        if (lane == 0) recs[c] = r;
    }
}

__global__ __launch_bounds__(64) void k_gunzip_inflate(const GzItem *items, const GzRun *runs, uint32_t n_runs, int32_t *status) {
    __shared__ InflLds S;
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = blockIdx.x; k < n_runs; k += gridDim.x) {
        __syncthreads();
        const uint32_t item = uni(runs[k].item), out_len = uni(runs[k].out_len);
        const uint8_t *const src = (const uint8_t *)(const glb8 *)uni64((uint64_t)items[item].src);
        uint8_t *const dst = (uint8_t *)(glb8 *)uni64((uint64_t)(items[item].dst + runs[k].out_off));
        BitIn b;
        b.src = src; b.win = S.in; b.n = uni(items[item].src_len); b.ip = uni(runs[k].src_start); b.bb = 0; b.bc = 0; b.wbase = b.ip;
        StopAt hook{out_len};
        uint32_t pos = 0;
        const int st = inflate_body(S, b, dst, out_len, lane, hook, &pos);
        // (the probe counted these very symbols: anything but the exact count says that the records were not this stream's)
        if (lane == 0) status[k] = st == 0 && pos == out_len ? 0 : E_CORRUPT;
    }
}

__global__ __launch_bounds__(64) void k_gunzip_single(const GzItem *items, const uint32_t *list, uint32_t n_list, GzSingle *res) {
    __shared__ InflLds S;
    __shared__ uint32_t T[256], red[64];
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = 0; k < 4; k++) {
        uint32_t c = lane * 4 + k;
        for (int j = 0; j < 8; j++) c = c & 1 ? (c >> 1) ^ CRC_POLY : c >> 1;
        T[lane * 4 + k] = c;
    }
    for (uint32_t e = blockIdx.x; e < n_list; e += gridDim.x) {
        __syncthreads();
        const uint32_t item = uni(list[e]);
        const uint8_t *const src = (const uint8_t *)(const glb8 *)uni64((uint64_t)items[item].src);
        uint8_t *const dst = (uint8_t *)(glb8 *)uni64((uint64_t)items[item].dst);
        const uint64_t n = uni(items[item].src_len);
        const uint32_t room = uni(items[item].room);
        uint64_t at = 0;
        uint32_t total = 0, members = 0, more = 1, sum_bad = 0, crc0 = 0, len0 = 0;
        int status = 0;
        while (more && status == 0) {  // (a member is at least 18 bytes of input)
            uint64_t data;
            status = member_header(src, n, at, lane, &data);
            if (status == 0) {
                BitIn b;
                b.src = src; b.win = S.in; b.n = n; b.ip = data; b.bb = 0; b.bc = 0; b.wbase = data;
                NoHook none;
                uint32_t got = 0;
                status = inflate_body(S, b, dst + total, room - total, lane, none, &got);
                Trailer t;
                if (status == 0) status = read_trailer(src, n, b.ip - (b.bc >> 3), lane, &t);
                if (status == 0) {
                    if (members == 0) {  // (the one member of nearly every item: its CRC is a workgroup's work in the CRC launch)
                        crc0 = t.crc; len0 = got;
                    } else {
                        wave_mem_sync();
                        if (wave_crc(T, red, dst + total, got, lane) != t.crc) sum_bad = 1;
                    }
                    if (t.isize != got) sum_bad = 1;
                    total += got;
                    members++;
                    if (t.next == NEXT_END) more = 0;
                    else if (t.next != NEXT_MEMBER) status = t.next;
                    at = t.after;
                }
            }
        }
        if (status == 0 && sum_bad) status = E_CRC;
        if (lane == 0) {
            GzSingle r;
            r.status = status; r.out_len = status == 0 ? total : 0; r.members = members; r.crc0 = crc0; r.len0 = len0; r.pad = 0;
            res[e] = r;
        }
    }
}

void launch_gunzip_scan(const GzItem *items, const GzScanChunk *chunks, uint32_t n_chunks, uint32_t *count, uint64_t *cands, hipStream_t s) {
    if (n_chunks) hipLaunchKernelGGL(k_gunzip_scan, dim3(n_chunks < 65536u ? n_chunks : 65536u), dim3(64), 0, s, items, chunks, n_chunks, count, cands);
}
void launch_gunzip_find(const gzcut::FindItem *items, const gzcut::FindChunk *chunks, uint32_t n_chunks, uint32_t cut, unsigned long long *slots,
                        unsigned long long *passed, hipStream_t s) {
    if (n_chunks && cut) hipLaunchKernelGGL(k_gunzip_find, dim3(n_chunks < 65536u ? n_chunks : 65536u), dim3(64), 0, s, items, chunks, n_chunks, cut, slots, passed);
}
void launch_gunzip_cut_probe(const GzItem *items, const gzcut::CutCand *cands, uint32_t n_cands, const uint64_t *stops, gzcut::CutRec *recs, hipStream_t s) {
    if (n_cands) hipLaunchKernelGGL(k_gunzip_cut_probe, dim3(n_cands < 65536u ? n_cands : 65536u), dim3(64), 0, s, items, cands, n_cands, stops, recs);
}
void launch_gunzip_cut_decode(const GzItem *items, const gzcut::CutPiece *pieces, uint32_t n_pieces, uint16_t *scratch, int32_t *status, hipStream_t s) {
    if (n_pieces) hipLaunchKernelGGL(k_gunzip_cut_decode, dim3(n_pieces < 65536u ? n_pieces : 65536u), dim3(64), 0, s, items, pieces, n_pieces, scratch, status);
}
void launch_gunzip_cut_tails(const GzItem *items, const gzcut::CutPiece *pieces, const gzcut::CutGroup *groups, uint32_t n_groups, const uint16_t *scratch,
                             unsigned long long *resolved, hipStream_t s) {
    if (n_groups) hipLaunchKernelGGL(k_gunzip_cut_tails, dim3(n_groups < 65536u ? n_groups : 65536u), dim3(256), 0, s, items, pieces, groups, n_groups, scratch, resolved);
}
void launch_gunzip_cut_apply(const GzItem *items, const gzcut::CutPiece *pieces, uint32_t n_pieces, const uint16_t *scratch, unsigned long long *resolved,
                             hipStream_t s) {
    if (n_pieces) hipLaunchKernelGGL(k_gunzip_cut_apply, dim3(n_pieces < 8192u ? n_pieces : 8192u, 8), dim3(256), 0, s, items, pieces, n_pieces, scratch, resolved);
}
void launch_gunzip_probe(const GzItem *items, const GzCand *cands, uint32_t n_cands, const uint32_t *stops, GzProbe *recs, hipStream_t s) {
    if (n_cands) hipLaunchKernelGGL(k_gunzip_probe, dim3(n_cands < 65536u ? n_cands : 65536u), dim3(64), 0, s, items, cands, n_cands, stops, recs);
}
void launch_gunzip_inflate(const GzItem *items, const GzRun *runs, uint32_t n_runs, int32_t *status, hipStream_t s) {
    if (n_runs) hipLaunchKernelGGL(k_gunzip_inflate, dim3(n_runs < 65536u ? n_runs : 65536u), dim3(64), 0, s, items, runs, n_runs, status);
}
void launch_gunzip_single(const GzItem *items, const uint32_t *list, uint32_t n_list, GzSingle *res, hipStream_t s) {
    if (n_list) hipLaunchKernelGGL(k_gunzip_single, dim3(n_list < 65536u ? n_list : 65536u), dim3(64), 0, s, items, list, n_list, res);
}

}  // namespace zn
