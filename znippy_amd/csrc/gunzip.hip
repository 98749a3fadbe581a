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
// Not done here: decoding dependent pieces in parallel from their predecessors' last 32 KiB, guessing block boundaries inside streams
// without flush points, xz.  (bzip2 files: bunzip2.hip; listing the members of the tar inside: tar_list.hip.)
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
