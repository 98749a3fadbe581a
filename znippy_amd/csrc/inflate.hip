// Raw DEFLATE (RFC 1951) of a batch of independent streams (znippy_inflate_batch): the selected entries of ZIP containers whose
// bytes are in device memory already.  wave = stream: one 64-lane workgroup walks one stream from its first bit to the final
// block's end-of-block.
//
//   tables    per stream in LDS (6.4 KiB per wave with the input window, so LDS never limits residency): a primary table per code
//             (literal/length 2^10, distance 2^9, code lengths 2^7 cells of 2 bytes: symbol << 4 | length) and, for the codes longer
//             than the primary index and for every cell no code reaches, the canonical walk over the counts per length and the
//             symbols sorted by code.  Built by the whole wave, as the FSE and Huffman builders of zstd_dev.h are: lanes count the
//             codes per length (ballots), the counts are prefixed, then lane = symbol fills its replicated cells.  The fixed
//             tables go through the same builder from constant lengths and are kept while consecutive blocks use them.
//   input     a 2 KiB window of the stream in LDS, loaded 16 bytes per lane and zero-filled behind src_len; the bit buffer is
//             refilled from it.  Bits consumed are counted against src_len after every symbol: a stream never ends early unseen.
//   output    literals are gathered one per lane and stored 64 at a time; a match and a stored block are copied by the whole wave
//             (coop_match / coop_copy).  A match reads bytes this wave stored before: wave_mem_sync stands between.
//   control   untrusted input: every value that steers a loop is wave-uniform and goes through readfirstlane, work items are taken
//             with a static stride, a failed check sets the status and the loops end through their conditions (no break in front
//             of a lane-masked statement; DESIGN.md §7c, the second form).  Every iteration of every loop consumes at least one
//             input bit or produces an output byte, and is bounded by src_len and out_len.
// Validity is zlib's (inflate.c / inftrees.c): the tests use it as arbiter.  All checks of a symbol come before its first byte.
// The stream decoder itself (tables, bit reader, body) is in inflate_dev.h, which targz.hip shares; k_inflate runs it with an empty hook.
//
// The CRC-32 (ZIP polynomial, reflected) of what was produced is a launch of its own: a workgroup per entry cuts it into 256
// equal segments from the back, every lane runs the table-driven CRC over its segment, and the lane CRCs are folded pairwise with
// crc(A || B) = crc(A) * x^(8 |B|) mod P  xor  crc(B) — zlib's crc32_combine — where all right-hand operands of a level have the same
// length, so one power serves the level and is squared for the next.  One path for every size.
#include "inflate_dev.h"

namespace zn {

namespace {

__device__ int inflate_stream(InflLds &S, const uint8_t *src, uint32_t src_len, uint8_t *dst, uint32_t out_len, uint32_t lane) {
    BitIn b;
    b.src = src; b.win = S.in; b.n = src_len; b.ip = 0; b.bb = 0; b.bc = 0; b.wbase = 0;
    NoHook none;
    uint32_t pos = 0;
    int st = inflate_body(S, b, dst, out_len, lane, none, &pos);
    if (st == 0 && pos != out_len) st = E_CORRUPT;
    return st;
}
}  // namespace

__global__ __launch_bounds__(64) void k_inflate(const InflateItem *items, uint32_t n_items, int32_t *status) {
    __shared__ InflLds S;
    const uint32_t lane = threadIdx.x;
    for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        __syncthreads();
        // (device memory, which a pointer that went through readfirstlane no longer says: through the global address space, so that the
        // stream's loads and stores are global_* instructions and not flat_*, which would count against the LDS counter as well)
        const uint8_t *const src = (const uint8_t *)(const glb8 *)uni64((uint64_t)items[it].src);
        uint8_t *const dst = (uint8_t *)(glb8 *)uni64((uint64_t)items[it].dst);
        const uint32_t src_len = uni(items[it].src_len), out_len = uni(items[it].out_len), method = uni(items[it].method);
        int st = 0;
        if (method == 0) coop_copy(dst, src, out_len, lane, 64);  // (src_len == out_len: the host has checked)
        else st = inflate_stream(S, src, src_len, dst, out_len, lane);
        if (lane == 0) status[it] = st;
    }
}

__global__ __launch_bounds__(256) void k_inflate_crc(const InflateItem *items, uint32_t n_items, int32_t *status, uint32_t *crc_out) {
    __shared__ uint32_t T[256], red[256];
    const uint32_t tid = threadIdx.x;
    {
        uint32_t c = tid;
        for (int k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ CRC_POLY : c >> 1;
        T[tid] = c;
    }
    __syncthreads();
    for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        if (status[it] == 0) {  // (one value for the whole workgroup)
            const uint8_t *const p = (const uint8_t *)(const glb8 *)(uint64_t)items[it].dst;
            const uint64_t len = items[it].out_len;
            const uint64_t seg = (len + 255) >> 8;
            // 256 segments of `seg` bytes, aligned to the END of the entry: the leading ones are empty or, one of them, short
            int64_t a = (int64_t)len - (int64_t)(256 - tid) * (int64_t)seg, e = a + (int64_t)seg;
            if (a < 0) a = 0;
            if (e < 0) e = 0;
            uint32_t crc = 0xFFFFFFFFu;
            for (; a + 16 <= e; a += 16) {
                uint32_t w[4];
                __builtin_memcpy(w, p + a, 16);
                for (int j = 0; j < 4; j++)
                    for (int k = 0; k < 4; k++) {
                        crc = T[(crc ^ w[j]) & 255] ^ (crc >> 8);
                        w[j] >>= 8;
                    }
            }
            for (; a < e; a++) crc = T[(crc ^ p[a]) & 255] ^ (crc >> 8);
            red[tid] = ~crc;  // (an empty segment: 0, which the fold leaves out of the result)
            __syncthreads();
            uint32_t pw = crc_xpow(8 * seg);
            for (uint32_t stride = 1; stride < 256; stride <<= 1) {
                if ((tid & (2 * stride - 1)) == 0) red[tid] = crc_mulmod(pw, red[tid]) ^ red[tid + stride];
                __syncthreads();
                pw = crc_mulmod(pw, pw);
            }
            if (tid == 0) {
                const uint32_t c = red[0];
                crc_out[it] = c;
                if (items[it].has_crc && c != items[it].want_crc) status[it] = E_CRC;
            }
            __syncthreads();
        }
    }
}

void launch_inflate(const InflateItem *items, uint32_t n_items, int32_t *status, hipStream_t s) {
    if (n_items) hipLaunchKernelGGL(k_inflate, dim3(n_items < 65536u ? n_items : 65536u), dim3(64), 0, s, items, n_items, status);
}
void launch_inflate_crc(const InflateItem *items, uint32_t n_items, int32_t *status, uint32_t *crc_out, hipStream_t s) {
    if (n_items) hipLaunchKernelGGL(k_inflate_crc, dim3(n_items < 65536u ? n_items : 65536u), dim3(256), 0, s, items, n_items, status, crc_out);
}

}  // namespace zn
