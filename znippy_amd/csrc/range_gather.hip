// Range reads (znippy_rows_read_ranges): the slice gather.  Every requested range is a run of bytes somewhere on the
// device — inside the blob region for a stored row, inside the context's range scratch for a decoded block or row — that
// has to land at its own place in the caller's output.  Byte-granular on both sides: a source and a destination share
// no alignment in general.
//
// The host (range_plan_pieces in host/range_plan.cc) cuts every range into pieces of at most RANGE_PIECE bytes whose
// destinations, from the second piece of a range on, start on a 128-byte line; one workgroup moves one piece:
//   head   the bytes in front of the destination's first whole 128-byte line, a byte per lane
//   body   whole lines, 16 bytes per lane with aligned 16-byte stores (eight neighbouring lanes write one line).  The
//          source of a body is read with aligned 16-byte loads as well: where it shares the destination's alignment one
//          load per lane, where it does not two neighbouring granules that are funnelled together (v_alignbyte).  Both
//          granules hold at least one byte of the piece, so no load leaves the aligned 16 bytes around a source byte.
//   tail   what is left behind the last whole line, a byte per lane
// Exactly the bytes [dst, dst + len) are written.  No wave primitive is used: every branch below depends on the piece
// alone (uniform over the workgroup) or is a bounds check in front of a plain load / store.
#include "common.h"

namespace zn {

// 16 source bytes from p, which is `sh` (1..15) bytes behind a 16-byte boundary: two aligned granules, shifted together
__device__ __forceinline__ uint4 load16_funnel(const uint8_t *p, uint32_t sh) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p - sh);
    const uint4 a = q[0], b = q[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint32_t by = sh & 3;
    uint4 r;
    switch (sh >> 2) {  // uniform over the workgroup
    case 0: r = make_uint4(__builtin_amdgcn_alignbyte(w[1], w[0], by), __builtin_amdgcn_alignbyte(w[2], w[1], by), __builtin_amdgcn_alignbyte(w[3], w[2], by), __builtin_amdgcn_alignbyte(w[4], w[3], by)); break;
    case 1: r = make_uint4(__builtin_amdgcn_alignbyte(w[2], w[1], by), __builtin_amdgcn_alignbyte(w[3], w[2], by), __builtin_amdgcn_alignbyte(w[4], w[3], by), __builtin_amdgcn_alignbyte(w[5], w[4], by)); break;
    case 2: r = make_uint4(__builtin_amdgcn_alignbyte(w[3], w[2], by), __builtin_amdgcn_alignbyte(w[4], w[3], by), __builtin_amdgcn_alignbyte(w[5], w[4], by), __builtin_amdgcn_alignbyte(w[6], w[5], by)); break;
    default: r = make_uint4(__builtin_amdgcn_alignbyte(w[4], w[3], by), __builtin_amdgcn_alignbyte(w[5], w[4], by), __builtin_amdgcn_alignbyte(w[6], w[5], by), __builtin_amdgcn_alignbyte(w[7], w[6], by)); break;
    }
    return r;
}

__global__ __launch_bounds__(256) void k_range_gather(const RangePiece *pieces, uint32_t n_pieces) {
    const uint32_t p = blockIdx.x, tid = threadIdx.x;
    if (p >= n_pieces) return;
    const uint8_t *const src = pieces[p].src;
    uint8_t *const dst = pieces[p].dst;
    const uint32_t len = pieces[p].len;
    const uint32_t to_line = (uint32_t)((128 - ((uintptr_t)dst & 127)) & 127);
    const uint32_t head = to_line < len ? to_line : len;
    for (uint32_t i = tid; i < head; i += 256) dst[i] = src[i];
    const uint32_t chunks = ((len - head) >> 7) << 3;  // 16-byte chunks of the whole lines
    const uint8_t *const s0 = src + head;
    uint8_t *const d0 = dst + head;
    const uint32_t sh = (uint32_t)((uintptr_t)s0 & 15);
    if (sh == 0) {
        for (uint32_t c = tid; c < chunks; c += 256) reinterpret_cast<uint4 *>(d0)[c] = reinterpret_cast<const uint4 *>(s0)[c];
    } else {
        for (uint32_t c = tid; c < chunks; c += 256) reinterpret_cast<uint4 *>(d0)[c] = load16_funnel(s0 + 16 * (size_t)c, sh);
    }
    for (uint32_t i = head + 16 * chunks + tid; i < len; i += 256) dst[i] = src[i];
}

// Verdict per private row of the partial route, and the call's measure of work: a row whose frame passed the block scan
// and whose needed blocks all decoded (row_flag == 0) is served from its blocks and adds their content bytes; any other
// row is left to the whole-row pass (late[] = 1).
__global__ __launch_bounds__(256) void k_range_status(const uint32_t *row_flag, const uint64_t *block_bytes, uint32_t n_rows, uint8_t *late, unsigned long long *decoded) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    const bool ok = row_flag[i] == 0;
    late[i] = ok ? 0 : 1;
    if (ok && block_bytes[i]) atomicAdd(decoded, (unsigned long long)block_bytes[i]);
}

void launch_range_gather(const RangePiece *pieces, uint32_t n_pieces, hipStream_t s) {
    if (n_pieces) hipLaunchKernelGGL(k_range_gather, dim3(n_pieces), dim3(256), 0, s, pieces, n_pieces);
}
void launch_range_status(const uint32_t *row_flag, const uint64_t *block_bytes, uint32_t n_rows, uint8_t *late, unsigned long long *decoded, hipStream_t s) {
    if (n_rows) hipLaunchKernelGGL(k_range_status, dim3((n_rows + 255) / 256), dim3(256), 0, s, row_flag, block_bytes, n_rows, late, decoded);
}

}  // namespace zn
