// Block tree of a row (znippy_rows_block_tree_build / _set_block_tree / znippy_rows_read_ranges_verified): BLAKE3 is a tree
// hash and 128 KiB = 128 chunks, a power of two, so every aligned 128 KiB block of a row is a complete subtree of the row's
// hash tree.  Entry k of a row is the NON-root chaining value of the subtree over chunks [128k, min(128k + 128, chunks of the
// row)), hashed with the row's own chunk counters; folded pairwise with the odd node promoted (fold_segments) and ROOT on the
// last parent, a row's entries give its digest.  Two kernels:
//   k_block_cvs        one wave per block: the block's chaining value, written or compared with the entry it should equal
//   k_block_tree_fold  one wave per row: the row's entries folded to its digest and compared with the index checksum —
//                      which is what authenticates the entries, wherever they came from
// The write side has a third (znippy_rounds_emit_block_tree):
//   k_round_block_entries  lane = entry: the entry made from the one or two 64-leaf tile chaining values the round's hash left
//                          in tile_cv — no input byte is read a second time
// Integer/byte work bounded by the VALU and HBM as in hash_kernels.hip; no MFMA, no inline assembly.
#include "common.h"
#include "hash_dev.h"

namespace zn {

// One wave per item, items taken by static stride (wave-uniform control flow, no cursor).  The wave hashes up to two halves of
// 64 leaves, lane = leaf; the bytes come through the wave's LDS stage (hash_ragged_through_stage: four lanes load one leaf's 64
// contiguous bytes, 16 leaves per load instruction, instead of every lane's own 64 bytes 1 KiB from its neighbour's), each half
// is folded inside the wave and one parent joins the two.
// Reads: exactly the item's bytes [src, src + bytes) — with one exception the caller vouches for: the last 1..15 bytes of a
// ragged leaf are read as the 16 bytes that END with them, so an item shorter than 16 bytes needs readable bytes in front of
// it.  Every item of a row is a block behind a whole block of the same row, or sits behind the guard of a scratch slot.
__global__ __launch_bounds__(256) void k_block_cvs(const BlockCvItem *items, uint32_t n_items, uint32_t *out, const uint32_t *expect,
                                                   uint32_t *verdict) {
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[4][STAGE_BYTES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint8_t *const stage = s_stage[w];
    const uint32_t stride = gridDim.x * 4;
    for (uint32_t it = blockIdx.x * 4 + w; it < n_items; it += stride) {  // (wave-uniform)
        const BlockCvItem item = items[it];
        const uint32_t n = item.bytes < BLOCK_TREE_BLK ? item.bytes : BLOCK_TREE_BLK;
        const uint32_t chunks = (n + 1023) >> 10;
        uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t h = 0; h * 64 < chunks; h++) {  // (wave-uniform: one or two halves)
            const uint32_t leaf = 64 * h + lane;
            const bool active = leaf < chunks;
            uint32_t leaf_len = 0;
            if (active) leaf_len = n - (leaf << 10) < 1024 ? n - (leaf << 10) : 1024;
            const uint32_t nblk = leaf_len ? (leaf_len + 63) >> 6 : 1u;
            const Cv8 r = hash_ragged_through_stage(item.src + (active ? (size_t)leaf << 10 : 0), nullptr, leaf_len, nblk,
                                                    item.first_chunk + leaf, false, active, stage);
            uint32_t cv[8];
#pragma unroll
            for (int i = 0; i < 8; i++) cv[i] = r.v[i];
            const uint32_t cnt = chunks - 64 * h < 64 ? chunks - 64 * h : 64;
            fold_segments(cv, 0, active ? cnt : 0, false);
            if (h == 0) {
#pragma unroll
                for (int i = 0; i < 8; i++) acc[i] = cv[i];
            } else {
                uint32_t L[8];
#pragma unroll
                for (int i = 0; i < 8; i++) L[i] = acc[i];
                b3::parent(acc, L, cv, false);  // (lane 0 holds both halves' nodes)
            }
        }
        if (lane == 0) {
            if (out) {
#pragma unroll
                for (int i = 0; i < 8; i++) out[(size_t)item.slot * 8 + i] = acc[i];
            }
            if (expect) {
                uint32_t diff = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) diff |= acc[i] ^ expect[(size_t)item.slot * 8 + i];
                verdict[it] = diff == 0 ? 1u : 0u;
            }
        }
    }
}

// One wave per row with entries: the row's n entries (2 .. 32,768: such rows are below 4 GiB) folded to its digest.  Six levels
// of pairing turn every aligned group of 64 nodes — the last, shorter one included, the odd node carried — into one node
// whatever its neighbours are (as k_merge_groups over tile CVs), so the fold goes level by level in groups of 64: the entries
// (global memory, read only) to at most 512 nodes in LDS, those to at most 8, those to the root.  verdict = the digest equals
// the row's checksum.
__global__ __launch_bounds__(64) void k_block_tree_fold(const BlockTreeRow *rows, uint32_t n_rows, const uint32_t *tree, const uint8_t *checksum,
                                                       uint32_t *verdict) {
    __shared__ __attribute__((aligned(16))) uint32_t s_a[512 * 8];
    __shared__ __attribute__((aligned(16))) uint32_t s_b[8 * 8];
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x >= n_rows) return;
    const BlockTreeRow u = rows[blockIdx.x];
    if (u.n < 2 || u.n > 32768) {  // (no such row has entries: nothing vouches for it)
        if (lane == 0) verdict[blockIdx.x] = 0;
        return;
    }
    const uint32_t *src = tree + (size_t)u.first * 8;
    uint32_t m = u.n;
    uint32_t cv[8];
    for (int level = 0; level < 2 && m > 64; level++) {  // (uniform over the wave)
        uint32_t *const dst = level == 0 ? s_a : s_b;
        const uint32_t groups = (m + 63) / 64;
        for (uint32_t g = 0; g < groups; g++) {
            const uint32_t cnt = m - 64 * g < 64 ? m - 64 * g : 64;
#pragma unroll
            for (int i = 0; i < 8; i++) cv[i] = lane < cnt ? src[((size_t)64 * g + lane) * 8 + i] : 0u;
            fold_segments(cv, 0, lane < cnt ? cnt : 0, false);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 8; i++) dst[g * 8 + i] = cv[i];
            }
        }
        __syncthreads();  // the level is complete before the next one reads it
        src = dst;
        m = groups;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) cv[i] = lane < m ? src[(size_t)lane * 8 + i] : 0u;
    fold_segments(cv, 0, lane < m ? m : 0, true);
    if (lane == 0) {
        const uint32_t *want = reinterpret_cast<const uint32_t *>(checksum + (size_t)u.row * 32);  // (the column is a device allocation: aligned)
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) diff |= cv[i] ^ want[i];
        verdict[blockIdx.x] = diff == 0 ? 1u : 0u;
    }
}

// Write side: a 128 KiB block is two 64-leaf tiles, and the hash of a round above 64 KiB leaves every tile's non-root chaining value
// in tile_cv[cv_base + t] (all routes; the merge kernels only read these slots).  Entry k of a unit with entries is therefore
// parent(tile_cv[cv_base + 2k], tile_cv[cv_base + 2k + 1]) with ROOT clear, or tile_cv[cv_base + 2k] itself where the last block has at
// most 64 chunks.  Lane = entry of the whole table; the lane finds its unit by a binary search of fixed trip count (`top` = the
// largest power of two below n_units, 0 for one unit) over units[].first, which rises strictly — every listed unit has at least two
// entries — and ends with the sentinel units[n_units].first = n_entries.  Every lane runs the one compress (a lane past the end
// redoes the last entry, a lone tile's lane pairs the tile with itself) and only the store is predicated.
// Reads: units[0 .. n_units), tile CVs cv_base + [0, n_cvs) of listed units.  Writes: tree[0 .. 8 * n_entries).
__global__ __launch_bounds__(256) void k_round_block_entries(const TreeUnit *units, uint32_t n_units, uint32_t top, uint32_t n_entries,
                                                             const uint32_t *tile_cv, uint32_t *tree) {
    const uint32_t e0 = blockIdx.x * 256 + threadIdx.x;
    const bool on = e0 < n_entries;
    const uint32_t e = on ? e0 : n_entries - 1;
    uint32_t lo = 0;  // the last unit whose first entry is <= e
    for (uint32_t step = top; step; step >>= 1) {  // (uniform over the grid)
        const uint32_t cand = lo + step;
        const uint32_t first = units[cand < n_units ? cand : n_units - 1].first;
        lo = cand < n_units && first <= e ? cand : lo;
    }
    const uint4 uw = *reinterpret_cast<const uint4 *>(units + lo);  // first, cv_base, n_cvs, -
    const uint32_t k = e - uw.x;
    const bool lone = 2 * k + 1 >= uw.z;
    const size_t il = (size_t)uw.y + 2 * k, ir = lone ? il : il + 1;
    const uint4 *const pl = reinterpret_cast<const uint4 *>(tile_cv + il * 8), *const pr = reinterpret_cast<const uint4 *>(tile_cv + ir * 8);
    const uint4 l0 = pl[0], l1 = pl[1], r0 = pr[0], r1 = pr[1];
    const uint32_t L[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
    const uint32_t R[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    uint32_t out[8];
    b3::parent(out, L, R, false);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = lone ? L[i] : out[i];
    if (on) {
        uint4 *const po = reinterpret_cast<uint4 *>(tree + (size_t)e0 * 8);
        po[0] = make_uint4(out[0], out[1], out[2], out[3]);
        po[1] = make_uint4(out[4], out[5], out[6], out[7]);
    }
}

void launch_round_block_entries(const TreeUnit *units, uint32_t n_units, uint32_t n_entries, const uint32_t *tile_cv, uint32_t *tree, hipStream_t s) {
    if (!n_units || !n_entries) return;
    uint32_t top = 0;
    for (uint32_t p = 1; p < n_units; p <<= 1) top = p;
    hipLaunchKernelGGL(k_round_block_entries, dim3((n_entries + 255) / 256), dim3(256), 0, s, units, n_units, top, n_entries, tile_cv, tree);
}
void launch_block_cvs(const BlockCvItem *items, uint32_t n_items, uint32_t *out, const uint32_t *expect, uint32_t *verdict, hipStream_t s) {
    if (!n_items) return;
    const uint32_t grid = std::min<uint32_t>((n_items + 3) / 4, 4096);
    hipLaunchKernelGGL(k_block_cvs, dim3(grid), dim3(256), 0, s, items, n_items, out, expect, verdict);
}
void launch_block_tree_fold(const BlockTreeRow *rows, uint32_t n_rows, const uint32_t *tree, const uint8_t *checksum, uint32_t *verdict, hipStream_t s) {
    if (n_rows) hipLaunchKernelGGL(k_block_tree_fold, dim3(n_rows), dim3(64), 0, s, rows, n_rows, tree, checksum, verdict);
}

}  // namespace zn
