// The host's plan of a range read (znippy_rows_read_ranges[_verified]) and of a block-tree build (znippy_rows_block_tree_build):
// everything those calls work out from caller data before and between their device passes (range_plan.cc).  Plain C++, no HIP
// call: device addresses are only added to, never dereferenced, so a stand-alone program checks all of it under the sanitizers
// (tests/test_range_plan_cpu.py).  api.hip queues the device work the plan describes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

namespace zn {

// ---- what the kernels read (range_gather.hip, block_tree.hip) ----
// one piece of a requested range — at most RANGE_PIECE bytes, moved by one workgroup from wherever the bytes are (blob region,
// range scratch) to their place in the caller's output
struct RangePiece {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t len;
    uint32_t pad;
};
constexpr uint32_t RANGE_PIECE = 32u << 10;
struct BlockCvItem {       // one block to hash, by one wave
    const uint8_t *src;    // its first byte, any alignment (an item of fewer than 16 bytes has readable bytes in front of it)
    uint64_t slot;         // entry index: out[slot] is written, expect[slot] compared
    uint32_t bytes;        // 1 .. 128 KiB
    uint32_t first_chunk;  // chunk counter of its first KiB inside the row (128 * block number)
};
struct BlockTreeRow {  // one row with entries
    uint64_t first;    // its first entry
    uint32_t n;        // 2 .. 32,768 entries
    uint32_t row;      // index of its checksum
};

// ---- constants and small rules ----
constexpr uint64_t RR_BLK = 128 * 1024;
constexpr uint64_t RR_GUARD = 8192;  // in front of a slot: the block decoder reads up to WIN_HIST bytes of history back from in front of a block
constexpr uint64_t RR_SCRATCH_MAX = 32ull << 30;  // what one pool of the range scratch may grow to
#ifndef ZN_RR_ITEMS_MAX  // (a test of the limit compiles the module with a small one)
#define ZN_RR_ITEMS_MAX 0x7FFFFFF0ull
#endif
constexpr uint64_t RR_ITEMS_MAX = ZN_RR_ITEMS_MAX;  // items of one launch
// the status codes the plan gives out: the ZNIPPY_E_* of include/znippy_hip.h (api.hip asserts that they are)
constexpr int32_t RP_OK = 0, RP_E_INVAL = -1, RP_E_NOMEM = -3, RP_E_DST_SMALL = -4, RP_E_CORRUPT = -5, RP_E_DIGEST = -8;
// Entries of a row: one per 128 KiB block of a row of more than one block and below 4 GiB; none otherwise (znippy_hip.h).
inline uint64_t tree_entries_of(uint64_t len) { return len > RR_BLK && len < (1ull << 32) ? (len + RR_BLK - 1) / RR_BLK : 0; }
// A row is read block by block only if it has more than one block and its length fits the block decoder's 32-bit arithmetic with
// room to spare: a row of exactly 2^32 - 1 bytes has entries but is read whole.
inline bool rr_by_blocks(uint64_t len) { return len > RR_BLK && len < 0xFFFFFFFFull; }

struct RrRow {                       // a distinct row the ranges of a call touch
    uint32_t row = 0;                // index in the table
    bool comp = false, partial = false, late = false;
    int32_t status = 0;              // 0, or the ZNIPPY_E_* of its whole decode
    int pool = 0;                    // which scratch region its bytes are in
    uint64_t slot = 0, first = 0;    // byte b of the row is at pool + slot + (b - first)
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0;
    std::vector<uint8_t> need;       // partial: per block, a range overlaps it
    bool sblocks = false;            // verified read, stored row with accepted entries: `need` blocks are hashed where they lie
    bool hashed = false;             // verified read: the row was hashed whole
    std::vector<uint8_t> bad;        // verified read: per block, its chaining value does not equal its entry
};

struct RrTable {  // a view of the table's host columns (effective lengths: a stored row's length is its blob)
    uint32_t n;
    uint64_t row_begin, blob_cap;  // blob_cap = ~0: size of the blob region not declared
    const uint64_t *h_blob_off, *h_blob_size, *h_len;
    const uint8_t *h_comp;
    const uint64_t *tree_first;  // n + 1 entries once the tree is laid out (n_tree_first says whether)
    size_t n_tree_first;
    const uint8_t *tree_accept;  // per row: its installed entries fold to its checksum; may be shorter than the table
    size_t n_tree_accept;
};

struct RrCall {  // a view of the caller's arguments
    const uint64_t *row, *begin, *len, *out;  // out = NULL: destinations packed back to back
    uint64_t n_ranges, out_cap, blob_base;
    bool verified;
};

struct RangePlan {
    std::vector<int32_t> st;       // per range: 0 or its ZNIPPY_E_*
    std::vector<uint64_t> dst;     // per range: its offset in the output region
    std::vector<uint32_t> of_row;  // range -> entry of `rows` (0xFFFFFFFF: nothing to move)
    std::vector<RrRow> rows;
    std::vector<uint32_t> part, whole, stored_whole;  // entries of `rows`: read block by block / decoded whole / stored and hashed whole
    uint64_t n_items = 0, n_todo = 0;                 // blocks of the `part` rows, and how many of them a range overlaps
    uint64_t need0 = 0;                               // bytes of scratch pool 0
};

// The private columns and lists of the block pass, one allocation: what api.hip uploads (the first up_bytes) and what the
// kernels write first (the rest).
struct RangeSlab {
    uint64_t *blob_off, *blob_size, *usize, *out_off, *block_bytes;
    uint32_t *cand_row, *cand_base, *cand_nb, *item_row, *item_k, *todo, *ctl;
    int32_t *status;
    uint8_t *comp;
    unsigned long long *decoded;
    uint32_t *row_flag, *item_src;
    uint8_t *late;
};

// 1: the blob of row `ri` lies inside the blob region that starts at blob_base (and ends blob_cap later, where declared)
bool rr_blob_in_region(const RrTable &t, uint32_t ri, uint64_t blob_base);
// The next slot of a scratch pool: `front` guard bytes behind the next multiple of 256, `bytes` of content, 256 spare.  0: the pool
// would pass RR_SCRATCH_MAX.
bool rr_slot_take(uint64_t &need, uint64_t front, uint64_t bytes, uint64_t &slot);

// Every range against the table, the output region and the blob region; the distinct rows the good ones touch, their need bitmaps,
// routes and slots in pool 0.  RP_OK or RP_E_NOMEM (pool 0 would pass its limit).
int range_plan_build(const RrTable &t, const RrCall &c, RangePlan &p);
// Bytes of the slab for p.part (and, in *up_bytes, how many of them are uploaded), its columns at `base`, and their content.
size_t range_slab_layout(const RangePlan &p, size_t *up_bytes);
void range_slab_bind(uint8_t *base, const RangePlan &p, RangeSlab &slab);
void range_slab_fill(const RrTable &t, const RangePlan &p, uint8_t *host_base);  // writes [host_base, host_base + layout) only
// late_flags[c] != 0: row p.part[c] goes to the whole-row pass, with a slot in pool 1.  RP_OK or RP_E_NOMEM.
int range_plan_late(const RrTable &t, RangePlan &p, const uint8_t *late_flags, std::vector<uint32_t> &late_rows, uint64_t &need1);
// Verified reads: every block that will serve a range, as an item of the compare launch; item_of = (entry of rows, block).
// Returns the bytes the call hashes: those items and the rows hashed whole.
uint64_t range_plan_block_items(const RrTable &t, RangePlan &p, const uint8_t *pool0, const uint8_t *d_blobs, uint64_t blob_base,
                                std::vector<BlockCvItem> &items, std::vector<std::pair<uint32_t, uint32_t>> &item_of);
// dec_blocks plus the length of every row decoded whole
uint64_t range_plan_decoded(const RrTable &t, const RangePlan &p, uint64_t dec_blocks);
// `len` bytes from src to dst, cut into pieces of at most RANGE_PIECE bytes whose destinations, from the second piece on, start on a
// 128-byte line; appended to `pieces` (also the gather of znippy_targz_find_batch: deflate_batch.cc)
void range_cut_pieces(const uint8_t *src, uint8_t *dst, uint64_t len, std::vector<RangePiece> &pieces);
// Failed rows and bad blocks into p.st; every good range cut into pieces (range_cut_pieces).
void range_plan_pieces(const RrTable &t, const RrCall &c, RangePlan &p, const uint8_t *const pools[2], const uint8_t *d_blobs, uint8_t *d_out,
                       std::vector<RangePiece> &pieces);

// Block-tree build: the rows with entries against the blob region (st[row] = RP_E_CORRUPT), a slot in pool 0 for every compressed
// one (sel = entries of `rows`).  RP_OK or RP_E_NOMEM.
int tree_plan_rows(const RrTable &t, uint64_t blob_base, std::vector<int32_t> &st, std::vector<RrRow> &rows, std::vector<uint32_t> &sel, uint64_t &need0);
// Every block of every row that decoded, as an item of the write launch; the others' statuses into st.  good = table rows.
void tree_plan_items(const RrTable &t, const std::vector<RrRow> &rows, const uint8_t *pool0, const uint8_t *d_blobs, uint64_t blob_base,
                     std::vector<int32_t> &st, std::vector<uint32_t> &good, std::vector<BlockCvItem> &items);

}  // namespace zn
