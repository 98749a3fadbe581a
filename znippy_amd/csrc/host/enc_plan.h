// Which kernels one write-side run (znippy_encode_hash_rounds_async) launches, on which streams and with what geometry.
// Plain C++, no HIP call: everything here is known before the run's first stream operation — the table's shape, the
// context's level, grids and switches, and whether the far window's buffers could be made (api.hip: rounds_launch).
// Behind the plan: the layout of the slab a run leaves its results in (ResSlab).
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int ENC_HIGH_TIER_LEVEL = 4;  // = HIGH_TIER_LEVEL of encode.h (api.hip asserts it)

struct EncShape {  // the table (znippy_rounds), as this run finds it
    uint32_t n;                  // rounds
    uint32_t n_items;            // output pieces: one per block of an encoded round, one per 64 KiB slice of a stored one
    uint32_t n_small, n_wide;    // encoder items of each variant (blocks <= 16 KiB / the rest)
    uint64_t in_bytes, enc_bytes;  // all rounds / rounds that go through the encoder
    int fuse_tiles;              // > 0: every round is a small encoded round (one block, no store path), this many hash tiles per dequeue
    uint32_t plan_n_tiles;       // tiles of the hash plan
    uint32_t n_tree_entries;     // block tree entries of the table (0 until emission was first switched on)
    uint64_t ldm_entries;        // far window: index entries of the rounds longer than one block (0: no such round)
    bool store_incompressible;   // opt-in (znippy_rounds_set_store_incompressible)
    bool emit_tree;              // opt-in (znippy_rounds_emit_block_tree)
    uint32_t blob_align;         // opt-in (znippy_rounds_set_blob_align), 1 = packed
};

struct EncEnv {  // the context
    int level, window_log;
    int encode_grid, encode_grid_small;  // resident workgroups of the wide / the small encoder variant
    bool nohash, no_fuse_hash, no_fused_store;  // ZNIPPY_NOHASH (diagnostic), ZNIPPY_NO_FUSE_HASH, ZNIPPY_NO_FUSED_STORE
    bool ldm_ok;  // ensure_ldm succeeded (asked only when enc_window_log says the run is windowed)
};

struct EncLaunch {  // one launch of the encoder kernel
    bool on;
    uint32_t n_items;  // entries of its list (retry launch: the bound; the count is on the device)
    bool use_order;    // through the share's index list (false: all items are of one kind, no indirection)
    int grid;
    uint32_t batch;    // items per cursor dequeue
};

struct EncPlan {
    bool high;          // the higher effort tier of the encoder
    int window_log;     // cross-block window of this run (0: every block stands alone)
    bool tail_mark;     // frames of several blocks end with an empty raw block
    bool far;           // the far window: ldm_index in front of the encoder
    bool fuse_hash;     // route: the small encoder's waves hash the rounds they encode (zstd_encode_hash)
    bool fuse_store;    // route: the hash runs behind the gather and copies the stored rounds it hashes
    bool fork_aux;      // neither of the two: the auxiliary stream is forked behind the clears and joined behind the gather
    bool hash_beside;   // route: ... and the hash runs there, beside the encoder (with ZNIPPY_NOHASH the fork is around nothing)
    bool emit_tree;     // the run was queued with block tree emission on
    bool tree_out;      // ... and the table has entries: block_tree_entries behind the merge, the tree leaves with the results
    bool store_decide;  // the opt-in pass that turns rounds whose frame is no smaller than the input into raw payloads
    bool pad;           // aligned blob offsets: round_pad in front of the scan
    bool small_pieces;  // gather with a lane per piece instead of a wave per piece
    EncLaunch wide, small, retry;  // in launch order; retry: what the small variant handed to the wide one
};

int enc_window_log(const EncEnv &e);  // this run's window: asked before the plan, for the far window's allocations
EncPlan enc_plan(const EncShape &s, const EncEnv &e);

// The results of one run, in one slab: [total u64][overflow u32, 4 bytes unused][blob_offset u64 x n][blob_size u64 x n]
// [digests 32 bytes x n].  The same over a device slab and over its pinned host mirror (both 16-byte aligned); the run clears
// everything in front of the digests.
struct ResSlab {
    uint8_t *base;
    uint32_t n;
    uint64_t *total() const { return reinterpret_cast<uint64_t *>(base); }
    uint32_t *overflow() const { return reinterpret_cast<uint32_t *>(base + 8); }
    uint64_t *blob_offset() const { return reinterpret_cast<uint64_t *>(base + 16); }
    uint64_t *blob_size() const { return blob_offset() + n; }
    uint32_t *digests() const { return reinterpret_cast<uint32_t *>(base + 16 + 16 * (size_t)n); }
    static size_t clear_bytes(size_t n) { return 16 + 16 * n; }
    static size_t bytes(size_t n) { return 16 + n * (8 + 8 + 32); }
};
