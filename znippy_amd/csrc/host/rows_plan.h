// Everything the read side decides on the host: the tile plan the hash kernels' work cursor runs over, what the pass over a
// row table's columns learns (RowsShape, RowClasses), what a finished run teaches the table (RowsHints), which kernels one run
// launches, on which streams and with what grids (RunPlan), the sizes of the context's grow-only pools, and the host's verdicts
// for rows that point outside a run's regions.  Plain C++, no HIP call and no getenv: api.hip keeps allocation, uploads and
// stream operations, and a stand-alone program tests this under the sanitizers (tests/test_rows_plan_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace zn {

// A hash work item = one wavefront's worth of BLAKE3 leaves (<= 64 x 1 KiB).
//   n_units >= 1 : `n_units` whole small units (each <= 64 leaves) packed so their leaves fill
//                  the wave's lanes; digests are finished inside the wave.
//   n_units == 0 : leaves [first_leaf, first_leaf+n_leaves) of big unit `first_unit`
//                  (first_leaf is a multiple of 64 -> a complete subtree); the subtree CV goes
//                  to tile_cv[cv_index] and the big-unit merge kernel finishes the tree.
struct Tile {
    uint32_t first_unit;
    uint32_t n_units;
    uint32_t first_leaf;
    uint32_t n_leaves;
    uint32_t cv_index;
    uint32_t pad;
};

struct BigUnit {  // a unit with more than 64 leaves
    uint32_t unit;
    uint32_t cv_base;  // first tile CV of this unit in tile_cv
    uint32_t n_cvs;    // ceil(leaves/64) >= 2
    uint32_t pad;      // n_cvs > 64: index (in CVs) of this unit's group CVs in tile_cv, ceil(n_cvs/64) of them
};

constexpr uint32_t BLOCK_TREE_BLK = 128u << 10;  // the 128 KiB block of this library's frames (and of the block tree's entries)
constexpr uint32_t XXH_WAVE_MIN = (64u << 10) + 1;  // checksum stage: frames of at least this many bytes get a wave, smaller ones four lanes
constexpr uint32_t RX_MIN = 256u << 10;  // resolve path: frames of at least this many bytes (less for tables with few rows above 64 KiB)
constexpr uint32_t BX_PREDEF_LL = 0, BX_PREDEF_OF = 64, BX_PREDEF_ML = 96, BX_POOL_FIRST = 160;  // predefined tables at the head of the FSE pool

}  // namespace zn

// ---- tile plan ------------------------------------------------------------------------------------------------------------------
struct PlanBuf {
    std::vector<zn::Tile> tiles;
    std::vector<zn::BigUnit> big;
    uint32_t n_tile_cv = 0;
    // units with more than 64 tile CVs: their CVs are first folded in groups of 64 by independent waves
    // (group g of big unit b: grp_big[g] = b, first CV = big[b].cv_base + 64 * grp_k[g]); results live behind the
    // tile CVs, from BigUnit::pad on
    std::vector<uint32_t> grp_big, grp_k;
};

// Greedy tile plan over unit lengths: whole small units are packed until a wave's 64 lanes are
// full; a unit with more than 64 leaves becomes ceil(leaves/64) slice tiles + one BigUnit.
template <class LenOf>
static void build_plan(LenOf len_of, uint32_t n, PlanBuf &p) {
    using zn::BigUnit; using zn::Tile;
    p.tiles.reserve((size_t)n / 4 + 16);
    uint32_t cur_first = 0, cur_units = 0, cur_leaves = 0;
    auto flush = [&]() {
        if (cur_units) p.tiles.push_back(Tile{cur_first, cur_units, 0, cur_leaves, 0, 0});
        cur_units = 0;
        cur_leaves = 0;
    };
    for (uint32_t u = 0; u < n; u++) {
        const uint64_t len_u = len_of(u);
        uint64_t leaves64 = len_u ? (len_u + 1023) >> 10 : 1;
        if (leaves64 > 64) {
            flush();
            uint32_t n_cvs = (uint32_t)((leaves64 + 63) / 64);
            p.big.push_back(BigUnit{u, p.n_tile_cv, n_cvs, 0});
            if (n_cvs > 64)
                for (uint32_t g = 0; g < (n_cvs + 63) / 64; g++) { p.grp_big.push_back((uint32_t)p.big.size() - 1); p.grp_k.push_back(g); }
            for (uint32_t t = 0; t < n_cvs; t++) {
                uint32_t first = t * 64;
                uint32_t nl = (uint32_t)std::min<uint64_t>(64, leaves64 - first);
                p.tiles.push_back(Tile{u, 0, first, nl, p.n_tile_cv + t, 0});
            }
            p.n_tile_cv += n_cvs;
        } else {
            uint32_t leaves = (uint32_t)leaves64;
            if (cur_units == 64 || cur_leaves + leaves > 64) flush();
            if (!cur_units) cur_first = u;
            cur_units++;
            cur_leaves += leaves;
            // a run of units of this same size (archives of fixed-size chunks: every BASELINE config): whole tiles at once —
            // exactly the tiles the unit-by-unit rule above would cut (tests/test_rows_plan_cpu.py).  The run's last tile stays
            // open even when it is a whole one: a smaller unit behind the run may still fit into it.
            if (cur_units == 1 && u + 1 < n && len_of(u + 1) == len_u) {
                uint32_t v = u + 1;
                while (v < n && len_of(v) == len_u) v++;
                const uint32_t per = std::min<uint32_t>(64 / leaves, 64), run = v - u, full = run / per;
                if (full >= 1) {
                    const uint32_t rest = run - full * per, closed = rest ? full : full - 1;
                    for (uint32_t t = 0; t < closed; t++) p.tiles.push_back(Tile{u + t * per, per, 0, per * leaves, 0, 0});
                    cur_first = u + closed * per; cur_units = rest ? rest : per; cur_leaves = cur_units * leaves;
                    u = v - 1;
                }
            }
        }
    }
    flush();
    uint32_t gb = 0;  // where each grouped unit's group CVs start (behind all tile CVs)
    for (BigUnit &b : p.big)
        if (b.n_cvs > 64) { b.pad = p.n_tile_cv + gb; gb += (b.n_cvs + 63) / 64; }
}
uint32_t plan_small_tiles(const PlanBuf &p);  // tiles of whole small units (the fused kernels' work)
uint32_t plan_max_cvs(const PlanBuf &p);      // tile CVs of the biggest unit (picks the merge launch)

// ---- table shape ----------------------------------------------------------------------------------------------------------------
struct RowCols {  // the caller's columns from row_begin on (host memory)
    const uint64_t *bo, *bs, *us, *oo;
    const uint8_t *bitmap;
    uint64_t row_begin, row_end;
    bool allc;  // every row compressed (the usual archive): the per-row passes skip the bit column
    uint32_t comp(uint32_t i) const { if (allc) return 1u; const uint64_t row = row_begin + i; return (bitmap[row >> 3] >> (row & 7)) & 1u; }
};
bool rows_all_compressed(const uint8_t *bitmap, uint64_t row_begin, uint64_t row_end);  // no bitmap: every row is

struct RowClasses {  // what the pass over the columns finds about the compressed rows above 64 KiB (rows_classify)
    std::vector<uint32_t> la, cand_row, cand_base, cand_nb, item_row, item_k, fz_base, fz_cap, fz_it_cand;
    std::vector<uint32_t> bt_tile, bt_item;  // fused block kernel: the big-slice tiles of the candidate rows, the item each belongs to
    uint64_t big_bytes = 0, big_blob = 0, n_big = 0, nblk = 0;
};

// The values of the context's switches (ZNIPPY_* environment, read once per context) that this module reads.
struct RowsSwitches {
    int dbg = 0;  // ZNIPPY_DBG bit set (FusedArgs::dbg)
    bool no_block_items = false, no_fused_blocks = false, ddbg = false, no_roles = false, no_fz = false, no_bx = false, no_rx = false, no_lean = false, no_stored_only = false;
    // ZNIPPY_ROLES_MIN: small tiles from which the role-split persistent kernel takes the table (0 = never; below
    // a few CU-fillings a persistent grid only adds start-up latency)
    unsigned roles_min = 2048;
    unsigned bx_big = 2048;  // ZNIPPY_BX_BIG (default: BX_BIG_SEQ)
    bool bx_big_set = false;
};

// What creation learns about a table; nothing here changes afterwards.
struct RowsShape {
    uint32_t n = 0;
    uint32_t n_compressed = 0;
    uint32_t n_list_a = 0;         // compressed rows with > 64 leaves that are no block candidates: general decoder
    uint32_t n_cand = 0, n_items = 0;  // block items: compressed rows of >= 2 blocks are tried block by block first
    uint32_t n_bt = 0;             // fused block kernel: big-slice tiles of the candidate rows
    uint32_t n_small_tiles = 0;    // tiles of whole small rows (the fused kernels' work)
    uint32_t n_tiles = 0, n_big_units = 0;
    // two-phase path for the candidates the block-item path gives up on (foreign frames): item slots per candidate
    // (2 x the expected blocks + 8: a writer may split blocks), content bytes of all candidates
    uint32_t fz_total = 0;
    uint64_t fz_bytes = 0;
    // batch path (k_bx_*): candidate slots (one per compressed row at most), item slots
    uint32_t bx_slots = 0, bx_item_cap = 0;
    uint64_t bx_bytes = 0;  // content bytes of all compressed rows
    uint64_t bx_nblk = 0;   // their 128 KiB blocks, as the index columns have them
    uint64_t rx_words = 0;  // resolve path: words its frames (compressed rows of >= rx_min bytes) can ask for
    uint64_t rx_words_small = 0;  // ... counting every row above 64 KiB
    uint32_t rx_min = zn::RX_MIN;  // a table whose rows above 64 KiB are few (<= 256 M words) resolves all of them: one wave per frame is the slower way
                                   // when the frames do not fill the chip (the image's source text: its 64-256 KiB frames were 1.6 ms of one-wave execution)
    bool rx_frames = false;        // the table has batch slots and rows the resolve path may take: it gets that path's buffers (ZNIPPY_NO_RX: never)
    int xxh_forms = 0;             // checksum stage: the forms the rows call for (BxArgs::xxh_forms)
    bool odd_out = false;          // some stored row's output offset is not a multiple of 16 (store-path kernel variant)
    bool wide_rows = false;        // big rows average >= 1 MiB: 1024-thread workgroups
    // extents of the table's rows: a run whose regions contain them has no bad row (rows_fit)
    uint64_t ext_min_bo = 0, ext_max_bend = 0, ext_max_oend = 0;
    bool ext_wrap = false;
    bool small_ok = false;         // small compressed rows only, with batch slots: a run may give every row to the batch path (RowsHints::small_off)
    bool lean_ok = false;          // the table's shape allows lean runs: small rows only
    bool lean_mixed_ok = false;    // small rows beside big stored / hashed units: the small rows' kernel beside the second hash pass
    bool lean_blocks_ok = false;   // big multi-block rows only (the fused block kernel in front)
};

// ONE pass over the caller's columns: the flags the runs need, the extents a run is validated against, and the big rows.
// Compressed rows above 64 KiB: frames of >= 2 blocks (and < 4 GiB) are tried block by block (each block a work item),
// the others go straight to the general decoder.  Then, from the counts and the tile plan `p` of the same columns: the batch
// path's capacities, the resolve threshold, the workgroup width, the lean shapes and the fused block kernel's lists.
void rows_classify(const RowCols &c, const RowsSwitches &sw, const PlanBuf &p, RowsShape &s, RowClasses &k);
// the done flags of the fused block kernel, tiles then items, in one allocation (one clear per run): its size, and where the items' flags start
size_t rows_done_bytes(const RowsShape &s, size_t *items_at);

// ---- hints ----------------------------------------------------------------------------------------------------------------------
// What a table remembers of its last finished run, and what the host has found wrong with it.
struct RowsHints {
    // Does the batch path have anything to do?  Its six launches cost ~0.1 ms even when every list is empty (the BASELINE
    // archives: every row is taken by the fused kernels): -1 not known yet (launch it), 0 nothing handed over (the serial
    // decoder alone stands behind the fused kernels, as a safety net), 1 something was.
    int bx_hint = -1;
    // Lean runs.  A table of small rows whose last finished run left nothing behind the role-split kernel — no tile on its
    // list, no row handed over — is run as memset + that kernel + verify: the three launches behind it (left-over tiles,
    // serial decoder, second hash pass) cost ~25 us of a 0.5 ms step for looking at empty lists.  The verify kernel checks
    // the lists; if this run did leave something (the blobs changed), its counters come back flagged and whoever reads the
    // run's results first runs it again in full — same inputs, the results the caller would have had.
    int lean_hint = -1;   // last finished run: 1 nothing left behind the roles kernel, 0 something was, -1 not known
    int lean_hint2 = -1;  // the same for the fused block kernel and the block items
    // Decode-only runs neither use up nor update the hints above (they cannot be flagged, so nothing they skip may be something a row
    // needs).  What they do keep is their own answer to bx_hint's question, which only ROUTES the undecoded frames (batch path, or the
    // serial decoders alone, which take whatever is handed over): a wrong answer costs time, never a row.  -1: not known (bx_hint is consulted)
    int plain_hint = -1;
    bool roles_off = false;   // a run of the role-split kernel left every tile on its list (rows of no shape it takes: 0.15 ms of looking)
    bool small_off = false;   // the fused kernels handed over every row: later runs skip them (the batch path's list is all rows)
    bool force_full = false;  // a lean run came back flagged, or a run failed: this table runs in full from now on
    uint32_t n_bad = 0;       // rows whose status the host decided for the run's regions (rows_verdicts)
};
struct HandCounts { uint32_t fused, serial, flagged, tiles, items; };  // a finished run's hand-over counts (api.hip: Hand)
// what a finished run's mirror says about the batch path's work: rows the fused kernel handed over + block candidates left
// flagged + the host's own list of big single-block rows
void rows_note_hint(const RowsShape &s, RowsHints &h, const HandCounts &left);
void rows_note_plain(const RowsShape &s, RowsHints &h, const HandCounts &left);  // the same reading of a decode-only run's mirror, into its own field
inline int rows_route_hint(const RowsHints &h, bool plain) { return plain && h.plain_hint >= 0 ? h.plain_hint : h.bx_hint; }  // the routing hint a run goes by: a decode-only run's own once it has one
void rows_force_full(RowsHints &h);  // a flagged or a failed run

// ---- run plan -------------------------------------------------------------------------------------------------------------------
struct RunEnv {  // the context (and the table's optional buffers) as a run finds it
    bool fz_lit_pool, fz_seq_pool, bx_fse_pool, bx_huf_pool, rx_pool;  // the pools exist
    bool rx_base;          // the table has the resolve path's buffers
    uint64_t rx_cap;       // words
    int cus, decode_grid;
    int gen_share;         // workgroups per CU the general decoder takes while block items / foreign frames run beside it (4 = the whole register file)
    bool xxh;              // batch checksums are on and the table has its list for them (bx_cand_ck)
    bool fork_verify;      // a lean run's verify goes to the auxiliary stream
    bool dst_misaligned;   // the run's output pointer is not 16-byte aligned
    const RowsSwitches *sw;
};
// Which kernels a run launches and on which streams.  Everything here is known before the run's first launch — the context's
// switches and pools, the table's shape, the hints of its last finished run.
struct RunPlan {
    bool empty;        // no row: the run is its clear
    bool bx;           // the batch path takes the undecoded frames (its pools exist, the last run did not find its lists empty)
    bool small_off;    // ... every row of the table: the fused small-row kernels are left out, all_rows is its list
    bool stored_only;  // no compressed row: one pass of the store path kernel over ALL tiles instead of stages 1 and 2
    bool roles;        // the role-split persistent kernel in front of k_fused_small
    bool lean;         // nothing behind the roles kernel but the verify, which checks the lists (rows_settle repeats a flagged run)
    bool lean_mixed;   // small rows beside big stored units: the small rows' kernels on the auxiliary stream beside the second hash pass
    bool small;        // k_fused_small (decode-only: its store-only form) runs ...
    int small_grid_cap;  // ... with at most this many workgroups (0: one per tile)
    bool decode;       // stage 2 runs: block items and the decoders behind the fused kernels
    bool items;        // ... the block items: header scan, fused block kernel, block decoder, two-phase path
    bool fused_blocks; // the fused block kernel and the compaction of what it leaves
    bool block_decoder;  // the serial block decoder behind it
    bool two_phase;    // round-2 two-phase path for the candidates the block items give up on
    bool decoders;     // ... the batch path (bx) or the serial flow
    bool one_stream;   // block items on the main stream: nothing else is expected there
    bool lean_blocks;  // ... and neither the block decoder nor the serial decoders behind the fused block kernel
    bool behind;       // round-2 flow: the general decoder behind the block items instead of beside them
    bool rx;           // batch path: big frames through the resolve stages
    bool third;        // batch path: the lane-per-block sequence kernel on a third stream beside the Huffman streams
    bool xxh;          // batch path: the checksum stage
    int items_grid, general_grid, fallback_grid;  // the block decoder's, the general decoder's, the last serial launch's workgroups
    uint32_t big_seq;  // batch path: blocks of this many sequences get a wave of their own; 0: picked from the table's histogram
    bool small_frames; // batch path: the table's frames average <= 64 KiB (the execute stage's small-window variant)
    uint64_t rx_bound; // resolve path: bound on the words a run can use (grid sizing)
    bool misaligned_dst;  // store path: some copy destination is not 16-byte aligned
    bool hash_skips_done;  // second hash pass: tiles the fused block kernel has hashed are skipped (tile_done)
    bool merge_big;    // ... and the big units' trees behind it
    bool copy_stored;  // decode-only: the copy of the stored rows no kernel in front has written
    bool check_lists;  // the run left stages out: the verify checks that their lists are empty ...
    bool lists_small;  // ... the small rows' lists (LEAN_SMALL), else the block items' (LEAN_BLOCKS)
    bool verify_aux;   // verify, result copy and the run's event on the auxiliary stream
};
// preset: the status column starts as the host's verdicts; verify: a verify-only run; plain: a decode-only run
RunPlan rows_plan(const RowsShape &s, const RowsHints &h, const RunEnv &e, int preset, bool verify, bool plain);

// ---- pool sizes -----------------------------------------------------------------------------------------------------------------
constexpr uint64_t POOL_REFUSED = ~0ull;  // more than a pool may hold: the call is refused
struct FzPoolSizes { uint64_t lit_bytes, seq_records; };
struct BxPoolSizes { uint64_t fse_cells, huf_cells; };
// Pools of the two-phase foreign-frame path.  Literals: a block's literals never exceed what it regenerates, so the
// candidates' content bytes (+ 80 bytes of slack per item) always suffice.  Sequence records (8 bytes each): real data
// runs at one sequence per 8-20 bytes; 1.5 bytes of pool per content byte covers one per 5.3 bytes, and a block that
// finds the pool empty simply stays with the serial decoder.  Both are capped (a 100 GB archive does not get 250 GB
// of scratch): what does not fit is decoded serially.
FzPoolSizes fz_pool_sizes(uint64_t content_bytes, uint32_t items);
// Table pools of the batch path (2-byte cells): a 10 KiB text frame needs ~1.5 KB of FSE cells and ~2 KB of Huffman cells; half a
// byte of each per content byte (+ 64 bytes per item) covers frames down to ~1 KiB, and a block that finds a pool empty stays with
// the serial decoder.  The FSE pool has the predefined tables at its head.
BxPoolSizes bx_pool_sizes(uint64_t content_bytes, uint32_t items);
// Word pool of the resolve path: 4 bytes per output byte of the frames it takes, in chunks of 1,024 words, at most 2^31 - 2^20
// words (a word with bit 31 clear is an index).  Frames that find no room are executed by a wave each.
uint64_t rx_pool_words(uint64_t words);
// Scratch of the verify-only runs: the slots of one table (+ slack for 16-byte reads behind the last one).  Unlike the pools above it
// is not optional — the rows that need it have nowhere else to go — and it is capped like them.  0: nothing is needed.
uint64_t verify_scratch_bytes(uint64_t bytes);
// Scratch of the range reads, capped the same way, both regions together (other_cap: what the other region holds).
uint64_t range_scratch_bytes(uint64_t bytes, uint64_t other_cap);

// ---- validation -----------------------------------------------------------------------------------------------------------------
// Every row's source range against the declared blob region (blob_cap ~0: not declared) and its output range against out_cap.
// A table whose extents fit the run's regions has no bad row.  (verify-only runs: the output side is the table's own slots in the
// scratch, which fit by construction — only the blob side is looked at.)
bool rows_fit(const RowsShape &s, uint64_t blob_base, uint64_t blob_cap, uint64_t out_cap, bool verify);
// The per-row pass for the other tables, overflow-safe: status[i] = RP_E_CORRUPT / RP_E_DST_SMALL for a bad row (status is sized
// and zeroed at the first one); returns their number.  verify: len and oo are not read.
uint32_t rows_verdicts(const uint64_t *bo, const uint64_t *bs, const uint64_t *len, const uint64_t *oo, uint32_t n, uint64_t blob_base, uint64_t blob_cap,
                       uint64_t out_cap, bool verify, std::vector<int32_t> &status);
