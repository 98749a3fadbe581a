// Shared host/device declarations for libznippy_hip.so (internal; the public surface is
// include/znippy_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "host/bz_plan.h"        // the lists of znippy_bunzip2_batch
#include "host/deflate_batch.h"  // the lists of the DEFLATE batch calls
#include "host/gz_cut_plan.h"    // the lists of the block-start search of znippy_gunzip_batch
#include "host/range_plan.h"
#include "host/rows_plan.h"  // Tile, BigUnit and the constants the read side's host plan shares with the kernels
#include "host/xz_plan.h"    // the lists of znippy_unxz_batch
#include "host/tar_list_plan.h"  // the lists of znippy_tar_list_batch

namespace zn {

// Where each unit's bytes live.  Units with sel==0 (or all units when sel==nullptr) are hashed
// from srcA+offA[u]; when copy_to_B is set those bytes are also copied to srcB+offB[u] (store
// path: blob -> output, fused with the hash).  Units with sel!=0 are hashed from srcB+offB[u]
// (decoded output of the zstd kernel).
struct HashArgs {
    const Tile *tiles;
    uint32_t n_tiles;
    const uint64_t *len;
    const uint8_t *srcA;
    const uint64_t *offA;
    uint64_t baseA;  // subtracted from offA (blob_base)
    uint8_t *srcB;
    const uint64_t *offB;
    const uint8_t *sel;
    const int32_t *status;          // per-unit decode status (read side), see hash_dev.h PASS_*
    const uint32_t *pending_count;  // rows handed to the general decoder (PASS_SECOND early-out)
    int pass;
    int copy_to_B;
    uint32_t *digests;  // 8 words per unit
    uint32_t *tile_cv;  // 8 words per big-unit tile
    int store_tiles;     // store path (copy_to_B): 0 = tiles per wave picked from the tile count; 1 / 2 = forced (ZNIPPY_STORE_G, A/B and tests)
    int fold_tiles_max;  // 0 = pick from the tile count; 1 = no deferred folding (no LDS: the launch shares the CUs with the encoder)
    const uint8_t *tile_done;  // optional, PASS_SECOND: tiles already hashed by the fused block kernel
    // optional (write side, store-heavy tables): copy only units with copy_mask != 0, and only if they end inside copy_cap
    const uint8_t *copy_mask;
    uint64_t copy_cap;
    int misaligned_dst;  // store path: some copy destination is not 16-byte aligned (host knowledge; picks the kernel variant)
};

// Row status values on the read side: 0 = done (stored row, or decoded+hashed by the fused
// small-row kernel), 1 = handed to the general decoder, 2 = decoded by the general decoder
// (still to be hashed by the second pass), < 0 = ZNIPPY_E_* (frame failed to decode).
struct DecodeArgs {
    const uint32_t *list_a;         // rows the host routes to the general decoder (big compressed rows)
    uint32_t n_list_a;
    const uint32_t *pending;        // rows the fused kernel could not handle
    const uint32_t *pending_count;
    const uint8_t *blobs;
    uint64_t blob_base;
    const uint64_t *blob_off, *blob_size, *usize, *out_off;
    const uint8_t *compressed;  // per row 0/1
    uint8_t *out;
    uint64_t out_cap;
    int32_t *status;
    uint32_t n_rows;
    uint32_t *cursor;    // atomic row cursor (the reference's AtomicUsize, decompress.rs:L104)
    uint8_t *lit_scratch;  // per resident workgroup: LIT_SCRATCH bytes
    unsigned long long *dbg;  // diagnostic only (ZNIPPY_DDBG): phase cycle counters [items, literals, seq tables, seq decode, execute, tail], never an output
    // Block items: frames of >= 2 blocks are first tried block by block, every block a work item of its own (a
    // frame written by this library has self-contained 128 KiB blocks; any frame that turns out not to — repeat
    // offsets, reused tables, a match reaching into an earlier block, another block size — is flagged and decoded
    // serially afterwards).  block_mode != 0: the work list is the item table instead of rows.
    int block_mode;
    const uint32_t *item_row, *item_k;  // item -> row, block index inside the row's frame
    const uint32_t *item_src;           // item -> offset of the block header inside the frame (0xFFFFFFFF: skip)
    uint32_t n_items;
    uint32_t *row_flag;                 // per row, != 0: decode this frame serially
    const uint8_t *item_done;           // optional: items already written (and hashed) by the fused block kernel
    const uint32_t *todo, *n_todo;      // optional: the items that are left (k_compact_items); n_work = *n_todo
    uint32_t *seq_scratch;
    int preset;  // != 0: status[] was initialised with the host's verdicts — a row with status < 0 is left alone
};

struct FusedArgs {
    HashArgs h;  // tiles, len (= usize), srcA = blobs, srcB = out, sel = compressed, status, digests
    const uint64_t *blob_size;
    uint64_t out_cap;
    int32_t *status;
    uint32_t *pending;
    uint32_t *pending_count;
    // diagnostic only (ZNIPPY_DBG, bit set): 1 skip the hash, 2 skip the decode, 4 hash recognised rows from the output
    // instead of their windows, 8 phase stamps -> dbg_buf, 16 no row stores, 32 no pattern expansion (scalar decoder),
    // 64 no s_setprio on the scalar decoder, 128 no lane-parallel recognition, 256 parent trees folded per wave
    int dbg;
    unsigned long long *dbg_buf;  // diagnostic stamps (ZNIPPY_DBG & 8); with bit 32768 the clock buffer of roles_clk_bytes() bytes
    uint32_t lds_pad;  // extra dynamic LDS per block: caps blocks/CU (in-flight footprint vs Infinity Cache)
    int preset;        // != 0: status[] was initialised with the host's verdicts — a row with status < 0 is left alone
    // role-split kernel (k_fused_roles): global work cursor over the plan's tiles, and the tiles it leaves to
    // k_fused_small (any tile that is not all "whole-leaf rows of the recognised periodic shape")
    uint32_t *cursor;
    uint32_t *tile_list;         // k_fused_roles: slow list (out); k_fused_small: tiles to process (nullptr = all)
    uint32_t *tile_count;
};

// Block items of the common shape (fused_small.hip, k_fused_blocks): the big-slice tiles of block-candidate rows.
struct FusedBlocksArgs {
    HashArgs h;  // as for the fused small-row kernel, pass = PASS_ALL
    const uint64_t *blob_size;
    const uint32_t *bt_tile, *bt_item;  // tile index in the plan, block item the tile belongs to
    uint32_t n_bt;
    const uint32_t *item_src;  // written by k_scan_blocks
    const uint32_t *row_flag;
    uint8_t *tile_done, *item_done;  // zeroed before the launch
    int dbg;
};
// verify (here and below): the no-store instantiation of the kernel (verify-only runs: rows are hashed, not written)
void launch_fused_blocks(const FusedBlocksArgs &a, hipStream_t s, bool verify = false);

void launch_hash_tiles(const HashArgs &a, hipStream_t s);
void launch_fused_small(const FusedArgs &a, hipStream_t s, int grid_cap = 0, bool verify = false);
void launch_fused_roles(const FusedArgs &a, int cus, hipStream_t s, bool verify = false);
void init_fused_tables();
// decode-only runs (znippy_decode_rows): the store-only forms of the three kernels above — small rows, block items of the common
// shape, stored rows above a tile (all = every tile: stored-only tables) — nothing is hashed
void launch_decode_small(const FusedArgs &a, hipStream_t s);
void launch_decode_blocks(const FusedBlocksArgs &a, hipStream_t s);
void launch_copy_stored(const HashArgs &a, bool all, hipStream_t s);
void launch_merge_big(const BigUnit *big, uint32_t n_big, uint32_t *tile_cv, uint32_t *digests, const uint32_t *grp_big,
                      const uint32_t *grp_k, uint32_t n_grp, uint32_t max_cvs, hipStream_t s);
void launch_verify(const uint32_t *digests, const uint8_t *checksum, const uint64_t *usize,
                   const int32_t *status, uint32_t n_rows, uint64_t row_begin, uint64_t *counters,
                   uint64_t *corrupt_rows, uint32_t corrupt_cap, hipStream_t s, const uint32_t *lean_lists = nullptr, uint32_t lean_mask = 0);
// what the two kernels take of a CU, from hipFuncGetAttributes (-1: not known)
int verify_footprint(int *regs, int *lds);
int roles_footprint(int *regs, int *waves_per_simd, int *lds);
size_t roles_clk_bytes(int cus);       // the ZNIPPY_DBG & 32768 buffer: 8 words, then 8 per wave of every workgroup a launch can have
void roles_geometry(uint32_t g[4]);    // waves per workgroup, ring slots, workgroups per CU, sizeof(RolesShared)
int decode_grid_size(int device);
void launch_decode(const DecodeArgs &a, int grid, bool wide, hipStream_t s);
// block-item path: header scan of the candidate frames, then (after the block-mode decode) the per-row verdict
struct BlockScanArgs {
    const uint32_t *cand_row, *cand_base, *cand_nblocks;  // candidate -> row, first item, number of items
    uint32_t n_cand;
    const uint8_t *blobs;
    uint64_t blob_base;
    const uint64_t *blob_off, *blob_size, *usize, *out_off;
    uint64_t out_cap;
    uint32_t *item_src;
    uint32_t *row_flag;
    int32_t *status;
    uint32_t *pending, *pending_count;
    int preset;  // != 0: rows with status < 0 (host verdict) are not candidates
};
void launch_scan_blocks(const BlockScanArgs &a, hipStream_t s);
void launch_compact_items(const uint8_t *item_done, uint32_t n_items, uint32_t *todo, uint32_t *n_todo, hipStream_t s);
void launch_finish_blocks(const BlockScanArgs &a, hipStream_t s, bool defer_flagged);  // defer_flagged: a flagged candidate is left to the batch path

// Foreign frames in two phases (zstd_decode.hip, k_fz_*): frames of >= 2 blocks that the block-item path gave up on
// (another writer's frames: repeat offsets, reused entropy tables, matches reaching into earlier blocks, any block
// size) are decoded block-PARALLEL where the format allows it — every block's literals and sequences are entropy-
// decoded by its own workgroup into scratch pools — and only the byte-moving sequence execution walks a frame in order.
struct FzItem {
    uint32_t src;       // offset of the block header inside the frame (written by the scan)
    uint32_t out;       // bytes the block regenerates
    uint32_t nseq;
    uint32_t lit_len;
    uint64_t seq_off;   // first record in the sequence pool
    uint64_t lit_off;   // lit_kind 0: offset inside the frame's blob; 1: the byte; 2: offset in the literal pool
    uint32_t lit_kind;
    int32_t err;        // != 0: this block needs the serial decoder (which also produces the error code)
    // Repeat offsets are resolved while the sequences are decoded (one scalar walk per block, all blocks at once),
    // against an UNKNOWN incoming history: a value is an offset, or FZ_SYM | k << 26 | d = "incoming entry k, minus d".
    // rep[] = the history the block leaves, in the same notation; the execute kernel substitutes frame by frame.
    uint32_t rep[3];
    uint32_t pad;
};
constexpr uint32_t FZ_SYM = 1u << 28;
struct FzArgs {
    const uint32_t *cand_row, *cand_fzbase, *cand_fzcap;  // candidate -> row, first item slot, item slots
    uint32_t n_cand;
    const uint32_t *it_cand;  // item slot -> candidate
    uint32_t total_items;
    uint32_t *cand_nb;        // blocks found per candidate (0: not taken by this path)
    FzItem *items;
    const uint8_t *blobs;
    uint64_t blob_base;
    const uint64_t *blob_off, *blob_size, *usize, *out_off;
    uint64_t out_cap;
    uint8_t *out;
    uint32_t *row_flag;       // in: != 0 = the block-item path gave up; out: 0 once the frame is decoded here
    const int32_t *status;
    int preset;
    uint8_t *lit_pool;
    uint64_t lit_cap;         // bytes
    unsigned long long *seq_pool;
    uint64_t seq_cap;         // records
    unsigned long long *pool_used;  // [0] literal bytes, [1] sequence records handed out, [2] frames decoded, [3] blocks given up (zeroed per run)
    uint32_t *cursor;
    unsigned long long *dbg;  // diagnostic only (ZNIPPY_DDBG): cycle / event counters of the execute kernel
};
void launch_fz_scan(const FzArgs &a, uint32_t *work, uint32_t *work_count, hipStream_t s);
void launch_fz_entropy(const FzArgs &a, int cus, const uint32_t *work, const uint32_t *work_count, hipStream_t s);
void launch_fz_exec(const FzArgs &a, hipStream_t s);

// Many foreign frames at once (zstd_batch.hip, k_bx_*): the serial chains of a block — table descriptions, Huffman
// streams, the FSE sequence bitstream — are decoded with LANE = block (or stream), 64 of them per wave, tables in
// scratch pools in device memory; execution stays wave = frame (k_fz_exec's body).  Everything is sized and listed on
// the device: the candidates are the host's list of big single-block rows, the rows the fused kernel handed over, and
// the block candidates the block-item path flagged.
struct BxPrep {            // per block item, written by k_bx_prep
    uint32_t frame;        // candidate slot
    uint32_t k;            // index of the block inside its frame
    uint32_t n_streams;    // Huffman streams (0: raw / RLE literals)
    uint32_t huf_off;      // decoding table in the Huffman pool (u16 cells), 1 << huf_log of them
    uint32_t huf_log;
    uint32_t st_off[4];    // streams: offset from the frame's first byte, bytes
    uint32_t st_len[4];
    uint32_t tab[3];       // LL / OF / ML decoding table in the FSE pool (2-byte cells, 16-byte aligned)
    uint32_t logs;         // log LL | log OF << 8 | log ML << 16
    uint32_t bs_off;       // sequences bitstream: offset from the frame's first byte
    uint32_t bs_len;       // bytes
};
constexpr uint32_t BX_BIG_SEQ = 2048;  // blocks of this many sequences get a wave of their own in the sequence stage
// FSE pool cell (2 bytes): symbol:6 | ns:10 << 6 (zstd_batch.hip)
struct BxArgs {
    const uint32_t *list_a; uint32_t n_list_a;
    const uint32_t *pending; const uint32_t *pending_count;
    const uint32_t *bc_row; uint32_t n_bc;  // block candidates: taken when row_flag != 0
    const uint8_t *blobs; uint64_t blob_base;
    const uint64_t *blob_off, *blob_size, *usize, *out_off;
    uint64_t out_cap;
    uint8_t *out;
    int32_t *status;
    int preset;
    uint32_t *row_flag;  // per row: 1 = taken here and not (yet) decoded
    uint32_t *cand_row, *cand_base, *cand_nb;  // per candidate slot (written by the scan)
    uint32_t slot_cap;
    FzItem *items; BxPrep *prep; uint32_t item_cap;
    uint32_t *ctr;  // [0] slots, [1] items, [2] Huffman list, [3] [5] [6] [7] sequence lists (64 / 32 / 16 / 1 blocks per wave), [4] execute cursor, [8] cursor of the wave-per-block list (zeroed per run)
    uint32_t *sort_tmp;  // 5 x item_cap entries: scratch of k_bx_sort
    uint32_t *huf_list, *seq_list;  // seq_list: four lists of item_cap entries (64 / 32 / 16 blocks per wave, wave per block)
    uint8_t *lit_pool; uint64_t lit_cap;
    unsigned long long *seq_pool; uint64_t seq_cap;
    uint16_t *fse_pool; uint64_t fse_cap;   // cells
    uint16_t *huf_pool; uint64_t huf_cap;   // cells
    unsigned long long *pool_used;  // [0] literal bytes [1] records [2] frames decoded [3] blocks given up [4..7] why [8] FSE cells [9] Huffman cells (zeroed per run)
    uint32_t *pending2, *pending2_count;  // what is left for the serial decoder
    unsigned long long *dbg;
    int small_frames;  // the table's frames average <= 64 KiB: the execute stage runs its small-window variant (more frames per CU)
    uint32_t big_seq;  // blocks of this many sequences get a wave of their own (BX_BIG_SEQ; ZNIPPY_BX_BIG for A/B runs)
    // The resolve path (k_rx_*): frames of >= RX_MIN bytes are not executed by one wave each but resolved in parallel — every
    // output byte gets a 32-bit word, RX_DONE | value for a literal byte, the word index it copies from for a match byte;
    // rounds of pointer jumping turn every word into a value; a last pass stores the bytes.  ctr[9] list length, [10] expand
    // cursor, [11] frames taken; pool_used[10] words handed out, [11] words in use (the extent the rounds run over).
    uint32_t *rx_ptr; uint64_t rx_cap;  // the word pool (rx_cap < 2^31 words: a word with bit 31 clear is an index)
    uint32_t *rx_chunk;                 // 1,024-word chunk of the pool -> candidate slot
    uint8_t *rx_cdone;                  // ... -> every word of the chunk is a value (set by a jump round, cleared by the plan)
    uint32_t *rx_base, *rx_fail;        // per candidate slot: first word (RX_NONE: not taken), a block did not check out
    uint32_t *rx_blk;                   // per block item: first output byte inside the frame, incoming repeat offsets [3]
    uint32_t *rx_list;                  // block items to expand
    uint32_t *rx_pending;               // [round]: words still unresolved after that round (zeroed per run)
    uint64_t rx_bound;                  // host's bound on the words a run can use (grid sizing)
    uint32_t rx_min;                    // frames of at least this many bytes are resolved (RX_MIN; less for tables with few rows above 64 KiB)
    // The checksum stage (k_bx_xxh_*, znippy_ctx_set_batch_checksums).  xxh_on is the context's switch as this run found it: the scan
    // then takes frames that end with a Content_Checksum trailer and notes them in cand_ck; the stage hashes what was decoded here
    // and hands a frame whose trailer differs back to the serial decoder (row_flag / rx_fail), which reports it.
    int xxh_on;
    int xxh_forms;                      // the forms the table's row sizes call for: bit 0 four lanes per frame (rows below XXH_WAVE_MIN), bit 1 a wave per frame
    uint32_t *cand_ck;                  // per candidate slot (written by the scan when xxh_on): 1 = the frame's last 4 bytes are its checksum
    unsigned long long *xxh_stat;       // [0] frames checked and right, [1] checked and wrong, [2] content bytes hashed (zeroed per run)
};
constexpr uint32_t RX_NONE = 0xFFFFFFFFu, RX_DONE = 0x80000000u, RX_ROUNDS = 12, RX_JUMPS = 6;
// the batch path's launches, in the order of a run: scan, prep (the tables), sort the work lists, fse (wave = block) beside huf
// and fse (lane = block), then exec — or the resolve path: plan, exec beside expand, jump round r, store —, the content checksums
// (xxh: only with BxArgs::xxh_on), finish
enum BxStage : int { BX_SCAN = 0, BX_PREP = 1, BX_HUF = 2, BX_FSE = 3, BX_EXEC = 4, BX_FINISH = 5, BX_FSE_WAVE = 6, BX_SORT = 7, BX_RX_PLAN = 8, BX_RX_EXPAND = 9,
                     BX_RX_JUMP = 10 /* + r */, BX_RX_STORE = 30, BX_XXH = 31 };
void launch_bx_stage(const BxArgs &a, int cus, int stage, hipStream_t s);  // stage: a BxStage
void bx_predefined_tables(uint16_t cells[160]);  // host: the three predefined tables as pool cells

// Range reads (range_gather.hip) and the block tree (block_tree.hip): RangePiece, RANGE_PIECE, BlockCvItem and BlockTreeRow are in
// host/range_plan.h, beside the host code that builds the lists of them (host/range_plan.cc) — plain C++ that a stand-alone program
// tests, which this header, with its HIP include, is not.
void launch_range_gather(const RangePiece *pieces, uint32_t n_pieces, hipStream_t s);
// per private row of the partial route: late[i] = the row goes to the whole-row pass; *decoded += block_bytes[i] of the others
void launch_range_status(const uint32_t *row_flag, const uint64_t *block_bytes, uint32_t n_rows, uint8_t *late, unsigned long long *decoded, hipStream_t s);

// Block tree (block_tree.hip): one 32-byte entry per 128 KiB block of a row of more than one block (and below 4 GiB).
// write mode: out != NULL; compare mode: expect != NULL, verdict[item] = 1 if the block's chaining value equals expect[slot]
void launch_block_cvs(const BlockCvItem *items, uint32_t n_items, uint32_t *out, const uint32_t *expect, uint32_t *verdict, hipStream_t s);
// verdict[i] = 1 if rows[i]'s entries fold to checksum[32 * row ..]
void launch_block_tree_fold(const BlockTreeRow *rows, uint32_t n_rows, const uint32_t *tree, const uint8_t *checksum, uint32_t *verdict, hipStream_t s);
// Write side (znippy_rounds_emit_block_tree): one big unit of a rounds table that has entries, in round order; the list ends with a
// sentinel whose `first` is the table's entry count
struct TreeUnit {
    uint32_t first;    // its first entry in the table's tree
    uint32_t cv_base;  // BigUnit::cv_base
    uint32_t n_cvs;    // BigUnit::n_cvs (>= 3): the unit has ceil(n_cvs / 2) entries
    uint32_t pad;
};
// tree[e] for every entry e of the table, from the tile CVs the run's hash left in tile_cv (read only)
void launch_round_block_entries(const TreeUnit *units, uint32_t n_units, uint32_t n_entries, const uint32_t *tile_cv, uint32_t *tree, hipStream_t s);


// The DEFLATE batch calls (inflate.hip, targz.hip, gunzip.hip): InflateItem, TargzItem, TargzResult, GzItem, GzScanChunk, GzCand,
// GzProbe, GzRun, GzSingle and GZ_SCAN_CHUNK are in host/deflate_batch.h, beside the host code that builds and reads the lists of them
// (host/deflate_batch.cc), for the reason given at RangePiece above.
// Raw DEFLATE of ZIP entries (znippy_inflate_batch): one wave per item the host has validated.
// status[i] = 0 or ZNIPPY_E_* for every item; no byte outside [dst, dst + out_len) of any item is written
void launch_inflate(const InflateItem *items, uint32_t n_items, int32_t *status, hipStream_t s);
// for every item with status 0: crc_out[i] = CRC-32 of its out_len bytes; status[i] = ZNIPPY_E_CHECKSUM where has_crc and it is not want_crc
void launch_inflate_crc(const InflateItem *items, uint32_t n_items, int32_t *status, uint32_t *crc_out, hipStream_t s);

// One tar member out of gzip-compressed tars (znippy_targz_find_batch): one wave per item, decoding only as far as the tar has to be read.
// filter: name_prefix then name_suffix, in device memory.  res[i] for every item; no byte outside [scratch, scratch + cap) is written
void launch_targz_find(const TargzItem *items, uint32_t n_items, const uint8_t *filter, uint32_t prefix_len, uint32_t suffix_len, TargzResult *res,
                       hipStream_t s);

// Whole gzip files (znippy_gunzip_batch).
// count[i] = candidates found in item i (byte 0 not among them); the first cand_cap of them, in no order, as pos << 1 | kind
// (0: behind 00 00 FF FF, 1: at 1F 8B 08) in cands[cand_base ..]
void launch_gunzip_scan(const GzItem *items, const GzScanChunk *chunks, uint32_t n_chunks, uint32_t *count, uint64_t *cands, hipStream_t s);
void launch_gunzip_probe(const GzItem *items, const GzCand *cands, uint32_t n_cands, const uint32_t *stops, GzProbe *recs, hipStream_t s);
void launch_gunzip_inflate(const GzItem *items, const GzRun *runs, uint32_t n_runs, int32_t *status, hipStream_t s);
// The block-start search (host/gz_cut_plan.h): slots[] starts as NONE everywhere and *passed as 0.  Every bit position of every
// searched item is tested (gz_cut_rules.h); a position that passes is counted and lowers the slot of its window of `cut` bytes.
void launch_gunzip_find(const gzcut::FindItem *items, const gzcut::FindChunk *chunks, uint32_t n_chunks, uint32_t cut, unsigned long long *slots,
                        unsigned long long *passed, hipStream_t s);
// The cut at the block starts found (host/gz_cut_plan.h): a record per candidate; the pieces of a pass decoded (status[k] of piece k:
// 0 or a ZNIPPY_E_*), marker pieces into scratch; then their last 32 KiB, group by group, and the rest of them made bytes.  The
// pieces and groups given are those of one pass; *resolved is added to.
void launch_gunzip_cut_probe(const GzItem *items, const gzcut::CutCand *cands, uint32_t n_cands, const uint64_t *stops, gzcut::CutRec *recs, hipStream_t s);
void launch_gunzip_cut_decode(const GzItem *items, const gzcut::CutPiece *pieces, uint32_t n_pieces, uint16_t *scratch, int32_t *status, hipStream_t s);
void launch_gunzip_cut_tails(const GzItem *items, const gzcut::CutPiece *pieces, const gzcut::CutGroup *groups, uint32_t n_groups, const uint16_t *scratch,
                             unsigned long long *resolved, hipStream_t s);
void launch_gunzip_cut_apply(const GzItem *items, const gzcut::CutPiece *pieces, uint32_t n_pieces, const uint16_t *scratch, unsigned long long *resolved,
                             hipStream_t s);
// list[k]: an item decoded from its first byte to its last by one wave, its members one after the other, trailers and padding checked
void launch_gunzip_single(const GzItem *items, const uint32_t *list, uint32_t n_list, GzSingle *res, hipStream_t s);

// Whole bzip2 files (znippy_bunzip2_batch, bunzip2.hip): BzItem, BzChunk, BzJob, BzRec, BzLand, BzSlice and the layout of a slot are
// in host/bz_plan.h.  `scratch` is n_slots x BZ_SLOT_BYTES; a job or landed block names its slot.
// *count = starts of the block magic found; each as item << 36 | bit in cands[0 .. min(*count, cap)), in no order
void launch_bunzip2_scan(const BzItem *items, const BzChunk *chunks, uint32_t n_chunks, uint32_t *count, uint64_t *cands, uint32_t cap, hipStream_t s);
// recs[j] for every job (all of it but out_len); a block's bytes in front of the inverse BWT into its slot
void launch_bunzip2_decode(const BzItem *items, const BzJob *jobs, uint32_t n_jobs, BzRec *recs, uint8_t *scratch, hipStream_t s);
// for every block job with status 0: the inverse BWT into the slot's out area, the slice table and recs[j].out_len
void launch_bunzip2_walk(const BzJob *jobs, uint32_t n_jobs, BzRec *recs, uint8_t *scratch, uint32_t split, hipStream_t s);
// every landed block's final run-length step into its place; no byte outside [dst + out_off, dst + out_off + out_len) is written
void launch_bunzip2_expand(const BzItem *items, const BzLand *lands, uint32_t n_lands, const uint8_t *scratch, hipStream_t s);
// crc[l] = the bzip2 CRC-32 of the bytes of landed block l
void launch_bunzip2_crc(const BzItem *items, const BzLand *lands, uint32_t n_lands, uint32_t *crc, hipStream_t s);

// The members of tars (znippy_tar_list_batch, tar_list.hip): TlItem, TlChunk, TlNode, TlSum, TlTotal and TlBase are in
// host/tar_list_plan.h.  Every per-node list has an entry for every node of every item.
// nodes[g], jump[g] = nodes[g].succ and mark[g] = (g is node 0 of its item) for every node
void launch_tar_scan(const TlItem *items, const TlChunk *chunks, uint32_t n_chunks, TlNode *nodes, uint8_t *mark, uint32_t *jump, hipStream_t s);
// one round of pointer doubling: a marked node marks jump_in's target; jump_out[g] = jump_in[jump_in[g]]
void launch_tar_chain(const uint32_t *jump_in, uint32_t *jump_out, uint8_t *mark, uint32_t n_nodes, hipStream_t s);
// pred, judge, prefix: pick[g] (bit 31: a listed member; below it its name's length), src[g] (where a pending name starts, or ~0),
// sums[0 .. n_chunks] as prefix sums and totals[k] (the keys have been reset to TL_KEY_NONE) for every item
void launch_tar_emit(const TlItem *items, uint32_t n_items, const TlChunk *chunks, uint32_t n_chunks, const TlNode *nodes, const uint8_t *mark, uint32_t *pred,
                     uint32_t n_nodes, const uint8_t *filter, uint32_t prefix_len, uint32_t suffix_len, uint32_t *pick, uint32_t *src, TlSum *sums,
                     TlTotal *totals, hipStream_t s);
// the records and names of the items with bases[k].take, at the places the bases name; nothing at or behind the caps
void launch_tar_emit_write(const TlItem *items, const TlChunk *chunks, uint32_t n_chunks, const TlNode *nodes, const uint32_t *pick, const uint32_t *src,
                           const TlSum *sums, const TlBase *bases, znippy_tar_member *members, uint64_t members_cap, char *names, uint64_t names_cap,
                           hipStream_t s);

// Whole xz files (znippy_unxz_batch, unxz.hip): XzItem, XzRange, XzJob and XzRec are in host/xz_plan.h.
// the bytes of every range to stage + at
void launch_unxz_tail(const XzItem *items, const XzRange *ranges, uint32_t n_ranges, uint8_t *stage, hipStream_t s);
// recs[j] for every job; a block's content into its place in the item's room, never a byte outside [out_off, out_off + out_len)
void launch_unxz_decode(const XzItem *items, const XzJob *jobs, uint32_t n_jobs, XzRec *recs, hipStream_t s);
// sums[j] = the CRC32 (check id 1) or CRC64 (check id 4) of the bytes of job j's place, 0 for every other check id
void launch_unxz_check(const XzItem *items, const XzJob *jobs, uint32_t n_jobs, uint64_t *sums, hipStream_t s);

}  // namespace zn
