// The host planning of the three DEFLATE batch calls — znippy_inflate_batch (raw DEFLATE of ZIP entries), znippy_targz_find_batch
// (one tar member out of gzip-compressed tars) and znippy_gunzip_batch (whole gzip files) — and the lists their kernels read.
// Plain C++, no HIP call and no I/O: device addresses are only added to, never dereferenced, so a stand-alone program checks all of
// it under the sanitizers (tests/test_deflate_batch_cpu.py).  api.hip queues the device work the plan describes, copies the
// kernels' answers into the batch and calls the next stage.  Those answers come from device memory that decoded untrusted input:
// every word of them is checked against what the host itself set up (caps, rooms, list lengths) before it is used as an index or a
// length, and a contradiction ends in a status.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "gz_plan.h"
#include "range_plan.h"

namespace zn {

// ---- what the kernels read and write (inflate.hip, targz.hip, gunzip.hip) ----
// Raw DEFLATE of ZIP entries: one item the host has validated, decoded by one wave.  The CRC launch of znippy_gunzip_batch reads
// the same items (src unused).
struct InflateItem {
    const uint8_t *src;  // the compressed bytes, any alignment
    uint8_t *dst;
    uint32_t src_len, out_len;  // both below 4 GiB
    uint32_t method;            // 8: DEFLATE; 0: a copy (src_len == out_len)
    uint32_t want_crc, has_crc;
    uint32_t pad;
};
// One tar member out of gzip-compressed tars: one item the host has validated, decoded by one wave only as far as the tar has to
// be read
struct TargzItem {
    const uint8_t *src;  // the gzip member, any alignment
    uint8_t *scratch;    // where the tar is inflated to: 16-byte aligned, cap rounded up to 16 bytes long
    uint32_t src_len;    // below 4 GiB
    uint32_t cap;        // inflated bytes the item may take: 512 .. 4 GiB - 16
    uint32_t whole;      // src is the whole file: input that ends inside the stream is damage, not "more"
    uint32_t pad;
};
struct TargzResult {
    int32_t status;    // 0 or ZNIPPY_E_*
    uint32_t pad;
    uint64_t off, len;  // status 0: the member is scratch[off .. off + len)
    uint64_t scanned;   // bytes inflated
};
// Whole gzip files: one item the host has validated
struct GzItem {
    const uint8_t *src;  // the file, any alignment
    uint8_t *dst;        // its room
    uint32_t src_len, room;  // both below 4 GiB
    uint32_t cand_base, cand_cap;  // its slice of the scan's candidate list
};
constexpr uint32_t GZ_SCAN_CHUNK = 4096;
struct GzScanChunk { uint32_t item, off; };  // bytes [off, off + GZ_SCAN_CHUNK) of the item: one wave of the scan
struct GzCand {  // one kept candidate: one wave of the probe
    uint32_t item, pos, kind;
    uint32_t stop0, stop1;  // stops[stop0 .. stop1): the kept flush candidates of its item behind pos, ascending
    uint32_t pad;
};
struct GzProbe {  // gzp::Probe without the candidate
    uint32_t data_start, end_kind, end_pos;
    int32_t status;
    uint64_t out;
    uint32_t reach, crc, isize;
    int32_t next;
};
struct GzRun {  // one wave of the decode launch
    uint32_t item, src_start;  // the first DEFLATE byte, relative to the item's source
    uint32_t out_off, out_len; // relative to the item's room; out_len > 0, and exact
};
struct GzSingle {  // what the single pass says about an item
    int32_t status;       // ZNIPPY_E_CHECKSUM here: an ISIZE, or the CRC-32 of a member behind the first
    uint32_t out_len, members;
    uint32_t crc0, len0;  // the first member's CRC-32 as its trailer has it, and its length: left to the CRC launch
    uint32_t pad;
};

// ---- constants ----
// the status codes the plan gives out: the ZNIPPY_E_* of include/znippy_hip.h (api.hip asserts that they are)
constexpr int32_t DB_OK = 0, DB_E_INVAL = -1, DB_E_NOMEM = -3, DB_E_DST_SMALL = -4, DB_E_CORRUPT = -5, DB_E_UNSUPPORTED = -6, DB_E_CHECKSUM = -7;
// Limits no real call reaches (a test of them compiles the module with small ones)
#ifndef ZN_GZ_LIST_MAX
#define ZN_GZ_LIST_MAX (1ull << 30)
#endif
#ifndef ZN_GZ_CHUNKS_MAX
#define ZN_GZ_CHUNKS_MAX (1ull << 30)
#endif
#ifndef ZN_TARGZ_NEED_MAX
#define ZN_TARGZ_NEED_MAX (1ull << 40)
#endif
constexpr uint64_t GZ_LIST_MAX = ZN_GZ_LIST_MAX;  // entries of the raw candidate list
// Chunks of the scan, an item counted as src_len / GZ_SCAN_CHUNK + 1 of them (one more than it has where its length is a multiple of the
// chunk).  With both limits at one value this one never speaks first: an item adds 16 + src_len / 256 candidates and at most
// src_len / 4096 + 1 chunks, so the candidate total passes the value before the chunk count can.  It guards the 32-bit chunk count of
// the launch should the two values ever differ, and has an override of its own so that a test can reach it.
constexpr uint64_t GZ_CHUNKS_MAX = ZN_GZ_CHUNKS_MAX;
constexpr uint64_t TARGZ_NEED_MAX = ZN_TARGZ_NEED_MAX;  // bytes of scratch one call may ask for (far beyond the scratch's own cap)

// ---- the placement rule znippy_inflate_batch and znippy_gunzip_batch share ----
// Items are placed in array order; with no offsets given they lie back to back, each taking out_len bytes whether it is admitted or
// not.  Once the running sum has wrapped, the offsets behind it are unknown.
struct Placement {
    uint64_t packed = 0;
    bool wrapped = false;
};
// One item against the source region [0, src_cap), the output region [0, out_cap) and the 4 GiB limit of both lengths: DB_E_INVAL,
// DB_E_DST_SMALL or DB_E_UNSUPPORTED, in this order, or DB_OK and its offset in the output region.  out_off: the item's offset, or
// NULL (packed).  Advances the placement either way.
int32_t place_item(Placement &p, uint64_t src_off, uint64_t src_len, uint64_t src_cap, const uint64_t *out_off, uint64_t out_len, uint64_t out_cap,
                   uint64_t *dst);

// ---- znippy_inflate_batch ----
struct InflateCall {  // a view of the caller's arguments (n > 0; the NULL checks are api.hip's)
    const uint8_t *d_src;
    uint64_t src_cap;
    const uint64_t *src_off, *src_len;
    const uint8_t *method;  // NULL: all DEFLATE
    uint8_t *d_out;
    uint64_t out_cap;
    const uint64_t *out_off;  // NULL: packed
    const uint64_t *out_len;
    const uint32_t *crc32;  // NULL: nothing to compare with
    uint64_t n;
};
struct InflateBatch {
    std::vector<int32_t> st;         // per array item
    std::vector<InflateItem> items;  // the list: the items that passed
    std::vector<uint32_t> item_of;   // list entry -> array item
    std::vector<int32_t> h_st;       // per list entry: what the kernels say (sized by inflate_admit, filled by api.hip)
    std::vector<uint32_t> h_crc;
};
// Every item by the placement rule, then its method (DB_E_UNSUPPORTED) and, stored, src_len != out_len (DB_E_CORRUPT)
void inflate_admit(const InflateCall &c, InflateBatch &b);
// h_st and h_crc, in list order, into the caller's arrays (either may be NULL), in array order; crc_out is 0 where nothing was decoded
void inflate_scatter(const InflateBatch &b, uint64_t n, int32_t *status, uint32_t *crc_out);

// ---- znippy_targz_find_batch ----
struct TargzCall {
    const uint8_t *d_src;
    uint64_t src_cap;
    const uint64_t *src_off, *src_len;
    const uint8_t *whole;  // NULL: every item is a whole file
    uint64_t n, scan_cap;  // scan_cap >= 512
    uint8_t *d_out;
    uint64_t out_cap;
    uint64_t *out_off, *out_len;
    uint64_t *scanned;  // may be NULL
};
struct TargzBatch {
    std::vector<int32_t> st;
    std::vector<TargzItem> items;
    std::vector<uint64_t> slice;    // list entry -> offset of its slice of the scratch
    std::vector<uint32_t> item_of;  // list entry -> array item
    uint64_t need = 0;              // bytes of scratch
    std::vector<TargzResult> res;   // per list entry: what the kernel says (sized by targz_admit, filled by api.hip)
    std::vector<RangePiece> pieces; // the gather's list
};
// Every item against the source region; cap = min(scan_cap, 1032 * src_len + 512, 4 GiB - 16) and a slice of that, rounded up to 16
// bytes, for each that passes; the caller's out_off, out_len and scanned zeroed.  DB_OK or DB_E_NOMEM (need above TARGZ_NEED_MAX).
int targz_admit(const TargzCall &c, TargzBatch &b);
// Pieces the gather can need: one per RANGE_PIECE bytes of output and two more per item.  DB_OK or DB_E_NOMEM (above RR_ITEMS_MAX).
int targz_piece_bound(uint64_t out_cap, size_t n_items, size_t *max_pieces);
void targz_bind(TargzBatch &b, uint8_t *scratch);  // slice offsets to scratch pointers
// res into st, out_off, out_len, scanned and pieces: the members found, back to back in array order.  A result whose off and len
// do not lie inside the item's cap is DB_E_CORRUPT; a member that no longer fits is DB_E_DST_SMALL; neither takes room, and those
// behind it may still fit.
void targz_pack(const TargzCall &c, TargzBatch &b);

// ---- znippy_gunzip_batch ----
struct GzCall {
    const uint8_t *d_src;
    uint64_t src_cap;
    const uint64_t *src_off, *src_len;
    uint64_t n;
    uint8_t *d_out;
    uint64_t out_cap;
    const uint64_t *out_off;  // NULL: packed
    const uint64_t *out_room;
    uint64_t seg_min;  // > 0
    uint64_t *out_len;
    uint32_t *members, *segments;  // may be NULL
};
// Index spaces: i an array item, k an entry of `items`, j an entry of `probed`, e an entry of `single`, c an entry of `cands`.
struct GzBatch {
    // gz_admit
    std::vector<int32_t> st;          // [i]
    std::vector<GzItem> items;        // [k]
    std::vector<uint32_t> item_of;    // k -> i
    std::vector<GzScanChunk> chunks;
    uint64_t cand_total = 0;          // entries of the raw candidate list
    // the scan's answer (sized by gz_admit / to gz_raw_end, filled by api.hip)
    std::vector<uint32_t> count;      // [k]
    std::vector<uint64_t> raw;
    // the cut at block starts (znippy_ctx_set_gunzip_cut; filled by api.hip, empty with the switch off): [k] != 0: the item is
    // decoded and checked already, and gz_candidates gives it neither a probe nor the single pass
    std::vector<uint8_t> cut_done;
    // gz_candidates
    std::vector<GzCand> cands;        // [c]
    std::vector<uint32_t> stops;      // kept flush positions, per probed item ascending
    std::vector<uint32_t> single;     // e -> k
    std::vector<uint32_t> probed;     // j -> k, in the order of their records
    std::vector<size_t> first_cand;   // [j], and one more: probed[j]'s entries of cands are [first_cand[j], first_cand[j + 1])
    // the probe's and the single pass's answers (sized by gz_candidates, filled by api.hip)
    std::vector<GzProbe> recs;        // [c]
    std::vector<GzSingle> sres;       // [e]
    // gz_decode_plan
    std::vector<int32_t> item_st;     // [k]
    std::vector<InflateItem> crc_items;  // the CRC launch: first members of single items, then non-empty runs
    std::vector<uint32_t> crc_item_of;   // its first entries (those that carry the CRC to compare with) -> k
    std::vector<gzp::Run> runs;
    std::vector<gzp::Member> mems;
    std::vector<gzp::ItemPlan> plans;    // [j]
    std::vector<gzp::Probe> scratch;     // (one item's records, reused)
    std::vector<GzRun> h_runs;           // the decode launch: the non-empty runs
    std::vector<uint32_t> run_item;      // entry of h_runs -> k
    std::vector<size_t> crc_of_run;      // entry of runs -> its entry of crc_items (non-empty runs)
    // the decode and CRC launches' answers (sized by gz_decode_plan, filled by api.hip)
    std::vector<int32_t> run_st, crc_st;
    std::vector<uint32_t> crc_got;
};
struct GzLayout {  // the one device allocation: offsets of its lists, each 16-byte aligned, and its size
    size_t items, chunks, count, raw, cands, stops, recs, runs, run_st, crc_items, crc_st, crc_got, single_list, single_res;
    size_t bytes;
};
// Every item by the placement rule; a source of no bytes is status 0 with no list entry (it still takes its room); a slice of
// 16 + src_len / 256 entries of the candidate list and a chunk per GZ_SCAN_CHUNK bytes for each that passes; the caller's out_len,
// members and segments zeroed.  DB_OK or DB_E_NOMEM (the candidate list above GZ_LIST_MAX, the chunks above GZ_CHUNKS_MAX).
int gz_admit(const GzCall &c, GzBatch &b);
// A kept candidate list is never longer than the raw one plus byte 0 of every item; a run per record and a CRC entry per record
// or item at most.
inline size_t gz_kept_max(const GzBatch &b) { return (size_t)b.cand_total + b.items.size(); }
GzLayout gz_layout(const GzBatch &b);
// How far the raw list is copied back: to the end of the last item that has candidates and room for them
uint64_t gz_raw_end(const GzBatch &b);
// count and raw[0 .. gz_raw_end) to the probe's lists: items with a kept candidate behind byte 0 are probed (the entry for byte 0
// first, then the kept ones in position order, each with the stops strictly behind it); items without one, and items whose count
// passed their slice, take the single pass.  DB_OK or DB_E_NOMEM.  That return cannot happen, whatever the device wrote: an item keeps at most count <= cand_cap
// candidates and one entry for byte 0, which is what gz_kept_max and cand_total count; so no test reaches it, here or in gz_decode_plan.
int gz_candidates(GzBatch &b, uint64_t seg_min);
// sres and recs to item_st, the decode launch's runs and the CRC launch's items.  DB_OK or DB_E_NOMEM (cannot happen, as
// above: plan_item gives a run per record at the most, and a single item one CRC entry).
int gz_decode_plan(GzBatch &b);
// run_st, crc_st and crc_got to st and the caller's out_len, members and segments.  A run that failed is DB_E_CORRUPT; a CRC that
// differs is DB_E_CHECKSUM where nothing else is wrong; a failed item reports no length and no counts.
void gz_verdict(const GzCall &c, GzBatch &b);

}  // namespace zn
