// The host planning of znippy_bunzip2_batch: which items pass, the lists the kernels of bunzip2.hip read, and the pure function from
// the records the decode and walk launches leave (one per decoded candidate) to what lands where, pass by pass.
// Plain C++: no HIP call and no I/O, device addresses are only added to.  The records come from device memory that decoded untrusted
// input, so nothing here trusts them: every record is checked against the item (source length, level, room) and against the chain
// before it is used, and a contradiction ends in a status (tests/test_bz_plan_cpu.py runs all of it under the sanitizers).
//
// The chain rule.  An item is walked from byte 0, where a stream header has to stand.  The record of a stream header says which
// magic follows its four bytes; the record of a block says at which bit the block ended and which magic stands there.  A block magic
// leads to the candidate at exactly that bit, an end magic (with the stream's combined CRC and the zero padding to a byte behind it)
// to a stream header where the rest starts with "BZh", else to the end of the item.  Only records the chain lands on count: a
// candidate the scan found inside block data, or inside ignored trailing bytes, is either passed by the chain and dropped undecoded,
// or was decoded ahead of the chain and its record is never read.  Positions along the chain strictly increase, so it ends.
//
// Passes.  A pass decodes up to slot_cap blocks: items in array order, each with the job the chain waits for first and then its
// candidates behind it in position order (a stream header takes no slot and is always read).  After a pass the chain of every item advances over the records it can reach; what it
// landed on is expanded and checksummed before the next pass reuses the slots.  The first unfinished item always gets the job its
// chain waits for, so every pass advances it: no result depends on slot_cap, only the number of passes does.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace zn {

// ---- what the kernels read and write (bunzip2.hip) ----
constexpr uint32_t BZ_BLOCK_MAX = 900000;  // bytes of a level-9 block in front of the final run-length step
constexpr uint32_t BZ_SCAN_CHUNK = 4096;
constexpr uint32_t BZ_SLICES = 256;        // slices of a block in the expand launch (one per thread)
constexpr uint32_t BZ_SPLIT_MIN = 16;      // (the splitter lists of the largest block fit the slot's byte area from this spacing on)
constexpr uint32_t BZ_SPLIT_DEFAULT = 256;  // (profiles/bunzip2_report.log: the best of the spacings swept)
// A slot, the scratch of one decoded block, sized for level 9 whatever the stream's level is (the level of a candidate ahead of
// the chain is not known when it is decoded): bytes[BZ_BLOCK_MAX] the block in front of the inverse BWT, later the splitter lists;
// tt[BZ_BLOCK_MAX] the successor array (successor << 8 | byte), later the slice table of the expand launch; out[BZ_BLOCK_MAX] the
// block behind the inverse BWT.  6 x 900,000 bytes.
constexpr size_t BZ_SLOT_BYTES_OFF = 0, BZ_SLOT_TT_OFF = BZ_BLOCK_MAX, BZ_SLOT_OUT_OFF = 5ull * BZ_BLOCK_MAX;
constexpr size_t BZ_SLOT_BYTES = 6ull * BZ_BLOCK_MAX;
constexpr uint64_t BZ_SCRATCH_DEFAULT = 1ull << 30;

struct BzItem {
    const uint8_t *src;  // the file, any alignment
    uint8_t *dst;        // its room (measure mode: NULL)
    uint32_t src_len, room;
};
struct BzChunk { uint32_t item, off; };  // bytes [off, off + BZ_SCAN_CHUNK) of the item: one wave of the scan
struct BzJob {  // one wave of the decode launch, one workgroup of the walk launch
    uint32_t item, kind;  // bzp::K_HEAD: a stream header at byte `pos`; bzp::K_BLOCK: a block whose magic starts at bit `pos`
    uint64_t pos;
    uint32_t slot, pad;
};
struct BzRec {  // what decode and walk say about a job
    int32_t status;       // 0 or ZNIPPY_E_*
    uint32_t next;        // status 0: bzp::NEXT_BLOCK or bzp::NEXT_END, the magic behind the header or block
    uint64_t end_bit;     // K_BLOCK: where that magic starts
    uint64_t after;       // NEXT_END: the first byte behind the combined CRC and the padding
    uint32_t n;           // K_BLOCK: bytes in front of the final run-length step
    uint32_t level;       // K_HEAD: 1..9
    uint32_t block_crc;   // K_BLOCK: as the block header has it
    uint32_t stream_crc;  // NEXT_END: as the trailer has it
    uint32_t tail;        // NEXT_END: up to three bytes at `after`, little endian
    uint32_t tail_len;    //           and how many of them exist
    uint32_t out_len;     // K_BLOCK: bytes behind the final run-length step (the walk launch)
    uint32_t orig;        // K_BLOCK: origPtr
};
struct BzLand {  // a block the chain landed on: one workgroup of the expand and CRC launches
    uint32_t item, slot;
    uint32_t out_off, out_len;  // relative to the item's room; exact
    uint32_t n;
    uint32_t crc;  // as the block header has it
};
struct BzSlice { uint32_t off, state; };  // where a slice's bytes go, relative to the block, and the run state in front of it (run | last << 8)

// the status codes the plan gives out: the ZNIPPY_E_* of include/znippy_hip.h (api.hip asserts that they are)
constexpr int32_t BZ_OK = 0, BZ_E_INVAL = -1, BZ_E_NOMEM = -3, BZ_E_DST_SMALL = -4, BZ_E_CORRUPT = -5, BZ_E_UNSUPPORTED = -6, BZ_E_CHECKSUM = -7;
#ifndef ZN_BZ_LIST_MAX
#define ZN_BZ_LIST_MAX (1ull << 30)
#endif
constexpr uint64_t BZ_LIST_MAX = ZN_BZ_LIST_MAX;  // entries of the candidate list, and chunks of the scan
constexpr uint64_t BZ_ITEMS_MAX = 1ull << 28;     // (a candidate is item << 36 | bit)

namespace bzp {

constexpr uint32_t K_HEAD = 0, K_BLOCK = 1;
constexpr uint32_t NEXT_BLOCK = 0, NEXT_END = 1;

// The chain of one item
struct Chain {
    uint32_t src_len = 0;
    uint64_t room = 0;
    bool measure = false;
    const uint64_t *cands = nullptr;  // the bit positions the scan found, ascending
    size_t n_cands = 0, cur = 0;      // cur: the first candidate the chain has not passed
    uint32_t kind = K_HEAD;           // what the chain waits for
    uint64_t pos = 0;
    uint32_t level = 0;
    uint64_t out = 0;                 // bytes landed so far
    uint32_t comb = 0;                // the combined CRC of the stream so far, from the block headers
    uint32_t streams = 0, blocks = 0;
    int32_t status = 0;               // the first failure in stream order
    bool sum_bad = false;             // a CRC that differs: E_CHECKSUM if nothing else is wrong
    bool done = false;
};

// The jobs of the next pass: at most slot_cap (> 0) block jobs, each in a slot of its own (0, 1, ...), and at most one header job
// per item, which needs no slot (its slot field is 0); first_job[k] .. first_job[k + 1] are item k's.  An item whose chain waits for
// a block that is no candidate fails here (E_CORRUPT).  Returns the number of jobs: 0 once every item is done.
size_t choose(std::vector<Chain> &items, size_t slot_cap, std::vector<BzJob> &jobs, std::vector<size_t> &first_job);
// Every chain over the records of the pass (recs[j] is jobs[j]'s); the blocks landed on are appended to `lands`.
void advance(std::vector<Chain> &items, const std::vector<BzJob> &jobs, const std::vector<size_t> &first_job, const BzRec *recs, std::vector<BzLand> &lands);
// The CRC launch's answers (got[l] is lands[l]'s) against the block headers
void fold_crc(std::vector<Chain> &items, const std::vector<BzLand> &lands, const uint32_t *got);
inline int32_t verdict(const Chain &c) { return c.status ? c.status : c.sum_bad ? BZ_E_CHECKSUM : BZ_OK; }

}  // namespace bzp

// ---- znippy_bunzip2_batch ----
struct BzCall {  // a view of the caller's arguments (n > 0; the NULL checks are api.hip's)
    const uint8_t *d_src;
    uint64_t src_cap;
    const uint64_t *src_off, *src_len;
    uint64_t n;
    uint8_t *d_out;  // NULL with out_cap 0: measure mode
    uint64_t out_cap;
    const uint64_t *out_off;   // NULL: packed
    const uint64_t *out_room;  // measure mode: not read
    uint64_t *out_len;
    uint32_t *streams, *blocks;  // may be NULL
};
struct BzBatch {
    bool measure = false;
    std::vector<int32_t> st;         // per array item
    std::vector<BzItem> items;       // [k]: the items that passed and have bytes
    std::vector<uint32_t> item_of;   // k -> array item
    std::vector<BzChunk> chunks;
    // The candidate list.  The block magic overlaps itself only at a shift of 45 bits (its last three bits 001 are its first three),
    // so an item of src_len bytes holds at most 8 * src_len / 45 + 1 starts of it; cand_total is the sum of that over the items,
    // the list is that long, and the scan has no overflow path.
    uint64_t cand_total = 0;
    std::vector<uint64_t> raw;       // the scan's answer: item << 36 | bit, in any order (sized and filled by api.hip)
    std::vector<bzp::Chain> chains;  // [k]
    std::vector<uint64_t> cands;     // every item's bit positions, ascending, item after item
    // a pass
    std::vector<BzJob> jobs;
    std::vector<size_t> first_job;
    std::vector<BzRec> recs;
    std::vector<BzLand> lands;
    std::vector<uint32_t> got_crc;
};
// Every item by the placement rule of the DEFLATE batch calls (measure mode: the source region and the 4 GiB limit alone); a source
// of no bytes is status 0 with no list entry; a chunk per BZ_SCAN_CHUNK bytes for each that passes; the caller's out_len, streams and
// blocks zeroed.  BZ_OK or BZ_E_NOMEM (the candidate list or the chunks above BZ_LIST_MAX, the items above BZ_ITEMS_MAX).
int bz_admit(const BzCall &c, BzBatch &b);
// Slots of the call: slot_cap, or with 0 what fits the budget, and never more than the candidates there can be.  0: not one slot
// fits.  A pass has at most that many jobs and one more per item.
inline size_t bz_jobs_max(const BzBatch &b, size_t n_slots) { return n_slots + b.items.size(); }
size_t bz_slots(const BzBatch &b, uint64_t slot_cap, uint64_t budget);
// raw[0 .. n_raw) to the chains: entries that name no item or no bit position of theirs are dropped
void bz_start(BzBatch &b, size_t n_raw);
// the chains to st and the caller's out_len, streams and blocks: a failed item reports no length and no counts
void bz_verdict(const BzCall &c, BzBatch &b);

}  // namespace zn
