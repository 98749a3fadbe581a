// The host planning of znippy_unxz_batch: which items pass, the container walk (xz file format 1.1.0) over the few bytes per block
// that the tail launch brings to the host, the block job list the decode launch reads, and the judgement of the records it leaves.
// Plain C++: no HIP call and no I/O, device addresses are only added to.  Every byte and every record comes from device memory that
// holds untrusted input, so nothing here trusts them: every size is checked against the item before it is used, sums cannot wrap,
// and a contradiction ends in a status (tests/test_xz_plan_cpu.py runs all of it under the sanitizers).
//
// The walk.  An xz file names its blocks' sizes in the index at the END of each stream, so an item is walked from its end, as
// `xz --list` does: stream padding (zero bytes, four at a time), the footer (CRC32, backward size, flags, "YZ"), the index the
// backward size points at (0x00, record count, unpadded / uncompressed size pairs as VLIs, zero padding, CRC32), the stream header
// at index start - sum of the padded block sizes - 12, whose flags must be the footer's; then the stream in front of that.  The walk
// asks for byte ranges (want) and is given them (give); a round serves one range per unfinished item.  The first range is the last
// XZ_TAIL bytes, which hold padding, footer and index of most files; with it the first round brings the item's first 12 bytes,
// where the header of a one-stream file stands, so a batch of one-stream files takes one round.  The ranges of a round do not
// overlap, so a round stages at most the source bytes.  Positions strictly decrease, so it ends.
//
// After the walk every block's source range, output offset, two sizes and check id are known (jobs).  The decode launch leaves a
// record per job, the check launch a CRC per job; xz_verdict folds them into the item's status: the first failure in stream order,
// a differing CRC only on an otherwise clean item.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace zn {

// ---- what the kernels read and write (unxz.hip) ----
constexpr uint32_t XZ_TAIL = 1024;  // bytes of an item's end asked for first
struct XzItem {
    const uint8_t *src;  // the file, any alignment
    uint8_t *dst;        // its room (measure mode: NULL)
    uint32_t src_len, room;
};
// bytes [off, off + len) of the item go to stage[at ..): one wave of the tail launch (head: the item's first 12 bytes, for give_head)
struct XzRange { uint32_t item, off, len, head; uint64_t at; };
struct XzJob {  // a block: one wave of the decode launch, one workgroup of the check launch
    uint32_t item;
    uint32_t src_off;   // of the block header, relative to the item
    uint32_t unpadded;  // header + compressed data + check field, as the index has it; [src_off, src_off + padded) lies inside the item
    uint32_t check;     // the stream's check id, 0..15
    uint32_t out_off, out_len;  // relative to the item's room; the index's uncompressed size; inside the room
};
constexpr uint64_t XZ_ABSENT = ~0ull;
struct XzRec {  // what the decode wave says about its block
    int32_t status;          // 0 or ZNIPPY_E_*
    uint32_t produced;       // bytes written (status 0: out_len)
    uint64_t hdr_comp;       // the block header's compressed size, XZ_ABSENT without one
    uint64_t hdr_uncomp;     // the block header's uncompressed size, likewise
    uint32_t check_lo, check_hi;  // the first eight bytes of the check field, little endian (zero where it is shorter)
    uint32_t hdr_size, comp; // bytes of the header, and of the compressed data the wave derived from the unpadded size
};

constexpr int32_t XZ_OK = 0, XZ_E_INVAL = -1, XZ_E_NOMEM = -3, XZ_E_DST_SMALL = -4, XZ_E_CORRUPT = -5, XZ_E_UNSUPPORTED = -6, XZ_E_CHECKSUM = -7;
constexpr uint64_t XZ_JOBS_MAX = 1ull << 28;

namespace xzp {

uint32_t crc32(const uint8_t *p, size_t n);
// bytes of the check field of check id 0..15
inline uint32_t check_size(uint32_t id) { return id == 0 ? 0u : 4u << ((id - 1) / 3); }
// A VLI at p[*pos .. end): at most 9 bytes, no needless trailing zero byte.  false: malformed or cut off.
bool vli(const uint8_t *p, size_t end, size_t *pos, uint64_t *v);

struct Block { uint64_t unpadded, uncomp; };
struct Stream {
    uint64_t hdr_pos;  // of the stream header
    uint32_t check;
    size_t first, n;   // its blocks in Walk::blocks, in file order
};
// The walk of one item, from its end
struct Walk {
    uint64_t src_len = 0;
    uint64_t end = 0;          // bytes [0, end) are not walked yet
    int stage = 0;             // S_TAIL, S_INDEX, S_HEADER
    uint64_t index_start = 0, index_size = 0;
    uint8_t flags[2] = {0, 0};
    uint64_t want_off = 0, want_len = 0;  // the bytes the next step needs (done: nothing)
    bool want_head = false, have_head = false;  // the first round of an item longer than XZ_TAIL asks for its first 12 bytes as well
    uint8_t head[12] = {0};
    int32_t status = 0;
    bool done = false;
    bool too_big = false;      // content of 4 GiB or more
    uint64_t content = 0;      // sum of the uncompressed sizes (saturates at 2^62)
    std::vector<Stream> streams;  // from the last to the first
    std::vector<Block> blocks;    // stream after stream as found (the last stream's first), each stream's in file order
};
void start(Walk &w, uint64_t src_len);
// the item's first 12 bytes, where want_head asks for them (before the give of the same round)
void give_head(Walk &w, const uint8_t *first12);
// bytes[0 .. want_len) are the item's [want_off, want_off + want_len): walks as far as they reach, then names the next range or ends
void give(Walk &w, const uint8_t *bytes);

}  // namespace xzp

// ---- znippy_unxz_batch ----
struct XzCall {  // a view of the caller's arguments (n > 0; the NULL checks are api.hip's)
    const uint8_t *d_src;
    uint64_t src_cap;
    const uint64_t *src_off, *src_len;
    uint64_t n;
    uint8_t *d_out;  // NULL with out_cap 0: measure mode
    uint64_t out_cap;
    const uint64_t *out_off;   // NULL: packed
    const uint64_t *out_room;  // measure mode: not read
    uint64_t *out_len;
    uint32_t *streams, *blocks, *unverified;  // may be NULL
};
struct XzBatch {
    bool measure = false;
    std::vector<int32_t> st;        // per array item
    std::vector<XzItem> items;      // [k]: the items that passed and have bytes
    std::vector<uint32_t> item_of;  // k -> array item
    std::vector<xzp::Walk> walks;   // [k]
    // a round of the tail stage
    std::vector<XzRange> ranges;
    std::vector<uint8_t> stage;
    // after the walk
    std::vector<XzJob> jobs;        // item after item, in stream order
    std::vector<size_t> first_job;  // [k] .. [k + 1]: item k's
    std::vector<XzRec> recs;        // the decode launch's answer (sized and filled by api.hip)
    std::vector<uint64_t> sums;     // the check launch's answer: CRC32 or CRC64 of the bytes written, per job
};
// Every item by the placement rule of the DEFLATE batch calls (measure mode: the source region and the 4 GiB limit alone); a source
// of no bytes is status 0 with nothing to walk; the caller's out_len, streams, blocks and unverified zeroed.
int xz_admit(const XzCall &c, XzBatch &b);
// The ranges of the next round (two per item at the most) and the bytes they take in the stage; 0 once every walk is done.
uint64_t xz_wants(XzBatch &b);
// b.stage holds the round's ranges: every walk goes on
void xz_give(XzBatch &b);
// The walks to statuses and the job list (measure mode: no jobs; out_len is the index's claim).  XZ_OK or XZ_E_NOMEM.
int xz_plan_jobs(const XzCall &c, XzBatch &b);
// recs and sums to st and the caller's out_len, streams, blocks and unverified: a failed item reports no length and no counts
void xz_verdict(const XzCall &c, XzBatch &b);

}  // namespace zn
