// The host planning of znippy_gunzip_batch: which flush candidates of an item are kept, and the pure function from the records the
// probe launch leaves (one per kept candidate: where its decoding ended, how many bytes it would produce, how far its matches reach
// in front of its own first byte) to the plan of the decode launch: runs, members, the item's status and counts.
// Plain C++: no HIP.  The records come from device memory that decoded untrusted input, so nothing here trusts them: every record is
// checked against the item (source length, room) and against the chain before it is used, and contradictions end in a status.
//
// The chain rule.  An item is walked from byte 0, which is a member candidate.  A record says where its piece ended: at a block
// boundary that is a kept flush candidate (the chain goes on with that candidate's record), at its member's trailer (the chain goes on
// with the member candidate behind the zero padding, or ends), or in an error.  Only records the chain lands on count.  A candidate
// that the pattern search found inside compressed or stored data is never landed on: the decoder of the piece in front of it stops
// at block boundaries only, and a position that is a block boundary of the true chain is a true boundary, whatever the bytes in front
// of it look like.
// A piece whose matches reach in front of its first byte cannot be decoded alone: it joins the run in front of it (and that run the
// one before, while the reach is longer than the run).  Its byte count and end are valid all the same, since symbol decoding does
// not depend on the window.  A reach beyond the member's first byte is what zlib calls "invalid distance too far back".
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace gzp {

constexpr int OK = 0, E_DST_SMALL = -4, E_CORRUPT = -5, E_UNSUPPORTED = -6, E_CHECKSUM = -7;  // ZNIPPY_*

constexpr uint32_t K_FLUSH = 0, K_MEMBER = 1;                                   // candidate kinds
constexpr uint32_t END_BOUNDARY = 0, END_TRAILER = 1, END_ERROR = 2, END_ROOM = 3;  // how a probe ended
constexpr int32_t NEXT_MEMBER = 0, NEXT_END = 1;  // behind a trailer and its zero padding: a member header, or the end of the item
                                                  // (negative: what the bytes there are instead, as a status)
constexpr uint64_t SEG_MIN_DEFAULT = 256;  // (profiles/gunzip_report.log: the best of the values swept)

struct Probe {
    uint32_t pos, kind;    // the candidate
    uint32_t data_start;   // its first DEFLATE byte (behind the header of a member candidate)
    uint32_t end_kind;
    uint32_t end_pos;      // END_BOUNDARY: the flush candidate reached; END_TRAILER: the first non-zero byte behind the trailer (or src_len)
    int32_t status;        // END_ERROR: the negative status
    uint64_t out;          // bytes the piece produces (END_ERROR, END_ROOM: up to where it stopped)
    uint32_t reach;        // the longest reach of a match in front of the piece's first byte (K_FLUSH only)
    uint32_t crc, isize;   // END_TRAILER
    int32_t next;          // END_TRAILER
};

struct Run {      // one wave of the decode launch
    uint32_t item;
    uint32_t src_start;         // the first DEFLATE byte, relative to the item's source
    uint64_t out_off, out_len;  // relative to the item's room; the exact count
};
struct Member {
    uint32_t item;
    uint32_t crc;               // as the trailer has it
    uint64_t out_off, out_len;
    size_t run0, run1;          // its runs, whose lengths add up to out_len: entries [run0, run1) of the run list
};
struct ItemPlan {
    int32_t status;    // 0, or the first failure in stream order; E_CHECKSUM (an ISIZE mismatch) only if everything else is clean
    uint32_t members, segments;
    uint64_t out_len;  // status 0 or E_CHECKSUM: the bytes of all members
};

// cands: the raw candidates of one item as (pos << 1 | kind), in any order.  Sorted in place; returns how many stay, at the front:
// every member candidate, and every flush candidate at least seg_min bytes behind the previous kept candidate (byte 0 is one).
size_t keep_candidates(uint64_t *cands, size_t n, uint64_t seg_min);

// recs: the records of one item, sorted by (pos, kind), the first one the member candidate at byte 0.  Appends the item's runs and
// members (none unless the status is 0 or E_CHECKSUM) and fills *plan.
void plan_item(const Probe *recs, size_t n, uint32_t item, uint64_t src_len, uint64_t room, std::vector<Run> &runs, std::vector<Member> &members,
               ItemPlan *plan);

// CRC-32 of A || B from the CRC-32s of A and of B and the length of B (zlib's crc32_combine): crc(A) * x^(8 |B|) mod P xor crc(B)
uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

}  // namespace gzp
