// The host side of the block-start search of znippy_gunzip_batch (znippy_ctx_set_gunzip_cut; gunzip.hip: k_gunzip_find): which
// items are searched, the grid of candidate slots, the chunks the search's waves take, and the reading of what the search left.
// Plain C++: no HIP.  Device addresses are only added to, never dereferenced, so a stand-alone program checks all of it under the
// sanitizers (tests/test_gz_cut_plan_cpu.py).
//
// The grid rule.  An item of at least 2 * cut source bytes is searched at every bit position.  Its source is divided into windows
// of cut bytes, counted from the item's byte 0, and every window has one slot: the lowest bit position of the window at which a
// valid non-final dynamic block header starts (gz_cut_rules.h), or NONE.  An item of src_len bytes has ceil(src_len / cut) slots,
// so the list cannot overflow, whatever the input holds.
// The slots come from device memory that searched untrusted input, so nothing here trusts them: a slot that names a position
// outside its own window counts as NONE.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "deflate_batch.h"

namespace gzcut {

constexpr int OK = 0, E_NOMEM = -3;  // ZNIPPY_*
constexpr uint64_t CUT_MIN = 64, CUT_MAX = 1ull << 30;
constexpr uint64_t NONE = ~0ull;
constexpr uint32_t FIND_CHUNK = 4096;  // source bytes one wave of the search takes: 32,768 bit positions
// Limits no real call reaches (a test of them compiles the module with small ones)
#ifndef ZN_GZ_CUT_SLOTS_MAX
#define ZN_GZ_CUT_SLOTS_MAX (1ull << 30)
#endif
constexpr uint64_t SLOTS_MAX = ZN_GZ_CUT_SLOTS_MAX;  // slots, and chunks, of one call

// 0 (off), or CUT_MIN .. CUT_MAX
inline bool cut_valid(uint64_t cut) { return cut == 0 || (cut >= CUT_MIN && cut <= CUT_MAX); }

struct FindItem {  // what the search reads of one searched item
    const uint8_t *src;
    uint32_t src_len, pad;
    uint64_t slot_base;  // its slots are [slot_base, slot_base + ceil(src_len / cut))
};
struct FindChunk { uint32_t item, off; };  // bytes [off, off + FIND_CHUNK) of searched item `item`: one wave

struct FindPlan {
    std::vector<FindItem> items;    // the searched items
    std::vector<uint32_t> item_of;  // searched item -> entry of the batch's item list
    std::vector<FindChunk> chunks;
    uint64_t n_slots = 0;
    uint64_t tested = 0;  // bit positions: 8 * src_len of every searched item
};

// items: the batch's admitted items (GzBatch::items).  OK, or E_NOMEM: more than SLOTS_MAX slots or chunks (nothing is searched).
int find_plan(const zn::GzItem *items, size_t n, uint64_t cut, FindPlan &p);

// slots[0 .. p.n_slots) as the search left them: how many hold a position of their own window
uint64_t count_kept(const FindPlan &p, const uint64_t *slots, uint64_t cut);
// the positions themselves, of searched item f, ascending
void kept_of(const FindPlan &p, size_t f, const uint64_t *slots, uint64_t cut, std::vector<uint64_t> &out);

// ---- cutting at the block starts found ----
// An item the search kept candidates in is a *cut item*.  Its candidates are byte 0, the kept block candidates, and the member and
// kept flush candidates of the scan (gzp::keep_candidates); each gets a wave of the cut probe (gunzip.hip: k_gunzip_cut_probe),
// which leaves a CutRec; plan_cut walks the chain of records from byte 0 as gzp::plan_item does — only candidates the chain lands
// on count, so a false candidate changes no result — member by member, and turns it into pieces.  A member's first piece, and a
// piece that reaches nowhere, is decoded straight into place; a piece that reaches back is decoded into 16-bit symbols in scratch
// (a marker piece: a symbol below 256 is a byte, 0x8000 | k names byte k of the 32,768 in front of the piece's first byte), from
// which two further launches make bytes.  The exception is a piece whose symbols alone exceed the scratch budget: it joins the run
// in front of it, as in gzp::plan_item.  A reach beyond the member's first byte is "too far back".  Consecutive pieces form passes
// whose marker pieces fit the budget.
// Nothing in a record is trusted, and the plan answers only for files that are clean: whatever else it meets — an error, a room too
// small, garbage behind a trailer, a wrong ISIZE, a contradiction — it returns false, and the item takes the stages of the switch
// off, which report what the file is.
constexpr uint32_t END_BOUNDARY = 0, END_TRAILER = 1, END_ERROR = 2, END_ROOM = 3;  // (gzp::END_*)
constexpr int32_t NEXT_MEMBER = 0, NEXT_END = 1;                                      // (gzp::NEXT_*)
constexpr uint32_t WINDOW = 32768;
constexpr uint16_t MARK = 0x8000;

struct CutCand {  // one wave of the cut probe
    uint32_t item;       // entry of the batch's item list
    uint32_t first;      // 1: a member starts here (its header is parsed), 0: a block or flush candidate
    uint64_t bit;        // its bit position in the item's source
    uint32_t stop0, stop1;  // stops[stop0 .. stop1): the item's kept candidates behind it, ascending bit positions
};
struct CutRec {
    uint64_t start_bit;  // of the first block (first: behind the member header)
    uint64_t end_bit;    // END_BOUNDARY: the kept candidate reached; END_TRAILER: the first non-zero byte behind the trailer (or the end)
    uint64_t out;        // bytes the piece produces
    uint32_t end_kind;
    int32_t status;
    uint32_t reach, crc, isize;
    int32_t next;
};
struct CutPiece {  // one wave of the cut decode
    uint32_t item;
    uint32_t marker;     // 1: into scratch as symbols; 0: into place
    uint64_t start_bit;
    uint32_t out_off, out_len;  // relative to the item's room; exact
    uint64_t sym_off;    // marker: its symbols are scratch[sym_off .. sym_off + out_len) (16-bit entries) of its pass
};
struct CutMember {
    uint32_t item;
    uint32_t crc;              // as the trailer has it
    size_t piece0, piece1;     // its pieces, whose lengths add up to its length
};
struct CutItemPlan {
    uint32_t item;
    uint32_t members;
    uint64_t out_len;
    size_t piece0, piece1;     // entries of the piece list
    size_t member0, member1;   // entries of the member list
};
struct CutGroup { uint32_t piece0, piece1; };  // consecutive pieces of one item inside one pass: one workgroup of the tails launch
struct CutPass {
    size_t piece0, piece1;  // entries of the piece list
    size_t group0, group1;  // entries of the group list
};

// cands[0 .. n), recs[0 .. n): the candidates of one item in ascending (bit, first) order, the member at byte 0 first, and their
// records.  Appends the item's pieces, members and plan and returns true, or appends nothing and returns false.  budget_syms:
// 16-bit entries of the scratch.
bool plan_cut(const CutCand *cands, const CutRec *recs, size_t n, uint32_t item, uint64_t src_len, uint64_t room, uint64_t budget_syms,
              std::vector<CutPiece> &pieces, std::vector<CutMember> &members, std::vector<CutItemPlan> &plans);
// the piece list -> passes: consecutive ranges of pieces whose marker pieces' symbols fit budget_syms (every marker piece does:
// plan_cut saw to it), and their groups; sets every marker piece's sym_off inside its pass
void make_passes(std::vector<CutPiece> &pieces, uint64_t budget_syms, std::vector<CutPass> &passes, std::vector<CutGroup> &groups);

}  // namespace gzcut
