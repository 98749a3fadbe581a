// The listing form of the tar walk of tar_rules.h: every regular member of a tar, in stream order, with its header, its bytes and its
// name — what the reference's tar_entries_from_bytes returns.  The rules are tar_rules.h's (checksum, number fields, which types carry
// data, the V7 directory, prefix/name, 'L' and pax path=, 'g' and 'K' stepped over, two zero blocks end the tar, one is stepped over);
// nothing in that header is changed.  They are cut differently here, so that the device (tar_list.hip) and the host (host/tar_list.cc)
// run the same text:
//   judge_header    what ONE 512-byte block says by itself, without anything in front of it: its kind, its size, and where the next
//                   header stands.  The device judges every block of a tar this way, in parallel, and then lets only the chain from
//                   byte 0 count; a block of member data that happens to look like a header is judged and never reached.
//   ext_pending     what an 'L' / 'x' / 'X' entry hands to the member behind it
//   list_step       the serial walk over the two, for the host
// The whole tar is given (`len` bytes): there is no "more".  A tar ends cleanly at the first of two zero blocks, or where its bytes
// end at a header boundary; in both cases only with no name or size pending.  Everything else a chain can run into is a status for
// the whole tar, and a tar with a status lists no member.
//
// TWO DEVIATIONS from walk_step and from `tarfile`.  (1) A pax size= record in front of a member is accepted only where it equals the
// member's size field.  Where it differs, `tarfile` and walk_step take the record's size and find the next header by it; a block
// judged alone cannot know that, so the tar is TR_UNSUP and nothing of it is listed — never a member at a wrong offset.  Writers emit
// a differing size= only for members of 8 GiB and more, and a tar given here is below 4 GiB.
// (2) A run of more than EXT_RUN_MAX
// extended headers ('L', 'x', 'X', 'g', 'K') with no member or zero block between them, at its first header too many: a member looks
// back over the run in front of it, and the bound keeps that look short whatever the input is (writers emit four in a row at most):
// TR_UNSUP.  As in tar_rules.h, GNU sparse members and 'L' / 'x' payloads above 8 KiB are TR_UNSUP too.
#pragma once
#include "tar_rules.h"

namespace tr {

// what a block is, judged alone
constexpr uint32_t K_ZERO = 0,  // a zero block with a block that is not zero (or the item's end) behind it: stepped over
    K_ZEROS = 1,                // the first of two zero blocks: the tar ends here
    K_END = 2,                  // the item's bytes end at this header boundary
    K_REG = 3,                  // a regular member ('0', '\0' that is no V7 directory, '7')
    K_OTHER = 4,                // any other member: links, directories, devices, unknown types
    K_EXT_L = 5, K_EXT_X = 6,   // a GNU long name; a pax header ('x', 'X') whose records are well formed
    K_SKIP = 7,                 // 'g', 'K': stepped over, and what is pending stays pending
    K_BAD = 8,                  // no header (checksum, size field), a bad pax record, or a step / a payload past the item's end
    K_UNSUP = 9;                // sparse, or a name payload above 8 KiB
constexpr uint32_t EXT_RUN_MAX = 64;
ZN_HD bool kind_is_ext(uint32_t k) { return k == K_EXT_L || k == K_EXT_X || k == K_SKIP; }
ZN_HD bool kind_is_terminal(uint32_t k) { return k == K_ZEROS || k == K_END || k >= K_BAD; }
ZN_HD int kind_status(uint32_t k) { return k == K_BAD ? E_CORRUPT : k == K_UNSUP ? E_UNSUP : 0; }  // of a terminal
// the node behind the last whole block of an item of `len` bytes: a clean end, or a header cut short
ZN_HD uint32_t end_kind(uint64_t len) { return len % BLOCK ? K_BAD : K_END; }

struct Block {
    uint32_t kind, type;  // type: the typeflag, '5' for a V7 directory
    uint64_t size;        // the size field
    uint64_t next;        // where the next header stands (not for a terminal); <= len
};

// The block at h (h + 512 <= len) of a tar of len bytes, which is not zero and whose checksum holds (zero_block, checksum_ok).
// For an 'L' / 'x' / 'X' header the payload, which has to lie inside the tar, is judged with it.
template <class Rd>
ZN_HD void judge_header(const Rd &rd, uint64_t h, uint64_t len, Block &b) {
    b.kind = K_BAD; b.type = 0; b.size = 0; b.next = h;
    const int64_t fsize = number_field(rd, h + 124, 12);
    if (fsize < 0) return;
    const uint64_t size = (uint64_t)fsize;
    uint32_t type = rd.u8(h + 156);
    const uint32_t nl = field_len(rd, h, 100);
    if (type == 0 && nl && rd.u8(h + nl - 1) == '/') type = '5';
    b.type = type; b.size = size;
    if (type == 'S') { b.kind = K_UNSUP; return; }
    uint32_t kind;
    uint64_t next = h + BLOCK + round_block(size);  // (h < 2^32 and size < 2^62: no wrap)
    if (type == 'L' || type == 'x' || type == 'X') {
        if (size > NAME_PAYLOAD_MAX) { b.kind = K_UNSUP; return; }
        if (size > len - (h + BLOCK)) return;  // the payload crosses the item's end
        kind = K_EXT_L;
        if (type != 'L') {
            Walk w;
            walk_init(w);
            const int r = pax_records(rd, h + BLOCK, size, w);
            if (r != TR_STEP) { b.kind = r == TR_UNSUP ? K_UNSUP : K_BAD; return; }
            kind = K_EXT_X;
        }
    } else if (type == 'g' || type == 'K') {
        kind = K_SKIP;
    } else {
        kind = type == '0' || type == 0 || type == '7' ? K_REG : K_OTHER;
        if (type >= '1' && type <= '6') next = h + BLOCK;
    }
    if (next > len) return;  // a step past the item's end: the member, or its padding, is cut short
    b.kind = kind; b.next = next;
}

// the name and the size an 'L' / 'x' entry at h (judged K_EXT_L / K_EXT_X, payload of `size` bytes) hands on: into a fresh Walk
template <class Rd>
ZN_HD void ext_pending(const Rd &rd, uint64_t h, uint32_t kind, uint64_t size, Walk &w) {
    walk_init(w);
    if (kind == K_EXT_L) { w.has_name = 1; w.name_off = h + BLOCK; w.name_len = field_len(rd, h + BLOCK, (uint32_t)size); }
    else if (kind == K_EXT_X) (void)pax_records(rd, h + BLOCK, size, w);
}

// the name of the member whose header stands at h: the pending name, else prefix "/" name, else name
template <class Rd>
ZN_HD NameOf<Rd> member_name(const Rd &rd, uint64_t h, const Walk &pend) {
    const uint32_t nl = field_len(rd, h, 100);
    NameOf<Rd> nm{rd, 0, h, 0, nl, 0};
    if (pend.has_name) { nm.a_off = pend.name_off; nm.a_len = pend.name_len; return nm; }
    const uint32_t pl = field_len(rd, h + 345, 155);
    if (pl) { nm.a_off = h + 345; nm.a_len = pl; nm.joined = 1; }
    else { nm.a_off = h; nm.a_len = nl; }
    return nm;
}

// ---- the serial listing ---------------------------------------------------------------------------------------------------
struct ListWalk {
    uint64_t h;      // where the next header stands
    uint32_t zeros;  // zero blocks in a row
    uint32_t run;    // extended headers in a row
    Walk pend;       // has_name, name_off, name_len, has_size, size_over: what the entries in front of the next member handed on
};
ZN_HD void list_init(ListWalk &lw) { lw.h = 0; lw.zeros = 0; lw.run = 0; walk_init(lw.pend); }

// One step over the tar rd[0, len).  TR_STEP: call again.  TR_FOUND: a regular member — header_off, b (type, size) and `name` are
// its; call again.  TR_NOENT: the tar ended cleanly.  TR_CORRUPT, TR_UNSUP: the status of the whole tar.
template <class Rd>
ZN_HD int list_step(ListWalk &lw, const Rd &rd, uint64_t len, uint64_t *header_off, Block &b, Walk &name) {
    const uint64_t h = lw.h;
    const bool pending = lw.pend.has_name || lw.pend.has_size;
    if (h == len) return pending ? TR_CORRUPT : TR_NOENT;
    if (h > len || len - h < BLOCK) return TR_CORRUPT;
    if (zero_block(rd, h)) {
        if (pending) return TR_CORRUPT;
        if (++lw.zeros == 2) return TR_NOENT;
        lw.run = 0;
        lw.h = h + BLOCK;
        return TR_STEP;
    }
    lw.zeros = 0;
    if (!checksum_ok(rd, h)) return TR_CORRUPT;
    judge_header(rd, h, len, b);
    if (b.kind == K_BAD) return TR_CORRUPT;
    if (b.kind == K_UNSUP) return TR_UNSUP;
    if (kind_is_ext(b.kind) && ++lw.run > EXT_RUN_MAX) return TR_UNSUP;  // deviation (2)
    lw.h = b.next;
    if (b.kind == K_SKIP) return TR_STEP;
    if (kind_is_ext(b.kind)) {  // of several names or sizes in front of one member the first wins
        Walk w;
        ext_pending(rd, h, b.kind, b.size, w);
        if (w.has_name && !lw.pend.has_name) { lw.pend.has_name = 1; lw.pend.name_off = w.name_off; lw.pend.name_len = w.name_len; }
        if (w.has_size && !lw.pend.has_size) { lw.pend.has_size = 1; lw.pend.size_over = w.size_over; }
        return TR_STEP;
    }
    if (lw.pend.has_size && lw.pend.size_over != b.size) return TR_UNSUP;  // deviation (1)
    lw.run = 0;
    name = lw.pend;
    *header_off = h;
    walk_init(lw.pend);
    return b.kind == K_REG ? TR_FOUND : TR_STEP;
}

}  // namespace tr
