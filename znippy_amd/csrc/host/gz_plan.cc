// See gz_plan.h.
#include "gz_plan.h"

#include <algorithm>

namespace gzp {

size_t keep_candidates(uint64_t *cands, size_t n, uint64_t seg_min) {
    std::sort(cands, cands + n);
    size_t kept = 0;
    uint64_t last = 0;  // byte 0
    for (size_t i = 0; i < n; i++) {
        const uint64_t pos = cands[i] >> 1;
        if ((cands[i] & 1) == K_FLUSH && pos - last < seg_min) continue;
        if (kept && cands[kept - 1] == cands[i]) continue;
        cands[kept++] = cands[i];
        last = pos;
    }
    return kept;
}

namespace {

const Probe *find(const Probe *recs, size_t n, uint64_t pos, uint32_t kind) {
    const uint64_t key = pos << 1 | kind;
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (((uint64_t)recs[mid].pos << 1 | recs[mid].kind) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && recs[lo].pos == pos && recs[lo].kind == kind ? recs + lo : nullptr;
}

uint32_t mulmod(uint32_t a, uint32_t b) {  // a * b mod P on the reflected polynomial
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = b & 1 ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}

}  // namespace

uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    uint32_t r = 0x80000000u, q = 0x40000000u;  // x^0, x^1; r becomes x^(8 len_b)
    for (uint64_t n = len_b; n; n >>= 1) {      // (len_b below 2^61)
        if (n & 1) r = mulmod(r, q);
        q = mulmod(q, q);
    }
    for (int k = 0; k < 3; k++) r = mulmod(r, r);
    return mulmod(r, crc_a) ^ crc_b;
}

void plan_item(const Probe *recs, size_t n, uint32_t item, uint64_t src_len, uint64_t room, std::vector<Run> &runs, std::vector<Member> &members,
               ItemPlan *plan) {
    const size_t runs0 = runs.size(), members0 = members.size();
    ItemPlan p{OK, 0, 0, 0};
    int status = OK;
    bool size_bad = false;
    uint64_t total = 0;         // bytes of the item so far
    uint64_t member_off = 0;    // where the current member's bytes start
    size_t member_run0 = runs0; // the current member's first run
    const Probe *r = find(recs, n, 0, K_MEMBER);
    if (!r) status = E_CORRUPT;
    // every step lands on a record with a larger position: at most n steps
    for (size_t steps = 0; r && status == OK; steps++) {
        if (steps > n || r->data_start < r->pos || r->data_start > src_len || r->pos >= src_len) { status = E_CORRUPT; break; }
        if (r->kind == K_MEMBER) {
            p.members++;
            member_off = total;
            member_run0 = runs.size();
        }
        if (r->out > room - total) { status = E_DST_SMALL; break; }  // (total <= room)  the overflow lies in front of whatever ended the piece
        if (r->end_kind == END_ERROR) { status = r->status < 0 ? r->status : E_CORRUPT; break; }
        if (r->end_kind == END_ROOM || r->end_kind > END_ROOM) { status = E_CORRUPT; break; }  // (a probe that saw the room exceeded, and a count that fits)
        const uint64_t in_member = total - member_off;
        if (r->kind == K_MEMBER ? r->reach != 0 : r->reach > in_member) { status = E_CORRUPT; break; }
        if (r->kind == K_MEMBER || r->reach == 0) {
            runs.push_back(Run{item, r->data_start, total, r->out});
        } else {
            // joins the run in front of it; that run joins its predecessor while the reach is longer than what the run holds
            while (runs.size() - member_run0 > 1 && r->reach > total - runs.back().out_off) {
                const Run last = runs.back();
                runs.pop_back();
                runs.back().out_len += last.out_len;
            }
            runs.back().out_len += r->out;  // (the member has a run: a flush record is landed on from a piece of the same member)
        }
        total += r->out;
        if (r->end_kind == END_BOUNDARY) {
            if (r->end_pos <= r->pos || r->end_pos >= src_len) { status = E_CORRUPT; break; }
            r = find(recs, n, r->end_pos, K_FLUSH);
            if (!r) status = E_CORRUPT;
            continue;
        }
        // END_TRAILER
        if (r->isize != (uint32_t)(total - member_off)) size_bad = true;
        members.push_back(Member{item, r->crc, member_off, total - member_off, member_run0, runs.size()});
        if (r->next == NEXT_END) break;
        if (r->next != NEXT_MEMBER) { status = r->next < 0 ? r->next : E_CORRUPT; break; }
        if (r->end_pos <= r->pos || r->end_pos >= src_len) { status = E_CORRUPT; break; }
        r = find(recs, n, r->end_pos, K_MEMBER);
        if (!r) status = E_CORRUPT;
    }
    if (status == OK && size_bad) status = E_CHECKSUM;
    if (status != OK && status != E_CHECKSUM) {
        runs.resize(runs0);
        members.resize(members0);
        p.members = 0;
    } else {
        p.segments = (uint32_t)(runs.size() - runs0);
        p.out_len = total;
    }
    p.status = status;
    *plan = p;
}

}  // namespace gzp
