// See gz_cut_plan.h.
#include "gz_cut_plan.h"

#include <algorithm>

namespace gzcut {

int find_plan(const zn::GzItem *items, size_t n, uint64_t cut, FindPlan &p) {
    p = FindPlan{};
    if (!cut_valid(cut) || cut == 0) return OK;
    uint64_t slots = 0, chunks = 0;
    for (size_t k = 0; k < n; k++) {
        const uint64_t len = items[k].src_len;
        if (len < 2 * cut) continue;
        slots += (len + cut - 1) / cut;  // (len below 2^32, at most 2^32 items: no wrap)
        chunks += (len + FIND_CHUNK - 1) / FIND_CHUNK;
    }
    if (slots > SLOTS_MAX || chunks > SLOTS_MAX) return E_NOMEM;
    p.chunks.reserve((size_t)chunks);
    for (size_t k = 0; k < n; k++) {
        const uint64_t len = items[k].src_len;
        if (len < 2 * cut) continue;
        const uint32_t f = (uint32_t)p.items.size();
        p.items.push_back(FindItem{items[k].src, items[k].src_len, 0, p.n_slots});
        p.item_of.push_back((uint32_t)k);
        p.n_slots += (len + cut - 1) / cut;
        p.tested += 8 * len;
        for (uint64_t off = 0; off < len; off += FIND_CHUNK) p.chunks.push_back(FindChunk{f, (uint32_t)off});
    }
    return OK;
}

uint64_t count_kept(const FindPlan &p, const uint64_t *slots, uint64_t cut) {
    uint64_t kept = 0;
    if (!cut) return 0;
    for (const FindItem &it : p.items) {
        const uint64_t n = ((uint64_t)it.src_len + cut - 1) / cut;
        for (uint64_t w = 0; w < n; w++) {
            const uint64_t v = slots[it.slot_base + w];
            if (v == NONE) continue;
            const uint64_t byte = v >> 3;
            if (byte < it.src_len && byte / cut == w) kept++;
        }
    }
    return kept;
}

void kept_of(const FindPlan &p, size_t f, const uint64_t *slots, uint64_t cut, std::vector<uint64_t> &out) {
    out.clear();
    if (!cut || f >= p.items.size()) return;
    const FindItem &it = p.items[f];
    const uint64_t n = ((uint64_t)it.src_len + cut - 1) / cut;
    for (uint64_t w = 0; w < n; w++) {
        const uint64_t v = slots[it.slot_base + w];
        if (v == NONE) continue;
        const uint64_t byte = v >> 3;
        if (byte < it.src_len && byte / cut == w) out.push_back(v);  // (ascending: window w's positions lie below window w + 1's)
    }
}

bool plan_cut(const CutCand *cands, const CutRec *recs, size_t n, uint32_t item, uint64_t src_len, uint64_t room, uint64_t budget_syms,
              std::vector<CutPiece> &pieces, std::vector<CutMember> &members, std::vector<CutItemPlan> &plans) {
    const size_t pieces0 = pieces.size(), members0 = members.size();
    const uint64_t nbits = src_len * 8;  // (src_len below 2^32)
    auto fail = [&] { pieces.resize(pieces0); members.resize(members0); return false; };
    // the candidate of this kind at this position, behind entry `from`
    auto find = [&](size_t from, uint64_t bit, uint32_t first) -> size_t {
        size_t lo = from + 1, hi = n;
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (cands[mid].bit < bit) lo = mid + 1;
            else hi = mid;
        }
        for (; lo < n && cands[lo].bit == bit; lo++)
            if ((cands[lo].first != 0) == (first != 0)) return lo;
        return n;
    };
    if (!n || !cands[0].first || cands[0].bit != 0) return false;
    uint64_t total = 0, member_off = 0;
    size_t at = 0, member_piece0 = pieces0;
    std::vector<uint64_t> lows;  // per piece of this item: the first byte of the room its matches reach
    // every step lands on a candidate with a larger position: at most n steps
    for (size_t steps = 0;; steps++) {
        if (steps >= n) return fail();
        const CutCand &c = cands[at];
        const CutRec &r = recs[at];
        if (c.first) {
            member_off = total;
            member_piece0 = pieces.size();
        }
        if (r.status != 0 || r.end_kind == END_ERROR || r.end_kind >= END_ROOM) return fail();
        if (r.start_bit < c.bit || r.start_bit >= nbits || (!c.first && r.start_bit != c.bit)) return fail();
        if (r.out > room - total) return fail();                 // (total <= room)
        if (r.out > 0xFFFFFFFFull) return fail();
        if (c.first ? r.reach != 0 : (r.reach > total - member_off || r.reach > WINDOW)) return fail();  // too far back, or no distance DEFLATE has
        if (r.reach != 0 && r.out > budget_syms) {
            // its symbols alone exceed the scratch: it joins the run in front of it, and that run its predecessor until a piece
            // decoded into place holds the reach (the member's first piece does)
            uint64_t low = total - r.reach;  // the first byte the run must hold
            while (pieces.back().marker || pieces.back().out_off > low) {
                low = std::min(low, lows.back());
                pieces.pop_back();
                lows.pop_back();
            }
            pieces.back().out_len = (uint32_t)(total + r.out - pieces.back().out_off);  // (below 2^32: inside the room)
        } else {
            pieces.push_back(CutPiece{item, r.reach != 0 ? 1u : 0u, r.start_bit, (uint32_t)total, (uint32_t)r.out, 0});
            lows.push_back(total - r.reach);  // (reach <= total - member_off)
        }
        total += r.out;
        if (r.end_kind == END_BOUNDARY) {
            if (r.end_bit <= r.start_bit || r.end_bit >= nbits) return fail();
            at = find(at, r.end_bit, 0);
            if (at >= n) return fail();
            continue;
        }
        // END_TRAILER: the member must say the size it has; behind it the file ends, or the next member starts where a candidate is
        if (r.isize != (uint32_t)(total - member_off)) return fail();
        members.push_back(CutMember{item, r.crc, member_piece0, pieces.size()});
        if (r.next == NEXT_END) break;
        if (r.next != NEXT_MEMBER || r.end_bit <= r.start_bit || r.end_bit >= nbits) return fail();
        at = find(at, r.end_bit, 1);
        if (at >= n) return fail();
    }
    plans.push_back(CutItemPlan{item, (uint32_t)(members.size() - members0), total, pieces0, pieces.size(), members0, members.size()});
    return true;
}

void make_passes(std::vector<CutPiece> &pieces, uint64_t budget_syms, std::vector<CutPass> &passes, std::vector<CutGroup> &groups) {
    size_t at = 0;
    while (at < pieces.size()) {
        CutPass ps{at, at, groups.size(), groups.size()};
        uint64_t used = 0;
        while (at < pieces.size()) {
            CutPiece &p = pieces[at];
            if (p.marker) {
                if (p.out_len > budget_syms - used) {
                    if (at == ps.piece0) used = 0;  // (cannot happen: plan_cut joins such a piece to the run in front; the caller checks)
                    else break;
                }
                p.sym_off = used;
                used += p.out_len;
            }
            if (groups.size() > ps.group0 && pieces[groups.back().piece1 - 1].item == p.item && groups.back().piece1 == at) groups.back().piece1 = (uint32_t)at + 1;
            else groups.push_back(CutGroup{(uint32_t)at, (uint32_t)at + 1});
            at++;
        }
        ps.piece1 = at;
        ps.group1 = groups.size();
        passes.push_back(ps);
    }
}

}  // namespace gzcut
