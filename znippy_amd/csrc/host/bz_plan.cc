// The host planning of znippy_bunzip2_batch (bz_plan.h).
#include "bz_plan.h"

#include <algorithm>

#include "deflate_batch.h"

namespace zn {

namespace bzp {

static void fail(Chain &c, int32_t status) {
    c.status = status;
    c.done = true;
}

size_t choose(std::vector<Chain> &items, size_t slot_cap, std::vector<BzJob> &jobs, std::vector<size_t> &first_job) {
    jobs.clear();
    first_job.assign(items.size() + 1, 0);
    size_t used = 0;  // slots taken: a block job has one, a header job needs none
    for (size_t k = 0; k < items.size(); k++) {
        Chain &c = items[k];
        first_job[k] = jobs.size();
        if (c.done || (c.kind == K_BLOCK && used >= slot_cap)) continue;
        uint64_t from = c.pos;  // candidates in front of this bit have been passed
        if (c.kind == K_HEAD) {
            jobs.push_back(BzJob{(uint32_t)k, K_HEAD, c.pos, 0, 0});
            from = 8 * c.pos + 32;
        }
        while (c.cur < c.n_cands && c.cands[c.cur] < from) c.cur++;
        if (c.kind == K_BLOCK && (c.cur == c.n_cands || c.cands[c.cur] != c.pos)) {  // (a record said that a block magic stands there)
            fail(c, BZ_E_CORRUPT);
            continue;
        }
        for (size_t j = c.cur; j < c.n_cands && used < slot_cap; j++) jobs.push_back(BzJob{(uint32_t)k, K_BLOCK, c.cands[j], (uint32_t)used++, 0});
    }
    first_job[items.size()] = jobs.size();
    for (size_t k = items.size(); k-- > 0;)  // (entries of items that got no job)
        if (first_job[k] > first_job[k + 1]) first_job[k] = first_job[k + 1];
    return jobs.size();
}

// the stream ended behind bit `end_bit` (where the end magic starts): its combined CRC, the padding, and what follows
static void stream_end(Chain &c, const BzRec &r, uint64_t end_bit) {
    const uint64_t trailer_end = end_bit + 48 + 32;
    if (r.after > c.src_len || 8 * r.after < trailer_end || 8 * r.after >= trailer_end + 8) return fail(c, BZ_E_CORRUPT);
    if (!c.measure && r.stream_crc != c.comb) c.sum_bad = true;
    c.streams++;
    c.comb = 0;
    if (c.src_len - r.after >= 3 && r.tail_len >= 3 && (r.tail & 0xFFFFFFu) == 0x685A42u) {  // "BZh": another stream, judged like the first
        c.kind = K_HEAD;
        c.pos = r.after;
    } else {
        c.done = true;  // any other rest is ignored
    }
}

static void advance_item(Chain &c, uint32_t k, const BzJob *jobs, const BzRec *recs, size_t j, size_t j1, std::vector<BzLand> &lands) {
    while (!c.done) {
        while (j < j1 && (jobs[j].kind != c.kind || jobs[j].pos < c.pos)) j++;
        if (j == j1) return;  // the record the chain waits for is a later pass's
        if (jobs[j].pos != c.pos) return fail(c, BZ_E_CORRUPT);  // (no candidate where a record said a block starts)
        const BzRec &r = recs[j];
        if (r.status != 0) return fail(c, r.status == BZ_E_UNSUPPORTED ? BZ_E_UNSUPPORTED : BZ_E_CORRUPT);
        if (r.next != NEXT_BLOCK && r.next != NEXT_END) return fail(c, BZ_E_CORRUPT);
        if (c.kind == K_HEAD) {
            if (r.level < 1 || r.level > 9 || 8 * c.pos + 32 + 48 > 8 * (uint64_t)c.src_len) return fail(c, BZ_E_CORRUPT);
            c.level = r.level;
            const uint64_t behind = 8 * c.pos + 32;
            if (r.next == NEXT_BLOCK) {
                c.kind = K_BLOCK;
                c.pos = behind;
            } else {
                stream_end(c, r, behind);
            }
            continue;
        }
        // a block: it ends behind its header, in front of a whole magic, and holds 1 .. level x 100,000 bytes
        if (r.end_bit <= c.pos + 48 + 32 + 1 + 24 || r.end_bit + 48 > 8 * (uint64_t)c.src_len) return fail(c, BZ_E_CORRUPT);
        if (r.n < 1 || r.n > c.level * 100000u || r.orig >= r.n) return fail(c, BZ_E_CORRUPT);
        if (!c.measure && r.out_len > c.room - c.out) return fail(c, BZ_E_DST_SMALL);
        if (!c.measure) lands.push_back(BzLand{k, jobs[j].slot, (uint32_t)c.out, r.out_len, r.n, r.block_crc});
        c.out += r.out_len;
        c.comb = (c.comb << 1 | c.comb >> 31) ^ r.block_crc;
        c.blocks++;
        if (r.next == NEXT_BLOCK) c.pos = r.end_bit;
        else stream_end(c, r, r.end_bit);
    }
}

void advance(std::vector<Chain> &items, const std::vector<BzJob> &jobs, const std::vector<size_t> &first_job, const BzRec *recs, std::vector<BzLand> &lands) {
    for (size_t k = 0; k < items.size(); k++) advance_item(items[k], (uint32_t)k, jobs.data(), recs, first_job[k], first_job[k + 1], lands);
}

void fold_crc(std::vector<Chain> &items, const std::vector<BzLand> &lands, const uint32_t *got) {
    for (size_t l = 0; l < lands.size(); l++)
        if (lands[l].crc != got[l]) items[lands[l].item].sum_bad = true;
}

}  // namespace bzp

int bz_admit(const BzCall &c, BzBatch &b) {
    b.measure = !c.d_out && !c.out_cap;
    b.st.assign(c.n, 0);
    b.cand_total = 0;
    Placement place;
    for (uint64_t i = 0; i < c.n; i++) {
        const uint64_t sl = c.src_len[i], room = b.measure ? 0 : c.out_room[i];
        uint64_t dst = 0;
        b.st[i] = place_item(place, c.src_off[i], sl, c.src_cap, !b.measure && c.out_off ? c.out_off + i : nullptr, room, c.out_cap, &dst);
        c.out_len[i] = 0;
        if (c.streams) c.streams[i] = 0;
        if (c.blocks) c.blocks[i] = 0;
        if (b.st[i] || !sl) continue;  // (no byte, no stream at all: nothing)
        BzItem it;
        it.src = c.d_src + c.src_off[i];
        it.dst = b.measure ? nullptr : c.d_out + dst;
        it.src_len = (uint32_t)sl; it.room = (uint32_t)room;
        b.cand_total += 8 * sl / 45 + 1;
        if (b.cand_total > BZ_LIST_MAX || b.chunks.size() + sl / BZ_SCAN_CHUNK + 1 > BZ_LIST_MAX || b.items.size() >= BZ_ITEMS_MAX) return BZ_E_NOMEM;
        for (uint64_t off = 0; off < sl; off += BZ_SCAN_CHUNK) b.chunks.push_back(BzChunk{(uint32_t)b.items.size(), (uint32_t)off});
        b.items.push_back(it);
        b.item_of.push_back((uint32_t)i);
    }
    return BZ_OK;
}

size_t bz_slots(const BzBatch &b, uint64_t slot_cap, uint64_t budget) {
    if (!slot_cap) slot_cap = budget / BZ_SLOT_BYTES;
    return (size_t)std::min<uint64_t>(slot_cap, b.cand_total);  // (a pass decodes every candidate at the most; cand_total >= 1 per item)
}

void bz_start(BzBatch &b, size_t n_raw) {
    std::sort(b.raw.begin(), b.raw.begin() + n_raw);
    b.cands.clear();
    b.chains.assign(b.items.size(), bzp::Chain{});
    std::vector<size_t> first(b.items.size() + 1, 0);
    size_t k = 0;
    for (size_t e = 0; e < n_raw; e++) {
        const uint64_t item = b.raw[e] >> 36, bit = b.raw[e] & ((1ull << 36) - 1);
        if (item >= b.items.size() || bit + 48 > 8 * (uint64_t)b.items[item].src_len) continue;
        if (e > 0 && b.raw[e] == b.raw[e - 1]) continue;  // (twice the same)
        while (k < item) first[++k] = b.cands.size();
        b.cands.push_back(bit);
    }
    while (k < b.items.size()) first[++k] = b.cands.size();
    for (size_t i = 0; i < b.items.size(); i++) {
        bzp::Chain &c = b.chains[i];
        c.src_len = b.items[i].src_len;
        c.room = b.items[i].room;
        c.measure = b.measure;
        c.cands = b.cands.data() + first[i];
        c.n_cands = first[i + 1] - first[i];
    }
}

void bz_verdict(const BzCall &c, BzBatch &b) {
    for (size_t k = 0; k < b.chains.size(); k++) {
        const uint32_t i = b.item_of[k];
        const bzp::Chain &ch = b.chains[k];
        b.st[i] = ch.done ? bzp::verdict(ch) : BZ_E_CORRUPT;  // (every chain is done when the passes end)
        if (b.st[i] != 0) continue;
        c.out_len[i] = ch.out;
        if (c.streams) c.streams[i] = ch.streams;
        if (c.blocks) c.blocks[i] = ch.blocks;
    }
}

}  // namespace zn
