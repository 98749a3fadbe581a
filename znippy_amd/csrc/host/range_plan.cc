// The plan of a range read and of a block-tree build (range_plan.h): arithmetic on caller data, stage by stage in the order api.hip
// runs the device passes between them.  Every sum of untrusted numbers is either checked before it is formed or meant modulo 2^64
// and said so.
#include "range_plan.h"

#include <string.h>

#include <algorithm>
#include <unordered_map>

namespace zn {

bool rr_blob_in_region(const RrTable &t, uint32_t ri, uint64_t blob_base) {
    const uint64_t bo = t.h_blob_off[ri], bs = t.h_blob_size[ri], bcap = t.blob_cap;
    return !(bo < blob_base || (bcap != ~0ull && (bs > bcap || bo - blob_base > bcap - bs)));
}

bool rr_slot_take(uint64_t &need, uint64_t front, uint64_t bytes, uint64_t &slot) {
    if (bytes > RR_SCRATCH_MAX) return false;  // (before it is added: a length near 2^64 must not wrap the sum)
    need = (need + 255) & ~255ull;
    slot = need + front;
    need = slot + bytes + 256;
    return need <= RR_SCRATCH_MAX;
}

// block k of a row of row_len bytes whose first entry is entry0, at `src`
static BlockCvItem block_cv_item(const uint8_t *src, uint64_t entry0, uint64_t row_len, uint32_t k) {
    return BlockCvItem{src, entry0 + k, (uint32_t)std::min<uint64_t>(RR_BLK, row_len - (uint64_t)k * RR_BLK), 128u * k};
}

int range_plan_build(const RrTable &t, const RrCall &c, RangePlan &p) {
    // verified: a row is looked at block by block only if its entries are installed and fold to its checksum
    auto by_blocks = [&](uint32_t ri) { return !c.verified || (ri < t.n_tree_accept && t.tree_accept[ri]); };

    // 1) every range against the table, the output region and the blob region; the distinct rows the good ones touch
    p.st.assign(c.n_ranges, 0);
    p.dst.assign(c.n_ranges, 0);
    p.of_row.assign(c.n_ranges, 0xFFFFFFFFu);
    std::unordered_map<uint32_t, uint32_t> row_at;
    uint64_t packed = 0;
    bool packed_wrap = false;
    for (uint64_t i = 0; i < c.n_ranges; i++) {
        const uint64_t len = c.len[i], begin = c.begin[i];
        const bool dst_known = c.out || !packed_wrap;
        p.dst[i] = c.out ? c.out[i] : packed;
        if (!c.out) { packed_wrap |= packed + len < packed; packed += len; }
        if (c.row[i] < t.row_begin || c.row[i] - t.row_begin >= t.n) { p.st[i] = RP_E_INVAL; continue; }
        const uint32_t ri = (uint32_t)(c.row[i] - t.row_begin);
        const uint64_t row_len = t.h_len[ri];
        if (begin > row_len || len > row_len - begin) { p.st[i] = RP_E_INVAL; continue; }
        if (!dst_known || len > c.out_cap || p.dst[i] > c.out_cap - len) { p.st[i] = RP_E_DST_SMALL; continue; }
        if (!rr_blob_in_region(t, ri, c.blob_base)) { p.st[i] = RP_E_CORRUPT; continue; }
        if (!len) continue;
        auto it = row_at.find(ri);
        if (it == row_at.end()) {
            it = row_at.emplace(ri, (uint32_t)p.rows.size()).first;
            RrRow w;
            w.row = ri;
            w.comp = t.h_comp[ri] != 0;
            w.partial = w.comp && rr_by_blocks(row_len) && by_blocks(ri);
            w.sblocks = c.verified && !w.comp && rr_by_blocks(row_len) && by_blocks(ri);
            if (w.partial || w.sblocks) w.need.assign((size_t)((row_len + RR_BLK - 1) / RR_BLK), 0);
            p.rows.push_back(std::move(w));
        }
        p.of_row[i] = it->second;
        RrRow &w = p.rows[it->second];
        if (w.partial || w.sblocks) {
            const uint32_t k0 = (uint32_t)(begin / RR_BLK), k1 = (uint32_t)((begin + len - 1) / RR_BLK);
            for (uint32_t k = k0; k <= k1; k++) w.need[k] = 1;
            w.kmin = std::min(w.kmin, k0); w.kmax = std::max(w.kmax, k1);
        }
    }

    // 2) slots in the scratch, the lists of the block pass, the rows decoded whole from the start
    for (uint32_t i = 0; i < p.rows.size(); i++) {
        RrRow &w = p.rows[i];
        if (!w.comp) {
            if (c.verified && !w.sblocks) p.stored_whole.push_back(i);  // hashed whole, where it lies, by a private verify-only run
            continue;
        }
        if (w.partial && p.n_items + w.need.size() >= RR_ITEMS_MAX) w.partial = false;
        const uint64_t row_len = t.h_len[w.row];
        bool fits;
        if (w.partial) {
            p.part.push_back(i);
            p.n_items += w.need.size();
            for (uint32_t k = w.kmin; k <= w.kmax; k++) p.n_todo += w.need[k];
            w.first = (uint64_t)w.kmin * RR_BLK;
            fits = rr_slot_take(p.need0, RR_GUARD, std::min<uint64_t>(row_len, ((uint64_t)w.kmax + 1) * RR_BLK) - w.first, w.slot);
        } else {
            p.whole.push_back(i);
            fits = rr_slot_take(p.need0, 0, row_len, w.slot);
        }
        if (!fits) return RP_E_NOMEM;
    }
    return RP_OK;
}

namespace {
struct Carver {  // 16-byte aligned pieces of a slab, one after the other; without a base only their sizes are added up
    uint8_t *base;
    size_t at = 0;
    template <class T>
    void take(T *&p, size_t n) {
        at = (at + 15) & ~(size_t)15;
        p = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += sizeof(T) * n;
    }
};
size_t carve(uint8_t *base, const RangePlan &p, RangeSlab &o, size_t *up_bytes) {
    const size_t m = p.part.size(), n_items = (size_t)p.n_items, n_todo = (size_t)p.n_todo;
    Carver c{base};
    c.take(o.blob_off, m); c.take(o.blob_size, m); c.take(o.usize, m); c.take(o.out_off, m); c.take(o.block_bytes, m);
    c.take(o.cand_row, m); c.take(o.cand_base, m); c.take(o.cand_nb, m);
    c.take(o.item_row, n_items); c.take(o.item_k, n_items); c.take(o.todo, n_todo);
    c.take(o.ctl, 4); c.take(o.status, m); c.take(o.comp, m);
    c.take(o.decoded, 1);
    if (up_bytes) *up_bytes = c.at;  // everything up to here is uploaded; what follows is written on the device first
    c.take(o.row_flag, m); c.take(o.item_src, n_items); c.take(o.late, m);
    return c.at;
}
}  // namespace

size_t range_slab_layout(const RangePlan &p, size_t *up_bytes) {
    RangeSlab none;
    return carve(nullptr, p, none, up_bytes);
}

void range_slab_bind(uint8_t *base, const RangePlan &p, RangeSlab &slab) { carve(base, p, slab, nullptr); }

void range_slab_fill(const RrTable &t, const RangePlan &p, uint8_t *host_base) {
    RangeSlab h;
    size_t up_bytes = 0;
    carve(host_base, p, h, &up_bytes);
    memset(host_base, 0, up_bytes);
    uint32_t item = 0, todo = 0;
    for (uint32_t c = 0; c < p.part.size(); c++) {
        const RrRow &w = p.rows[p.part[c]];
        const uint64_t row_len = t.h_len[w.row];
        h.blob_off[c] = t.h_blob_off[w.row]; h.blob_size[c] = t.h_blob_size[w.row]; h.usize[c] = row_len;
        // the block decoder puts block k at out + out_off + k * 128 KiB: the column is biased (modulo 2^64, as the kernels add) so that
        // the row's first needed block lands at the head of its slot
        h.out_off[c] = w.slot - w.first;
        h.cand_row[c] = c; h.cand_base[c] = item; h.cand_nb[c] = (uint32_t)w.need.size();
        h.comp[c] = 1;
        for (uint32_t k = 0; k < w.need.size(); k++) {
            h.item_row[item + k] = c; h.item_k[item + k] = k;
            if (!w.need[k]) continue;
            h.todo[todo++] = item + k;
            h.block_bytes[c] += std::min<uint64_t>(RR_BLK, row_len - (uint64_t)k * RR_BLK);
        }
        item += (uint32_t)w.need.size();
    }
    h.ctl[0] = todo;  // [0] length of the to-do list, [1] the decoder's work cursor, [2] a hand-over count that stays zero
}

int range_plan_late(const RrTable &t, RangePlan &p, const uint8_t *late_flags, std::vector<uint32_t> &late_rows, uint64_t &need1) {
    need1 = 0;
    for (uint32_t c = 0; c < p.part.size(); c++) {
        if (!late_flags[c]) continue;
        RrRow &w = p.rows[p.part[c]];
        w.late = true; w.pool = 1; w.first = 0;
        if (!rr_slot_take(need1, 0, t.h_len[w.row], w.slot)) return RP_E_NOMEM;
        late_rows.push_back(p.part[c]);
    }
    return RP_OK;
}

uint64_t range_plan_block_items(const RrTable &t, RangePlan &p, const uint8_t *pool0, const uint8_t *d_blobs, uint64_t blob_base,
                                std::vector<BlockCvItem> &items, std::vector<std::pair<uint32_t, uint32_t>> &item_of) {
    uint64_t hashed = 0;
    for (uint32_t i = 0; i < p.rows.size(); i++) {
        RrRow &w = p.rows[i];
        const uint64_t row_len = t.h_len[w.row];
        if (w.hashed) hashed += row_len;
        if (!((w.partial && !w.late) || w.sblocks) || w.status) continue;
        w.bad.assign(w.need.size(), 0);
        for (uint32_t k = w.kmin; k <= w.kmax; k++) {
            if (!w.need[k]) continue;
            const uint64_t at = (uint64_t)k * RR_BLK;
            const uint8_t *src = w.comp ? pool0 + w.slot + (at - w.first) : d_blobs + (t.h_blob_off[w.row] - blob_base) + at;
            items.push_back(block_cv_item(src, t.tree_first[w.row], row_len, k));
            item_of.emplace_back(i, k);
            hashed += items.back().bytes;
        }
    }
    return hashed;
}

uint64_t range_plan_decoded(const RrTable &t, const RangePlan &p, uint64_t dec_blocks) {
    uint64_t dec = dec_blocks;
    for (const RrRow &w : p.rows)
        if (w.comp && (!w.partial || w.late) && (w.status == 0 || w.status == RP_E_DIGEST)) dec += t.h_len[w.row];
    return dec;
}

void range_cut_pieces(const uint8_t *src, uint8_t *dst, uint64_t len, std::vector<RangePiece> &pieces) {
    uint64_t step = std::min<uint64_t>(len, RANGE_PIECE - ((uintptr_t)dst & 127));  // every later piece starts on a 128-byte line of the output
    while (len) {
        pieces.push_back(RangePiece{src, dst, (uint32_t)step, 0});
        src += step; dst += step; len -= step;
        step = std::min<uint64_t>(len, RANGE_PIECE);
    }
}

void range_plan_pieces(const RrTable &t, const RrCall &c, RangePlan &p, const uint8_t *const pools[2], const uint8_t *d_blobs, uint8_t *d_out,
                       std::vector<RangePiece> &pieces) {
    for (uint64_t i = 0; i < c.n_ranges; i++) {
        if (p.of_row[i] == 0xFFFFFFFFu) continue;
        const RrRow &w = p.rows[p.of_row[i]];
        if (w.status) { p.st[i] = w.status; continue; }
        if (!w.bad.empty()) {  // a block whose hash does not chain to the checksum fails every range that overlaps it
            bool bad = false;
            for (uint64_t k = c.begin[i] / RR_BLK; k <= (c.begin[i] + c.len[i] - 1) / RR_BLK; k++) bad |= w.bad[k] != 0;
            if (bad) { p.st[i] = RP_E_DIGEST; continue; }
        }
        const uint8_t *src = w.comp ? pools[w.pool] + w.slot + (c.begin[i] - w.first) : d_blobs + (t.h_blob_off[w.row] - c.blob_base) + c.begin[i];
        range_cut_pieces(src, d_out + p.dst[i], c.len[i], pieces);
    }
}

int tree_plan_rows(const RrTable &t, uint64_t blob_base, std::vector<int32_t> &st, std::vector<RrRow> &rows, std::vector<uint32_t> &sel, uint64_t &need0) {
    need0 = 0;
    for (uint32_t ri = 0; ri < t.n; ri++) {
        if (t.tree_first[ri + 1] == t.tree_first[ri]) continue;
        if (!rr_blob_in_region(t, ri, blob_base)) { st[ri] = RP_E_CORRUPT; continue; }
        RrRow w;
        w.row = ri;
        w.comp = t.h_comp[ri] != 0;
        if (w.comp) {
            if (!rr_slot_take(need0, 0, t.h_len[ri], w.slot)) return RP_E_NOMEM;
            sel.push_back((uint32_t)rows.size());
        }
        rows.push_back(std::move(w));
    }
    return RP_OK;
}

void tree_plan_items(const RrTable &t, const std::vector<RrRow> &rows, const uint8_t *pool0, const uint8_t *d_blobs, uint64_t blob_base,
                     std::vector<int32_t> &st, std::vector<uint32_t> &good, std::vector<BlockCvItem> &items) {
    for (const RrRow &w : rows) {
        if (w.status) { st[w.row] = w.status; continue; }
        good.push_back(w.row);
        const uint8_t *base = w.comp ? pool0 + w.slot : d_blobs + (t.h_blob_off[w.row] - blob_base);
        const uint32_t nb = (uint32_t)(t.tree_first[w.row + 1] - t.tree_first[w.row]);
        for (uint32_t k = 0; k < nb; k++) items.push_back(block_cv_item(base + (uint64_t)k * RR_BLK, t.tree_first[w.row], t.h_len[w.row], k));
    }
}

}  // namespace zn
