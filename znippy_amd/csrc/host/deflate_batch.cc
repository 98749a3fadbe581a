// The host planning of znippy_inflate_batch, znippy_targz_find_batch and znippy_gunzip_batch (deflate_batch.h).
#include "deflate_batch.h"

#include <string.h>

#include <algorithm>

namespace zn {

int32_t place_item(Placement &p, uint64_t src_off, uint64_t src_len, uint64_t src_cap, const uint64_t *out_off, uint64_t out_len, uint64_t out_cap,
                   uint64_t *dst) {
    const bool dst_known = out_off || !p.wrapped;
    *dst = out_off ? *out_off : p.packed;
    if (!out_off) { p.wrapped |= p.packed + out_len < p.packed; p.packed += out_len; }
    if (src_off > src_cap || src_len > src_cap - src_off) return DB_E_INVAL;
    if (!dst_known || out_len > out_cap || *dst > out_cap - out_len) return DB_E_DST_SMALL;
    if (src_len >= (1ull << 32) || out_len >= (1ull << 32)) return DB_E_UNSUPPORTED;
    return DB_OK;
}

// ---- znippy_inflate_batch ----

void inflate_admit(const InflateCall &c, InflateBatch &b) {
    b.st.assign(c.n, 0);
    Placement place;
    for (uint64_t i = 0; i < c.n; i++) {
        const uint64_t sl = c.src_len[i], ol = c.out_len[i];
        const unsigned m = c.method ? c.method[i] : 8u;
        uint64_t dst;
        if ((b.st[i] = place_item(place, c.src_off[i], sl, c.src_cap, c.out_off ? c.out_off + i : nullptr, ol, c.out_cap, &dst))) continue;
        if (m != 0 && m != 8) { b.st[i] = DB_E_UNSUPPORTED; continue; }
        if (m == 0 && sl != ol) { b.st[i] = DB_E_CORRUPT; continue; }
        InflateItem it;
        it.src = c.d_src + c.src_off[i];
        it.dst = c.d_out + dst;
        it.src_len = (uint32_t)sl; it.out_len = (uint32_t)ol;
        it.method = m;
        it.want_crc = c.crc32 ? c.crc32[i] : 0; it.has_crc = c.crc32 ? 1 : 0;
        it.pad = 0;
        b.items.push_back(it);
        b.item_of.push_back((uint32_t)i);
    }
    b.h_st.assign(b.items.size(), 0);
    b.h_crc.assign(b.items.size(), 0);
}

void inflate_scatter(const InflateBatch &b, uint64_t n, int32_t *status, uint32_t *crc_out) {
    if (crc_out) memset(crc_out, 0, sizeof(uint32_t) * n);
    if (status) memcpy(status, b.st.data(), sizeof(int32_t) * n);
    for (size_t k = 0; k < b.items.size(); k++) {
        if (status) status[b.item_of[k]] = b.h_st[k];
        if (crc_out) crc_out[b.item_of[k]] = b.h_crc[k];
    }
}

// ---- znippy_targz_find_batch ----

int targz_admit(const TargzCall &c, TargzBatch &b) {
    b.st.assign(c.n, 0);
    b.need = 0;
    for (uint64_t i = 0; i < c.n; i++) {
        const uint64_t so = c.src_off[i], sl = c.src_len[i];
        c.out_off[i] = c.out_len[i] = 0;
        if (c.scanned) c.scanned[i] = 0;
        if (so > c.src_cap || sl > c.src_cap - so) { b.st[i] = DB_E_INVAL; continue; }
        if (sl >= (1ull << 32)) { b.st[i] = DB_E_UNSUPPORTED; continue; }
        // no valid DEFLATE expands more than 1032 : 1, and one item walks at most 4 GiB - 16 bytes of tar
        const uint64_t cap = std::min<uint64_t>(std::min<uint64_t>(c.scan_cap, 1032 * sl + 512), 0xFFFFFFF0ull);
        TargzItem it;
        it.src = c.d_src + so;
        it.scratch = nullptr;
        it.src_len = (uint32_t)sl; it.cap = (uint32_t)cap;
        it.whole = c.whole ? c.whole[i] != 0 : 1; it.pad = 0;
        b.items.push_back(it);
        b.slice.push_back(b.need);
        b.item_of.push_back((uint32_t)i);
        b.need += (cap + 15) & ~15ull;
        if (b.need > TARGZ_NEED_MAX) return DB_E_NOMEM;  // (the sum stays small)
    }
    b.res.assign(b.items.size(), TargzResult{});
    return DB_OK;
}

int targz_piece_bound(uint64_t out_cap, size_t n_items, size_t *max_pieces) {
    *max_pieces = (size_t)(out_cap / RANGE_PIECE) + 2 * n_items;
    return *max_pieces > RR_ITEMS_MAX ? DB_E_NOMEM : DB_OK;
}

void targz_bind(TargzBatch &b, uint8_t *scratch) {
    for (size_t k = 0; k < b.items.size(); k++) b.items[k].scratch = scratch + b.slice[k];
}

void targz_pack(const TargzCall &c, TargzBatch &b) {
    b.pieces.reserve(2 * b.items.size());
    uint64_t packed = 0;
    for (size_t k = 0; k < b.items.size(); k++) {
        const uint32_t i = b.item_of[k];
        const TargzResult &r = b.res[k];
        b.st[i] = r.status;
        if (c.scanned) c.scanned[i] = r.scanned;
        if (r.status != 0) continue;
        if (r.off > b.items[k].cap || r.len > b.items[k].cap - r.off) { b.st[i] = DB_E_CORRUPT; continue; }  // (the kernel's word is checked, not trusted)
        if (r.len > c.out_cap - packed) { b.st[i] = DB_E_DST_SMALL; continue; }
        c.out_off[i] = packed; c.out_len[i] = r.len;
        range_cut_pieces(b.items[k].scratch + r.off, c.d_out + packed, r.len, b.pieces);
        packed += r.len;
    }
}

// ---- znippy_gunzip_batch ----

int gz_admit(const GzCall &c, GzBatch &b) {
    b.st.assign(c.n, 0);
    b.cand_total = 0;
    Placement place;
    for (uint64_t i = 0; i < c.n; i++) {
        const uint64_t sl = c.src_len[i], room = c.out_room[i];
        uint64_t dst;
        b.st[i] = place_item(place, c.src_off[i], sl, c.src_cap, c.out_off ? c.out_off + i : nullptr, room, c.out_cap, &dst);
        c.out_len[i] = 0;
        if (c.members) c.members[i] = 0;
        if (c.segments) c.segments[i] = 0;
        if (b.st[i] || !sl) continue;  // (no byte, no member at all: nothing, as gzip.decompress(b"") gives)
        GzItem it;
        it.src = c.d_src + c.src_off[i];
        it.dst = c.d_out + dst;
        it.src_len = (uint32_t)sl; it.room = (uint32_t)room;
        it.cand_base = (uint32_t)b.cand_total; it.cand_cap = (uint32_t)(16 + sl / 256);
        b.cand_total += it.cand_cap;
        if (b.cand_total > GZ_LIST_MAX || b.chunks.size() + sl / GZ_SCAN_CHUNK + 1 > GZ_CHUNKS_MAX) return DB_E_NOMEM;
        for (uint64_t off = 0; off < sl; off += GZ_SCAN_CHUNK) b.chunks.push_back(GzScanChunk{(uint32_t)b.items.size(), (uint32_t)off});
        b.items.push_back(it);
        b.item_of.push_back((uint32_t)i);
    }
    b.count.assign(b.items.size(), 0);
    return DB_OK;
}

GzLayout gz_layout(const GzBatch &b) {
    GzLayout l;
    l.bytes = 0;
    auto carve = [&l](size_t sz) { const size_t at = l.bytes; l.bytes += (sz + 15) & ~(size_t)15; return at; };
    const size_t n_items = b.items.size(), n_kept_max = gz_kept_max(b);
    l.items = carve(sizeof(GzItem) * n_items);
    l.chunks = carve(sizeof(GzScanChunk) * b.chunks.size());
    l.count = carve(sizeof(uint32_t) * n_items);
    l.raw = carve(sizeof(uint64_t) * b.cand_total);
    l.cands = carve(sizeof(GzCand) * n_kept_max);
    l.stops = carve(sizeof(uint32_t) * b.cand_total);
    l.recs = carve(sizeof(GzProbe) * n_kept_max);
    l.runs = carve(sizeof(GzRun) * n_kept_max);
    l.run_st = carve(sizeof(int32_t) * n_kept_max);
    l.crc_items = carve(sizeof(InflateItem) * n_kept_max);
    l.crc_st = carve(sizeof(int32_t) * n_kept_max);
    l.crc_got = carve(sizeof(uint32_t) * n_kept_max);
    l.single_list = carve(sizeof(uint32_t) * n_items);
    l.single_res = carve(sizeof(GzSingle) * n_items);
    return l;
}

// the scan found candidates in item k, and no more than its slice holds
static bool gz_has_raw(const GzBatch &b, size_t k) { return b.count[k] && b.count[k] <= b.items[k].cand_cap; }

uint64_t gz_raw_end(const GzBatch &b) {
    uint64_t raw_end = 0;
    for (size_t k = 0; k < b.items.size(); k++)
        if (gz_has_raw(b, k)) raw_end = (uint64_t)b.items[k].cand_base + b.count[k];
    return raw_end;
}

int gz_candidates(GzBatch &b, uint64_t seg_min) {
    for (uint32_t k = 0; k < b.items.size(); k++) {
        if (k < b.cut_done.size() && b.cut_done[k]) continue;  // (decoded already, at block starts: api.hip, host/gz_cut_plan.h)
        if (!gz_has_raw(b, k)) { b.single.push_back(k); continue; }  // (its slice of raw was not copied back, or holds nothing)
        uint64_t *const c = b.raw.data() + b.items[k].cand_base;
        const size_t kept = gzp::keep_candidates(c, b.count[k], seg_min);
        if (!kept) { b.single.push_back(k); continue; }
        b.probed.push_back(k);
        b.first_cand.push_back(b.cands.size());
        const uint32_t stop_begin = (uint32_t)b.stops.size();
        for (size_t j = 0; j < kept; j++)
            if ((c[j] & 1) == gzp::K_FLUSH) b.stops.push_back((uint32_t)(c[j] >> 1));
        const uint32_t stop_end = (uint32_t)b.stops.size();
        b.cands.push_back(GzCand{k, 0, gzp::K_MEMBER, stop_begin, stop_end, 0});
        uint32_t next_stop = stop_begin;  // the first flush candidate behind the position
        for (size_t j = 0; j < kept; j++) {
            const uint32_t pos = (uint32_t)(c[j] >> 1), kind = (uint32_t)(c[j] & 1);
            while (next_stop < stop_end && b.stops[next_stop] <= pos) next_stop++;
            b.cands.push_back(GzCand{k, pos, kind, next_stop, stop_end, 0});
        }
    }
    b.first_cand.push_back(b.cands.size());
    if (b.cands.size() > gz_kept_max(b) || b.stops.size() > b.cand_total) return DB_E_NOMEM;
    b.recs.assign(b.cands.size(), GzProbe{});
    b.sres.assign(b.single.size(), GzSingle{});
    return DB_OK;
}

static void gz_crc_item(GzBatch &b, uint8_t *dst, uint64_t len, bool has, uint32_t want) {
    InflateItem it;
    it.src = nullptr; it.dst = dst; it.src_len = 0; it.out_len = (uint32_t)len;
    it.method = 8; it.want_crc = want; it.has_crc = has ? 1 : 0; it.pad = 0;
    b.crc_items.push_back(it);
}

int gz_decode_plan(GzBatch &b) {
    b.item_st.assign(b.items.size(), 0);
    // the single pass: the first member of every item that decoded is left to the CRC launch
    for (size_t e = 0; e < b.single.size(); e++) {
        const uint32_t k = b.single[e];
        const GzSingle &r = b.sres[e];
        b.item_st[k] = r.status;
        if (r.status == 0 && (r.out_len > b.items[k].room || r.len0 > r.out_len)) b.item_st[k] = DB_E_CORRUPT;  // (the kernel's word is checked, not trusted)
        if (b.item_st[k] != 0) continue;
        gz_crc_item(b, b.items[k].dst, r.len0, true, r.crc0);
        b.crc_item_of.push_back(k);
    }
    // the probed items: plan_item checks the records
    b.plans.assign(b.probed.size(), gzp::ItemPlan{});
    for (size_t j = 0; j < b.probed.size(); j++) {
        const uint32_t k = b.probed[j];
        b.scratch.clear();
        for (size_t c = b.first_cand[j]; c < b.first_cand[j + 1]; c++) {
            const GzProbe &r = b.recs[c];
            b.scratch.push_back(gzp::Probe{b.cands[c].pos, b.cands[c].kind, r.data_start, r.end_kind, r.end_pos, r.status, r.out, r.reach, r.crc, r.isize, r.next});
        }
        gzp::plan_item(b.scratch.data(), b.scratch.size(), k, b.items[k].src_len, b.items[k].room, b.runs, b.mems, &b.plans[j]);
        b.item_st[k] = b.plans[j].status;
    }
    // the non-empty runs: one wave of the decode launch and one entry of the CRC launch each (the CRCs of a member's runs are
    // combined on the host: a long member is many workgroups)
    b.crc_of_run.assign(b.runs.size(), 0);
    for (size_t r = 0; r < b.runs.size(); r++) {
        const gzp::Run &run = b.runs[r];
        if (!run.out_len) continue;
        b.h_runs.push_back(GzRun{run.item, run.src_start, (uint32_t)run.out_off, (uint32_t)run.out_len});
        b.run_item.push_back(run.item);
        b.crc_of_run[r] = b.crc_items.size();
        gz_crc_item(b, b.items[run.item].dst + run.out_off, run.out_len, false, 0);
    }
    if (b.h_runs.size() > gz_kept_max(b) || b.crc_items.size() > gz_kept_max(b)) return DB_E_NOMEM;
    b.run_st.assign(b.h_runs.size(), 0);
    b.crc_st.assign(b.crc_items.size(), 0);
    b.crc_got.assign(b.crc_items.size(), 0);
    return DB_OK;
}

void gz_verdict(const GzCall &c, GzBatch &b) {
    for (size_t r = 0; r < b.h_runs.size(); r++)
        if (b.run_st[r] != 0) b.item_st[b.run_item[r]] = DB_E_CORRUPT;
    // (the status test below is defensive: a single item that failed has no CRC entry, and the loop above touches probed items only)
    for (size_t f = 0; f < b.crc_item_of.size(); f++)
        if (b.crc_st[f] != 0 && b.item_st[b.crc_item_of[f]] == 0) b.item_st[b.crc_item_of[f]] = DB_E_CHECKSUM;
    for (const gzp::Member &m : b.mems) {
        uint32_t crc = 0;
        for (size_t r = m.run0; r < m.run1; r++)
            if (b.runs[r].out_len) crc = gzp::crc32_combine(crc, b.crc_got[b.crc_of_run[r]], b.runs[r].out_len);
        if (crc != m.crc && b.item_st[m.item] == 0) b.item_st[m.item] = DB_E_CHECKSUM;
    }
    for (size_t e = 0; e < b.single.size(); e++) {
        const uint32_t k = b.single[e], i = b.item_of[k];
        b.st[i] = b.item_st[k];
        if (b.st[i] != 0) continue;
        c.out_len[i] = b.sres[e].out_len;
        if (c.members) c.members[i] = b.sres[e].members;
        if (c.segments) c.segments[i] = 1;
    }
    for (size_t j = 0; j < b.probed.size(); j++) {
        const uint32_t k = b.probed[j], i = b.item_of[k];
        b.st[i] = b.item_st[k];
        if (b.st[i] != 0) continue;
        c.out_len[i] = b.plans[j].out_len;
        if (c.members) c.members[i] = b.plans[j].members;
        if (c.segments) c.segments[i] = b.plans[j].segments;
    }
}

}  // namespace zn
