// The host planning of znippy_tar_list_batch; see tar_list_plan.h.
#include "tar_list_plan.h"

#include <string.h>

#include <algorithm>

namespace zn {

int tl_admit(const TlCall &c, TlBatch &b) {
    b.measure = !c.members;
    b.st.assign(c.n, TL_OK);
    for (uint64_t i = 0; i <= c.n; i++) c.member_first[i] = 0;
    *c.names_bytes = *c.out_bytes = 0;
    uint64_t nodes = 0;
    for (uint64_t i = 0; i < c.n; i++) {
        const uint64_t off = c.tar_off[i], len = c.tar_len[i];
        if (off > c.tar_cap || len > c.tar_cap - off) { b.st[i] = TL_E_INVAL; continue; }
        if (len >= (1ull << 32)) { b.st[i] = TL_E_UNSUPPORTED; continue; }
        if (!len) continue;
        const uint32_t blocks = (uint32_t)(len / 512);
        if (nodes + blocks + 1 > TL_NODES_MAX) return TL_E_NOMEM;
        const uint32_t k = (uint32_t)b.items.size();
        b.items.push_back(TlItem{c.d_tar + off, (uint32_t)len, blocks, (uint32_t)nodes, (uint32_t)b.chunks.size()});
        b.item_of.push_back((uint32_t)i);
        for (uint32_t first = 0; first <= blocks; first += TL_CHUNK) b.chunks.push_back(TlChunk{k, first, std::min(TL_CHUNK, blocks + 1 - first), 0});
        nodes += blocks + 1;
        b.max_nodes = std::max(b.max_nodes, blocks + 1);
    }
    b.n_nodes = nodes;
    b.totals.assign(b.items.size(), TlTotal{0, 0, 0, 0});
    b.bases.assign(b.items.size(), TlBase{0, 0, 0, 0, 0});
    return TL_OK;
}

TlLayout tl_layout(const TlBatch &b, uint64_t filter_bytes) {
    TlLayout at{};
    auto carve = [&at](size_t sz) { const size_t o = at.bytes; at.bytes += (sz + 15) & ~(size_t)15; return o; };
    const size_t n_items = b.items.size(), n_chunks = b.chunks.size(), n_nodes = (size_t)b.n_nodes;
    at.items = carve(sizeof(TlItem) * n_items);
    at.chunks = carve(sizeof(TlChunk) * n_chunks);
    at.filter = carve(filter_bytes + 16);
    at.nodes = carve(sizeof(TlNode) * n_nodes);
    at.mark = carve(n_nodes);
    at.jump_a = carve(sizeof(uint32_t) * n_nodes);
    at.jump_b = carve(sizeof(uint32_t) * n_nodes);
    at.pred = carve(sizeof(uint32_t) * n_nodes);
    at.pick = carve(sizeof(uint32_t) * n_nodes);
    at.src = carve(sizeof(uint32_t) * n_nodes);
    at.sums = carve(sizeof(TlSum) * (n_chunks + 1));
    at.totals = carve(sizeof(TlTotal) * n_items);
    at.bases = carve(sizeof(TlBase) * n_items);
    return at;
}

uint32_t tl_rounds(uint32_t max_nodes) {
    uint32_t r = 0;
    while (r < 32 && (1ull << r) < max_nodes) r++;
    return r;
}

int tl_staging(const TlCall &c, const TlBatch &b, size_t *members, size_t *names, size_t *pieces) {
    *members = *names = *pieces = 0;
    if (b.measure) return TL_OK;
    uint64_t blocks = 0, bytes = 0;
    for (const TlItem &it : b.items) { blocks += it.blocks; bytes += it.len; }
    const uint64_t m = std::min(c.members_cap, blocks), nb = std::min(c.names_cap, bytes);
    // a member with bytes takes two blocks at the least; a piece per RANGE_PIECE bytes of output and two more per such member
    const uint64_t p = c.d_out ? std::min(c.out_cap, bytes) / RANGE_PIECE + 2 * std::min(m, blocks / 2) : 0;
    if (p >= (1ull << 32)) return TL_E_NOMEM;
    *members = (size_t)m; *names = (size_t)nb; *pieces = (size_t)p;
    return TL_OK;
}

void tl_place(const TlCall &c, TlBatch &b) {
    uint64_t m = 0, nb = 0, ob = 0;
    size_t k = 0;
    for (uint64_t i = 0; i < c.n; i++) {
        c.member_first[i] = m;
        if (k == b.items.size() || b.item_of[k] != i) continue;
        const TlItem &it = b.items[k];
        const TlTotal &t = b.totals[k];
        TlBase &base = b.bases[k];
        k++;
        base = TlBase{0, 0, 0, 0, 0};
        if (t.key != TL_KEY_NONE) {
            const uint64_t code = t.key & 255, node = t.key >> 8;
            b.st[i] = code == TL_KEY_UNSUP && node <= it.blocks ? TL_E_UNSUPPORTED : TL_E_CORRUPT;
            continue;
        }
        // a member takes a block, a name's bytes are bytes of the item, and so are the members' own
        if (t.cnt > it.blocks || t.names > it.len || t.out > it.len) { b.st[i] = TL_E_CORRUPT; continue; }
        if (!b.measure &&
            (t.cnt > c.members_cap - m || t.names > c.names_cap - nb || (c.d_out && t.out > c.out_cap - std::min(ob, c.out_cap)))) {
            b.st[i] = TL_E_DST_SMALL;
            continue;
        }
        base = TlBase{m, nb, ob, 1, 0};
        m += t.cnt; nb += t.names; ob += t.out;
    }
    c.member_first[c.n] = m;
    *c.names_bytes = nb;
    *c.out_bytes = ob;
    b.take_members = m; b.take_names = nb; b.take_out = ob;
}

namespace {
// the records of one taken item against the item: true if they are what a listing of it can be
bool records_hold(const TlItem &it, const TlTotal &t, const TlBase &base, const znippy_tar_member *recs, size_t n_recs, size_t n_names) {
    if (base.member > n_recs || t.cnt > n_recs - base.member || base.names > n_names || t.names > n_names - base.names) return false;
    uint64_t floor = 0, nb = 0, ob = 0;  // floor: where the next header may stand at the earliest
    for (uint64_t j = 0; j < t.cnt; j++) {
        const znippy_tar_member &r = recs[base.member + j];
        if (r.header_off % 512 || r.header_off < floor || r.header_off > it.len || it.len - r.header_off < 512) return false;
        if (r.data_off != r.header_off + 512 || r.size > it.len - r.data_off) return false;
        if (r.typeflag != '0' && r.typeflag != 0 && r.typeflag != '7') return false;
        if (r.name_off != base.names + nb || r.name_len > t.names - nb) return false;
        if (r.out_off != base.out + ob || r.size > t.out - ob) return false;
        floor = r.data_off + ((r.size + 511) & ~511ull);
        nb += r.name_len; ob += r.size;
    }
    return nb == t.names && ob == t.out;
}
}  // namespace

void tl_accept(const TlCall &c, TlBatch &b, const znippy_tar_member *recs, size_t n_recs, const char *names, size_t n_names) {
    uint64_t m = 0, nb = 0, ob = 0;
    size_t k = 0;
    b.pieces.clear();
    for (uint64_t i = 0; i < c.n; i++) {
        c.member_first[i] = m;
        if (k == b.items.size() || b.item_of[k] != i) continue;
        const TlItem &it = b.items[k];
        const TlTotal &t = b.totals[k];
        const TlBase &base = b.bases[k];
        k++;
        if (!base.take) continue;
        // (m, nb and ob never pass the places tl_place gave out, so what fitted there fits here)
        if (!records_hold(it, t, base, recs, n_recs, n_names) || t.cnt > c.members_cap - m || t.names > c.names_cap - nb) {
            b.st[i] = TL_E_CORRUPT;
            continue;
        }
        for (uint64_t j = 0; j < t.cnt; j++) {
            znippy_tar_member r = recs[base.member + j];
            r.name_off = r.name_off - base.names + nb;
            r.out_off = r.out_off - base.out + ob;
            c.members[m + j] = r;
            if (c.d_out && r.size) range_cut_pieces(it.base + r.data_off, c.d_out + r.out_off, r.size, b.pieces);
        }
        if (t.names) memcpy(c.names + nb, names + base.names, t.names);
        m += t.cnt; nb += t.names; ob += t.out;
    }
    c.member_first[c.n] = m;
    *c.names_bytes = nb;
    *c.out_bytes = ob;
}

}  // namespace zn
