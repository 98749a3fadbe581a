// The host planning of znippy_unxz_batch (xz_plan.h says what it does and why nothing here trusts a byte or a record).
#include "xz_plan.h"

#include <algorithm>

#include "deflate_batch.h"  // the placement rule

namespace zn {

namespace xzp {

namespace {

enum { S_TAIL = 0, S_INDEX = 1, S_HEADER = 2 };
constexpr uint64_t SAT = 1ull << 62;

inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

void fail(Walk &w, int32_t st) {
    w.status = st;
    w.done = true;
    w.want_len = 0;
}
void ask(Walk &w, uint64_t off, uint64_t len) {
    w.want_off = off;
    w.want_len = len;
}
void ask_tail(Walk &w) {
    const uint64_t len = std::min<uint64_t>(w.end, XZ_TAIL);
    w.stage = S_TAIL;
    ask(w, w.end - len, len);
}

}  // namespace

uint32_t crc32(const uint8_t *p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}

bool vli(const uint8_t *p, size_t end, size_t *pos, uint64_t *v) {
    uint64_t r = 0;
    for (uint32_t i = 0; i < 9; i++) {
        if (*pos >= end) return false;
        const uint8_t b = p[(*pos)++];
        r |= (uint64_t)(b & 0x7F) << (7 * i);
        if (!(b & 0x80)) {
            if (b == 0 && i > 0) return false;  // a needless trailing zero byte
            *v = r;
            return true;
        }
    }
    return false;  // longer than 9 bytes
}

void start(Walk &w, uint64_t src_len) {
    w = Walk{};
    w.src_len = src_len;
    w.end = src_len;
    if (!src_len) {
        w.done = true;
        return;
    }
    ask_tail(w);
    w.want_head = src_len > XZ_TAIL;  // (a shorter item's first range holds them)
}

void give_head(Walk &w, const uint8_t *first12) {
    if (!w.want_head) return;
    for (int k = 0; k < 12; k++) w.head[k] = first12[k];
    w.want_head = false;
    w.have_head = true;
}

void give(Walk &w, const uint8_t *bytes) {
    if (w.done) return;
    const uint64_t wo = w.want_off, wl = w.want_len;
    auto in = [&](uint64_t off, uint64_t len) -> const uint8_t * {
        if (off >= wo && len <= wl && off - wo <= wl - len) return bytes + (off - wo);
        return w.have_head && off == 0 && len == 12 ? w.head : nullptr;
    };
    for (;;) {
        if (w.stage == S_TAIL) {
            // stream padding, four zero bytes at a time
            while (w.end >= 4) {
                const uint8_t *p = in(w.end - 4, 4);
                if (!p) return ask_tail(w);  // (the bytes given have been used up: `end` has moved)
                if (p[0] | p[1] | p[2] | p[3]) break;
                w.end -= 4;
            }
            if (w.end < 32) return fail(w, XZ_E_CORRUPT);  // no room for a stream: padding at the start, nothing but padding, or a stump
            const uint8_t *p = in(w.end - 12, 12);
            if (!p) return ask_tail(w);
            if (p[10] != 'Y' || p[11] != 'Z') return fail(w, XZ_E_CORRUPT);
            if (crc32(p + 4, 6) != le32(p)) return fail(w, XZ_E_CORRUPT);
            if (p[8] != 0 || (p[9] & 0xF0)) return fail(w, XZ_E_UNSUPPORTED);
            w.flags[0] = p[8];
            w.flags[1] = p[9];
            const uint64_t backward = ((uint64_t)le32(p + 4) + 1) * 4, index_end = w.end - 12;
            if (backward > index_end - 12) return fail(w, XZ_E_CORRUPT);  // (end >= 32) no room for the index and a stream header
            w.index_size = backward;
            w.index_start = index_end - backward;
            w.stage = S_INDEX;
        }
        if (w.stage == S_INDEX) {
            const uint8_t *p = in(w.index_start, w.index_size);
            if (!p) return ask(w, w.index_start, w.index_size);
            const size_t limit = (size_t)w.index_size - 4;  // (index_size >= 4)
            if (p[0] != 0) return fail(w, XZ_E_CORRUPT);
            if (crc32(p, limit) != le32(p + limit)) return fail(w, XZ_E_CORRUPT);
            size_t pos = 1;
            uint64_t count = 0;
            if (!vli(p, limit, &pos, &count)) return fail(w, XZ_E_CORRUPT);
            if (count > (limit - pos) / 2) return fail(w, XZ_E_CORRUPT);  // a record is two bytes at the least
            Stream s;
            s.first = w.blocks.size();
            s.n = (size_t)count;
            s.check = w.flags[1] & 0x0F;
            uint64_t sum = 0;
            for (uint64_t r = 0; r < count; r++) {
                Block b;
                if (!vli(p, limit, &pos, &b.unpadded) || !vli(p, limit, &pos, &b.uncomp)) return fail(w, XZ_E_CORRUPT);
                if (b.unpadded < 5 || b.unpadded > w.index_start) return fail(w, XZ_E_CORRUPT);
                sum += (b.unpadded + 3) & ~3ull;  // (both below 2^32 + 4)
                if (sum > w.index_start) return fail(w, XZ_E_CORRUPT);
                w.content = std::min<uint64_t>(w.content + std::min<uint64_t>(b.uncomp, SAT), SAT);
                w.blocks.push_back(b);
            }
            if (limit - pos >= 4) return fail(w, XZ_E_CORRUPT);
            for (; pos < limit; pos++)
                if (p[pos]) return fail(w, XZ_E_CORRUPT);
            if (sum + 12 > w.index_start) return fail(w, XZ_E_CORRUPT);
            if (w.content >= (1ull << 32)) w.too_big = true;
            s.hdr_pos = w.index_start - sum - 12;
            w.streams.push_back(s);
            w.stage = S_HEADER;
        }
        if (w.stage == S_HEADER) {
            const uint64_t at = w.streams.back().hdr_pos;
            const uint8_t *p = in(at, 12);
            if (!p) return ask(w, at, 12);
            static const uint8_t magic[6] = {0xFD, '7', 'z', 'X', 'Z', 0x00};
            for (int k = 0; k < 6; k++)
                if (p[k] != magic[k]) return fail(w, XZ_E_CORRUPT);
            if (crc32(p + 6, 2) != le32(p + 8)) return fail(w, XZ_E_CORRUPT);
            if (p[6] != w.flags[0] || p[7] != w.flags[1]) return fail(w, XZ_E_CORRUPT);
            w.end = at;
            if (!w.end) {
                w.done = true;
                w.want_len = 0;
                return;
            }
            w.stage = S_TAIL;
        }
    }
}

}  // namespace xzp

int xz_admit(const XzCall &c, XzBatch &b) {
    b.measure = !c.d_out && !c.out_cap;
    b.st.assign(c.n, 0);
    Placement place;
    for (uint64_t i = 0; i < c.n; i++) {
        const uint64_t sl = c.src_len[i], room = b.measure ? 0 : c.out_room[i];
        uint64_t dst = 0;
        b.st[i] = place_item(place, c.src_off[i], sl, c.src_cap, !b.measure && c.out_off ? c.out_off + i : nullptr, room, c.out_cap, &dst);
        c.out_len[i] = 0;
        if (c.streams) c.streams[i] = 0;
        if (c.blocks) c.blocks[i] = 0;
        if (c.unverified) c.unverified[i] = 0;
        if (b.st[i] || !sl) continue;  // (no byte, no stream at all: nothing)
        XzItem it;
        it.src = c.d_src + c.src_off[i];
        it.dst = b.measure ? nullptr : c.d_out + dst;
        it.src_len = (uint32_t)sl;
        it.room = (uint32_t)room;
        b.items.push_back(it);
        b.item_of.push_back((uint32_t)i);
        b.walks.emplace_back();
        xzp::start(b.walks.back(), sl);
    }
    return XZ_OK;
}

uint64_t xz_wants(XzBatch &b) {
    b.ranges.clear();
    uint64_t at = 0;
    for (size_t k = 0; k < b.walks.size(); k++) {
        const xzp::Walk &w = b.walks[k];
        if (w.done) continue;
        if (w.want_head) {  // (in front of the item's other range: xz_give hands it over first)
            b.ranges.push_back(XzRange{(uint32_t)k, 0, 12, 1, at});
            at += 16;
        }
        b.ranges.push_back(XzRange{(uint32_t)k, (uint32_t)w.want_off, (uint32_t)w.want_len, 0, at});
        at += (w.want_len + 15) & ~15ull;
    }
    return at;
}

void xz_give(XzBatch &b) {
    for (const XzRange &r : b.ranges) {
        if (r.head) xzp::give_head(b.walks[r.item], b.stage.data() + r.at);
        else xzp::give(b.walks[r.item], b.stage.data() + r.at);
    }
}

int xz_plan_jobs(const XzCall &c, XzBatch &b) {
    b.jobs.clear();
    b.first_job.assign(b.walks.size() + 1, 0);
    for (size_t k = 0; k < b.walks.size(); k++) {
        b.first_job[k] = b.jobs.size();
        const uint32_t i = b.item_of[k];
        const xzp::Walk &w = b.walks[k];
        if (!w.done) b.st[i] = XZ_E_CORRUPT;  // (every walk is done when the rounds end)
        else if (w.status) b.st[i] = w.status;
        else if (w.too_big) b.st[i] = XZ_E_UNSUPPORTED;
        else if (!b.measure && w.content > b.items[k].room) b.st[i] = XZ_E_DST_SMALL;
        if (b.st[i] || b.measure) continue;
        uint64_t out = 0;
        for (size_t s = w.streams.size(); s-- > 0;) {
            const xzp::Stream &S = w.streams[s];
            uint64_t pos = S.hdr_pos + 12;
            for (size_t r = 0; r < S.n; r++) {
                const xzp::Block &B = w.blocks[S.first + r];
                if (b.jobs.size() >= XZ_JOBS_MAX) return XZ_E_NOMEM;
                b.jobs.push_back(XzJob{(uint32_t)k, (uint32_t)pos, (uint32_t)B.unpadded, S.check, (uint32_t)out, (uint32_t)B.uncomp});
                pos += (B.unpadded + 3) & ~3ull;
                out += B.uncomp;
            }
        }
    }
    b.first_job[b.walks.size()] = b.jobs.size();
    return XZ_OK;
}

void xz_verdict(const XzCall &c, XzBatch &b) {
    for (size_t k = 0; k < b.walks.size(); k++) {
        const uint32_t i = b.item_of[k];
        if (b.st[i]) continue;
        const xzp::Walk &w = b.walks[k];
        uint32_t n_blocks = 0, unverified = 0;
        for (const xzp::Stream &S : w.streams) {
            n_blocks += (uint32_t)S.n;
            if (S.check != 1 && S.check != 4) unverified += (uint32_t)S.n;
        }
        int32_t status = 0;
        bool sum_bad = false;
        if (!b.measure) {
            for (size_t j = b.first_job[k]; j < b.first_job[k + 1] && !status; j++) {
                const XzJob &J = b.jobs[j];
                const XzRec &r = b.recs[j];
                const uint32_t cs = xzp::check_size(J.check);
                if (r.status) {
                    status = r.status == XZ_E_UNSUPPORTED ? XZ_E_UNSUPPORTED : XZ_E_CORRUPT;
                } else if (r.hdr_size < 8 || r.hdr_size > 1024 || (r.hdr_size & 3) || (uint64_t)r.hdr_size + cs > J.unpadded ||
                           r.comp != J.unpadded - r.hdr_size - cs || r.produced != J.out_len) {
                    status = XZ_E_CORRUPT;  // a record that contradicts the index
                } else if ((r.hdr_comp != XZ_ABSENT && r.hdr_comp != r.comp) || (r.hdr_uncomp != XZ_ABSENT && r.hdr_uncomp != J.out_len)) {
                    status = XZ_E_CORRUPT;  // the block header names other sizes than the index
                } else if (J.check == 1) {
                    sum_bad |= (uint32_t)b.sums[j] != r.check_lo;
                } else if (J.check == 4) {
                    sum_bad |= b.sums[j] != ((uint64_t)r.check_hi << 32 | r.check_lo);
                }
            }
        }
        b.st[i] = status ? status : sum_bad ? XZ_E_CHECKSUM : XZ_OK;
        if (b.st[i]) continue;
        c.out_len[i] = w.content;
        if (c.streams) c.streams[i] = (uint32_t)w.streams.size();
        if (c.blocks) c.blocks[i] = n_blocks;
        if (c.unverified) c.unverified[i] = unverified;
    }
}

}  // namespace zn
