// The compiled host layer's read-side decisions (read_plan.h).  Every column value is untrusted: sums that may wrap are either
// checked or wrap harmlessly into a request the device library's own checks (znippy_rows_set_blob_cap, rows_validate) refuse.
#include "read_plan.h"

#include <algorithm>
#include <cstring>
#include <unordered_set>

namespace zn {

size_t RowTable::add(uint64_t file_pos, uint64_t blob_size, uint64_t len, bool compressed, const uint8_t *checksum32) {
    const size_t k = bo.size();
    bo.push_back(sum); bs.push_back(blob_size); us.push_back(len); fpos.push_back(file_pos);
    if ((k & 7) == 0) bitmap.push_back(0);
    if (compressed) bitmap[k >> 3] |= (uint8_t)(1u << (k & 7));
    if (checksum32) ck.insert(ck.end(), checksum32, checksum32 + 32);
    sum += blob_size;
    return k;
}

RowTable RowTable::subset(const std::vector<size_t> &list) const {
    RowTable s;
    for (size_t k : list) s.bo[s.add(fpos[k], bs[k], us[k], comp(k), ck.empty() ? nullptr : &ck[32 * k])] = bo[k];
    s.sum = sum;
    return s;
}

std::vector<SlabRead> RowTable::reads() const {
    std::vector<SlabRead> out;
    for (size_t k = 0; k < n(); k++)
        if (bs[k]) out.push_back(SlabRead{fpos[k], bo[k], bs[k]});
    return out;
}

RowsRead plan_rows_read(const IndexView &v, const uint64_t *row_ids, size_t n, bool verify) {
    RowsRead p;
    p.out_off.assign(n, 0);
    uint64_t lo = UINT64_MAX, hi = 0;
    for (size_t k = 0; k < n; k++) {
        const uint64_t r = row_ids[k], len = v.row_len(r);
        if (p.total + len < p.total) { p.rc = RDP_E_CORRUPT; p.err = "row sizes overflow"; return p; }
        if (!v.blob_in_file(r)) { p.rc = RDP_E_CORRUPT; p.err = "blob range outside the archive"; return p; }
        p.t.add(v.blob_offset[r], v.blob_size[r], len, v.compressed[r] != 0, verify ? v.ck(r) : nullptr);
        p.out_off[k] = p.total;
        p.total += len;
        lo = std::min(lo, v.blob_offset[r]);
        hi = std::max(hi, v.blob_offset[r] + v.blob_size[r]);
    }
    if (!n) return p;
    // Rows of one batch lie side by side in the archive and one read of the span [lo, hi) between the first and the last blob is
    // the cheapest way to get them, gaps of other rows' bytes included.  Scattered rows (a file's chunks among other files', the
    // two entries of a duplicate path) are packed instead, one read each, once the span is more than twice their bytes + 1 MiB.
    if (hi - lo > 2 * p.t.sum + (1u << 20)) {
        p.nblob = p.t.sum;
        p.reads = p.t.reads();
    } else {
        p.t.bo = p.t.fpos;
        p.base = lo;
        p.nblob = hi - lo;
        if (p.nblob) p.reads.push_back(SlabRead{lo, 0, p.nblob});
    }
    return p;
}

int32_t map_range(const IndexView &v, const uint64_t *rows, size_t n_rows, uint64_t off, uint64_t len, std::vector<RangeHit> *hits, uint64_t *covered) {
    const uint64_t end = off + len < off ? UINT64_MAX : off + len;
    hits->clear();
    *covered = 0;
    for (size_t i = 0; i < n_rows; i++) {
        const uint64_t r = rows[i], lo = v.fdata_offset[r];
        const uint64_t x = std::max(off, lo), y = std::min(end, lo + v.row_len(r));  // (a chunk whose end wraps 2^64 is touched by nothing)
        if (x >= y) continue;
        if (!v.blob_in_file(r)) return RDP_E_CORRUPT;
        hits->push_back(RangeHit{r, x - lo, y - x});
        *covered += y - x;
    }
    return RDP_OK;
}

RangeRead plan_range_read(const IndexView &v, const uint64_t *rows, size_t n_rows, uint64_t off, uint64_t len, bool verify) {
    RangeRead p;
    std::vector<RangeHit> hits;
    uint64_t covered = 0;
    p.rc = map_range(v, rows, n_rows, off, len, &hits, &covered);
    if (p.rc) return p;
    for (const RangeHit &h : hits) {
        // chunks that overlap (the two entries of a duplicate path both begin at 0) cover more than was asked for: the caller's
        // buffer has room for len bytes, so what the chunks in front have left of them is all a chunk gives
        const uint64_t take = std::min(h.len, len - p.total);
        if (!take) break;
        p.rg.add(p.t.add(v.blob_offset[h.row], v.blob_size[h.row], v.row_len(h.row), v.compressed[h.row] != 0, verify ? v.ck(h.row) : nullptr), h.begin, take);
        p.arow.push_back(h.row);
        p.total += take;
    }
    return p;
}

FileRangesRead plan_file_ranges(const IndexView &v, const std::vector<FileRange> &req) {
    FileRangesRead p;
    p.at.assign(req.size(), 0);
    p.st.assign(req.size(), 0);
    std::unordered_map<uint64_t, uint64_t> row_at;  // compressed archive row -> table row
    std::vector<RangeHit> hits;
    for (size_t i = 0; i < req.size(); i++) {
        p.at[i] = p.total;
        uint64_t covered = 0;
        if (map_range(v, req[i].rows->data(), req[i].rows->size(), req[i].off, req[i].len, &hits, &covered) || covered != req[i].len) {
            p.st[i] = RDP_E_CORRUPT;  // a blob outside the archive, or the index does not cover the file: nothing of it is read
            continue;
        }
        for (const RangeHit &h : hits) {
            const uint64_t r = h.row;
            if (!v.compressed[r]) {
                p.rg.add(p.t.add(v.blob_offset[r] + h.begin, h.len, h.len, false, nullptr), 0, h.len);
            } else {
                auto it = row_at.find(r);
                if (it == row_at.end()) it = row_at.emplace(r, p.t.add(v.blob_offset[r], v.blob_size[r], v.row_len(r), true, nullptr)).first;
                p.rg.add(it->second, h.begin, h.len);
            }
            p.of_req.push_back(i);
        }
        p.total += req[i].len;
    }
    return p;
}

std::pair<uint64_t, uint64_t> split_rows(const uint64_t *w, uint64_t n, uint32_t rank, uint32_t world) {
    if (world <= 1) return {0, n};
    std::vector<long double> c(n);
    long double acc = 0;
    for (uint64_t i = 0; i < n; i++) { acc += (long double)std::max<uint64_t>(w[i], 1); c[i] = acc; }
    // cut r: the first row at which the running weight reaches r / world of the whole (cut 0 = 0, cut world = n; monotone in r)
    const auto cut = [&](uint64_t r) -> uint64_t {
        if (r == 0) return 0;
        if (r >= world) return n;
        return (uint64_t)(std::lower_bound(c.begin(), c.end(), acc * r / world) - c.begin());
    };
    return {cut(rank), cut((uint64_t)rank + 1)};
}

FirstTouch read_plan_first_touch(const IndexView &v, uint64_t begin, uint64_t end, bool per_rank) {
    FirstTouch f;
    f.first.assign(v.n, 0);
    std::unordered_set<std::string> uniq;
    uniq.reserve(v.n * 2);
    for (uint64_t r = 0; r < v.n; r++) {
        if (r && v.path[r] == v.path[r - 1]) continue;
        if (uniq.insert(v.path[r]).second) f.first[r] = 1;
        else f.adjacent = false;
    }
    f.n_unique = uniq.size();
    if (!per_rank) return f;
    std::fill(f.first.begin(), f.first.end(), 0);
    uniq.clear();
    for (uint64_t r = begin; r < end; r++) {
        if (r > begin && v.path[r] == v.path[r - 1]) continue;
        if (uniq.insert(v.path[r]).second) f.first[r] = 1;
    }
    f.final_size.reserve(f.n_unique * 2);
    for (uint64_t r = 0; r < v.n; r++) {
        uint64_t &fs = f.final_size[v.path[r]];
        fs = std::max(fs, v.fdata_offset[r] + v.row_len(r));
    }
    return f;
}

uint64_t cut_batch(const IndexView &v, uint64_t i, uint64_t end, uint64_t batch_bytes, bool verify_only) {
    const auto row_cost = [&](uint64_t r) { return verify_only ? v.blob_size[r] + (v.compressed[r] ? v.usize[r] : 0) : v.usize[r]; };
    uint64_t j = i, nbytes = 0;
    while (j < end && (j == i || nbytes + row_cost(j) <= batch_bytes)) nbytes += row_cost(j++);
    return j;
}

std::vector<std::pair<uint64_t, uint64_t>> cut_writers(const uint64_t *out_off, uint64_t total, const std::string *paths, uint64_t i, uint64_t n, unsigned n_writers) {
    std::vector<std::pair<uint64_t, uint64_t>> parts;
    uint64_t k0 = 0;
    for (unsigned w = 0; w < n_writers && k0 < n; w++) {
        uint64_t k1 = n;
        if (w + 1 < n_writers) {
            const uint64_t target = total / n_writers * (w + 1);
            k1 = (uint64_t)(std::lower_bound(out_off + k0, out_off + n, target) - out_off);
            k1 = std::max(k1, k0 + 1);
            while (k1 < n && paths[i + k1] == paths[i + k1 - 1]) k1++;
        }
        parts.emplace_back(k0, k1);
        k0 = k1;
    }
    return parts;
}

bool sidecar_layout(const uint8_t *raw, uint64_t size, const IndexView &v, std::vector<uint64_t> *first) {
    if (size < B3T_HEADER || (size - B3T_HEADER) % 32 != 0) return false;  // (before any header field is read)
    uint32_t log = 0, zero = 0;
    uint64_t n_rows = 0, n_entries = 0;
    std::memcpy(&log, raw + 8, 4);
    std::memcpy(&zero, raw + 12, 4);
    std::memcpy(&n_rows, raw + 16, 8);
    std::memcpy(&n_entries, raw + 24, 8);
    if (std::memcmp(raw, B3T_MAGIC, 8) != 0 || log != B3T_BLOCK_LOG || zero != 0 || n_rows != v.n || n_entries != (size - B3T_HEADER) / 32) return false;
    first->assign(v.n + 1, 0);
    for (uint64_t r = 0; r < v.n; r++) (*first)[r + 1] = (*first)[r] + v.tree_entries(r);
    return first->back() == n_entries;
}

size_t take_tree(const uint8_t *packed, size_t at, uint64_t entries, std::vector<uint8_t> *dst) {
    const size_t nb = 32 * (size_t)entries;
    dst->insert(dst->end(), packed + at, packed + at + nb);
    return at + nb;
}

}  // namespace zn
