"""The host's plan of a range read and of a block-tree build (znippy_amd/csrc/host/range_plan.cc) as a stand-alone host program
under AddressSanitizer and UBSan.  The program reads a table and calls from stdin, runs every planner function in the order
api.hip does — with made-up device addresses, and with verdicts of the device passes that follow a fixed rule — and prints what
they planned; `Model` below restates the rules of include/znippy_hip.h (znippy_rows_read_ranges, _read_ranges_verified,
_block_tree_build) in plain Python and prints the same, and the two are compared field by field.  The slab functions get a heap
buffer of exactly range_slab_layout bytes, so a write outside it is the sanitizer's to find.

Long lists are printed as a count and a position-weighted sum (CHK below); up to `full` values are printed in full as well.

The item limit (0x7FFFFFF0 blocks in one launch) needs 2 GiB of need bitmaps to reach — 65,536 rows just under 4 GiB with
32,768 blocks each — so that case runs a second build of the program whose limit is overridden at compile time
(-DZN_RR_ITEMS_MAX=40)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "znippy_amd", "csrc", "host")

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include "range_plan.h"
using namespace zn;

static size_t g_full = 64;
static std::string word() { char b[64]; if (scanf("%63s", b) != 1) return ""; return b; }
static uint64_t num() { const std::string w = word(); if (w.empty()) { printf("short input\n"); exit(2); } return strtoull(w.c_str(), nullptr, 0); }
template <class V, class F>
static void emit(const char *name, const V &v, size_t n, F get) {
    uint64_t chk = 0;
    for (size_t i = 0; i < n; i++) chk += (uint64_t)(i + 1) * (uint64_t)get(v[i]) + 1;
    printf("%s %zu %" PRIu64, name, n, chk);
    if (n <= g_full) for (size_t i = 0; i < n; i++) printf(" %" PRIu64, (uint64_t)get(v[i]));
    printf("\n");
}
template <class V> static void emit(const char *name, const V &v, size_t n) { emit(name, v, n, [](auto x) { return (uint64_t)x; }); }

static uint8_t *const POOL0 = (uint8_t *)0x700000000000ull, *const POOL1 = (uint8_t *)0x710000000000ull;
static uint8_t *const BLOBS = (uint8_t *)0x720000000000ull, *const OUT = (uint8_t *)0x730000000000ull;

struct Table {
    std::vector<uint64_t> bo, bs, len, first;
    std::vector<uint8_t> comp, accept;
    RrTable view{};
};

static void read_table(Table &t) {
    const uint32_t n = (uint32_t)num();
    const uint64_t row_begin = num(), blob_cap = num();
    const size_t n_accept = (size_t)num();
    t.bo.resize(n); t.bs.resize(n); t.len.resize(n); t.comp.resize(n); t.accept.resize(n_accept);
    for (uint32_t i = 0; i < n; i++) { t.bo[i] = num(); t.bs[i] = num(); t.len[i] = num(); t.comp[i] = (uint8_t)num(); }
    for (size_t i = 0; i < n_accept; i++) t.accept[i] = (uint8_t)num();
    t.first.assign((size_t)n + 1, 0);
    for (uint32_t i = 0; i < n; i++) t.first[i + 1] = t.first[i] + tree_entries_of(t.len[i]);
    t.view = RrTable{n, row_begin, blob_cap, t.bo.data(), t.bs.data(), t.len.data(), t.comp.data(), t.first.data(), t.first.size(), t.accept.data(), t.accept.size()};
    emit("tree_first", t.first, t.first.size());
}

static void rows_out(const char *tag, const RangePlan &p) {
    for (size_t i = 0; i < p.rows.size(); i++) {
        const RrRow &w = p.rows[i];
        uint64_t need = 0, bad = 0;
        for (size_t k = 0; k < w.need.size(); k++) need += (k + 1) * w.need[k];
        for (size_t k = 0; k < w.bad.size(); k++) bad += (k + 1) * w.bad[k];
        printf("%s %zu row %u comp %d partial %d sblocks %d late %d pool %d status %d hashed %d kmin %u kmax %u slot %" PRIu64 " first %" PRIu64 " need %zu %" PRIu64 " bad %zu %" PRIu64 "\n",
               tag, i, w.row, w.comp, w.partial, w.sblocks, w.late, w.pool, w.status, w.hashed, w.kmin, w.kmax, w.slot, w.first, w.need.size(), need, w.bad.size(), bad);
    }
}

// C verified blob_base out_cap has_out out_skew late_mode fail_mode bad_mode n_ranges, then per range: row begin len [out]
static void call(const Table &t) {
    const bool verified = num() != 0;
    const uint64_t blob_base = num(), out_cap = num();
    const bool has_out = num() != 0;
    const uint64_t out_skew = num(), late_mode = num(), fail_mode = num(), bad_mode = num(), n = num();
    std::vector<uint64_t> row(n), begin(n), len(n), out(n);
    for (uint64_t i = 0; i < n; i++) { row[i] = num(); begin[i] = num(); len[i] = num(); if (has_out) out[i] = num(); }
    const RrCall c{row.data(), begin.data(), len.data(), has_out ? out.data() : nullptr, n, out_cap, blob_base, verified};
    RangePlan p;
    int rc = range_plan_build(t.view, c, p);
    printf("build %d\n", rc);
    if (rc) return;
    emit("st0", p.st, p.st.size(), [](int32_t x) { return (uint64_t)(int64_t)x; });
    emit("dst", p.dst, p.dst.size());
    emit("of_row", p.of_row, p.of_row.size());
    rows_out("w", p);
    emit("part", p.part, p.part.size()); emit("whole", p.whole, p.whole.size()); emit("stored_whole", p.stored_whole, p.stored_whole.size());
    printf("n_items %" PRIu64 " n_todo %" PRIu64 " need0 %" PRIu64 "\n", p.n_items, p.n_todo, p.need0);

    const size_t m = p.part.size();
    uint64_t dec_blocks = 0;
    std::vector<uint8_t> late_flags(m, 0);
    if (m) {
        size_t up = 0;
        const size_t total = range_slab_layout(p, &up);
        std::unique_ptr<uint8_t[]> buf(new uint8_t[total]);  // exactly the layout: a write outside it is the sanitizer's
        uint8_t *base = buf.get();
        memset(base, 0xEE, total);
        RangeSlab h, d;
        range_slab_bind(base, p, h);
        range_slab_bind(POOL1 + 4096, p, d);  // (any address: the device side of the slab is only pointed into)
        range_slab_fill(t.view, p, base);
        printf("layout %zu %zu\n", total, up);
#define COL(f, cnt) do { printf("at %zu %zu ", (size_t)((uint8_t *)h.f - base), (size_t)((uint8_t *)d.f - (POOL1 + 4096))); emit(#f, h.f, cnt); } while (0)
        COL(blob_off, m); COL(blob_size, m); COL(usize, m); COL(out_off, m); COL(block_bytes, m);
        COL(cand_row, m); COL(cand_base, m); COL(cand_nb, m); COL(item_row, p.n_items); COL(item_k, p.n_items); COL(todo, p.n_todo);
        COL(ctl, 4); COL(status, m); COL(comp, m); COL(decoded, 1);
        COL(row_flag, 0); COL(item_src, 0); COL(late, 0);  // written on the device first: where they are, not what is in them
#undef COL
        for (size_t i = up; i < total; i++) if (base[i] != 0xEE) { printf("the fill wrote behind the uploaded part\n"); exit(2); }
        // the block pass's verdicts, by rule: which rows it gives up on; the others' needed blocks are decoded
        for (size_t k = 0; k < m; k++) {
            late_flags[k] = late_mode == 1 || (late_mode == 2 && (k & 1)) || (late_mode == 3 && k + 1 == m);
            if (!late_flags[k]) dec_blocks += h.block_bytes[k];
        }
    }
    // the whole-row passes' verdicts, by rule
    auto whole_pass = [&](const std::vector<uint32_t> &sel, bool verify) {
        for (uint32_t i : sel) {
            RrRow &w = p.rows[i];
            w.status = fail_mode && i % 3 == 1 ? (fail_mode == 2 && verify ? RP_E_DIGEST : RP_E_CORRUPT) : 0;
            if (verify) w.hashed = w.status == 0 || w.status == RP_E_DIGEST;  // (a row that decodes is hashed, whatever the digest says)
        }
    };
    whole_pass(p.whole, verified);
    whole_pass(p.stored_whole, true);
    if (m) {
        std::vector<uint32_t> late;
        uint64_t need1 = 0;
        rc = range_plan_late(t.view, p, late_flags.data(), late, need1);
        printf("late %d\n", rc);
        if (rc) return;
        printf("need1 %" PRIu64 "\n", need1);
        emit("late_rows", late, late.size());
        whole_pass(late, verified);
    }
    if (verified) {
        std::vector<BlockCvItem> items;
        std::vector<std::pair<uint32_t, uint32_t>> item_of;
        const uint64_t hashed = range_plan_block_items(t.view, p, POOL0, BLOBS, blob_base, items, item_of);
        printf("hashed %" PRIu64 "\n", hashed);
        emit("bi.src", items, items.size(), [](const BlockCvItem &x) { return (uint64_t)(uintptr_t)x.src; });
        emit("bi.slot", items, items.size(), [](const BlockCvItem &x) { return x.slot; });
        emit("bi.bytes", items, items.size(), [](const BlockCvItem &x) { return (uint64_t)x.bytes; });
        emit("bi.first_chunk", items, items.size(), [](const BlockCvItem &x) { return (uint64_t)x.first_chunk; });
        emit("bi.row", item_of, item_of.size(), [](const std::pair<uint32_t, uint32_t> &x) { return (uint64_t)x.first; });
        emit("bi.k", item_of, item_of.size(), [](const std::pair<uint32_t, uint32_t> &x) { return (uint64_t)x.second; });
        for (size_t j = 0; j < items.size(); j++)
            if (bad_mode && j % 5 == 3) p.rows[item_of[j].first].bad[item_of[j].second] = 1;
    }
    const uint8_t *const pools[2] = {POOL0, POOL1};
    std::vector<RangePiece> pieces;
    range_plan_pieces(t.view, c, p, pools, BLOBS, OUT + out_skew, pieces);
    rows_out("v", p);
    emit("st", p.st, p.st.size(), [](int32_t x) { return (uint64_t)(int64_t)x; });
    emit("pc.src", pieces, pieces.size(), [](const RangePiece &x) { return (uint64_t)(uintptr_t)x.src; });
    emit("pc.dst", pieces, pieces.size(), [](const RangePiece &x) { return (uint64_t)(uintptr_t)x.dst; });
    emit("pc.len", pieces, pieces.size(), [](const RangePiece &x) { return (uint64_t)x.len; });
    emit("pc.pad", pieces, pieces.size(), [](const RangePiece &x) { return (uint64_t)x.pad; });
    printf("decoded %" PRIu64 "\n", range_plan_decoded(t.view, p, dec_blocks));
}

// B blob_base fail_mode
static void tree_build(const Table &t) {
    const uint64_t blob_base = num(), fail_mode = num();
    std::vector<int32_t> st(t.view.n, 0);
    std::vector<RrRow> rows;
    std::vector<uint32_t> sel;
    uint64_t need0 = 0;
    const int rc = tree_plan_rows(t.view, blob_base, st, rows, sel, need0);
    printf("tree_rows %d\n", rc);
    if (rc) return;
    printf("need0 %" PRIu64 "\n", need0);
    emit("tw.row", rows, rows.size(), [](const RrRow &w) { return (uint64_t)w.row; });
    emit("tw.comp", rows, rows.size(), [](const RrRow &w) { return (uint64_t)w.comp; });
    emit("tw.slot", rows, rows.size(), [](const RrRow &w) { return w.slot; });
    emit("sel", sel, sel.size());
    for (size_t j = 0; j < sel.size(); j++) rows[sel[j]].status = fail_mode && (j & 1) ? RP_E_CORRUPT : 0;  // the decode run's verdicts, by rule
    std::vector<uint32_t> good;
    std::vector<BlockCvItem> items;
    tree_plan_items(t.view, rows, POOL0, BLOBS, blob_base, st, good, items);
    emit("good", good, good.size());
    emit("tst", st, st.size(), [](int32_t x) { return (uint64_t)(int64_t)x; });
    emit("ti.src", items, items.size(), [](const BlockCvItem &x) { return (uint64_t)(uintptr_t)x.src; });
    emit("ti.slot", items, items.size(), [](const BlockCvItem &x) { return x.slot; });
    emit("ti.bytes", items, items.size(), [](const BlockCvItem &x) { return (uint64_t)x.bytes; });
    emit("ti.first_chunk", items, items.size(), [](const BlockCvItem &x) { return (uint64_t)x.first_chunk; });
}

int main() {
    Table t;
    for (std::string w = word(); !w.empty(); w = word()) {
        printf("# %s\n", w.c_str());
        if (w == "F") g_full = (size_t)num();
        else if (w == "T") read_table(t);
        else if (w == "C") call(t);
        else if (w == "B") tree_build(t);
        else if (w == "S") {  // the slot rule alone: need front bytes
            uint64_t need = num(), slot = 0;
            const uint64_t front = num(), bytes = num();
            const bool ok = rr_slot_take(need, front, bytes, slot);
            if (ok) printf("slot 1 %" PRIu64 " %" PRIu64 "\n", need, slot); else printf("slot 0\n");
        } else if (w == "E") printf("entries %" PRIu64 " by_blocks %d\n", tree_entries_of(num()), (int)rr_by_blocks(num()));
        else { printf("bad command\n"); return 2; }
    }
    printf("limits %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", RR_BLK, RR_GUARD, RR_SCRATCH_MAX, RR_ITEMS_MAX, RANGE_PIECE);
    return 0;
}
"""

M64 = (1 << 64) - 1
BLK = 128 * 1024
GUARD = 8192
SCRATCH_MAX = 32 << 30
ITEMS_MAX = 0x7FFFFFF0
PIECE = 32 << 10
NONE = 0xFFFFFFFF
E_INVAL, E_NOMEM, E_DST_SMALL, E_CORRUPT, E_DIGEST = -1, -3, -4, -5, -8   # znippy_hip.h
POOL0, POOL1, BLOBS, OUT = 0x7000_0000_0000, 0x7100_0000_0000, 0x7200_0000_0000, 0x7300_0000_0000
LENGTHS = [0, 1, 131_072, 131_073, 262_144, 262_145, 300_001, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 5]


def chk(vals):
    """sum((i + 1) * v + 1) modulo 2^64 over the list."""
    a = np.array([v & M64 for v in vals], dtype=np.uint64) if not isinstance(vals, np.ndarray) else vals.astype(np.uint64)
    if not len(a):
        return 0
    with np.errstate(over="ignore"):
        return int((np.arange(1, len(a) + 1, dtype=np.uint64) * a + np.uint64(1)).sum(dtype=np.uint64))


def weighted(bits):
    return int((np.arange(1, len(bits) + 1, dtype=np.uint64) * bits.astype(np.uint64)).sum()) if len(bits) else 0


class Table:
    """Rows laid back to back behind `base`: a compressed row's blob is a third of it and a few bytes, a stored row IS its blob."""

    def __init__(self, rows, row_begin=0, blob_cap=M64, accept=None, base=0, blob_off=None):
        self.len = [n for n, _ in rows]
        self.comp = [int(c) for _, c in rows]
        self.bs = [n // 3 + 20 if c else n for n, c in rows]
        self.bo, at = [], base
        for s in self.bs:
            self.bo.append(at)
            at += s
        if blob_off:
            for i, v in blob_off.items():
                self.bo[i] = v
        self.end = at
        self.row_begin, self.blob_cap = row_begin, blob_cap
        self.accept = [] if accept is None else list(accept)
        self.n = len(rows)
        self.first = [0]
        for n in self.len:   # znippy_rows_block_tree_layout: one entry per block of a row of more than one block and below 4 GiB
            self.first.append(self.first[-1] + (-(-n // BLK) if BLK < n < 2**32 else 0))

    def text(self):
        out = [f"T {self.n} {self.row_begin} {self.blob_cap} {len(self.accept)}"]
        out += [f"{self.bo[i]} {self.bs[i]} {self.len[i]} {self.comp[i]}" for i in range(self.n)]
        out.append(" ".join(str(a) for a in self.accept))
        return "\n".join(out)

    def blob_ok(self, i, blob_base):
        bo, bs = self.bo[i], self.bs[i]
        return bo >= blob_base and (self.blob_cap == M64 or bo - blob_base + bs <= self.blob_cap)


class Lines:
    def __init__(self, full):
        self.out, self.full = [], full

    def emit(self, name, vals, front=""):
        vals = list(vals) if not isinstance(vals, np.ndarray) else vals
        s = f"{front}{name} {len(vals)} {chk(vals)}"
        if len(vals) <= self.full:
            s += "".join(f" {int(v) & M64}" for v in vals)
        self.out.append(s)


class Row:
    def __init__(self, row, comp):
        self.row, self.comp = row, comp
        self.partial = self.sblocks = self.late = self.hashed = False
        self.pool = self.status = self.slot = self.first = 0
        self.kmin, self.kmax = NONE, 0
        self.need = np.zeros(0, np.uint8)
        self.bad = np.zeros(0, np.uint8)

    def text(self, tag, i):
        return (f"{tag} {i} row {self.row} comp {int(self.comp)} partial {int(self.partial)} sblocks {int(self.sblocks)} late {int(self.late)} pool {self.pool} "
                f"status {self.status} hashed {int(self.hashed)} kmin {self.kmin} kmax {self.kmax} slot {self.slot} first {self.first} "
                f"need {len(self.need)} {weighted(self.need)} bad {len(self.bad)} {weighted(self.bad)}")


def slot_take(need, front, nbytes):
    """A slot of a scratch pool: 256-aligned, `front` guard bytes, the content, 256 spare; a pool stops at 32 GiB.  -> (need, slot) or None."""
    slot = -(-need // 256) * 256 + front
    need = slot + nbytes + 256
    return (need, slot) if need <= SCRATCH_MAX else None


def align16(at):
    return (at + 15) & ~15


def model_call(t, verified=0, blob_base=0, out_cap=1 << 24, out=None, skew=0, late_mode=0, fail_mode=0, bad_mode=0, ranges=(), full=64, items_max=ITEMS_MAX, what=None):
    """What a call plans, from the header's rules; `ranges` = [(row, begin, len)], out = offsets or None (packed)."""
    L = Lines(full)
    n = len(ranges)
    st, dst, of_row, rows, at_row = [0] * n, [0] * n, [NONE] * n, [], {}
    packed, wrapped = 0, False
    for i, (row, begin, ln) in enumerate(ranges):
        known = out is not None or not wrapped
        dst[i] = out[i] if out is not None else packed & M64
        if out is None:
            packed += ln
            wrapped |= packed > M64    # every range behind a wrap of the packed sum has no destination
        ri = row - t.row_begin
        if not 0 <= ri < t.n or begin + ln > t.len[ri]:
            st[i] = E_INVAL
        elif not known or dst[i] + ln > out_cap:
            st[i] = E_DST_SMALL
        elif not t.blob_ok(ri, blob_base):
            st[i] = E_CORRUPT
        elif ln:
            if ri not in at_row:
                at_row[ri] = len(rows)
                w = Row(ri, bool(t.comp[ri]))
                # block by block: more than one block, below 2^32 - 1, and (verified) entries that were accepted
                by_blocks = BLK < t.len[ri] < 0xFFFFFFFF and (not verified or (ri < len(t.accept) and t.accept[ri]))
                w.partial = w.comp and by_blocks
                w.sblocks = bool(verified) and not w.comp and by_blocks
                if w.partial or w.sblocks:
                    w.need = np.zeros(-(-t.len[ri] // BLK), np.uint8)
                rows.append(w)
            of_row[i] = at_row[ri]
            w = rows[at_row[ri]]
            if w.partial or w.sblocks:
                k0, k1 = begin // BLK, (begin + ln - 1) // BLK
                w.need[k0:k1 + 1] = 1
                w.kmin, w.kmax = min(w.kmin, k0), max(w.kmax, k1)
    part, whole, stored_whole = [], [], []
    n_items = n_todo = need0 = 0
    nomem = False
    for i, w in enumerate(rows):
        if not w.comp:
            if verified and not w.sblocks:
                stored_whole.append(i)
            continue
        if w.partial and n_items + len(w.need) >= items_max:
            w.partial = False
        if w.partial:
            part.append(i)
            n_items += len(w.need)
            n_todo += int(w.need.sum())
            w.first = w.kmin * BLK
            got = slot_take(need0, GUARD, min(t.len[w.row], (w.kmax + 1) * BLK) - w.first)
        else:
            whole.append(i)
            got = slot_take(need0, 0, t.len[w.row])
        if got is None:
            nomem = True
            break
        need0, w.slot = got
    L.out.append(f"build {E_NOMEM if nomem else 0}")
    if nomem:
        return L.out
    L.emit("st0", st); L.emit("dst", dst); L.emit("of_row", of_row)
    L.out += [w.text("w", i) for i, w in enumerate(rows)]
    L.emit("part", part); L.emit("whole", whole); L.emit("stored_whole", stored_whole)
    L.out.append(f"n_items {n_items} n_todo {n_todo} need0 {need0}")

    m = len(part)
    dec_blocks = 0
    late_flags = [0] * m
    if m:
        # the slab: columns one after the other, each on a 16-byte boundary; the uploaded part ends behind `decoded`
        cols = [("blob_off", 8, m), ("blob_size", 8, m), ("usize", 8, m), ("out_off", 8, m), ("block_bytes", 8, m), ("cand_row", 4, m), ("cand_base", 4, m),
                ("cand_nb", 4, m), ("item_row", 4, n_items), ("item_k", 4, n_items), ("todo", 4, n_todo), ("ctl", 4, 4), ("status", 4, m), ("comp", 1, m),
                ("decoded", 8, 1), ("row_flag", 4, m), ("item_src", 4, n_items), ("late", 1, m)]
        at, where, up = 0, {}, 0
        for name, size, cnt in cols:
            at = align16(at)
            where[name] = at
            at += size * cnt
            if name == "decoded":
                up = at
        L.out.append(f"layout {at} {up}")
        val = {name: [] for name, _, _ in cols}
        item_row, item_k, todo = [], [], []
        base = 0
        for c, i in enumerate(part):
            w = rows[i]
            ln = t.len[w.row]
            nb = len(w.need)
            ks = np.nonzero(w.need)[0]
            val["blob_off"].append(t.bo[w.row]); val["blob_size"].append(t.bs[w.row]); val["usize"].append(ln)
            val["out_off"].append((w.slot - w.first) & M64)    # block k lands at out_off + k * 128 KiB: the first needed block at the head of the slot
            val["block_bytes"].append(int(sum(min(BLK, ln - int(k) * BLK) for k in ks)))
            val["cand_row"].append(c); val["cand_base"].append(base); val["cand_nb"].append(nb)
            item_row.append(np.full(nb, c, np.uint64)); item_k.append(np.arange(nb, dtype=np.uint64)); todo.append(ks.astype(np.uint64) + np.uint64(base))
            base += nb
        val["item_row"], val["item_k"], val["todo"] = np.concatenate(item_row), np.concatenate(item_k), np.concatenate(todo)
        val["ctl"] = [n_todo, 0, 0, 0]
        val["status"], val["comp"], val["decoded"] = [0] * m, [1] * m, [0]
        for name, _, _ in cols:   # where a column is on the host and on the device side, and (the uploaded ones) what is in it
            L.emit(name, val[name], f"at {where[name]} {where[name]} ")
        for k in range(m):
            late_flags[k] = int(late_mode == 1 or (late_mode == 2 and k & 1) or (late_mode == 3 and k + 1 == m))
            if not late_flags[k]:
                dec_blocks += val["block_bytes"][k]

    def whole_pass(sel, verify):   # the rule the program stands in for the device passes with
        for i in sel:
            w = rows[i]
            w.status = ((E_DIGEST if fail_mode == 2 and verify else E_CORRUPT) if fail_mode and i % 3 == 1 else 0)
            if verify:
                w.hashed = w.status in (0, E_DIGEST)
    whole_pass(whole, verified)
    whole_pass(stored_whole, True)
    if m:
        late, need1 = [], 0
        for c, i in enumerate(part):
            if not late_flags[c]:
                continue
            w = rows[i]
            w.late, w.pool, w.first = True, 1, 0
            got = slot_take(need1, 0, t.len[w.row])
            if got is None:
                L.out.append(f"late {E_NOMEM}")
                return L.out
            need1, w.slot = got
            late.append(i)
        L.out += ["late 0", f"need1 {need1}"]
        L.emit("late_rows", late)
        whole_pass(late, verified)
    if verified:
        hashed = 0
        src, slot, nbytes, chunk, irow, ik = [], [], [], [], [], []
        for i, w in enumerate(rows):
            ln = t.len[w.row]
            if w.hashed:
                hashed += ln
            if not ((w.partial and not w.late) or w.sblocks) or w.status:
                continue
            w.bad = np.zeros(len(w.need), np.uint8)
            for k in (int(k) for k in np.nonzero(w.need)[0]):
                src.append(POOL0 + w.slot + k * BLK - w.first if w.comp else BLOBS + t.bo[w.row] - blob_base + k * BLK)
                slot.append(t.first[w.row] + k); nbytes.append(min(BLK, ln - k * BLK)); chunk.append(128 * k); irow.append(i); ik.append(k)
                hashed += nbytes[-1]
        L.out.append(f"hashed {hashed}")
        for name, v in (("bi.src", src), ("bi.slot", slot), ("bi.bytes", nbytes), ("bi.first_chunk", chunk), ("bi.row", irow), ("bi.k", ik)):
            L.emit(name, v)
        for j in range(len(src)):
            if bad_mode and j % 5 == 3:
                rows[irow[j]].bad[ik[j]] = 1
    psrc, pdst, plen = [], [], []
    for i, (row, begin, ln) in enumerate(ranges):
        if of_row[i] == NONE:
            continue
        w = rows[of_row[i]]
        if w.status:
            st[i] = w.status
            continue
        if len(w.bad) and w.bad[begin // BLK:(begin + ln - 1) // BLK + 1].any():
            st[i] = E_DIGEST
            continue
        s = (POOL0, POOL1)[w.pool] + w.slot + begin - w.first if w.comp else BLOBS + t.bo[w.row] - blob_base + begin
        d = OUT + skew + dst[i]
        step = min(ln, PIECE - d % 128)     # from the second piece on, a destination starts on a 128-byte line
        while ln:
            psrc.append(s); pdst.append(d); plen.append(step)
            s, d, ln = s + step, d + step, ln - step
            step = min(ln, PIECE)
    L.out += [w.text("v", i) for i, w in enumerate(rows)]
    L.emit("st", st)
    L.emit("pc.src", psrc); L.emit("pc.dst", pdst); L.emit("pc.len", plen); L.emit("pc.pad", [0] * len(plen))
    dec = dec_blocks + sum(t.len[w.row] for w in rows if w.comp and (not w.partial or w.late) and w.status in (0, E_DIGEST))
    L.out.append(f"decoded {dec}")
    return L.out


def call_text(verified=0, blob_base=0, out_cap=1 << 24, out=None, skew=0, late_mode=0, fail_mode=0, bad_mode=0, ranges=(), **_):
    head = f"C {int(verified)} {blob_base} {out_cap} {int(out is not None)} {skew} {late_mode} {fail_mode} {bad_mode} {len(ranges)}"
    body = [f"{r} {b} {n}" + (f" {out[i]}" if out is not None else "") for i, (r, b, n) in enumerate(ranges)]
    return "\n".join([head] + body)


def model_tree(t, blob_base=0, fail_mode=0, full=64):
    L = Lines(full)
    st, rows, sel, need0 = [0] * t.n, [], [], 0
    for ri in range(t.n):
        if t.first[ri + 1] == t.first[ri]:
            continue
        if not t.blob_ok(ri, blob_base):
            st[ri] = E_CORRUPT
            continue
        w = Row(ri, bool(t.comp[ri]))
        if w.comp:
            got = slot_take(need0, 0, t.len[ri])
            if got is None:
                return [f"tree_rows {E_NOMEM}"]
            need0, w.slot = got
            sel.append(len(rows))
        rows.append(w)
    L.out += ["tree_rows 0", f"need0 {need0}"]
    L.emit("tw.row", [w.row for w in rows]); L.emit("tw.comp", [int(w.comp) for w in rows]); L.emit("tw.slot", [w.slot for w in rows]); L.emit("sel", sel)
    for j, i in enumerate(sel):
        rows[i].status = E_CORRUPT if fail_mode and j & 1 else 0
    u64 = np.uint64
    good, src, slot, nbytes, chunk = [], [np.zeros(0, u64)], [np.zeros(0, u64)], [np.zeros(0, u64)], [np.zeros(0, u64)]
    for w in rows:
        if w.status:
            st[w.row] = w.status
            continue
        good.append(w.row)
        base = POOL0 + w.slot if w.comp else BLOBS + t.bo[w.row] - blob_base
        k = np.arange(t.first[w.row + 1] - t.first[w.row], dtype=u64)     # every block of the row, the last one ragged
        src.append(u64(base) + k * u64(BLK)); slot.append(u64(t.first[w.row]) + k)
        nbytes.append(np.minimum(u64(BLK), u64(t.len[w.row]) - k * u64(BLK))); chunk.append(u64(128) * k)
    L.emit("good", good); L.emit("tst", st)
    for name, v in (("ti.src", src), ("ti.slot", slot), ("ti.bytes", nbytes), ("ti.first_chunk", chunk)):
        L.emit(name, np.concatenate(v))
    return L.out


def pick(rng, vals):
    return vals[int(rng.integers(len(vals)))]


def build_program(d, name, extra=()):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / name
    # (gcc links the sanitizers' runtimes dynamically unless told otherwise; linked into the program they do not care what else
    # the process loads)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + list(extra) +
                   ["-I", HOST, str(main), os.path.join(HOST, "range_plan.cc"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_program(tmp_path_factory.mktemp("range_plan"), "plan")


def run(exe, text, timeout=120):
    r = subprocess.run([exe], input=text + "\n", capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-3000:])
    return r.stdout.splitlines()


def sections(lines):
    """The program's output cut at its '# X' lines -> [(command, lines)]."""
    out = []
    assert lines[-1].startswith("limits ")     # (the program's last word)
    for ln in lines[:-1]:
        if ln.startswith("# "):
            out.append((ln[2:], []))
        else:
            out[-1][1].append(ln)
    return out


def check(exe, t, calls, trees=(), full=64, items_max=ITEMS_MAX):
    """One table, many calls: the program's plan of each against the model's, line by line."""
    text = [f"F {full}", t.text()] + [call_text(**c) for c in calls] + [f"B {b.get('blob_base', 0)} {b.get('fail_mode', 0)}" for b in trees]
    got = sections(run(exe, "\n".join(text)))
    assert [c for c, _ in got] == ["F", "T"] + ["C"] * len(calls) + ["B"] * len(trees)
    first = Lines(full)
    first.emit("tree_first", t.first)
    assert got[1][1] == first.out
    for k, c in enumerate(calls):
        want = model_call(t, full=full, items_max=items_max, **c)
        have = got[2 + k][1]
        for a, b in zip(have, want):
            assert a == b, (c.get("what", k), "program", a, "model", b)
        assert len(have) == len(want), (c.get("what", k), have[len(want):], want[len(have):])
    for k, b in enumerate(trees):
        want = model_tree(t, full=full, **b)
        have = got[2 + len(calls) + k][1]
        for x, y in zip(have, want):
            assert x == y, ("tree", k, "program", x, "model", y)
        assert len(have) == len(want)
    return got


def field(lines, name):
    """The values of a list the program printed in full."""
    for ln in lines:
        p = ln.split()
        if p[0] == "at":
            p = p[3:]
        if p[0] == name:
            assert len(p) == 3 + int(p[1]), (name, "not printed in full")
            return [int(v) for v in p[3:]]
    raise KeyError(name)


def statuses(lines, name="st"):
    return [v - (1 << 64) if v >> 63 else v for v in field(lines, name)]


def every_table():
    """The lengths, each as a compressed and as a stored row (one table; verified calls see the entries accepted, rejected or missing)."""
    return [(n, c) for n in LENGTHS for c in (1, 0)]


def boundary_ranges(sizes):   # tests/test_gpu_ranges.py, plus what a length of 0 leaves of it
    out = []
    for row, L in enumerate(sizes):
        out += [(row, 0, min(1, L)), (row, 0, min(L, 1 << 20)), (row, max(L, 1) - 1, min(1, L)), (row, L, 0), (row, 0, 0)]
        if L > 1600:
            out += [(row, 10, 1001), (row, 500, 1001)]    # the two overlap
        if L >= 131_073:
            out += [(row, 131_071, 2), (row, 131_072, 1)]
        if L > 141_000:
            out += [(row, 140_000, 777)]                   # inside block 1
        if L >= 262_145:
            out += [(row, 100_000, 262_145 - 100_000)]     # blocks 0-2
        if L > BLK:
            out += [(row, L - 1, 1), (row, (L - 1) // BLK * BLK, 1)]   # the ragged last block only
    return out


def test_constants_and_the_two_boundaries(program):
    lines = run(program, "\n".join(f"E {n} {n}" for n in LENGTHS + [0xFFFFFFFE]))
    got = [ln for ln in lines if not ln.startswith("#")]
    for n, ln in zip(LENGTHS + [0xFFFFFFFE], got):
        assert ln == f"entries {-(-n // BLK) if BLK < n < 2**32 else 0} by_blocks {int(BLK < n < 0xFFFFFFFF)}", n
    assert got[LENGTHS.index(2**32 - 1)] == "entries 32768 by_blocks 0"     # entries, but read whole
    assert got[-1] == f"limits {BLK} {GUARD} {SCRATCH_MAX} {ITEMS_MAX} {PIECE}"


def test_every_length_on_every_route(program):
    rows = every_table()
    sizes = [n for n, _ in rows]
    ranges = boundary_ranges(sizes)
    accept = {"accepted": [1] * len(rows), "rejected": [0] * len(rows), "short": [1] * 7, "alternating": [i & 1 for i in range(len(rows))]}
    calls = [dict(what="unverified", ranges=ranges, out_cap=1 << 26)]
    t = Table(rows)
    check(program, t, calls + [dict(what="verified, no tree", verified=1, ranges=ranges, out_cap=1 << 26)], trees=[{}, dict(fail_mode=1)])
    for name, acc in accept.items():
        t = Table(rows, accept=acc, base=(1 << 40) + 12345)
        for fail in (0, 1, 2):
            check(program, t, [dict(what=(name, fail, late), verified=1, blob_base=(1 << 40) + 12345, ranges=ranges, out_cap=1 << 26, fail_mode=fail, bad_mode=fail, late_mode=late)
                               for late in (0, 1, 2, 3)])
    # a row of 2^32 - 1 bytes has entries and is still read (and, stored, hashed) whole; its neighbour one byte shorter goes by blocks
    t = Table([(2**32 - 1, 1), (2**32 - 1, 0), (2**32 - 2, 1), (2**32 - 2, 0)], accept=[1, 1, 1, 1])
    got = check(program, t, [dict(verified=1, ranges=[(r, 2**32 - 70_000, 5) for r in range(4)])])
    rows_out = [ln.split() for ln in got[2][1] if ln.startswith("w ")]
    assert [(w[7], w[9]) for w in rows_out] == [("0", "0"), ("0", "0"), ("1", "0"), ("0", "1")]     # (partial, sblocks)
    assert t.first == [0, 32768, 65536, 98304, 131072]


def test_validation_cases(program):
    """Every case of test_validation_on_the_host (tests/test_gpu_ranges.py) and the ones the issue adds."""
    t = Table([(300_001, 1), (1000, 0), (9_000, 1)])
    t.blob_cap = t.end - 1                        # the last row's blob ends one byte outside
    good = [(0, 200_000, 777), (1, 10, 99)]
    cap = 4000
    cases = [((3, 0, 1), E_INVAL), ((0, 300_000, 2), E_INVAL), ((0, 5, (1 << 64) - 3), E_INVAL), ((0, 300_002, 0), E_INVAL), ((1, 0, 50), E_DST_SMALL),
             ((2, 0, 10), E_CORRUPT), ((0, 300_001, 0), 0), ((0, 2, M64), E_INVAL), ((0, M64, 2), E_INVAL)]
    calls = []
    for (row, begin, n), code in cases:
        at = cap - 20 if code == E_DST_SMALL else 2000
        calls.append(dict(what=(row, begin, n), ranges=[good[0], (row, begin, n), good[1]], out=[1, at, 1000], out_cap=cap))
    calls.append(dict(what="no bytes at and behind out_cap", ranges=[(1, 1000, 0), (1, 0, 0)], out=[cap, cap + 1], out_cap=cap))
    got = check(program, t, calls)
    for ((_, code), (_, lines)) in zip(cases, got[2:]):
        assert statuses(lines) == [0, code, 0]
        assert "decoded 131072" in lines
    assert statuses(got[-1][1]) == [0, E_DST_SMALL]
    # a table that does not start at row 0; a blob in front of the blob region; an undeclared blob size
    t = Table([(5000, 1), (5000, 0)], row_begin=7, base=1000)
    got = check(program, t, [dict(ranges=[(6, 0, 1), (7, 0, 1), (8, 0, 1), (9, 0, 1), (0, 0, 1)]), dict(blob_base=1001, ranges=[(7, 0, 1), (8, 4999, 1)]),
                             dict(blob_base=1000, ranges=[(7, 0, 1), (8, 4999, 1)])], trees=[dict(blob_base=1001)])
    assert statuses(got[2][1]) == [E_INVAL, 0, 0, E_INVAL, E_INVAL]
    assert statuses(got[3][1]) == [E_CORRUPT, 0] and statuses(got[4][1]) == [0, 0]
    t = Table([(300_001, 1), (300_001, 0)], blob_cap=M64, blob_off={1: 1 << 41})
    assert statuses(check(program, t, [dict(ranges=[(0, 0, 1), (1, 0, 1)])], trees=[{}])[2][1]) == [0, 0]
    t.blob_cap = 1 << 40
    assert statuses(check(program, t, [dict(ranges=[(0, 0, 1), (1, 0, 1)])], trees=[{}])[2][1]) == [0, E_CORRUPT]


def test_packed_destinations_that_wrap(program):
    t = Table([(5000, 1), (1000, 0)])
    # the sum passes 2^64 at the fourth range: whatever comes behind it has no destination, though the wrapped sum would fit — a range with
    # no bytes included; a range that fails an earlier check keeps that verdict
    ranges = [(1, 0, 10), (1, 5, 20), (0, 0, M64 - 40), (0, 0, 41), (1, 0, 1), (1, 0, 0), (5, 0, 1), (0, 9, 100)]
    got = check(program, t, [dict(ranges=ranges, out_cap=1 << 20)])
    assert statuses(got[2][1]) == [0, 0, E_INVAL, E_DST_SMALL, E_DST_SMALL, E_DST_SMALL, E_INVAL, E_DST_SMALL]
    assert field(got[2][1], "dst") == [0, 10, 30, M64 - 10, 30, 31, 31, 32]
    # ... and a sum that reaches 2^64 exactly has wrapped as well
    got = check(program, t, [dict(ranges=[(1, 0, 16), (0, 0, M64 - 15), (1, 0, 1)], out_cap=1 << 20)])
    assert statuses(got[2][1]) == [0, E_INVAL, E_DST_SMALL] and field(got[2][1], "dst") == [0, 16, 0]


def test_overlapping_ranges_and_single_blocks(program):
    t = Table([(300_001, 1), (300_001, 0), (262_144, 1)], accept=[1, 1, 1])
    sets = [[(0, 10, 1001), (0, 500, 1001)], [(0, 10, 1001), (0, 500, 1001), (0, 900, 200_000)], [(0, 5, 5)], [(0, 300_000, 1)], [(0, 262_144, 10), (1, 262_144, 10)],
            [(0, 100_000, 162_145), (1, 100_000, 162_145)], [(2, 131_072, 131_072)], [(2, 0, 262_144)], [(0, 0, 1), (0, 300_000, 1)]]
    for v in (0, 1):
        got = check(program, t, [dict(what=s, verified=v, ranges=s) for s in sets])
        assert "decoded 131072" in got[2][1] and f"decoded {300_001 - 2 * BLK}" in got[5][1] and "decoded 300001" in got[7][1]
        assert f"decoded {BLK + 300_001 - 2 * BLK}" in got[10][1]     # the first and the last block: the slot spans all three, two are decoded


def test_pieces_at_every_residue(program):
    lens = [1, 127, 128, 129, PIECE - 1, PIECE, PIECE + 1, 3 * PIECE + 5]
    t = Table([(300_001, 0), (300_001, 1)])
    for skew in (0, 77):
        ranges, out, at = [], [], 0
        for res in range(128):
            for n in lens:
                at = -(-at // 128) * 128 + 128 + (res - skew) % 128      # OUT + skew + at is `res` behind a 128-byte line
                ranges.append((res & 1, res * 7, n)); out.append(at)
                at += n
        got = check(program, t, [dict(ranges=ranges, out=out, out_cap=at, skew=skew)], full=1 << 20)[2][1]
        src, dst, ln = field(got, "pc.src"), field(got, "pc.dst"), field(got, "pc.len")
        k = 0
        for (row, begin, n), o in zip(ranges, out):
            want_src = BLOBS + t.bo[0] + begin if row == 0 else POOL0 + GUARD + begin    # row 1: its slot is the first, behind the guard
            d0, first = OUT + skew + o, True
            while n:
                assert (src[k], dst[k]) == (want_src, d0) and 1 <= ln[k] <= PIECE and ln[k] <= n
                assert first or dst[k] % 128 == 0, (row, begin, n)
                want_src, d0, n, first, k = want_src + ln[k], d0 + ln[k], n - ln[k], False, k + 1
        assert k == len(ln)       # the pieces tile the ranges exactly, in order
        assert sorted({(OUT + skew + o) % 128 for o in out}) == list(range(128))


def test_scratch_limit(program):
    lines = [ln for ln in run(program, f"S 0 0 {SCRATCH_MAX - 256}\nS 0 0 {SCRATCH_MAX - 255}\nS 1 {GUARD} {SCRATCH_MAX - 256 - 256 - GUARD}\n"
                              f"S 1 {GUARD} {SCRATCH_MAX - 256 - 256 - GUARD + 1}\nS 256 0 {M64 - 300}\nS 0 0 {M64}") if not ln.startswith("#")]
    assert lines[:6] == [f"slot 1 {SCRATCH_MAX} 0", "slot 0", f"slot 1 {SCRATCH_MAX} {256 + GUARD}", "slot 0", "slot 0", "slot 0"]
    big = 2**32 + 5
    for n_big, code in ((7, 0), (8, E_NOMEM)):     # 7 x (4 GiB + 5 + 256) and a small row: under; an eighth: over
        t = Table([(big, 1)] * n_big + [(BLK, 1)])
        got = check(program, t, [dict(ranges=[(r, 5, 1) for r in range(n_big + 1)])])
        assert got[2][1][0] == f"build {code}"
    # the late pass has a pool of its own with the same limit: rows just under 4 GiB, every one given up on
    t = Table([(2**32 - 2, 1)] * 9)
    got = check(program, t, [dict(ranges=[(r, 5, 1) for r in range(n)], late_mode=1) for n in (7, 8, 9)])
    assert ["late 0" in g[1] for g in got[2:]] == [True, False, False] and f"late {E_NOMEM}" in got[4][1]
    # the tree build decodes every compressed row with entries whole
    t = Table([(2**32 - 2, 1)] * 7 + [(2**32 - 2, 0)] * 3)
    assert check(program, t, [], trees=[{}])[2][1][0] == "tree_rows 0"
    t = Table([(2**32 - 2, 1)] * 8)
    assert check(program, t, [], trees=[{}])[2][1][0] == f"tree_rows {E_NOMEM}"


def test_row_length_near_2_64_does_not_wrap_the_slot_sum(program):
    """A defect this test found in the code the module was cut from: a whole-row slot was added to the pool's size before the sum was
    compared with the limit, so a table row whose length is close to 2^64 wrapped the sum, the call went on, and the rows behind it were
    given slots that overlap the rows in front.  The slot rule refuses a length above the limit before it adds it."""
    t = Table([(5000, 1), (M64 - 5000, 1), (5000, 1)])     # 5,376 + (2^64 - 5,001) + 256 = 2^64 + 631: row 2 would land at 768, inside row 0's slot
    got = check(program, t, [dict(ranges=[(0, 0, 10), (1, 0, 10), (2, 0, 10)]), dict(ranges=[(0, 0, 10), (2, 0, 10)])], trees=[{}])
    assert got[2][1][0] == f"build {E_NOMEM}" and got[3][1][0] == "build 0"


def test_item_limit(tmp_path_factory):
    """(a second build of the program with the limit at 40: see the module's docstring)"""
    exe = build_program(tmp_path_factory.mktemp("range_plan_items"), "plan40", ["-DZN_RR_ITEMS_MAX=40"])
    assert run(exe, "")[-1] == f"limits {BLK} {GUARD} {SCRATCH_MAX} 40 {PIECE}"
    rows = [(10 * BLK + 1, 1)] * 5        # 11 blocks each: the fourth would make 44 — it and, at 33 + 11 >= 40, the fifth are read whole
    t = Table(rows + [(3 * BLK, 1), (2 * BLK, 1)], accept=[1] * 7)     # 33 + 3 = 36 fits; 36 + 2 = 38 fits as well: 40 itself is never reached
    for v in (0, 1):
        got = check(exe, t, [dict(verified=v, ranges=[(r, BLK + 5, 10) for r in range(7)])], items_max=40)[2][1]
        assert field(got, "part") == [0, 1, 2, 5, 6] and field(got, "whole") == [3, 4] and "n_items 38 n_todo 5 need0" in " ".join(got)
    t = Table(rows[:3] + [(7 * BLK, 1), (6 * BLK, 1)])                   # 33 + 7 = 40: refused; 33 + 6 = 39: taken
    got = check(exe, t, [dict(ranges=[(r, 5, 10) for r in range(5)])], items_max=40)[2][1]
    assert field(got, "part") == [0, 1, 2, 4] and field(got, "whole") == [3]


def test_tree_build(program):
    rows = [(5000, 1), (300_001, 1), (300_001, 0), (BLK, 1), (BLK + 1, 0), (2**32 - 1, 1), (2**32, 1), (262_144, 1), (0, 0), (262_145, 1)]
    t = Table(rows, blob_off={7: 3})      # a corrupt extent among them: row 7's blob starts in front of the blob region
    t2 = Table(rows, base=50)
    t2.blob_cap = t2.end - 50 - 1         # ... and the last row's ends one byte outside
    for tab, base in ((t, 10), (t2, 50)):
        got = check(program, tab, [], trees=[dict(blob_base=base), dict(blob_base=base, fail_mode=1)])
        st = statuses(got[2][1], "tst")
        assert [i for i, s in enumerate(st) if s == E_CORRUPT] == ([7] if tab is t else [9])
        assert field(got[2][1], "tw.row") == ([1, 2, 4, 5, 9] if tab is t else [1, 2, 4, 5, 7])


def test_seeded_random_calls(program):
    rng = np.random.default_rng(20260101)
    n_calls = 0
    for _ in range(40):
        n = int(rng.integers(1, 17))
        rows = [(LENGTHS[int(rng.integers(len(LENGTHS)))], int(rng.integers(2))) for _ in range(n)]
        base = pick(rng, [0, 12345, (1 << 40) + 12345])
        t = Table(rows, row_begin=pick(rng, [0, 3]), base=base, accept=[int(rng.integers(2)) for _ in range(int(rng.integers(0, n + 1)))])
        if rng.integers(3) == 0:
            t.blob_cap = t.end - base - int(rng.integers(0, 3))
        calls = []
        for _ in range(8):
            out_cap = pick(rng, [0, 4000, 1 << 20, 1 << 24])
            ranges, out = [], []
            for _ in range(int(rng.integers(1, 65))):
                row = int(rng.integers(-1, n + 1)) + t.row_begin
                L = t.len[row - t.row_begin] if 0 <= row - t.row_begin < n else 1000
                kind = int(rng.integers(8))
                begin = int(rng.integers(0, L + 1)) if kind else pick(rng, [L, L + 1, M64, max(L, 1) - 1])
                if kind > 2 and L > BLK:
                    begin = min(L, int(rng.integers(0, 4)) * BLK + pick(rng, [0, 1, BLK - 1, 70_000]))     # near the front, where ranges share blocks
                ln = pick(rng, [0, 1, 127, 4096, BLK, BLK + 1, 300_001, (M64 - begin + 1) & M64, max(L - begin, 0)])
                ranges.append((max(row, 0), begin, min(ln, 1 << 21) if kind != 1 else ln))
                out.append(int(rng.integers(0, max(out_cap, 1) + 2)))
            calls.append(dict(verified=int(rng.integers(2)), blob_base=pick(rng, [base, base, base + 1, 0]), out_cap=out_cap, out=out if rng.integers(2) else None,
                              skew=int(rng.integers(128)), late_mode=int(rng.integers(4)), fail_mode=int(rng.integers(3)), bad_mode=int(rng.integers(2)), ranges=ranges))
        check(program, t, calls, trees=[dict(blob_base=base, fail_mode=int(rng.integers(2)))])
        n_calls += len(calls)
    assert n_calls == 320
