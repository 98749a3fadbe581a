// The read side's host decisions (rows_plan.h).
#include "rows_plan.h"
#include "range_plan.h"

extern "C" void zn_rows_extents(const uint64_t *bo, const uint64_t *bs, const uint64_t *oo, const uint64_t *us, size_t n, uint64_t out[8]);  // extents.cc

using namespace zn;

uint32_t plan_small_tiles(const PlanBuf &p) {
    uint32_t n = 0;
    for (const Tile &t : p.tiles) n += t.n_units != 0;
    return n;
}
uint32_t plan_max_cvs(const PlanBuf &p) {
    uint32_t m = 0;
    for (const BigUnit &b : p.big) m = std::max(m, b.n_cvs);
    return m;
}

bool rows_all_compressed(const uint8_t *bitmap, uint64_t row_begin, uint64_t row_end) {
    bool allc = true;
    if (bitmap) {
        uint64_t row = row_begin;
        for (; row < row_end && (row & 7); row++) allc &= (bitmap[row >> 3] >> (row & 7)) & 1;
        for (; row + 8 <= row_end && allc; row += 8) allc &= bitmap[row >> 3] == 0xFF;
        for (; row < row_end && allc; row++) allc &= (bitmap[row >> 3] >> (row & 7)) & 1;
    }
    return allc;
}

// the pass over the columns (s.n is set): counts, extents and the lists of the compressed rows above 64 KiB
static void classify_rows(const RowCols &c, const RowsSwitches &sw, RowsShape &s, RowClasses &k) {
    constexpr uint64_t BLK = BLOCK_TREE_BLK;
    const uint32_t n = s.n;
    if (c.allc) {  // the vectorised pass; the row-by-row one below only if the table has big rows
        uint64_t e[8];
        zn_rows_extents(c.bo, c.bs, c.oo, c.us, n, e);
        if (e[6] == 0) {
            s.ext_min_bo = e[0]; s.ext_max_bend = e[1]; s.ext_max_oend = e[2]; s.ext_wrap = e[3] != 0;
            s.n_compressed = n; s.bx_bytes = e[4]; k.nblk = e[5];
            s.xxh_forms = 1;  // (no row above 64 KiB: the checksum stage's quad form alone)
            return;
        }
    }
    uint64_t min_bo = ~0ull, max_bend = 0, max_oend = 0;
    bool wrap = false;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t comp = c.comp(i);
        const uint64_t bo = c.bo[i], bs = c.bs[i], oo = c.oo[i], us = comp ? c.us[i] : bs;  // a stored row IS its blob
        s.n_compressed += comp;
        if (!comp && (oo & 15)) s.odd_out = true;
        min_bo = std::min(min_bo, bo);
        wrap |= bo + bs < bo || oo + us < oo;
        max_bend = std::max(max_bend, bo + bs);
        max_oend = std::max(max_oend, oo + us);
        if (!comp) continue;
        k.nblk += us ? (us + BLK - 1) / BLK : 1;
        s.bx_bytes += us;
        if (us > 65536 && us < (1ull << 30)) s.rx_words_small += (us + 1023) & ~1023ull;
        if (us >= RX_MIN && us < (1ull << 30)) s.rx_words += (us + 1023) & ~1023ull;
        s.xxh_forms |= us < XXH_WAVE_MIN ? 1 : 2;
        if (us <= 64 * 1024) continue;
        k.big_bytes += us;
        k.big_blob += bs;
        k.n_big++;
        const uint64_t nb = (us + BLK - 1) / BLK;
        if (nb >= 2 && us < 0xFFFFFFFFull && k.item_row.size() + nb < 0x7FFFFFFFull && !sw.no_block_items) {
            k.cand_row.push_back(i);
            k.cand_base.push_back((uint32_t)k.item_row.size());
            k.cand_nb.push_back((uint32_t)nb);
            for (uint32_t b = 0; b < nb; b++) { k.item_row.push_back(i); k.item_k.push_back(b); }
            // (the round-2 two-phase path stands behind the block items only where the batch path does not)
            if (!sw.no_fz && sw.no_bx && k.fz_it_cand.size() + 2 * nb + 8 < 0x7FFFFFFFull) {
                const uint32_t cap = (uint32_t)(2 * nb + 8);
                k.fz_base.push_back((uint32_t)k.fz_it_cand.size());
                k.fz_cap.push_back(cap);
                k.fz_it_cand.insert(k.fz_it_cand.end(), cap, (uint32_t)k.cand_row.size() - 1);
                s.fz_bytes += us;
            } else { k.fz_base.push_back(0); k.fz_cap.push_back(0); }
        } else k.la.push_back(i);
    }
    s.ext_min_bo = min_bo; s.ext_max_bend = max_bend; s.ext_max_oend = max_oend; s.ext_wrap = wrap;
}

// fused block kernel: the big-slice tiles of the candidate rows and the item each belongs to (a slice of 64 leaves is half a block)
static void block_tiles(uint32_t n, const PlanBuf &p, RowClasses &k) {
    std::vector<uint32_t> row_base(n, 0xFFFFFFFFu);
    for (size_t c = 0; c < k.cand_row.size(); c++) row_base[k.cand_row[c]] = k.cand_base[c];
    for (uint32_t ti = 0; ti < (uint32_t)p.tiles.size(); ti++) {
        const Tile &t = p.tiles[ti];
        if (t.n_units == 0 && row_base[t.first_unit] != 0xFFFFFFFFu) {
            k.bt_tile.push_back(ti);
            k.bt_item.push_back(row_base[t.first_unit] + (t.first_leaf >> 7));
        }
    }
}

void rows_classify(const RowCols &c, const RowsSwitches &sw, const PlanBuf &p, RowsShape &s, RowClasses &k) {
    s.n = (uint32_t)(c.row_end - c.row_begin);
    s.n_tiles = (uint32_t)p.tiles.size();
    s.n_big_units = (uint32_t)p.big.size();
    s.n_small_tiles = plan_small_tiles(p);
    classify_rows(c, sw, s, k);
    s.n_list_a = (uint32_t)k.la.size();
    s.n_cand = (uint32_t)k.cand_row.size();
    s.n_items = (uint32_t)k.item_row.size();
    s.fz_total = s.n_cand ? (uint32_t)k.fz_it_cand.size() : 0;
    if (s.n_compressed && !sw.no_bx) {
        s.bx_nblk = k.nblk;
        if (s.rx_words_small && s.rx_words_small <= (256ull << 20)) { s.rx_min = 65537; s.rx_words = s.rx_words_small; }
        // a writer may split blocks (libzstd's high levels cut a 128 KiB block into 2-5; runs of equal bytes come as
        // strings of small RLE blocks): half as many again + up to 64k more, shared by all frames.  Frames that find no
        // slot stay with the serial decoder.  (A table too big for 31-bit item numbers has no batch path.)
        const uint64_t cap = k.nblk + k.nblk / 2 + std::min<uint64_t>(3 * k.nblk, 65536) + 1024;
        if (cap < 0x7FFFFFFFull) { s.bx_slots = s.n_compressed; s.bx_item_cap = (uint32_t)cap; }
        s.rx_frames = s.bx_slots && (s.rx_words || s.rx_words_small) && !sw.no_rx;
    }
    // 1024-thread workgroups pay off where a few very long copies dominate (multi-MiB frames of periodic or stored
    // data: a frame that is < 2 % of its content); entropy-coded frames are a serial bitstream and want the narrow
    // variant's window execution instead, whatever their size
    s.wide_rows = k.n_big && k.big_bytes / k.n_big >= (1u << 20) && k.big_blob * 50 < k.big_bytes;
    const bool hints = !sw.no_lean && s.n_list_a == 0;  // what the lean forms of a run have in common
    s.small_ok = c.allc && hints && !sw.no_bx && s.n_cand == 0 && s.n_small_tiles == s.n_tiles && s.n_small_tiles > 0 && s.bx_slots;
    s.lean_mixed_ok = hints && s.n_cand == 0 && s.n_small_tiles > 0 && s.n_small_tiles < s.n_tiles;
    s.lean_blocks_ok = c.allc && hints && s.n_cand > 0 && s.n_small_tiles == 0;
    s.lean_ok = c.allc && hints && s.n_cand == 0 && p.big.empty() && s.n_small_tiles == s.n_tiles && s.n_small_tiles > 0;
    if (s.n_cand && !sw.no_fused_blocks) {
        block_tiles(s.n, p, k);
        s.n_bt = (uint32_t)k.bt_tile.size();
    }
}

size_t rows_done_bytes(const RowsShape &s, size_t *items_at) {
    *items_at = (std::max<size_t>(s.n_tiles, 16) + 15) & ~(size_t)15;
    return *items_at + std::max<size_t>(s.n_items, 16);
}

void rows_note_hint(const RowsShape &s, RowsHints &h, const HandCounts &left) {
    const bool handed = left.fused || left.serial || left.flagged;
    h.bx_hint = (handed || s.n_list_a) ? 1 : 0;
    h.lean_hint = (handed || left.tiles) ? 0 : 1;
    h.lean_hint2 = (handed || left.items) ? 0 : 1;
    if (s.n_small_tiles && left.tiles >= s.n_small_tiles) h.roles_off = true;  // the role-split kernel took not one tile: not this table's kernel
    // ... and when the fused kernels handed over every row of a table of small compressed rows, the next runs give the rows to the
    // batch path themselves (100k rows of real text: 0.26 ms of parsing each frame only to pass it on)
    if (s.small_ok && left.fused >= s.n) h.small_off = true;
    if (h.small_off) h.bx_hint = 1;
}
void rows_note_plain(const RowsShape &s, RowsHints &h, const HandCounts &left) {
    h.plain_hint = (left.fused || left.serial || left.flagged || s.n_list_a) ? 1 : 0;
}
void rows_force_full(RowsHints &h) {
    h.force_full = true;
    h.lean_hint = 0; h.lean_hint2 = 0;
}

RunPlan rows_plan(const RowsShape &s, const RowsHints &h, const RunEnv &e, int preset, bool verify, bool plain) {
    const RowsSwitches &sw = *e.sw;
    RunPlan p{};
    p.empty = s.n == 0;
    const int route = rows_route_hint(h, plain);  // bx_hint, or a decode-only run's own copy of it
    p.bx = s.bx_slots && e.fz_lit_pool && e.fz_seq_pool && e.bx_fse_pool && e.bx_huf_pool && route != 0;
    p.small_off = p.bx && h.small_off && !h.n_bad && !h.force_full && !sw.dbg;
    // (a repository of small files the reference stores as they are — png, jpg, gz —, or one big jar.  The fused small-row kernel
    // copies a stored row with each lane's own 64-byte stores: 100k x 10 KiB stored rows 0.85 ms there, 0.63 through the store path kernel)
    p.stored_only = s.n_compressed == 0 && !preset && !sw.dbg && !sw.no_stored_only && !h.force_full;
    // (a decode-only run is never a lean run: nothing it queues could flag it, so it leaves nothing out that a row might need — and it has
    //  no use for the role-split kernel, whose loaders feed hashers)
    const bool may_skip = !preset && !h.force_full && !plain;  // a run may leave out what the table's last finished run had no use for
    if (!p.small_off && !p.stored_only) {
        // Tables with enough small tiles go to the role-split persistent kernel first (loader + hasher waves: tiles whose rows are all whole-leaf rows of
        // the recognised periodic shape); what it leaves on its list — and small tables, where a persistent grid only adds start-up latency — is k_fused_small's.
        p.roles = !sw.no_roles && sw.roles_min != 0 && s.n_small_tiles >= sw.roles_min && s.n_small_tiles > 0 && !(sw.dbg & (1 | 2 | 4 | 8 | 128)) && !h.roles_off && !plain;
        // A table of small rows AND big stored / hashed units (BASELINE configs[4]: 3,500 small files beside 6 GB of jars) whose
        // last run handed nothing over: nothing of the small rows' kernel and the second hash pass depends on the other (C5:
        // 0.28 ms of a 3.45 ms step ran in front of the pass).
        p.lean_mixed = s.lean_mixed_ok && h.lean_hint == 1 && h.bx_hint == 0 && may_skip && !sw.dbg && !sw.ddbg;
        p.lean = p.roles && s.lean_ok && h.lean_hint == 1 && h.bx_hint == 0 && may_skip && !sw.dbg;
        // what the roles kernel leaves on its list, capped at five workgroups per CU behind it; a lean run leaves it out
        p.small = s.n_small_tiles && !p.lean;
        p.small_grid_cap = p.roles ? e.cus * 5 : 0;
    }
    p.misaligned_dst = !verify && (s.odd_out || e.dst_misaligned);
    p.merge_big = s.n_big_units != 0;
    p.copy_stored = p.stored_only || s.n_big_units;  // (stored rows above a tile; stored_only: every row)
    // a run that left stages out: its lists must be empty, or the counters come back flagged
    p.lists_small = p.lean || p.lean_mixed;
    // A lean run has nothing between its one kernel and the verify, and nothing of the NEXT run's kernels reads what the verify
    // writes (the other slot is theirs): the next run's kernel follows this run's directly.
    p.verify_aux = e.fork_verify && p.lean;
    p.check_lists = p.lean || p.lean_mixed;
    p.decode = !p.lean && !p.lean_mixed && !p.stored_only;
    if (!p.decode) return p;
    p.items = s.n_cand != 0;
    p.fused_blocks = p.items && s.n_bt;  // blocks of the common shape: written and hashed in one go, skipped by the block decoder and the second hash pass
    p.hash_skips_done = p.fused_blocks;
    p.two_phase = p.items && s.fz_total;
    p.items_grid = std::min<int>(e.decode_grid, (int)s.n_items);
    // a table of big rows only whose last run handed nothing over: the main stream has nothing for the block items to run beside, and
    // the fork and the join between two streams were ~0.1 ms of C3's 1.09 ms step
    p.one_stream = s.n_cand && route == 0 && s.n_small_tiles == 0;
    // ... and when its last run needed neither the serial block decoder nor the serial decoder behind it (every block item was written and hashed by the
    // fused block kernel), those three launches are left out, the way a lean run of a table of small rows leaves out what stands behind the roles kernel.
    p.lean_blocks = p.one_stream && s.lean_blocks_ok && h.lean_hint2 == 1 && may_skip && s.n_bt && !sw.ddbg && !s.fz_total;
    p.block_decoder = p.items && !p.lean_blocks;
    p.check_lists = p.lean_blocks;
    if (!s.n_compressed) return p;
    p.decoders = true;
    // (the serial decoder's launch then returns at once instead of waiting for CUs next to the block kernels: C3's 0.25 ms that only waited)
    p.behind = !p.bx && s.n_cand && route == 0;
    p.rx = p.bx && e.rx_base && e.rx_pool && s.rx_words;
    // (only where the chip is not full of blocks anyway: 100k blocks, both kernels chip-wide: 2.98 ms together against 1.85 + 0.96 in a row)
    p.third = p.bx && s.bx_nblk <= 32768;
    if (p.bx) {
        p.xxh = e.xxh;
        // 0: the blocks that get a wave of their own are picked from the table's histogram (k_bx_split: one workgroup per
        // list, worth its ~0.1-0.4 ms where the chip is not full of blocks anyway); big tables keep the fixed threshold
        p.big_seq = sw.bx_big_set || s.bx_nblk > 32768 ? sw.bx_big : 0u;
        p.small_frames = s.bx_bytes / s.n_compressed <= 65536;
        if (p.rx) p.rx_bound = std::min<uint64_t>(s.rx_words, e.rx_cap);
        p.fallback_grid = std::min<int>(e.decode_grid, (int)s.n_compressed);  // what the batch path left: any compressed row
    } else {
        // A full grid of the general decoder (4 workgroups per CU at 128 VGPRs) is the whole register file: whatever the auxiliary
        // stream launches then waits until workgroups run out of rows.  With candidates for the block / foreign-frame
        // paths it leaves them a quarter.
        const int gen_grid = s.n_cand && !p.behind ? e.decode_grid / 4 * e.gen_share : e.decode_grid;
        p.general_grid = std::min<int>(gen_grid, (int)s.n_compressed);
        p.fallback_grid = std::min<int>(e.decode_grid, (int)s.n_cand);  // what the block items gave up on
    }
    return p;
}

FzPoolSizes fz_pool_sizes(uint64_t content_bytes, uint32_t items) {
    constexpr uint64_t CAP = 16ull << 30;
    return FzPoolSizes{std::min<uint64_t>(content_bytes + 80ull * items + 4096, CAP), std::min<uint64_t>(content_bytes * 3 / 2 + 4096, CAP) / 8};
}
BxPoolSizes bx_pool_sizes(uint64_t content_bytes, uint32_t items) {
    constexpr uint64_t CAP = 16ull << 30;
    const uint64_t bytes = std::min<uint64_t>(content_bytes / 2 + 64ull * items + 4096, CAP);
    return BxPoolSizes{bytes / 2 + BX_POOL_FIRST, bytes / 2};
}
uint64_t rx_pool_words(uint64_t words) {
    constexpr uint64_t CAP = (1ull << 31) - (1ull << 20);
    return std::min<uint64_t>((words + 1023) & ~1023ull, CAP);
}
uint64_t verify_scratch_bytes(uint64_t bytes) {
    constexpr uint64_t CAP = 16ull << 30;
    if (!bytes) return 0;
    return bytes > CAP ? POOL_REFUSED : bytes + 4096;
}
uint64_t range_scratch_bytes(uint64_t bytes, uint64_t other_cap) {
    constexpr uint64_t CAP = 16ull << 30;
    if (!bytes) return 0;
    return bytes > CAP || bytes + other_cap > CAP + 8192 ? POOL_REFUSED : bytes + 4096;
}

bool rows_fit(const RowsShape &s, uint64_t blob_base, uint64_t blob_cap, uint64_t out_cap, bool verify) {
    return !s.ext_wrap && (s.n == 0 || (s.ext_min_bo >= blob_base && (blob_cap == ~0ull || s.ext_max_bend - blob_base <= blob_cap) && (verify || s.ext_max_oend <= out_cap)));
}
uint32_t rows_verdicts(const uint64_t *bo_, const uint64_t *bs_, const uint64_t *len_, const uint64_t *oo_, uint32_t n, uint64_t blob_base, uint64_t blob_cap,
                       uint64_t out_cap, bool verify, std::vector<int32_t> &status) {
    uint32_t bad = 0;
    if (verify) out_cap = ~0ull;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t bo = bo_[i], bs = bs_[i], len = verify ? 0 : len_[i], oo = verify ? 0 : oo_[i];
        int code = 0;
        if (bo < blob_base) code = RP_E_CORRUPT;
        else if (blob_cap != ~0ull && (bs > blob_cap || bo - blob_base > blob_cap - bs)) code = RP_E_CORRUPT;
        else if (len > out_cap || oo > out_cap - len) code = RP_E_DST_SMALL;
        if (code) {
            if (status.empty()) status.assign(n, 0);
            status[i] = code;
            bad++;
        }
    }
    return bad;
}
