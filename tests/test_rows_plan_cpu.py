"""The read side's host decisions (znippy_amd/csrc/host/rows_plan.cc: the tile plan, what table creation learns about the rows, the
hints of a finished run, the plan of a run, the pool sizes, the host's verdicts) as a stand-alone host program under
AddressSanitizer and UBSan.  Cases go in on stdin, every field comes back, and models written from the statements of the rules
— the comments beside the code — are compared with it field by field.  One process per grid:
  run plan   three grids, each a full product of the dimensions that meet in a rule (plan_grids): shapes (small tiles only below, at
             and above roles_min / big stored units beside them / candidates only / candidates and small tiles / no compressed row /
             empty, with the lean-shape flags each allows) x the four hints in {-1, 0, 1} x roles_off, small_off, force_full, n_bad
             x the three kinds of run; that whole product again under each switch by itself; the shapes x the hints that route x
             each pool absent x bx_nblk 32768 / 32769 x the checksum switch x an odd output pointer x two decoder grids
  hints      the 32 zero / non-zero patterns of the five hand-over counts, the two thresholds at -1, 0, +1, x shapes x hints so far
  tables     columns drawn from the sizes at which a rule changes (no data of that size: only the columns exist): tile plan against
             the unit-by-unit greedy rule WITHOUT the run shortcut, classification row by row, the fused block kernel's lists
  verdicts   regions and rows at 0, 1, 2^32, 2^64 - 1 and sums that wrap; the pool sizes around their caps and rounding steps
The two 0x7FFFFFFF caps on the item lists' lengths are out of a test's reach (2^31 list entries); they are in rows_plan.cc as they
were in api.hip."""
import itertools
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
#include "rows_plan.h"
typedef unsigned long long ull;
static bool rd(ull *v, int n) { for (int i = 0; i < n; i++) if (scanf("%llu", &v[i]) != 1) return false; return true; }
static ull weighted(const std::vector<uint32_t> &v) { ull s = 0; for (size_t i = 0; i < v.size(); i++) s += (ull)(i + 1) * ((ull)v[i] + 1); return s; }
static void list(const std::vector<uint32_t> &v) { printf(" %zu %llu", v.size(), weighted(v)); }
static RowsSwitches switches(const ull *v) {  // 12 values
    RowsSwitches sw;
    sw.dbg = (int)v[0]; sw.no_block_items = v[1]; sw.no_fused_blocks = v[2]; sw.ddbg = v[3]; sw.no_roles = v[4]; sw.no_fz = v[5]; sw.no_bx = v[6]; sw.no_rx = v[7];
    sw.no_lean = v[8]; sw.no_stored_only = v[9]; sw.roles_min = (unsigned)v[10]; sw.bx_big_set = v[11] != 0; sw.bx_big = v[11] ? (unsigned)v[11] : 2048;
    return sw;
}
int main() {
    char tag[8];
    while (scanf("%7s", tag) == 1) {
        if (tag[0] == 'P') {  // 16 shape + 8 hints + 13 env + 12 switches + preset verify plain
            ull v[52];
            if (!rd(v, 52)) { printf("bad line\n"); return 2; }
            RowsShape s;
            s.n = (uint32_t)v[0]; s.n_compressed = (uint32_t)v[1]; s.n_cand = (uint32_t)v[2]; s.n_items = (uint32_t)v[3]; s.n_bt = (uint32_t)v[4]; s.n_small_tiles = (uint32_t)v[5];
            s.n_big_units = (uint32_t)v[6]; s.fz_total = (uint32_t)v[7]; s.bx_slots = (uint32_t)v[8]; s.bx_nblk = v[9]; s.bx_bytes = v[10]; s.rx_words = v[11]; s.odd_out = v[12];
            s.lean_ok = v[13]; s.lean_mixed_ok = v[14]; s.lean_blocks_ok = v[15];
            RowsHints h;
            h.bx_hint = (int)v[16] - 1; h.lean_hint = (int)v[17] - 1; h.lean_hint2 = (int)v[18] - 1; h.plain_hint = (int)v[19] - 1;
            h.roles_off = v[20]; h.small_off = v[21]; h.force_full = v[22]; h.n_bad = (uint32_t)v[23];
            const RowsSwitches sw = switches(v + 37);
            const RunEnv e{v[24] != 0, v[25] != 0, v[26] != 0, v[27] != 0, v[28] != 0, v[29] != 0, v[30], (int)v[31], (int)v[32], (int)v[33], v[34] != 0, v[35] != 0, v[36] != 0, &sw};
            const RunPlan p = rows_plan(s, h, e, (int)v[49], v[50] != 0, v[51] != 0);
            printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %u %d %llu %d %d %d %d %d %d %d\n", p.empty, p.bx, p.small_off, p.stored_only, p.roles, p.lean,
                   p.lean_mixed, p.small, p.small_grid_cap, p.decode, p.items, p.fused_blocks, p.block_decoder, p.two_phase, p.decoders, p.one_stream, p.lean_blocks, p.behind, p.rx, p.third,
                   p.xxh, p.items_grid, p.general_grid, p.fallback_grid, p.big_seq, p.small_frames, (ull)p.rx_bound, p.misaligned_dst, p.hash_skips_done, p.merge_big, p.copy_stored,
                   p.check_lists, p.lists_small, p.verify_aux);
        } else if (tag[0] == 'H') {  // n n_small_tiles n_list_a small_ok | small_off roles_off so far | fused serial flagged tiles items
            ull v[11];
            if (!rd(v, 11)) { printf("bad line\n"); return 2; }
            RowsShape s;
            s.n = (uint32_t)v[0]; s.n_small_tiles = (uint32_t)v[1]; s.n_list_a = (uint32_t)v[2]; s.small_ok = v[3];
            RowsHints h, hp;
            h.small_off = v[4]; h.roles_off = v[5];
            const HandCounts left{(uint32_t)v[6], (uint32_t)v[7], (uint32_t)v[8], (uint32_t)v[9], (uint32_t)v[10]};
            rows_note_hint(s, h, left);
            rows_note_plain(s, hp, left);
            printf("%d %d %d %d %d %d %d %u  %d %d %d %d\n", h.bx_hint, h.lean_hint, h.lean_hint2, h.plain_hint, h.roles_off, h.small_off, h.force_full, h.n_bad,
                   hp.plain_hint, hp.bx_hint, rows_route_hint(h, false), rows_route_hint(hp, true) + 10 * rows_route_hint(h, true));
        } else if (tag[0] == 'T') {  // n row_begin use_bitmap + 12 switches, then n rows: bo bs us oo comp
            ull v[15];
            if (!rd(v, 15)) { printf("bad line\n"); return 2; }
            const uint32_t n = (uint32_t)v[0];
            const uint64_t rb = v[1];
            // heap blocks of exactly the columns' sizes: a read past a column is the sanitizer's
            uint64_t *bo = (uint64_t *)malloc(8 * (size_t)n + 1), *bs = (uint64_t *)malloc(8 * (size_t)n + 1), *us = (uint64_t *)malloc(8 * (size_t)n + 1), *oo = (uint64_t *)malloc(8 * (size_t)n + 1);
            const size_t bm_bytes = (size_t)((rb + n + 7) >> 3);
            uint8_t *bm = (uint8_t *)calloc(bm_bytes + 1, 1);
            for (uint32_t i = 0; i < n; i++) {
                ull r[5];
                if (!rd(r, 5)) { printf("bad line\n"); return 2; }
                bo[i] = r[0]; bs[i] = r[1]; us[i] = r[2]; oo[i] = r[3];
                if (r[4]) bm[(rb + i) >> 3] |= (uint8_t)(1u << ((rb + i) & 7));
            }
            const RowsSwitches sw = switches(v + 3);
            const bool allc = v[2] != 2 && rows_all_compressed(v[2] ? bm : nullptr, rb, rb + n);  // 2: the bit column is consulted row by row even if every bit is set
            const RowCols c{bo, bs, us, oo, v[2] ? bm : nullptr, rb, rb + n, allc};
            PlanBuf p;
            build_plan([&](uint32_t i) -> uint64_t { return c.comp(i) ? us[i] : bs[i]; }, n, p);
            printf("plan %zu %zu %u %zu %u %u", p.tiles.size(), p.big.size(), p.n_tile_cv, p.grp_big.size(), plan_small_tiles(p), plan_max_cvs(p));
            for (const zn::Tile &t : p.tiles) printf(" %u %u %u %u %u %u", t.first_unit, t.n_units, t.first_leaf, t.n_leaves, t.cv_index, t.pad);
            for (const zn::BigUnit &b : p.big) printf(" %u %u %u %u", b.unit, b.cv_base, b.n_cvs, b.pad);
            for (size_t g = 0; g < p.grp_big.size(); g++) printf(" %u %u", p.grp_big[g], p.grp_k[g]);
            printf("\n");
            RowsShape s;
            RowClasses k;
            rows_classify(c, sw, p, s, k);
            size_t items_at;
            const size_t done = rows_done_bytes(s, &items_at);
            printf("shape %d %u %u %u %u %u %u %u %u %u %u %llu %u %u %llu %llu %llu %llu %u %d %d %d %d %llu %llu %llu %d %d %d %d %d %zu %zu", allc, s.n, s.n_compressed, s.n_list_a, s.n_cand, s.n_items, s.n_bt,
                   s.n_small_tiles, s.n_tiles, s.n_big_units, s.fz_total, (ull)s.fz_bytes, s.bx_slots, s.bx_item_cap, (ull)s.bx_bytes, (ull)s.bx_nblk, (ull)s.rx_words, (ull)s.rx_words_small, s.rx_min,
                   s.rx_frames, s.xxh_forms, s.odd_out, s.wide_rows, (ull)s.ext_min_bo, (ull)s.ext_max_bend, (ull)s.ext_max_oend, s.ext_wrap, s.small_ok, s.lean_ok, s.lean_mixed_ok, s.lean_blocks_ok, done, items_at);
            list(k.la); list(k.cand_row); list(k.cand_base); list(k.cand_nb); list(k.item_row); list(k.item_k); list(k.fz_base); list(k.fz_cap); list(k.fz_it_cand); list(k.bt_tile); list(k.bt_item);
            printf("\n");
            free(bo); free(bs); free(us); free(oo); free(bm);
        } else if (tag[0] == 'V') {  // blob_base blob_cap out_cap verify n, then n rows: bo bs len oo
            ull v[5];
            if (!rd(v, 5)) { printf("bad line\n"); return 2; }
            const uint32_t n = (uint32_t)v[4];
            std::vector<uint64_t> col[4];
            RowsShape s;
            s.n = n; s.ext_min_bo = ~0ull;
            for (uint32_t i = 0; i < n; i++) {
                ull r[4];
                if (!rd(r, 4)) { printf("bad line\n"); return 2; }
                for (int q = 0; q < 4; q++) col[q].push_back(r[q]);
                s.ext_min_bo = std::min<uint64_t>(s.ext_min_bo, r[0]); s.ext_max_bend = std::max<uint64_t>(s.ext_max_bend, r[0] + r[1]); s.ext_max_oend = std::max<uint64_t>(s.ext_max_oend, r[3] + r[2]);
                s.ext_wrap |= r[0] + r[1] < r[0] || r[3] + r[2] < r[3];
            }
            std::vector<int32_t> st;
            // (a verify-only run has no length and no output column on the host: the pass must not read them)
            const uint32_t bad = rows_verdicts(col[0].data(), col[1].data(), v[3] ? nullptr : col[2].data(), v[3] ? nullptr : col[3].data(), n, v[0], v[1], v[2], v[3] != 0, st);
            printf("%d %u %zu", rows_fit(s, v[0], v[1], v[2], v[3] != 0), bad, st.size());
            for (int32_t x : st) printf(" %d", x);
            printf("\n");
        } else if (tag[0] == 'S') {  // content_bytes items words bytes other_cap
            ull v[5];
            if (!rd(v, 5)) { printf("bad line\n"); return 2; }
            const FzPoolSizes f = fz_pool_sizes(v[0], (uint32_t)v[1]);
            const BxPoolSizes b = bx_pool_sizes(v[0], (uint32_t)v[1]);
            printf("%llu %llu %llu %llu %llu %llu %llu\n", (ull)f.lit_bytes, (ull)f.seq_records, (ull)b.fse_cells, (ull)b.huf_cells, (ull)rx_pool_words(v[2]), (ull)verify_scratch_bytes(v[3]),
                   (ull)range_scratch_bytes(v[3], v[4]));
        } else { printf("bad line\n"); return 2; }
    }
    return 0;
}
"""

U64 = 1 << 64
BLK = 128 * 1024
CUS, DG = 256, 1024          # a 256-CU chip, four resident decoder workgroups per CU
SHAPE = ("n", "n_compressed", "n_cand", "n_items", "n_bt", "n_small_tiles", "n_big_units", "fz_total", "bx_slots", "bx_nblk", "bx_bytes", "rx_words", "odd_out",
         "lean_ok", "lean_mixed_ok", "lean_blocks_ok")
HINTS = ("bx_hint", "lean_hint", "lean_hint2", "plain_hint", "roles_off", "small_off", "force_full", "n_bad")
ENV = ("fz_lit_pool", "fz_seq_pool", "bx_fse_pool", "bx_huf_pool", "rx_pool", "rx_base", "rx_cap", "cus", "decode_grid", "gen_share", "xxh", "fork_verify", "dst_misaligned")
SW = ("dbg", "no_block_items", "no_fused_blocks", "ddbg", "no_roles", "no_fz", "no_bx", "no_rx", "no_lean", "no_stored_only", "roles_min", "bx_big")
RUN = ("preset", "verify", "plain")
PLAN = ("empty", "bx", "small_off", "stored_only", "roles", "lean", "lean_mixed", "small", "small_grid_cap", "decode", "items", "fused_blocks", "block_decoder", "two_phase", "decoders",
        "one_stream", "lean_blocks", "behind", "rx", "third", "xxh", "items_grid", "general_grid", "fallback_grid", "big_seq", "small_frames", "rx_bound", "misaligned_dst", "hash_skips_done",
        "merge_big", "copy_stored", "check_lists", "lists_small", "verify_aux")
ROLES_MIN = 2048


def plan_shapes():
    """Coherent table shapes, as rows of SHAPE."""
    z = dict.fromkeys(SHAPE, 0)
    out = []
    for nst in (ROLES_MIN - 1, ROLES_MIN, ROLES_MIN + 1):           # small tiles only, below / at / above roles_min
        for lean_ok in (0, 1):
            out.append(dict(z, n=6 * nst, n_compressed=6 * nst, n_small_tiles=nst, bx_slots=6 * nst, bx_nblk=6 * nst, bx_bytes=6 * nst * 10240, lean_ok=lean_ok))
    for mixed_ok in (0, 1):                                         # big stored units beside them, at odd output offsets
        out.append(dict(z, n=5002, n_compressed=5000, n_small_tiles=ROLES_MIN, n_big_units=2, bx_slots=5000, bx_nblk=5000, bx_bytes=5000 * 10240, odd_out=1, lean_mixed_ok=mixed_ok))
    for blocks_ok, fz in itertools.product((0, 1), (0, 56)):        # candidates only (with and without the two-phase slots)
        out.append(dict(z, n=10, n_compressed=10, n_cand=10, n_items=30, n_bt=60, n_big_units=10, fz_total=fz, bx_slots=10, bx_nblk=30, bx_bytes=10 * 300_001, rx_words=10 * 300_032,
                        lean_blocks_ok=blocks_ok))
    out.append(dict(z, n=5010, n_compressed=5010, n_cand=10, n_items=30, n_bt=60, n_small_tiles=ROLES_MIN, n_big_units=10, bx_slots=5010, bx_nblk=5030, bx_bytes=54_200_000,
                    rx_words=10 * 300_032))                          # candidates and small tiles
    out.append(dict(z, n=5001, n_small_tiles=ROLES_MIN, n_big_units=1, odd_out=1))   # no compressed row
    out.append(dict(z))                                             # empty
    return out


def product(*dims):
    return [c.reshape(-1) for c in np.meshgrid(*[np.arange(d) if isinstance(d, int) else np.array(d, dtype=np.int64) for d in dims], indexing="ij")]


def plan_grids():
    """Columns of the three run-plan grids, one behind the other: dict name -> int64 column.  (The full product of every dimension
    would be 10^9 lines: each grid is a full product of the dimensions that meet in a rule.)
      hints     shapes x the four hints x roles_off, small_off, force_full, n_bad x the three kinds of run
      switches  the same product x each switch by itself (ZNIPPY_DBG as 1 and as 16, ZNIPPY_ROLES_MIN=0)
      pools     shapes x bx_hint, plain_hint, small_off x the kinds x each pool absent x bx_nblk 32768 / 32769 x the checksum switch
                (and a word pool smaller than the table's words) x an odd output pointer x ZNIPPY_BX_BIG x a decoder grid below and
                above the shapes' candidate, item and row counts"""
    shapes = plan_shapes()
    switch_sets = [{k: 1} for k in SW[1:10]] + [dict(dbg=1), dict(dbg=16), dict(roles_min=0)]
    env0 = dict(fz_lit_pool=1, fz_seq_pool=1, bx_fse_pool=1, bx_huf_pool=1, rx_pool=1, rx_base=1, rx_cap=1 << 20, cus=CUS, decode_grid=DG, gen_share=3, xxh=0, fork_verify=1, dst_misaligned=0)
    sw0 = dict.fromkeys(SW, 0, ) | dict(roles_min=ROLES_MIN)
    grids = []

    def add(si, kind, hints, env_sets=({},), env_i=None, sw_sets=({},), sw_i=None, **over):
        g = {k: np.array([sh[k] for sh in shapes], dtype=np.int64)[si] for k in SHAPE}
        g.update({k: np.array([dict(env0, **e)[k] for e in env_sets], dtype=np.int64)[0 * si if env_i is None else env_i] for k in ENV})
        g.update({k: np.array([dict(sw0, **w)[k] for w in sw_sets], dtype=np.int64)[0 * si if sw_i is None else sw_i] for k in SW})
        g.update(dict(bx_hint=0 * si - 1, lean_hint=0 * si + 1, lean_hint2=0 * si + 1, plain_hint=0 * si - 1, roles_off=0 * si, small_off=0 * si, force_full=0 * si, n_bad=0 * si))
        g.update(hints)
        g.update(over)
        g.update(preset=(g["n_bad"] != 0).astype(np.int64), verify=(kind == 1).astype(np.int64), plain=(kind == 2).astype(np.int64))   # (rows_launch presets the status column when the host found bad rows)
        grids.append(g)

    si, b, l, l2, ph, ro, so, ff, nb, kind = product(len(shapes), 3, 3, 3, 3, 2, 2, 2, 2, 3)
    add(si, kind, dict(bx_hint=b - 1, lean_hint=l - 1, lean_hint2=l2 - 1, plain_hint=ph - 1, roles_off=ro, small_off=so, force_full=ff, n_bad=3 * nb))
    si, b, l, l2, ph, ro, so, ff, nb, kind, sw = product(len(shapes), 3, 3, 3, 3, 2, 2, 2, 2, 3, len(switch_sets))
    add(si, kind, dict(bx_hint=b - 1, lean_hint=l - 1, lean_hint2=l2 - 1, plain_hint=ph - 1, roles_off=ro, small_off=so, force_full=ff, n_bad=3 * nb), sw_sets=switch_sets, sw_i=sw)
    pool_sets = [{}] + [{k: 0} for k in ENV[:6]]
    si, b, ph, so, kind, pools, nblk, xxh, mis, big, dg = product(len(shapes), 3, 3, 2, 3, len(pool_sets), 2, 2, 2, 2, (8, DG))
    comp = np.array([sh["n_compressed"] for sh in shapes], dtype=np.int64)[si]
    add(si, kind, dict(bx_hint=b - 1, plain_hint=ph - 1, small_off=so), env_sets=pool_sets, env_i=pools, sw_sets=[{}, dict(bx_big=777)], sw_i=big,
        bx_nblk=np.where(comp > 0, 32768 + nblk, 0), xxh=xxh, rx_cap=np.where(xxh > 0, 1000, 1 << 20), dst_misaligned=mis, decode_grid=dg)
    return {k: np.concatenate([g[k] for g in grids]) for k in grids[0]}


class PlanModel:
    """The run plan, from the statements of its rules, over columns of cases."""

    def __init__(self, c):
        T = lambda k: c[k].astype(bool)
        plain, verify, preset = T("plain"), T("verify"), T("preset")
        dbg, ddbg = c["dbg"], T("ddbg")
        nst, n_cand, n_comp = c["n_small_tiles"], c["n_cand"], c["n_compressed"]
        self.empty = c["n"] == 0
        # the routing hint: a decode-only run's own once it has one
        route = np.where(plain & (c["plain_hint"] >= 0), c["plain_hint"], c["bx_hint"])
        # the batch path takes the undecoded frames: the table has slots, its four pools exist, the last run did not find its lists empty
        self.bx = (c["bx_slots"] > 0) & T("fz_lit_pool") & T("fz_seq_pool") & T("bx_fse_pool") & T("bx_huf_pool") & (route != 0)
        self.small_off = self.bx & T("small_off") & (c["n_bad"] == 0) & ~T("force_full") & (dbg == 0)
        self.stored_only = (n_comp == 0) & ~preset & (dbg == 0) & ~T("no_stored_only") & ~T("force_full")
        may_skip = ~preset & ~T("force_full") & ~plain            # a run may leave out what the last finished run had no use for
        front = ~self.small_off & ~self.stored_only                # stage 1 runs
        self.roles = front & ~T("no_roles") & (c["roles_min"] != 0) & (nst >= c["roles_min"]) & (nst > 0) & ((dbg & (1 | 2 | 4 | 8 | 128)) == 0) & ~T("roles_off") & ~plain
        clean = (c["lean_hint"] == 1) & (c["bx_hint"] == 0) & may_skip & (dbg == 0)    # the last run handed nothing over
        self.lean_mixed = front & T("lean_mixed_ok") & clean & ~ddbg
        self.lean = self.roles & T("lean_ok") & clean
        self.small = front & (nst > 0) & ~self.lean
        self.small_grid_cap = np.where(self.roles, 5 * c["cus"], 0)
        self.decode = ~self.lean & ~self.lean_mixed & ~self.stored_only
        self.items = self.decode & (n_cand > 0)
        self.fused_blocks = self.items & (c["n_bt"] > 0)
        self.two_phase = self.items & (c["fz_total"] > 0)
        self.one_stream = self.items & (route == 0) & (nst == 0)   # nothing for the block items to run beside
        self.lean_blocks = self.one_stream & T("lean_blocks_ok") & (c["lean_hint2"] == 1) & may_skip & (c["n_bt"] > 0) & ~ddbg & (c["fz_total"] == 0)
        self.block_decoder = self.items & ~self.lean_blocks
        self.decoders = self.decode & (n_comp > 0)
        self.behind = self.decoders & ~self.bx & (n_cand > 0) & (route == 0)
        batch = self.decoders & self.bx
        self.rx = batch & T("rx_base") & T("rx_pool") & (c["rx_words"] > 0)
        self.third = batch & (c["bx_nblk"] <= 32768)
        self.xxh = batch & T("xxh")
        self.big_seq = np.where(batch & ((c["bx_big"] != 0) | (c["bx_nblk"] > 32768)), np.where(c["bx_big"] != 0, c["bx_big"], 2048), 0)
        self.small_frames = batch & (c["bx_bytes"] // np.maximum(n_comp, 1) <= 65536)
        self.rx_bound = np.where(self.rx, np.minimum(c["rx_words"], c["rx_cap"]), 0)
        dg = c["decode_grid"]
        self.items_grid = np.where(self.decode, np.minimum(dg, c["n_items"]), 0)
        # the general decoder leaves a quarter of its grid (gen_share of four) to what runs beside it
        gen = np.where((n_cand > 0) & ~self.behind, dg // 4 * c["gen_share"], dg)
        self.general_grid = np.where(self.decoders & ~self.bx, np.minimum(gen, n_comp), 0)
        self.fallback_grid = np.where(self.decoders, np.minimum(dg, np.where(self.bx, n_comp, n_cand)), 0)
        self.misaligned_dst = ~verify & (T("odd_out") | T("dst_misaligned"))
        self.hash_skips_done = self.fused_blocks
        self.merge_big = c["n_big_units"] > 0
        self.copy_stored = self.stored_only | (c["n_big_units"] > 0)
        self.check_lists = self.lean | self.lean_mixed | self.lean_blocks
        self.lists_small = self.lean | self.lean_mixed
        self.verify_aux = T("fork_verify") & self.lean


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("rows_plan")
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "plan"
    # (gcc links the sanitizers' runtimes dynamically unless told otherwise; linked into the program they do not care what else
    # the process loads)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", HOST, str(main), os.path.join(HOST, "rows_plan.cc"), os.path.join(HOST, "extents.cc"), "-o", str(exe)], check=True)
    return str(exe)


def run(program, text, timeout=300):
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    return r.stdout


def test_run_plan_over_the_grids(program):
    c = plan_grids()
    names = SHAPE + HINTS + ENV + SW + RUN
    cols = np.stack([c[k] + (1 if k in HINTS[:4] else 0) for k in names], axis=1)      # (the hints travel as 0, 1, 2)
    assert len(cols) == 15 * 81 * 16 * 3 * (1 + 12) + 15 * 18 * 3 * 7 * 32 and 10 ** 5 <= len(cols) <= 10 ** 6    # no case is left out
    text = "\n".join("P " + " ".join(map(str, row)) for row in cols.tolist()) + "\n"
    got = np.array(run(program, text).split(), dtype=np.int64).reshape(len(cols), len(PLAN))
    m = PlanModel(c)
    for j, name in enumerate(PLAN):
        want = np.asarray(getattr(m, name)).astype(np.int64)
        bad = np.nonzero(got[:, j] != want)[0]
        assert not len(bad), (name, len(bad), "first", dict(zip(names, cols[bad[0]].tolist())), "got", int(got[bad[0], j]), "want", int(want[bad[0]]))
        assert len(np.unique(want)) >= 2, name                       # the grids reach both sides of every rule
    p = {name: got[:, j] for j, name in enumerate(PLAN)}
    B = lambda k: p[k].astype(bool)
    plain, full = c["plain"].astype(bool), c["preset"].astype(bool) | c["force_full"].astype(bool)
    assert not (plain & (B("lean") | B("lean_mixed") | B("lean_blocks") | B("roles"))).any()      # a decode-only run is never lean and never uses the roles kernel
    assert not (B("lean") & ~B("roles")).any()
    assert (B("decode") == ~(B("lean") | B("lean_mixed") | B("stored_only"))).all()
    assert not (B("lean_blocks") & ~B("one_stream")).any()
    assert not ((B("rx") | B("third")) & ~B("bx")).any()
    assert not (full & (B("lean") | B("lean_mixed") | B("lean_blocks") | B("small_off") | B("stored_only") | B("check_lists"))).any()   # a preset or force_full run skips nothing
    assert (B("check_lists") == (B("lean") | B("lean_mixed") | B("lean_blocks"))).all()
    assert not (B("verify_aux") & ~B("lean")).any()


def test_hint_update(program):
    """What a finished run's hand-over counts teach the table: all 32 zero / non-zero patterns, the `>= n_small_tiles` and `>= n`
    thresholds at -1, 0, +1, crossed with the shapes and with what earlier runs had set."""
    lines, want = [], []
    for n, nst, la, small_ok in ((3000, 500, 0, 1), (3000, 500, 0, 0), (3000, 500, 3, 0), (4, 0, 0, 0), (4, 0, 2, 0), (5001, 2048, 0, 0), (0, 0, 0, 0)):
        for so0, ro0 in itertools.product((0, 1), (0, 1)):
            for pat in itertools.product((0, 1), repeat=5):
                fused_vals = [0] if not pat[0] else sorted({1, max(n - 1, 1), max(n, 1), n + 1})
                tiles_vals = [0] if not pat[3] else sorted({1, max(nst - 1, 1), max(nst, 1), nst + 1})
                for fused, tiles in itertools.product(fused_vals, tiles_vals):
                    serial, flagged, items = 7 * pat[1], 2 * pat[2], 5 * pat[4]
                    lines.append(f"H {n} {nst} {la} {small_ok} {so0} {ro0} {fused} {serial} {flagged} {tiles} {items}")
                    handed = bool(fused or serial or flagged)          # something went to the decoders behind the fused kernels
                    small_off = bool(so0 or (small_ok and fused >= n))  # the fused kernels handed over every row of a table of small rows
                    roles_off = bool(ro0 or (nst and tiles >= nst))      # the role-split kernel took not one tile
                    bx = 1 if (handed or la or small_off) else 0
                    plain = 1 if (handed or la) else 0
                    # force_full and n_bad are not the update's to touch; a table with its own decode-only hint routes such runs by it
                    want.append([bx, 0 if (handed or tiles) else 1, 0 if (handed or items) else 1, -1, int(roles_off), int(small_off), 0, 0, plain, -1, bx, plain + 10 * bx])
    got = [[int(x) for x in line.split()] for line in run(program, "\n".join(lines) + "\n").splitlines()]
    assert len(got) == len(want)
    for line, g, w in zip(lines, got, want):
        assert g == w, (line, g, w)


# ---- tables: tile plan, classification, fused block lists ---------------------------------------------------------------------------

SIZES = [0, 1, 1024, 65536, 65537, 131072, 131073, 262143, 262144, 2 ** 30 - 1, 2 ** 30, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32]
SW0 = dict(dbg=0, no_block_items=0, no_fused_blocks=0, ddbg=0, no_roles=0, no_fz=0, no_bx=0, no_rx=0, no_lean=0, no_stored_only=0, roles_min=ROLES_MIN, bx_big=0)


def weighted(v):
    return sum((i + 1) * (x + 1) for i, x in enumerate(v)) % U64


def tile_model(lens):
    """The unit-by-unit greedy rule, without the run shortcut: whole small units are packed until a tile has 64 units or the next
    would make more than 64 leaves; a unit of more than 64 leaves closes the tile and becomes slices of 64 leaves + one big unit."""
    tiles, big, grp = [], [], []
    cur = None
    n_cv = 0
    for u, ln in enumerate(lens):
        leaves = max((ln + 1023) // 1024, 1)
        if leaves > 64:
            if cur:
                tiles.append(cur)
                cur = None
            n_cvs = (leaves + 63) // 64
            big.append([u, n_cv, n_cvs, 0])
            if n_cvs > 64:
                grp += [(len(big) - 1, g) for g in range((n_cvs + 63) // 64)]
            tiles += [[u, 0, 64 * t, min(64, leaves - 64 * t), n_cv + t, 0] for t in range(n_cvs)]
            n_cv += n_cvs
        else:
            if cur and (cur[1] == 64 or cur[3] + leaves > 64):
                tiles.append(cur)
                cur = None
            if not cur:
                cur = [u, 0, 0, 0, 0, 0]
            cur[1] += 1
            cur[3] += leaves
    if cur:
        tiles.append(cur)
    gb = 0
    for b in big:                                                        # the group CVs lie behind all tile CVs
        if b[2] > 64:
            b[3] = n_cv + gb
            gb += (b[2] + 63) // 64
    return tiles, big, n_cv, grp


def shape_model(rows, row_begin, use_bitmap, sw, tiles, big):
    """rows: (bo, bs, us, oo, comp).  Every RowsShape field and every list, row by row from the rules."""
    n = len(rows)
    allc = use_bitmap != 2 and (not use_bitmap or all(r[4] for r in rows))
    s = dict(allc=int(allc), n=n, n_compressed=0, fz_bytes=0, bx_bytes=0, rx_words=0, rx_words_small=0, rx_min=256 << 10, xxh_forms=0, odd_out=0, ext_wrap=0)
    la, cand_row, cand_base, cand_nb, item_row, item_k, fz_base, fz_cap, fz_it = ([] for _ in range(9))
    min_bo, max_bend, max_oend, nblk, big_bytes, big_blob, n_big = U64 - 1, 0, 0, 0, 0, 0, 0
    for i, (bo, bs, us, oo, comp) in enumerate(rows):
        if not use_bitmap:
            comp = 1
        ln = us if comp else bs                                          # a stored row is its blob
        s["n_compressed"] += comp
        s["odd_out"] |= int(not comp and oo % 16 != 0)
        min_bo = min(min_bo, bo)
        s["ext_wrap"] |= int(bo + bs >= U64 or oo + ln >= U64)
        max_bend, max_oend = max(max_bend, (bo + bs) % U64), max(max_oend, (oo + ln) % U64)
        if not comp:
            continue
        nb = max((us + BLK - 1) // BLK, 1)
        nblk += nb
        s["bx_bytes"] += us
        if 65536 < us < 2 ** 30:
            s["rx_words_small"] += (us + 1023) // 1024 * 1024
        if 256 << 10 <= us < 2 ** 30:
            s["rx_words"] += (us + 1023) // 1024 * 1024
        s["xxh_forms"] |= 1 if us <= 65536 else 2
        if us <= 65536:
            continue
        big_bytes, big_blob, n_big = big_bytes + us, big_blob + bs, n_big + 1
        if nb >= 2 and us < 2 ** 32 - 1 and not sw["no_block_items"]:   # tried block by block: every block an item
            cand_row.append(i); cand_base.append(len(item_row)); cand_nb.append(nb)
            item_row += [i] * nb; item_k += list(range(nb))
            if not sw["no_fz"] and sw["no_bx"]:                          # the two-phase slots: only where the batch path is off
                fz_base.append(len(fz_it)); fz_cap.append(2 * nb + 8); fz_it += [len(cand_row) - 1] * (2 * nb + 8)
                s["fz_bytes"] += us
            else:
                fz_base.append(0); fz_cap.append(0)
        else:
            la.append(i)
    if allc and n_big == 0:
        s["xxh_forms"] = 1                                               # no row above 64 KiB: the quad form alone (whatever the row count)
    s.update(ext_min_bo=min_bo, ext_max_bend=max_bend, ext_max_oend=max_oend, bx_bytes=s["bx_bytes"] % U64)
    s.update(n_list_a=len(la), n_cand=len(cand_row), n_items=len(item_row), fz_total=len(fz_it) if cand_row else 0)
    s.update(n_tiles=len(tiles), n_big_units=len(big), n_small_tiles=sum(1 for t in tiles if t[1]))
    s.update(bx_nblk=0, bx_slots=0, bx_item_cap=0)
    if s["n_compressed"] and not sw["no_bx"]:
        s["bx_nblk"] = nblk
        if 0 < s["rx_words_small"] <= 256 << 20:                         # few rows above 64 KiB: all of them are resolved
            s["rx_min"], s["rx_words"] = 65537, s["rx_words_small"]
        cap = nblk + nblk // 2 + min(3 * nblk, 65536) + 1024
        if cap < 0x7FFFFFFF:
            s["bx_slots"], s["bx_item_cap"] = s["n_compressed"], cap
    # the resolve path's buffers: a table with batch slots and a row above 64 KiB below 1 GiB, unless the path is switched off
    s["rx_frames"] = int(s["bx_slots"] > 0 and (s["rx_words"] > 0 or s["rx_words_small"] > 0) and not sw["no_rx"])
    s["wide_rows"] = int(n_big > 0 and big_bytes // n_big >= 1 << 20 and big_blob * 50 < big_bytes)
    hints = not sw["no_lean"] and not la
    nst, nt = s["n_small_tiles"], s["n_tiles"]
    s["small_ok"] = int(allc and hints and not sw["no_bx"] and not cand_row and nst == nt and nst > 0 and s["bx_slots"] > 0)
    s["lean_mixed_ok"] = int(hints and not cand_row and 0 < nst < nt)
    s["lean_blocks_ok"] = int(allc and hints and len(cand_row) > 0 and nst == 0)
    s["lean_ok"] = int(allc and hints and not cand_row and not big and nst == nt and nst > 0)
    bt_tile, bt_item = [], []
    if cand_row and not sw["no_fused_blocks"]:                           # a slice tile of 64 leaves is half a block
        base = dict(zip(cand_row, cand_base))
        for ti, t in enumerate(tiles):
            if t[1] == 0 and t[0] in base:
                bt_tile.append(ti); bt_item.append(base[t[0]] + t[2] // 128)
    s["n_bt"] = len(bt_tile)
    s["items_at"] = (max(nt, 16) + 15) // 16 * 16
    s["done"] = s["items_at"] + max(s["n_items"], 16)
    return s, [la, cand_row, cand_base, cand_nb, item_row, item_k, fz_base, fz_cap, fz_it, bt_tile, bt_item]


SHAPE_OUT = ("allc", "n", "n_compressed", "n_list_a", "n_cand", "n_items", "n_bt", "n_small_tiles", "n_tiles", "n_big_units", "fz_total", "fz_bytes", "bx_slots", "bx_item_cap", "bx_bytes",
             "bx_nblk", "rx_words", "rx_words_small", "rx_min", "rx_frames", "xxh_forms", "odd_out", "wide_rows", "ext_min_bo", "ext_max_bend", "ext_max_oend", "ext_wrap", "small_ok", "lean_ok",
             "lean_mixed_ok", "lean_blocks_ok", "done", "items_at")


def tables():
    """(rows, row_begin, use_bitmap, switches) of every table."""
    rng = np.random.default_rng(77)
    out = []

    def table(us_list, stored=(), row_begin=0, use_bitmap=None, oo0=0, sw=None, gap=0, ratio=40):
        rows, bo, oo = [], 1000, oo0
        for i, us in enumerate(us_list):
            comp = 0 if i in stored else 1
            bs = us if not comp else min(max(us // ratio, 9), 1 << 20)
            rows.append((bo % U64, bs, us if comp else us + 5, oo % U64, comp))     # (a stored row's size column is not looked at: the row is its blob)
            bo, oo = bo + bs, oo + us + gap
        out.append((rows, row_begin, int(bool(stored)) if use_bitmap is None else int(use_bitmap), dict(SW0, **(sw or {}))))

    sw_sets = [{}, dict(no_block_items=1), dict(no_fz=1, no_bx=1), dict(no_bx=1), dict(no_fz=1), dict(no_lean=1), dict(no_fused_blocks=1), dict(no_rx=1)]
    for k, sw in enumerate(sw_sets):
        sizes = SIZES if k < 3 else SIZES[:10]                           # (rows of 4 GiB are 65,536 tiles each: under the first three switch sets only)
        table(sizes, sw=sw)                                              # every size once, all compressed
        table(sizes, use_bitmap=2, sw=sw)                                # ... through the bit column, row by row
        table(sizes + [5000, 70000, 300001], stored=(1, 3, 4, 7, len(sizes), len(sizes) + 1), row_begin=3, oo0=5, gap=3, sw=sw)   # stored rows at odd output offsets
    for k in range(12):                                                  # random draws: small rows only, some with one big size
        us = [int(x) for x in rng.choice(SIZES[:4] + [10240, 10240, 4096], size=int(rng.integers(1, 40)))]
        if k % 3 == 0:
            us.insert(int(rng.integers(0, len(us) + 1)), int(rng.choice(SIZES[4:9])))
        table(us, stored=set(int(x) for x in rng.choice(len(us), size=len(us) // 4, replace=False)) if k % 2 else (), row_begin=int(rng.integers(0, 20)), sw=sw_sets[k % len(sw_sets)])
    table([10240] * 30, oo0=U64 - 100_000)                               # output offsets that wrap 2^64
    table([10240] * 30, stored=(4,), oo0=U64 - 100_000, row_begin=9)
    table([4 << 20, 5 << 20], ratio=100)                                 # long copies: frames below 2 % of their content
    table([4 << 20, 5 << 20], ratio=50)                                  # ... and at 2 %
    for ub in (0, 1, 2):                                                 # small rows only: the vectorised pass (0, 1) and the row-by-row one (2)
        table([10240] * 100 + [0, 1, 65536, 4096], use_bitmap=ub)
        table([0], use_bitmap=ub)
    table([10240] * 20 + [200_000, 300_000], stored=(20, 21))            # small rows beside big stored units
    table([])
    # tile plan: 0, 1..64 and 65 leaves; 64 * 64 and 64 * 64 + 1 leaves (the second has grouped CVs); runs of equal lengths whose length
    # sits around the multiples of 64 / leaves
    table([0, 1, 1023, 1024, 1025, 63 * 1024, 64 * 1024, 64 * 1024 + 1, 65 * 1024, 64 * 64 * 1024, 64 * 64 * 1024 + 1, 64 * 64 * 64 * 1024 + 1, 7], sw=dict(no_block_items=1))
    for leaves in (1, 2, 3, 6, 10, 21, 32, 33, 64):
        per = 64 // leaves
        us = []
        for run in sorted({1, 2, per - 1, per, per + 1, 2 * per - 1, 2 * per, 2 * per + 1, 3 * per + 1} - {0}):
            us += [leaves * 1024 - int(rng.integers(0, 3))] * run + [int(rng.choice([1, 5000, 20000, 65 * 1024]))]
        table(us)
        table(us, stored=tuple(range(0, len(us), 5)))
    return out


def test_tables(program):
    ts = tables()
    text = []
    for rows, rb, ub, sw in ts:
        text.append(f"T {len(rows)} {rb} {int(ub)} " + " ".join(str(sw[k]) for k in SW))
        text += [" ".join(map(str, r)) for r in rows]
    out = run(program, "\n".join(text) + "\n").splitlines()
    assert len(out) == 2 * len(ts)
    seen = {k: set() for k in SHAPE_OUT}
    for ti, (rows, rb, ub, sw) in enumerate(ts):
        plan = [int(x) for x in out[2 * ti].split()[1:]]
        shape = [int(x) for x in out[2 * ti + 1].split()[1:]]
        lens = [us if (comp or not ub) else bs for bo, bs, us, oo, comp in rows]                 # (no bit column: every row is compressed)
        tiles, big, n_cv, grp = tile_model(lens)
        nt, nb, ng = plan[0], plan[1], plan[3]
        assert plan[:6] == [len(tiles), len(big), n_cv, len(grp), sum(1 for t in tiles if t[1]), max([b[2] for b in big], default=0)], (ti, plan[:6])
        got_tiles = [plan[6 + 6 * i:12 + 6 * i] for i in range(nt)]
        got_big = [plan[6 + 6 * nt + 4 * i:10 + 6 * nt + 4 * i] for i in range(nb)]
        got_grp = [tuple(plan[6 + 6 * nt + 4 * nb + 2 * i:8 + 6 * nt + 4 * nb + 2 * i]) for i in range(ng)]
        assert got_tiles == tiles and got_big == big and got_grp == grp, ti
        # every unit is covered exactly once and in order, no tile holds more than 64 units or leaves, CV indices are dense
        at, cv = 0, 0
        for t in got_tiles:
            assert t[3] <= 64 and t[1] <= 64, (ti, t)
            if t[1]:
                assert t[0] == at, (ti, t)
                at += t[1]
            else:
                assert t[0] == at and t[4] == cv and t[2] % 64 == 0, (ti, t)
                cv += 1
                at += int(t[2] + t[3] == max((lens[t[0]] + 1023) // 1024, 1))
        assert at == len(rows) and cv == n_cv, ti
        want, lists = shape_model(rows, rb, ub, sw, tiles, big)
        for j, k in enumerate(SHAPE_OUT):
            assert shape[j] == want[k], (ti, k, shape[j], want[k], sw)
            seen[k].add(shape[j])
        rest = shape[len(SHAPE_OUT):]
        assert rest == [x for v in lists for x in (len(v), weighted(v))], (ti, rest)
    for k in SHAPE_OUT:
        assert len(seen[k]) >= 2, k                                      # the tables reach both sides of every rule
    # the vectorised all-compressed pass and the row-by-row one agree in everything but the shapes only an all-compressed table has
    same = [j for j, k in enumerate(SHAPE_OUT) if k not in ("allc", "small_ok", "lean_ok", "lean_blocks_ok")]
    pairs = [(a, b) for a in range(len(ts)) for b in range(len(ts)) if ts[a][2] == 0 and ts[b][2] == 2 and ts[a][0] == ts[b][0] and ts[a][3] == ts[b][3] and len(ts[a][0]) > 1]
    assert pairs
    for a, b in pairs:
        fa, fb = out[2 * a + 1].split()[1:], out[2 * b + 1].split()[1:]
        assert [fa[j] for j in same] == [fb[j] for j in same] and fa[len(SHAPE_OUT):] == fb[len(SHAPE_OUT):] and out[2 * a] == out[2 * b], (a, b)


# ---- verdicts and pool sizes ----------------------------------------------------------------------------------------------------------

E_CORRUPT, E_DST_SMALL = -5, -4


def test_codes():
    text = open(os.path.join(ROOT, "include", "znippy_hip.h")).read()
    import re
    assert int(re.search(r"#define ZNIPPY_E_CORRUPT \((-?\d+)\)", text).group(1)) == E_CORRUPT
    assert int(re.search(r"#define ZNIPPY_E_DST_SMALL \((-?\d+)\)", text).group(1)) == E_DST_SMALL


def test_verdicts(program):
    edge = [0, 1, 2 ** 32, U64 - 1]
    rows = [(bo, bs, ln, oo) for bo in edge + [U64 - 2 ** 32] for bs in edge for ln in (0, 1, 2 ** 32, U64 - 1) for oo in (0, 1, U64 - 1)]
    lines, want = [], []
    for base, bcap, ocap, verify in itertools.product(edge, edge, edge, (0, 1)):
        for chunk in (rows, rows[:1], [(max(base, 1), 0, 0, 0)], []):
            lines.append(f"V {base} {bcap} {ocap} {verify} {len(chunk)}")
            lines += [" ".join(map(str, r)) for r in chunk]
            codes = []
            for bo, bs, ln, oo in chunk:
                if bo < base or (bcap != U64 - 1 and bo - base + bs > bcap):      # the blob is not inside the declared region (2^64 - 1: not declared)
                    codes.append(E_CORRUPT)
                elif not verify and oo + ln > ocap:                                 # its bytes would not land inside the output region
                    codes.append(E_DST_SMALL)
                else:
                    codes.append(0)
            bad = sum(1 for x in codes if x)
            # the table's extents answer for all rows at once: no sum wraps, and the extreme ends lie inside the regions
            wrap = any(bo + bs >= U64 or oo + ln >= U64 for bo, bs, ln, oo in chunk)
            fit = not wrap and (not chunk or (min(r[0] for r in chunk) >= base and (bcap == U64 - 1 or max(r[0] + r[1] for r in chunk) - base <= bcap) and
                                              (verify or max(r[3] + r[2] for r in chunk) <= ocap)))
            want.append((bad, codes, fit))
    got = run(program, "\n".join(lines) + "\n").splitlines()
    assert len(got) == len(want)
    n_fit = 0
    for g, (bad, codes, fit) in zip(got, want):
        g = [int(x) for x in g.split()]
        assert g[1] == bad and g[0] == int(fit), (g[:3], bad, fit)
        assert g[3:] == (codes if bad else []), g[:3]                      # every row the model calls bad carries the model's code
        assert not (g[0] and bad), "a table that fits has no bad row"
        n_fit += g[0]
    assert n_fit > 0


def test_pool_sizes(program):
    CAP = 16 << 30
    RX_CAP = 2 ** 31 - 2 ** 20
    cases = []
    for content in (0, 1, 7, 8, 4096, CAP - 4097, CAP - 4096, CAP - 4095, 2 * CAP // 3 - 2731, 2 * CAP // 3 - 2730, 2 * CAP, 2 * CAP + 1, CAP):
        for items in (0, 1, 1000):
            cases.append((content, items, content, content, 0))
    for words in (0, 1, 1023, 1024, 1025, RX_CAP - 1, RX_CAP, RX_CAP + 1, 2 ** 40):
        cases.append((0, 0, words, 0, 0))
    for b in (0, 1, CAP - 1, CAP, CAP + 1):
        for other in (0, 4096, 8192, 8193, CAP):
            cases.append((0, 0, 0, b, other))
    got = [[int(x) for x in line.split()] for line in run(program, "".join("S %d %d %d %d %d\n" % c for c in cases)).splitlines()]
    REFUSED = U64 - 1
    for (content, items, words, b, other), g in zip(cases, got):
        lit = min(content + 80 * items + 4096, CAP)                       # the content bytes + 80 bytes of slack per item, capped
        seq = min(content * 3 // 2 + 4096, CAP) // 8                      # 1.5 bytes of pool per content byte, in 8-byte records
        tab = min(content // 2 + 64 * items + 4096, CAP)                  # half a byte of each table pool per content byte + 64 per item
        want = [lit, seq, tab // 2 + 160, tab // 2, min((words + 1023) // 1024 * 1024, RX_CAP),
                0 if not b else (REFUSED if b > CAP else b + 4096),
                0 if not b else (REFUSED if b > CAP or b + other > CAP + 8192 else b + 4096)]
        assert g == want, ((content, items, words, b, other), g, want)
