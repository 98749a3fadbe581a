"""The host side of the gunzip cut at block starts (znippy_amd/csrc/host/gz_cut_plan.cc) as stand-alone host programs under
AddressSanitizer and UBSan: the grid rule against the model, slot lists and probe records as a device that searched and decoded
untrusted input could leave them, the contradictory ones included, and the passes under a budget.  Every case gives a count or a status, never a sanitizer report; the arrays the program hands
over are heap copies of exactly what is named, so a read past them is caught."""
import os
import shutil
import subprocess

import pytest

import gz_cut_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "znippy_amd", "csrc", "host")
NONE = (1 << 64) - 1
E_NOMEM = -3

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gz_cut_plan.h"
// stdin: cases.  "P cut n" and n source lengths, then m and m slot values (m must be the plan's slot count, or 0 for none):
//   -> "rc items slots tested chunks kept | item_of slot_base ..."   and exit code 3 where the plan contradicts itself
int main() {
    unsigned long long cut; size_t n;
    while (scanf(" P %llu %zu", &cut, &n) == 2) {
        zn::GzItem *items = (zn::GzItem *)malloc(n ? n * sizeof(zn::GzItem) : 1);
        for (size_t i = 0; i < n; i++) {
            unsigned len;
            if (scanf("%u", &len) != 1) return 2;
            items[i] = zn::GzItem{(const uint8_t *)(uintptr_t)(0x1000 + 16 * i), nullptr, len, 0, 0, 0};
        }
        gzcut::FindPlan p;
        p.tested = 99;  // (what an earlier call left: must go)
        const int rc = gzcut::find_plan(items, n, cut, p);
        size_t m;
        if (scanf("%zu", &m) != 1) return 2;
        uint64_t *slots = (uint64_t *)malloc(m ? m * sizeof(uint64_t) : 1);
        for (size_t i = 0; i < m; i++) { unsigned long long v; if (scanf("%llu", &v) != 1) return 2; slots[i] = v; }
        // the plan against itself: slots back to back, every chunk inside its item, the chunks of an item cover it once
        uint64_t base = 0, chunk = 0;
        for (size_t f = 0; f < p.items.size(); f++) {
            const gzcut::FindItem &it = p.items[f];
            if (it.slot_base != base || p.item_of[f] >= n || items[p.item_of[f]].src != it.src || items[p.item_of[f]].src_len != it.src_len) return 3;
            base += (it.src_len + cut - 1) / cut;
            for (uint64_t off = 0; off < it.src_len; off += gzcut::FIND_CHUNK, chunk++)
                if (chunk >= p.chunks.size() || p.chunks[chunk].item != f || p.chunks[chunk].off != off) return 3;
        }
        if (base != p.n_slots || chunk != p.chunks.size() || p.item_of.size() != p.items.size()) return 3;
        if (m && m != p.n_slots) return 2;
        const uint64_t kept = m ? gzcut::count_kept(p, slots, cut) : 0;
        printf("%d %zu %" PRIu64 " %" PRIu64 " %zu %" PRIu64 " |", rc, p.items.size(), p.n_slots, p.tested, p.chunks.size(), kept);
        for (size_t f = 0; f < p.items.size(); f++) printf(" %u %" PRIu64, p.item_of[f], p.items[f].slot_base);
        printf("\n");
        free(slots);
        free(items);
    }
    return 0;
}
"""


def build(tmp_path_factory, name, defines=()):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp(name)
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "plan"
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   list(defines) + ["-I", HOST, str(main), os.path.join(HOST, "gz_cut_plan.cc"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory, "gz_cut_plan")


def plan(program, cut, lens, slots=()):
    """-> (rc, searched items, slots, tested, chunks, kept, [(item_of, slot_base)])"""
    text = "P %d %d\n%s\n%d %s\n" % (cut, len(lens), " ".join(map(str, lens)), len(slots), " ".join(map(str, slots)))
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    head, rest = r.stdout.split("|")
    v = [int(x) for x in rest.split()]
    return tuple(int(x) for x in head.split()) + (list(zip(v[::2], v[1::2])),)


def test_grid(program):
    # off, and values that are no valid cut, search nothing
    for cut in (0, 1, 63, (1 << 30) + 1):
        assert plan(program, cut, [1 << 20, 5]) == (0, 0, 0, 0, 0, 0, [])
    # items below 2 * cut are not searched; the others take ceil(len / cut) slots and a chunk per 4096 bytes, in item order
    lens = [0, 127, 128, 129, 4096, 4097, 100_000, 127]
    want_items = [(k, n) for k, n in enumerate(lens) if M.searched(n, 64)]
    rc, n_items, n_slots, tested, chunks, kept, where = plan(program, 64, lens)
    assert rc == 0 and n_items == len(want_items) == 5 and kept == 0
    assert n_slots == sum(-(-n // 64) for _, n in want_items) and tested == 8 * sum(n for _, n in want_items)
    assert chunks == sum(-(-n // 4096) for _, n in want_items)
    assert [k for k, _ in where] == [k for k, _ in want_items]
    # the largest item and the largest cut
    assert plan(program, 1 << 30, [(1 << 32) - 1, (1 << 31) - 1])[:5] == (0, 1, 4, 8 * ((1 << 32) - 1), 1 << 20)
    assert plan(program, 64, [])[:5] == (0, 0, 0, 0, 0)


def test_slots_are_not_trusted(program):
    cut, lens = 64, [200, 100, 130]                       # searched: item 0 (4 slots, the last of 8 bytes) and item 2 (3 slots, the last of 2 bytes)
    def kept(slots):
        return plan(program, cut, lens, slots)[5]
    assert kept([NONE] * 7) == 0
    good = [8 * 0 + 3, 8 * 127 + 7, NONE, 8 * 199 + 7, 8 * 63, NONE, 8 * 129]
    assert kept(good) == 5
    # the model's grid rule over the same positions
    assert len(M.kept([3, 8 * 127 + 7, 8 * 199 + 7], 200, cut)) + len(M.kept([8 * 63, 8 * 129], 130, cut)) == 5
    bad = [8 * 64,            # the next window's position
           8 * 63 + 7,        # the window in front
           0,                 # byte 0 in window 2
           8 * 200,           # the first byte behind the item
           NONE - 1,          # nearly NONE: a byte far behind the item
           8 * 130,           # behind item 2, inside its last window's span
           1 << 63]
    assert kept(bad) == 0
    for i, v in enumerate(bad):                            # each on its own among good ones
        assert kept(good[:i] + [v] + good[i + 1:]) == 5 - (good[i] != NONE)


def test_limits(tmp_path_factory):
    small = build(tmp_path_factory, "gz_cut_plan_small", ["-DZN_GZ_CUT_SLOTS_MAX=10"])
    assert plan(small, 64, [640])[:3] == (0, 1, 10)
    assert plan(small, 64, [641]) == (E_NOMEM, 0, 0, 0, 0, 0, [])             # 11 slots
    assert plan(small, 64, [320, 100, 321]) == (E_NOMEM, 0, 0, 0, 0, 0, [])   # 5 + 6
    assert plan(small, 1 << 20, [11 * 4096])[:1] == (0,)                      # below 2 * cut: not searched
    assert plan(small, 4096, [10 * 4096 + 1]) == (E_NOMEM, 0, 0, 0, 0, 0, []) # 11 chunks and 11 slots


# ---- the plan of the cut: records as a device that decoded untrusted input could leave them ------------------------------------------

MAIN_CUT = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gz_cut_plan.h"
// stdin: cases.  "C src_len room budget n" and n lines "first bit start_bit end_bit out end_kind status reach crc isize next"
//   -> "ok crc out_len | marker start_bit out_off out_len ... | passes as piece0 piece1 group0 group1 ... | groups ... | sym_off ..."
int main() {
    unsigned long long src_len, room, budget; size_t n;
    while (scanf(" C %llu %llu %llu %zu", &src_len, &room, &budget, &n) == 4) {
        gzcut::CutCand *cands = (gzcut::CutCand *)malloc(n ? n * sizeof(gzcut::CutCand) : 1);
        gzcut::CutRec *recs = (gzcut::CutRec *)malloc(n ? n * sizeof(gzcut::CutRec) : 1);
        for (size_t i = 0; i < n; i++) {
            unsigned long long bit, start, end, out;
            gzcut::CutCand &c = cands[i]; gzcut::CutRec &r = recs[i];
            if (scanf("%u %llu %llu %llu %llu %u %d %u %u %u %d", &c.first, &bit, &start, &end, &out, &r.end_kind, &r.status, &r.reach, &r.crc, &r.isize, &r.next) != 11) return 2;
            c.item = 3; c.bit = bit; c.stop0 = c.stop1 = 0; r.start_bit = start; r.end_bit = end; r.out = out;
        }
        std::vector<gzcut::CutPiece> pieces(1, gzcut::CutPiece{77, 0, 7, 7, 7, 7});  // (what other items left: must stay)
        std::vector<gzcut::CutItemPlan> plans;
        std::vector<gzcut::CutMember> mems(1, gzcut::CutMember{77, 7, 7, 7});
        const bool ok = gzcut::plan_cut(cands, recs, n, 3, src_len, room, budget, pieces, mems, plans);
        free(cands); free(recs);
        if (pieces[0].item != 77 || mems[0].item != 77 ||
            (ok ? plans.size() != 1 || plans[0].piece0 != 1 || plans[0].piece1 != pieces.size() || plans[0].member0 != 1 || plans[0].member1 != mems.size() ||
                      plans[0].members != mems.size() - 1
                : pieces.size() != 1 || mems.size() != 1 || !plans.empty())) return 3;
        // the members' pieces are consecutive and cover the item's pieces once; the crc printed is the sum of theirs
        uint32_t crcs = 0;
        for (size_t m = 1, at = 1; m < mems.size(); m++) {
            if (mems[m].item != 3 || mems[m].piece0 != at || mems[m].piece1 <= at || mems[m].piece1 > pieces.size() || pieces[mems[m].piece0].marker) return 3;
            at = mems[m].piece1;
            crcs += mems[m].crc;
            if (m + 1 == mems.size() && at != pieces.size()) return 3;
        }
        printf("%d %u %" PRIu64 " |", ok ? 1 : 0, crcs, ok ? plans[0].out_len : 0);
        uint64_t sum = 0;
        for (size_t p = 1; p < pieces.size(); p++) {
            if (pieces[p].item != 3 || pieces[p].out_off != sum || sum + pieces[p].out_len > room) return 3;
            sum += pieces[p].out_len;
            printf(" %u %" PRIu64 " %u %u", pieces[p].marker, pieces[p].start_bit, pieces[p].out_off, pieces[p].out_len);
        }
        if (ok && sum != plans[0].out_len) return 3;
        pieces.erase(pieces.begin());
        std::vector<gzcut::CutPass> passes; std::vector<gzcut::CutGroup> groups;
        gzcut::make_passes(pieces, budget, passes, groups);
        printf(" |");
        size_t at = 0, g = 0;
        for (const gzcut::CutPass &ps : passes) {
            // passes and groups are consecutive and cover the pieces once; the marker pieces of a pass lie back to back inside the budget
            if (ps.piece0 != at || ps.piece1 <= ps.piece0 || ps.group0 != g || ps.group1 <= ps.group0) return 3;
            uint64_t used = 0;
            for (size_t p = ps.piece0; p < ps.piece1; p++)
                if (pieces[p].marker) { if (pieces[p].sym_off != used || pieces[p].out_len > budget - used) return 3; used += pieces[p].out_len; }
            size_t gp = ps.piece0;
            for (size_t k = ps.group0; k < ps.group1; k++) { if (groups[k].piece0 != gp || groups[k].piece1 <= gp) return 3; gp = groups[k].piece1; }
            if (gp != ps.piece1) return 3;
            at = ps.piece1; g = ps.group1;
            printf(" %zu %zu", ps.piece0, ps.piece1);
        }
        if (at != pieces.size() || g != groups.size()) return 3;
        printf("\n");
    }
    return 0;
}
"""
BOUNDARY, TRAILER, ERROR, ROOM = 0, 1, 2, 3
NEXT_MEMBER, NEXT_END = 0, 1


@pytest.fixture(scope="module")
def cut_program(tmp_path_factory):
    global MAIN
    keep, MAIN = MAIN, MAIN_CUT
    try:
        return build(tmp_path_factory, "gz_cut_plan_pieces")
    finally:
        MAIN = keep


def rec(bit, end_kind, end_bit=0, out=0, reach=0, status=0, crc=0, isize=None, next=NEXT_END, first=None, start=None):
    first = (bit == 0) if first is None else first
    return (int(first), bit, (80 if first else bit) if start is None else start, end_bit, out, end_kind, status, reach, crc, isize, next)


def plan_cut(program, src_len, room, recs, budget=1 << 30):
    """-> (ok, crc, out_len, [pieces as (marker, start_bit, out_off, out_len)], [passes as (piece0, piece1)])"""
    total = sum(r[4] for r in recs)
    recs = [r[:9] + ((total & 0xFFFFFFFF) if r[9] is None else r[9],) + r[10:] for r in sorted(recs, key=lambda r: (r[1], r[0]))]
    text = "C %d %d %d %d\n" % (src_len, room, budget, len(recs)) + "".join(" ".join(str(v) for v in r) + "\n" for r in recs)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    head, pieces, passes = r.stdout.split("|")
    v, w = [int(x) for x in pieces.split()], [int(x) for x in passes.split()]
    ok, crc, out_len = (int(x) for x in head.split())
    return bool(ok), crc, out_len, [tuple(v[i:i + 4]) for i in range(0, len(v), 4)], list(zip(w[::2], w[1::2]))


def refused(program, src_len, room, recs, budget=1 << 30):
    assert plan_cut(program, src_len, room, recs, budget)[:4] == (False, 0, 0, [])


def test_plan_cut_chain(cut_program):
    # three pieces: the first into place, one that reaches back (a marker piece), one that reaches nowhere; a false candidate at 3000
    # whose record says garbage, and one the chain never lands on
    recs = [rec(0, BOUNDARY, 2001, out=1000), rec(2001, BOUNDARY, 4003, out=50_000, reach=700), rec(4003, TRAILER, 8000, out=30, crc=5),
            rec(3000, ERROR, status=-5, out=17), rec(5000, BOUNDARY, 100, out=1 << 40, reach=70_000)]
    recs = [r if r[9] is not None else r[:9] + (51_030,) + r[10:] for r in recs]
    assert plan_cut(cut_program, 1000, 51_030, recs) == (True, 5, 51_030, [(0, 80, 0, 1000), (1, 2001, 1000, 50_000), (0, 4003, 51_000, 30)], [(0, 3)])
    refused(cut_program, 1000, 51_029, recs)                       # the room one byte short: left to the stages behind, which say so
    # budgets: one that holds the marker piece exactly, one a symbol short
    assert plan_cut(cut_program, 1000, 51_030, recs, budget=50_000)[0]
    # ... a symbol short: the piece joins the run in front of it, which is decoded into place and holds its reach
    assert plan_cut(cut_program, 1000, 51_030, recs, budget=49_999)[3] == [(0, 80, 0, 51_000), (0, 4003, 51_000, 30)]
    # an empty piece counts
    recs = [rec(0, BOUNDARY, 500, out=10), rec(500, BOUNDARY, 600, out=0), rec(600, TRAILER, 8000, out=5, reach=3, crc=9)]
    assert plan_cut(cut_program, 1000, 15, recs)[3] == [(0, 80, 0, 10), (0, 500, 10, 0), (1, 600, 10, 5)]


def test_plan_cut_passes(cut_program):
    # budgets that force one marker piece per pass; pieces into place ride along
    recs = [rec(0, BOUNDARY, 1000, out=100)] + [rec(1000 * k, BOUNDARY, 1000 * (k + 1), out=100, reach=(k & 1) * 50) for k in range(1, 9)]
    recs.append(rec(9000, TRAILER, 16_000, out=100, reach=1))
    ok, _, out_len, pieces, passes = plan_cut(cut_program, 2000, 1000, recs, budget=100)
    assert ok and out_len == 1000 and [p[0] for p in pieces] == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert passes == [(0, 3), (3, 5), (5, 7), (7, 9), (9, 10)]
    assert plan_cut(cut_program, 2000, 1000, recs, budget=250)[4] == [(0, 5), (5, 9), (9, 10)]
    assert plan_cut(cut_program, 2000, 1000, recs)[4] == [(0, 10)]


def test_plan_cut_contradictions(cut_program):
    ok = rec(0, BOUNDARY, 2000, out=10)
    end = rec(2000, TRAILER, 8000, out=5)
    assert plan_cut(cut_program, 1000, 100, [ok, end])[0]
    cases = [
        [],                                                                      # no record at all
        [rec(80, TRAILER, 8000, out=1, first=False)],                            # none at byte 0
        [rec(0, TRAILER, 8000, out=1, first=False)],                             # byte 0 is no member start
        [ok],                                                                    # the chain lands where no record is
        [ok, rec(2000, BOUNDARY, 2000, out=1)],                                  # an end that is its own start
        [ok, rec(2000, BOUNDARY, 1000, out=1), rec(1000, BOUNDARY, 2000, out=1)],  # a cycle
        [ok, rec(2000, BOUNDARY, 8000, out=1)],                                  # an end at the source's end
        [ok, rec(2000, BOUNDARY, 1 << 62, out=1)],                               # ... far behind it
        [rec(0, BOUNDARY, 0, out=1, start=80)],                                  # an end in front of the first block
        [ok, rec(2000, TRAILER, 8000, out=5, next=NEXT_MEMBER)],                 # another member at the source's end
        [ok, rec(2000, TRAILER, 4000, out=5, next=NEXT_MEMBER, isize=5)],        # ... where no record is
        [ok, rec(2000, TRAILER, 4000, out=5, next=NEXT_MEMBER, isize=5), rec(4000, TRAILER, 8000, out=1, isize=1)],  # ... where a block candidate is
        [ok, rec(2000, TRAILER, 2000, out=5, next=NEXT_MEMBER, isize=5)],        # ... at the piece's own start
        [ok, rec(2000, TRAILER, 8000, out=5, next=-5)],                          # garbage behind the trailer
        [ok, rec(2000, TRAILER, 8000, out=5, isize=14)],                         # ISIZE is not the size
        [ok, rec(2000, ERROR, status=-5, out=3)], [ok, rec(2000, ERROR, out=3)], [ok, rec(2000, ROOM, out=3)], [ok, rec(2000, 9, 8000, out=3)],
        [ok, rec(2000, TRAILER, 8000, out=5, status=-5)],                        # a status beside an end
        [rec(0, TRAILER, 8000, out=5, reach=1)],                                 # the first piece reaches back
        [ok, rec(2000, TRAILER, 8000, out=5, reach=11)],                         # a reach beyond the member's first byte
        [rec(0, BOUNDARY, 2000, out=40_000), rec(2000, TRAILER, 8000, out=5, reach=32_769)],  # a distance DEFLATE has not
        [ok, rec(2000, TRAILER, 8000, out=5, start=2001)],                       # a block candidate whose piece starts elsewhere
        [rec(0, TRAILER, 8000, out=5, start=8000)],                              # a first block at the source's end
        [rec(0, BOUNDARY, 2000, out=(1 << 64) - 1)], [ok, rec(2000, TRAILER, 8000, out=(1 << 64) - 5)],  # counts that overflow
        [rec(0, TRAILER, 8000, out=1 << 32, isize=0)],                           # a piece of 4 GiB
    ]
    for recs in cases:
        refused(cut_program, 1000, 100 if not recs or recs[0][4] < 1 << 20 else 1 << 33, recs)


def test_plan_cut_members_and_joins(cut_program):
    M = lambda bit, *a, **k: rec(bit, *a, first=True, start=bit + 80, **k)   # noqa: E731
    # three members, the second empty, a block candidate and a flush candidate inside the third; reaches count from the member's first byte
    recs = [rec(0, BOUNDARY, 1000, out=100, isize=0), rec(1000, TRAILER, 2000, out=50, reach=100, isize=150, crc=1, next=NEXT_MEMBER),
            M(2000, TRAILER, 3000, out=0, isize=0, crc=2, next=NEXT_MEMBER),
            M(3000, BOUNDARY, 4000, out=10, isize=0), rec(4000, BOUNDARY, 5000, out=20, reach=10, isize=0), rec(5000, TRAILER, 8000, out=5, isize=35, crc=4)]
    ok, crcs, out_len, pieces, passes = plan_cut(cut_program, 1000, 185, recs)
    assert ok and crcs == 7 and out_len == 185
    assert pieces == [(0, 80, 0, 100), (1, 1000, 100, 50), (0, 2080, 150, 0), (0, 3080, 150, 10), (1, 4000, 160, 20), (0, 5000, 180, 5)]
    # a reach of 11 in the third member is in front of its first byte, whatever the members in front hold
    refused(cut_program, 1000, 185, recs[:4] + [rec(4000, BOUNDARY, 5000, out=20, reach=11, isize=0)] + recs[5:])
    # the wrong ISIZE of a member in the middle; a member record the chain reaches through a block boundary
    refused(cut_program, 1000, 185, recs[:2] + [M(2000, TRAILER, 3000, out=0, isize=1, crc=2, next=NEXT_MEMBER)] + recs[3:])
    refused(cut_program, 1000, 185, [rec(0, BOUNDARY, 2000, out=150, isize=0)] + recs[2:])
    # joins: a piece above the budget takes the pieces in front of it along until one decoded into place holds every reach
    recs = [rec(0, BOUNDARY, 1000, out=100, isize=0), rec(1000, BOUNDARY, 2000, out=10, isize=0), rec(2000, BOUNDARY, 3000, out=10, reach=50, isize=0),
            rec(3000, BOUNDARY, 4000, out=5, isize=0), rec(4000, BOUNDARY, 5000, out=300, reach=2, isize=0), rec(5000, TRAILER, 8000, out=7, reach=1, isize=432)]
    assert plan_cut(cut_program, 1000, 432, recs)[3] == [(0, 80, 0, 100), (0, 1000, 100, 10), (1, 2000, 110, 10), (0, 3000, 120, 5), (1, 4000, 125, 300), (1, 5000, 425, 7)]
    # budget 299: the piece of 300 joins the piece of 5 in front of it, which holds its reach of 2
    assert plan_cut(cut_program, 1000, 432, recs, budget=299)[3] == [(0, 80, 0, 100), (0, 1000, 100, 10), (1, 2000, 110, 10), (0, 3000, 120, 305), (1, 5000, 425, 7)]
    # ... with a reach of 6 it does not: the marker piece in front cannot head a run, so everything back to the piece at 1000 joins —
    # and that piece must hold the marker piece's reach of 50 as well, which it does not: the member's first piece takes them all
    far = recs[:4] + [rec(4000, BOUNDARY, 5000, out=300, reach=6, isize=0)] + recs[5:]
    assert plan_cut(cut_program, 1000, 432, far, budget=299)[3] == [(0, 80, 0, 425), (1, 5000, 425, 7)]
    # a budget below every marker piece: two runs, the second headed by the one piece behind the first that reaches nowhere
    assert plan_cut(cut_program, 1000, 432, recs, budget=1)[3] == [(0, 80, 0, 120), (0, 3000, 120, 312)]
