"""The host planning of znippy_bunzip2_batch (znippy_amd/csrc/host/bz_plan.cc) as a stand-alone host program under AddressSanitizer
and UBSan.  The records it reads come from device memory that decoded untrusted input, so the cases here are hand-written records,
the contradictory ones included: every case must give the expected plan or a status, never a sanitizer report.  The program plays
the passes the way api.hip does — choose, the records of the chosen jobs, advance, fold_crc — with heap copies of exactly the records
of a pass, so a read past them is caught."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "znippy_amd", "csrc", "host")
E_INVAL, E_NOMEM, E_DST_SMALL, E_CORRUPT, E_UNSUPPORTED, E_CHECKSUM = -1, -3, -4, -5, -6, -7
HEAD, BLOCK = 0, 1
NEXT_BLOCK, NEXT_END = 0, 1
BZH = 0x685A42

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "bz_plan.h"
using namespace zn;
struct Known { uint32_t kind; uint64_t pos; BzRec r; uint32_t crc_ok; };
// stdin: cases.
// "P src_len room measure slot_cap n_raw n_known", n_raw values (item << 36 | bit, any order: item 1 is the one under test, item 0 and 2
// are empty streams beside it) and n_known lines "kind pos status next end_bit after n level block_crc stream_crc tail tail_len out_len
// orig crc_ok": a job without a line gets a record that failed (what a false candidate leaves)
//   -> "status out_len streams blocks passes L slot out_off out_len ..."
// "A out_cap n" and n lines "src_off src_len room" (src_cap 1000, packed rooms) -> the statuses, then items, chunks, cand_total
int main() {
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'P') {
            unsigned long long src_len, room, slot_cap; unsigned measure; size_t n_raw, n_known;
            if (scanf("%llu %llu %u %llu %zu %zu", &src_len, &room, &measure, &slot_cap, &n_raw, &n_known) != 6) return 2;
            BzBatch b;
            b.measure = measure != 0;
            const uint8_t empty[14] = {0};
            b.items.push_back(BzItem{empty, nullptr, 14, 0});
            b.items.push_back(BzItem{empty, nullptr, (uint32_t)src_len, (uint32_t)room});
            b.items.push_back(BzItem{empty, nullptr, 14, 0});
            b.raw.resize(n_raw);
            for (size_t i = 0; i < n_raw; i++) { unsigned long long v; if (scanf("%llu", &v) != 1) return 2; b.raw[i] = v; }
            std::vector<Known> known(n_known);
            for (auto &k : known) {
                unsigned long long pos, end_bit, after;
                if (scanf("%u %llu %d %u %llu %llu %u %u %u %u %u %u %u %u %u", &k.kind, &pos, &k.r.status, &k.r.next, &end_bit, &after, &k.r.n, &k.r.level,
                          &k.r.block_crc, &k.r.stream_crc, &k.r.tail, &k.r.tail_len, &k.r.out_len, &k.r.orig, &k.crc_ok) != 15) return 2;
                k.pos = pos; k.r.end_bit = end_bit; k.r.after = after;
            }
            bz_start(b, n_raw);
            if (b.chains.size() != 3) return 3;
            unsigned passes = 0;
            std::vector<BzLand> all;
            while (bzp::choose(b.chains, (size_t)slot_cap, b.jobs, b.first_job)) {
                if (b.jobs.size() > bz_jobs_max(b, (size_t)slot_cap) || ++passes > 1000) return 3;
                BzRec *recs = (BzRec *)malloc(b.jobs.size() * sizeof(BzRec));
                size_t next_slot = 0;  // block jobs take the slots 0, 1, ... below slot_cap; a header job takes none
                for (size_t j = 0; j < b.jobs.size(); j++) {
                    if (b.jobs[j].kind == bzp::K_BLOCK ? b.jobs[j].slot != next_slot++ || b.jobs[j].slot >= slot_cap : b.jobs[j].slot != 0) return 3;
                    BzRec r;
                    memset(&r, 0, sizeof r);
                    r.status = BZ_E_CORRUPT;
                    if (b.jobs[j].item != 1) {  // the empty streams beside: a header, the end magic behind it
                        if (b.jobs[j].kind != bzp::K_HEAD || b.jobs[j].pos != 0) return 3;
                        r.status = 0; r.next = bzp::NEXT_END; r.level = 9; r.after = 14;
                    }
                    for (const auto &k : known)
                        if (b.jobs[j].item == 1 && k.kind == b.jobs[j].kind && k.pos == b.jobs[j].pos) r = k.r;
                    recs[j] = r;
                }
                b.lands.clear();
                bzp::advance(b.chains, b.jobs, b.first_job, recs, b.lands);
                free(recs);
                uint32_t *got = (uint32_t *)malloc(b.lands.size() * sizeof(uint32_t) + 1);
                for (size_t l = 0; l < b.lands.size(); l++) {
                    const BzLand &ld = b.lands[l];
                    if (ld.item != 1 || ld.slot >= slot_cap || (uint64_t)ld.out_off + ld.out_len > room) return 3;
                    got[l] = ld.crc;
                    for (const auto &job : b.jobs)
                        for (const auto &k : known)
                            if (job.kind == bzp::K_BLOCK && job.slot == ld.slot && k.kind == bzp::K_BLOCK && k.pos == job.pos && !k.crc_ok) got[l] ^= 1;
                    all.push_back(ld);
                }
                bzp::fold_crc(b.chains, b.lands, got);
                free(got);
            }
            for (int k = 0; k < 3; k += 2)
                if (!b.chains[k].done || bzp::verdict(b.chains[k]) != 0 || b.chains[k].streams != 1 || b.chains[k].out != 0) return 3;
            const bzp::Chain &c = b.chains[1];
            if (!c.done) return 3;
            const int st = bzp::verdict(c);
            printf("%d %" PRIu64 " %u %u %u L", st, st ? 0 : c.out, st ? 0 : c.streams, st ? 0 : c.blocks, passes);
            for (const auto &ld : all) printf(" %u %u %u", ld.slot, ld.out_off, ld.out_len);
            printf("\n");
        } else if (what == 'A') {
            unsigned long long out_cap; size_t n;
            if (scanf("%llu %zu", &out_cap, &n) != 2) return 2;
            std::vector<uint64_t> so(n), sl(n), room(n), ol(n, 99);
            std::vector<uint32_t> streams(n, 99), blocks(n, 99);
            for (size_t i = 0; i < n; i++) { unsigned long long a, c, d; if (scanf("%llu %llu %llu", &a, &c, &d) != 3) return 2; so[i] = a; sl[i] = c; room[i] = d; }
            uint8_t *const src = (uint8_t *)0x1000, *const dst = (uint8_t *)0x100000;  // (device addresses: only added to)
            BzBatch b;
            const BzCall call{src, 1000, so.data(), sl.data(), n, out_cap ? dst : nullptr, out_cap, nullptr, room.data(), ol.data(), streams.data(), blocks.data()};
            const int rc = bz_admit(call, b);
            printf("%d", rc);
            for (size_t i = 0; i < n; i++) printf(" %d", b.st[i]);
            uint64_t bound = 0;
            for (const auto &it : b.items) bound += 8ull * it.src_len / 45 + 1;
            if (rc == 0 && bound != b.cand_total) return 3;
            for (size_t i = 0; i < n; i++) if (ol[i] || streams[i] || blocks[i]) return 3;
            printf(" I %zu %zu %" PRIu64 " S %zu %zu %zu\n", b.items.size(), b.chunks.size(), b.cand_total, bz_slots(b, 0, 1ull << 30), bz_slots(b, 3, 0),
                   bz_slots(b, 0, BZ_SLOT_BYTES - 1));
        } else return 2;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("bz_plan")
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "plan"
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", HOST, str(main)] + [os.path.join(HOST, f) for f in ("bz_plan.cc", "deflate_batch.cc", "gz_plan.cc", "range_plan.cc")] +
                   ["-o", str(exe)], check=True)
    return str(exe)


def head(pos=0, level=1, next=NEXT_BLOCK, status=0, after=0, stream_crc=0, tail=0, tail_len=0):
    return (HEAD, pos, status, next, 8 * pos + 32, after, 0, level, 0, stream_crc, tail, tail_len, 0, 0, 1)


def block(pos, end_bit, n=1000, out_len=1200, crc=7, next=NEXT_BLOCK, status=0, after=0, stream_crc=0, tail=0, tail_len=0, orig=0, crc_ok=1):
    return (BLOCK, pos, status, next, end_bit, after, n, 0, crc, stream_crc, tail, tail_len, out_len, orig, crc_ok)


def fold(crcs):
    c = 0
    for x in crcs:
        c = (((c << 1) | (c >> 31)) & 0xFFFFFFFF) ^ x
    return c


def plan(program, src_len, room, cands, recs, slot_cap=1000, measure=0, item=1):
    """-> (status, out_len, streams, blocks, passes, [lands as (slot, out_off, out_len)])"""
    raw = [(item << 36) | c for c in cands]
    text = "P %d %d %d %d %d %d\n%s\n" % (src_len, room, measure, slot_cap, len(raw), len(recs), " ".join(str(v) for v in raw))
    text += "".join(" ".join(str(v) for v in r) + "\n" for r in recs)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    first, lands = r.stdout.split(" L")
    v = [int(x) for x in lands.split()]
    return tuple(int(x) for x in first.split()) + ([tuple(v[i:i + 3]) for i in range(0, len(v), 3)],)


# a stream of three blocks in 1000 bytes: header, blocks at bits 32, 2000 and 4003, the end magic at 6001, the end at byte 761
def three_blocks(**last):
    kw = dict(next=NEXT_END, after=761, stream_crc=fold([7, 8, 9]))
    kw.update(last)
    return [head(), block(32, 2000, crc=7), block(2000, 4003, crc=8, out_len=5), block(4003, 6001, crc=9, **kw)]


def test_chain_and_false_candidates(program):
    cands = [32, 2000, 4003]
    assert plan(program, 1000, 2405, cands, three_blocks())[:4] == (0, 2405, 1, 3)
    # candidates inside block data and inside the ignored rest: some fail, one even decodes; the chain lands on neither
    extra = [500, 3000, 7000]
    recs = three_blocks() + [block(3000, 3500, out_len=1 << 30)]
    st, out, streams, blocks, passes, lands = plan(program, 1000, 2405, cands + extra, recs)
    assert (st, out, streams, blocks, passes) == (0, 2405, 1, 3, 1)
    assert [(o, n) for _, o, n in lands] == [(0, 1200), (1200, 5), (1205, 1200)]
    # the scan's entries in any order, twice, for items that do not exist and beyond the item: dropped
    junk = [(5 << 36) | 40, (1 << 36) | (8 * 1000 - 47), (1 << 36) | 2000]
    text = plan(program, 1000, 2405, [4003, 32, 2000, 2000], recs + [block(8 * 1000 - 47, 9000)])
    assert text[:4] == (0, 2405, 1, 3)
    assert plan(program, 1000, 2405, [4003, 32, 2000] + [j - (1 << 36) for j in junk], recs)[:4] == (0, 2405, 1, 3)


@pytest.mark.parametrize("slot_cap", [1, 2, 3, 5, 1000])
def test_slot_cap_changes_passes_only(program, slot_cap):
    cands = [32, 500, 2000, 3000, 4003, 7000]
    recs = three_blocks(tail=BZH, tail_len=3) + [head(761, level=9, next=NEXT_END, after=775)]
    st, out, streams, blocks, passes, lands = plan(program, 1000, 2405, cands, recs, slot_cap=slot_cap)
    assert (st, out, streams, blocks) == (0, 2405, 2, 3)
    assert [(o, n) for _, o, n in lands] == [(0, 1200), (1200, 5), (1205, 1200)]
    assert all(s < slot_cap for s, _, _ in lands)
    # the second stream's header is read in a pass behind the one that reached it; with one slot every block is a pass of its own
    # (candidates go in position order, the false ones at 500 and 3000 among them)
    assert passes == {1: 4, 2: 4, 3: 3}.get(slot_cap, 2)


def test_statuses(program):
    cands = [32, 2000, 4003]
    ok = three_blocks()
    run = lambda recs, room=2405, src_len=1000, c=cands, **kw: plan(program, src_len, room, c, recs, **kw)[:4]  # noqa: E731
    bad = lambda st: (st, 0, 0, 0)  # noqa: E731
    assert run(ok, room=2404) == bad(E_DST_SMALL)          # an offset sum beyond the room
    assert run(ok, room=1200) == bad(E_DST_SMALL)
    assert run(ok, room=2404, measure=1) == (0, 2405, 1, 3)
    assert run([head(status=E_CORRUPT)] + ok[1:]) == bad(E_CORRUPT)
    assert run([head(level=0)] + ok[1:]) == bad(E_CORRUPT)
    assert run([head(level=10)] + ok[1:]) == bad(E_CORRUPT)
    assert run([ok[0], block(32, 2000, status=E_UNSUPPORTED)] + ok[2:]) == bad(E_UNSUPPORTED)
    assert run([ok[0], block(32, 2000, status=-99)] + ok[2:]) == bad(E_CORRUPT)
    assert run([ok[0], block(32, 2000, next=7)] + ok[2:]) == bad(E_CORRUPT)
    # a record ending before it starts, or inside its own header
    assert run([ok[0], block(32, 20)] + ok[2:]) == bad(E_CORRUPT)
    assert run([ok[0], block(32, 32 + 105)] + ok[2:]) == bad(E_CORRUPT)
    # a length beyond level x 100,000, none at all, origPtr beyond it
    assert run([ok[0], block(32, 2000, n=100001)] + ok[2:]) == bad(E_CORRUPT)
    assert run([head(level=2), block(32, 2000, n=100001)] + ok[2:]) == (0, 2405, 1, 3)
    assert run([ok[0], block(32, 2000, n=0)] + ok[2:]) == bad(E_CORRUPT)
    assert run([ok[0], block(32, 2000, n=10, orig=10)] + ok[2:]) == bad(E_CORRUPT)
    # a chain that never reaches an end: the block behind is no candidate, or the records point into the void
    assert run(ok[:3]) == bad(E_CORRUPT)
    assert run([ok[0], ok[1], block(2000, 2500)] + ok[3:]) == bad(E_CORRUPT)
    assert run(ok, c=[32, 2000]) == bad(E_CORRUPT)
    assert run(ok, c=[]) == bad(E_CORRUPT)
    # an end position beyond src_len, an end that is not behind its trailer
    assert run(ok[:3] + [block(4003, 8 * 1000 - 40, crc=9)]) == bad(E_CORRUPT)
    assert run(three_blocks(after=1001)) == bad(E_CORRUPT)
    assert run(three_blocks(after=760)) == bad(E_CORRUPT)
    assert run(three_blocks(after=762)) == bad(E_CORRUPT)
    assert run(three_blocks(after=1 << 60)) == bad(E_CORRUPT)
    # checksums: the lowest rank, and not looked at in measure mode
    assert run(three_blocks(stream_crc=1)) == bad(E_CHECKSUM)
    assert run(three_blocks(stream_crc=1), measure=1) == (0, 2405, 1, 3)
    assert run([ok[0], block(32, 2000, crc=7, crc_ok=0)] + ok[2:]) == bad(E_CHECKSUM)
    assert run([ok[0], block(32, 2000, crc=7, crc_ok=0)] + ok[2:], room=2404) == bad(E_DST_SMALL)
    assert run([ok[0], block(32, 2000, crc=7, crc_ok=0), ok[2], block(4003, 6001, status=E_CORRUPT)]) == bad(E_CORRUPT)
    # a rest that is not "BZh", or too short to be, is ignored; one that is gets judged: our status where the arbiter drops it
    assert run(three_blocks(tail=0x005A42, tail_len=3)) == (0, 2405, 1, 3)
    assert run(three_blocks(tail=BZH, tail_len=2)) == (0, 2405, 1, 3)
    assert run(three_blocks(after=998, tail=BZH, tail_len=3), src_len=1000) == bad(E_CORRUPT)   # (998 is not behind this trailer)
    assert run(three_blocks(tail=BZH, tail_len=3) + [head(761, status=E_CORRUPT)]) == bad(E_CORRUPT)
    assert run(three_blocks(tail=BZH, tail_len=3)) == bad(E_CORRUPT)                              # (no record: the job failed)
    # an empty stream
    assert run([head(next=NEXT_END, after=14)], src_len=14, c=[]) == (0, 0, 1, 0)
    assert run([head(next=NEXT_END, after=14, stream_crc=3)], src_len=14, c=[]) == bad(E_CHECKSUM)


def test_admit(program):
    def admit(out_cap, items):
        text = "A %d %d\n" % (out_cap, len(items)) + "".join("%d %d %d\n" % it for it in items)
        r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
        st, rest = r.stdout.split(" I ")
        counts, slots = rest.split(" S ")
        return [int(x) for x in st.split()], [int(x) for x in counts.split()], [int(x) for x in slots.split()]

    st, counts, slots = admit(100, [(0, 14, 10), (14, 0, 5), (900, 101, 1), (20, 45, 84), (20, 5000, 1)])  # (a refused item keeps its room)
    assert st == [0, 0, 0, E_INVAL, 0, E_INVAL]
    assert counts == [2, 2, (8 * 14 // 45 + 1) + (8 * 45 // 45 + 1)]
    assert slots == [counts[2], 3, 0]
    st, counts, slots = admit(100, [(0, 14, 60), (14, 14, 41), (28, 14, 0)])
    assert st == [0, 0, E_DST_SMALL, E_DST_SMALL]  # (the packed offset of the third lies beyond the region)
    # measure mode: no output region, the rooms are not read
    st, counts, slots = admit(0, [(0, 14, 1 << 40), (14, 900, 7), (999, 2, 0)])
    assert st == [0, 0, 0, E_INVAL] and counts == [2, 2, (8 * 14 // 45 + 1) + (8 * 900 // 45 + 1)]
