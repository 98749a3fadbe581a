"""The host planning of znippy_gunzip_batch (znippy_amd/csrc/host/gz_plan.cc) as a stand-alone host program under AddressSanitizer
and UBSan.  The probe records it reads come from device memory that decoded untrusted input, so the cases here are hand-written
records, the contradictory ones included: every case must give the expected plan or an error code, never a sanitizer report.  The
record arrays the program hands to the planner are heap copies of exactly the records named, so a read past them is caught."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "znippy_amd", "csrc", "host")
E_DST_SMALL, E_CORRUPT, E_UNSUPPORTED, E_CHECKSUM = -4, -5, -6, -7
FLUSH, MEMBER = 0, 1
BOUNDARY, TRAILER, ERROR, ROOM = 0, 1, 2, 3
NEXT_MEMBER, NEXT_END = 0, 1

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "gz_plan.h"
// stdin: cases.  "P src_len room n" and n lines "pos kind data_start end_kind end_pos status out reach crc isize next":
//   -> "status members segments out_len R src_start out_off out_len ... M crc out_off out_len ..."
// "K seg_min n" and a line of n values pos << 1 | kind -> the kept ones
// "C crc_a crc_b len_b" -> crc32_combine
int main() {
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'P') {
            unsigned long long src_len, room; size_t n;
            if (scanf("%llu %llu %zu", &src_len, &room, &n) != 3) return 2;
            gzp::Probe *recs = (gzp::Probe *)malloc(n ? n * sizeof(gzp::Probe) : 1);
            for (size_t i = 0; i < n; i++) {
                gzp::Probe &r = recs[i];
                unsigned long long out;
                if (scanf("%u %u %u %u %u %d %llu %u %u %u %d", &r.pos, &r.kind, &r.data_start, &r.end_kind, &r.end_pos, &r.status, &out, &r.reach, &r.crc,
                          &r.isize, &r.next) != 11) return 2;
                r.out = out;
            }
            std::vector<gzp::Run> runs(1, gzp::Run{77, 7, 7, 7});   // (what other items left: must stay)
            std::vector<gzp::Member> mems(1, gzp::Member{77, 7, 7, 7});
            gzp::ItemPlan p;
            gzp::plan_item(recs, n, 3, src_len, room, runs, mems, &p);
            free(recs);
            if (runs[0].item != 77 || mems[0].item != 77) return 3;
            printf("%d %u %u %" PRIu64 " R", p.status, p.members, p.segments, p.out_len);
            for (size_t i = 1; i < runs.size(); i++) {
                if (runs[i].item != 3) return 3;
                printf(" %u %" PRIu64 " %" PRIu64, runs[i].src_start, runs[i].out_off, runs[i].out_len);
            }
            printf(" M");
            for (size_t i = 1; i < mems.size(); i++) {
                // a member's runs are its own, follow those of the member before, and hold exactly its bytes
                uint64_t sum = 0;
                if (mems[i].run0 > mems[i].run1 || mems[i].run1 > runs.size() || mems[i].run0 != (i > 1 ? mems[i - 1].run1 : 1)) return 3;
                for (size_t r = mems[i].run0; r < mems[i].run1; r++) sum += runs[r].out_len;
                if (sum != mems[i].out_len || (mems[i].run0 < mems[i].run1 && runs[mems[i].run0].out_off != mems[i].out_off)) return 3;
                printf(" %u %" PRIu64 " %" PRIu64, mems[i].crc, mems[i].out_off, mems[i].out_len);
            }
            printf("\n");
        } else if (what == 'K') {
            unsigned long long seg_min; size_t n;
            if (scanf("%llu %zu", &seg_min, &n) != 2) return 2;
            uint64_t *c = (uint64_t *)malloc(n ? n * sizeof(uint64_t) : 1);
            for (size_t i = 0; i < n; i++) { unsigned long long v; if (scanf("%llu", &v) != 1) return 2; c[i] = v; }
            const size_t kept = gzp::keep_candidates(c, n, seg_min);
            if (kept > n) return 3;
            printf("K");
            for (size_t i = 0; i < kept; i++) printf(" %" PRIu64, c[i]);
            printf("\n");
            free(c);
        } else if (what == 'C') {
            unsigned a, b; unsigned long long len;
            if (scanf("%u %u %llu", &a, &b, &len) != 3) return 2;
            printf("C %u\n", gzp::crc32_combine(a, b, len));
        } else return 2;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("gz_plan")
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "plan"
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", HOST, str(main), os.path.join(HOST, "gz_plan.cc"), "-o", str(exe)], check=True)
    return str(exe)


def rec(pos, kind, end_kind, end_pos=0, out=0, reach=0, status=0, crc=0, isize=None, next=NEXT_END, data_start=None):
    return (pos, kind, pos + (10 if kind == MEMBER else 0) if data_start is None else data_start, end_kind, end_pos, status, out, reach, crc,
            out & 0xFFFFFFFF if isize is None else isize, next)


def plan(program, src_len, room, recs):
    """-> (status, members, segments, out_len, [runs as (src_start, out_off, out_len)], [members as (crc, out_off, out_len)])"""
    recs = sorted(recs, key=lambda r: (r[0], r[1]))
    text = "P %d %d %d\n" % (src_len, room, len(recs)) + "".join(" ".join(str(v) for v in r) + "\n" for r in recs)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    head, rest = r.stdout.split(" R", 1)
    runs, mems = rest.split(" M")
    three = lambda s: [tuple(int(x) for x in s.split()[i:i + 3]) for i in range(0, len(s.split()), 3)]  # noqa: E731
    st, m, sg, ol = (int(x) for x in head.split())
    return st, m, sg, ol, three(runs), three(mems)


def failed(program, src_len, room, recs, status):
    assert plan(program, src_len, room, recs) == (status, 0, 0, 0, [], [])


def test_one_member_and_flush_chain(program):
    # one member, nothing else
    assert plan(program, 100, 50, [rec(0, MEMBER, TRAILER, 100, out=50, crc=9)]) == (0, 1, 1, 50, [(10, 0, 50)], [(9, 0, 50)])
    # three independent pieces; a false candidate at 300 (its record says garbage) and one the chain never lands on at 500
    recs = [rec(0, MEMBER, BOUNDARY, 200, out=1000), rec(200, FLUSH, BOUNDARY, 400, out=2000), rec(400, FLUSH, TRAILER, 900, out=30, isize=3030, crc=5),
            rec(300, FLUSH, ERROR, status=E_CORRUPT, out=17), rec(500, MEMBER, ROOM, out=1 << 40), rec(600, FLUSH, BOUNDARY, 100, out=3, reach=70000)]
    assert plan(program, 900, 3030, recs) == (0, 1, 3, 3030, [(10, 0, 1000), (200, 1000, 2000), (400, 3000, 30)], [(5, 0, 3030)])
    # the same chain in a room one byte short
    failed(program, 900, 3029, recs, E_DST_SMALL)


def test_dependent_pieces_join(program):
    # a sync flush: the second piece reaches 5 bytes back and joins the first
    recs = [rec(0, MEMBER, BOUNDARY, 200, out=4096), rec(200, FLUSH, TRAILER, 400, out=4096, reach=5, isize=8192)]
    assert plan(program, 400, 8192, recs) == (0, 1, 1, 8192, [(10, 0, 8192)], [(0, 0, 8192)])
    # several in a row, then an independent one, then one whose reach is longer than the run it would join: that run joins too
    recs = [rec(0, MEMBER, BOUNDARY, 100, out=100), rec(100, FLUSH, BOUNDARY, 200, out=100, reach=1), rec(200, FLUSH, BOUNDARY, 300, out=100, reach=200),
            rec(300, FLUSH, BOUNDARY, 400, out=50), rec(400, FLUSH, BOUNDARY, 500, out=10), rec(500, FLUSH, TRAILER, 600, out=40, reach=20, isize=400)]
    assert plan(program, 600, 400, recs) == (0, 1, 2, 400, [(10, 0, 300), (300, 300, 100)], [(0, 0, 400)])
    # the reach goes through an empty independent piece into the run in front of it
    recs = [rec(0, MEMBER, BOUNDARY, 100, out=100), rec(100, FLUSH, BOUNDARY, 105, out=0), rec(105, FLUSH, TRAILER, 300, out=7, reach=3, isize=107)]
    assert plan(program, 300, 107, recs) == (0, 1, 1, 107, [(10, 0, 107)], [(0, 0, 107)])
    # a reach in front of the member's first byte: zlib's "invalid distance too far back"
    recs = [rec(0, MEMBER, BOUNDARY, 100, out=100), rec(100, FLUSH, TRAILER, 300, out=7, reach=101, isize=107)]
    failed(program, 300, 107, recs, E_CORRUPT)
    # a second member never joins the first: a member record with a reach is a contradiction
    recs = [rec(0, MEMBER, TRAILER, 100, out=100, next=NEXT_MEMBER), rec(100, MEMBER, TRAILER, 300, out=7, reach=3)]
    failed(program, 300, 107, recs, E_CORRUPT)


def test_members_empty_pieces_and_padding(program):
    # three members, the middle one empty, zero padding in front of the third (its candidate lies behind the padding); an empty piece
    recs = [rec(0, MEMBER, TRAILER, 40, out=11, crc=1, next=NEXT_MEMBER), rec(40, MEMBER, TRAILER, 67, out=0, crc=0, next=NEXT_MEMBER),
            rec(67, MEMBER, BOUNDARY, 90, out=5), rec(90, FLUSH, BOUNDARY, 95, out=0), rec(95, FLUSH, TRAILER, 120, out=0, crc=3, isize=5)]
    assert plan(program, 120, 16, recs) == (0, 3, 5, 16, [(10, 0, 11), (50, 11, 0), (77, 11, 5), (90, 16, 0), (95, 16, 0)], [(1, 0, 11), (0, 11, 0), (3, 11, 5)])
    # garbage behind the first trailer: the probe says what is there
    for what in (E_CORRUPT, E_UNSUPPORTED):
        failed(program, 120, 16, [rec(0, MEMBER, TRAILER, 40, out=11, next=what)] + recs[1:], what)
    # ... and an ISIZE that is wrong is E_CHECKSUM only because everything else decoded; the plan is kept
    bad = [rec(0, MEMBER, TRAILER, 40, out=11, crc=1, isize=12, next=NEXT_MEMBER)] + recs[1:]
    assert plan(program, 120, 16, bad)[:4] == (E_CHECKSUM, 3, 5, 16)
    failed(program, 120, 16, bad[:1] + [rec(40, MEMBER, ERROR, status=E_CORRUPT)] + bad[2:], E_CORRUPT)
    # ISIZE is taken mod 2^32
    assert plan(program, 100, (1 << 32) + 5, [rec(0, MEMBER, TRAILER, 100, out=(1 << 32) + 5, isize=5)])[:4] == (0, 1, 1, (1 << 32) + 5)


def test_errors_in_the_chain(program):
    recs = [rec(0, MEMBER, BOUNDARY, 200, out=1000), rec(200, FLUSH, ERROR, status=E_CORRUPT, out=10), rec(400, FLUSH, TRAILER, 900, out=30)]
    failed(program, 900, 5000, recs, E_CORRUPT)
    # the room is exceeded in front of the error: the first failure in stream order decides
    failed(program, 900, 1005, recs, E_DST_SMALL)
    failed(program, 900, 5000, [recs[0], rec(200, FLUSH, ROOM, out=4001)], E_DST_SMALL)
    # the header of the first member
    failed(program, 900, 5000, [rec(0, MEMBER, ERROR, status=E_UNSUPPORTED)], E_UNSUPPORTED)


def test_contradictions(program):
    ok = rec(0, MEMBER, BOUNDARY, 200, out=10)
    cases = [
        [],                                                                              # no record at all
        [rec(5, MEMBER, TRAILER, 100, out=1)],                                           # none at byte 0
        [rec(0, FLUSH, TRAILER, 100, out=1)],                                            # byte 0 is no member candidate
        [ok],                                                                            # the chain lands where no record is
        [ok, rec(200, MEMBER, TRAILER, 300, out=1)],                                     # ... of the kind it needs
        [ok, rec(200, FLUSH, BOUNDARY, 200, out=1)],                                     # an end that is its own start
        [ok, rec(200, FLUSH, BOUNDARY, 100, out=1), rec(100, FLUSH, BOUNDARY, 200, out=1)],  # a loop
        [ok, rec(200, FLUSH, BOUNDARY, 5000, out=1)],                                    # an end behind the source
        [rec(0, MEMBER, TRAILER, 100, out=1, next=NEXT_MEMBER)],                         # a next member at the end of the source
        [rec(0, MEMBER, TRAILER, 50, out=1, next=NEXT_MEMBER)],                          # ... where no record is
        [rec(0, MEMBER, TRAILER, 50, out=1, next=7)],                                    # a next that is none of the values
        [rec(0, MEMBER, ERROR, status=0)],                                               # an error without a status
        [rec(0, MEMBER, ERROR, status=5)],
        [rec(0, MEMBER, ROOM, out=3)],                                                   # the room exceeded by a count that fits
        [rec(0, MEMBER, 9, 100, out=3)],                                                 # an end kind that does not exist
        [rec(0, MEMBER, TRAILER, 100, out=1, data_start=101)],                           # a first DEFLATE byte behind the source
        [ok, rec(200, FLUSH, TRAILER, 300, out=1, data_start=100)],                      # ... in front of the candidate
    ]
    for recs in cases:
        failed(program, 100 if len(recs) < 2 else 1000, 100, recs, E_CORRUPT)
    # counts that overflow the room, one of them the sum
    failed(program, 1000, 100, [rec(0, MEMBER, BOUNDARY, 200, out=(1 << 64) - 1)], E_DST_SMALL)
    failed(program, 1000, (1 << 32) - 1, [rec(0, MEMBER, BOUNDARY, 200, out=(1 << 32) - 2), rec(200, FLUSH, TRAILER, 300, out=(1 << 64) - 1)], E_DST_SMALL)
    # a source of no bytes has no record that could be landed on
    failed(program, 0, 100, [rec(0, MEMBER, TRAILER, 0, out=0)], E_CORRUPT)


def test_keep_candidates(program):
    def keep(seg_min, cands):
        text = "K %d %d\n%s\n" % (seg_min, len(cands), " ".join(str(p << 1 | k) for p, k in cands))
        r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
        return [(int(v) >> 1, int(v) & 1) for v in r.stdout.split()[1:]]
    assert keep(1, []) == []
    # any order in; position order out; members are always kept and count as the candidate kept before
    raw = [(900, FLUSH), (100, FLUSH), (50, FLUSH), (160, MEMBER), (200, FLUSH), (161, FLUSH), (1000, FLUSH), (950, MEMBER)]
    assert keep(1, raw) == sorted(raw)
    assert keep(100, raw) == [(100, FLUSH), (160, MEMBER), (900, FLUSH), (950, MEMBER)]
    assert keep(1 << 40, raw) == [(160, MEMBER), (950, MEMBER)]
    # both kinds at one position
    assert keep(4, [(8, MEMBER), (8, FLUSH), (8, FLUSH)]) == [(8, FLUSH), (8, MEMBER)]


def test_crc32_combine(program):
    import zlib

    import gen
    data = gen.pseudo_text(70_001, seed=6)
    cuts = [(0, 0), (0, 1), (1, 0), (1, 1), (5, 64), (64, 65_535), (70_000, 1), (35_000, 35_001)]
    text = "".join("C %d %d %d\n" % (zlib.crc32(data[:a]), zlib.crc32(data[a:a + b]), b) for a, b in cuts) + "C 7 0 0\nC 0 9 %d\n" % (1 << 40)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    got = [int(line.split()[1]) for line in r.stdout.splitlines()]
    assert got[:len(cuts)] == [zlib.crc32(data[:a + b]) for a, b in cuts]
    assert got[len(cuts):] == [7, 9]                       # nothing appended; appended to nothing, however long
