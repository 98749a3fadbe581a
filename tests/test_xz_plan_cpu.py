"""The host planning of znippy_unxz_batch (znippy_amd/csrc/host/xz_plan.cc) as a stand-alone host program under AddressSanitizer and
UBSan.  The bytes it parses and the records it judges come from device memory that holds untrusted input, so the cases here are
hand-written footers, indexes and decode records, the contradictory ones included: every case must give the expected plan or a
status, never a sanitizer report.  The program plays the rounds the way api.hip does — the ranges the walks ask for, heap copies of
exactly those bytes, give — so a read past a range is caught."""
import os
import shutil
import struct
import subprocess

import pytest

import xz_build as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "znippy_amd", "csrc", "host")
OK, E_INVAL, E_NOMEM, E_DST_SMALL, E_CORRUPT, E_UNSUPPORTED, E_CHECKSUM = 0, -1, -3, -4, -5, -6, -7
ABSENT = (1 << 64) - 1

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "xz_plan.h"
using namespace zn;
// stdin: cases.
// "W n" and n bytes in hex: the walk of one item by xzp::start / give, every range a heap copy of exactly its bytes
//   -> "status content too_big streams blocks rounds"
// "F room measure n n_recs", n bytes in hex and n_recs lines "status produced hdr_comp hdr_uncomp check_lo check_hi hdr_size comp sum":
// a batch of an empty item, the file and an empty stream through xz_admit .. xz_verdict; a job without a line gets a record that failed
//   -> "rc st0 st1 st2 out_len streams blocks unverified rounds J n_jobs (src_off unpadded check out_off out_len)..."
static bool read_hex(size_t n, std::vector<uint8_t> &v) {
    v.resize(n);
    for (size_t i = 0; i < n; i++) { unsigned x; if (scanf("%2x", &x) != 1) return false; v[i] = (uint8_t)x; }
    return true;
}
int main() {
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'W') {
            size_t n; std::vector<uint8_t> f;
            if (scanf("%zu", &n) != 1 || !read_hex(n, f)) return 2;
            xzp::Walk w;
            xzp::start(w, n);
            unsigned rounds = 0;
            while (!w.done) {
                if (++rounds > 100000 || w.want_len == 0 || w.want_off > n || w.want_len > n - w.want_off) return 3;
                if (w.want_head) {
                    uint8_t *first = (uint8_t *)malloc(12);
                    memcpy(first, f.data(), 12);
                    xzp::give_head(w, first);
                    free(first);
                }
                uint8_t *copy = (uint8_t *)malloc(w.want_len);
                memcpy(copy, f.data() + w.want_off, w.want_len);
                xzp::give(w, copy);
                free(copy);
            }
            size_t blocks = 0;
            for (const auto &s : w.streams) blocks += s.n;
            if (w.status == 0 && blocks != w.blocks.size()) return 3;
            printf("%d %" PRIu64 " %d %zu %zu %u\n", w.status, w.status ? 0 : w.content, (int)w.too_big, w.streams.size(), blocks, rounds);
        } else if (what == 'F') {
            unsigned long long room; unsigned measure; size_t n, n_recs; std::vector<uint8_t> f;
            if (scanf("%llu %u %zu %zu", &room, &measure, &n, &n_recs) != 4 || !read_hex(n, f)) return 2;
            static const uint8_t empty[32] = {0xFD, '7', 'z', 'X', 'Z', 0, 0, 4, 0xE6, 0xD6, 0xB4, 0x46, 0, 0, 0, 0, 0x1C, 0xDF, 0x44, 0x21,
                                              0x1F, 0xB6, 0xF3, 0x7D, 1, 0, 0, 0, 0, 4, 'Y', 'Z'};
            std::vector<uint8_t> src(f);
            src.insert(src.end(), empty, empty + 32);
            const uint64_t so[3] = {0, 0, n}, sl[3] = {0, n, 32}, rooms[3] = {0, room, 0};
            uint64_t ol[3] = {9, 9, 9}; uint32_t streams[3] = {9, 9, 9}, blocks[3] = {9, 9, 9}, unv[3] = {9, 9, 9};
            std::vector<uint8_t> out((size_t)room + 1);
            const XzCall call{src.data(), src.size(), so, sl, 3, measure ? nullptr : out.data(), measure ? 0 : room, nullptr, measure ? nullptr : rooms,
                              ol, streams, blocks, unv};
            XzBatch b;
            int rc = xz_admit(call, b);
            unsigned rounds = 0;
            if (!rc) {
                uint64_t need;
                while ((need = xz_wants(b))) {
                    if (++rounds > 100000) return 3;
                    uint64_t total = 0;
                    b.stage.assign((size_t)need, 0xEE);
                    for (const XzRange &r : b.ranges) {
                        if (r.item >= b.items.size() || r.len == 0 || r.off > b.items[r.item].src_len || r.len > b.items[r.item].src_len - r.off ||
                            r.at + r.len > need) return 3;
                        memcpy(b.stage.data() + r.at, b.items[r.item].src + r.off, r.len);
                        total += r.len;
                    }
                    if (total > src.size()) return 3;   // (the staging bound: a round never asks for more than the source bytes)
                    xz_give(b);
                }
                rc = xz_plan_jobs(call, b);
            }
            if (!rc) {
                b.recs.resize(b.jobs.size());
                b.sums.resize(b.jobs.size());
                for (size_t j = 0; j < b.jobs.size(); j++) {
                    XzRec r; memset(&r, 0, sizeof r); r.status = XZ_E_CORRUPT;
                    unsigned long long sum = 0;
                    if (j < n_recs) {
                        unsigned long long hc, hu;
                        if (scanf("%d %u %llu %llu %u %u %u %u %llu", &r.status, &r.produced, &hc, &hu, &r.check_lo, &r.check_hi, &r.hdr_size, &r.comp, &sum) != 9) return 2;
                        r.hdr_comp = hc; r.hdr_uncomp = hu;
                    }
                    b.recs[j] = r; b.sums[j] = sum;
                }
                for (size_t j = b.jobs.size(); j < n_recs; j++) { long long x[9]; for (auto &v : x) if (scanf("%lld", &v) != 1) return 2; }
                xz_verdict(call, b);
            }
            printf("%d %d %d %d %" PRIu64 " %u %u %u %u J %zu", rc, b.st[0], b.st[1], b.st[2], ol[1], streams[1], blocks[1], unv[1], rounds, b.jobs.size());
            if (ol[0] || ol[2] || streams[0] || blocks[0] || unv[0] || (b.st[2] == 0 && streams[2] != 1)) return 3;
            for (const XzJob &j : b.jobs) {
                const XzItem &it = b.items[j.item];
                if ((uint64_t)j.src_off + ((j.unpadded + 3) & ~3u) > it.src_len || (uint64_t)j.out_off + j.out_len > it.room) return 3;
                printf(" %u %u %u %u %u", j.src_off, j.unpadded, j.check, j.out_off, j.out_len);
            }
            printf("\n");
        } else return 2;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("xz_plan")
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "plan"
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", HOST, str(main)] + [os.path.join(HOST, f) for f in ("xz_plan.cc", "deflate_batch.cc", "gz_plan.cc", "range_plan.cc")] +
                   ["-o", str(exe)], check=True)
    return str(exe)


def run(program, text):
    p = subprocess.run([program], input=text, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return [[int(v) if v != "J" else v for v in line.split()] for line in p.stdout.splitlines()]


def walk(program, files):
    """-> [(status, content, too_big, streams, blocks, rounds)]"""
    return [tuple(r) for r in run(program, "".join("W %d %s\n" % (len(f), f.hex()) for f in files))]


def rec(job, status=0, produced=None, hdr_comp=ABSENT, hdr_uncomp=ABSENT, check=0, hdr_size=12, comp=None, sum=0):
    """the record an honest wave leaves for a job (src_off, unpadded, check id, out_off, out_len), fields replaceable"""
    cs = X.check_size(job[2])
    return (status, job[4] if produced is None else produced, hdr_comp, hdr_uncomp, check & 0xFFFFFFFF, check >> 32, hdr_size,
            job[1] - hdr_size - cs if comp is None else comp, sum)


def batch(program, f, room, recs=(), measure=0):
    """-> (rc, [st0, st1, st2], out_len, streams, blocks, unverified, rounds, [jobs as 5-tuples])"""
    text = "F %d %d %d %d %s\n" % (room, measure, len(f), len(recs), f.hex()) + "".join(" ".join(str(v) for v in r) + "\n" for r in recs)
    r = run(program, text)[0]
    at = r.index("J")
    jobs = r[at + 2:]
    assert len(jobs) == 5 * r[at + 1]
    return r[0], r[1:4], r[4], r[5], r[6], r[7], r[8], [tuple(jobs[i:i + 5]) for i in range(0, len(jobs), 5)]


def fake(records, check=X.CHECK_CRC64, body=None, **kw):
    """a stream whose blocks are filler bytes: the walk reads none of them"""
    if body is None:
        body = b"".join(b"\xAB" * ((u + 3) & ~3) for u, _ in records)
    return X.stream([body], check, records=records, **kw)


def test_walks(program):
    one = fake([(100, 1000), (7, 0), (4001, 70000)])
    long_index = fake([(8 + i % 5, i) for i in range(900)])
    files = [one, one + bytes(8), one + fake([(5, 1)], X.CHECK_NONE), one + bytes(4) + one + bytes(2048), fake([]), long_index,
             fake([(100, (1 << 32) - 1)]), fake([(100, (1 << 32) - 1), (20, 1)])]
    got = walk(program, files)
    assert got[0] == (OK, 71000, 0, 1, 3, 1)              # the tail, and with it the first 12 bytes: the stream header 4 KB further to the front
    assert got[1] == (OK, 71000, 0, 1, 3, 1)
    assert got[2] == (OK, 71001, 0, 2, 4, 1)
    assert got[3][:5] == (OK, 142000, 0, 2, 6) and got[3][5] >= 5   # 2 KiB of padding are two tails
    assert got[4] == (OK, 0, 0, 1, 0, 1)
    assert got[5][:5] == (OK, sum(range(900)), 0, 1, 900) and got[5][5] == 2   # the tail with the first 12 bytes, the index
    assert got[6] == (OK, (1 << 32) - 1, 0, 1, 1, 1) and got[7][:3] == (OK, 1 << 32, 1)


def test_contradictions_of_the_container(program):
    recs = [(100, 1000), (50, 20)]
    ix = X.index(recs)
    good = fake(recs)
    v9 = b"\xff" * 8 + b"\x7f"            # 2^63 - 1
    cases = {
        "backward size beyond the item": fake(recs, footer=X.stream_footer(len(ix), 4, backward=len(good) // 4)),
        "backward size that leaves no room for a header": fake(recs, footer=X.stream_footer(len(ix), 4, backward=(len(good) - 24) // 4)),
        "backward size of 2^32 words": fake(recs, footer=X.stream_footer(len(ix), 4, backward=0xFFFFFFFF)),
        "record count beyond the bytes": fake(recs, index_bytes=X.index(recs, count=3)),
        "record count of 2^63 - 1": fake(recs, index_bytes=X.index(recs, count=(1 << 63) - 1)),
        "unpadded sizes that overflow 64 bits": fake(recs, index_bytes=X.index([(v9, 1), (v9, 1), (v9, 1)])),
        "uncompressed sizes that overflow 64 bits": None,
        "a VLI of 10 bytes": fake(recs, index_bytes=X.index([(b"\x80" * 9 + b"\x01", 1000), recs[1]])),
        "a VLI of 9 bytes with the top bit": fake(recs, index_bytes=X.index([(b"\xff" * 9, 1000), recs[1]])),
        "a VLI with a trailing zero byte": fake(recs, index_bytes=X.index([(b"\xe4\x80\x00", 1000), recs[1]])),
        "a VLI cut off by the CRC": fake(recs, index_bytes=X.index([recs[0], (50, b"\x94")])),
        "an unpadded size of 4": fake([(4, 0)]),
        "an index of nothing but the indicator": fake(recs, index_bytes=b"\x00\x00\x00\x00" + struct.pack("<I", X.crc32(bytes(4)))),
        "sizes that do not add up": fake(recs, body=b"\xAB" * 156),
        "sizes that are less than the blocks": fake(recs, body=b"\xAB" * 4000),
        "sizes that are more than the blocks": fake(recs, body=b"\xAB" * 148),
        "footer flags 00 14": fake(recs, check=0x14),
        "three bytes": b"\x00YZ",
        "a footer alone": good[-12:],
        "zeros": bytes(4096 + 4),
        "a stream behind a stump": b"\x01\x02\x03" + good,
    }
    cases.pop("uncompressed sizes that overflow 64 bits")
    got = walk(program, list(cases.values()))
    for (name, f), g in zip(cases.items(), got):
        assert g[0] == (E_UNSUPPORTED if name == "footer flags 00 14" else E_CORRUPT) and g[1] == 0, (name, g)
    # sums of uncompressed sizes saturate: 2 x (2^63 - 1) is "4 GiB or more", not a small number
    f = fake([(100, v9), (50, v9)])
    assert walk(program, [f])[0][:3] == (OK, 1 << 62, 1)
    assert batch(program, f, 1 << 20)[1][1] == E_UNSUPPORTED and batch(program, f, 0, measure=1)[1][1] == E_UNSUPPORTED


def test_plans_and_honest_records(program):
    first = fake([(100, 1000), (17, 0), (4001, 70000)], check=X.CHECK_CRC32)
    f = first + bytes(4) + fake([(60, 5)], check=X.CHECK_SHA256)
    rc, st, out_len, streams, blocks, unv, rounds, jobs = batch(program, f, 71005)
    assert rc == 0 and st == [OK, E_CORRUPT, OK]   # (no record was given: every job failed)
    assert jobs == [(12, 100, 1, 0, 1000), (112, 17, 1, 1000, 0), (132, 4001, 1, 1000, 70000), (len(first) + 4 + 12, 60, 10, 71000, 5)], jobs
    recs = [rec(j, check=5, sum=5 if j[2] == 1 else 77) for j in jobs]
    assert batch(program, f, 71005, recs)[:6] == (0, [OK, OK, OK], 71005, 2, 4, 1)
    assert batch(program, f, 71004, recs)[1] == [OK, E_DST_SMALL, OK]
    rc, st, out_len, streams, blocks, unv, rounds, jobs0 = batch(program, f, 0, measure=1)
    assert (rc, st, out_len, streams, blocks, unv) == (0, [OK, OK, OK], 71005, 2, 4, 1) and len(jobs0) == 0
    # CRC64 compares all eight bytes
    g = fake([(100, 1000)], check=X.CHECK_CRC64)
    j = batch(program, g, 1000)[7][0]
    assert batch(program, g, 1000, [rec(j, check=0x1122334455667788, sum=0x1122334455667788)])[1][1] == OK
    assert batch(program, g, 1000, [rec(j, check=0x1122334455667788, sum=0x0122334455667788)])[1][1] == E_CHECKSUM


def test_contradictory_records(program):
    f = fake([(100, 1000), (60, 500)], check=X.CHECK_CRC32)
    jobs = batch(program, f, 1500)[7][:2]
    good = [rec(j, check=9, sum=9) for j in jobs]
    assert batch(program, f, 1500, good)[1][1] == OK

    def second(**kw):
        return batch(program, f, 1500, [good[0], rec(jobs[1], **dict(dict(check=9, sum=9), **kw))])[1:3]

    assert second(sum=8) == ([OK, E_CHECKSUM, OK], 0)
    assert second(status=E_UNSUPPORTED) == ([OK, E_UNSUPPORTED, OK], 0)
    for kw in (dict(status=E_CORRUPT), dict(status=1), dict(status=E_DST_SMALL), dict(status=-2147483648), dict(produced=499), dict(produced=501),
               dict(produced=0xFFFFFFFF), dict(hdr_comp=45), dict(hdr_comp=0), dict(hdr_uncomp=499), dict(hdr_uncomp=1 << 63),
               dict(hdr_size=0), dict(hdr_size=4), dict(hdr_size=14), dict(hdr_size=1028), dict(hdr_size=60), dict(hdr_size=0xFFFFFFFC),
               dict(comp=43), dict(comp=0xFFFFFFFF)):
        assert second(**kw) == ([OK, E_CORRUPT, OK], 0), kw
    assert second(hdr_comp=44, hdr_uncomp=500) == ([OK, OK, OK], 1500)       # a header that names the index's sizes
    # the first failure in stream order decides; a differing check only on an otherwise clean item
    bad_first = [rec(jobs[0], check=9, sum=8), rec(jobs[1], status=E_UNSUPPORTED)]
    assert batch(program, f, 1500, bad_first)[1][1] == E_UNSUPPORTED
    assert batch(program, f, 1500, [rec(jobs[0], status=E_UNSUPPORTED), rec(jobs[1], status=E_CORRUPT)])[1][1] == E_UNSUPPORTED


def test_admission(program):
    f = fake([(100, 1000)])
    assert batch(program, f, 999)[1] == [OK, E_DST_SMALL, OK] and batch(program, f, 999)[7] == []
    assert batch(program, f[:-1], 1000)[1][1] == E_CORRUPT
