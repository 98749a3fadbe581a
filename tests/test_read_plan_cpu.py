"""The compiled host layer's read-side decisions (znippy_amd/csrc/host/read_plan.cc: which blobs a read takes and where they land,
what a private row table says, how a byte range maps to chunks, ranks, batches, writer parts, first touch, the sidecar's layout) as a
stand-alone host program under AddressSanitizer and UBSan.  An index goes in on stdin as columns — heap blocks of exactly the
columns' sizes, so a read past a column is the sanitizer's — followed by calls; every output field comes back and is compared with
models written here from the statements of the rules (read_plan.h), not from the code.  Unsigned sums that the rules let wrap
(a chunk's end, a blob sum) are modelled modulo 2^64.  Cases are drawn from where a rule changes."""
import bisect
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "znippy_amd", "csrc", "host")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include "read_plan.h"
typedef unsigned long long ull;
using namespace zn;
static bool rd(ull *v, int n) { for (int i = 0; i < n; i++) if (scanf("%llu", &v[i]) != 1) return false; return true; }
static ull weigh(const std::vector<uint8_t> &b) { ull s = 0; for (size_t i = 0; i < b.size(); i++) s += (ull)(i + 1) * b[i]; return s; }
static void table(const RowTable &t) {
    printf(" %zu %llu %zu", t.n(), (ull)t.sum, t.bitmap.size());
    for (uint8_t b : t.bitmap) printf(" %u", b);
    printf(" %zu %llu", t.ck.size(), weigh(t.ck));
    for (size_t k = 0; k < t.n(); k++) printf(" %llu %llu %llu %llu", (ull)t.bo[k], (ull)t.bs[k], (ull)t.us[k], (ull)t.fpos[k]);
}
static void ranges(const RangeList &g) {
    printf(" %zu", g.n());
    for (size_t k = 0; k < g.n(); k++) printf(" %llu %llu %llu", (ull)g.row[k], (ull)g.begin[k], (ull)g.len[k]);
}
struct Index {  // columns in heap blocks of exactly their sizes
    uint64_t n = 0;
    std::string *path = nullptr;
    uint32_t *seq = nullptr;
    uint64_t *fd = nullptr, *us = nullptr, *bo = nullptr, *bs = nullptr;
    uint8_t *comp = nullptr, *ck = nullptr;
    IndexView v;
    void clear() { delete[] path; free(seq); free(fd); free(us); free(bo); free(bs); free(comp); free(ck); }
    bool read(uint64_t rows, uint64_t file_size) {
        clear();
        n = rows;
        path = new std::string[n];
        seq = (uint32_t *)malloc(4 * n); fd = (uint64_t *)malloc(8 * n); us = (uint64_t *)malloc(8 * n); bo = (uint64_t *)malloc(8 * n); bs = (uint64_t *)malloc(8 * n);
        comp = (uint8_t *)malloc(n); ck = (uint8_t *)malloc(32 * n);
        for (uint64_t r = 0; r < n; r++) {
            ull x[7];  // path id, chunk_seq, fdata_offset, compressed, usize, blob_offset, blob_size
            if (!rd(x, 7)) return false;
            path[r] = "p" + std::to_string(x[0]); seq[r] = (uint32_t)x[1]; fd[r] = x[2]; comp[r] = (uint8_t)x[3]; us[r] = x[4]; bo[r] = x[5]; bs[r] = x[6];
            for (int j = 0; j < 32; j++) ck[32 * r + j] = (uint8_t)(r * 31 + j * 7 + 3);
        }
        v.path = path; v.chunk_seq = seq; v.fdata_offset = fd; v.compressed = comp; v.usize = us; v.blob_offset = bo; v.blob_size = bs; v.checksum = ck;
        v.n = n; v.file_size = file_size;
        return true;
    }
};
static uint64_t *list(ull n) {  // n values in a block of exactly that size
    uint64_t *p = (uint64_t *)malloc(8 * n);
    for (ull i = 0; i < n; i++) { ull x; if (scanf("%llu", &x) != 1) exit(2); p[i] = x; }
    return p;
}
int main() {
    char tag[8];
    Index ix;
    while (scanf("%7s", tag) == 1) {
        ull a[4];
        if (tag[0] == 'I') {  // n file_size, then the rows
            if (!rd(a, 2) || !ix.read(a[0], a[1])) { printf("bad line\n"); return 2; }
            continue;
        }
        if (tag[0] == 'R') {  // verify n ids
            if (!rd(a, 2)) return 2;
            uint64_t *ids = list(a[1]);
            const RowsRead p = plan_rows_read(ix.v, ids, a[1], a[0] != 0);
            printf("%d %d %llu %llu %llu %zu", p.rc, !p.err ? 0 : strstr(p.err, "overflow") ? 1 : 2, (ull)p.total, (ull)p.base, (ull)p.nblob, p.reads.size());
            for (const SlabRead &r : p.reads) printf(" %llu %llu %llu", (ull)r.fpos, (ull)r.at, (ull)r.len);
            if (!p.rc) {
                table(p.t);
                for (uint64_t o : p.out_off) printf(" %llu", (ull)o);
            }
            free(ids);
        } else if (tag[0] == 'M' || tag[0] == 'G') {  // [verify] off len n rows
            if (!rd(a, 4)) return 2;
            uint64_t *rows = list(a[3]);
            if (tag[0] == 'M') {
                std::vector<RangeHit> hits;
                uint64_t covered = 0;
                const int32_t rc = map_range(ix.v, rows, a[3], a[1], a[2], &hits, &covered);
                printf("%d %llu %zu", rc, (ull)(rc ? 0 : covered), rc ? (size_t)0 : hits.size());
                if (!rc) for (const RangeHit &h : hits) printf(" %llu %llu %llu", (ull)h.row, (ull)h.begin, (ull)h.len);
            } else {
                const RangeRead p = plan_range_read(ix.v, rows, a[3], a[1], a[2], a[0] != 0);
                printf("%d %llu", p.rc, (ull)p.total);
                table(p.t);
                ranges(p.rg);
                for (uint64_t r : p.arow) printf(" %llu", (ull)r);
            }
            free(rows);
        } else if (tag[0] == 'F') {  // n requests, each: off len n rows
            if (!rd(a, 1)) return 2;
            std::vector<std::vector<uint64_t>> rows(a[0]);
            std::vector<FileRange> req;
            for (ull i = 0; i < a[0]; i++) {
                ull q[3];
                if (!rd(q, 3)) return 2;
                uint64_t *l = list(q[2]);
                rows[i].assign(l, l + q[2]);
                rows[i].shrink_to_fit();
                free(l);
                req.push_back(FileRange{&rows[i], q[0], q[1]});
            }
            const FileRangesRead p = plan_file_ranges(ix.v, req);
            printf("%llu", (ull)p.total);
            table(p.t);
            ranges(p.rg);
            for (size_t q : p.of_req) printf(" %zu", q);
            for (size_t i = 0; i < req.size(); i++) printf(" %llu %d", (ull)p.at[i], p.st[i]);
        } else if (tag[0] == 'T') {  // begin end per_rank
            if (!rd(a, 3)) return 2;
            const FirstTouch f = read_plan_first_touch(ix.v, a[0], a[1], a[2] != 0);
            printf("%d %zu %zu", f.adjacent, f.n_unique, f.first.size());
            for (uint8_t b : f.first) printf(" %u", b);
            std::map<std::string, uint64_t> fs(f.final_size.begin(), f.final_size.end());
            printf(" %zu", fs.size());
            for (const auto &kv : fs) printf(" %s %llu", kv.first.c_str() + 1, (ull)kv.second);
        } else if (tag[0] == 'S') {  // rank world
            if (!rd(a, 2)) return 2;
            const auto r = split_rows(ix.v.usize, ix.v.n, (uint32_t)a[0], (uint32_t)a[1]);
            printf("%llu %llu", (ull)r.first, (ull)r.second);
        } else if (tag[0] == 'B') {  // i end batch_bytes verify_only
            if (!rd(a, 4)) return 2;
            printf("%llu", (ull)cut_batch(ix.v, a[0], a[1], a[2], a[3] != 0));
        } else if (tag[0] == 'W') {  // i n n_writers total, then n output offsets
            if (!rd(a, 4)) return 2;
            uint64_t *oo = list(a[1]);
            const auto parts = cut_writers(oo, a[3], ix.v.path, a[0], a[1], (unsigned)a[2]);
            printf("%zu", parts.size());
            for (const auto &p : parts) printf(" %llu %llu", (ull)p.first, (ull)p.second);
            free(oo);
        } else if (tag[0] == 'C') {  // size, then the file's bytes
            if (!rd(a, 1)) return 2;
            uint8_t *raw = (uint8_t *)malloc(a[0]);
            for (ull i = 0; i < a[0]; i++) { unsigned x; if (scanf("%2x", &x) != 1) return 2; raw[i] = (uint8_t)x; }
            std::vector<uint64_t> first;
            const bool ok = sidecar_layout(raw, a[0], ix.v, &first);
            printf("%d", ok);
            if (ok) for (uint64_t f : first) printf(" %llu", (ull)f);
            free(raw);
        } else if (tag[0] == 'U') {  // n rows (fpos bs us comp) of a table with checksums, then a list: the subset, and an entry copy
            if (!rd(a, 1)) return 2;
            RowTable t;
            for (ull k = 0; k < a[0]; k++) {
                ull x[4];
                if (!rd(x, 4)) return 2;
                uint8_t ck[32];
                for (int j = 0; j < 32; j++) ck[j] = (uint8_t)(k * 31 + j * 7 + 3);
                t.add(x[0], x[1], x[2], x[3] != 0, ck);
            }
            if (!rd(a + 1, 1)) return 2;
            uint64_t *l = list(a[1]);
            const RowTable s = t.subset(std::vector<size_t>(l, l + a[1]));
            free(l);
            table(t);
            table(s);
            printf(" %zu", s.reads().size());
        } else if (tag[0] == 'K') {  // entries in the buffer, first entry, entries taken, bytes already in dst
            if (!rd(a, 4)) return 2;
            uint8_t *packed = (uint8_t *)malloc(32 * a[0]);
            for (ull i = 0; i < 32 * a[0]; i++) packed[i] = (uint8_t)(i * 13 + 1);
            std::vector<uint8_t> dst(a[3], 9);
            const size_t at = take_tree(packed, 32 * a[1], a[2], &dst);
            printf("%zu %zu %llu", at, dst.size(), weigh(dst));
            free(packed);
        } else { printf("bad line\n"); return 2; }
        printf("\n");
    }
    ix.clear();
    return 0;
}
"""

U64 = 1 << 64
BLK = 128 * 1024
E_CORRUPT = -5
N_CASES = {}                                                            # test -> calls compared (the counts the commit message states)


def test_code():
    text = open(os.path.join(ROOT, "include", "znippy_hip.h")).read()
    assert int(re.search(r"#define ZNIPPY_E_CORRUPT \((-?\d+)\)", text).group(1)) == E_CORRUPT


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("read_plan")
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "plan"
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", HOST, str(main), os.path.join(HOST, "read_plan.cc"), "-o", str(exe)], check=True)
    return str(exe)


class Row:
    """One index row.  path: a number."""

    def __init__(self, path, fdata, comp, usize, bo, bs, seq=0):
        self.path, self.fdata, self.comp, self.usize, self.bo, self.bs, self.seq = path, fdata, int(comp), usize, bo, bs, seq

    @property
    def len(self):                                                      # a stored row is its blob
        return self.usize if self.comp else self.bs

    def line(self):
        return f"{self.path} {self.seq} {self.fdata} {self.comp} {self.usize} {self.bo} {self.bs}"


def index_text(rows, file_size):
    return f"I {len(rows)} {file_size}\n" + "".join(r.line() + "\n" for r in rows)


def check(program, name, text, want):
    """Runs the calls of `text` (index lines give no output) and compares each output line, field by field, with the model's."""
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-3000:])
    got = [line.split() for line in r.stdout.splitlines()]
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        w = [str(int(x)) for x in w]
        assert g == w, (name, i, [(j, a, b) for j, (a, b) in enumerate(zip(g, w)) if a != b][:4], len(g), len(w))
    N_CASES[name] = N_CASES.get(name, 0) + len(want)


# ---- models ------------------------------------------------------------------------------------------------------------------------

def ck_of(r):
    return bytes((r * 31 + j * 7 + 3) & 255 for j in range(32))


def weigh(b):
    return sum((i + 1) * x for i, x in enumerate(b)) % U64


def table_fields(trows, bo=None, total=None, ck=None):
    """trows: (fpos, bs, us, comp).  A packed table: every blob behind the ones before it."""
    packed, at = [], 0
    for _, bs, _, _ in trows:
        packed.append(at % U64)
        at += bs
    bo = packed if bo is None else bo
    bits = bytearray((len(trows) + 7) // 8)
    for k, t in enumerate(trows):
        if t[3]:
            bits[k // 8] |= 1 << (k % 8)
    ck = b"" if ck is None else ck
    out = [len(trows), (at if total is None else total) % U64, len(bits)] + list(bits) + [len(ck), weigh(ck)]
    for k, (fpos, bs, us, _) in enumerate(trows):
        out += [bo[k], bs, us, fpos % U64]
    return out


def in_file(row, file_size):
    return row.bo + row.bs <= file_size


def model_rows_read(rows, file_size, ids, verify):
    total, offs = 0, []
    for r in ids:
        if total + rows[r].len >= U64:
            return [E_CORRUPT, 1, total, 0, 0, 0]
        if not in_file(rows[r], file_size):
            return [E_CORRUPT, 2, total, 0, 0, 0]
        offs.append(total)
        total += rows[r].len
    trows = [(rows[r].bo, rows[r].bs, rows[r].len, rows[r].comp) for r in ids]
    ck = b"".join(ck_of(r) for r in ids) if verify else None
    if not ids:
        return [0, 0, 0, 0, 0, 0] + table_fields([])
    lo, hi, blobs = min(rows[r].bo for r in ids), max(rows[r].bo + rows[r].bs for r in ids), sum(rows[r].bs for r in ids) % U64
    if hi - lo > (2 * blobs + (1 << 20)) % U64:                         # scattered: every blob by itself, packed in table order
        t = table_fields(trows, ck=ck)
        reads = [(f, t[5 + len(t[3:3 + t[2]]) + 4 * k], bs) for k, (f, bs, _, _) in enumerate(trows) if bs]
        head = [0, 0, total, 0, blobs, len(reads)]
    else:                                                               # the span between the first and the last blob, in one read
        t = table_fields(trows, bo=[x[0] for x in trows], ck=ck)
        reads = [(lo, 0, hi - lo)] if hi > lo else []
        head = [0, 0, total, lo, hi - lo, len(reads)]
    return head + [x for r in reads for x in r] + t + offs


def model_map(rows, file_size, frows, off, ln):
    """-> (rc, covered, hits); hits: (archive row, first byte inside the chunk, bytes)."""
    end = min(off + ln, U64 - 1)
    hits, covered = [], 0
    for r in frows:
        f, n = rows[r].fdata, rows[r].len
        if f + n >= U64:                                                # a chunk whose end wraps is touched by nothing
            continue
        x, y = max(off, f), min(end, f + n)
        if x >= y:
            continue
        if not in_file(rows[r], file_size):
            return E_CORRUPT, 0, []
        hits.append((r, x - f, y - x))
        covered += y - x
    return 0, covered, hits


def model_range_read(rows, file_size, frows, off, ln, verify):
    rc, _, hits = model_map(rows, file_size, frows, off, ln)
    if rc:
        return [rc, 0] + table_fields([]) + [0]
    total, trows, rg, arow = 0, [], [], []
    for r, b, n in hits:
        take = min(n, ln - total)                                       # never more than the caller's buffer holds
        if not take:
            break
        rg += [len(trows), b, take]
        trows.append((rows[r].bo, rows[r].bs, rows[r].len, rows[r].comp))
        arow.append(r)
        total += take
    assert total <= ln
    return [0, total] + table_fields(trows, ck=b"".join(ck_of(r) for r in arow) if verify else None) + [len(arow)] + rg + arow


def model_file_ranges(rows, file_size, reqs):
    total, trows, rg, of_req, at, st, row_at = 0, [], [], [], [], [], {}
    for i, (off, ln, frows) in enumerate(reqs):
        at.append(total)
        rc, covered, hits = model_map(rows, file_size, frows, off, ln)
        if rc or covered != ln:                                         # the index does not cover the file
            st.append(E_CORRUPT)
            continue
        st.append(0)
        for r, b, n in hits:
            if not rows[r].comp:                                        # a stored chunk: the bytes asked for, as a row of their own
                rg += [len(trows), 0, n]
                trows.append((rows[r].bo + b, n, n, 0))
            else:                                                       # a compressed chunk: its whole frame, once per pass
                if r not in row_at:
                    row_at[r] = len(trows)
                    trows.append((rows[r].bo, rows[r].bs, rows[r].len, 1))
                rg += [row_at[r], b, n]
            of_req.append(i)
        total += ln
    return [total] + table_fields(trows) + [len(of_req)] + rg + of_req + [x for p in zip(at, st) for x in p]


# ---- plan_rows_read ------------------------------------------------------------------------------------------------------------------

def test_plan_rows_read(program):
    MB = 1 << 20
    text, want = [], []

    def case(rows, file_size, ids_list):
        text.append(index_text(rows, file_size))
        for ids in ids_list:
            for verify in (0, 1):
                text.append(f"R {verify} {len(ids)} " + " ".join(map(str, ids)) + "\n")
                want.append(model_rows_read(rows, file_size, ids, verify))

    # n = 0, 1, 9 (the bit column's second byte), stored and compressed mixed, a row of no bytes
    rows = [Row(k, 0, k % 3 != 1, 1000 + k, 100 * k, 100 if k != 4 else 0) for k in range(12)]
    case(rows, 100 * 12, [[], [0], [1], list(range(9)), list(range(12)), [8, 7, 3], [4], [11, 0]])
    # row sizes whose sum wraps (exactly 2^64, and one below), a blob one byte past the file and far past it, offset + size wrapping
    rows = [Row(0, 0, 1, U64 - 10, 0, 10), Row(1, 0, 1, 9, 10, 10), Row(2, 0, 1, 10, 20, 10), Row(3, 0, 0, 5, 30, 71), Row(4, 0, 0, 5, 101, 0),
            Row(5, 0, 1, 5, U64 - 4, 8), Row(6, 0, 0, 5, 100, 0), Row(7, 0, 1, 5, 30, 70)]
    case(rows, 100, [[0, 1], [0, 2], [1, 0, 2], [3], [4], [5], [6], [7], [1, 3, 0, 2], [0, 2, 3]])
    # the span against 2 * blobs + 1 MiB: at it, one below, one above (two blobs of 1000 bytes with a gap between them)
    for gap in (-1, 0, 1):
        far = 2 * 2000 + MB + gap - 1000                                # the second blob ends at 2 * sum + 1 MiB + gap
        rows = [Row(0, 0, 1, 5000, 0, 1000), Row(1, 0, 0, 0, far, 1000), Row(0, 0, 1, 7000, 10 * MB, 3000), Row(2, 0, 1, 1, 50, 0)]
        case(rows, 20 * MB, [[0, 1], [1, 0], [0, 2], [2, 0], [2, 1, 0], [0, 3, 2], [3]])   # (out of file order in the pack case too)
    check(program, "plan_rows_read", "".join(text), want)
    assert any(w[0] == E_CORRUPT and w[1] == 1 for w in want) and any(w[1] == 2 for w in want)
    assert any(not w[0] and w[3] == 0 and w[5] > 1 for w in want) and any(not w[0] and w[5] == 1 and w[3] > 0 for w in want)   # packed, and a span


# ---- ranges ----------------------------------------------------------------------------------------------------------------------------

def range_file():
    """One file of five chunks: [0,1000) compressed, [1000,1500) stored, [1500,3000) compressed, a hole, [3500,4000) stored,
    [4000,4100) compressed; behind them rows of other files."""
    rows = [Row(0, 0, 1, 1000, 0, 300), Row(0, 1000, 0, 77, 300, 500), Row(0, 1500, 1, 1500, 800, 400), Row(0, 3500, 0, 1, 1200, 500),
            Row(0, 4000, 1, 100, 1700, 60), Row(1, 0, 1, 10, 1760, 5)]
    return rows, 1765


def test_range_mapper(program):
    rows, fs = range_file()
    frows = [0, 1, 2, 3, 4]
    edges = [0, 1000, 1500, 3000, 3500, 4000, 4100]
    spans = {(0, 0), (500, 0), (4100, 10), (5000, 1), (0, 5000), (0, U64 - 1), (1, U64 - 1), (U64 - 1, 1), (U64 - 1, U64 - 1), (2, U64 - 2), (3999, 2)}
    for e in edges:                                                     # begin / end exactly on a chunk edge, one byte inside, one outside
        for d0 in (-1, 0, 1):
            for e2 in edges:
                for d1 in (-1, 0, 1):
                    lo, hi = e + d0, e2 + d1
                    if 0 <= lo <= hi:
                        spans.add((lo, hi - lo))
    spans = sorted(spans)
    text, want = [index_text(rows, fs)], []
    for off, ln in spans:
        text.append(f"M 0 {off} {ln} 5 0 1 2 3 4\n")
        rc, covered, hits = model_map(rows, fs, frows, off, ln)
        want.append([rc, covered, len(hits)] + [x for h in hits for x in h])
        for verify in (0, 1):
            text.append(f"G {verify} {off} {ln} 5 0 1 2 3 4\n")
            want.append(model_range_read(rows, fs, frows, off, ln, verify))
    # over the hole the single-range path reads short
    assert model_range_read(rows, fs, frows, 2900, 700, 0)[1] == 200 and model_map(rows, fs, frows, 0, 5000)[1] == 3600
    # a blob one past the end of the archive, a blob whose end wraps, a chunk whose end wraps, overlapping chunks (a duplicate path)
    bad = [Row(0, 0, 1, 1000, 0, 300), Row(0, 1000, 0, 0, 1266, 500), Row(0, 1500, 1, 100, U64 - 3, 10), Row(0, 1600, 1, U64 - 1000, 300, 5),
           Row(0, 1600, 0, 0, 305, 50), Row(0, 0, 1, 700, 400, 100), Row(0, 0, 0, 0, 500, 1200)]
    text.append(index_text(bad, 1765))
    for off, ln, fr in ((0, 1000, [0, 1, 2]), (0, 1001, [0, 1, 2]), (1499, 1, [0, 1, 2]), (1500, 1, [0, 1, 2]), (1600, 10, [0, 3, 4]), (0, U64 - 1, [0, 3, 4]),
                        (0, 500, [0, 5, 6]), (0, 1100, [5, 0, 6]), (600, 900, [0, 5, 6]), (0, 5000, [0, 5, 6]), (999, 1, [5, 0, 6])):
        text.append(f"M 0 {off} {ln} {len(fr)} " + " ".join(map(str, fr)) + "\n")
        rc, covered, hits = model_map(bad, 1765, fr, off, ln)
        want.append([rc, covered, len(hits)] + [x for h in hits for x in h])
        text.append(f"G 1 {off} {ln} {len(fr)} " + " ".join(map(str, fr)) + "\n")
        want.append(model_range_read(bad, 1765, fr, off, ln, 1))
    check(program, "range_mapper", "".join(text), want)
    assert any(w[0] == E_CORRUPT for w in want)


def test_file_ranges(program):
    rows, fs = range_file()
    f0 = [0, 1, 2, 3, 4]
    passes = [
        [(1600, 100, f0), (1500, 1500, f0), (2999, 1, f0)],             # one compressed chunk, three requests of one pass: one table row
        [(900, 700, f0), (1000, 500, f0), (1100, 10, f0)],              # stored and compressed mixed; stored slices are rows of their own
        [(2900, 700, f0)],                                              # over the hole: the index does not cover the file
        [(0, 100, f0), (4000, 101, f0), (3500, 600, f0), (0, 0, f0), (4100, 1, f0), (U64 - 1, 5, f0)],   # past the end, empty, wrapping
        [(0, 10, [5]), (0, 11, [5]), (990, 20, f0), (5, 5, [5])],       # two files in one pass
        [],
    ]
    text, want = [index_text(rows, fs)], []
    for reqs in passes:
        text.append(f"F {len(reqs)}\n" + "".join(f"{o} {n} {len(fr)} " + " ".join(map(str, fr)) + "\n" for o, n, fr in reqs))
        want.append(model_file_ranges(rows, fs, reqs))
    assert want[0][1] == 1 and want[2][0] == 0 and want[2][-1] == E_CORRUPT
    bad = [Row(0, 0, 1, 1000, 0, 300), Row(0, 1000, 0, 0, 1266, 500), Row(0, 1500, 1, 100, U64 - 3, 10)]
    text.append(index_text(bad, 1765))
    for reqs in ([(0, 1000, [0, 1, 2]), (900, 200, [0, 1, 2]), (10, 10, [0, 1, 2])], [(1500, 100, [0, 1, 2]), (999, 1, [0, 1, 2])]):
        text.append(f"F {len(reqs)}\n" + "".join(f"{o} {n} {len(fr)} " + " ".join(map(str, fr)) + "\n" for o, n, fr in reqs))
        want.append(model_file_ranges(bad, 1765, reqs))
    check(program, "file_ranges", "".join(text), want)


def test_table_subset_and_entry_copy(program):
    trows = [(1000 + 50 * k, 10 * (k % 4), 500 + k, k % 3 == 0) for k in range(19)]
    text, want = [], []
    for lst in ([], [0], [18], [3, 9, 10, 17], list(range(9)), list(range(19)), [8, 8, 0]):
        text.append(f"U {len(trows)} " + " ".join(f"{f} {b} {u} {int(c)}" for f, b, u, c in trows) + f" {len(lst)} " + " ".join(map(str, lst)) + "\n")
        full = table_fields(trows, ck=b"".join(ck_of(k) for k in range(len(trows))))
        bo = [full[3 + full[2] + 2 + 4 * k] for k in range(len(trows))]
        # the subset's rows lie where they lay: this table's slab
        sub = table_fields([trows[k] for k in lst], bo=[bo[k] for k in lst], total=full[1], ck=b"".join(ck_of(k) for k in lst))
        want.append(full + sub + [sum(1 for k in lst if trows[k][1])])
    for total, first, n, had in ((0, 0, 0, 0), (5, 0, 5, 0), (5, 4, 1, 3), (5, 5, 0, 7), (40, 13, 20, 64)):
        text.append(f"K {total} {first} {n} {had}\n")
        packed = bytes((i * 13 + 1) & 255 for i in range(32 * total))
        dst = bytes([9]) * had + packed[32 * first:32 * (first + n)]
        want.append([32 * (first + n), len(dst), weigh(dst)])
    check(program, "table", "".join(text), want)


# ---- ranks, batches, writers, first touch ----------------------------------------------------------------------------------------------

def model_split(w, rank, world):
    """Rank r takes rows [cut(r), cut(r + 1)): cut(r) is the first row at which the running weight (a row weighs at least 1) reaches
    r / world of the whole."""
    if world <= 1:
        return [0, len(w)]
    cum, acc = [], 0
    for x in w:
        acc += max(x, 1)
        cum.append(acc)

    def cut(r):
        if r >= world:
            return len(w)
        return next((i for i, c in enumerate(cum) if c * world >= acc * r), len(w))
    return [cut(rank), cut(rank + 1)]


def test_split_rows(program):
    text, want = [], []
    for w in ([0] * 7, [0] * 48, [5, 5, 1 << 63, 5, 5], [3, 0], [9], []):
        rows = [Row(k, 0, 1, x, 0, 0) for k, x in enumerate(w)]
        text.append(index_text(rows, 0))
        for world in (1, 2, 3, 16, 2 ** 32 - 1):
            ranks = [0, 1, 2, world // 2, world - 2, world - 1] if world > 16 else range(world)
            cuts = []
            for rank in ranks:
                text.append(f"S {rank} {world}\n")
                want.append(model_split(w, rank, world))
                cuts.append(want[-1])
            if world <= 16:                                             # monotone, and the ranks cover [0, n)
                assert cuts[0][0] == 0 and cuts[-1][1] == len(w) and all(a[1] == b[0] and a[0] <= a[1] for a, b in zip(cuts, cuts[1:] + [[len(w)] * 2]))
    check(program, "split_rows", "".join(text), want)


def test_cut_batch(program):
    # usize 100 each but row 0 (1000) and row 5 (stored, blob 40); blobs 10
    rows = [Row(k, 0, k != 5, 1000 if k == 0 else 100, 0, 40 if k == 5 else 10) for k in range(12)]
    text, want = [index_text(rows, 10 ** 6)], []
    for verify_only in (0, 1):
        cost = [(r.bs + (r.usize if r.comp else 0)) if verify_only else r.usize for r in rows]
        for i in range(12):
            for end in (i, i + 1, 12):
                for batch in (0, 1, 99, 100, 110, 199, 200, 220, 330, 399, 400, 440, 10 ** 9):
                    j, taken = i, 0
                    while j < end and (j == i or taken + cost[j] <= batch):   # at least one row, then whatever still fits
                        taken += cost[j]
                        j += 1
                    text.append(f"B {i} {end} {batch} {verify_only}\n")
                    want.append([j])
    check(program, "cut_batch", "".join(text), want)


def model_writers(off, total, paths, n_writers):
    n, parts, k0 = len(off), [], 0
    for w in range(n_writers):
        if k0 >= n:
            break
        k1 = n
        if w + 1 < n_writers:                                           # not the last writer: up to its share of the bytes, at least one row,
            k1 = max(bisect.bisect_left(off, total // n_writers * (w + 1), k0), k0 + 1)
            while k1 < n and paths[k1] == paths[k1 - 1]:                # ... and to the end of the file it is in
                k1 += 1
        parts.append((k0, k1))
        k0 = k1
    return parts


def test_cut_writers(program):
    text, want = [], []
    for paths, lens in (([0] * 8, [100] * 8),                                       # one path over the whole batch
                        ([0, 1, 1, 1, 1, 2, 3, 4], [100] * 8),                      # targets inside a run of equal paths
                        ([0, 1, 2], [5, 5, 5]), ([0], [7]), ([0, 1, 2, 3], [0] * 4),  # fewer rows than writers; total = 0
                        (list(range(10)), [1, 1, 1, 1000, 1, 1, 1, 1, 1, 1]), ([3, 3, 4, 4, 5, 5, 3, 3], [10, 20, 30, 40, 50, 60, 70, 80])):
        for lead in (0, 2):                                             # the batch begins at archive row `lead`
            rows = [Row(99, 0, 1, 1, 0, 0)] * lead + [Row(p, 0, 1, n, 0, 0) for p, n in zip(paths, lens)]
            text.append(index_text(rows, 0))
            off = [sum(lens[:k]) for k in range(len(lens))]
            for nw in (1, 2, 4):
                text.append(f"W {lead} {len(lens)} {nw} {sum(lens)} " + " ".join(map(str, off)) + "\n")
                parts = model_writers(off, sum(lens), paths, nw)
                assert parts[0][0] == 0 and parts[-1][1] == len(lens) and all(a[1] == b[0] for a, b in zip(parts, parts[1:])) and len(parts) <= nw
                assert all(paths[b[0]] != paths[b[0] - 1] for b in parts[1:])        # cut only where the path changes
                want.append([len(parts)] + [x for p in parts for x in p])
    check(program, "cut_writers", "".join(text), want)


def test_first_touch(program):
    text, want = [], []
    cases = [[0, 0, 1, 2, 2, 2, 3],                                     # adjacent duplicates
             [0, 1, 1, 0, 2],                                           # a duplicate that is not adjacent
             [5], [], [1, 1, 1, 1], [0, 1, 0, 1, 0]]
    for paths in cases:
        rows = []
        for k, p in enumerate(paths):
            seq = sum(1 for q in paths[:k] if q == p)
            stored = k == len(paths) - 1 or k == 1                      # (the last chunk stored: its length is its blob's)
            rows.append(Row(p, 1000 * seq, not stored, 1000 if not stored else 1, 0, 333 + k, seq))
        text.append(index_text(rows, 10 ** 6))
        n = len(paths)
        uniq = sorted(set(paths), key=str)
        adjacent = all(paths[k] == paths[k - 1] or paths[k] not in paths[:k] for k in range(1, n))
        for b, e in sorted({(0, n), (0, n // 2), (n // 2, n), (min(1, n), max(n - 1, min(1, n))), (n, n)}):   # rank boundaries inside a file too
            for per_rank in (0, 1):
                text.append(f"T {b} {e} {per_rank}\n")
                if per_rank:
                    first = [int(b <= k < e and paths[k] not in paths[b:k]) for k in range(n)]
                    final = [(p, max((r.fdata + r.len) % U64 for r in rows if r.path == p)) for p in uniq]
                else:
                    first, final = [int(paths[k] not in paths[:k]) for k in range(n)], []
                want.append([int(adjacent), len(uniq), n] + first + [len(final)] + [x for f in final for x in f])
    check(program, "first_touch", "".join(text), want)
    assert any(w[0] == 0 for w in want)


# ---- the sidecar's layout --------------------------------------------------------------------------------------------------------------

def entries_of(n):
    """One entry per 128 KiB block of a row of more than one block and below 4 GiB."""
    return (n + BLK - 1) // BLK if BLK < n < 2 ** 32 else 0


def test_sidecar_layout(program):
    lens = [BLK, BLK + 1, 5, 3 * BLK, 2 ** 32, 2 ** 32 - 1 - 7 * BLK * 4000, 2 ** 40, 0]
    lens[5] = 9 * BLK + 1
    rows = [Row(k, 0, k % 2 == 0, n if k % 2 == 0 else 1, 0, n if k % 2 else 1) for k, n in enumerate(lens)]   # stored rows: the blob's length counts
    n_entries = sum(entries_of(r.len) for r in rows)
    assert [entries_of(n) for n in lens] == [0, 2, 0, 3, 0, 10, 0, 0]

    def sidecar(magic=b"ZNPYB3T1", log=17, zero=0, n_rows=len(rows), n_ent=n_entries, body=n_entries, tail=b""):
        return magic + struct.pack("<IIQQ", log, zero, n_rows, n_ent) + bytes(range(32)) * body + tail

    good = sidecar()
    files = [good, b"", good[:31], good[:32], good[:33], sidecar(tail=b"\x01" * 31), sidecar(tail=b"\x01"),        # 0, 31, 32, 33 bytes; a partial entry
             sidecar(magic=b"ZNPYB3T2"), sidecar(log=16), sidecar(zero=1), sidecar(n_rows=len(rows) + 1), sidecar(n_rows=len(rows) - 1),
             sidecar(n_ent=n_entries + 1), sidecar(n_ent=n_entries - 1),
             sidecar(n_ent=n_entries + 1, body=n_entries + 1), sidecar(n_ent=n_entries - 1, body=n_entries - 1)]         # whole, but not the index's sum
    first = [sum(entries_of(r.len) for r in rows[:k]) for k in range(len(rows) + 1)]
    text, want = [index_text(rows, 0)], []
    for k, f in enumerate(files):
        text.append(f"C {len(f)} {f.hex()}\n")
        want.append([1] + first if k == 0 else [0])
    text.append(index_text([], 0))                                      # an empty index: the header alone
    for f in (sidecar(n_rows=0, n_ent=0, body=0), sidecar(n_rows=0, n_ent=1, body=1), good[:32]):
        text.append(f"C {len(f)} {f.hex()}\n")
        want.append([1, 0] if f[16:32] == bytes(16) and len(f) == 32 else [0])
    check(program, "sidecar_layout", "".join(text), want)


def test_case_counts():
    """(runs last: what the tests above compared)"""
    print("read_plan cases:", ", ".join(f"{k} {v}" for k, v in sorted(N_CASES.items())))
