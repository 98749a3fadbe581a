"""The host planning of znippy_inflate_batch, znippy_targz_find_batch and znippy_gunzip_batch (znippy_amd/csrc/host/deflate_batch.cc,
with gz_plan.cc and range_plan.cc) as a stand-alone host program under AddressSanitizer and UBSan.  The stages between the device
passes read words the kernels wrote while decoding untrusted input; a correct kernel never writes a contradictory one, so the cases
here hand the stages such words directly: every case must give the expected lists and statuses, never a sanitizer report.  Every
array the program hands to the module is a heap copy of exactly the length named, so a read past it is caught.

The expected values are worked out here from the rules of include/znippy_hip.h (placement, limits, candidate rule, status
precedence), from zlib (CRCs) and from tests/gz_model.py (the kept candidates of real gzip files), not from the module.

The list limits (2^30 candidates, 2^30 chunks, 2^40 bytes of scratch, 0x7FFFFFF0 pieces) need source data nobody can allocate, so
those cases run further builds of the program whose limits are overridden at compile time.  The "cannot happen" E_NOMEM returns of
gz_candidates and gz_decode_plan stay unreached: no input, contradictory or not, makes a list longer than gz_kept_max."""
import os
import shutil
import subprocess
import zlib

import pytest

import deflate_build as DB
import gen
import gz_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "znippy_amd", "csrc", "host")
E_INVAL, E_NOMEM, E_DST_SMALL, E_CORRUPT, E_UNSUPPORTED, E_CHECKSUM = -1, -3, -4, -5, -6, -7
FLUSH, MEMBER = 0, 1
BOUNDARY, TRAILER, ERROR, ROOM = 0, 1, 2, 3
NEXT_MEMBER, NEXT_END = 0, 1
PIECE = 32 << 10
CHUNK = 4096
M64 = (1 << 64) - 1
SENTINEL = 7777          # what the program fills the caller's output arrays with before a call
SIZES = dict(item=32, chunk=8, cand=24, probe=40, run=16, inflate_item=40, single=24)

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "deflate_batch.h"
using namespace zn;
// device bases: only ever added to
static uint8_t *const SRC = (uint8_t *)(uintptr_t)0x100000000000ull, *const OUT = (uint8_t *)(uintptr_t)0x200000000000ull,
                      *const SCRATCH = (uint8_t *)(uintptr_t)0x300000000000ull;
// a heap array of exactly n values
template <typename T> struct Arr {
    T *p;
    explicit Arr(size_t n) : p((T *)malloc(n ? n * sizeof(T) : 1)) {}
    Arr(const Arr &) = delete;
    ~Arr() { free(p); }
    operator T *() const { return p; }
};
static bool u64(uint64_t *v) { unsigned long long x; if (scanf("%llu", &x) != 1) return false; *v = x; return true; }
static bool u32(uint32_t *v) { uint64_t x; if (!u64(&x)) return false; *v = (uint32_t)x; return true; }
static bool i32(int32_t *v) { long long x; if (scanf("%lld", &x) != 1) return false; *v = (int32_t)x; return true; }
template <typename T> static void line(const char *name, const T *p, size_t n) {
    printf("%s", name);
    for (size_t i = 0; i < n; i++) printf(" %lld", (long long)p[i]);
    printf("\n");
}
static void line_u64(const char *name, const uint64_t *p, size_t n) {
    printf("%s", name);
    for (size_t i = 0; i < n; i++) printf(" %" PRIu64, p[i]);
    printf("\n");
}
// an exact-length copy: a vector built from a range allocates just that
template <typename T> static std::vector<T> exact(const std::vector<T> &v) { return std::vector<T>(v.begin(), v.end()); }

// "P n src_cap out_cap has_off" + n x "src_off src_len out_off out_len" -> "place" + n x "status dst"
static int placement() {
    uint64_t n, src_cap, out_cap, has_off;
    if (!u64(&n) || !u64(&src_cap) || !u64(&out_cap) || !u64(&has_off)) return 2;
    Placement p;
    printf("place");
    for (uint64_t i = 0; i < n; i++) {
        uint64_t so, sl, oo, ol, dst = 0;
        if (!u64(&so) || !u64(&sl) || !u64(&oo) || !u64(&ol)) return 2;
        const int32_t st = place_item(p, so, sl, src_cap, has_off ? &oo : nullptr, ol, out_cap, &dst);
        printf(" %d %" PRIu64, st, st ? 0 : dst);
    }
    printf("\n");
    return 0;
}

// "I n src_cap out_cap has_off has_method has_crc" + n x "src_off src_len out_off out_len method crc", then n_items x "status crc"
static int inflate() {
    uint64_t n, src_cap, out_cap, has_off, has_method, has_crc;
    if (!u64(&n) || !u64(&src_cap) || !u64(&out_cap) || !u64(&has_off) || !u64(&has_method) || !u64(&has_crc)) return 2;
    Arr<uint64_t> so(n), sl(n), oo(n), ol(n);
    Arr<uint8_t> method(n);
    Arr<uint32_t> crc(n);
    for (uint64_t i = 0; i < n; i++) {
        uint32_t m;
        if (!u64(&so[i]) || !u64(&sl[i]) || !u64(&oo[i]) || !u64(&ol[i]) || !u32(&m) || !u32(&crc[i])) return 2;
        method[i] = (uint8_t)m;
    }
    InflateBatch b;
    inflate_admit(InflateCall{SRC, src_cap, so, sl, has_method ? method.p : nullptr, OUT, out_cap, has_off ? oo.p : nullptr, ol, has_crc ? crc.p : nullptr, n}, b);
    if (b.st.size() != n || b.item_of.size() != b.items.size() || b.h_st.size() != b.items.size() || b.h_crc.size() != b.items.size()) return 3;
    line("st", b.st.data(), n);
    printf("items");
    for (size_t k = 0; k < b.items.size(); k++) {
        const InflateItem &it = b.items[k];
        printf(" %u %" PRIu64 " %" PRIu64 " %u %u %u %u %u %u", b.item_of[k], (uint64_t)(it.src - SRC), (uint64_t)(it.dst - OUT), it.src_len, it.out_len, it.method,
               it.want_crc, it.has_crc, it.pad);
    }
    printf("\n");
    for (size_t k = 0; k < b.items.size(); k++)
        if (!i32(&b.h_st[k]) || !u32(&b.h_crc[k])) return 0;  // (the case ends here)
    Arr<int32_t> status(n);
    Arr<uint32_t> crc_out(n);
    for (uint64_t i = 0; i < n; i++) { status[i] = 7777; crc_out[i] = 7777; }
    inflate_scatter(b, n, status, crc_out);
    line("status", status.p, n);
    line("crc_out", crc_out.p, n);
    inflate_scatter(b, n, nullptr, nullptr);
    return 0;
}

// "C src dst len" -> "pieces" + per piece "src dst len"
static void print_pieces(const std::vector<RangePiece> &pieces, const uint8_t *src0, const uint8_t *dst0) {
    printf("pieces");
    for (const RangePiece &p : pieces) printf(" %" PRIu64 " %" PRIu64 " %u", (uint64_t)(p.src - src0), (uint64_t)(p.dst - dst0), p.len);
    printf("\n");
}
static int cut() {
    uint64_t src, dst, len;
    if (!u64(&src) || !u64(&dst) || !u64(&len)) return 2;
    std::vector<RangePiece> pieces(1, RangePiece{nullptr, nullptr, 77, 0});  // (what others left: must stay)
    range_cut_pieces(SCRATCH + src, OUT + dst, len, pieces);
    if (pieces[0].len != 77) return 3;
    pieces.erase(pieces.begin());
    print_pieces(pieces, SCRATCH, OUT);
    return 0;
}

// "T n src_cap out_cap scan_cap has_whole has_scanned out_shift" + n x "src_off src_len whole", then n_items x "status off len scanned"
static int targz() {
    uint64_t n, src_cap, out_cap, scan_cap, has_whole, has_scanned, shift;
    if (!u64(&n) || !u64(&src_cap) || !u64(&out_cap) || !u64(&scan_cap) || !u64(&has_whole) || !u64(&has_scanned) || !u64(&shift)) return 2;
    Arr<uint64_t> so(n), sl(n), out_off(n), out_len(n), scanned(n);
    Arr<uint8_t> whole(n);
    for (uint64_t i = 0; i < n; i++) {
        uint32_t w;
        if (!u64(&so[i]) || !u64(&sl[i]) || !u32(&w)) return 2;
        whole[i] = (uint8_t)w;
        out_off[i] = out_len[i] = scanned[i] = 7777;
    }
    const TargzCall call{SRC, src_cap, so, sl, has_whole ? whole.p : nullptr, n, scan_cap, OUT + shift, out_cap, out_off, out_len, has_scanned ? scanned.p : nullptr};
    TargzBatch b;
    const int rc = targz_admit(call, b);
    printf("admit %d\n", rc);
    if (rc) return 0;
    if (b.st.size() != n || b.item_of.size() != b.items.size() || b.slice.size() != b.items.size() || b.res.size() != b.items.size()) return 3;
    line("st", b.st.data(), n);
    line_u64("out_off", out_off, n);
    line_u64("out_len", out_len, n);
    line_u64("scanned", scanned, n);
    printf("need %" PRIu64 "\nitems", b.need);
    for (size_t k = 0; k < b.items.size(); k++) {
        const TargzItem &it = b.items[k];
        if (it.scratch || it.pad) return 3;
        printf(" %u %" PRIu64 " %u %u %u %" PRIu64, b.item_of[k], (uint64_t)(it.src - SRC), it.src_len, it.cap, it.whole, b.slice[k]);
    }
    printf("\n");
    size_t max_pieces = 0;
    const int brc = targz_piece_bound(out_cap, b.items.size(), &max_pieces);
    printf("bound %d %zu\n", brc, max_pieces);
    targz_bind(b, SCRATCH);
    for (size_t k = 0; k < b.items.size(); k++)
        if (b.items[k].scratch != SCRATCH + b.slice[k]) return 3;
    std::vector<TargzResult> res(b.items.size());
    for (TargzResult &r : res) {
        r.pad = 0;
        if (!i32(&r.status) || !u64(&r.off) || !u64(&r.len) || !u64(&r.scanned)) return 0;  // (the case ends here)
    }
    b.res = exact(res);
    targz_pack(call, b);
    line("st", b.st.data(), n);
    line_u64("out_off", out_off, n);
    line_u64("out_len", out_len, n);
    line_u64("scanned", scanned, n);
    print_pieces(b.pieces, SCRATCH, OUT + shift);
    return 0;
}

// "G n src_cap out_cap has_off has_counts seg_min" + n x "src_off src_len out_off room", then the stages' inputs (see gunzip() in the test)
static int gunzip() {
    uint64_t n, src_cap, out_cap, has_off, has_counts, seg_min;
    if (!u64(&n) || !u64(&src_cap) || !u64(&out_cap) || !u64(&has_off) || !u64(&has_counts) || !u64(&seg_min)) return 2;
    Arr<uint64_t> so(n), sl(n), oo(n), room(n), out_len(n);
    Arr<uint32_t> members(n), segments(n);
    for (uint64_t i = 0; i < n; i++) {
        if (!u64(&so[i]) || !u64(&sl[i]) || !u64(&oo[i]) || !u64(&room[i])) return 2;
        out_len[i] = 7777; members[i] = segments[i] = 7777;
    }
    const GzCall call{SRC, src_cap, so, sl, n, OUT, out_cap, has_off ? oo.p : nullptr, room, seg_min, out_len, has_counts ? members.p : nullptr,
                      has_counts ? segments.p : nullptr};
    GzBatch b;
    int rc = gz_admit(call, b);
    printf("admit %d\n", rc);
    if (rc) return 0;
    const size_t n_items = b.items.size();
    if (b.st.size() != n || b.item_of.size() != n_items || b.count.size() != n_items) return 3;
    line("st", b.st.data(), n);
    line_u64("out_len", out_len, n);
    line("members", members.p, n);
    line("segments", segments.p, n);
    printf("items");
    for (size_t k = 0; k < n_items; k++) {
        const GzItem &it = b.items[k];
        printf(" %u %" PRIu64 " %" PRIu64 " %u %u %u %u", b.item_of[k], (uint64_t)(it.src - SRC), (uint64_t)(it.dst - OUT), it.src_len, it.room, it.cand_base, it.cand_cap);
    }
    printf("\nchunks");
    for (const GzScanChunk &c : b.chunks) printf(" %u %u", c.item, c.off);
    printf("\ncand_total %" PRIu64 " %zu\n", b.cand_total, gz_kept_max(b));  // (and gz_kept_max)
    const GzLayout l = gz_layout(b);
    printf("layout %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", l.items, l.chunks, l.count, l.raw, l.cands, l.stops, l.recs, l.runs, l.run_st,
           l.crc_items, l.crc_st, l.crc_got, l.single_list, l.single_res, l.bytes);
    printf("sizes %zu %zu %zu %zu %zu %zu %zu\n", sizeof(GzItem), sizeof(GzScanChunk), sizeof(GzCand), sizeof(GzProbe), sizeof(GzRun), sizeof(InflateItem),
           sizeof(GzSingle));
    // the scan's answer
    std::vector<uint32_t> count(n_items);
    for (uint32_t &v : count)
        if (!u32(&v)) return 0;  // (the case ends here)
    b.count = exact(count);
    const uint64_t raw_end = gz_raw_end(b);
    printf("raw_end %" PRIu64 "\n", raw_end);
    std::vector<uint64_t> raw(raw_end);
    for (uint64_t &v : raw)
        if (!u64(&v)) return 0;  // (the case ends here)
    b.raw = exact(raw);
    rc = gz_candidates(b, seg_min);
    printf("candidates %d\n", rc);
    if (rc) return 0;
    if (b.first_cand.size() != b.probed.size() + 1 || b.recs.size() != b.cands.size() || b.sres.size() != b.single.size()) return 3;
    printf("cands");
    for (const GzCand &c : b.cands) printf(" %u %u %u %u %u %u", c.item, c.pos, c.kind, c.stop0, c.stop1, c.pad);
    printf("\n");
    line("stops", b.stops.data(), b.stops.size());
    line("single", b.single.data(), b.single.size());
    line("probed", b.probed.data(), b.probed.size());
    line("first_cand", b.first_cand.data(), b.first_cand.size());
    // the probe's and the single pass's answers
    std::vector<GzProbe> recs(b.cands.size());
    for (GzProbe &r : recs)
        if (!u32(&r.data_start) || !u32(&r.end_kind) || !u32(&r.end_pos) || !i32(&r.status) || !u64(&r.out) || !u32(&r.reach) || !u32(&r.crc) || !u32(&r.isize) ||
            !i32(&r.next)) return 0;  // (the case ends here)
    std::vector<GzSingle> sres(b.single.size());
    for (GzSingle &r : sres) {
        r.pad = 0;
        if (!i32(&r.status) || !u32(&r.out_len) || !u32(&r.members) || !u32(&r.crc0) || !u32(&r.len0)) return 0;  // (or here)
    }
    b.recs = exact(recs);
    b.sres = exact(sres);
    rc = gz_decode_plan(b);
    printf("plan %d\n", rc);
    if (rc) return 0;
    if (b.item_st.size() != n_items || b.run_item.size() != b.h_runs.size() || b.crc_of_run.size() != b.runs.size() || b.run_st.size() != b.h_runs.size() ||
        b.crc_st.size() != b.crc_items.size() || b.crc_got.size() != b.crc_items.size() || b.plans.size() != b.probed.size())
        return 3;
    line("item_st", b.item_st.data(), n_items);
    printf("runs");
    for (size_t r = 0; r < b.h_runs.size(); r++) printf(" %u %u %u %u %u", b.run_item[r], b.h_runs[r].item, b.h_runs[r].src_start, b.h_runs[r].out_off, b.h_runs[r].out_len);
    printf("\ncrc_items");
    for (const InflateItem &it : b.crc_items) {
        if (it.src || it.src_len || it.method != 8 || it.pad) return 3;
        printf(" %" PRIu64 " %u %u %u", (uint64_t)(it.dst - OUT), it.out_len, it.has_crc, it.want_crc);
    }
    printf("\n");
    line("crc_item_of", b.crc_item_of.data(), b.crc_item_of.size());
    printf("crc_of_run");
    for (size_t r = 0; r < b.runs.size(); r++) printf(" %lld", b.runs[r].out_len ? (long long)b.crc_of_run[r] : -1ll);
    printf("\n");
    // the decode and CRC launches' answers
    std::vector<int32_t> run_st(b.h_runs.size()), crc_st(b.crc_items.size());
    std::vector<uint32_t> crc_got(b.crc_items.size());
    for (int32_t &v : run_st)
        if (!i32(&v)) return 0;  // (the case ends here)
    for (size_t c = 0; c < crc_st.size(); c++)
        if (!i32(&crc_st[c]) || !u32(&crc_got[c])) return 0;  // (or here)
    b.run_st = exact(run_st);
    b.crc_st = exact(crc_st);
    b.crc_got = exact(crc_got);
    gz_verdict(call, b);
    line("st", b.st.data(), n);
    line_u64("out_len", out_len, n);
    line("members", members.p, n);
    line("segments", segments.p, n);
    return 0;
}

int main() {
    printf("limits %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u\n", GZ_LIST_MAX, TARGZ_NEED_MAX, RR_ITEMS_MAX, RANGE_PIECE, GZ_SCAN_CHUNK);
    char what;
    if (scanf(" %c", &what) != 1) return 0;
    switch (what) {
    case 'P': return placement();
    case 'I': return inflate();
    case 'C': return cut();
    case 'T': return targz();
    case 'G': return gunzip();
    }
    return 2;
}
"""


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
                   ["-I", HOST, str(main)] + [os.path.join(HOST, f) for f in ("deflate_batch.cc", "gz_plan.cc", "range_plan.cc")] + ["-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_program(tmp_path_factory.mktemp("deflate_batch"), "plan")


@pytest.fixture(scope="module")
def small_limits(tmp_path_factory):
    return build_program(tmp_path_factory.mktemp("deflate_batch_limits"), "plan_small", ["-DZN_GZ_LIST_MAX=40", "-DZN_TARGZ_NEED_MAX=4096", "-DZN_RR_ITEMS_MAX=40"])


@pytest.fixture(scope="module")
def small_chunk_limit(tmp_path_factory):
    """(the chunk limit alone: at one value with the candidate limit it is never the one that is reached — an item adds
    16 + len / 256 candidates and at most len / 4096 + 1 chunks)"""
    return build_program(tmp_path_factory.mktemp("deflate_batch_chunks"), "plan_chunks", ["-DZN_GZ_CHUNKS_MAX=5"])


def run(exe, text):
    """-> {first word of a line: [its integers]}; a word that comes twice (before and after a stage) gets a list of both"""
    r = subprocess.run([exe], input=text + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-3000:])
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        out.setdefault(w[0], []).append([int(v) for v in w[1:]])
    return out


def rows(vals, k):
    assert len(vals) % k == 0
    return [tuple(vals[i:i + k]) for i in range(0, len(vals), k)]


def lines(*parts):
    return "\n".join(" ".join(str(v) for v in p) for p in parts)


# ---- the placement rule ----

def place(program, items, src_cap=1 << 33, out_cap=1 << 33, has_off=False):
    """items: (src_off, src_len, out_off, out_len) -> [(status, dst)]"""
    return rows(run(program, lines(("P", len(items), src_cap, out_cap, int(has_off)), *items))["place"][0], 2)


def test_placement_packed_and_wrapped(program):
    # back to back, refused items taking their room too
    assert place(program, [(0, 5, 0, 10), (0, 5, 0, 0), (1 << 40, 5, 0, 7), (0, 5, 0, 3)], out_cap=20) == [(0, 0), (0, 10), (E_INVAL, 0), (0, 17)]
    # the sum wraps at the second item: it does not fit, and where the ones behind it lie is not known
    assert place(program, [(0, 1, 0, 10), (0, 1, 0, M64 - 4), (0, 1, 0, 20), (0, 1, 0, 3)], out_cap=M64) == \
        [(0, 0), (E_DST_SMALL, 0), (E_DST_SMALL, 0), (E_DST_SMALL, 0)]
    # ... with offsets given, every item stands alone
    assert place(program, [(0, 1, 0, 10), (0, 1, 5, M64 - 4), (0, 1, 90, 20), (0, 1, M64, 3)], out_cap=200, has_off=True) == \
        [(0, 0), (E_DST_SMALL, 0), (0, 90), (E_DST_SMALL, 0)]


def test_placement_regions_and_precedence(program):
    G4 = 1 << 32
    assert place(program, [(M64 - 3, 8, 0, 1)]) == [(E_INVAL, 0)]                         # src_off + src_len wraps
    assert place(program, [(100, 1, 0, 1), (99, 1, 0, 1), (101, 0, 0, 1)], src_cap=100) == [(E_INVAL, 0), (0, 1), (E_INVAL, 0)]
    assert place(program, [(0, 1, 0, 11)], out_cap=10) == [(E_DST_SMALL, 0)]
    assert place(program, [(0, 1, 1, 10), (0, 1, 0, 10)], out_cap=10, has_off=True) == [(E_DST_SMALL, 0), (0, 0)]
    # 2^32 - 1 is taken, 2^32 is not, for either length
    assert place(program, [(0, G4 - 1, 0, G4 - 1), (0, G4, 0, 1), (0, 1, 0, G4)], has_off=True) == [(0, 0), (E_UNSUPPORTED, 0), (E_UNSUPPORTED, 0)]
    # an item that fails two checks shows the earlier one: source region, then output region, then the 4 GiB limit
    assert place(program, [(M64, G4, 0, G4)], out_cap=10) == [(E_INVAL, 0)]
    assert place(program, [(0, G4, 0, G4)], out_cap=10) == [(E_DST_SMALL, 0)]


# ---- znippy_inflate_batch ----

def inflate(program, items, results=None, src_cap=1 << 33, out_cap=1 << 33, has_off=True, has_method=True, has_crc=True):
    """items: (src_off, src_len, out_off, out_len, method, crc); results: per list entry (status, crc)"""
    return run(program, lines(("I", len(items), src_cap, out_cap, int(has_off), int(has_method), int(has_crc)), *items, *(results or [])))


def test_inflate_admit_and_scatter(program):
    G4 = 1 << 32
    items = [(M64, 5, 0, G4, 9, 1),          # everything wrong: the source region speaks first
             (0, 5, 0, 6, 8, 11),            # fine
             (0, G4, 0, 5, 9, 2),            # 4 GiB before the method
             (0, 5, 50, 5, 9, 3),            # a method that is neither
             (0, 5, 60, 6, 0, 4),            # stored, the lengths differ
             (7, 5, 70, 5, 0, 12),           # stored, fine
             (0, 5, 95, 6, 9, 5),            # the output region before the method
             (20, 0, 80, 0, 8, 13)]          # nothing to nothing
    got = inflate(program, items, [(0, 101), (E_CORRUPT, 0), (E_CHECKSUM, 103)], out_cap=100)
    assert got["st"][0] == [E_INVAL, 0, E_UNSUPPORTED, E_UNSUPPORTED, E_CORRUPT, 0, E_DST_SMALL, 0]
    # (item, src, dst, src_len, out_len, method, want_crc, has_crc, pad)
    assert rows(got["items"][0], 9) == [(1, 0, 0, 5, 6, 8, 11, 1, 0), (5, 7, 70, 5, 5, 0, 12, 1, 0), (7, 20, 80, 0, 0, 8, 13, 1, 0)]
    assert got["status"][0] == [E_INVAL, 0, E_UNSUPPORTED, E_UNSUPPORTED, E_CORRUPT, E_CORRUPT, E_DST_SMALL, E_CHECKSUM]
    assert got["crc_out"][0] == [0, 101, 0, 0, 0, 0, 0, 103]
    # no methods, no CRCs, packed: all DEFLATE, nothing to compare with
    got = inflate(program, [(0, 5, 0, 6, 0, 9), (0, 5, 0, 7, 0, 9)], [(0, 1), (0, 2)], has_off=False, has_method=False, has_crc=False)
    assert rows(got["items"][0], 9) == [(0, 0, 0, 5, 6, 8, 0, 0, 0), (1, 0, 6, 5, 7, 8, 0, 0, 0)]
    assert got["status"][0] == [0, 0] and got["crc_out"][0] == [1, 2]
    # nothing passes: an empty list, and the statuses all the same
    got = inflate(program, [(M64, 1, 0, 1, 8, 0)], [])
    assert got["items"][0] == [] and got["status"][0] == [E_INVAL] and got["crc_out"][0] == [0]


def test_inflate_lengths_at_4gib(program):
    G4 = 1 << 32
    got = inflate(program, [(0, G4 - 1, 0, G4 - 1, 8, 0), (0, G4, G4, 1, 8, 0), (0, 1, G4, G4, 8, 0), (0, G4 - 1, G4, G4 - 1, 0, 0)])
    assert got["st"][0] == [0, E_UNSUPPORTED, E_UNSUPPORTED, 0]
    assert rows(got["items"][0], 9) == [(0, 0, 0, G4 - 1, G4 - 1, 8, 0, 1, 0), (3, 0, G4, G4 - 1, G4 - 1, 0, 0, 1, 0)]


# ---- the piece helper, znippy_targz_find_batch ----

def check_pieces(pieces, src, dst, length):
    """the rule of the gather's list for one member: (src, dst, len) pieces that tile it, later ones on 128-byte lines"""
    at = 0
    for k, (s, d, n) in enumerate(pieces):
        assert (s, d) == (src + at, dst + at) and 0 < n <= PIECE
        assert k == 0 or d % 128 == 0
        at += n
    assert at == length


def test_piece_cutting(program):
    for shift in (0, 1, 127):
        for length in (0, 1, PIECE - 128, PIECE - 127, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE - 127, 2 * PIECE, 2 * PIECE + 1, 3 * PIECE + 5):
            dst = 4096 + shift
            pieces = rows(run(program, f"C 77 {dst} {length}")["pieces"][0], 3)
            check_pieces(pieces, 77, dst, length)
            first = min(length, PIECE - shift)                         # the first piece ends on a line, or the member
            assert len(pieces) == (1 if length else 0) + -(-(length - first) // PIECE)
            assert len(pieces) <= length // PIECE + 2


def targz(program, items, results=None, src_cap=1 << 33, out_cap=1 << 20, scan_cap=1 << 20, has_whole=True, has_scanned=True, shift=0):
    """items: (src_off, src_len, whole); results: per list entry (status, off, len, scanned)"""
    return run(program, lines(("T", len(items), src_cap, out_cap, scan_cap, int(has_whole), int(has_scanned), shift), *items, *(results or [])))


def test_targz_admit(program):
    G4 = 1 << 32
    # scan_cap below, between and above 1032 * len + 512 of the items; 4 GiB - 16 at the most; slices rounded up to 16 bytes
    items = [(0, 1, 1), (M64, 1, 1), (10, 100, 0), (1 << 33, 0, 2), (0, G4, 1), (0, G4 - 1, 1)]
    for scan_cap, caps in ((1000, [1000, 1000, 512, 1000]), (1544 + 7, [1544, 1551, 512, 1551]), (1 << 50, [1544, 103_712, 512, 0xFFFFFFF0])):
        got = targz(program, items, scan_cap=scan_cap)
        assert got["admit"][0] == [0]
        assert got["st"][0] == [0, E_INVAL, 0, 0, E_UNSUPPORTED, 0]
        assert got["out_off"][0] == got["out_len"][0] == got["scanned"][0] == [0] * 6
        slices, need = [], 0
        for c in caps:
            slices.append(need)
            need += (c + 15) // 16 * 16
        # (item, src, src_len, cap, whole, slice)
        assert rows(got["items"][0], 6) == [(0, 0, 1, caps[0], 1, slices[0]), (2, 10, 100, caps[1], 0, slices[1]), (3, 1 << 33, 0, caps[2], 1, slices[2]),
                                            (5, 0, G4 - 1, caps[3], 1, slices[3])]
        assert got["need"][0] == [need]
        assert got["bound"][0] == [0, (1 << 20) // PIECE + 8]
    # no `whole`: every item is a whole file; no `scanned`: not written
    got = targz(program, [(0, 1, 0)], has_whole=False, has_scanned=False)
    assert rows(got["items"][0], 6) == [(0, 0, 1, 1544, 1, 0)] and got["scanned"][0] == [SENTINEL]


def test_targz_pack(program):
    # three members found; the second does not fit what is left of out_cap, the third does.  Items 1 and 4 are not in the list.
    items = [(0, 100, 1), (M64, 1, 1), (0, 100, 1), (0, 100, 1), (0, 1 << 32, 1), (0, 100, 1)]
    cap = 103_712
    res = [(0, 512, 1000, 2048), (0, 1024, 3001, 5000), (0, 0, 3000, 4000), (-9, 5, 5, 777)]
    got = targz(program, items, res, out_cap=4000)
    assert got["st"][1] == [0, E_INVAL, E_DST_SMALL, 0, E_UNSUPPORTED, -9]
    assert got["out_off"][1] == [0, 0, 0, 1000, 0, 0] and got["out_len"][1] == [1000, 0, 0, 3000, 0, 0]
    assert got["scanned"][1] == [2048, 0, 5000, 4000, 0, 777]
    slice_ = (cap + 15) // 16 * 16
    assert rows(got["pieces"][0], 3) == [(512, 0, 1000), (2 * slice_, 1000, 3000)]
    # off + len one past cap, off alone past cap, and sums that wrap: E_CORRUPT, no room taken, no piece; the member behind them is placed at 0
    for off, length in ((cap - 9, 10), (cap + 1, 0), (M64, 2), (2, M64), (M64, M64)):
        got = targz(program, items[:1] + items[2:4], [(0, off, length, 1), (0, cap - 10, 10, 2), (0, cap, 0, 3)], out_cap=4000)
        assert got["st"][1] == [E_CORRUPT, 0, 0]
        assert got["out_off"][1] == [0, 0, 10] and got["out_len"][1] == [0, 10, 0]
        assert rows(got["pieces"][0], 3) == [(slice_ + cap - 10, 0, 10)]
    # out_cap 0: only members of no bytes fit
    got = targz(program, [(0, 100, 1), (0, 100, 1)], [(0, 0, 0, 1), (0, 0, 1, 1)], out_cap=0)
    assert got["st"][1] == [0, E_DST_SMALL] and got["pieces"][0] == []


def test_targz_pieces(program):
    # members whose destinations fall at every alignment, lengths around the piece size; the count stays within the bound
    for shift in (0, 1, 127):
        lens = [PIECE - 1, 1, PIECE, PIECE + 1, 0, 2 * PIECE + 127, 126, 3]
        out_cap = sum(lens)
        got = targz(program, [(0, 1 << 20, 1)] * len(lens), [(0, 16 * k, n, 0) for k, n in enumerate(lens)], out_cap=out_cap, scan_cap=1 << 20, shift=shift)
        assert got["st"][1] == [0] * len(lens)
        pieces = rows(got["pieces"][0], 3)
        assert len(pieces) <= got["bound"][0][1] == out_cap // PIECE + 2 * len(lens)
        packed, at = 0, 0
        for k, n in enumerate(lens):
            assert (got["out_off"][1][k], got["out_len"][1][k]) == (packed, n)
            mine = []
            while at < len(pieces) and pieces[at][1] < packed + n:
                mine.append(pieces[at])
                at += 1
            # (the program prints destinations relative to d_out: the line rule is about the address)
            check_pieces([(s, d + shift, ln) for s, d, ln in mine], k * (1 << 20) + 16 * k, packed + shift, n)
            packed += n
        assert at == len(pieces)


def test_targz_limits(small_limits):
    assert run(small_limits, "")["limits"][0] == [40, 4096, 40, PIECE, CHUNK]
    # 4096 bytes of scratch: 2 x 2048 is the limit, 16 more is beyond it
    assert targz(small_limits, [(0, 100, 1)] * 2, scan_cap=2048)["admit"][0] == [0]
    assert targz(small_limits, [(0, 100, 1)] * 2 + [(0, 100, 1)], scan_cap=2048)["admit"][0] == [E_NOMEM]
    assert targz(small_limits, [(0, 100, 1), (M64, 1, 1), (0, 100, 1)], scan_cap=2049)["admit"][0] == [E_NOMEM]
    # 40 pieces
    assert targz(small_limits, [(0, 1, 1)] * 4, out_cap=32 * PIECE + PIECE - 1, scan_cap=512)["bound"][0] == [0, 40]
    assert targz(small_limits, [(0, 1, 1)] * 4, out_cap=33 * PIECE, scan_cap=512)["bound"][0] == [E_NOMEM, 41]


# ---- znippy_gunzip_batch ----

def gunzip(program, items, counts=None, raw=None, recs=None, sres=None, run_st=None, crcs=None, src_cap=1 << 33, out_cap=1 << 33, has_off=False,
           has_counts=True, seg_min=1):
    """items: (src_off, src_len, out_off, room); counts: per list entry; raw: the raw list up to raw_end, as (pos, kind) or None
    for an entry nobody wrote; recs: per kept candidate (data_start, end_kind, end_pos, status, out, reach, crc, isize, next);
    sres: per single item (status, out_len, members, crc0, len0); run_st: per run; crcs: per CRC entry (status, crc)"""
    parts = [("G", len(items), src_cap, out_cap, int(has_off), int(has_counts), seg_min), *items]
    if counts is not None:
        parts += [counts, [0xDEAD0000 if r is None else r[0] << 1 | r[1] for r in raw or []]]
    if recs is not None:
        parts += [*recs, *(sres or [])]
    if run_st is not None:
        parts += [run_st, *(crcs or [])]
    return run(program, lines(*parts))


def test_gz_admit(program):
    # cand_cap = 16 + len / 256, cand_base cumulative; 4096 bytes are one chunk of the scan, 4097 two
    items = [(0, 255, 0, 10), (300, 256, 0, 20), (600, 511, 0, 30), (2000, 4096, 0, 5), (7000, 4097, 0, 6)]
    got = gunzip(program, items)
    assert got["admit"][0] == [0] and got["st"][0] == [0] * 5
    # (item, src, dst, src_len, room, cand_base, cand_cap)
    assert rows(got["items"][0], 7) == [(0, 0, 0, 255, 10, 0, 16), (1, 300, 10, 256, 20, 16, 17), (2, 600, 30, 511, 30, 33, 17), (3, 2000, 60, 4096, 5, 50, 32),
                                        (4, 7000, 65, 4097, 6, 82, 32)]
    assert rows(got["chunks"][0], 2) == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (4, 4096)]
    assert got["cand_total"][0] == [114, 119]
    assert got["out_len"][0] == [0] * 5 and got["members"][0] == [0] * 5 and got["segments"][0] == [0] * 5
    # refused items in front: a chunk's item is the list index; a source of no bytes is status 0, has no entry and still takes its room
    items = [(M64, 1, 0, 100), (0, 10, 0, 7), (5, 0, 0, 1000), (0, 1 << 32, 0, 1), (0, 5000, 0, 9)]
    got = gunzip(program, items, has_counts=False)
    assert got["st"][0] == [E_INVAL, 0, 0, E_UNSUPPORTED, 0]
    assert rows(got["items"][0], 7) == [(1, 0, 100, 10, 7, 0, 16), (4, 0, 1108, 5000, 9, 16, 35)]
    assert rows(got["chunks"][0], 2) == [(0, 0), (1, 0), (1, 4096)]
    assert got["members"][0] == [SENTINEL] * 5 and got["segments"][0] == [SENTINEL] * 5      # (not given: not written)
    # the placement rule is the shared one: a wrapped sum, offsets given, 4 GiB - 1
    got = gunzip(program, [(0, 1, 0, 10), (0, 1, 0, M64 - 4), (0, 1, 0, 20)], out_cap=M64)
    assert got["st"][0] == [0, E_DST_SMALL, E_DST_SMALL]
    G4 = 1 << 32
    got = gunzip(program, [(0, G4 - 1, 8, G4 - 1), (0, 1, 0, G4), (0, 1, 1, 1 << 33)], has_off=True)
    assert got["st"][0] == [0, E_UNSUPPORTED, E_DST_SMALL]
    assert rows(got["items"][0], 7) == [(0, 0, 8, G4 - 1, G4 - 1, 0, 16 + (G4 - 1) // 256)]
    assert len(got["chunks"][0]) == 2 * (G4 // CHUNK)


def test_gz_layout(program):
    got = gunzip(program, [(0, 255, 0, 10), (300, 5000, 0, 20), (0, 0, 0, 1)])
    offs, (kept_max, cand_total, n_items, n_chunks) = got["layout"][0], (53, 51, 2, 3)
    assert got["cand_total"][0] == [cand_total, kept_max] and got["sizes"][0] == list(SIZES.values())
    S = SIZES
    want = [S["item"] * n_items, S["chunk"] * n_chunks, 4 * n_items, 8 * cand_total, S["cand"] * kept_max, 4 * cand_total, S["probe"] * kept_max,
            S["run"] * kept_max, 4 * kept_max, S["inflate_item"] * kept_max, 4 * kept_max, 4 * kept_max, 4 * n_items, S["single"] * n_items]
    at = 0
    for off, size in zip(offs, want):        # in this order, each on a 16-byte line, none overlapping the next
        assert off == at and off % 16 == 0
        at += (size + 15) // 16 * 16
    assert offs[-1] == at


def test_gz_limits(small_limits):
    # 40 raw candidates: two items of 16 fit, a third does not (the chunk limit has a build and a test of its own below)
    assert gunzip(small_limits, [(0, 255, 0, 1)] * 2)["admit"][0] == [0]
    assert gunzip(small_limits, [(0, 255, 0, 1)] * 2 + [(0, 0, 0, 1), (M64, 1, 0, 1)])["admit"][0] == [0]
    assert gunzip(small_limits, [(0, 255, 0, 1)] * 3)["admit"][0] == [E_NOMEM]
    assert gunzip(small_limits, [(0, 256 * 8, 0, 1)])["admit"][0] == [0]            # 24 candidates, 1 chunk
    assert gunzip(small_limits, [(0, 256 * 24, 0, 1)])["admit"][0] == [0]           # 40 candidates
    assert gunzip(small_limits, [(0, 256 * 25, 0, 1)])["admit"][0] == [E_NOMEM]     # 41


def test_gz_chunk_limit(small_chunk_limit):
    # an item counts as len / 4096 + 1 chunks, one more than it has where its length is a multiple of 4096: with the limit at 5,
    # 5 * 4096 - 1 bytes (5 chunks, counted as 5) pass and 5 * 4096 bytes (5 chunks, counted as 6) do not, nor does a byte more
    got = gunzip(small_chunk_limit, [(0, 5 * CHUNK - 1, 0, 1)])
    assert got["admit"][0] == [0] and rows(got["chunks"][0], 2) == [(0, CHUNK * j) for j in range(5)]
    assert gunzip(small_chunk_limit, [(0, 5 * CHUNK, 0, 1)])["admit"][0] == [E_NOMEM]
    assert gunzip(small_chunk_limit, [(0, 5 * CHUNK + 1, 0, 1)])["admit"][0] == [E_NOMEM]
    # the chunks of the items in front count: 2 + 2 and one more item of one chunk is 5; of two chunks, 6
    two = (0, CHUNK + 1, 0, 1)
    assert gunzip(small_chunk_limit, [two, (M64, 1, 0, 1), two, (0, 0, 0, 1), (0, 1, 0, 1)])["admit"][0] == [0]
    assert gunzip(small_chunk_limit, [two, two, two])["admit"][0] == [E_NOMEM]


def cand_rows(got):
    return rows(got["cands"][0], 6)


def test_gz_candidates_single_or_probed(program):
    # four items of 16 candidates each: none found; exactly as many as fit; one more than fit; in between
    items = [(0, 100, 0, 10)] * 4
    full = [(10 + 5 * j, FLUSH) for j in range(16)]
    raw = [None] * 16 + full + [None] * 16 + [(50, FLUSH), (20, MEMBER)]
    got = gunzip(program, items, [0, 16, 17, 2], raw)
    assert got["raw_end"][0] == [50]                       # (the third item's slice is inside it, and is not read: see below)
    assert got["candidates"][0] == [0]
    assert got["single"][0] == [0, 2] and got["probed"][0] == [1, 3] and got["first_cand"][0] == [0, 17, 20]
    assert got["stops"][0] == [p for p, _ in full] + [50]
    c = cand_rows(got)
    assert c[0] == (1, 0, MEMBER, 0, 16, 0)                # byte 0 first, with the item's whole stop range
    assert c[1:17] == [(1, p, FLUSH, j + 1, 16, 0) for j, (p, _) in enumerate(full)]     # stops strictly behind the position
    assert c[17:] == [(3, 0, MEMBER, 16, 17, 0), (3, 20, MEMBER, 16, 17, 0), (3, 50, FLUSH, 17, 17, 0)]
    # the last item overflows: the list is copied back as far as the one before it, and no further
    got = gunzip(program, items[:3], [0, 3, 17], [None] * 16 + [(9, FLUSH), (8, MEMBER), (30, FLUSH)])
    assert got["raw_end"][0] == [19]
    assert got["single"][0] == [0, 2] and got["probed"][0] == [1]
    # ... and nothing at all where no item has candidates that fit
    got = gunzip(program, items[:2], [0, 1000], [])
    assert got["raw_end"][0] == [0] and got["single"][0] == [0, 1] and got["cands"][0] == [] and got["first_cand"][0] == [0]


def test_gz_candidates_seg_min(program):
    raw = [(900, FLUSH), (100, FLUSH), (50, FLUSH), (160, MEMBER), (200, FLUSH), (161, FLUSH), (1000, FLUSH), (950, MEMBER)]
    # every flush candidate closer than seg_min to the one kept before it: the single pass
    got = gunzip(program, [(0, 2000, 0, 10)], [3], [(10, FLUSH), (40, FLUSH), (99, FLUSH)], seg_min=100)
    assert got["single"][0] == [0] and got["probed"][0] == [] and got["cands"][0] == [] and got["stops"][0] == []
    # member candidates are kept whatever seg_min is, flush candidates by their distance; stops are the kept flush positions only
    got = gunzip(program, [(0, 2000, 0, 10)], [len(raw)], raw, seg_min=100)
    assert got["probed"][0] == [0] and got["stops"][0] == [100, 900]
    assert cand_rows(got) == [(0, 0, MEMBER, 0, 2, 0), (0, 100, FLUSH, 1, 2, 0), (0, 160, MEMBER, 1, 2, 0), (0, 900, FLUSH, 2, 2, 0), (0, 950, MEMBER, 2, 2, 0)]
    got = gunzip(program, [(0, 2000, 0, 10)], [len(raw)], raw, seg_min=1 << 40)
    assert got["stops"][0] == [] and cand_rows(got) == [(0, 0, MEMBER, 0, 0, 0), (0, 160, MEMBER, 0, 0, 0), (0, 950, MEMBER, 0, 0, 0)]
    # both kinds at one position: the flush candidate first, and its own position is no stop behind it
    got = gunzip(program, [(0, 2000, 0, 10)], [2], [(8, MEMBER), (8, FLUSH)], seg_min=4)
    assert cand_rows(got) == [(0, 0, MEMBER, 0, 1, 0), (0, 8, FLUSH, 1, 1, 0), (0, 8, MEMBER, 1, 1, 0)]


def raw_candidates(data):
    """every position behind 00 00 FF FF and every 1F 8B 08 behind byte 0 (include/znippy_hip.h), in the order a scan by chunks
    that finish in any order might leave them: here, by a fixed shuffle"""
    raw, at = [], data.find(b"\x00\x00\xff\xff")
    while at >= 0:
        if at + 4 < len(data):
            raw.append((at + 4, FLUSH))
        at = data.find(b"\x00\x00\xff\xff", at + 1)
    at = data.find(b"\x1f\x8b\x08", 1)
    while at >= 0:
        raw.append((at, MEMBER))
        at = data.find(b"\x1f\x8b\x08", at + 1)
    return [raw[(7 * j + 3) % len(raw)] for j in range(len(raw))] if len(raw) % 7 else raw[::-1]


def gzip_member(content, flush, every):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    out = b""
    for at in range(0, len(content), every):
        out += c.compress(content[at:at + every]) + (c.flush(flush) if at + every < len(content) else b"")
    return out + c.flush()


def test_gz_candidates_against_the_model(program):
    text = gen.pseudo_text(60_000, seed=5)
    in_data = b"\x00\x00\xff\xff" * 3 + b"\x1f\x8b\x08 a stored block with both patterns in its data"
    stored = DB.Bits()
    DB.stored_block(stored, in_data)
    files = [gzip_member(text, zlib.Z_FULL_FLUSH, 4000), gzip_member(text, zlib.Z_SYNC_FLUSH, 1500),
             gzip_member(text[:9000], zlib.Z_FULL_FLUSH, 3000) + bytes(5) + gzip_member(text[9000:20_000], zlib.Z_SYNC_FLUSH, 2500) + gzip_member(b"", None, 1),
             gzip_member(text[:3000], None, 1 << 20),
             gzip_member(text[:300], zlib.Z_FULL_FLUSH, 4),                               # more candidates than 16 + len / 256
             DB.gz_member(stored.bytes(), in_data)]
    for seg_min in (1, 256, 2000):
        items, counts, raw, at = [], [], [], 0
        for f in files:
            mine = raw_candidates(f)
            cap = 16 + len(f) // 256
            items.append((at, len(f), 0, 1 << 20))
            counts.append(len(mine))
            raw += mine[:cap] + [None] * (cap - len(mine))        # the scan keeps the first cand_cap it finds
            at += len(f)
        got = gunzip(program, items, counts, None, seg_min=seg_min)
        raw_end = got["raw_end"][0][0]
        got = gunzip(program, items, counts, raw[:raw_end], seg_min=seg_min)
        by_item = {}
        for k, pos, kind, _, _, _ in cand_rows(got):
            by_item.setdefault(k, []).append((pos, kind))
        for k, f in enumerate(files):
            kept, overflow = gz_model.candidates(f, seg_min)
            if overflow or not kept:
                assert k in got["single"][0] and k not in by_item, (k, seg_min)
            else:
                assert k in got["probed"][0] and by_item[k] == [(0, MEMBER)] + kept, (k, seg_min)
        assert sorted(got["single"][0] + got["probed"][0]) == list(range(len(files)))
        assert 4 in got["single"][0] and 0 in got["probed"][0]


def rec(end_kind, data_start=0, end_pos=0, status=0, out=0, reach=0, crc=0, isize=None, next=NEXT_END):
    return (data_start, end_kind, end_pos, status, out, reach, crc, out & 0xFFFFFFFF if isize is None else isize, next)


def test_gz_single_results(program):
    # six items of the single pass, rooms 100 each, packed
    items = [(0, 50, 0, 100)] * 6
    sres = [(0, 100, 2, 111, 60),            # fine: two members, the first of 60 bytes
            (0, 101, 1, 222, 50),            # out_len = room + 1
            (0, 40, 1, 333, 41),             # len0 > out_len
            (E_CHECKSUM, 10, 1, 444, 10),    # the kernel's own verdict
            (0, 0, 1, 0, 0),                 # one empty member
            (0, 100, 1, 555, 100)]
    got = gunzip(program, items, [0] * 6, [], [], sres, [], [(0, 111), (0, 0), (E_CHECKSUM, 999)])
    assert got["plan"][0] == [0]
    assert got["item_st"][0] == [0, E_CORRUPT, E_CORRUPT, E_CHECKSUM, 0, 0]
    # (dst, len, has_crc, want): an entry for each item that decoded, and for no other
    assert rows(got["crc_items"][0], 4) == [(0, 60, 1, 111), (400, 0, 1, 0), (500, 100, 1, 555)]
    assert got["crc_item_of"][0] == [0, 4, 5] and got["runs"][0] == []
    assert got["st"][1] == [0, E_CORRUPT, E_CORRUPT, E_CHECKSUM, 0, E_CHECKSUM]
    assert got["out_len"][1] == [100, 0, 0, 0, 0, 0] and got["members"][1] == [2, 0, 0, 0, 1, 0] and got["segments"][1] == [1, 0, 0, 0, 1, 0]


def three_run_item(content, cuts, base=0):
    """records of one member of three independent runs cut at `cuts`, source positions 100 and 200: -> (raw, recs)"""
    a, b = cuts
    raw = [(base + 100, FLUSH), (base + 200, FLUSH)]
    recs = [rec(BOUNDARY, base + 10, base + 100, out=a), rec(BOUNDARY, base + 100, base + 200, out=b - a),
            rec(TRAILER, base + 200, base + 300, out=len(content) - b, crc=zlib.crc32(content), isize=len(content))]
    return raw, recs


def test_gz_runs_and_verdict(program):
    data = gen.pseudo_text(5000, seed=9)
    A, B = data[:3000], data[3000:]
    crcs_a = [zlib.crc32(A[:1000]), zlib.crc32(A[1000:1700]), zlib.crc32(A[1700:])]
    # item 0: the single pass.  item 1: one member of three runs.  item 2: a member with an empty run in the middle, then the
    # three-run member as its second.  item 3: refused by gz_admit.  item 4: single, and fine.
    items = [(0, 50, 0, 10), (100, 300, 0, 3000), (500, 700, 0, 5000), (M64, 1, 0, 7), (2000, 9, 0, 5)]
    raw1, recs1 = three_run_item(A, (1000, 1700))
    raw2b, recs2b = three_run_item(A, (1000, 1700), base=400)
    raw2 = [(150, FLUSH), (160, FLUSH), (400, MEMBER)] + raw2b
    recs2 = [rec(BOUNDARY, 10, 150, out=1500), rec(BOUNDARY, 150, 160, out=0),
             rec(TRAILER, 160, 400, out=500, crc=zlib.crc32(B), isize=2000, next=NEXT_MEMBER)] + recs2b
    counts = [0, 2, 5, 0]
    raw = [None] * 16 + raw1 + [None] * 15 + raw2
    recs = recs1 + recs2
    sres = [(0, 10, 1, 77, 10), (0, 5, 1, 88, 5)]

    def go(run_st=None, crc_edit=None, sres=sres, first=((0, 77), (0, 88))):
        crcs = list(first) + [(0, c) for c in crcs_a] + [(0, zlib.crc32(B[:1500])), (0, zlib.crc32(B[1500:]))] + [(0, c) for c in crcs_a]
        for at, val in (crc_edit or {}).items():
            crcs[at] = val
        return gunzip(program, items, counts, raw, recs, sres, run_st or [0] * 8, crcs)

    got = go()
    assert got["single"][0] == [0, 3] and got["probed"][0] == [1, 2] and got["first_cand"][0] == [0, 3, 9]
    assert got["plan"][0] == [0] and got["item_st"][0] == [0, 0, 0, 0]
    # (run_item, item, src_start, out_off, out_len): the non-empty runs
    runs = rows(got["runs"][0], 5)
    assert runs == [(1, 1, 10, 0, 1000), (1, 1, 100, 1000, 700), (1, 1, 200, 1700, 1300),
                    (2, 2, 10, 0, 1500), (2, 2, 160, 1500, 500), (2, 2, 410, 2000, 1000), (2, 2, 500, 3000, 700), (2, 2, 600, 3700, 1300)]
    # the CRC list: the single items' first members (with the CRC to compare), then the non-empty runs (without)
    dst = [0, 10, 3010, 8010, 8017]
    assert rows(got["crc_items"][0], 4) == [(dst[0], 10, 1, 77), (dst[4], 5, 1, 88)] + [(dst[k] + off, n, 0, 0) for _, k, _, off, n in runs]
    assert got["crc_item_of"][0] == [0, 3]
    assert got["crc_of_run"][0] == [2, 3, 4, 5, -1, 6, 7, 8, 9]                 # (the empty run has no entry, and those behind it move up)
    want_len, want_mem, want_seg = [10, 3000, 5000, 0, 5], [1, 1, 2, 0, 1], [1, 3, 6, 0, 1]
    assert got["st"][1] == [0, 0, 0, E_INVAL, 0]
    assert (got["out_len"][1], got["members"][1], got["segments"][1]) == (want_len, want_mem, want_seg)

    def only_failed(got, i, status):
        """item i reports the status and nothing else; the arrays of the other items are as in the clean call"""
        assert got["st"][1] == [status if k == i else s for k, s in enumerate([0, 0, 0, E_INVAL, 0])]
        for name, want in (("out_len", want_len), ("members", want_mem), ("segments", want_seg)):
            assert got[name][1] == [0 if k == i else v for k, v in enumerate(want)], name

    # one run's CRC altered: its member's combined CRC differs.  The same for the second member of an item
    only_failed(go(crc_edit={3: (0, crcs_a[1] ^ 1)}), 1, E_CHECKSUM)
    only_failed(go(crc_edit={8: (0, crcs_a[1] ^ 1)}), 2, E_CHECKSUM)
    only_failed(go(crc_edit={5: (0, 5)}), 2, E_CHECKSUM)
    # a run that failed is E_CORRUPT, even where every CRC is right
    only_failed(go(run_st=[0, E_CORRUPT, 0, 0, 0, 0, 0, 0]), 1, E_CORRUPT)
    only_failed(go(run_st=[0, 0, 0, 0, 0, 0, 0, E_DST_SMALL]), 2, E_CORRUPT)
    only_failed(go(run_st=[0, 0, 0, 0, 0, 0, 0, 1], crc_edit={8: (0, 0)}), 2, E_CORRUPT)
    # the first member of a single item: what the CRC launch says counts where the item's status was 0
    only_failed(go(crc_edit={0: (E_CHECKSUM, 1)}), 0, E_CHECKSUM)
    only_failed(go(crc_edit={1: (E_CHECKSUM, 1)}), 4, E_CHECKSUM)
    # ... and the status words of the run entries are not read (the launch compares nothing there)
    got = go(crc_edit={4: (E_CHECKSUM, crcs_a[2])})
    assert got["st"][1] == [0, 0, 0, E_INVAL, 0]
    # a single item that failed by itself has no CRC entry: every entry moves up by one, and item 4's is the first
    got = go(sres=[(E_CORRUPT, 0, 0, 0, 0), sres[1]], first=[(0, 88)])
    assert got["crc_item_of"][0] == [3] and got["crc_of_run"][0] == [1, 2, 3, 4, -1, 5, 6, 7, 8]
    only_failed(got, 0, E_CORRUPT)


def test_gz_contradictory_records(program):
    # a probed item whose records contradict each other: plan_item's E_CORRUPT, no run, no CRC entry; the item beside it is decoded
    items = [(0, 300, 0, 100), (300, 300, 0, 100)]
    raw = [(100, FLUSH)] + [None] * 16 + [(100, FLUSH)]
    recs = [rec(BOUNDARY, 10, 100, out=50), rec(BOUNDARY, 100, 100, out=1),                   # an end that is its own start
            rec(BOUNDARY, 10, 100, out=60), rec(TRAILER, 100, 300, out=40, crc=zlib.crc32(b"x" * 100), isize=100)]
    got = gunzip(program, items, [1, 1], raw, recs, [], [0, 0], [(0, zlib.crc32(b"x" * 60)), (0, zlib.crc32(b"x" * 40))])
    assert got["item_st"][0] == [E_CORRUPT, 0]
    assert rows(got["runs"][0], 5) == [(1, 1, 10, 0, 60), (1, 1, 100, 60, 40)]
    assert rows(got["crc_items"][0], 4) == [(100, 60, 0, 0), (160, 40, 0, 0)]
    assert got["st"][1] == [E_CORRUPT, 0] and got["out_len"][1] == [0, 100] and got["members"][1] == [0, 1] and got["segments"][1] == [0, 2]
    # a count that passes the room
    recs[1] = rec(TRAILER, 100, 300, out=51, isize=101)
    got = gunzip(program, items, [1, 1], raw, recs, [], [0, 0], [(0, zlib.crc32(b"x" * 60)), (0, zlib.crc32(b"x" * 40))])
    assert got["st"][1] == [E_DST_SMALL, 0]
