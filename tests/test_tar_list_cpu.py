"""The tar listing (znippy_amd/csrc/tar_list_rules.h behind host/tar_list.cc) and the host planning of znippy_tar_list_batch
(host/tar_list_plan.cc) as a stand-alone host program under AddressSanitizer and UBSan.  Tars written by `tarfile` in its three
formats go through znippy_tar_list_members and the answers are compared with `tarfile`'s reading; hand-built headers cover what
`tarfile` does not write; every truncation of one small tar and a sample of mutations of its headers must give the answer of the
Python listing (tests/tar_list_model.py, itself pinned to `tarfile` here); the plan is fed forged device answers.  Every buffer the
program hands to the code under test is a heap copy of exactly the bytes it names, so a read past one is caught: an answer or a
status, never a sanitizer report."""
import functools
import io
import os
import shutil
import subprocess
import tarfile

import pytest

import tar_list_model as M
from test_tar_rules_cpu import FORMATS, LONG, LONGER, base256, body, header, make_tar, octal, pax, small, standard  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "znippy_amd", "csrc", "host")

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tar_list.h"
#include "tar_list_plan.h"
using namespace zn;

static std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> f;
    FILE *fp = fopen(path, "rb");
    if (!fp) exit(2);
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) f.insert(f.end(), buf, buf + n);
    fclose(fp);
    return f;
}
struct Listing { int rc; uint64_t n, nb, ob; std::vector<znippy_tar_member> m; std::vector<char> names; };
// measure, then list with exact caps: heap copies of exactly the bytes named, and lists of exactly the sizes measured
static Listing list(const uint8_t *p, size_t n, const char *prefix, const char *suffix) {
    uint8_t *b = (uint8_t *)malloc(n ? n : 1);
    if (n) memcpy(b, p, n);
    Listing l{};
    l.rc = znippy_tar_list_members(b, n, prefix, strlen(prefix), suffix, strlen(suffix), nullptr, 0, nullptr, 0, &l.n, &l.nb, &l.ob);
    if (l.rc == 0) {
        znippy_tar_member *m = (znippy_tar_member *)malloc(l.n ? l.n * sizeof *m : 1);
        char *names = (char *)malloc(l.nb ? l.nb : 1);
        uint64_t n2 = 0, nb2 = 0, ob2 = 0;
        const int rc2 = znippy_tar_list_members(b, n, prefix, strlen(prefix), suffix, strlen(suffix), m, l.n, names, l.nb, &n2, &nb2, &ob2);
        if (rc2 != 0 || n2 != l.n || nb2 != l.nb || ob2 != l.ob) exit(5);
        // one entry, one byte short: DST_SMALL with the same counts
        if (l.n && (znippy_tar_list_members(b, n, prefix, strlen(prefix), suffix, strlen(suffix), m, l.n - 1, names, l.nb, &n2, &nb2, &ob2) != -4 || n2 != l.n)) exit(6);
        if (l.nb && (znippy_tar_list_members(b, n, prefix, strlen(prefix), suffix, strlen(suffix), m, l.n, names, l.nb - 1, &n2, &nb2, &ob2) != -4 || nb2 != l.nb)) exit(6);
        l.m.assign(m, m + l.n);
        l.names.assign(names, names + l.nb);
        free(m); free(names);
    } else if (l.n || l.nb || l.ob) exit(7);
    free(b);
    return l;
}
static void show(const Listing &l, bool members) {
    printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", l.rc, l.n, l.nb, l.ob);
    if (!members) return;
    for (const znippy_tar_member &m : l.m) {
        printf("m %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u ", m.header_off, m.data_off, m.size, m.out_off, m.typeflag);
        for (uint32_t i = 0; i < m.name_len; i++) printf("%02x", (unsigned char)l.names[m.name_off + i]);
        printf("\n");
    }
}

// ---- the plan, fed forged device answers ----
struct Plan {
    std::vector<uint8_t> tar;
    uint8_t *heap;
    uint64_t off[3], len[3], first[4], nb, ob;
    std::vector<znippy_tar_member> members;
    std::vector<char> names;
    TlCall c;
    TlBatch b;
    std::vector<znippy_tar_member> recs;   // the honest staging lists
    std::vector<char> rnames;
    explicit Plan(const std::vector<uint8_t> &t, uint64_t members_cap = 64, uint64_t names_cap = 4096) : tar(t) {
        heap = (uint8_t *)malloc(3 * tar.size());
        for (int i = 0; i < 3; i++) { memcpy(heap + i * tar.size(), tar.data(), tar.size()); off[i] = i * tar.size(); len[i] = tar.size(); }
        members.resize(members_cap ? members_cap : 1);
        names.resize(names_cap ? names_cap : 1);
        c = TlCall{heap, 3 * tar.size(), off, len, 3, members.data(), members_cap, names.data(), names_cap, nullptr, 0, first, &nb, &ob};
        if (tl_admit(c, b) != TL_OK || b.items.size() != 3) exit(8);
        // what an honest device reports
        for (size_t k = 0; k < 3; k++) {
            const Listing l = list(tar.data(), tar.size(), "", "");
            b.totals[k] = TlTotal{TL_KEY_NONE, l.n, l.nb, l.ob};
        }
    }
    ~Plan() { free(heap); }
    void honest_records() {
        recs.clear(); rnames.clear();
        for (size_t k = 0; k < 3; k++) {
            if (!b.bases[k].take) continue;
            const Listing l = list(tar.data(), tar.size(), "", "");
            for (znippy_tar_member m : l.m) { m.name_off += b.bases[k].names; m.out_off += b.bases[k].out; recs.push_back(m); }
            rnames.insert(rnames.end(), l.names.begin(), l.names.end());
        }
    }
    void accept_and_show(const char *what) {
        // exact heap copies of the staging lists
        znippy_tar_member *r = (znippy_tar_member *)malloc(recs.size() ? recs.size() * sizeof *r : 1);
        if (!recs.empty()) memcpy(r, recs.data(), recs.size() * sizeof *r);
        char *nm = (char *)malloc(rnames.size() ? rnames.size() : 1);
        if (!rnames.empty()) memcpy(nm, rnames.data(), rnames.size());
        tl_accept(c, b, r, recs.size(), nm, rnames.size());
        free(r); free(nm);
        printf("%s %d %d %d | %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " | %" PRIu64 " %" PRIu64 "\n", what, b.st[0], b.st[1], b.st[2], first[0], first[1],
               first[2], first[3], nb, ob);
    }
};

static void plan_cases(const std::vector<uint8_t> &tar) {
    {   // admission
        uint8_t *heap = (uint8_t *)malloc(4096);
        const uint64_t off[6] = {0, 4000, ~0ull - 7, 16, 0, 512}, len[6] = {1024, 97, 16, 1ull << 32, 0, 1000};
        uint64_t first[7], nb, ob;
        TlCall c{heap, 4096, off, len, 6, nullptr, 0, nullptr, 0, nullptr, 0, first, &nb, &ob};
        TlBatch b;
        const int rc = tl_admit(c, b);
        printf("admit %d:", rc);
        for (int s : b.st) printf(" %d", s);
        printf(" | items %zu chunks %zu nodes %" PRIu64 " max %u\n", b.items.size(), b.chunks.size(), b.n_nodes, b.max_nodes);
        c.tar_cap = 1ull << 40;  // the 4 GiB item lies inside now, and is refused for its size
        TlBatch b2;
        const int rc2 = tl_admit(c, b2);
        printf("admit2 %d: %d\n", rc2, b2.st[3]);
        const TlLayout at = tl_layout(b, 5);
        printf("layout %d\n", at.bytes > at.bases && at.bases > at.totals && at.nodes > at.filter && at.bytes % 16 == 0);
        size_t m, n, p;
        printf("staging %d %zu %zu %zu\n", tl_staging(c, b, &m, &n, &p), m, n, p);
        free(heap);
    }
    printf("rounds %u %u %u %u %u %u %u\n", tl_rounds(1), tl_rounds(2), tl_rounds(3), tl_rounds(4), tl_rounds(5), tl_rounds(4097), tl_rounds(0xFFFFFFFFu));
    { Plan p(tar); tl_place(p.c, p.b); p.honest_records(); p.accept_and_show("honest"); show(Listing{0, p.first[3], p.nb, p.ob, p.members, p.names}, false); }
    {   // the honest records are what the listing says, item after item
        Plan p(tar); tl_place(p.c, p.b); p.honest_records(); p.accept_and_show("again");
        const Listing l = list(tar.data(), tar.size(), "", "");
        bool same = p.first[3] == 3 * l.n;
        for (uint64_t j = 0; same && j < p.first[3]; j++) {
            const znippy_tar_member &a = p.members[j], &e = l.m[j % l.n];
            same = a.header_off == e.header_off && a.size == e.size && a.name_len == e.name_len && a.name_off == e.name_off + (j / l.n) * l.nb &&
                   !memcmp(p.names.data() + a.name_off, l.names.data() + e.name_off, a.name_len);
        }
        printf("same %d\n", same);
    }
    // keys
    { Plan p(tar); p.b.totals[1].key = 3ull << 8 | TL_KEY_UNSUP; tl_place(p.c, p.b); p.honest_records(); p.accept_and_show("key_unsup"); }
    { Plan p(tar); p.b.totals[1].key = 3ull << 8 | TL_KEY_CORRUPT; tl_place(p.c, p.b); p.honest_records(); p.accept_and_show("key_corrupt"); }
    { Plan p(tar); p.b.totals[1].key = 0x1234567890ull; tl_place(p.c, p.b); p.honest_records(); p.accept_and_show("key_garbage"); }
    { Plan p(tar); p.b.totals[1].key = (1ull << 40) | TL_KEY_UNSUP; tl_place(p.c, p.b); p.honest_records(); p.accept_and_show("key_far_node"); }
    // totals that an item of this size cannot have
    { Plan p(tar); p.b.totals[1].cnt = p.b.items[1].blocks + 1; tl_place(p.c, p.b); p.honest_records(); p.accept_and_show("more_than_blocks"); }
    { Plan p(tar); p.b.totals[1].names = p.b.items[1].len + 1; tl_place(p.c, p.b); p.honest_records(); p.accept_and_show("names_beyond"); }
    { Plan p(tar); p.b.totals[1].out = ~0ull; tl_place(p.c, p.b); p.honest_records(); p.accept_and_show("out_beyond"); }
    { Plan p(tar); p.b.totals[1].cnt = ~0ull; tl_place(p.c, p.b); p.honest_records(); p.accept_and_show("cnt_huge"); }
    // caps: the middle item one short
    { const Listing l = list(tar.data(), tar.size(), "", ""); Plan p(tar, 2 * l.n - 1, 4096); tl_place(p.c, p.b); p.honest_records(); p.accept_and_show("members_short"); }
    { const Listing l = list(tar.data(), tar.size(), "", ""); Plan p(tar, 64, 2 * l.nb - 1); tl_place(p.c, p.b); p.honest_records(); p.accept_and_show("names_short"); }
    // records that contradict their item (item 1's start at recs[n])
    const uint64_t n = list(tar.data(), tar.size(), "", "").n;
#define FORGE(what, code) { Plan p(tar); tl_place(p.c, p.b); p.honest_records(); znippy_tar_member *r = p.recs.data() + n; (void)r; code; p.accept_and_show(what); }
    FORGE("size_outside", r[1].size = p.tar.size())
    FORGE("size_wraps", r[1].size = ~0ull - 100)
    FORGE("header_outside", r[2].header_off = p.tar.size(); r[2].data_off = p.tar.size() + 512)
    FORGE("header_far", r[2].header_off = ~0ull - 511; r[2].data_off = 0)
    FORGE("header_odd", r[0].header_off += 1; r[0].data_off += 1)
    FORGE("data_elsewhere", r[0].data_off += 512)
    FORGE("out_of_order", std::swap(r[0], r[1]))
    FORGE("twice", r[1] = r[0])
    FORGE("name_elsewhere", r[1].name_off += 1)
    FORGE("name_long", r[1].name_len += 1)
    FORGE("name_huge", r[1].name_len = 0xFFFFFFFFu)
    FORGE("out_elsewhere", r[1].out_off += 1)
    FORGE("typeflag", r[1].typeflag = '5')
    FORGE("short_list", p.recs.resize(2 * n))
    FORGE("short_names", p.rnames.resize(p.rnames.size() - 1))
    FORGE("first_item", p.recs[0].size += 1)
    FORGE("last_item", p.recs[2 * n].header_off = 512 * 1000)
}

// argv: file prefix suffix mode [mutants];  "list": the file; "trunc": every file[0 .. k), 0 <= k <= size; "mut": the file with byte
// off ^= x for every (off: 4 bytes, x: 1 byte) of the mutants file; "plan": the plan cases over the file
int main(int argc, char **argv) {
    if (argc < 5) return 2;
    std::vector<uint8_t> f = read_file(argv[1]);
    const char *mode = argv[4];
    if (!strcmp(mode, "list")) show(list(f.data(), f.size(), argv[2], argv[3]), true);
    else if (!strcmp(mode, "trunc")) { for (size_t k = 0; k <= f.size(); k++) show(list(f.data(), k, argv[2], argv[3]), false); }
    else if (!strcmp(mode, "mut") && argc > 5) {
        const std::vector<uint8_t> mu = read_file(argv[5]);
        for (size_t i = 0; i + 5 <= mu.size(); i += 5) {
            uint32_t off;
            memcpy(&off, mu.data() + i, 4);
            if (off >= f.size()) return 2;
            f[off] ^= mu[i + 4];
            show(list(f.data(), f.size(), argv[2], argv[3]), false);
            f[off] ^= mu[i + 4];
        }
    } else if (!strcmp(mode, "plan")) plan_cases(f);
    else return 2;
    // null arguments are refused, not followed
    uint64_t v = 0;
    znippy_tar_member m;
    char c;
    if (znippy_tar_list_members(nullptr, 512, "", 0, "", 0, nullptr, 0, nullptr, 0, &v, &v, &v) != -1 ||
        znippy_tar_list_members(f.data(), 0, "", 0, "", 0, nullptr, 0, nullptr, 0, nullptr, &v, &v) != -1 ||
        znippy_tar_list_members(f.data(), 0, nullptr, 1, "", 0, nullptr, 0, nullptr, 0, &v, &v, &v) != -1 ||
        znippy_tar_list_members(f.data(), 0, "", 0, "", 0, nullptr, 1, &c, 1, &v, &v, &v) != -1 ||
        znippy_tar_list_members(f.data(), 0, "", 0, "", 0, &m, 1, nullptr, 1, &v, &v, &v) != -1)
        return 4;
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("tar_list")
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "list"
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", HOST, str(main)] + [os.path.join(HOST, f) for f in ("tar_list.cc", "tar_list_plan.cc", "range_plan.cc")] + ["-o", str(exe)], check=True)
    return str(exe)


def run(program, tmp_path, data, prefix=b"", suffix=b"", mode="list", mutants=None):
    p = tmp_path / "input.bin"
    p.write_bytes(data)
    args = [program, str(p), prefix, suffix, mode]
    if mutants is not None:
        q = tmp_path / "mutants.bin"
        q.write_bytes(mutants)
        args.append(str(q))
    r = subprocess.run(args, capture_output=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    return r.stdout.decode().splitlines()


def parse(lines):
    """[(rc, [(header_off, data_off, size, name, typeflag)], names_bytes, out_bytes)] of the program's "list" lines"""
    out = []
    for line in lines:
        f = line.split()
        if f[0] == "m":
            out[-1][1].append((int(f[1]), int(f[2]), int(f[3]), bytes.fromhex(f[6]) if len(f) > 6 else b"", int(f[5])))
            assert int(f[4]) == sum(m[2] for m in out[-1][1][:-1])  # out_off counts the sizes up
        else:
            out.append((int(f[0]), [], int(f[2]), int(f[3])))
            assert int(f[1]) == 0 or int(f[0]) == 0
    return out


def listed(program, tmp_path, data, prefix=b"", suffix=b""):
    """the program's listing, checked against the model: (status, members)"""
    (got,) = parse(run(program, tmp_path, data, prefix, suffix))
    want = M.listing(data, prefix, suffix)
    assert (got[0], got[1]) == want, (prefix, suffix, got, want)
    assert got[2] == sum(len(m[3]) for m in got[1]) and got[3] == sum(m[2] for m in got[1])
    return got[0], got[1]


def tarfile_members(data, prefix=b"", suffix=b""):
    out = []
    with tarfile.open(fileobj=io.BytesIO(data), mode="r:") as tf:
        for ti in tf:
            name = ti.name.encode("utf-8", "surrogateescape")
            if ti.isreg() and not ti.issparse() and name.startswith(prefix) and name.endswith(suffix):
                out.append((ti.offset, ti.offset_data, ti.size, name))
    return out


def check_against_tarfile(program, tmp_path, data, prefix=b"", suffix=b""):
    st, members = listed(program, tmp_path, data, prefix, suffix)
    want = tarfile_members(data, prefix, suffix)
    assert st == 0
    # (tarfile's offset is that of the first extended header in front of a member; ours is the member's own header)
    assert [(m[1], m[2], m[3]) for m in members] == [(w[1], w[2], w[3]) for w in want], (members, want)
    for m in members:
        assert m[1] == m[0] + 512 and m[4] in (0, ord("0"), ord("7"))
    return members


# ---- tars from tarfile ---------------------------------------------------------------------------------------------------
def nested(fmt):
    inner = standard(fmt, "first")
    return make_tar(fmt, [("outer/a.txt", b"a"), ("outer/inner.tar", inner), ("outer/z.txt", b"zz")])


def many(n, fmt="gnu"):
    return make_tar(fmt, [("m/%d" % i, bytes([i & 255]) * (i % 3)) for i in range(n)])


@functools.lru_cache(maxsize=None)
def valid_tars():
    """the valid tars of the CPU and GPU tests, by name"""
    tars = {}
    for fmt in FORMATS:
        for where in ("first", "last", "absent"):
            tars["standard-%s-%s" % (fmt, where)] = standard(fmt, where)
        names = [("pkg-1.0/a.txt", b"a"), (LONG, b"long name")] + ([(LONGER, b"longer name")] if fmt != "ustar" else []) + [("pkg-1.0/z.txt", b"zz")]
        tars["long-" + fmt] = make_tar(fmt, names)
        tars["utf8-" + fmt] = make_tar(fmt, [("pkg-1.0/a.txt", b"a"), ("pkg-1.0/café/Cargo.toml", b"utf-8"), ("pkg-1.0/naïve.rs", body(513))])
        tars["nested-" + fmt] = nested(fmt)
    tars["empty"] = make_tar("gnu", [])
    tars["many"] = many(3000)
    return tars


@pytest.mark.parametrize("name", sorted(valid_tars()))
def test_members_match_tarfile(program, tmp_path, name):
    data = valid_tars()[name]
    members = check_against_tarfile(program, tmp_path, data)
    if name.startswith("nested"):
        assert [m[3] for m in members] == [b"outer/a.txt", b"outer/inner.tar", b"outer/z.txt"]  # the inner tar's members are off the chain
    if name == "many":
        assert len(members) == 3000
    if name.startswith("standard"):
        for prefix, suffix in [(b"pkg-1.0/src/", b""), (b"", b".rs"), (b"pkg-1.0/src/f5", b"3.rs"), (b"", b"/Cargo.toml"), (b"pkg-1.0/" + b"d" * 60, b"notes.txt"),
                               (b"pkg-1.0", b"pkg-1.0"), (b"", b"z" * 400)]:
            check_against_tarfile(program, tmp_path, data, prefix, suffix)
        assert len(check_against_tarfile(program, tmp_path, data, b"", b".rs")) == 5


def test_no_tar_and_single_zero_blocks(program, tmp_path):
    assert listed(program, tmp_path, b"") == (0, [])
    assert listed(program, tmp_path, b"this is a text file named .crate, and it is longer than a block" * 10)[0] == M.E_CORRUPT
    assert listed(program, tmp_path, bytes(512)) == (0, [])
    assert listed(program, tmp_path, bytes(511))[0] == M.E_CORRUPT
    t = make_tar("gnu", [("a", b"A")])
    st, members = listed(program, tmp_path, bytes(512) + t)  # one zero block is stepped over, as tar -i does
    assert st == 0 and [m[:4] for m in members] == [(512, 1024, 1, b"a")]
    member = header(b"a", octal(1), b"0") + b"A" + bytes(511)
    # headers behind the two zero blocks are not reached; a member's bytes of eight zero blocks are not the end
    st, members = listed(program, tmp_path, member + bytes(1024) + member)
    assert st == 0 and len(members) == 1
    t = header(b"zeros", octal(4096), b"0") + bytes(4096) + member + bytes(1024)
    st, members = listed(program, tmp_path, t)
    assert st == 0 and [m[:4] for m in members] == [(0, 512, 4096, b"zeros"), (4608, 5120, 1, b"a")]
    # a member whose bytes are a valid header with a size far beyond the tar
    t = header(b"trap", octal(512), b"0") + header(b"far", octal(1 << 30), b"0") + member + bytes(1024)
    st, members = listed(program, tmp_path, t)
    assert st == 0 and [m[3] for m in members] == [b"trap", b"a"]
    # the end of the bytes at a header boundary is a clean end; inside a member or its padding it is not
    assert listed(program, tmp_path, member)[0] == 0 and listed(program, tmp_path, member[:513])[0] == M.E_CORRUPT
    assert listed(program, tmp_path, member[:1023])[0] == M.E_CORRUPT


# ---- hand-built headers ----------------------------------------------------------------------------------------------------
def entry(typeflag, payload):
    return header(b"././@LongLink", octal(len(payload)), typeflag) + payload + bytes(-len(payload) % 512)


MEMBER = header(b"short", octal(2), b"0") + b"hi" + bytes(510)
END = bytes(1024)


def test_types_by_hand(program, tmp_path):
    cargo = header(b"pkg/Cargo.toml", octal(3), b"0") + b"abc" + bytes(509)
    for typeflag in b"123456":  # no data follows, whatever the size says; and they are not listed
        t = header(b"pkg/thing", octal(1000), bytes([typeflag])) + cargo + END
        assert [m[:4] for m in check_against_tarfile(program, tmp_path, t)] == [(512, 1024, 3, b"pkg/Cargo.toml")]
    t = header(b"pkg/thing", octal(1000), b"Z") + bytes(1024) + cargo + END  # an unknown type is followed by its data
    assert [m[:4] for m in check_against_tarfile(program, tmp_path, t)] == [(1536, 2048, 3, b"pkg/Cargo.toml")]
    t = header(b"pkg/dir/", octal(1000), b"\0") + header(b"pkg/Cargo.toml", octal(3), b"\0") + b"abc" + bytes(509) + END  # a V7 directory
    assert [m[:5] for m in check_against_tarfile(program, tmp_path, t)] == [(512, 1024, 3, b"pkg/Cargo.toml", 0)]
    t = header(b"pkg/Cargo.toml", octal(3), b"7") + b"abc" + bytes(509) + END
    assert [m[:5] for m in check_against_tarfile(program, tmp_path, t)] == [(0, 512, 3, b"pkg/Cargo.toml", ord("7"))]
    # the prefix field, a base-256 size, the signed checksum
    t = header(b"Cargo.toml", octal(2), b"0", prefix=b"pkg-9/sub") + b"hi" + bytes(510) + END
    assert [m[3] for m in check_against_tarfile(program, tmp_path, t)] == [b"pkg-9/sub/Cargo.toml"]
    t = header(b"pkg/Cargo.toml", base256(700), b"0") + body(700) + bytes(324) + END
    assert [m[:3] for m in check_against_tarfile(program, tmp_path, t)] == [(0, 512, 700)]
    t = header(b"pkg/\xff\xfe\xc3\xa9/Cargo.toml", octal(2), b"0", signed=True) + b"hi" + bytes(510) + END
    assert sum(t[:148] + b"        " + t[156:512]) != int(t[148:154], 8)
    assert len(check_against_tarfile(program, tmp_path, t)) == 1
    for field in (b"12x45678901\0", b"\xff" * 12, base256(1 << 62)):  # no number
        assert listed(program, tmp_path, header(b"pkg/Cargo.toml", field, b"0") + END)[0] == M.E_CORRUPT
    # a member that crosses the end of the tar
    assert listed(program, tmp_path, header(b"big", base256(1 << 33), b"0") + bytes(2048))[0] == M.E_CORRUPT


def test_extended_headers_by_hand(program, tmp_path):
    # 'K' and 'g' are stepped over and name nothing
    t = entry(b"K", b"pkg/Cargo.toml\0") + MEMBER + END
    assert [m[:4] for m in check_against_tarfile(program, tmp_path, t)] == [(1024, 1536, 2, b"short")]
    t = entry(b"g", pax(b"comment", b"Cargo.toml")) + MEMBER + END
    assert [m[3] for m in check_against_tarfile(program, tmp_path, t)] == [b"short"]
    # 'L' then 'x': the first wins; the last path= of one payload counts; 'K' between a name and its member changes nothing
    t = entry(b"L", b"first/Cargo.toml\0") + entry(b"x", pax(b"path", b"second/Cargo.toml")) + MEMBER + MEMBER + END
    assert [m[:4] for m in check_against_tarfile(program, tmp_path, t)] == [(2048, 2560, 2, b"first/Cargo.toml"), (3072, 3584, 2, b"short")]
    t = entry(b"x", pax(b"path", b"one") + pax(b"path", b"two")) + entry(b"K", b"link\0") + MEMBER + END
    assert [m[3] for m in check_against_tarfile(program, tmp_path, t)] == [b"two"]
    # a name for a member that is not listed is used up by it
    t = entry(b"L", b"a/long/dir\0") + header(b"d", octal(0), b"5") + MEMBER + END
    assert [m[3] for m in check_against_tarfile(program, tmp_path, t)] == [b"short"]
    # size= equal to the size field is accepted; one that differs is unsupported (the deviation), for listed and unlisted members
    t = entry(b"x", pax(b"path", b"p/Cargo.toml") + pax(b"size", b"2")) + MEMBER + END
    assert [m[:4] for m in check_against_tarfile(program, tmp_path, t)] == [(1024, 1536, 2, b"p/Cargo.toml")]
    for size in (b"1", b"3", b"513", b"8589934592"):
        assert listed(program, tmp_path, entry(b"x", pax(b"size", size)) + MEMBER + END)[0] == M.E_UNSUPPORTED
    assert listed(program, tmp_path, entry(b"x", pax(b"size", b"1")) + header(b"d", octal(0), b"5") + MEMBER + END)[0] == M.E_UNSUPPORTED
    # payloads above 8 KiB, sparse members
    for t in (entry(b"L", b"n" * 8193), entry(b"x", pax(b"path", b"n" * 8200)), header(b"sparse", octal(0), b"S"), entry(b"x", pax(b"GNU.sparse.major", b"1"))):
        assert listed(program, tmp_path, t + MEMBER + END)[0] == M.E_UNSUPPORTED
    st, members = listed(program, tmp_path, entry(b"L", b"n" * 8192) + MEMBER + END)
    assert st == 0 and members[0][3] == b"n" * 8192
    # a run of extended headers: 64 in front of a member are looked back over, the 65th is unsupported whatever follows
    skip = entry(b"g", pax(b"comment", b"c"))
    st, members = listed(program, tmp_path, entry(b"L", b"the/first/name\0") + skip * 63 + MEMBER + MEMBER + END)
    assert st == 0 and [m[3] for m in members] == [b"the/first/name", b"short"]
    assert listed(program, tmp_path, skip * 64 + MEMBER + skip * 64 + MEMBER + bytes(512) + skip * 64 + END)[0] == 0
    for t in (skip * 65 + MEMBER + END, entry(b"L", b"n\0") + skip * 64 + MEMBER + END, MEMBER + skip * 65, skip * 64 + entry(b"K", b"k\0") + b"junk" * 128):
        assert listed(program, tmp_path, t)[0] == M.E_UNSUPPORTED
    # a name with nothing behind it; bad pax records; a payload that crosses the end
    for t in (entry(b"L", b"name\0") + END, entry(b"L", b"name\0"), entry(b"L", b"name\0") + bytes(512) + MEMBER + END, entry(b"x", b"12 path=a\n") + MEMBER + END,
              entry(b"x", b"9 path\n") + MEMBER + END, entry(b"x", pax(b"size", b"")) + MEMBER + END, header(b"././@LongLink", octal(600), b"L") + b"n" * 512):
        assert listed(program, tmp_path, t)[0] == M.E_CORRUPT


# ---- damage ------------------------------------------------------------------------------------------------------------------
def mutation_sample(data):
    """(off, x) — byte off ^= x — over the three headers of small(): x in {1, 0x80, 0xFF} at every byte, every x in the size, checksum
    and typeflag fields"""
    sample = []
    for first in (0, 1024, 2048):
        for k in range(512):
            full = 124 <= k < 136 or 148 <= k < 157
            sample += [(first + k, x) for x in (range(1, 256) if full else (1, 0x80, 0xFF))]
    return sample


def test_every_truncation(program, tmp_path):
    data = small()
    lines = run(program, tmp_path, data, mode="trunc")
    assert len(lines) == len(data) + 1
    clean = []
    for k, line in enumerate(lines):
        rc, n = (int(x) for x in line.split()[:2])
        st, members = M.listing(data[:k])
        assert (rc, n) == (st, len(members)), (k, line)
        assert rc in (0, M.E_CORRUPT)
        if rc == 0:
            clean.append(k)
    assert clean == [0, 2048, 3072, 4608, 5120] + list(range(5632, len(data) + 1))


def test_a_mutation_sample_of_the_headers(program, tmp_path):
    data = small()
    sample = mutation_sample(data)
    assert len(sample) == 20484
    lines = run(program, tmp_path, data, mode="mut", mutants=b"".join(off.to_bytes(4, "little") + bytes([x]) for off, x in sample))
    assert len(lines) == len(sample)
    counts = {}
    mut = bytearray(data)
    for (off, x), line in zip(sample, lines):
        rc, n = (int(v) for v in line.split()[:2])
        mut[off] = data[off] ^ x
        st, members = M.listing(bytes(mut))
        mut[off] = data[off]
        assert (rc, n) == (st, len(members)), (off, x, line)
        counts[(rc, n)] = counts.get((rc, n), 0) + 1
    print(counts)
    assert counts.get((M.E_CORRUPT, 0)) and counts.get((0, 3))


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def test_plan_cases(program, tmp_path):
    data = small()
    n, nb, ob = 3, sum(len(m[3]) for m in M.listing(data)[1]), 2 + 70 + 600
    lines = run(program, tmp_path, data, mode="plan")
    got = {line.split()[0]: line.split(None, 1)[1] for line in lines if not line[0].isdigit() and not line.startswith("-")}
    # outside tar_cap, an offset that wraps, (outside), nothing, inside: 1024 bytes are 3 nodes, 1000 bytes are 2
    assert got["admit"] == "0: 0 -1 -1 -1 0 0 | items 2 chunks 2 nodes 5 max 3"
    assert got["admit2"] == "0: -6"
    assert got["layout"] == "1" and got["staging"] == "0 0 0 0"
    assert got["rounds"] == "0 1 2 2 3 13 32"
    whole = "0 0 0 | 0 %d %d %d | %d %d" % (n, 2 * n, 3 * n, 3 * nb, 3 * ob)
    assert got["honest"] == whole and got["again"] == whole and got["same"] == "1"

    def middle(code):  # the middle item has the status and takes no room
        return "0 %d 0 | 0 %d %d %d | %d %d" % (code, n, n, 2 * n, 2 * nb, 2 * ob)

    assert got["key_unsup"] == middle(M.E_UNSUPPORTED) and got["key_corrupt"] == middle(M.E_CORRUPT)
    assert got["key_garbage"] == middle(M.E_CORRUPT) and got["key_far_node"] == middle(M.E_CORRUPT)
    for case in ("more_than_blocks", "names_beyond", "out_beyond", "cnt_huge"):
        assert got[case] == middle(M.E_CORRUPT), case
    # (the three items are alike: what is one short for the second is short for the third as well)
    assert got["members_short"] == got["names_short"] == "0 -4 -4 | 0 %d %d %d | %d %d" % (n, n, n, nb, ob)
    for case in ("size_outside", "size_wraps", "header_outside", "header_far", "header_odd", "data_elsewhere", "out_of_order", "twice", "name_elsewhere",
                 "name_long", "name_huge", "out_elsewhere", "typeflag"):
        assert got[case] == middle(M.E_CORRUPT), (case, got[case])
    # a staging list that is too short fails the items that reach beyond it
    assert got["short_list"] == "0 0 -5 | 0 %d %d %d | %d %d" % (n, 2 * n, 2 * n, 2 * nb, 2 * ob)
    assert got["short_names"] == got["short_list"]
    assert got["first_item"] == "-5 0 0 | 0 0 %d %d | %d %d" % (n, 2 * n, 2 * nb, 2 * ob)
    assert got["last_item"] == "0 0 -5 | 0 %d %d %d | %d %d" % (n, 2 * n, 2 * n, 2 * nb, 2 * ob)
