"""The tar walk and the gzip header rule (znippy_amd/csrc/tar_rules.h behind host/tar_walk.cc) as a stand-alone host program under
AddressSanitizer and UBSan.  Tars written by `tarfile` in its three formats go through znippy_tar_find_member and the answers are
compared with `tarfile`'s reading; hand-built headers cover what `tarfile` does not write; every truncation and every single-byte
mutation of the headers of one small tar must give the answer of the Python restatement of the rules (tests/targz_model.py, itself
pinned to `tarfile` here) — an answer or an error code, never a sanitizer report.  Every buffer the program hands to the walker is a
heap copy of exactly the bytes it names, so a read past one is caught."""
import gzip
import io
import os
import shutil
import subprocess
import tarfile

import pytest

import targz_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "znippy_amd", "csrc", "host")
ERRORS = (M.E_CORRUPT, M.E_UNSUPPORTED, M.E_NOENT)

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tar_walk.h"
// one line per call: "rc data_off size need"
static void find(const uint8_t *p, size_t n, int ended, const char *prefix, const char *suffix) {
    uint8_t *b = (uint8_t *)malloc(n ? n : 1);
    if (n) memcpy(b, p, n);
    uint64_t off = 0, size = 0, need = 0;
    const int rc = znippy_tar_find_member(b, n, ended, prefix, strlen(prefix), suffix, strlen(suffix), &off, &size, &need);
    free(b);
    printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", rc, off, size, need);
}
static void gz(const uint8_t *p, size_t n) {
    uint8_t *b = (uint8_t *)malloc(n ? n : 1);
    if (n) memcpy(b, p, n);
    uint64_t off = 0;
    const int rc = znippy_gzip_header(b, n, &off);
    free(b);
    printf("%d %" PRIu64 " 0 0\n", rc, off);
}
// argv: file prefix suffix mode [from to];  "one": the file, ended and not ended; "trunc": every file[0 .. k), 0 <= k < size, ended and
// not; "mut": every file with byte k, from <= k < to, replaced by each of the 255 other values (ended); "gz", "gztrunc": the gzip header
int main(int argc, char **argv) {
    if (argc < 5) return 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    std::vector<uint8_t> f;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) f.insert(f.end(), buf, buf + n);
    fclose(fp);
    const size_t from = argc > 5 ? strtoull(argv[5], nullptr, 0) : 0, to = argc > 6 ? strtoull(argv[6], nullptr, 0) : f.size();
    const char *mode = argv[4];
    if (!strcmp(mode, "one")) {
        find(f.data(), f.size(), 1, argv[2], argv[3]);
        find(f.data(), f.size(), 0, argv[2], argv[3]);
    } else if (!strcmp(mode, "trunc")) {
        for (size_t k = 0; k < f.size(); k++) {
            find(f.data(), k, 1, argv[2], argv[3]);
            find(f.data(), k, 0, argv[2], argv[3]);
        }
    } else if (!strcmp(mode, "mut")) {
        for (size_t k = from; k < to && k < f.size(); k++)
            for (unsigned x = 1; x < 256; x++) {
                f[k] ^= (uint8_t)x;
                find(f.data(), f.size(), 1, argv[2], argv[3]);
                f[k] ^= (uint8_t)x;
            }
    } else if (!strcmp(mode, "gz")) {
        gz(f.data(), f.size());
    } else if (!strcmp(mode, "gztrunc")) {
        for (size_t k = 0; k <= f.size(); k++) gz(f.data(), k);
    } else return 2;
    // null arguments are refused, not followed
    uint64_t v = 0;
    if (znippy_tar_find_member(nullptr, 512, 1, "", 0, "", 0, &v, &v, &v) != -1 || znippy_tar_find_member(f.data(), 0, 1, "", 0, "", 0, nullptr, &v, &v) != -1 ||
        znippy_tar_find_member(f.data(), 0, 1, nullptr, 1, "", 0, &v, &v, &v) != -1 || znippy_gzip_header(nullptr, 10, &v) != -1 ||
        znippy_gzip_header(f.data(), 0, nullptr) != -1)
        return 4;
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("tar_rules")
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "walk"
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", HOST, str(main), os.path.join(HOST, "tar_walk.cc"), "-o", str(exe)], check=True)
    return str(exe)


def run(program, tmp_path, data, prefix="", suffix="", mode="one", start=0, stop=None):
    p = tmp_path / "input.bin"
    p.write_bytes(data)
    r = subprocess.run([program, str(p), prefix, suffix, mode, str(start), str(len(data) if stop is None else stop)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    return [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


# ---- tars from tarfile ---------------------------------------------------------------------------------------------------
FORMATS = {"ustar": tarfile.USTAR_FORMAT, "gnu": tarfile.GNU_FORMAT, "pax": tarfile.PAX_FORMAT}
LONG = "pkg-1.0/" + "d" * 60 + "/" + "e" * 70 + "/Cargo.toml"              # above 100 bytes: ustar splits it at a slash
LONGER = "pkg-1.0/" + "/".join(["x" * 50] * 6) + "/deep/Cargo.toml"        # above 256 bytes: no ustar
SIZES = (0, 1, 511, 512, 513)


def body(n, salt=0):
    return bytes((i * 7 + salt) & 255 for i in range(n))


def make_tar(fmt, names):
    """members in the order given: (name, bytes) a file, (name, None) a directory, (name, "->target") a symlink"""
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=FORMATS[fmt]) as tf:
        for name, what in names:
            ti = tarfile.TarInfo(name)
            if what is None:
                ti.type = tarfile.DIRTYPE
                tf.addfile(ti)
            elif isinstance(what, str):
                ti.type = tarfile.SYMTYPE
                ti.linkname = what[2:]
                tf.addfile(ti)
            else:
                ti.size = len(what)
                tf.addfile(ti, io.BytesIO(what))
    return b.getvalue()


def standard(fmt, where):
    """a crate-like tar with members of every size around a block; the Cargo.toml first, last, or absent"""
    cargo = [("pkg-1.0/Cargo.toml", b"[package]\nname = \"pkg\"\n" * 9)]
    members = [("pkg-1.0", None), ("pkg-1.0/link", "->src/lib.rs")] + [("pkg-1.0/src/f%d.rs" % n, body(n, n)) for n in SIZES]
    members.append((LONG.replace("Cargo.toml", "notes.txt"), body(700)))
    if fmt != "ustar":
        members.append((LONGER.replace("Cargo.toml", "notes.txt"), body(300, 3)))
    if where == "first":
        members = cargo + members
    elif where == "last":
        members = members + cargo
    return make_tar(fmt, members)


def tarfile_first(data, prefix, suffix):
    with tarfile.open(fileobj=io.BytesIO(data), mode="r:") as tf:
        for ti in tf:
            name = ti.name.encode("utf-8", "surrogateescape")
            if ti.isreg() and not ti.issparse() and name.startswith(prefix.encode()) and name.endswith(suffix.encode()):
                return ti.offset_data, ti.size
    return None


def check_against_tarfile(program, tmp_path, data, prefix, suffix):
    want = tarfile_first(data, prefix, suffix)
    ended, open_ = run(program, tmp_path, data, prefix, suffix)
    model = M.walk(data, True, prefix.encode(), suffix.encode())
    if want is None:
        assert ended[0] == M.E_NOENT and open_[0] == M.E_NOENT and model[0] == M.E_NOENT, (prefix, suffix, ended, open_, model)
    else:
        assert ended[:3] == (0,) + want and open_[:3] == (0,) + want and model[:3] == (0,) + want, (prefix, suffix, want, ended, open_, model)
    return want


@pytest.mark.parametrize("where", ["first", "last", "absent"])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_members_match_tarfile(program, tmp_path, fmt, where):
    data = standard(fmt, where)
    want = check_against_tarfile(program, tmp_path, data, "", "/Cargo.toml")
    assert (want is None) == (where == "absent")
    for n in SIZES:
        off, size = check_against_tarfile(program, tmp_path, data, "", "/f%d.rs" % n)
        assert size == n
    # prefix only, suffix only, both, the whole name as both, no filter (the first REGULAR member: not the directory, not the link)
    for prefix, suffix in [("pkg-1.0/src/", ""), ("", ".rs"), ("pkg-1.0/src/f5", "3.rs"), ("pkg-1.0/src/f1.rs", "pkg-1.0/src/f1.rs"), ("", ""),
                           ("pkg-1.0/" + "d" * 60, "notes.txt"), ("", "/deep/notes.txt")]:
        want = check_against_tarfile(program, tmp_path, data, prefix, suffix)
        assert want is not None or (suffix == "/deep/notes.txt" and fmt == "ustar")
    # a directory and a link are no candidates; a prefix and a suffix that never meet on one name; a filter longer than any name
    for prefix, suffix in [("pkg-1.0", "pkg-1.0"), ("", "/link"), ("pkg-1.0/src/", "notes.txt"), ("", "z" * 400)]:
        assert check_against_tarfile(program, tmp_path, data, prefix, suffix) is None


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_long_names(program, tmp_path, fmt):
    names = [("pkg-1.0/a.txt", b"a"), (LONG, b"long name")] + ([(LONGER, b"longer name")] if fmt != "ustar" else []) + [("pkg-1.0/z.txt", b"zz")]
    data = make_tar(fmt, names)
    # (the first Cargo.toml in stream order is LONG's; the deeper one is reached through its own directory)
    assert check_against_tarfile(program, tmp_path, data, "", "/Cargo.toml") is not None
    assert check_against_tarfile(program, tmp_path, data, "pkg-1.0/" + "d" * 60, "") is not None
    if fmt != "ustar":
        off, size = check_against_tarfile(program, tmp_path, data, "", "/deep/Cargo.toml")
        assert data[off:off + size] == b"longer name"
        assert check_against_tarfile(program, tmp_path, data, "pkg-1.0/" + "x" * 50 + "/", "") is not None
    # the member behind a long name has its own, short name again
    off, size = check_against_tarfile(program, tmp_path, data, "", "z.txt")
    assert data[off:off + size] == b"zz"
    # a non-ASCII name: pax writes it as a path= record, the others as raw bytes
    data = make_tar(fmt, [("pkg-1.0/a.txt", b"a"), ("pkg-1.0/café/Cargo.toml", b"utf-8")])
    off, size = check_against_tarfile(program, tmp_path, data, "pkg-1.0/caf", "/Cargo.toml")
    assert data[off:off + size] == b"utf-8"


def test_an_empty_tar_and_no_tar(program, tmp_path):
    assert check_against_tarfile(program, tmp_path, make_tar("gnu", []), "", "") is None
    ended, open_ = run(program, tmp_path, b"", "", "")
    assert ended[0] == M.E_NOENT and open_ == (M.E_MORE, 0, 0, 512)
    ended, open_ = run(program, tmp_path, b"this is a text file named .crate, and it is longer than a block" * 10, "", "")
    assert ended[0] == M.E_CORRUPT and open_[0] == M.E_CORRUPT
    # one zero block and then the end; one zero block and then a member (the walk goes on, as tar -i does)
    ended, open_ = run(program, tmp_path, bytes(512), "", "")
    assert ended[0] == M.E_NOENT and open_ == (M.E_MORE, 0, 0, 1024)
    t = make_tar("gnu", [("a", b"A")])
    ended, open_ = run(program, tmp_path, bytes(512) + t, "", "")
    assert ended == open_ == (0, 1024, 1, 0)


# ---- hand-built headers ----------------------------------------------------------------------------------------------------
def header(name, size_field, typeflag, prefix=b"", signed=False, magic=b"ustar\x0000"):
    h = bytearray(512)
    h[0:len(name)] = name
    h[100:108] = b"0000644\0"
    h[108:116] = h[116:124] = b"0000000\0"
    h[124:136] = size_field
    h[136:148] = b"00000000000\0"
    h[148:156] = b"        "
    h[156:157] = typeflag
    h[257:265] = magic
    h[345:345 + len(prefix)] = prefix
    s = sum(c - 256 if c > 127 else c for c in h) if signed else sum(h)
    h[148:156] = b"%06o\0 " % s
    return bytes(h)


def octal(n):
    return b"%011o\0" % n


def base256(n):
    return b"\x80" + n.to_bytes(11, "big")


def test_types_that_carry_no_data_whatever_their_size_says(program, tmp_path):
    for typeflag in b"123456":
        t = header(b"pkg/thing", octal(1000), bytes([typeflag])) + header(b"pkg/Cargo.toml", octal(3), b"0") + b"abc" + bytes(509) + bytes(1024)
        assert tarfile_first(t, "", "Cargo.toml") == (1024, 3)
        assert check_against_tarfile(program, tmp_path, t, "", "Cargo.toml") == (1024, 3)
    # an unknown type is followed by its data; a V7 directory ('\0' with a trailing slash) is not
    t = header(b"pkg/thing", octal(1000), b"Z") + bytes(1024) + header(b"pkg/Cargo.toml", octal(3), b"0") + b"abc" + bytes(509) + bytes(1024)
    assert check_against_tarfile(program, tmp_path, t, "", "Cargo.toml") == (2048, 3)
    t = header(b"pkg/dir/", octal(1000), b"\0") + header(b"pkg/Cargo.toml", octal(3), b"\0") + b"abc" + bytes(509) + bytes(1024)
    assert check_against_tarfile(program, tmp_path, t, "", "Cargo.toml") == (1024, 3)
    assert check_against_tarfile(program, tmp_path, t, "pkg/dir", "") is None
    # a contiguous file ('7') is a candidate
    t = header(b"pkg/Cargo.toml", octal(3), b"7") + b"abc" + bytes(509) + bytes(1024)
    assert check_against_tarfile(program, tmp_path, t, "", "Cargo.toml") == (512, 3)


def test_prefix_field_base256_and_signed_checksum(program, tmp_path):
    # the prefix is joined whenever it is there and the type is no GNU type — with the GNU magic too
    for magic in (b"ustar\x0000", b"ustar  \0"):
        t = header(b"Cargo.toml", octal(2), b"0", prefix=b"pkg-9/sub", magic=magic) + b"hi" + bytes(510) + bytes(1024)
        assert check_against_tarfile(program, tmp_path, t, "pkg-9/sub/", "") == (512, 2)
        assert check_against_tarfile(program, tmp_path, t, "Cargo", "") is None
    # a base-256 size; high bytes in the name with the signed sum
    t = header(b"pkg/Cargo.toml", base256(700), b"0") + body(700) + bytes(324) + bytes(1024)
    assert check_against_tarfile(program, tmp_path, t, "", "Cargo.toml") == (512, 700)
    t = header(b"pkg/\xff\xfe\xc3\xa9/Cargo.toml", octal(2), b"0", signed=True) + b"hi" + bytes(510) + bytes(1024)
    assert sum(t[:148] + b"        " + t[156:512]) != int(t[148:154], 8)
    assert check_against_tarfile(program, tmp_path, t, "", "Cargo.toml") == (512, 2)
    # blanks around an octal field, as old tars write it
    t = header(b"pkg/Cargo.toml", b"        2 \0\0", b"0") + b"hi" + bytes(510) + bytes(1024)
    assert check_against_tarfile(program, tmp_path, t, "", "Cargo.toml") == (512, 2)
    # no number: corrupt.  A negative base-256 size: corrupt
    for field in (b"12x45678901\0", b"\xff" * 12):
        t = header(b"pkg/Cargo.toml", field, b"0") + bytes(1024)
        assert run(program, tmp_path, t, "", "Cargo.toml")[0][0] == M.E_CORRUPT
        assert M.walk(t, True, b"", b"Cargo.toml")[0] == M.E_CORRUPT


def test_a_size_of_two_to_the_33(program, tmp_path):
    big = 1 << 33
    # the wanted member itself: found, and its bytes are not there.  Another member: the walk steps 2^33 bytes ahead
    t = header(b"pkg/Cargo.toml", base256(big), b"0") + bytes(2048)
    ended, open_ = run(program, tmp_path, t, "", "Cargo.toml")
    assert ended[0] == M.E_CORRUPT and open_ == (M.E_MORE, 0, 0, 512 + big)
    assert M.walk(t, False, b"", b"Cargo.toml") == open_
    t = header(b"pkg/big.bin", base256(big), b"0") + bytes(2048)
    ended, open_ = run(program, tmp_path, t, "", "Cargo.toml")
    assert ended[0] == M.E_CORRUPT and open_ == (M.E_MORE, 0, 0, 512 + big + 512)
    assert M.walk(t, False, b"", b"Cargo.toml") == open_
    # sizes whose sums would wrap are refused
    for field in (base256(1 << 62), base256((1 << 88) - 1)):
        t = header(b"pkg/big.bin", field, b"0") + bytes(2048)
        assert run(program, tmp_path, t, "", "Cargo.toml")[0][0] == M.E_CORRUPT


def test_long_name_entries_by_hand(program, tmp_path):
    def entry(typeflag, payload):
        return header(b"././@LongLink", octal(len(payload)), typeflag) + payload + bytes(-len(payload) % 512)

    member = header(b"short", octal(2), b"0") + b"hi" + bytes(510)
    end = bytes(1024)
    # 'K' (a long link name) is stepped over and names nothing; 'g' likewise, even with a path= record
    t = entry(b"K", b"pkg/Cargo.toml\0") + member + end
    assert check_against_tarfile(program, tmp_path, t, "", "Cargo.toml") is None
    assert check_against_tarfile(program, tmp_path, t, "short", "") == (1536, 2)
    t = entry(b"g", pax(b"comment", b"Cargo.toml")) + member + end
    assert check_against_tarfile(program, tmp_path, t, "short", "") == (1536, 2)
    # (a path= in a global header, which tarfile would give to every later member, is stepped over with the rest of it)
    t = entry(b"g", pax(b"path", b"glob/Cargo.toml")) + member + end
    assert run(program, tmp_path, t, "short", "")[0][:3] == (0, 1536, 2) == M.walk(t, True, b"short")[:3]
    # of two names in front of one member the first wins, as in tarfile; a pax size= record replaces the size field
    t = entry(b"L", b"first/Cargo.toml\0") + entry(b"x", pax(b"path", b"second/Cargo.toml")) + member + end
    assert check_against_tarfile(program, tmp_path, t, "first/", "Cargo.toml") == (2560, 2)
    t = entry(b"x", pax(b"path", b"one/Cargo.toml") + pax(b"path", b"two/Cargo.toml") + pax(b"size", b"1")) + member + end
    assert check_against_tarfile(program, tmp_path, t, "two/", "Cargo.toml") == (1536, 1)
    # payloads above 8 KiB, sparse members: unsupported.  A long name with nothing behind it: corrupt
    for t in (entry(b"L", b"n" * 8193), entry(b"x", pax(b"path", b"n" * 8200)), header(b"sparse", octal(0), b"S"),
              entry(b"x", pax(b"GNU.sparse.major", b"1")) + member):
        assert run(program, tmp_path, t + member + end, "", "")[0][0] == M.E_UNSUPPORTED
        assert M.walk(t + member + end, True)[0] == M.E_UNSUPPORTED
    for t in (entry(b"L", b"name\0") + end, entry(b"L", b"name\0"), entry(b"x", b"12 path=a\n") + member + end, entry(b"x", b"9 path\n") + member + end):
        assert run(program, tmp_path, t, "", "")[0][0] == M.E_CORRUPT
        assert M.walk(t, True)[0] == M.E_CORRUPT


def pax(key, value):
    n = len(key) + len(value) + 3
    d = len(str(n + len(str(n))))
    while len(str(n + d)) != d:
        d += 1
    return b"%d %s=%s\n" % (n + d, key, value)


# ---- damage ------------------------------------------------------------------------------------------------------------------
def small():
    """a long-named first member, the wanted one second: three headers and a name payload in front of the answer's bytes"""
    return make_tar("gnu", [("pkg-1.0/" + "v" * 120 + "/info.json", b"{}"), ("pkg-1.0/Cargo.toml", b"[package]\n" * 7), ("pkg-1.0/src/lib.rs", body(600))])


def test_every_truncation(program, tmp_path):
    data = small()
    want = tarfile_first(data, "", "/Cargo.toml")
    results = run(program, tmp_path, data, "", "/Cargo.toml", "trunc")
    assert len(results) == 2 * len(data)
    for k in range(len(data)):
        ended, open_ = results[2 * k], results[2 * k + 1]
        assert ended[:3] == M.walk(data[:k], True, b"", b"/Cargo.toml")[:3], (k, ended)
        assert open_[:3] == M.walk(data[:k], False, b"", b"/Cargo.toml")[:3], (k, open_)
        if k >= want[0] + want[1]:
            assert ended == open_ == (0,) + want + (0,), (k, ended, open_)
        else:
            # (the end of the first member's block is a header boundary with nothing pending)
            assert ended[0] == (M.E_NOENT if k in (0, 2048) else M.E_CORRUPT) and open_[0] == M.E_MORE and k < open_[3] <= want[0] + want[1], (k, ended, open_)


def test_every_single_byte_mutation_of_the_headers(program, tmp_path):
    data = small()
    want = tarfile_first(data, "", "/Cargo.toml")
    assert want == (2560, 70)  # in front: the 'L' header, its payload, the first member's header and block, the wanted member's header
    same = errors = 0
    for first in (0, 1024, 2048):  # the three headers
        results = run(program, tmp_path, data, "", "/Cargo.toml", "mut", first, first + 512)
        assert len(results) == 255 * 512
        it = iter(results)
        for k in range(first, first + 512):
            mut = bytearray(data)
            for x in range(1, 256):
                res = next(it)
                mut[k] = data[k] ^ x
                assert res[:3] == M.walk(bytes(mut), True, b"", b"/Cargo.toml")[:3], (k, x, res)
                if res[0] != 0:
                    assert res[0] in ERRORS, (k, x, res)
                    errors += 1
                    continue
                # a clean answer describes the tar as it now is: where tarfile still reads the mutant, its view
                try:
                    tf_view = tarfile_first(bytes(mut), "", "/Cargo.toml")
                except Exception:
                    tf_view = None
                if tf_view is not None:
                    assert res[1:3] == tf_view, (k, x, res, tf_view)
                same += res[1:3] == want
    assert same and errors


# ---- gzip headers ------------------------------------------------------------------------------------------------------------
def gz_header(extra=None, name=None, comment=None, hcrc=False, flags=0):
    flg = flags | (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\x02\xff"
    if extra is not None:
        h += len(extra).to_bytes(2, "little") + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += b"\x12\x34"
    return h


def test_gzip_headers(program, tmp_path):
    deflate = b"\x03\x00" + b"trailer."
    cases = [gz_header(), gz_header(extra=b""), gz_header(extra=b"ab\x02\x00xy"), gz_header(name=b"pkg-1.0.crate"), gz_header(comment=b"made by hand"),
             gz_header(hcrc=True), gz_header(extra=b"\0" * 300, name=b"n", comment=b"", hcrc=True), gz_header(name=b"")]
    for h in cases:
        (res,) = run(program, tmp_path, h + deflate, mode="gz")
        assert res[:2] == (0, len(h)) == M.gzip_header(h + deflate), (h, res)
        assert gzip.decompress(h + deflate[:2] + bytes(8)) == b""  # (Python reads the same header)
        # every truncation: short of the header's end it is "more", from there on the answer
        results = run(program, tmp_path, h + deflate, mode="gztrunc")
        assert len(results) == len(h) + len(deflate) + 1
        for k, res in enumerate(results):
            assert res[:2] == ((M.E_MORE, 0) if k < len(h) else (0, len(h))) == M.gzip_header((h + deflate)[:k]), (h, k, res)
    # what Python's gzip writes, with a file name
    b = io.BytesIO()
    with gzip.GzipFile("pkg-1.0.crate", "wb", fileobj=b, mtime=0) as g:
        g.write(b"x")
    (res,) = run(program, tmp_path, b.getvalue(), mode="gz")
    assert res[:2] == (0, 10 + len("pkg-1.0.crate") + 1)
    # not gzip; another method; reserved flag bits — judged as soon as the byte is there
    for bad, code in [(b"PK\x03\x04" + bytes(20), M.E_CORRUPT), (b"\x1f\x8c\x08" + bytes(20), M.E_CORRUPT), (b"\x1f\x8b\x07" + bytes(20), M.E_UNSUPPORTED),
                      (gz_header(flags=0x20) + deflate, M.E_UNSUPPORTED), (gz_header(flags=0x80) + deflate, M.E_UNSUPPORTED), (b"\x1f\x8b\x09", M.E_UNSUPPORTED),
                      (b"\x1e", M.E_CORRUPT)]:
        (res,) = run(program, tmp_path, bad, mode="gz")
        assert res[0] == code == M.gzip_header(bad)[0], (bad, res)
    assert run(program, tmp_path, b"", mode="gz")[0][0] == M.E_MORE
