"""The ZIP directory locator (znippy_amd/csrc/host/zip_dir.cc) as a stand-alone host program under AddressSanitizer and UBSan:
containers made by `zipfile` go through the three functions and the answers are compared with `ZipInfo`; every truncation and every
single-byte mutation of one small container's directory and end record must give the same answer or an error code, never a sanitizer
report.  Every buffer the program hands to the locator is a heap copy of exactly the bytes it names, so a read past one is caught."""
import io
import os
import shutil
import struct
import subprocess
import zipfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "znippy_amd", "csrc", "host")
OK, E_INVAL, E_CORRUPT, E_UNSUPPORTED, E_NOENT = 0, -1, -5, -6, -9
ERRORS = (E_CORRUPT, E_UNSUPPORTED, E_NOENT)

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "zip_dir.h"
// one line per container: "rc_end dir_off dir_size n  rc_find lho csize usize crc method flags name_len dir_pos  rc_local data_off"
static void locate(const std::vector<uint8_t> &f, const char *prefix, const char *suffix) {
    const size_t tl = f.size() < ZN_ZIP_TAIL_MAX ? f.size() : ZN_ZIP_TAIL_MAX;
    uint8_t *tail = (uint8_t *)malloc(tl ? tl : 1);
    if (tl) memcpy(tail, f.data() + (f.size() - tl), tl);
    uint64_t off = 0, size = 0, n = 0, data_off = 0;
    znippy_zip_entry e;
    memset(&e, 0, sizeof e);
    int r1 = znippy_zip_end_of_directory(tail, tl, f.size(), &off, &size, &n), r2 = 1, r3 = 1;
    free(tail);
    if (r1 == 0) {
        if (off > f.size() || size > f.size() - off) { printf("directory outside the file\n"); exit(3); }
        uint8_t *dir = (uint8_t *)malloc(size ? size : 1);
        if (size) memcpy(dir, f.data() + off, size);
        r2 = znippy_zip_find_entry(dir, size, n, prefix, strlen(prefix), suffix, strlen(suffix), &e);
        free(dir);
    }
    if (r2 == 0) {
        const size_t have = e.local_header_offset < f.size() ? f.size() - e.local_header_offset : 0, hl = have < 30 ? have : 30;
        uint8_t *h = (uint8_t *)malloc(hl ? hl : 1);
        if (hl) memcpy(h, f.data() + e.local_header_offset, hl);
        r3 = znippy_zip_local_data_offset(h, hl, &data_off);
        free(h);
    }
    printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u %u %u %d %" PRIu64 "\n", r1, off, size, n, r2,
           e.local_header_offset, e.compressed_size, e.uncompressed_size, e.crc32, e.method, e.flags, e.name_len, e.dir_pos, r3, data_off);
}
// argv: file prefix suffix mode [from];  mode "one": the file as it is; "trunc": every file[0 .. k), from <= k < size;
// "mut": every file with byte k, from <= k < size, replaced by each of the 255 other values
int main(int argc, char **argv) {
    if (argc < 5) return 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    std::vector<uint8_t> f;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) f.insert(f.end(), buf, buf + n);
    fclose(fp);
    const size_t from = argc > 5 ? strtoull(argv[5], nullptr, 0) : 0;
    if (!strcmp(argv[4], "one")) locate(f, argv[2], argv[3]);
    else if (!strcmp(argv[4], "trunc")) {
        for (size_t k = from; k < f.size(); k++) locate(std::vector<uint8_t>(f.begin(), f.begin() + k), argv[2], argv[3]);
    } else if (!strcmp(argv[4], "mut")) {
        for (size_t k = from; k < f.size(); k++)
            for (unsigned x = 1; x < 256; x++) {
                f[k] ^= (uint8_t)x;
                locate(f, argv[2], argv[3]);
                f[k] ^= (uint8_t)x;
            }
    } else return 2;
    // null arguments are refused, not followed
    uint64_t v = 0;
    znippy_zip_entry e;
    if (znippy_zip_end_of_directory(nullptr, 0, 0, &v, &v, &v) != -1 || znippy_zip_find_entry(nullptr, 4, 1, "", 0, "", 0, &e) != -1 ||
        znippy_zip_find_entry(nullptr, 0, 0, "", 0, "", 0, nullptr) != -1 || znippy_zip_local_data_offset(nullptr, 30, &v) != -1)
        return 4;
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("zip_dir")
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "locate"
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", HOST, str(main), os.path.join(HOST, "zip_dir.cc"), "-o", str(exe)], check=True)
    return str(exe)


class Result:
    def __init__(self, line):
        v = [int(x) for x in line.split()]
        assert len(v) == 15, line
        (self.rc_end, self.dir_off, self.dir_size, self.n, self.rc_find, self.lho, self.csize, self.usize, self.crc, self.method, self.flags,
         self.name_len, self.dir_pos, self.rc_local, self.data_off) = v

    @property
    def rc(self):
        """the first code of the chain that is not 0 (a step behind a failed one is not made and prints 1)"""
        for c in (self.rc_end, self.rc_find, self.rc_local):
            if c != 0:
                return c
        return 0


def locate(program, tmp_path, data, prefix="", suffix="", mode="one", start=0):
    p = tmp_path / "container.zip"
    p.write_bytes(data)
    r = subprocess.run([program, str(p), prefix, suffix, mode, str(start)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    return [Result(x) for x in r.stdout.splitlines()]


def first_match(zf, prefix, suffix):
    for zi in zf.infolist():
        name = zi.orig_filename.encode("utf-8" if zi.flag_bits & 0x800 else "cp437")
        if name.startswith(prefix.encode()) and name.endswith(suffix.encode()):
            return zi
    return None


def local_lens(data, zi):
    """name and extra length as the LOCAL header has them"""
    return struct.unpack_from("<HH", data, zi.header_offset + 26)


def local_extra_len(data, zi):
    return local_lens(data, zi)[1]


def agrees(res, data, zi):
    """the comparison: offsets, sizes, CRC and method are ZipInfo's, the data offset is header + 30 + name + LOCAL extra"""
    return (res.rc == 0 and res.lho == zi.header_offset and res.csize == zi.compress_size and res.usize == zi.file_size and res.crc == zi.CRC and
            res.method == zi.compress_type and res.flags == zi.flag_bits and
            res.data_off == 30 + sum(local_lens(data, zi)))


POM = b"<project><modelVersion>4.0.0</modelVersion>" + b"<dependency>x</dependency>" * 40 + b"</project>"


def jar(comment=b"", stream=False, pom=True, extra_local=False):
    class Unseekable(io.RawIOBase):   # zipfile then writes data descriptors (flag bit 3) and zeros in the local header
        def __init__(self):
            self.b = bytearray()

        def writable(self):
            return True

        def write(self, d):
            self.b += d
            return len(d)

    sink = Unseekable() if stream else io.BytesIO()
    with zipfile.ZipFile(sink, "w") as zf:
        zf.writestr(zipfile.ZipInfo("META-INF/MANIFEST.MF"), b"Manifest-Version: 1.0\n", zipfile.ZIP_STORED)
        zf.writestr(zipfile.ZipInfo("g/a/Main.class"), bytes(range(256)) * 9, zipfile.ZIP_DEFLATED)
        if pom:
            zi = zipfile.ZipInfo("META-INF/maven/g/a/pom.xml")
            if extra_local:
                zi.extra = struct.pack("<HH", 0xCAFE, 12) + b"local-extra!"
            zf.writestr(zi, POM, zipfile.ZIP_DEFLATED)
            zf.writestr(zipfile.ZipInfo("META-INF/maven/g/a/pom.properties"), b"version=1\n", zipfile.ZIP_STORED)
        zf.comment = comment
    return bytes(sink.b) if stream else sink.getvalue()


@pytest.mark.parametrize("comment", [b"", b"c", b"k" * 65535], ids=["comment0", "comment1", "comment65535"])
@pytest.mark.parametrize("stream", [False, True])
def test_entries_match_zipinfo(program, tmp_path, comment, stream):
    data = jar(comment, stream)
    zf = zipfile.ZipFile(io.BytesIO(data))
    for prefix, suffix in [("", "pom.xml"), ("META-INF/maven/", "pom.xml"), ("g/", ".class"), ("", ""), ("META-INF/MANIFEST.MF", ""),
                           ("META-INF/maven/g/a/pom.xml", "META-INF/maven/g/a/pom.xml"), ("", ".properties")]:
        zi = first_match(zf, prefix, suffix)
        assert zi is not None
        (res,) = locate(program, tmp_path, data, prefix, suffix)
        assert agrees(res, data, zi), (prefix, suffix, vars(res))
        assert res.data_off == 30 + len(zi.filename) + len(zi.extra)
        assert (res.dir_off, res.n) == (zf.start_dir, len(zf.infolist()))
        assert data[res.lho + res.data_off:res.lho + res.data_off + res.csize] == (
            zf.read(zi) if zi.compress_type == 0 else data[res.lho + res.data_off:res.lho + res.data_off + zi.compress_size])
        if stream:
            assert res.flags & 8
    # a prefix and a suffix that are each present but never on one name; a name shorter than either
    for prefix, suffix in [("g/", "pom.xml"), ("", "nothing-ends-like-this"), ("META-INF/maven/g/a/pom.xml.longer", "")]:
        (res,) = locate(program, tmp_path, data, prefix, suffix)
        assert (res.rc_end, res.rc_find) == (0, E_NOENT)


def test_an_empty_archive_and_a_jar_without_the_entry(program, tmp_path):
    b = io.BytesIO()
    zipfile.ZipFile(b, "w").close()
    (res,) = locate(program, tmp_path, b.getvalue(), "", "pom.xml")
    assert (res.rc_end, res.n, res.dir_size, res.rc_find) == (0, 0, 0, E_NOENT)
    (res,) = locate(program, tmp_path, jar(pom=False), "", "pom.xml")
    assert (res.rc_end, res.rc_find) == (0, E_NOENT)
    (res,) = locate(program, tmp_path, b"this is a text file named .jar, long enough to hold an end record\n" * 3, "", "pom.xml")
    assert res.rc_end == E_CORRUPT
    (res,) = locate(program, tmp_path, b"", "", "pom.xml")
    assert res.rc_end == E_CORRUPT


def test_local_extra_field_that_differs_from_the_central_one(program, tmp_path):
    data = bytearray(jar(extra_local=True))
    zf = zipfile.ZipFile(io.BytesIO(bytes(data)))
    zi = first_match(zf, "", "pom.xml")
    # zipfile writes one extra field to both places: take the central copy out, so that only the local header has it
    at = data.index(b"PK\x01\x02" + b"", zf.start_dir)
    while data[at + 46:at + 46 + len(zi.filename)] != zi.filename.encode():
        at = data.index(b"PK\x01\x02", at + 4)
    n, m, k = struct.unpack_from("<HHH", data, at + 28)
    assert m == 16
    del data[at + 46 + n:at + 46 + n + m]
    struct.pack_into("<H", data, at + 30, 0)
    end = data.rindex(b"PK\x05\x06")
    struct.pack_into("<I", data, end + 12, struct.unpack_from("<I", data, end + 12)[0] - m)
    data = bytes(data)
    zf = zipfile.ZipFile(io.BytesIO(data))
    zi = first_match(zf, "", "pom.xml")
    assert zi.extra == b"" and local_extra_len(data, zi) == 16 and zf.read(zi) == POM
    (res,) = locate(program, tmp_path, data, "", "pom.xml")
    assert agrees(res, data, zi) and res.data_off == 30 + len(zi.filename) + 16
    import zlib
    assert zlib.decompressobj(-15).decompress(data[res.lho + res.data_off:res.lho + res.data_off + res.csize]) == POM


def test_zip64_and_encryption_are_refused(program, tmp_path):
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w") as zf:
        with zf.open(zipfile.ZipInfo("META-INF/maven/g/a/pom.xml"), "w", force_zip64=True) as w:
            w.write(POM)
    data = b.getvalue()
    (res,) = locate(program, tmp_path, data, "", "pom.xml")
    # zipfile gives such an entry a zip64 extra field in its local header; whether it also writes the 0xFFFFFFFF markers there depends
    # on the Python version.  With markers the entry is refused; without them it is an ordinary entry whose local extra field differs
    # from the (empty) central one
    zi = zipfile.ZipFile(io.BytesIO(data)).infolist()[0]
    if b"\xff\xff\xff\xff" in data[18:26]:
        assert res.rc == E_UNSUPPORTED, vars(res)
    else:
        assert agrees(res, data, zi) and res.data_off == 30 + len(zi.filename) + 20 and zi.extra == b"", vars(res)
    # zip64 markers in the central record and in the end record; a zip64 locator in front of the end record
    data = bytearray(jar())
    zf = zipfile.ZipFile(io.BytesIO(bytes(data)))
    end = data.rindex(b"PK\x05\x06")
    pom_at = data.index(b"PK\x01\x02", zf.start_dir)
    while not data[pom_at + 46:].startswith(b"META-INF/maven/g/a/pom.xml"):
        pom_at = data.index(b"PK\x01\x02", pom_at + 4)
    for at, size in [(pom_at + 20, 4), (pom_at + 24, 4), (pom_at + 42, 4), (pom_at + 34, 2), (end + 10, 2), (end + 8, 2), (end + 12, 4), (end + 16, 4)]:
        d = bytearray(data)
        d[at:at + size] = b"\xff" * size
        (res,) = locate(program, tmp_path, bytes(d), "", "pom.xml")
        assert res.rc == E_UNSUPPORTED, (at - end, at - pom_at, vars(res))
    d = bytes(data[:end]) + b"PK\x06\x07" + bytes(16) + bytes(data[end:])
    (res,) = locate(program, tmp_path, d, "", "pom.xml")
    assert res.rc_end == E_UNSUPPORTED
    # several disks
    d = bytearray(data)
    struct.pack_into("<H", d, end + 4, 1)
    assert locate(program, tmp_path, bytes(d), "", "pom.xml")[0].rc_end == E_UNSUPPORTED
    # the encryption bit, hand-set: in the central record (the scan refuses), in the local header alone (the header call refuses);
    # set on another entry it does not matter
    d = bytearray(data)
    d[pom_at + 8] |= 1
    assert locate(program, tmp_path, bytes(d), "", "pom.xml")[0].rc_find == E_UNSUPPORTED
    assert locate(program, tmp_path, bytes(d), "", ".class")[0].rc == 0
    d = bytearray(data)
    d[first_match(zf, "", "pom.xml").header_offset + 6] |= 1
    res = locate(program, tmp_path, bytes(d), "", "pom.xml")[0]
    assert (res.rc_find, res.rc_local) == (0, E_UNSUPPORTED)


def small():
    b = io.BytesIO()
    with zipfile.ZipFile(b, "w") as zf:
        zf.writestr(zipfile.ZipInfo("a.class"), b"\xca\xfe\xba\xbe" * 8, zipfile.ZIP_STORED)
        zf.writestr(zipfile.ZipInfo("META-INF/pom.xml"), POM, zipfile.ZIP_DEFLATED)
        zf.comment = b"hi"
    return b.getvalue()


def raw_view(data, res):
    """what the bytes of a (mutated) container say at the places the result names, read independently"""
    at = res.dir_off + res.dir_pos
    sig, _, _, flags, method, _, _, crc, csize, usize, n, m, k, disk, _, _, lho = struct.unpack_from("<IHHHHHHIIIHHHHHII", data, at)
    ln, lm = struct.unpack_from("<HH", data, lho + 26)
    return (sig == 0x02014B50 and data[lho:lho + 4] == b"PK\x03\x04" and
            (res.lho, res.csize, res.usize, res.crc, res.method, res.flags, res.name_len, res.data_off) == (lho, csize, usize, crc, method, flags, n, 30 + ln + lm))


def test_every_truncation_of_tail_and_directory(program, tmp_path):
    data = small()
    zf = zipfile.ZipFile(io.BytesIO(data))
    results = locate(program, tmp_path, data, "", "pom.xml", "trunc", zf.start_dir)
    assert len(results) == len(data) - zf.start_dir
    for k, res in zip(range(zf.start_dir, len(data)), results):
        # no proper prefix holds an end record whose comment ends with the file
        assert res.rc in ERRORS, (k, vars(res))


def test_every_single_byte_mutation_of_tail_and_directory(program, tmp_path):
    data = small()
    zf = zipfile.ZipFile(io.BytesIO(data))
    zi0 = first_match(zf, "", "pom.xml")
    (res,) = locate(program, tmp_path, data, "", "pom.xml")
    assert agrees(res, data, zi0)
    results = locate(program, tmp_path, data, "", "pom.xml", "mut", zf.start_dir)
    assert len(results) == 255 * (len(data) - zf.start_dir)
    clean = same = 0
    it = iter(results)
    for k in range(zf.start_dir, len(data)):
        for x in range(1, 256):
            res = next(it)
            if res.rc != 0:
                assert res.rc in ERRORS, (k, x, vars(res))
                continue
            clean += 1
            mut = bytearray(data)
            mut[k] ^= x
            mut = bytes(mut)
            # a clean answer describes the container as it now is: ZipInfo's view of it where zipfile still reads the mutant and finds the
            # same entry, the bytes at the places the answer names otherwise (zipfile refuses more than the locator looks at: versions,
            # name encodings, an entry count it re-derives)
            try:
                zi = first_match(zipfile.ZipFile(io.BytesIO(mut)), "", "pom.xml")
            except Exception:
                zi = None
            if zi is not None and zi.header_offset == res.lho and zi.header_offset + 30 <= len(mut):
                assert agrees(res, mut, zi), (k, x, vars(res))
                same += 1
            else:
                assert raw_view(mut, res), (k, x, vars(res))
    assert clean and same
