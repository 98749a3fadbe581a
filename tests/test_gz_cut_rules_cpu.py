"""The block-start test of the gunzip cut search (znippy_amd/csrc/gz_cut_rules.h) as a stand-alone host program under
AddressSanitizer and UBSan, run over every bit position of real streams and compared with the model (tests/gz_cut_model.py), which
was written from the RFC on its own.  The program copies each stream into a heap block of exactly its length, so a read at or past
the end is caught.  The test must miss no true start of a non-final dynamic block, at any of the eight bit offsets."""
import os
import shutil
import subprocess
import zlib

import pytest

import deflate_build as D
import gen
import gz_cut_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "znippy_amd", "csrc")

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "gz_cut_rules.h"
// argv: files.  Per file one line: "pos:end" of every bit position that passes, then "| q" and the count of positions that pass
// the 13-bit test
int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t *p = (uint8_t *)malloc(n ? n : 1);
        if (n && fread(p, 1, n, f) != (size_t)n) return 2;
        fclose(f);
        uint64_t quick = 0;
        for (uint64_t bit = 0; bit < 8ull * n; bit++) {
            uint64_t end = 0;
            const bool q = gzc::quick13((uint32_t)gzc::peek(p, n, bit) & 0x1FFFu);
            quick += q;
            const bool ok = gzc::block_start(p, n, bit, &end);
            if (ok && !q) return 3;  // (the quick test is part of the whole test)
            if (ok) printf("%" PRIu64 ":%" PRIu64 " ", bit, end);
        }
        printf("| %" PRIu64 "\n", quick);
        free(p);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("gz_cut_rules")
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "rules"
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, str(main), "-o", str(exe)], check=True)
    return str(exe), d


def run(program, streams):
    """-> per stream ([(pos, end)], count of the quick test)"""
    exe, d = program
    paths = []
    for i, s in enumerate(streams):
        p = d / f"s{len(os.listdir(d))}_{i}.bin"
        p.write_bytes(s)
        paths.append(str(p))
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    out = []
    for line in r.stdout.splitlines():
        hits, quick = line.split("|")
        out.append(([tuple(int(x) for x in h.split(":")) for h in hits.split()], int(quick)))
    assert len(out) == len(streams)
    return out


def check(program, streams, valid=True):
    """the program agrees with the model at every bit position and, on valid streams, misses no true start; returns those starts"""
    found = []
    for s, (hits, quick) in zip(streams, run(program, streams)):
        b = M.Bits(s)
        assert quick == len(M.quick_positions(s))
        assert [p for p, _ in hits] == M.passing_positions(s)
        for p, end in hits:
            assert M.dynamic_header(b, p + 3)[2] == end, p
        starts = M.true_starts(s) if valid else []
        assert set(starts) <= {p for p, _ in hits}, "a true block start was missed"
        found += starts
    return found


def test_corpus_streams(program):
    streams = [s for _, s, _, _ in D.corpus()]
    found = check(program, streams)
    assert len(found) > 100 and {p & 7 for p in found} == set(range(8)), "the true starts cover every bit offset"


@pytest.mark.parametrize("level", [1, 6, 9])
def test_zlib_output(program, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    text = gen.pseudo_text(160_000, seed=level)
    s = c.compress(text) + c.flush()
    found = check(program, [s])
    assert len(found) >= 1


def test_short_and_truncated(program):
    # every prefix of a header-heavy stream: the input ends inside the header at most positions, and nothing reads past it
    s = next(s for what, s, _, _ in D.corpus() if M.true_starts(s))
    at = M.true_starts(s)[0] >> 3
    check(program, [s[at:at + n] for n in range(0, 120)] + [b"", b"\x04", bytes(40), b"\xff" * 40], valid=False)
