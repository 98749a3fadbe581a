"""XXH64 in lane-decomposed pieces (znippy_amd/csrc/xxh64_lanes.h) as a stand-alone host program under AddressSanitizer and
UBSan.  The header is plain C++ that the checksum stage of the batch path (zstd_batch.hip, k_bx_xxh_quad / k_bx_xxh_wave) is
built from; the program below emulates both of the stage's lane decompositions in plain loops, lane by lane, and prints the
hash each gives for every input of a file:

  quad  four lanes per frame, lane j walks accumulator j over the stripes in steps of four loads followed by four rounds, for
        MORE trips than the frame has stripes (a wave runs to the longest of its 16 frames; the others are predicated)
  wave  64 lanes load the 16 stripes of a group (512 contiguous bytes, zero behind the last stripe) and premultiply them; every
        lane then walks the chain of accumulator lane & 3 through the premultiplied words of lanes 4 s + (lane & 3) — the last
        group of a frame whose stripe count is no multiple of 16 is walked as far as it has stripes

Each input is copied into a heap buffer of exactly its length before it is hashed, so a read past the end is the sanitizer's to
find.  The values are compared with zstd_synth.xxh64 (the tests' own XXH64, itself checked against libzstd's trailers)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import zstd_synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "znippy_amd", "csrc")

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "xxh64_lanes.h"

// k_bx_xxh_quad: lanes j = 0..3 of one quad; `trips` is the wave's trip count (>= the frame's stripes)
static uint64_t quad_form(const uint8_t *p, uint64_t len, uint32_t trips) {
    const uint32_t stripes = (uint32_t)(len / xxl::STRIPE);
    uint64_t v[4];
    for (uint32_t j = 0; j < 4; j++) {
        uint64_t acc = xxl::acc_init(j);
        const uint8_t *const q = p + 8 * j;
        for (uint32_t i = 0; i < trips; i += 4) {
            uint64_t in[4];
            for (uint32_t k = 0; k < 4; k++) in[k] = i + k < stripes ? xxl::load64(q + (uint64_t)xxl::STRIPE * (i + k)) : 0ull;
            for (uint32_t k = 0; k < 4; k++) acc = i + k < stripes ? xxl::stripe_round(acc, in[k]) : acc;
        }
        v[j] = acc;
    }
    return xxl::finish(v, p, len);  // the quad's first lane
}

// k_bx_xxh_wave: 64 lanes, one frame
static uint64_t wave_form(const uint8_t *p, uint64_t len) {
    const uint64_t stripes = len / xxl::STRIPE, body = stripes * xxl::STRIPE, groups = (stripes + 15) / 16;
    uint64_t acc[64], next[64], pre[64];
    auto word = [&](uint64_t g, uint32_t lane) { const uint64_t o = 512 * g + 8 * lane; return o + 8 <= body ? xxl::load64(p + o) : 0ull; };
    for (uint32_t lane = 0; lane < 64; lane++) { acc[lane] = xxl::acc_init(lane & 3); next[lane] = word(0, lane); }
    for (uint64_t g = 0; g < groups; g++) {
        for (uint32_t lane = 0; lane < 64; lane++) { pre[lane] = xxl::premul(next[lane]); next[lane] = word(g + 1, lane); }
        const uint32_t cnt = (uint32_t)(stripes - 16 * g < 16 ? stripes - 16 * g : 16);
        for (uint32_t s = 0; s < cnt; s++)
            for (uint32_t lane = 0; lane < 64; lane++) acc[lane] = xxl::chain(acc[lane], pre[4 * s + (lane & 3)]);
    }
    for (uint32_t lane = 4; lane < 64; lane++)
        if (acc[lane] != acc[lane & 3]) { printf("lanes disagree\n"); exit(3); }
    const uint64_t v[4] = {acc[0], acc[1], acc[2], acc[3]};
    return xxl::finish(v, p, len);  // lane 0
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < n; c++) {
        uint64_t len = 0;
        if (fread(&len, 8, 1, f) != 1) return 2;
        std::unique_ptr<uint8_t[]> buf(new uint8_t[len]);  // exactly len bytes
        if (len && fread(buf.get(), 1, len, f) != len) return 2;
        const uint32_t stripes = (uint32_t)(len / 32);
        // trip counts of a wave whose longest frame is this one, a little longer, and much longer
        const uint64_t q0 = quad_form(buf.get(), len, stripes), q1 = quad_form(buf.get(), len, stripes + 5), q2 = quad_form(buf.get(), len, stripes + 2048);
        if (q0 != q1 || q0 != q2) { printf("trip counts disagree at %" PRIu64 "\n", len); return 3; }
        printf("%" PRIu64 " %016" PRIx64 " %016" PRIx64 "\n", len, q0, wave_form(buf.get(), len));
    }
    fclose(f);
    return 0;
}
"""

LENGTHS = list(range(0, 601)) + [1023, 1024, 1025, 131072, 300001]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("xxh64_lanes")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "xxh"
    # (gcc links the sanitizers' runtimes dynamically unless told otherwise; linked into the program they do not care what else
    # the process loads)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, str(main), "-o", str(exe)], check=True)
    return str(exe), d


def test_both_lane_forms_against_reference(program):
    exe, d = program
    rng = np.random.default_rng(0x58584836)
    inputs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in LENGTHS]
    path = d / "inputs.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(inputs)))
        for b in inputs:
            f.write(struct.pack("<Q", len(b)))
            f.write(b)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(inputs)
    for b, line in zip(inputs, lines):
        n, quad, wave = line.split()
        want = "%016x" % zstd_synth.xxh64(b)
        assert int(n) == len(b)
        assert quad == want, ("quad form", len(b), quad, want)
        assert wave == want, ("wave form", len(b), wave, want)


def test_header_is_plain_cxx():
    """No HIP in the header: the host compiler above read it without the HIP runtime's headers, and it names none."""
    text = open(os.path.join(CSRC, "xxh64_lanes.h")).read()
    assert "hip/hip_runtime" not in text and "__builtin_amdgcn" not in text and "__shfl" not in text
