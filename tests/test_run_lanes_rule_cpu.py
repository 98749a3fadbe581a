"""The overlap rule of the run lanes (znippy_amd/csrc/host/run_overlap.cc: may a lean run be queued beside the run in front of
it?) as a stand-alone host program under AddressSanitizer and UBSan: a table of run pairs goes through the rule and the answers
are compared with what the rule's statement (include/znippy_hip.h, znippy_decode_verify_rows: Run lanes) gives for each."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "znippy_amd", "csrc", "host")

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "run_overlap.h"
// stdin, one case per line: "R a a_len b b_len" (regions) or "P" + 2 x (table slot lane verify d_blobs blob_base blob_cap d_out out_cap)
static zn_run_desc desc(char **&p) {
    uint64_t v[9];
    for (int i = 0; i < 9; i++) v[i] = strtoull(*p++, nullptr, 0);
    zn_run_desc d;
    memset(&d, 0, sizeof d);
    d.table = (const void *)(uintptr_t)v[0]; d.slot = (uint32_t)v[1]; d.lane_run = (uint8_t)v[2]; d.verify_only = (uint8_t)v[3];
    d.d_blobs = v[4]; d.blob_base = v[5]; d.blob_cap = v[6]; d.d_out = v[7]; d.out_cap = v[8];
    return d;
}
int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        char *tok[32]; int n = 0;
        for (char *t = strtok(line, " \n"); t && n < 32; t = strtok(nullptr, " \n")) tok[n++] = t;
        if (!n) continue;
        char **p = tok + 1;
        if (tok[0][0] == 'R' && n == 5) {
            uint64_t v[4];
            for (int i = 0; i < 4; i++) v[i] = strtoull(*p++, nullptr, 0);
            printf("%d\n", zn_regions_disjoint(v[0], v[1], v[2], v[3]));
        } else if (tok[0][0] == 'P' && n == 19) {
            const zn_run_desc a = desc(p), b = desc(p);
            printf("%d\n", zn_runs_may_overlap(&a, &b));
        } else { printf("bad line\n"); return 2; }
    }
    printf("%d\n", zn_runs_may_overlap(nullptr, nullptr));
    return 0;
}
"""

UND = (1 << 64) - 1
T1, T2 = 0x1000, 0x2000
K = 1 << 20


def run(table=T1, slot=0, lane=1, verify=0, blobs=0x10 * K, base=0, bcap=K, out=0x20 * K, ocap=4 * K):
    return (table, slot, lane, verify, blobs, base, bcap, out, ocap)


# (what, prev, next, may overlap)
PAIRS = [
    ("identical arguments, the table's two slots", run(slot=0), run(slot=1), 1),
    ("identical arguments, undeclared blob size", run(slot=0, bcap=UND), run(slot=1, bcap=UND), 1),
    ("identical but for the blob base", run(slot=0, bcap=UND), run(slot=1, bcap=UND, base=64), 0),
    ("identical but for the declared blob size", run(slot=0), run(slot=1, bcap=K + 1), 0),
    ("same slot of one table", run(slot=1), run(slot=1), 0),
    ("same slot, different tables, identical buffers: the tables differ, the outputs collide", run(slot=1), run(table=T2, slot=1), 0),
    ("different tables, disjoint everything", run(slot=0), run(table=T2, slot=0, blobs=0x30 * K, out=0x40 * K), 1),
    ("different tables, same blobs, disjoint outputs", run(slot=0), run(table=T2, slot=0, out=0x40 * K), 1),
    ("predecessor is no lane run", run(slot=0, lane=0), run(slot=1), 0),
    ("successor is no lane run", run(slot=0), run(slot=1, lane=0), 0),
    ("other blobs, disjoint outputs", run(slot=0), run(slot=1, blobs=0x30 * K, out=0x40 * K), 1),
    ("other blobs, outputs that touch", run(slot=0), run(slot=1, blobs=0x30 * K, out=0x20 * K + 4 * K), 1),
    ("other blobs, outputs that overlap by one byte", run(slot=0), run(slot=1, blobs=0x30 * K, out=0x20 * K + 4 * K - 1), 0),
    ("other blobs, the same output", run(slot=0), run(slot=1, blobs=0x30 * K), 0),
    ("other blobs of undeclared size, disjoint outputs", run(slot=0), run(slot=1, blobs=0x30 * K, bcap=UND, out=0x40 * K), 0),
    ("predecessor's blobs of undeclared size, successor writes elsewhere", run(slot=0, bcap=UND), run(slot=1, blobs=0x30 * K, out=0x40 * K), 0),
    ("successor reads inside the predecessor's output", run(slot=0), run(slot=1, blobs=0x20 * K + K, out=0x40 * K), 0),
    ("successor's blobs end where the predecessor's output begins", run(slot=0), run(slot=1, blobs=0x20 * K - K, out=0x40 * K), 1),
    ("successor writes over the predecessor's blobs", run(slot=0), run(slot=1, blobs=0x30 * K, out=0x10 * K - 2 * K), 0),
    ("verify-only successor, same output as nobody: other blobs", run(slot=0), run(slot=1, verify=1, blobs=0x30 * K, out=0, ocap=0), 1),
    ("verify-only successor reading the predecessor's output", run(slot=0), run(slot=1, verify=1, blobs=0x20 * K, out=0, ocap=0), 0),
    ("verify-only predecessor, successor decodes the same blobs", run(slot=0, verify=1, out=0, ocap=0), run(slot=1), 1),
    ("verify-only predecessor, successor writes over its blobs", run(slot=0, verify=1, out=0, ocap=0), run(slot=1, blobs=0x30 * K, out=0x10 * K), 0),
    ("both verify-only, other blobs", run(slot=0, verify=1, out=0, ocap=0), run(slot=1, verify=1, blobs=0x30 * K, out=0, ocap=0), 1),
    ("both verify-only, identical, undeclared", run(slot=0, verify=1, bcap=UND, out=0, ocap=0), run(slot=1, verify=1, bcap=UND, out=0, ocap=0), 1),
    ("verify-only successor with blobs of undeclared size, other blobs", run(slot=0), run(slot=1, verify=1, blobs=0x30 * K, bcap=UND, out=0, ocap=0), 0),
    ("a decode run and a verify-only run with the same blobs are not identical runs, but cannot collide", run(slot=0), run(slot=1, verify=1, out=0, ocap=0), 1),
    ("zero-length outputs at one address", run(slot=0, ocap=0), run(slot=1, blobs=0x30 * K, ocap=0), 1),
    ("zero-length blob region inside the predecessor's output", run(slot=0), run(slot=1, blobs=0x20 * K + 5, bcap=0, out=0x40 * K), 1),
    ("predecessor's output wraps 2^64", run(slot=0, out=UND - 100, ocap=4 * K), run(slot=1, blobs=0x30 * K, out=0x40 * K), 0),
    ("successor's blob region wraps 2^64", run(slot=0), run(slot=1, blobs=UND - 10, bcap=K, out=0x40 * K), 0),
    ("successor's output ends at 2^64 - 1 and wraps nothing", run(slot=0), run(slot=1, blobs=0x30 * K, out=UND - 4 * K, ocap=4 * K), 1),
]

# (a, a_len, b, b_len, disjoint)
REGIONS = [
    (0, 10, 10, 10, 1), (0, 11, 10, 10, 0), (10, 10, 0, 10, 1), (10, 10, 0, 11, 0), (5, 1, 0, 10, 0), (0, 10, 5, 1, 0),
    (5, 0, 0, 10, 1), (0, 10, 5, 0, 1), (0, 0, 0, 0, 1),
    (UND - 5, 5, 0, 10, 1), (UND - 5, 6, 0, 10, 0), (UND - 5, 6, 100, 10, 0), (0, 10, UND, 1, 0), (0, UND, UND - 1, 1, 0), (0, UND - 1, UND - 1, 1, 1),
]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("run_lanes_rule")
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "rule"
    # (gcc links the sanitizers' runtimes dynamically unless told otherwise; linked into the program they do not care what else
    # the process loads)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", HOST, str(main), os.path.join(HOST, "run_overlap.cc"), "-o", str(exe)], check=True)
    return str(exe)


def test_rule_over_the_table_of_cases(program):
    lines = [f"R {a} {al} {b} {bl}" for a, al, b, bl, _ in REGIONS]
    lines += ["P " + " ".join(str(v) for v in p + n) for _, p, n, _ in PAIRS]
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(REGIONS) + len(PAIRS) + 1
    for (a, al, b, bl, want), g in zip(REGIONS, got):
        assert g == want, ("regions", hex(a), al, hex(b), bl, g)
    for (what, _, _, want), g in zip(PAIRS, got[len(REGIONS):]):
        assert g == want, (what, g)
    assert got[-1] == 0   # null descriptions: never


def test_a_reader_and_a_writer_of_one_region_in_both_orders(program):
    """A run that reads where another writes is ordered whichever of them is queued first."""
    a, b = run(slot=0), run(slot=1, verify=1, blobs=0x20 * K, out=0, ocap=0)   # b reads what a writes
    lines = ["P " + " ".join(str(v) for v in a + b), "P " + " ".join(str(v) for v in b + a)]
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(x) for x in r.stdout.split()] == [0, 0, 0]   # (a behind b: a writes where b still reads)
