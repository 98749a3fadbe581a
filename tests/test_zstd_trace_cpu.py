"""oracle.zstd_trace: the oracle's strict RFC 8878 decode (oracle/zstd_ref.c) with a recorder that says what a frame contains:
header form, blocks, literal sections, Huffman trees, sequence counts, table modes with their counts as read, and every sequence.
It is what the encoder's edge tests (test_gpu_encoder_edges.py) read the encoder's frames with.

Three sources say the trace is right.  The hand-built corpus of zstd_synth_cases.py is written from a description: the trace of the
frame must give that description back (literal bytes, sequences, and wherever the case records them the modes, count forms, table
logs and tree shapes).  `zstd_synth.execute` of any traced description must be the decoded bytes.  libzstd's frames (levels 1, 3,
19, one of three blocks) go through the same check.  The recorder itself runs as a stand-alone program under AddressSanitizer and
UBSan over all those frames, with buffers of exactly the size it asked for and with none at all, and must print what the in-process
trace found."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import gen
import zstd_synth as Z
import zstd_synth_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALID = {c.name: c for c in K.valid_cases()}
KIND_SHIFT = {"ll": 6, "of": 4, "ml": 2}


def trace_of(oracle, c):
    return oracle.zstd_trace(c.frame, cap=len(c.want))


def strip(norm):
    norm = list(norm)
    while norm and norm[-1] == 0:
        norm.pop()
    return norm


@pytest.mark.parametrize("name", list(VALID))
def test_trace_gives_the_description_back(oracle, name):
    c = VALID[name]
    tr = trace_of(oracle, c)
    assert tr["content"] == c.want and len(tr["frames"]) == 1
    F = tr["frames"][0]
    B = F["blocks"]
    assert F["regenerated"] == len(c.want)
    assert (F["fcs_bytes"] == 0) == c.no_size == (not F["has_size"])
    if not c.no_size:
        assert F["content_size"] == len(c.want)
    want_types = [0 if isinstance(b, Z.Raw) else (1 if isinstance(b, Z.Rle) else 2) for b in c.blocks]
    assert [b["type"] for b in B][:len(want_types)] == want_types and len(B) - len(want_types) in (0, 1)
    assert [b["last"] for b in B] == [0] * (len(B) - 1) + [1]
    at = 0
    for b, d in zip(B, c.blocks):
        assert b["at"] == at
        if b["type"] == 0:
            assert b["size"] == len(d.data)
            at += len(d.data)
        elif b["type"] == 1:
            assert b["size"] == d.n and tr["content"][at] == d.byte
            at += d.n
        else:
            assert b["lits"]["bytes"] == d.lits and b["lits"]["regen"] == len(d.lits)
            assert [tuple(int(x) for x in s[:3]) for s in b["seqs"]] == d.seqs and b["nseq"] == len(d.seqs)
            assert b["lits"]["type"] == {"raw": 0, "rle": 1, "huf": 2, "treeless": 3}[d.lit.get("type", "raw")]
            if d.lit.get("fmt") is not None:
                assert b["lits"]["size_format"] == d.lit["fmt"]
            assert b["lits"]["streams"] == (0 if b["lits"]["type"] < 2 else (1 if b["lits"]["size_format"] == 0 else 4))
            assert (b["huf"] is not None) == (b["lits"]["type"] == 2)
            if b["huf"]:
                assert b["huf"]["kind"] == d.lit.get("wdesc", "direct")
                given = d.lit.get("weights")
                assert b["huf"]["weights"] == list(given if given is not None else Z.huf_weights(d.lits))
                W = b["huf"]["weights"]
                assert 1 << b["huf"]["max_bits"] == sum(1 << (w - 1) for w in W if w) and b["huf"]["max_bits"] <= 11
                assert b["huf"]["longest"] == b["huf"]["max_bits"] + 1 - min(w for w in W if w)
            if d.nseq_form:
                assert b["nseq_bytes"] == d.nseq_form
            assert (b["modes"] is None) == (not d.seqs)
            for kind in ("ll", "of", "ml") if d.seqs else ():
                t, choice = b["tables"][kind], getattr(d, kind)
                assert t["mode"] == (b["modes"] >> KIND_SHIFT[kind]) & 3
                if choice == "pre":
                    assert t["mode"] == 0 and t["log"] == Z.DEFAULTS[kind][1]
                elif choice == "rle" or (isinstance(choice, tuple) and choice[0] == "rle"):
                    assert t["mode"] == 1 and t["rle_symbol"] is not None
                elif choice == "rep":
                    assert t["mode"] == 3
                elif isinstance(choice, tuple):
                    assert t["mode"] == 2 and t["log"] == choice[2] and t["norm"] == strip(choice[1])
                if t["mode"] == 2:
                    assert sum(abs(x) for x in t["norm"]) == 1 << t["log"]
            assert all(int(s[3]) >= 1 for s in b["seqs"])
            for s in b["seqs"]:
                if int(s[2]) > 3:
                    assert int(s[3]) == int(s[2]) - 3
            at += len(d.lits) + sum(s[1] for s in d.seqs)
    assert at == len(c.want)
    for key, val in c.promise.items():
        if key == "fhd":
            assert F["fhd"] == val and F["fcs_bytes"] == (((val >> 5) & 1) if val >> 6 == 0 else 1 << (val >> 6))
        elif key == "skippable":
            assert len(tr["skippable"]) == val
        elif key == "types":
            assert [b["type"] for b in B] == val
        elif key == "sizes":
            for i, v in (val.items() if isinstance(val, dict) else enumerate(val)):
                assert B[i]["size"] == v
        elif key == "modes":
            for i, v in val.items():
                assert B[i]["modes"] == v
        elif key == "lit":
            for i, v in val.items():
                L = B[i]["lits"]
                assert (L["type"], L["size_format"], L["regen"]) == v
        elif key == "nseq":
            for i, v in val.items():
                assert (B[i]["nseq_bytes"], B[i]["nseq"]) == v
        elif key == "fse":
            for i, kinds in val.items():
                for kind, (log, low) in kinds.items():
                    t = B[i]["tables"][kind]
                    assert (t["mode"], t["log"], t["norm"].count(-1)) == (2, log, low)
        elif key == "tree":
            for i, v in val.items():
                assert B[i]["huf"]["kind"] == v
        elif key == "nweights":
            for i, v in val.items():
                assert len(B[i]["huf"]["weights"]) - 1 == v
        elif key == "last_weight":
            for i, v in val.items():
                assert B[i]["huf"]["weights"][-1] == v
        elif key == "huf_bits":
            for i, v in val.items():
                assert B[i]["huf"]["max_bits"] == v
        elif key == "max_codes":
            for i, v in val.items():
                got = dict(ll=max(Z.ll_code(int(s[0]))[0] for s in B[i]["seqs"]), ml=max(Z.ml_code(int(s[1]))[0] for s in B[i]["seqs"]),
                           of=max(Z.of_code(int(s[2]))[0] for s in B[i]["seqs"]))
                assert all(got[k] == x for k, x in v.items())
        else:
            assert key in ("fcs_raw", "zero_runs"), key


def says_the_bytes_again(oracle, frame, data):
    """execute(trace) == decode, resolved distances as the executor's own history gives them; -> the trace."""
    tr = oracle.zstd_trace(frame, cap=len(data))
    assert tr["content"] == data == oracle.zstd_decompress(frame, cap=len(data))
    blocks = [b for f in tr["frames"] for b in Z.blocks_of_trace(f, tr["content"])]
    assert len(tr["frames"]) == 1 and Z.execute(blocks) == data
    return tr


@pytest.mark.parametrize("name", list(VALID))
def test_executing_the_trace_is_the_decode(oracle, name):
    c = VALID[name]
    says_the_bytes_again(oracle, c.frame, c.want)


def byte_skew(n, seed, symbols=200):
    """As test_gpu_levels._byte_skew: an alphabet reaching beyond 127, skewed, nothing to match."""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, symbols + 1) ** 1.2
    vals = ((np.arange(symbols) * 37 + 11) % 256).astype(np.uint8)
    return vals[rng.choice(symbols, size=n, p=w / w.sum())].tobytes()


LIBZSTD = [(kind, n, level) for kind, n in (("pseudo_text", 3000), ("pseudo_text", 70_000), ("byte_skew", 20_000), ("pseudo_text", 300_000))
           for level in (1, 3, 19)]


def libzstd_input(kind, n):
    return gen.pseudo_text(n, seed=n % 97) if kind == "pseudo_text" else byte_skew(n, 3)


@pytest.mark.parametrize("kind,n,level", LIBZSTD)
def test_libzstd_frames(oracle, kind, n, level):
    if not oracle.have_libzstd():
        pytest.skip("no libzstd on this machine")
    data = libzstd_input(kind, n)
    frame = oracle.libzstd_compress(data, level)
    tr = says_the_bytes_again(oracle, frame, data)
    B = tr["frames"][0]["blocks"]
    assert len(B) >= (n + Z.BLOCK_MAX - 1) // Z.BLOCK_MAX and sum(b["type"] == 2 for b in B) >= 1
    if kind == "byte_skew":
        assert any(b["type"] == 2 and b["huf"] and b["huf"]["kind"] == "fse" for b in B)      # symbols beyond 127: FSE-compressed weights
    if n == 300_000:
        assert len(B) >= 3


# ---- the recorder under the sanitizers, as a program of its own ---------------------------------------------------------------

MAIN = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int64_t oracle_zstd_trace(uint8_t *dst, size_t cap, const uint8_t *src, size_t n, int64_t *ev, size_t ev_cap, uint64_t *sq, size_t sq_cap,
                          uint8_t *lit, size_t lit_cap, uint64_t *need);
int64_t oracle_zstd_decompress(uint8_t *dst, size_t cap, const uint8_t *src, size_t n);
static uint32_t adler(const void *p, size_t n) {
    const uint8_t *b = (const uint8_t *)p; uint32_t a = 1, s = 0; size_t i;
    for (i = 0; i < n; i++) { a = (a + b[i]) % 65521u; s = (s + a) % 65521u; }
    return (s << 16) | a;
}
/* file: records of u32 frame bytes, u32 output capacity, the frame.  Every buffer is a heap block of exactly the size in use. */
int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : NULL;
    uint32_t h[2];
    if (!f) return 2;
    while (fread(h, 4, 2, f) == 2) {
        uint8_t *src = (uint8_t *)malloc(h[0] + !h[0]), *dst = (uint8_t *)malloc(h[1] + !h[1]), *plain = (uint8_t *)malloc(h[1] + !h[1]);
        uint64_t need[3], again[3];
        int64_t r0, r1, r2;
        if (fread(src, 1, h[0], f) != h[0]) return 2;
        r0 = oracle_zstd_decompress(plain, h[1], src, h[0]);
        r1 = oracle_zstd_trace(dst, h[1], src, h[0], NULL, 0, NULL, 0, NULL, 0, need);      /* no room at all: counts only */
        {
            int64_t *ev = (int64_t *)malloc(need[0] * 8 + !need[0]);
            uint64_t *sq = (uint64_t *)malloc(need[1] * 32 + !need[1]);
            uint8_t *lit = (uint8_t *)malloc(need[2] + !need[2]);
            r2 = oracle_zstd_trace(dst, h[1], src, h[0], ev, need[0], sq, need[1], lit, need[2], again);
            if (r0 != r1 || r1 != r2 || memcmp(need, again, sizeof need) || (r0 > 0 && memcmp(plain, dst, (size_t)r0))) { printf("MISMATCH\n"); return 3; }
            printf("%lld %llu %llu %llu %u %u %u\n", (long long)r2, (unsigned long long)need[0], (unsigned long long)need[1],
                   (unsigned long long)need[2], adler(ev, need[0] * 8), adler(sq, need[1] * 32), adler(lit, need[2]));
            if (need[0] > 8) {                                                               /* a room one record short */
                int64_t *small = (int64_t *)malloc((need[0] - 3) * 8);
                oracle_zstd_trace(dst, h[1], src, h[0], small, need[0] - 3, sq, need[1] / 2, lit, need[2] / 2, again);
                if (memcmp(need, again, sizeof need)) { printf("MISMATCH\n"); return 3; }
                free(small);
            }
            free(ev); free(sq); free(lit);
        }
        free(src); free(dst); free(plain);
    }
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no host C compiler"
    d = tmp_path_factory.mktemp("zstd_trace")
    main = d / "main.c"
    main.write_text(MAIN)
    exe = d / "trace"
    static = ["-static-libasan", "-static-libubsan"] if "gcc" in os.path.basename(cc) else []
    subprocess.run([cc, "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   [str(main), os.path.join(ROOT, "oracle", "zstd_ref.c"), "-o", str(exe)], check=True)
    return str(exe), d


def test_recorder_under_sanitizers(oracle, program):
    exe, d = program
    frames = [(c.frame, len(c.want)) for c in K.valid_cases()] + [(c.frame, len(c.want) + 16) for c in K.invalid_cases()]
    if oracle.have_libzstd():
        for kind, n, level in LIBZSTD:
            data = libzstd_input(kind, n)
            frames.append((oracle.libzstd_compress(data, level), n))
    frames += [(f[:len(f) // 2], cap) for f, cap in frames[::7]]                             # cut in the middle: errors part-way through
    path = d / "frames.bin"
    with open(path, "wb") as fh:
        for f, cap in frames:
            fh.write(struct.pack("<II", len(f), cap) + f)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(frames)
    ok = 0
    for (f, cap), line in zip(frames, lines):
        got = [int(x) for x in line.split()]
        try:
            tr = oracle.zstd_trace(f, cap=cap)
        except ValueError:
            assert got[0] < 0
            continue
        ok += 1
        assert got[0] == len(tr["content"])
        blocks = [b for fr in tr["frames"] for b in fr["blocks"] if b["type"] == 2]
        assert got[2] == sum(b["nseq"] for b in blocks) and got[3] == sum(b["lits"]["regen"] for b in blocks)
        sq = np.concatenate([b["seqs"] for b in blocks] + [np.zeros((0, 4), np.uint64)])
        assert got[5] == zlib.adler32(np.ascontiguousarray(sq).tobytes())
        assert got[6] == zlib.adler32(b"".join(b["lits"]["bytes"] for b in blocks))
    assert ok >= len(K.valid_cases())
