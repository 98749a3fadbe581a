"""The plan of a write-side run (znippy_amd/csrc/host/enc_plan.cc: which kernels znippy_encode_hash_rounds_async launches, on
which streams, with what geometry) as a stand-alone host program under AddressSanitizer and UBSan.  Shapes go in on stdin, every
EncPlan field comes back, and a model written from the statements of the rules — the comments of the launch function before it
was split, restated in `Model` below — is compared with it field by field.

Two grids, each a full product, go through ONE process:
  routes    level x window_log x far-window buffers x the three switches x store_incompressible x emit_tree x blob_align x fuse_tiles
            x (n_small, n_wide in {0, 1, many}) x (n_items == n, > n) x enc_bytes around half of in_bytes x mean piece 16384 / 16385
  geometry  n_small x n_wide over {0} and the sizes around the two ends of the batch clamp, x fuse_tiles x ZNIPPY_NO_FUSE_HASH
            x (n_items == n, > n)
(the sizes of the batch clamp are a share's own, so they are crossed with each other instead of with every route.)  Tables are
coherent where the plan's inputs are coupled in a real table: one with no more pieces than rounds has no stored pieces, no far
window regions and no tree entries; the others have three stored pieces and some of each.
The slab layout (ResSlab) is checked by the same program over heap blocks of exactly ResSlab::bytes(n)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "znippy_amd", "csrc", "host")

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "enc_plan.h"
// stdin: "P" + 13 shape fields + 8 context fields (the order of EncShape and EncEnv), or "L n" (slab layout)
static void launch(const EncLaunch &l) { printf(" %d %u %d %d %u", l.on, l.n_items, l.use_order, l.grid, l.batch); }
int main() {
    char tag[8];
    while (scanf("%7s", tag) == 1) {
        if (tag[0] == 'P') {
            unsigned long long v[21];
            for (auto &x : v) if (scanf("%llu", &x) != 1) { printf("bad line\n"); return 2; }
            EncShape s{};
            s.n = (uint32_t)v[0]; s.n_items = (uint32_t)v[1]; s.n_small = (uint32_t)v[2]; s.n_wide = (uint32_t)v[3];
            s.in_bytes = v[4]; s.enc_bytes = v[5]; s.fuse_tiles = (int)v[6]; s.plan_n_tiles = (uint32_t)v[7];
            s.n_tree_entries = (uint32_t)v[8]; s.ldm_entries = v[9];
            s.store_incompressible = v[10] != 0; s.emit_tree = v[11] != 0; s.blob_align = (uint32_t)v[12];
            EncEnv e{};
            e.level = (int)v[13]; e.window_log = (int)v[14]; e.encode_grid = (int)v[15]; e.encode_grid_small = (int)v[16];
            e.nohash = v[17] != 0; e.no_fuse_hash = v[18] != 0; e.no_fused_store = v[19] != 0; e.ldm_ok = v[20] != 0;
            const EncPlan p = enc_plan(s, e);
            printf("%d %d %d %d %d %d %d %d %d %d %d %d %d", p.high, p.window_log, p.tail_mark, p.far, p.fuse_hash, p.fuse_store, p.fork_aux,
                   p.hash_beside, p.emit_tree, p.tree_out, p.store_decide, p.pad, p.small_pieces);
            launch(p.wide); launch(p.small); launch(p.retry);
            printf(" %d\n", enc_window_log(e));
        } else if (tag[0] == 'L') {
            unsigned long long n;
            if (scanf("%llu", &n) != 1) { printf("bad line\n"); return 2; }
            const size_t bytes = ResSlab::bytes(n);
            uint8_t *b = (uint8_t *)malloc(bytes);
            memset(b, 0xEE, bytes);
            const ResSlab r{b, (uint32_t)n};
            *r.total() = 1; *r.overflow() = 2;
            for (size_t i = 0; i < n; i++) { r.blob_offset()[i] = 3; r.blob_size()[i] = 4; memset(r.digests() + 8 * i, 5, 32); }
            size_t covered = 0;  // every byte but the four unused ones was written, by exactly the field the layout names
            for (size_t i = 0; i < bytes; i++) covered += b[i] != 0xEE;
            printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", (size_t)((uint8_t *)r.total() - b), (size_t)((uint8_t *)r.overflow() - b),
                   (size_t)((uint8_t *)r.blob_offset() - b), (size_t)((uint8_t *)r.blob_size() - b), (size_t)((uint8_t *)r.digests() - b),
                   ResSlab::clear_bytes(n), bytes, covered);
            free(b);
        } else { printf("bad line\n"); return 2; }
    }
    return 0;
}
"""

HIGH_TIER_LEVEL = 4
G, GS = 256 * 8, 256 * 16     # the grids of a 256-CU chip: 8 / 16 resident workgroups per CU for the wide / the small variant
SHAPE = ("n", "n_items", "n_small", "n_wide", "in_bytes", "enc_bytes", "fuse_tiles", "plan_n_tiles", "n_tree_entries", "ldm_entries",
         "store_incompressible", "emit_tree", "blob_align")
ENV = ("level", "window_log", "encode_grid", "encode_grid_small", "nohash", "no_fuse_hash", "no_fused_store", "ldm_ok")
OUT = ("high", "window_log", "tail_mark", "far", "fuse_hash", "fuse_store", "fork_aux", "hash_beside", "emit_tree", "tree_out", "store_decide",
       "pad", "small_pieces") + tuple(f"{w}.{f}" for w in ("wide", "small", "retry") for f in ("on", "n_items", "use_order", "grid", "batch")) + \
      ("enc_window_log",)


def clamp_sizes(g):
    """A share's sizes around both ends of max(1, min(16, n / (2 g)))."""
    return [1, 2 * g - 1, 2 * g, 32 * g, 32 * g + 1]


def table(n_small, n_wide, more_pieces, enc_sel, mean, fuse_tiles, store_inc, emit, align):
    """Coherent table shapes, over columns.  more_pieces: n_items > n (a table with stored rounds and rounds of several blocks)."""
    more = more_pieces.astype(bool)
    n_items = n_small + n_wide + np.where(more | (n_small + n_wide == 0), 3, 0)
    n = np.where(more, np.maximum(1, n_items - 2), n_items)
    in_bytes = n_items * mean
    enc_bytes = np.choose(enc_sel, [0 * in_bytes, in_bytes // 2 - 1, in_bytes // 2, in_bytes // 2 + 1])
    return dict(n=n, n_items=n_items, n_small=n_small, n_wide=n_wide, in_bytes=in_bytes, enc_bytes=enc_bytes, fuse_tiles=fuse_tiles,
                plan_n_tiles=(n + 5) // 6 + 1, n_tree_entries=np.where(more, 7, 0), ldm_entries=np.where(more, 2048, 0),
                store_incompressible=store_inc, emit_tree=emit, blob_align=align)


def product(*dims):
    """The full product of the dimensions' values, one int64 column per dimension."""
    return [c.reshape(-1) for c in np.meshgrid(*[np.array(d, dtype=np.int64) for d in dims], indexing="ij")]


def grids():
    """(shape columns, context columns) of both grids, one behind the other."""
    sw = (0, 1)
    lvl, wl, ldm, nh, nfh, nfs, si, et, al, ft, ns, nw, more, es, mean = product(
        (HIGH_TIER_LEVEL - 1, HIGH_TIER_LEVEL), (0, 20), sw, sw, sw, sw, sw, sw, (1, 16, 64), (0, 1, 2),
        (0, 1, 32 * GS + 1), (0, 1, 32 * G + 1), sw, range(4), (16384, 16385))
    routes = table(ns, nw, more, es, mean, ft, si, et, al), dict(level=lvl, window_log=wl, nohash=nh, no_fuse_hash=nfh, no_fused_store=nfs, ldm_ok=ldm)
    ns, nw, ft, nfh, more = product([0] + clamp_sizes(GS), [0] + clamp_sizes(G), (0, 1, 2), sw, sw)
    z = 0 * ns
    geometry = table(ns, nw, more, z + 3, z + 4096, ft, z, z, z + 1), dict(level=z + 3, window_log=z, nohash=z, no_fuse_hash=nfh, no_fused_store=z, ldm_ok=z + 1)
    s = {k: np.concatenate([routes[0][k], geometry[0][k]]) for k in SHAPE}
    e = {k: np.concatenate([routes[1][k], geometry[1][k]]) for k in routes[1]}
    e["encode_grid"], e["encode_grid_small"] = 0 * e["level"] + G, 0 * e["level"] + GS
    return s, e


class Model:
    """The rules, from their statements, over columns of cases (int64; the biggest product here is far below 2^63)."""

    def __init__(self, s, e):
        T = lambda x: x.astype(bool)
        high = e["level"] >= HIGH_TIER_LEVEL                          # levels 4-22: the higher effort tier
        self.high = high
        self.window_log = np.where(high, e["window_log"], 0)           # the fast tier keeps its frames
        self.enc_window_log = self.window_log
        self.tail_mark = high & (self.window_log == 0)                  # the closing block says every block stands alone: not with a window
        self.far = (self.window_log != 0) & (s["ldm_entries"] != 0) & T(e["ldm_ok"])   # any failure leaves the far window off
        nohash = T(e["nohash"])
        store_inc = T(s["store_incompressible"])
        # tables of small encoded rounds only: the encoder's waves hash the rounds they encode
        self.fuse_hash = (s["fuse_tiles"] > 0) & ~store_inc & ~nohash & ~T(e["no_fuse_hash"])
        # store-heavy: most bytes are skip rounds (at least half of them do not go through the encoder)
        heavy = (s["in_bytes"] > 0) & ((s["in_bytes"] - s["enc_bytes"]) * 2 >= s["in_bytes"])
        self.fuse_store = heavy & ~store_inc & ~T(e["no_fused_store"]) & ~nohash
        self.fork_aux = ~self.fuse_store & ~self.fuse_hash               # otherwise the hash runs beside the encoder on the auxiliary stream
        self.hash_beside = self.fork_aux & ~nohash
        self.emit_tree = T(s["emit_tree"]) & ~nohash                    # the no-hash switch leaves nothing to make entries from
        self.tree_out = self.emit_tree & (s["n_tree_entries"] > 0)
        self.store_decide = store_inc
        self.pad = s["blob_align"] > 1
        # lane-per-piece gather: only tables without blocks above 16 KiB whose pieces average 16 KiB at most — or store-heavy ones
        self.small_pieces = (s["n_items"] > 0) & (s["n_wide"] == 0) & (self.fuse_store | (s["in_bytes"] // np.maximum(s["n_items"], 1) <= 16384))
        for name, cnt, g in (("wide", s["n_wide"], e["encode_grid"]), ("small", s["n_small"], e["encode_grid_small"])):
            on = cnt > 0
            grid = np.minimum(g, cnt)
            if name == "small":  # the encoder that hashes dequeues tiles: ceil(tiles / fuse_tiles) workgroups, capped by the grid
                ft = np.maximum(s["fuse_tiles"], 1)
                grid = np.where(self.fuse_hash, np.minimum(g, (s["plan_n_tiles"] + ft - 1) // ft), grid)
            self.launch(name, on, cnt, cnt != s["n_items"],              # all of one kind: no indirection
                        grid, np.clip(cnt // (2 * g), 1, 16))
        on = s["n_small"] > 0                                            # second wide launch: whatever the small variant handed over
        self.launch("retry", on, s["n_small"], on, np.minimum(e["encode_grid"], s["n_small"]), np.ones_like(s["n"]))

    def launch(self, name, on, n_items, use_order, grid, batch):
        for f, v in (("on", on), ("n_items", n_items), ("use_order", use_order), ("grid", grid), ("batch", batch)):
            setattr(self, f"{name}.{f}", np.where(on, v, 0))            # a launch that is off has no geometry


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("enc_plan")
    main = d / "main.cc"
    main.write_text(MAIN)
    exe = d / "plan"
    # (gcc links the sanitizers' runtimes dynamically unless told otherwise; linked into the program they do not care what else
    # the process loads)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) and "g++" in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", HOST, str(main), os.path.join(HOST, "enc_plan.cc"), "-o", str(exe)], check=True)
    return str(exe)


def test_plan_over_both_grids(program):
    s, e = grids()
    cols = np.stack([s[k] for k in SHAPE] + [e[k] for k in ENV], axis=1)
    assert len(cols) == 2 ** 8 * 3 * 3 * 9 * 2 * 4 * 2 + 36 * 3 * 2 * 2    # no case is left out
    text = "\n".join("P " + " ".join(map(str, row)) for row in cols.tolist()) + "\n"
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    got = np.array(r.stdout.split(), dtype=np.int64).reshape(len(cols), len(OUT))
    m = Model(s, e)
    for j, name in enumerate(OUT):
        want = np.asarray(getattr(m, name)).astype(np.int64)
        bad = np.nonzero(got[:, j] != want)[0]
        assert not len(bad), (name, len(bad), "first", dict(zip(SHAPE + ENV, cols[bad[0]].tolist())), "got", int(got[bad[0], j]), "want", int(want[bad[0]]))
    # the grids reach both sides of every rule
    for name in OUT:
        assert len(np.unique(np.asarray(getattr(m, name)).astype(np.int64))) >= 2, name
    assert set(np.unique(getattr(m, "wide.batch"))) >= {0, 1, 16} and set(np.unique(getattr(m, "small.batch"))) >= {0, 1, 16}
    assert (m.fuse_hash & (getattr(m, "small.grid") < GS) & (s["n_small"] > GS)).any()      # the tile count, not the grid, sizes a fused launch
    assert (m.fuse_hash & (getattr(m, "small.grid") == GS)).any()                            # ... and the grid caps it


def test_slab_layout(program):
    """[total u64][overflow u32 + 4 unused][blob_offset u64 x n][blob_size u64 x n][digests 32 x n]: 48 bytes per round behind 16."""
    ns = [0, 1, 2, 7, 1000]
    r = subprocess.run([program], input="".join(f"L {n}\n" for n in ns), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert rows == [[0, 8, 16, 16 + 8 * n, 16 + 16 * n, 16 + 16 * n, 16 + 48 * n, 12 + 48 * n] for n in ns]
