"""Every route of the write-side launch (api.hip: rounds_launch; the plan: host/enc_plan.cc), pinned by its launch sequence.

Each route runs on ONE RoundTable: three encode_hash_async calls into three blob buffers with results_lagged(1) between them, kernel
timing on, and after every call the ordered names of Context.kernel_times() are compared with a literal list.  The lists in
EXPECT were recorded on the commit BEFORE the launch was split into a plan and stages, so they pin that commit's sequence, not
the code's own.  Every run's blobs are decoded by the oracle and compared with the source, its digests with the oracle's BLAKE3."""
import hashlib

import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu

TEXT, SKIP_LEN = 320_000, 70_001
KIB = 1024

ROUNDS = {  # (source offset, length, skip) over pseudo-text [0, TEXT) and incompressible bytes behind it
    # 8 rounds of 4 KiB text: every round one small block, no store path — the encoder's waves hash what they encode
    "small": [(4 * KIB * i, 4 * KIB, 0) for i in range(8)],
    # small, wide and multi-block rounds: both encoder variants through their index lists, the retry launch, big hash units
    "mixed": [(0, 4 * KIB, 0), (5_000, 20 * KIB, 0), (30_000, 200 * KIB, 0), (1_000, 4 * KIB, 0), (250_000, 20 * KIB, 0), (77, 4 * KIB, 0)],
    # most bytes stored, at odd blob offsets: the hash behind the gather copies what it hashes
    "stored": [(TEXT + SKIP_LEN * i, SKIP_LEN, 1) for i in range(6)] + [(9_000, 4 * KIB, 0), (100_000, 4 * KIB, 0)],
    # ... with stored rounds of two blocks, which have block tree entries (a round of one block has none)
    "stored_big": [(TEXT + 2 * SKIP_LEN * i, 2 * SKIP_LEN - 1, 1) for i in range(3)] + [(9_000, 4 * KIB, 0), (100_000, 4 * KIB, 0)],
    "empty": [],
    "one_empty_round": [(0, 0, 0)],
}
ROUNDS["mixed_far"] = ROUNDS["mixed"] + [(10, 300_001, 0)]

ROUTES = {  # name: (rounds, table options, (level, window_log) or None, environment of the context or None)
    "fused_hash": ("small", {}, None, None),
    "hash_beside": ("mixed", {}, None, None),
    "fused_store": ("stored", {}, None, None),
    "store_incompressible": ("mixed", dict(store_inc=True), None, None),
    "blob_align_64": ("mixed", dict(align=64), None, None),
    "window": ("mixed_far", {}, (19, 17), None),
    "tree_fused_store": ("stored", dict(emit=True), None, None),
    "tree_hash_beside": ("mixed", dict(emit=True), None, None),
    "tree_fused_store_big": ("stored_big", dict(emit=True), None, None),
    "small_no_fuse_hash": ("small", {}, None, {"ZNIPPY_NO_FUSE_HASH": "1"}),
    "stored_no_fuse_hash": ("stored", {}, None, {"ZNIPPY_NO_FUSE_HASH": "1"}),
    "small_no_fused_store": ("small", {}, None, {"ZNIPPY_NO_FUSED_STORE": "1"}),
    "stored_no_fused_store": ("stored", {}, None, {"ZNIPPY_NO_FUSED_STORE": "1"}),
    "empty": ("empty", {}, None, None),
    "one_empty_round": ("one_empty_round", {}, None, None),
}

_BESIDE = "zstd_encode blake3_tiles blake3_merge_big piece_scan gather"
EXPECT = {  # recorded on the parent commit: the names after each of the three calls
    "fused_hash": ["zstd_encode_hash piece_scan gather"] * 3,
    "hash_beside": [_BESIDE] * 3,
    "fused_store": ["zstd_encode piece_scan gather blake3_tiles blake3_merge_big"] * 3,
    "store_incompressible": ["zstd_encode blake3_tiles blake3_merge_big store_decide piece_scan gather"] * 3,
    "blob_align_64": ["zstd_encode blake3_tiles blake3_merge_big round_pad piece_scan gather"] * 3,
    "window": ["ldm_index zstd_encode blake3_tiles blake3_merge_big piece_scan gather"] * 3,
    "tree_fused_store": ["zstd_encode piece_scan gather blake3_tiles blake3_merge_big"] * 3,    # (no round above one block: no entries)
    "tree_hash_beside": ["zstd_encode blake3_tiles blake3_merge_big block_tree_entries piece_scan gather"] * 3,
    "tree_fused_store_big": ["zstd_encode piece_scan gather blake3_tiles blake3_merge_big block_tree_entries"] * 3,
    "small_no_fuse_hash": ["zstd_encode blake3_tiles piece_scan gather"] * 3,
    "stored_no_fuse_hash": ["zstd_encode piece_scan gather blake3_tiles blake3_merge_big"] * 3,
    "small_no_fused_store": ["zstd_encode_hash piece_scan gather"] * 3,
    "stored_no_fused_store": [_BESIDE] * 3,
    "empty": [""] * 3,
    "one_empty_round": ["zstd_encode_hash piece_scan gather"] * 3,
}


def source():
    return gen.pseudo_text(TEXT, seed=61) + gen.incompressible(62, 6 * SKIP_LEN)


def run_route(ctx, d_src, rounds, opts):
    """Three queued runs on one table.  Per run: names, lagged results (copied), the blob region; tree: the last run's, or None."""
    import torch
    from znippy_amd import hip
    so, ln, sk = (np.array([r[k] for r in rounds], dt) for k, dt in ((0, np.uint64), (1, np.uint64), (2, np.uint8)))
    rt = hip.RoundTable(ctx, so, ln, sk if sk.any() else None)
    try:
        if opts.get("store_inc"):
            rt.set_store_incompressible(True)
        if opts.get("align", 1) > 1:
            rt.set_blob_align(opts["align"])
        if opts.get("emit"):
            rt.emit_block_tree()
        cap = rt.blob_bound()
        bufs = [torch.zeros(cap + 64, dtype=torch.uint8, device="cuda") for _ in range(3)]
        names, res = [], []
        take = lambda r: {k: (v.copy() if hasattr(v, "copy") else v) for k, v in r.items()}
        for k in range(3):
            rt.encode_hash_async(d_src, bufs[k], blob_cap=cap)
            names.append(" ".join(name for name, _ in ctx.kernel_times()))
            if k and rounds:
                res.append(take(rt.results_lagged(1)))
        if rounds:
            res.append(take(rt.results_lagged(0)))
            comp = rt.results()["compressed"].copy()          # (store_incompressible: which rounds the device stored)
        else:
            res, comp = [take(rt.results())] * 3, np.zeros(0, np.uint8)
        for k, r in enumerate(res):
            r["compressed"] = comp
            r["region"] = bufs[k][:int(r["blob_bytes"])].cpu().numpy()
        tree = rt.block_tree() if opts.get("emit") else None
    finally:
        rt.close()
    return names, res, tree


def digest_of(out):
    """sha256 of everything a route's three runs produced (the byte-identity record of a build)."""
    names, res, tree = out
    h = hashlib.sha256()
    for r in res:
        for k in ("region", "blob_offset", "blob_size", "checksum", "compressed"):
            h.update(np.ascontiguousarray(r[k]).tobytes())
        h.update(int(r["blob_bytes"]).to_bytes(8, "little"))
    if tree is not None:
        h.update(np.ascontiguousarray(tree).tobytes())
    return h.hexdigest()


def route_ctx(env, tier):
    """A context of the route's own: its switches, kernel timing on, its level and window."""
    from gpu_cases import make_ctx
    ctx = make_ctx(env or {})
    ctx.set_kernel_timing(2)
    if tier:
        ctx.set_level(tier[0])
        ctx.set_window_log(tier[1])
    return ctx


@pytest.fixture(scope="module")
def src(oracle):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    data = source()
    ref = {}

    def blake3(off, n):
        if (off, n) not in ref:
            ref[(off, n)] = oracle.blake3(data[off:off + n])
        return ref[(off, n)]
    return data, torch.from_numpy(np.frombuffer(data + bytes(64), np.uint8).copy()).cuda(), blake3


@pytest.mark.parametrize("name", list(ROUTES))
def test_route(src, oracle, name):
    import b3_tree
    data, d_src, blake3 = src
    key, opts, tier, env = ROUTES[name]
    rounds = ROUNDS[key]
    ctx = route_ctx(env, tier)
    try:
        names, res, tree = run_route(ctx, d_src, rounds, opts)
    finally:
        ctx.close()
    assert names == EXPECT[name], names
    want = np.stack([np.frombuffer(blake3(o, n), np.uint8) for o, n, _ in rounds]) if rounds else np.zeros((0, 32), np.uint8)
    for k, r in enumerate(res):
        assert np.array_equal(r["checksum"], want), (name, k)
        assert np.array_equal(r["region"], res[-1]["region"]), (name, k, "the runs of one table wrote different blobs")
        for q in ("blob_offset", "blob_size"):
            assert np.array_equal(r[q], res[-1][q]), (name, k, q)
    r = res[-1]
    end = 0
    for i, (o, n, skip) in enumerate(rounds):
        bo, bs = int(r["blob_offset"][i]), int(r["blob_size"][i])
        assert bo % opts.get("align", 1) == 0 and bo >= end, (name, i, bo)
        assert not r["region"][end:bo].any(), (name, i, "gap bytes")
        end = bo + bs
        f = r["region"][bo:end].tobytes()
        assert bool(r["compressed"][i]) == (not skip) or opts.get("store_inc"), (name, i)
        if r["compressed"][i]:
            assert oracle.zstd_decompress(f) == data[o:o + n], (name, i)
        else:
            assert f == data[o:o + n], (name, i)
    assert end == int(r["blob_bytes"]), name
    if tree is not None:
        ref = [b3_tree.entries(data[o:o + n]) for o, n, _ in rounds]
        assert np.array_equal(tree, np.concatenate(ref)), name
