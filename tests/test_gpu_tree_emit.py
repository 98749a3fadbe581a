"""Block tree from the write side (znippy_rounds_emit_block_tree / _block_tree_layout / _block_tree): the entries the encode +
hash run leaves, made from the hash's own 64-leaf tile chaining values.

The reference is tests/b3_tree.py — BLAKE3 in numpy, nothing of the library — and, for the rounds too long for it, the read
side's producer (RowTable.build_block_tree, an independent kernel that test_gpu_block_tree.py pins to b3_tree) plus the
authentication of znippy_rows_set_block_tree.  The entries depend on the source bytes alone, so every hash route, level and
setting has to give the same ones."""
import ctypes as C
import os

import numpy as np
import pytest

import b3_tree
import gen

pytestmark = pytest.mark.gpu

BLK = 128 * 1024
LENS = [0, 1, 10240, 65536, 65537, 131072, 131073, 196608, 196609, 262144, 262145, 300001]
HALF = 320_000


def require_api():
    from znippy_amd import _lib
    L = _lib.lib()
    for name in ("znippy_rounds_emit_block_tree", "znippy_rounds_block_tree_layout", "znippy_rounds_block_tree"):
        assert hasattr(L, name), name
    return L


class Source:
    """One staging buffer and a reference cache keyed by (offset, length)."""

    def __init__(self, oracle, data):
        self.oracle, self.data = oracle, data
        self.np = np.frombuffer(data + bytes(64), np.uint8).copy()
        self._dev, self._ref = None, {}

    def dev(self):
        import torch
        if self._dev is None:
            self._dev = torch.from_numpy(self.np).cuda()
        return self._dev

    def ref(self, off, n):
        if (off, n) not in self._ref:
            d = self.data[off:off + n]
            assert len(d) == n
            self._ref[(off, n)] = (b3_tree.entries(d), self.oracle.blake3(d))
        return self._ref[(off, n)]

    def tree(self, rounds):
        parts = [self.ref(o, n)[0] for o, n, _ in rounds]
        return np.concatenate(parts) if parts else np.zeros((0, 32), np.uint8)

    def digests(self, rounds):
        return np.stack([np.frombuffer(self.ref(o, n)[1], np.uint8) for o, n, _ in rounds])


def table(ctx, rounds):
    from znippy_amd import hip
    so, ln, sk = (np.array([r[k] for r in rounds], dt) for k, dt in ((0, np.uint64), (1, np.uint64), (2, np.uint8)))
    return hip.RoundTable(ctx, so, ln, sk if sk.any() else None)


def run(ctx, src, rounds, emit=True, align=1, shift=0, store_inc=False):
    """One run on a new table: dict(tree, results copied, region, names)."""
    import torch
    rt = table(ctx, rounds)
    try:
        if store_inc:
            rt.set_store_incompressible(True)
        if align > 1:
            rt.set_blob_align(align)
        if emit:
            rt.emit_block_tree()
        bound = rt.blob_bound()
        buf = torch.zeros(shift + bound + 64, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        enc = rt.encode_hash(src.dev(), buf[shift:], blob_cap=bound)
        names = [k for k, _ in ctx.kernel_times()]
        out = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in enc.items()}
        out["names"] = names
        out["region"] = buf[shift:shift + int(enc["blob_bytes"])].cpu().numpy()
        out["layout"] = rt.block_tree_layout()
        out["tree"] = rt.block_tree() if emit else None
    finally:
        rt.close()
    return out


def check_tree(src, rounds, out, what):
    n, first = out["layout"]
    assert np.array_equal(first, b3_tree.row_first([r[1] for r in rounds])), what
    ref = src.tree(rounds)
    assert n == ref.shape[0] and out["tree"].shape == ref.shape, (what, n, ref.shape)
    if not np.array_equal(out["tree"], ref):
        k = int(np.nonzero((out["tree"] != ref).any(axis=1))[0][0])
        raise AssertionError((what, "first differing entry", k, "round", int(np.searchsorted(first, k, side="right")) - 1))
    assert np.array_equal(out["checksum"], src.digests(rounds)), what
    for i, (o, ln, _) in enumerate(rounds):  # the entries chain to the checksum the same run returned
        e = out["tree"][int(first[i]):int(first[i + 1])]
        if len(e):
            assert b3_tree.digest_from_entries(e) == out["checksum"][i].tobytes(), (what, i)


# ---- small lengths -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small(oracle):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    require_api()
    src = Source(oracle, gen.pseudo_text(HALF, seed=11) + gen.incompressible(12, HALF))
    rounds = []
    for i, n in enumerate(LENS):
        rounds.append((1000 * i, n, 0))                 # text, encoded; the rounds overlap each other
        rounds.append((HALF + 777 * i, n, i & 1))       # incompressible, stored and encoded in turn
    rounds += [(250_000, 140_000, 0),                   # across the border of the two halves
               (0, 300_001, 1), (0, 300_001, 0),        # the same bytes stored and encoded
               (HALF, 131_073, 1), (HALF, 131_073, 1)]  # the same round twice
    return src, rounds


def test_small_lengths(gpu_ctx, small):
    src, rounds = small
    out = run(gpu_ctx, src, rounds)
    stored = sum(n for _, n, s in rounds if s)
    assert stored * 2 < sum(n for _, n, _ in rounds)    # (the hash runs beside the encoder)
    assert "block_tree_entries" in out["names"], out["names"]
    assert out["names"].index("block_tree_entries") == out["names"].index("blake3_merge_big") + 1
    check_tree(src, rounds, out, "small")
    one = src.ref(HALF + 777 * 6, 131_073)[0]           # 131,073 bytes: the second entry is one 1-byte chunk
    assert one.shape == (2, 32)
    # all stored: the store path's kernel, and each round alone: a list of one unit
    flipped = [(o, n, 1) for o, n, _ in rounds]
    check_tree(src, flipped, run(gpu_ctx, src, flipped), "small, all stored")
    for r in [(3000, 196_608, 1), (HALF, 131_073, 0), (0, 131_072, 0)]:
        check_tree(src, [r], run(gpu_ctx, src, [r]), ("alone", r))


# ---- every hash route ----------------------------------------------------------------------------------------------------------

ROUTE_SPANS = [(HALF, 8 * 65536 + 1), (HALF + 600_000, 300_001), (HALF + 100, 196_608), (HALF + 5, 131_073), (HALF + 900_000, 70_000),
               (0, 5_000), (1_000, 140_000), (7, 300_001), (HALF + 3 * 65536, 4 * 65536)]
STORED_FIRST = 5  # the first five spans are the incompressible half


def route_rounds(stored):
    return [(o, n, 1 if stored and i < STORED_FIRST else 0) for i, (o, n) in enumerate(ROUTE_SPANS)]


@pytest.fixture(scope="module")
def route(oracle):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    require_api()
    src = Source(oracle, gen.pseudo_text(HALF, seed=21) + gen.incompressible(22, 1_000_000))
    return src, src.tree(route_rounds(False))


def env_ctx(env):
    from znippy_amd import hip
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return hip.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


ROUTES = [  # name, stored rounds, run options, level, window_log, environment of a context of its own
    ("mixed", False, {}, None, 0, None),
    ("store_shift", True, dict(align=1), None, 0, None),
    ("store_shift_odd_base", True, dict(align=1, shift=3), None, 0, None),
    ("store_aligned_wg_fold", True, dict(align=128), None, 0, None),
    ("store_g_2", True, dict(align=128), None, 0, {"ZNIPPY_STORE_G": "2"}),
    ("store_incompressible", True, dict(store_inc=True), None, 0, None),
    ("store_incompressible_mixed", False, dict(store_inc=True), None, 0, None),
    ("level_3", False, {}, 3, 0, None),
    ("level_19", False, {}, 19, 0, None),
    ("level_19_window_17", False, {}, 19, 17, None),
    ("level_19_window_17_stored", True, dict(align=16), 19, 17, None),
]


@pytest.mark.parametrize("name,stored,opts,level,window_log,env", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_hash_route(gpu_ctx, route, name, stored, opts, level, window_log, env):
    src, first_case = route
    rounds = route_rounds(stored)
    if stored:  # store-heavy: the hash kernel copies what it hashes; the first round's 8 whole slices fill two workgroups
        assert sum(n for _, n, s in rounds if s) * 2 >= sum(n for _, n, _ in rounds)
    ctx = env_ctx(env) if env else gpu_ctx
    old = (ctx.level, ctx.window_log)
    try:
        if level is not None:
            ctx.set_level(level)
            ctx.set_window_log(window_log)
        out = run(ctx, src, rounds, **opts)
    finally:
        if env:
            ctx.close()
        else:
            ctx.set_level(old[0])
            ctx.set_window_log(old[1])
    check_tree(src, rounds, out, name)
    assert np.array_equal(out["tree"], first_case), name
    if opts.get("store_inc"):
        assert not out["compressed"][:STORED_FIRST].any(), (name, out["compressed"])


# ---- merge routes --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("skip", [1, 0], ids=["stored", "encoded"])
@pytest.mark.parametrize("n", [(4 << 20) + BLK + 5, (16 << 20) + 70_000], ids=["65_tile_cvs", "258_tile_cvs"])
def test_merge_routes(gpu_ctx, n, skip):
    import torch
    from znippy_amd import hip
    require_api()
    assert -(-n // 65536) in (67, 258)  # more than 64 tile CVs / more than 256: k_merge_units / k_merge_groups + k_merge_big
    mib = gen.pseudo_text(1 << 20, seed=31)
    data = np.concatenate([np.frombuffer(mib * 3, np.uint8), np.random.default_rng(32).integers(0, 256, n - (3 << 20) + 64, dtype=np.uint8)])
    d_src = torch.from_numpy(data).cuda()
    # the reference: the same bytes as one stored row, entries by the read side's producer, digest checked by its fold
    one = np.array([n], np.uint64)
    rt = table(gpu_ctx, [(0, n, skip)])
    rt.emit_block_tree()
    d_blob = torch.zeros(rt.blob_bound() + 64, dtype=torch.uint8, device="cuda")
    enc = rt.encode_hash(d_src, d_blob)
    names = [k for k, _ in gpu_ctx.kernel_times()]
    ck, bs, bo = enc["checksum"].copy(), enc["blob_size"].copy(), enc["blob_offset"].copy()
    tree = rt.block_tree()
    assert rt.block_tree_layout()[0] == -(-n // BLK) == tree.shape[0]
    rt.close()
    assert "block_tree_entries" in names
    stored = hip.RowTable(gpu_ctx, np.zeros(1, np.uint64), one, one, None, np.zeros(1, np.uint8), ck)
    ref, status = stored.build_block_tree(d_src, blob_cap=n)
    stored.close()
    assert (status == 0).all(), status  # (the producer's entries fold to the checksum the encode run returned)
    assert np.array_equal(tree, ref), int(np.nonzero((tree != ref).any(axis=1))[0][0])
    rows = hip.RowTable(gpu_ctx, bo, bs, one, np.zeros(1, np.uint64), np.array([0 if skip else 1], np.uint8), ck)
    assert (rows.set_block_tree(tree) == 0).all()
    bad = tree.copy()
    bad[-1, 5] ^= 1
    assert rows.set_block_tree(bad)[0] != 0
    rows.close()


# ---- end to end: the emitted tree serves verified range reads ---------------------------------------------------------------------

def test_end_to_end_verified_ranges(gpu_ctx, route):
    import torch
    from znippy_amd import hip
    src, _ = route
    for stored in (True, False):
        rounds = route_rounds(stored)
        out = run(gpu_ctx, src, rounds, align=16 if stored else 1)
        lens = np.array([r[1] for r in rounds], np.uint64)
        oo = (np.cumsum(lens) - lens).astype(np.uint64)
        rows = hip.RowTable(gpu_ctx, out["blob_offset"], out["blob_size"], lens, oo, np.packbits(out["compressed"].astype(bool), bitorder="little"),
                            out["checksum"])
        assert (rows.set_block_tree(out["tree"]) == 0).all()
        begins = np.array([max(0, n - 5000) for _, n, _ in rounds], np.uint64)
        rl = np.minimum(lens - begins, 4096).astype(np.uint64)
        want_hashed = 0
        for (_, n, _), b, m in zip(rounds, begins, rl):
            b, m = int(b), int(m)
            if n <= BLK:
                want_hashed += n                         # at most one block: verified whole
            else:
                want_hashed += sum(min(BLK, n - k * BLK) for k in range(b // BLK, (b + m - 1) // BLK + 1))
        d_blobs = torch.from_numpy(np.concatenate([out["region"], np.zeros(64, np.uint8)])).cuda()
        d_out = torch.zeros(int(rl.sum()) + 64, dtype=torch.uint8, device="cuda")
        status, decoded, hashed = rows.read_ranges_verified(d_blobs, np.arange(len(rounds)), begins, rl, d_out, blob_cap=len(out["region"]))
        rows.close()
        assert (status == 0).all(), (stored, status)
        got = d_out[:int(rl.sum())].cpu().numpy().tobytes()
        assert got == b"".join(src.data[o + int(b):o + int(b) + int(m)] for (o, _, _), b, m in zip(rounds, begins, rl)), stored
        assert hashed == want_hashed, (stored, hashed, want_hashed)


# ---- tables without entries -----------------------------------------------------------------------------------------------------

def test_table_without_entries(gpu_ctx, oracle):
    require_api()
    sizes = [0, 1, 100, 5000, 10240, 7000] * 8
    src = Source(oracle, gen.pseudo_text(60_000, seed=41))
    rounds = [(37 * i, n, 0) for i, n in enumerate(sizes)]
    plain = run(gpu_ctx, src, rounds, emit=False)
    out = run(gpu_ctx, src, rounds)
    assert "zstd_encode_hash" in out["names"]  # (the encoder hashes these rounds itself: no merge, nothing to make entries from)
    assert out["names"] == plain["names"] and "block_tree_entries" not in out["names"]
    assert out["layout"][0] == 0 and not out["layout"][1].any()
    assert out["tree"].shape == (0, 32)
    for k in ("blob_offset", "blob_size", "checksum", "compressed", "region"):
        assert np.array_equal(out[k], plain[k]), k
    assert out["blob_bytes"] == plain["blob_bytes"]
    assert np.array_equal(out["checksum"], src.digests(rounds))
    # rounds of exactly one block, and big rounds of exactly two tiles, have none either
    rounds = [(0, 131_072, 0), (5, 65_537, 1), (9, 131_072, 1)]
    src = Source(oracle, gen.pseudo_text(140_000, seed=42))
    out = run(gpu_ctx, src, rounds)
    assert out["layout"][0] == 0 and out["tree"].shape == (0, 32) and "block_tree_entries" not in out["names"]
    assert np.array_equal(out["checksum"], src.digests(rounds))


# ---- two runs in flight ------------------------------------------------------------------------------------------------------------

def test_two_runs_in_flight(gpu_ctx, oracle, route):
    import torch
    src, _ = route
    other = Source(oracle, gen.pseudo_text(HALF, seed=51) + gen.incompressible(52, 1_000_000))
    for stored in (False, True):
        rounds = route_rounds(stored)
        want = {id(src): src.tree(rounds), id(other): other.tree(rounds)}
        assert not np.array_equal(want[id(src)], want[id(other)])
        rt = table(gpu_ctx, rounds)
        rt.emit_block_tree()
        cap = rt.blob_bound()
        bufs = [torch.zeros(cap + 64, dtype=torch.uint8, device="cuda") for _ in range(3)]
        rt.encode_hash_async(src.dev(), bufs[0], blob_cap=cap)
        rt.encode_hash_async(other.dev(), bufs[1], blob_cap=cap)
        assert np.array_equal(rt.block_tree(lag=1), want[id(src)]), stored
        assert np.array_equal(rt.block_tree(lag=0), want[id(other)]), stored
        rt.encode_hash_async(src.dev(), bufs[2], blob_cap=cap)   # the third run reuses the first slot
        assert np.array_equal(rt.block_tree(lag=0), want[id(src)]), stored
        assert np.array_equal(rt.block_tree(lag=1), want[id(other)]), stored
        assert np.array_equal(rt.results_lagged(0)["checksum"], src.digests(rounds))
        assert np.array_equal(rt.results_lagged(1)["checksum"], other.digests(rounds))
        rt.close()


# ---- switching ---------------------------------------------------------------------------------------------------------------------

def test_switching(gpu_ctx, route):
    import torch
    from znippy_amd._lib import E_INVAL, ZnippyError
    src, first_case = route
    for stored in (False, True):
        rounds = route_rounds(stored)
        never = run(gpu_ctx, src, rounds, emit=False)
        assert "block_tree_entries" not in never["names"]
        rt = table(gpu_ctx, rounds)
        rt.emit_block_tree(True)
        rt.emit_block_tree(False)
        cap = rt.blob_bound()
        bufs = [torch.zeros(cap + 64, dtype=torch.uint8, device="cuda") for _ in range(2)]
        enc = rt.encode_hash(src.dev(), bufs[0], blob_cap=cap)
        assert [k for k, _ in gpu_ctx.kernel_times()] == never["names"]
        for k in ("blob_offset", "blob_size", "checksum", "compressed"):
            assert np.array_equal(enc[k], never[k]), k
        assert int(enc["blob_bytes"]) == never["blob_bytes"]
        assert np.array_equal(bufs[0][:never["blob_bytes"]].cpu().numpy(), never["region"])
        with pytest.raises(ZnippyError) as e:
            rt.block_tree()
        assert e.value.code == E_INVAL
        assert rt.block_tree_layout()[0] == first_case.shape[0]   # the layout does not need the switch
        # switched on between two queued runs: only the later one has a tree
        rt.encode_hash_async(src.dev(), bufs[0], blob_cap=cap)
        rt.emit_block_tree(True)
        rt.encode_hash_async(src.dev(), bufs[1], blob_cap=cap)
        rt.emit_block_tree(False)                                   # neither queued run sees this
        with pytest.raises(ZnippyError) as e:
            rt.block_tree(lag=1)
        assert e.value.code == E_INVAL
        assert np.array_equal(rt.block_tree(lag=0), first_case)
        with pytest.raises(ZnippyError) as e:
            rt.block_tree(lag=2)
        assert e.value.code == E_INVAL
        rt.close()


def test_invalid_arguments(gpu_ctx, route):
    import torch
    from znippy_amd import _lib, hip
    from znippy_amd._lib import E_INVAL
    L = require_api()
    src, first_case = route
    rounds = route_rounds(False)
    rt = table(gpu_ctx, rounds)
    n, first = C.c_uint64(), np.zeros(len(rounds) + 1, np.uint64)
    buf = np.zeros((first_case.shape[0], 32), np.uint8)
    assert L.znippy_rounds_emit_block_tree(None, 1) == E_INVAL
    assert L.znippy_rounds_block_tree_layout(None, rt.h, C.byref(n), None) == E_INVAL
    assert L.znippy_rounds_block_tree_layout(gpu_ctx.h, None, C.byref(n), None) == E_INVAL
    assert L.znippy_rounds_block_tree_layout(gpu_ctx.h, rt.h, None, _lib.np_ptr(first)) == E_INVAL
    assert L.znippy_rounds_block_tree_layout(gpu_ctx.h, rt.h, C.byref(n), None) == 0 and n.value == first_case.shape[0]
    assert L.znippy_rounds_block_tree(gpu_ctx.h, rt.h, 0, _lib.np_ptr(buf)) == E_INVAL          # no run yet
    rt.emit_block_tree()
    d_blob = torch.zeros(rt.blob_bound() + 64, dtype=torch.uint8, device="cuda")
    rt.encode_hash(src.dev(), d_blob)
    assert L.znippy_rounds_block_tree(None, rt.h, 0, _lib.np_ptr(buf)) == E_INVAL
    assert L.znippy_rounds_block_tree(gpu_ctx.h, None, 0, _lib.np_ptr(buf)) == E_INVAL
    assert L.znippy_rounds_block_tree(gpu_ctx.h, rt.h, 0, None) == E_INVAL                      # entries, and nowhere to put them
    assert L.znippy_rounds_block_tree(gpu_ctx.h, rt.h, 1, _lib.np_ptr(buf)) == E_INVAL          # one run only
    assert L.znippy_rounds_block_tree(gpu_ctx.h, rt.h, 2, _lib.np_ptr(buf)) == E_INVAL
    other = hip.Context(0)                                                                       # a table of another context
    assert L.znippy_rounds_block_tree(other.h, rt.h, 0, _lib.np_ptr(buf)) == E_INVAL
    assert L.znippy_rounds_block_tree_layout(other.h, rt.h, C.byref(n), None) == E_INVAL
    other.close()
    assert L.znippy_rounds_block_tree(gpu_ctx.h, rt.h, 0, _lib.np_ptr(buf)) == 0 and np.array_equal(buf, first_case)
    rt.close()
    # a closed context (destroyed while a table keeps it alive)
    h, r = C.c_void_p(), C.c_void_p()
    assert L.znippy_ctx_create(0, None, C.byref(h)) == 0
    one = np.array([0], np.uint64), np.array([300_001], np.uint64)
    assert L.znippy_rounds_create(h, _lib.np_ptr(one[0]), _lib.np_ptr(one[1]), None, 1, C.byref(r)) == 0
    L.znippy_ctx_destroy(h)
    assert L.znippy_rounds_emit_block_tree(r, 1) == E_INVAL
    assert L.znippy_rounds_block_tree_layout(h, r, C.byref(n), None) == E_INVAL
    assert L.znippy_rounds_block_tree(h, r, 0, _lib.np_ptr(buf)) == E_INVAL
    L.znippy_rounds_destroy(r)
