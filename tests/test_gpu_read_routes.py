"""Every route of the read-side launch (api.hip: rows_launch; the plan: host/rows_plan.cc), pinned by its launch sequence.

Each route runs on a context of its own (its switches, kernel timing at level 2) and on ONE RowTable: four runs, each read before the
next is queued, so the table's hints are settled and the sequence is deterministic (pipelined orders: test_gpu_lean.py,
test_gpu_run_slots.py, test_gpu_run_lanes.py).  After every queue call the ordered names of Context.kernel_times() are compared with
a literal list.  The lists in EXPECT were recorded on the commit BEFORE the plan moved into the host module, so they pin that
commit's sequences, not the code's own.  Every run's rows and counters are compared with the oracle's read loop.

The routes: small_periodic (the roles kernel, lean from run 2 on), small_text (everything is handed over, then the batch path alone),
stored_only, blocks (frames of 300,001 bytes: block items on one stream from run 2 on — their short last blocks keep the block
decoder in the sequence), blocks_whole (whole blocks only: lean_blocks from run 2 on), mixed_stored (lean_mixed), foreign (the batch
path with the resolve stages), bad_row (preset runs, never lean), empty; then the switches that change a route, and the verify-only
and decode-only forms."""
import numpy as np
import pytest

import gen
import gpu_cases
import workloads

pytestmark = pytest.mark.gpu

ROLES = {"ZNIPPY_ROLES_MIN": "1"}
BASE = 64  # bad_row: the blob region starts here, and one row points in front of it
BAD = 5


def _periodic_rows(n):
    return [gpu_cases.periodic(45, 10240, 1)] * n


def _case(name):
    """(contents, frames — None: a stored row; "own": this library's encoder)."""
    z = lambda e, **kw: workloads.libzstd_compress_adv(e, level=19, **kw) if kw else workloads.libzstd_compress(e, 19)
    if name in ("small_periodic", "bad_row"):
        rows = _periodic_rows(256)
        return rows, [z(rows[0])] * 256
    if name == "small_text":
        data = gpu_cases.py_corpus(256 * 10240)
        rows = [data[i * 10240:(i + 1) * 10240] for i in range(256)]
        return rows, [z(e) for e in rows]
    if name == "stored_only":
        rows = [gen.incompressible(300 + i, 70_001 if i == 7 else 1000 + 37 * i) for i in range(64)]
        return rows, [None] * 64
    if name == "blocks":
        rows = [gen.text(300_001) if i % 2 else gen.binary(300_001) for i in range(4)]
        return rows, "own"
    if name == "blocks_whole":  # whole blocks only: the fused block kernel takes every item
        rows = [gen.text(4 * 131072) if i % 2 else gen.binary(4 * 131072) for i in range(4)]
        return rows, "own"
    if name == "mixed_stored":
        rows = _periodic_rows(128) + [gen.incompressible(70 + i, 200_000) for i in range(2)]
        return rows, [z(rows[0])] * 128 + [None] * 2
    if name in ("foreign", "foreign_ck"):
        data = gpu_cases.py_corpus(3 << 20)
        rows = [data[i * 10240:(i + 1) * 10240] for i in range(32)] + [data[2_000_000:2_000_000 + n] for n in (65_537, 131_073)] + [data[1_700_000:1_700_000 + 300_001]]
        return rows, [z(e, checksum=True) if name == "foreign_ck" else z(e) for e in rows]
    if name == "empty":
        return [], []
    raise KeyError(name)


ROUTES = {  # name: (case, environment of the context, kind of run: dv decode+verify, v verify-only, d decode-only)
    "small_periodic": ("small_periodic", ROLES, "dv"),
    "small_text": ("small_text", ROLES, "dv"),
    "stored_only": ("stored_only", {}, "dv"),
    "blocks": ("blocks", {}, "dv"),
    "blocks_whole": ("blocks_whole", {}, "dv"),
    "mixed_stored": ("mixed_stored", ROLES, "dv"),
    "foreign": ("foreign", {}, "dv"),
    "bad_row": ("bad_row", ROLES, "dv"),
    "empty": ("empty", {}, "dv"),
    "small_periodic_no_roles": ("small_periodic", dict(ROLES, ZNIPPY_NO_ROLES="1"), "dv"),
    "small_periodic_no_lean": ("small_periodic", dict(ROLES, ZNIPPY_NO_LEAN="1"), "dv"),
    "small_periodic_no_bx": ("small_periodic", dict(ROLES, ZNIPPY_NO_BX="1"), "dv"),
    "blocks_no_fused_blocks": ("blocks", {"ZNIPPY_NO_FUSED_BLOCKS": "1"}, "dv"),
    "blocks_no_block_items": ("blocks", {"ZNIPPY_NO_BLOCK_ITEMS": "1"}, "dv"),
    "blocks_no_bx": ("blocks", {"ZNIPPY_NO_BX": "1"}, "dv"),
    "foreign_no_rx": ("foreign", {"ZNIPPY_NO_RX": "1"}, "dv"),
    "foreign_no_bx": ("foreign", {"ZNIPPY_NO_BX": "1"}, "dv"),
    "foreign_checksums": ("foreign_ck", {"ZNIPPY_BX_CHECKSUM": "1"}, "dv"),
    "stored_only_no_stored_only": ("stored_only", {"ZNIPPY_NO_STORED_ONLY": "1"}, "dv"),
    "small_periodic_verify": ("small_periodic", ROLES, "v"),
    "small_periodic_decode": ("small_periodic", ROLES, "d"),
    "blocks_verify": ("blocks", {}, "v"),
    "blocks_decode": ("blocks", {}, "d"),
    "stored_only_verify": ("stored_only", {}, "v"),
    "stored_only_decode": ("stored_only", {}, "d"),
    "foreign_verify": ("foreign", {}, "v"),
    "foreign_decode": ("foreign", {}, "d"),
}

_BX_HEAD = "zstd_batch_scan zstd_batch_tables zstd_batch_sort zstd_batch_sequences_long zstd_batch_sequences zstd_batch_huffman"
_RX = "zstd_resolve_plan zstd_batch_execute zstd_resolve_expand zstd_resolve_jump zstd_resolve_store"
_BX_TAIL = "zstd_batch_finish zstd_decode_fallback"
_BX = f"{_BX_HEAD} zstd_batch_execute {_BX_TAIL}"   # the batch path, every frame executed by a wave
_BXR = f"{_BX_HEAD} {_RX} {_BX_TAIL}"               # ... big frames through the resolve stages
EXPECT = {  # recorded on the parent commit: the names after each of the four calls
    "small_periodic": [f"decode_verify_roles decode_verify_fused {_BX} blake3_second_pass verify"] + ["decode_verify_roles verify"] * 3,
    "small_text": [f"decode_verify_roles decode_verify_fused {_BX} blake3_second_pass verify"] + [f"{_BX} blake3_second_pass verify"] * 3,
    "stored_only": ["blake3_second_pass blake3_merge_big verify"] * 4,
    "blocks": [f"zstd_block_scan decode_verify_fused_blocks zstd_decode_blocks {_BXR} blake3_second_pass blake3_merge_big verify"] + ["zstd_block_scan decode_verify_fused_blocks zstd_decode_blocks zstd_decode_general zstd_decode_fallback blake3_second_pass blake3_merge_big verify"] * 3,
    "blocks_whole": [f"zstd_block_scan decode_verify_fused_blocks zstd_decode_blocks {_BXR} blake3_second_pass blake3_merge_big verify"] + ["zstd_block_scan decode_verify_fused_blocks blake3_second_pass blake3_merge_big verify"] * 3,
    "mixed_stored": [f"decode_verify_roles decode_verify_fused {_BX} blake3_second_pass blake3_merge_big verify"] + ["decode_verify_roles decode_verify_fused blake3_second_pass blake3_merge_big verify"] * 3,
    "foreign": [f"decode_verify_fused zstd_block_scan decode_verify_fused_blocks zstd_decode_blocks {_BXR} blake3_second_pass blake3_merge_big verify"] * 4,
    "bad_row": [f"decode_verify_roles decode_verify_fused {_BX} blake3_second_pass verify"] + ["decode_verify_roles decode_verify_fused zstd_decode_general blake3_second_pass verify"] * 3,
    "empty": [""] * 4,
    "small_periodic_no_roles": [f"decode_verify_fused {_BX} blake3_second_pass verify"] + ["decode_verify_fused zstd_decode_general blake3_second_pass verify"] * 3,
    "small_periodic_no_lean": [f"decode_verify_roles decode_verify_fused {_BX} blake3_second_pass verify"] + ["decode_verify_roles decode_verify_fused zstd_decode_general blake3_second_pass verify"] * 3,
    "small_periodic_no_bx": ["decode_verify_roles decode_verify_fused zstd_decode_general blake3_second_pass verify"] + ["decode_verify_roles verify"] * 3,
    "blocks_no_fused_blocks": [f"zstd_block_scan zstd_decode_blocks {_BXR} blake3_second_pass blake3_merge_big verify"] + ["zstd_block_scan zstd_decode_blocks zstd_decode_general zstd_decode_fallback blake3_second_pass blake3_merge_big verify"] * 3,
    "blocks_no_block_items": [f"{_BXR} blake3_second_pass blake3_merge_big verify"] * 4,
    "blocks_no_bx": ["zstd_block_scan decode_verify_fused_blocks zstd_decode_blocks zstd_foreign_entropy zstd_foreign_execute zstd_decode_general zstd_decode_fallback blake3_second_pass blake3_merge_big verify"] * 4,
    "foreign_no_rx": [f"decode_verify_fused zstd_block_scan decode_verify_fused_blocks zstd_decode_blocks {_BX} blake3_second_pass blake3_merge_big verify"] * 4,
    "foreign_no_bx": ["decode_verify_fused zstd_block_scan decode_verify_fused_blocks zstd_decode_blocks zstd_foreign_entropy zstd_foreign_execute zstd_decode_general zstd_decode_fallback blake3_second_pass blake3_merge_big verify"] * 4,
    "foreign_checksums": [f"decode_verify_fused zstd_block_scan decode_verify_fused_blocks zstd_decode_blocks {_BX_HEAD} {_RX} zstd_batch_checksum {_BX_TAIL} blake3_second_pass blake3_merge_big verify"] * 4,
    "stored_only_no_stored_only": ["decode_verify_fused blake3_second_pass blake3_merge_big verify"] * 4,
    "small_periodic_verify": [f"verify_roles verify_small {_BX} blake3_hash_only verify"] + ["verify_roles verify"] * 3,
    "small_periodic_decode": [f"decode_small {_BX} count_rows"] + ["decode_small zstd_decode_general count_rows"] * 3,
    "blocks_verify": [f"zstd_block_scan verify_blocks zstd_decode_blocks {_BXR} blake3_hash_only blake3_merge_big verify"] + ["zstd_block_scan verify_blocks zstd_decode_blocks zstd_decode_general zstd_decode_fallback blake3_hash_only blake3_merge_big verify"] * 3,
    "blocks_decode": [f"zstd_block_scan decode_blocks zstd_decode_blocks {_BXR} copy_stored count_rows"] + ["zstd_block_scan decode_blocks zstd_decode_blocks zstd_decode_general zstd_decode_fallback copy_stored count_rows"] * 3,
    "stored_only_verify": ["blake3_hash_only blake3_merge_big verify"] * 4,
    "stored_only_decode": ["copy_stored count_rows"] * 4,
    "foreign_verify": [f"verify_small zstd_block_scan verify_blocks zstd_decode_blocks {_BXR} blake3_hash_only blake3_merge_big verify"] * 4,
    "foreign_decode": [f"decode_small zstd_block_scan decode_blocks zstd_decode_blocks {_BXR} copy_stored count_rows"] * 4,
}


def make_cases(oracle):
    """name -> (archive, the oracle's read loop over it), built at first use and shared."""
    made, dig = {}, {}

    def blake3(e):
        if e not in dig:
            dig[e] = np.frombuffer(oracle.blake3(e), np.uint8)
        return dig[e]

    def get(name):
        if name in made:
            return made[name]
        rows, frames = _case(name)
        if frames == "own":  # this library's own frames: self-contained 128 KiB blocks
            from znippy_amd import hip
            ctx = hip.Context(0)
            by = {e: ctx.compress(e) for e in set(rows)}
            ctx.close()
            frames = [by[e] for e in rows]
        blobs = [f if f is not None else e for e, f in zip(rows, frames)]
        bs = np.array([len(b) for b in blobs], np.uint64)
        us = np.array([len(e) for e in rows], np.uint64)
        arch = dict(blobs=np.frombuffer(b"".join(blobs) + bytes(64), np.uint8).copy(), blob_offset=(np.cumsum(bs) - bs).astype(np.uint64), blob_size=bs,
                    usize=us, out_off=(np.cumsum(us) - us).astype(np.uint64), compressed=np.array([f is not None for f in frames], np.uint8),
                    checksum=np.stack([blake3(e) for e in rows]) if rows else np.zeros((0, 32), np.uint8))
        want = gpu_cases.oracle_rows(oracle, arch) if rows else (None, [], np.zeros(0, np.uint8))
        made[name] = arch, want
        return made[name]
    return get


def run_route(name, arch):
    """Four runs on one table of a context of the route's own: (names after each queue call, per run: counters, corrupt list, status,
    output bytes or None, digests or None)."""
    import torch
    from znippy_amd import hip
    case, env, kind = ROUTES[name]
    ctx = gpu_cases.make_ctx(env)
    ctx.set_kernel_timing(2)
    try:
        total = int(arch["usize"].sum())
        bad = case == "bad_row"
        base = BASE if bad else 0
        bo = arch["blob_offset"] + np.uint64(base)
        if bad:
            bo[BAD] = BASE - 1
        d_blobs = torch.from_numpy(np.concatenate([np.zeros(base, np.uint8), arch["blobs"]])).cuda()
        d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        rt = hip.RowTable(ctx, bo, arch["blob_size"], arch["usize"], arch["out_off"], np.packbits(arch["compressed"].astype(bool), bitorder="little"), arch["checksum"])
        names, res = [], []
        for _ in range(4):
            d_out.zero_()
            if kind == "dv":
                rt.decode_verify_async(d_blobs[base:] if bad else d_blobs, d_out, blob_base=base)
            elif kind == "v":
                rt.verify_async(d_blobs)
            else:
                rt.decode_async(d_blobs, d_out)
            names.append(" ".join(k for k, _ in ctx.kernel_times()))
            c, corrupt, status = rt.results()
            res.append((dict(c), sorted(int(x) for x in corrupt), status.copy(), None if kind == "v" else d_out[:total].cpu().numpy(),
                        None if kind == "d" else rt.digests().copy()))
        rt.close()
    finally:
        ctx.close()
    return names, res


def check_runs(name, arch, want, want_corrupt, want_out, res):
    """Every run's counters, verdicts, bytes and digests against the oracle's read loop."""
    n = len(arch["usize"])
    for k, (c, corrupt, status, out, dig) in enumerate(res):
        if not n:
            assert not any(c.values()) and not corrupt, (name, k, c)
            continue
        ok = np.ones(n, bool)
        if ROUTES[name][0] == "bad_row":  # the host's verdict for the one row, the oracle's for the others
            ok[BAD] = False
            assert status[BAD] < 0 and c["decode_errors"] == 1 and c["total_chunks"] == want["total_chunks"], (name, k, c)
            assert c["verified_bytes"] == want["verified_bytes"] - int(arch["usize"][BAD]) and c["corrupt_rows"] == 0, (name, k, c)
        else:
            assert c == want, (name, k, c, want)
        assert (status[ok] == 0).all() and corrupt == sorted(int(x) for x in want_corrupt) == [], (name, k)
        if out is not None:
            for i in np.nonzero(ok)[0]:
                a, b = int(arch["out_off"][i]), int(arch["out_off"][i] + arch["usize"][i])
                assert np.array_equal(out[a:b], want_out[a:b]), (name, k, int(i))
        if dig is not None:
            assert np.array_equal(dig[ok], arch["checksum"][ok]), (name, k)


@pytest.fixture(scope="module")
def cases(oracle):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return make_cases(oracle)


@pytest.mark.parametrize("name", list(ROUTES))
def test_route(cases, name):
    arch, (want, want_corrupt, want_out) = cases(ROUTES[name][0])
    names, res = run_route(name, arch)
    assert names == EXPECT[name], names
    check_runs(name, arch, want, want_corrupt, want_out, res)


# ---- the tile plan behind a run of equal rows ---------------------------------------------------------------------------------------

def _run_tail_rows():
    """Runs of equal rows that end exactly on a whole tile (64 // leaves rows, twice) with a one-leaf row behind each: where 64 leaves
    are not used up (6, 10 and 21 leaves per row) that row joins the run's last tile, as the unit-by-unit rule has it; at 1 and 32
    leaves the tile is full and the row opens the next."""
    rows = []
    for leaves in (1, 6, 10, 21, 32):
        rows += [gen.pseudo_text(leaves * 1024, seed=leaves)] * (2 * (64 // leaves)) + [gen.pseudo_text(700, seed=100 + leaves)]
    return rows


@pytest.mark.parametrize("stored", [False, True], ids=["compressed", "stored"])
@pytest.mark.parametrize("env", [{}, ROLES], ids=["default", "roles_min_1"])
def test_rows_behind_a_run_that_ends_on_a_whole_tile(oracle, env, stored):
    import torch
    from znippy_amd import hip
    rows = _run_tail_rows()
    by = {e: (None if stored else workloads.libzstd_compress(e, 3)) for e in set(rows)}
    blobs = [by[e] if by[e] is not None else e for e in rows]
    bs = np.array([len(b) for b in blobs], np.uint64)
    us = np.array([len(e) for e in rows], np.uint64)
    dig = {e: np.frombuffer(oracle.blake3(e), np.uint8) for e in set(rows)}
    arch = dict(blobs=np.frombuffer(b"".join(blobs) + bytes(64), np.uint8).copy(), blob_offset=(np.cumsum(bs) - bs).astype(np.uint64), blob_size=bs, usize=us,
                out_off=(np.cumsum(us) - us).astype(np.uint64), compressed=np.full(len(rows), 0 if stored else 1, np.uint8), checksum=np.stack([dig[e] for e in rows]))
    want, want_corrupt, want_out = gpu_cases.oracle_rows(oracle, arch)
    ctx = gpu_cases.make_ctx(env)
    try:
        rt = None
        for rep in range(2):    # (the second run goes by the first one's hints)
            counters, corrupt, status, out, rt = gpu_cases.run_gpu(ctx, arch, rt=rt)
            assert counters == want and len(corrupt) == 0 and (status == 0).all(), (rep, counters, want)
            assert np.array_equal(out, want_out) and np.array_equal(rt.digests(), arch["checksum"]), rep
        rt.close()
        # the write side hashes over the same plan
        d_src = torch.from_numpy(np.frombuffer(b"".join(rows) + bytes(64), np.uint8).copy()).cuda()
        wt = hip.RoundTable(ctx, arch["out_off"], us, None)
        assert np.array_equal(wt.hash(d_src), arch["checksum"])
        wt.close()
    finally:
        ctx.close()
