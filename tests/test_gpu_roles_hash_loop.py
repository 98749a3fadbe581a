"""The 6 x 10 hash loop of the role-split read kernel (csrc/fused_small.hip, roles_hash_6x10: two passes per iteration
over two message sets, the previous tile's parent tree riding in lanes 60..63 with its levels read from a table, the
leaf chaining values left in the wave's node array by the last pass) against the oracle's restated read loop
(decompress.rs:L135-190): bytes, digests, counters, corrupt rows and per-row status, on the smallest tables at which
the loop can go wrong — one to three tiles (flush only / one ride / a ride and a flush), a tile of another shape in
between, more tiles than ring slots through one workgroup, periods around the 64-byte block and at the recogniser's
limit, literals that end inside a block, on a block boundary and around the first leaf boundary, one damaged row.
Every row has content of its own, so that a digest written to the wrong row shows; every table runs as a decode +
verify run (k_fused_roles<true>) and as a verify-only run (k_fused_roles<false>)."""
import numpy as np
import pytest

from gpu_cases import build_archive, make_ctx, run_gpu

pytestmark = pytest.mark.gpu

ROW = 10240


def _row(period, seed, size=ROW, prefix=0):
    """`prefix` random bytes, then a random pattern of `period` bytes repeated to `size`; short patterns differ by seed."""
    rng = np.random.default_rng(100_003 * period + 7 * prefix + seed)
    pre = rng.integers(0, 256, size=prefix, dtype=np.uint8).tobytes()
    pat = bytearray(rng.integers(0, 256, size=period, dtype=np.uint8).tobytes())
    if period < 4:
        pat[0] = (17 * seed + period) % 256
    pat = bytes(pat)
    return (pre + pat * ((size - prefix) // period + 1))[:size]


def _plain(n, seed0=0, size=ROW):
    return [_row(45, seed0 + i, size) for i in range(n)]


PERIODS = [1, 3, 45, 63, 64, 65, 127, 128, 129, 959, 960]
PREFIXES = [0, 19, 64, 1000, 1024, 1030]

# name -> (rows, every tile is a plain 6 x 10 tile of the recognised shape)
TABLES = {
    "tiles_1": (lambda: _plain(6), True),                                     # the tree is only flushed, never rides
    "tiles_2": (lambda: _plain(12), True),                                    # one ride, then the flush
    "tiles_2_and_one_row": (lambda: _plain(13), False),                       # the flush comes after a tile of another shape
    "tiles_3": (lambda: _plain(18), True),
    # the issue's rows (the planner packs 64 leaves: the 9 KiB rows share their tile with the first 10 KiB row behind them) ...
    "other_shape_between": (lambda: _plain(6) + _plain(6, 50, 9216) + _plain(6, 100), False),
    # ... and seven 9 KiB rows, a full tile of their own, so that the tiles in front and behind are both 6 x 10
    "full_other_tile_between": (lambda: _plain(6) + _plain(7, 50, 9216) + _plain(6, 100), False),
    "periods": (lambda: [_row(p, i) for p in PERIODS for i in range(6)], False),
    "prefixes": (lambda: [_row(45, i, prefix=q) for q in PREFIXES for i in range(6)], False),
}


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (archive, the oracle's counters, corrupt list and bytes): built on first use, shared by both kinds of run."""
    made = {}

    def get(name, rows=None, mutate=None):
        if name not in made:
            arch = build_archive(oracle, rows() if rows else TABLES[name][0](), level=19)
            if mutate:
                mutate(arch)
            n = len(arch["usize"])
            bitmap = np.packbits(arch["compressed"].astype(bool), bitorder="little")
            want_out = np.zeros(int(arch["usize"].sum()), dtype=np.uint8)
            want, want_corrupt = oracle.decompress_rows(arch["blobs"], arch["blob_offset"], arch["blob_size"], arch["usize"],
                                                        arch["out_off"], bitmap, arch["checksum"], 0, n, out=want_out)
            made[name] = (arch, want, [int(x) for x in want_corrupt], want_out)
        return made[name]

    return get


def _decode(ctx, case):
    arch, want, want_corrupt, want_out = case
    counters, corrupt, status, out, rt = run_gpu(ctx, arch, pad_blobs=3)
    names = [k for k, _ in ctx.kernel_times()]
    assert counters == want
    assert [int(x) for x in corrupt] == want_corrupt
    assert np.array_equal(out, want_out)
    digests = rt.digests().copy()
    rt.close()
    return status, digests, names


def _verify(ctx, case):
    import torch
    from znippy_amd import hip
    arch, want, want_corrupt, _ = case
    d_blobs = torch.from_numpy(np.concatenate([arch["blobs"], np.zeros(32, np.uint8)])).cuda()
    bitmap = np.packbits(arch["compressed"].astype(bool), bitorder="little")
    rt = hip.RowTable(ctx, arch["blob_offset"], arch["blob_size"], arch["usize"], arch["out_off"], bitmap, arch["checksum"])
    counters, corrupt, status = rt.verify(d_blobs)
    names = [k for k, _ in ctx.kernel_times()]
    assert counters == want
    assert [int(x) for x in corrupt] == want_corrupt
    status, digests = status.copy(), rt.digests().copy()
    rt.close()
    return status, digests, names


RUNS = {"decode": (_decode, "decode_verify_roles"), "verify_only": (_verify, "verify_roles")}


@pytest.mark.parametrize("kind", list(RUNS))
@pytest.mark.parametrize("name", list(TABLES))
def test_table(gpu_ctx_roles, cases, name, kind):
    run, kernel = RUNS[kind]
    case = cases(name)
    status, digests, names = run(gpu_ctx_roles, case)
    assert (status == 0).all()
    assert np.array_equal(digests, case[0]["checksum"])
    if TABLES[name][1]:
        assert kernel in names


@pytest.mark.parametrize("kind", list(RUNS))
def test_more_tiles_than_ring_slots_through_one_workgroup(cases, kind):
    """40 tiles through the 32 slots of ONE workgroup (ZNIPPY_LDS_PAD=1 caps the grid): every hasher wave rides trees
    from tile to tile and every slot group is refilled."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    run, kernel = RUNS[kind]
    case = cases("tiles_40", rows=lambda: _plain(240))
    ctx = make_ctx({"ZNIPPY_ROLES_MIN": "1", "ZNIPPY_LDS_PAD": "1"})
    try:
        status, digests, names = run(ctx, case)
    finally:
        ctx.close()
    assert (status == 0).all()
    assert np.array_equal(digests, case[0]["checksum"])
    assert kernel in names


BAD_ROW = 6 + 2   # third row of the second of three tiles


def _flip_a_literal(arch):
    """One byte of row BAD_ROW's literals (the row's first bytes stand in its frame as they are) is flipped."""
    a, n = int(arch["blob_offset"][BAD_ROW]), int(arch["blob_size"][BAD_ROW])
    frame = arch["blobs"][a:a + n].tobytes()
    o = int(arch["out_off"][BAD_ROW])
    head = arch["src"][o:o + 16].tobytes()
    at = frame.find(head)
    assert at > 0, "the row's literals are not stored raw"
    blobs = arch["blobs"].copy()
    blobs[a + at + 5] ^= 0x20
    arch["blobs"] = blobs


@pytest.mark.parametrize("kind", list(RUNS))
def test_one_damaged_literal_byte(gpu_ctx_roles, cases, kind):
    """Exactly the damaged row is reported: its five neighbours and both other tiles verify; counters as the oracle's."""
    run, kernel = RUNS[kind]
    case = cases("damaged", rows=lambda: _plain(18, 300), mutate=_flip_a_literal)
    arch, want, want_corrupt, _ = case
    assert want_corrupt == [BAD_ROW] and want["corrupt_rows"] == 1
    status, digests, names = run(gpu_ctx_roles, case)
    assert (status == 0).all()
    good = np.ones(18, bool)
    good[BAD_ROW] = False
    assert np.array_equal(digests[good], arch["checksum"][good])
    assert not np.array_equal(digests[BAD_ROW], arch["checksum"][BAD_ROW])
    assert kernel in names
