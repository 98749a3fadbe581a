"""The ring of the role-split read kernel (csrc/fused_small.hip: one loader wave and R_WAVES - 1 hasher waves around
R_SLOTS slots in groups of four) at the tile counts where its geometry matters, against the oracle's restated read loop
(decompress.rs:L135-190): bytes, digests, counters, corrupt rows and per-row status.  Through ONE workgroup
(ZNIPPY_LDS_PAD=1 caps the grid) 7, 8, 15, 16, 17 and 33 tiles: one round of seven hashers and one more, the sixteen-slot
ring less one, the ring, the ring and one more (the first refill of a group), two rings and one; through TWO workgroups
that share the cursor (ZNIPPY_LDS_PAD=2) 9 and 35 tiles with a tile of another shape in the middle, both loaders closing
with empty groups.  Rows of six different periods and literal prefixes in one tile, the order rotated from tile to tile:
what a descriptor kept per row must get right and a tile of equal rows hides — with one damaged literal byte in such a
tile, and two consecutive asynchronous runs of one table with the run lanes on and off.  Every row has content of its own,
so that a digest written to the wrong row shows; every table runs as a decode + verify run (k_fused_roles<true>) and as a
verify-only run (k_fused_roles<false>).  Whether libzstd wrote a row in the shape the kernel recognises (one compressed
block: raw literals and one sequence, within the staged window) is checked here on the CPU, frame by frame; the kernel's
name is asserted for the tables in which every row has it."""
import numpy as np
import pytest

from gpu_cases import build_archive, make_ctx, run_gpu

pytestmark = pytest.mark.gpu

ROW = 10240
WIN, WSTRIDE = 512, 608   # csrc/fused_small.hip: bytes of a frame that are staged, and a row's window


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


def _tiles(n, seed0=0):
    return _plain(6 * n, seed0)


def _with_other_shape(n):
    """n tiles in all: seven 9 KiB rows (a full tile of their own) in the middle of plain 6 x 10 tiles."""
    front = (n - 1) // 2
    return _tiles(front) + _plain(7, 5000, 9216) + _tiles(n - 1 - front, 1000)


PERIODS = [1, 3, 45, 64, 65, 960]
PREFIXES = [0, 19, 64, 1000, 1024, 1030]
# the same, with every row's literals inside the staged window
PERIODS_IN = [2, 3, 45, 64, 65, 200]
PREFIXES_IN = [0, 19, 64, 100, 200, 250]


def _mixed(periods, prefixes, seed0=0):
    """Three tiles of six rows: row i of tile r has period i and prefix (i + 2 r) mod 6."""
    return [_row(periods[i], seed0 + 10 * r + i, prefix=prefixes[(i + 2 * r) % 6]) for r in range(3) for i in range(6)]


def recognised(frame, usize):
    """Is this zstd frame of the shape parse_fast takes: a single-segment or windowed frame without checksum or dictionary,
    one block — compressed, the last — with raw literals and exactly one sequence, frame and literals within the window?"""
    f = bytes(frame)
    n = len(f)
    if n < 12 or n > WIN or f[:4] != b"\x28\xb5\x2f\xfd":
        return False
    fhd = f[4]
    if fhd & 0x0F:
        return False
    single, fcs_flag = (fhd >> 5) & 1, fhd >> 6
    fcs_bytes = single if fcs_flag == 0 else 1 << fcs_flag
    if not fcs_bytes:
        return False
    pos = 6 - single
    fcs = int.from_bytes(f[pos:pos + fcs_bytes], "little") + (256 if fcs_bytes == 2 else 0)
    if fcs != usize:
        return False
    pos += fcs_bytes
    bh = int.from_bytes(f[pos:pos + 3], "little")
    if (bh & 7) != 5 or pos + 3 + (bh >> 3) != n:   # last block, compressed, ends the frame
        return False
    pos += 3
    lh = int.from_bytes(f[pos:pos + 3], "little")
    if lh & 3:
        return False
    sf = (lh >> 2) & 3
    regen = (lh & 0xFF) >> 3 if sf & 1 == 0 else ((lh & 0xFFFF) >> 4 if sf == 1 else lh >> 4)
    lit_at = pos + (1 if sf & 1 == 0 else (2 if sf == 1 else 3))
    sp = lit_at + regen
    return regen >= 1 and sp + 3 <= n and f[sp] == 1 and lit_at + regen + 64 <= WSTRIDE


# name -> rows
TABLES = {
    "mixed": lambda: _mixed(PERIODS, PREFIXES),
    "mixed_in_window": lambda: _mixed(PERIODS_IN, PREFIXES_IN, 500),
}
ONE_WORKGROUP = [7, 8, 15, 16, 17, 33]
TWO_WORKGROUPS = [9, 35]


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (archive, the oracle's counters, corrupt list and bytes, every row is of the recognised shape): built on
    first use, shared by both kinds of run."""
    made = {}

    def get(name, rows, mutate=None):
        if name not in made:
            arch = build_archive(oracle, rows(), level=19)
            n = len(arch["usize"])
            shape = all(bool(arch["compressed"][i]) and
                        recognised(arch["blobs"][int(arch["blob_offset"][i]):int(arch["blob_offset"][i] + arch["blob_size"][i])],
                                   int(arch["usize"][i])) for i in range(n))
            if mutate:
                mutate(arch)
            bitmap = np.packbits(arch["compressed"].astype(bool), bitorder="little")
            want_out = np.zeros(int(arch["usize"].sum()), dtype=np.uint8)
            want, want_corrupt = oracle.decompress_rows(arch["blobs"], arch["blob_offset"], arch["blob_size"], arch["usize"],
                                                        arch["out_off"], bitmap, arch["checksum"], 0, n, out=want_out)
            made[name] = (arch, want, [int(x) for x in want_corrupt], want_out, shape)
        return made[name]

    return get


def _decode(ctx, case):
    arch, want, want_corrupt, want_out, _ = case
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
    arch, want, want_corrupt, _, _ = case
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


def _through(n_workgroups, run, kernel, case):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = make_ctx({"ZNIPPY_ROLES_MIN": "1", "ZNIPPY_LDS_PAD": str(n_workgroups)})
    try:
        status, digests, names = run(ctx, case)
    finally:
        ctx.close()
    assert (status == 0).all()
    assert np.array_equal(digests, case[0]["checksum"])
    assert kernel in names
    return names


@pytest.mark.parametrize("kind", list(RUNS))
@pytest.mark.parametrize("tiles", ONE_WORKGROUP)
def test_through_one_workgroup(cases, tiles, kind):
    run, kernel = RUNS[kind]
    case = cases(f"one_{tiles}", lambda: _tiles(tiles, 37 * tiles))
    assert case[4], "libzstd did not write these rows as raw literals and one sequence"
    assert len(case[0]["usize"]) == 6 * tiles
    _through(1, run, kernel, case)


@pytest.mark.parametrize("kind", list(RUNS))
@pytest.mark.parametrize("tiles", TWO_WORKGROUPS)
def test_through_two_workgroups_sharing_the_cursor(cases, tiles, kind):
    """Both workgroups publish empty closing groups; a tile of seven 9 KiB rows sits in the middle."""
    run, kernel = RUNS[kind]
    case = cases(f"two_{tiles}", lambda: _with_other_shape(tiles))
    _through(2, run, kernel, case)


@pytest.mark.parametrize("kind", list(RUNS))
@pytest.mark.parametrize("name", list(TABLES))
def test_periods_and_prefixes_inside_one_tile(gpu_ctx_roles, cases, name, kind):
    run, kernel = RUNS[kind]
    case = cases(name, TABLES[name])
    if name == "mixed_in_window":
        assert case[4], "every row of this table was chosen to be of the recognised shape"
    status, digests, names = run(gpu_ctx_roles, case)
    assert (status == 0).all()
    assert np.array_equal(digests, case[0]["checksum"])
    if case[4]:
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
def test_one_damaged_literal_byte_in_a_mixed_tile(gpu_ctx_roles, cases, kind):
    """Exactly the damaged row is reported: its five neighbours of other periods and both other tiles verify."""
    run, kernel = RUNS[kind]
    case = cases("mixed_damaged", lambda: _mixed(PERIODS_IN, PREFIXES_IN, 900), mutate=_flip_a_literal)
    arch, want, want_corrupt, _, shape = case
    assert want_corrupt == [BAD_ROW] and want["corrupt_rows"] == 1
    status, digests, names = run(gpu_ctx_roles, case)
    assert (status == 0).all()
    good = np.ones(18, bool)
    good[BAD_ROW] = False
    assert np.array_equal(digests[good], arch["checksum"][good])
    assert not np.array_equal(digests[BAD_ROW], arch["checksum"][BAD_ROW])
    if shape:
        assert kernel in names


@pytest.mark.parametrize("lanes", ["run_lanes", "no_run_lanes"])
def test_two_consecutive_async_runs(cases, lanes):
    """17 tiles, two runs in flight (decode_verify_async twice, results_lagged): counters and digests as the oracle's, with
    the run lanes and with every run in queue order on the main stream."""
    import torch
    from znippy_amd import hip
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    arch, want, want_corrupt, want_out, shape = cases("one_17", lambda: _tiles(17, 37 * 17))
    env = {"ZNIPPY_ROLES_MIN": "1"}
    if lanes == "no_run_lanes":
        env["ZNIPPY_NO_RUN_LANES"] = "1"
    ctx = make_ctx(env)
    try:
        d_blobs = torch.from_numpy(np.concatenate([arch["blobs"], np.zeros(32, np.uint8)])).cuda()
        total = int(arch["usize"].sum())
        d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        bitmap = np.packbits(arch["compressed"].astype(bool), bitorder="little")
        rt = hip.RowTable(ctx, arch["blob_offset"], arch["blob_size"], arch["usize"], arch["out_off"], bitmap, arch["checksum"])
        for _ in range(2):   # (the first run of a table is never lean: the pair below is)
            rt.decode_verify_async(d_blobs, d_out)
            assert rt.results_lagged(0) == want
        d_out.zero_()
        rt.decode_verify_async(d_blobs, d_out)
        rt.decode_verify_async(d_blobs, d_out)
        assert rt.results_lagged(1) == want
        assert rt.results_lagged(0) == want
        counters, corrupt, status = rt.results()
        assert counters == want and [int(x) for x in corrupt] == want_corrupt and (status == 0).all()
        assert np.array_equal(rt.digests(), arch["checksum"])
        ctx.sync()
        assert np.array_equal(d_out.cpu().numpy()[:total], want_out)
        print("lane counters", ctx.run_lane_stats())
        rt.close()
    finally:
        ctx.close()
