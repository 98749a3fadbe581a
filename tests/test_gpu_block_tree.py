"""Block tree (znippy_rows_block_tree_build / _set_block_tree) and range reads verified block by block against the row
checksum (znippy_rows_read_ranges_verified).

The reference is tests/b3_tree.py — BLAKE3 in numpy, nothing of the library — and the oracle's digests.  Which route a row
took shows in hashed_bytes / decoded_bytes, figures worked out from the geometry alone; output regions carry a sentinel, so
a byte written for a range that failed shows."""
import ctypes as C

import numpy as np
import pytest

import b3_tree
import gen
import test_gpu_ranges as tr
from gpu_cases import foreign_archive
from range_checks import verified_and_check

pytestmark = pytest.mark.gpu

BLK = 128 * 1024
SENTINEL = tr.SENTINEL
HIGH_BASE = (1 << 40) + 12345
TREE_LENGTHS = [131_073, 132_096, 132_097, 262_144, 262_145, 300_001, 655_361, 8_388_609, 5_000, 131_072]


def digests(oracle, rows):
    return np.stack([np.frombuffer(oracle.blake3(r), np.uint8) for r in rows])


def stored_table(ctx, rows, ck, base=0):
    """Stored rows, row i's blob at a source alignment of i % 16."""
    from znippy_amd import hip
    bo, parts, cur = [], [], 0
    for i, r in enumerate(rows):
        pad = (i % 16 - cur) % 16
        parts += [bytes(pad), r]
        bo.append(cur + pad)
        cur += pad + len(r)
    bs = np.array([len(r) for r in rows], np.uint64)
    rt = hip.RowTable(ctx, np.array(bo, np.uint64) + np.uint64(base), bs, bs, None, np.zeros((len(rows) + 7) // 8, np.uint8), ck)
    d_blobs = tr.to_dev(b"".join(parts))
    assert d_blobs.data_ptr() % 16 == 0
    return rt, d_blobs, np.array(bo, np.uint64)


# ---- 1. build == reference, byte for byte ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tree_rows(oracle):
    mib = gen.pseudo_text(1 << 20, seed=70)
    rows = [gen.pseudo_text(n, seed=60 + i) if n != 8_388_609 else mib * 8 + b"!" for i, n in enumerate(TREE_LENGTHS)]
    a, b, c = (gen.pseudo_text(BLK, seed=80 + i) for i in range(3))
    rows.append(a + b + b + c)                                   # blocks 1 and 2 identical: only the chunk counter tells their entries apart
    ref = b3_tree.table_tree(rows)
    twins = b3_tree.entries(rows[-1])
    assert bytes(twins[1]) != bytes(twins[2])
    return dict(rows=rows, ref=ref, ck=digests(oracle, rows), frames={level: tr.own_frames(level, rows) for level in (3, 19)})


def check_build(rt, d_blobs, rows, ref, base):
    n, first = rt.block_tree_layout()
    assert np.array_equal(first, b3_tree.row_first([len(r) for r in rows])) and n == ref.shape[0]
    tree, status = rt.build_block_tree(d_blobs, blob_base=base)
    assert (status == 0).all(), status
    assert tree.shape == ref.shape
    if not np.array_equal(tree, ref):
        k = int(np.nonzero((tree != ref).any(axis=1))[0][0])
        raise AssertionError(("first differing entry", k, "row", int(np.searchsorted(first, k, side="right")) - 1))
    return tree


@pytest.mark.parametrize("level", [3, 19])
@pytest.mark.parametrize("base", [0, HIGH_BASE], ids=["base0", "far_base"])
def test_build_own_frames(gpu_ctx, tree_rows, level, base):
    T = tree_rows
    rt, d_blobs, _ = tr.table_of(gpu_ctx, T["frames"][level], T["rows"], checksum=T["ck"], base=base)
    check_build(rt, d_blobs, T["rows"], T["ref"], base)
    names = set(dict(gpu_ctx.kernel_times()))
    assert {"block_tree_cvs", "block_tree_fold"} <= names, sorted(names)
    rt.close()
    # a table without a checksum column: the same entries, nothing compared
    rt, d_blobs, _ = tr.table_of(gpu_ctx, T["frames"][level], T["rows"], checksum=None, base=base)
    check_build(rt, d_blobs, T["rows"], T["ref"], base)
    assert "block_tree_fold" not in dict(gpu_ctx.kernel_times())
    rt.close()


@pytest.fixture(scope="module")
def stored_rows(oracle):
    rows = [gen.incompressible(20 + i, 300_001) for i in range(16)]
    return dict(rows=rows, ref=b3_tree.table_tree(rows), ck=digests(oracle, rows))


@pytest.mark.parametrize("base", [0, HIGH_BASE], ids=["base0", "far_base"])
def test_build_stored_rows_at_every_alignment(gpu_ctx, stored_rows, base):
    S = stored_rows
    rt, d_blobs, bo = stored_table(gpu_ctx, S["rows"], S["ck"], base)
    assert sorted(int(x) % 16 for x in bo) == list(range(16))
    check_build(rt, d_blobs, S["rows"], S["ref"], base)
    rt.close()


@pytest.fixture(scope="module")
def foreign_rows(oracle):
    rows = [gen.pseudo_text(300_001, seed=3), gen.pseudo_text(200_000, seed=4), gen.pseudo_text(131_072, seed=5)]
    return dict(rows=rows, A=foreign_archive(oracle, rows, 19), ref=b3_tree.table_tree(rows))


@pytest.mark.parametrize("base", [0, HIGH_BASE], ids=["base0", "far_base"])
def test_build_foreign_frames(gpu_ctx, foreign_rows, base):
    from znippy_amd import hip
    F = foreign_rows
    A = F["A"]
    rt = hip.RowTable(gpu_ctx, A["bo"] + np.uint64(base), A["bs"], A["us"], A["oo"], None, A["ck"])
    check_build(rt, tr.to_dev(A["blobs"]), F["rows"], F["ref"], base)
    rt.close()


def test_build_reports_bad_rows(gpu_ctx, oracle):
    from znippy_amd import _lib, hip
    rows = [gen.pseudo_text(300_001, seed=90 + i) for i in range(4)]
    frames = tr.own_frames(3, rows)
    ck = digests(oracle, rows)
    ck[1, 7] ^= 0x10                                             # row 1: a wrong checksum
    bs = np.array([len(f) for f in frames], np.uint64)
    bo = (np.cumsum(bs) - bs).astype(np.uint64)
    bs[2] -= 1                                                   # row 2: a truncated frame
    us = np.array([len(r) for r in rows], np.uint64)
    d_blobs = tr.to_dev(b"".join(frames))
    plain = hip.RowTable(gpu_ctx, bo, bs, us, (np.cumsum(us) - us).astype(np.uint64), None, None)
    _, want = plain.decode(d_blobs, tr.sentinel(int(us.sum()) + 64))
    want = want.copy()
    plain.close()
    assert want[2] < 0 and want[2] != _lib.E_DIGEST
    rt = hip.RowTable(gpu_ctx, bo, bs, us, None, None, ck)
    blob_cap = int(bo[3] + bs[3]) - 1                            # row 3: its blob ends one byte outside the region
    tree, status = rt.build_block_tree(d_blobs, blob_cap=blob_cap)
    assert list(status) == [0, _lib.E_DIGEST, want[2], _lib.E_CORRUPT], status
    ref = b3_tree.entries(rows[0])
    assert np.array_equal(tree[:3], ref) and not tree[3:].any()
    rt.close()


# ---- 2. set authenticates ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def auth_rows(oracle):
    sizes = [300_001, 262_145, 262_144, 5_000, 655_361]
    rows = [gen.pseudo_text(n, seed=100 + i) for i, n in enumerate(sizes)]
    return dict(sizes=sizes, rows=rows, frames=tr.own_frames(3, rows), ck=digests(oracle, rows), tree=b3_tree.table_tree(rows),
                first=b3_tree.row_first(sizes))


def one_range(rt, d_blobs, rows, row, begin, n):
    """One verified range: (status, decoded, hashed), its bytes checked when the status is 0."""
    region = tr.sentinel(n + 64)
    status, decoded, hashed = rt.read_ranges_verified(d_blobs, [row], [begin], [n], region, out_offsets=[32])
    got = region.cpu().numpy()
    assert (got[:32] == SENTINEL).all() and (got[32 + n:] == SENTINEL).all()
    if status[0] == 0:
        assert got[32:32 + n].tobytes() == rows[row][begin:begin + n]
    else:
        assert (got == SENTINEL).all()
    return int(status[0]), decoded, hashed


def test_set_authenticates(gpu_ctx, auth_rows):
    from znippy_amd import _lib
    R = auth_rows
    rows, first = R["rows"], R["first"]
    rt, d_blobs, _ = tr.table_of(gpu_ctx, R["frames"], rows, checksum=R["ck"])
    # a tree the library never saw: every row accepted, and a range costs one block
    assert (rt.set_block_tree(R["tree"]) == 0).all()
    for row in (0, 1, 2, 4):
        assert one_range(rt, d_blobs, rows, row, BLK + 100, 4096) == (0, min(BLK, R["sizes"][row] - BLK), min(BLK, R["sizes"][row] - BLK))
    # one flipped bit in one entry rejects exactly that row, which is then verified whole
    bad = R["tree"].copy()
    bad[int(first[4]) + 3, 31] ^= 0x80
    assert list(rt.set_block_tree(bad)) == [0, 0, 0, 0, _lib.E_DIGEST]
    assert one_range(rt, d_blobs, rows, 4, BLK + 100, 4096) == (0, 655_361, 655_361)
    assert one_range(rt, d_blobs, rows, 0, BLK + 100, 4096) == (0, BLK, BLK)
    # two swapped entries of a row
    bad = R["tree"].copy()
    bad[[int(first[0]), int(first[0]) + 1]] = bad[[int(first[0]) + 1, int(first[0])]]
    assert list(rt.set_block_tree(bad)) == [_lib.E_DIGEST, 0, 0, 0, 0]
    # another row's entries of equal count (rows 0 and 1 have three each)
    bad = R["tree"].copy()
    bad[int(first[0]):int(first[1])], bad[int(first[1]):int(first[2])] = R["tree"][int(first[1]):int(first[2])], R["tree"][int(first[0]):int(first[1])]
    assert list(rt.set_block_tree(bad)) == [_lib.E_DIGEST, _lib.E_DIGEST, 0, 0, 0]
    # the library's own tree is accepted; None removes it
    built, status = rt.build_block_tree(d_blobs)
    assert (status == 0).all() and np.array_equal(built, R["tree"])
    assert (rt.set_block_tree(built) == 0).all()
    assert one_range(rt, d_blobs, rows, 1, 5, 100) == (0, BLK, BLK)
    assert (rt.set_block_tree(None) == 0).all()
    assert one_range(rt, d_blobs, rows, 1, 5, 100) == (0, 262_145, 262_145)
    rt.close()
    rt, d_blobs, _ = tr.table_of(gpu_ctx, R["frames"], rows, checksum=None)
    with pytest.raises(_lib.ZnippyError) as e:
        rt.set_block_tree(R["tree"])
    assert e.value.code == _lib.E_INVAL
    with pytest.raises(_lib.ZnippyError) as e:
        rt.read_ranges_verified(d_blobs, [0], [0], [1], tr.sentinel(64))
    assert e.value.code == _lib.E_INVAL
    rt.close()


# ---- 3. verified reads return the unverified call's bytes -----------------------------------------------------------------

@pytest.fixture(scope="module")
def own_rows(oracle):
    rows = [gen.pseudo_text(n, seed=40 + i) for i, n in enumerate(tr.ROW_SIZES[:-1])] + [tr.mixed(tr.ROW_SIZES[-1], seed=9)]
    return dict(rows=rows, frames={level: tr.own_frames(level, rows) for level in (3, 19)}, ck=digests(oracle, rows), tree=b3_tree.table_tree(rows))


@pytest.mark.parametrize("level", [3, 19])
@pytest.mark.parametrize("base", [0, HIGH_BASE], ids=["base0", "far_base"])
def test_verified_reads_on_own_frames(gpu_ctx, own_rows, level, base):
    O = own_rows
    rows = O["rows"]
    rt, d_blobs, _ = tr.table_of(gpu_ctx, O["frames"][level], rows, checksum=O["ck"], base=base)
    assert (rt.set_block_tree(O["tree"]) == 0).all()
    ranges = tr.boundary_ranges(tr.ROW_SIZES)
    all_bytes = sum(tr.ROW_SIZES)
    assert tr.expected_decoded(ranges, tr.ROW_SIZES) == all_bytes
    kw = dict(blob_base=base)
    verified_and_check(rt, d_blobs, rows, ranges, ("in order", level), want=(all_bytes, all_bytes), **kw)
    names = set(dict(gpu_ctx.kernel_times()))
    assert {"range_scan", "range_decode_blocks", "range_verify_blocks", "range_decode_rows", "range_copy"} <= names, sorted(names)
    shuffled = [ranges[i] for i in np.random.default_rng(level).permutation(len(ranges))]
    verified_and_check(rt, d_blobs, rows, shuffled, ("shuffled", level), guard=1, want=(all_bytes, all_bytes), **kw)
    verified_and_check(rt, d_blobs, rows, shuffled, ("shuffled, packed", level), guard=64, packed=True, want=(all_bytes, all_bytes), **kw)
    few = [(4, 300_000, 1), (4, 262_144, 5), (2, 131_072, 1), (0, 17, 3)]
    work = (300_001 - 2 * BLK) + 1 + 5_000
    verified_and_check(rt, d_blobs, rows, few, ("few", level), want=(work, work), **kw)
    # the unverified call on the same table is what it was
    tr.read_and_check(rt, d_blobs, rows, ranges, ("unverified", level), want_decoded=all_bytes, **kw)
    assert "range_verify_blocks" not in dict(gpu_ctx.kernel_times())
    rt.close()


def test_one_range_hashes_one_block(gpu_ctx, oracle):
    row = gen.pseudo_text(1 << 20, seed=77)
    rt, d_blobs, _ = tr.table_of(gpu_ctx, tr.own_frames(19, [row]), [row], checksum=digests(oracle, [row]))
    assert (rt.set_block_tree(b3_tree.entries(row)) == 0).all()
    verified_and_check(rt, d_blobs, [row], [(0, 3 * BLK + 1000, 4096)], "inside block 3", want=(BLK, BLK))
    names = set(dict(gpu_ctx.kernel_times()))
    assert "range_decode_rows" not in names and {"range_decode_blocks", "range_verify_blocks"} <= names, sorted(names)
    verified_and_check(rt, d_blobs, [row], [(0, 4 * BLK - 2048, 4096)], "blocks 3 and 4", want=(2 * BLK, 2 * BLK))
    rt.close()


@pytest.mark.parametrize("base", [0, HIGH_BASE], ids=["base0", "far_base"])
def test_verified_reads_on_stored_rows(gpu_ctx, oracle, stored_rows, base):
    S = stored_rows
    small = [gen.incompressible(50, 5_000), gen.incompressible(51, 131_072)]
    rows = S["rows"][:3] + small
    ck = np.concatenate([S["ck"][:3], digests(oracle, small)])
    rt, d_blobs, _ = stored_table(gpu_ctx, rows, ck, base)
    assert (rt.set_block_tree(S["ref"][:9]) == 0).all()
    sizes = [len(r) for r in rows]
    ranges = tr.boundary_ranges(sizes)
    verified_and_check(rt, d_blobs, rows, ranges, "all of it", want=(0, sum(sizes)), blob_base=base)
    few = [(0, 300_000, 1), (1, 131_071, 2), (2, 5, 9), (2, 100, 50), (3, 1, 1)]
    verified_and_check(rt, d_blobs, rows, few, "few", guard=3, want=(0, (300_001 - 2 * BLK) + 2 * BLK + BLK + 5_000), blob_base=base)
    rt.close()


# ---- 4. substitution is caught, and only where a range looks -------------------------------------------------------------

SUB_LEN = 3 * BLK + 5_001
SUB_AT = [2 * BLK, 3 * BLK - 1, SUB_LEN - 1]                     # first and last byte of block 2, the row's last byte in a ragged tail


@pytest.fixture(scope="module")
def sub_rows(oracle):
    rows = [gen.pseudo_text(SUB_LEN, seed=120), gen.pseudo_text(262_145, seed=121)]
    altered = []
    for at in SUB_AT:
        x = bytearray(rows[0])
        x[at] ^= 0x21
        altered.append(bytes(x))
    return dict(rows=rows, altered=altered, frames=tr.own_frames(19, rows + altered), ck=digests(oracle, rows), tree=b3_tree.table_tree(rows))


def sub_ranges(at):
    bad_block = at // BLK
    ranges = [(0, at, 1), (0, at - 3000, min(4096, SUB_LEN - (at - 3000))), (0, bad_block * BLK - 10, 20)]
    good = [(0, 5, 4096), (0, BLK - 1, 2), (1, BLK, 300)] + [(0, k * BLK + 77, 1000) for k in range(4) if k != bad_block and k * BLK + 1077 <= SUB_LEN]
    return ranges, good


def check_substitution(rt, d_blobs, rows, actual, at):
    from znippy_amd import _lib
    bad, good = sub_ranges(at)
    ranges = bad + good
    lens = np.array([n for _, _, n in ranges], np.uint64)
    offs = (np.cumsum(lens) - lens).astype(np.uint64) + np.uint64(16)
    args = ([r for r, _, _ in ranges], [b for _, b, _ in ranges], lens)
    region = tr.sentinel(int(lens.sum()) + 64)
    status, _ = rt.read_ranges(d_blobs, *args, region, out_offsets=offs)
    assert (status == 0).all()                                   # the unverified call vouches for nothing: it returns the other content
    got = region.cpu().numpy()
    assert got[16] == actual[at] != rows[0][at]
    region = tr.sentinel(int(lens.sum()) + 64)
    status, _, _ = rt.read_ranges_verified(d_blobs, *args, region, out_offsets=offs)
    assert list(status) == [_lib.E_DIGEST] * len(bad) + [0] * len(good), status
    expect = np.full(int(lens.sum()) + 64, SENTINEL, np.uint8)
    for (row, begin, n), o in list(zip(ranges, offs))[len(bad):]:
        expect[int(o):int(o) + n] = np.frombuffer(rows[row][begin:begin + n], np.uint8)
    assert np.array_equal(region.cpu().numpy(), expect)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["block2_first", "block2_last", "ragged_last"])
def test_substituted_frame(gpu_ctx, sub_rows, which):
    S = sub_rows
    frames = [S["frames"][2 + which], S["frames"][1]]            # a valid frame of this encoder, of a content that differs in one byte
    rt, d_blobs, _ = tr.table_of(gpu_ctx, frames, S["rows"], checksum=S["ck"])
    assert (rt.set_block_tree(S["tree"]) == 0).all()
    check_substitution(rt, d_blobs, S["rows"], S["altered"][which], SUB_AT[which])
    rt.close()


@pytest.mark.parametrize("which", [0, 1, 2], ids=["block2_first", "block2_last", "ragged_last"])
def test_flipped_byte_of_a_stored_row(gpu_ctx, oracle, which):
    rows = [gen.incompressible(130, SUB_LEN), gen.incompressible(131, 262_145)]
    rt, d_blobs, bo = stored_table(gpu_ctx, rows, digests(oracle, rows))
    assert (rt.set_block_tree(b3_tree.table_tree(rows)) == 0).all()
    d_blobs[int(bo[0]) + SUB_AT[which]] ^= 0x21
    actual = bytearray(rows[0])
    actual[SUB_AT[which]] ^= 0x21
    check_substitution(rt, d_blobs, rows, bytes(actual), SUB_AT[which])
    rt.close()


# ---- 5. the whole route -------------------------------------------------------------------------------------------------------

def whole_route(gpu_ctx, rows, frames, ck, tag, install):
    """Rows the call decodes whole: verified whole with the right bytes; with a wrong checksum every range of the row fails."""
    from znippy_amd import _lib
    sizes = [len(r) for r in rows]
    ranges = tr.fallback_ranges(sizes)
    rt, d_blobs, _ = tr.table_of(gpu_ctx, frames, rows, checksum=ck)
    if install:
        assert (rt.set_block_tree(b3_tree.table_tree(rows)) == 0).all()
    verified_and_check(rt, d_blobs, rows, ranges, tag, want=(sum(sizes), sum(sizes)))
    rt.close()
    wrong = ck.copy()
    wrong[0, 0] ^= 1
    rt, d_blobs, _ = tr.table_of(gpu_ctx, frames, rows, checksum=wrong)
    if install:
        assert list(rt.set_block_tree(b3_tree.table_tree(rows))) == [_lib.E_DIGEST] + [0] * (len(rows) - 1)
    lens = np.array([n for _, _, n in ranges], np.uint64)
    region = tr.sentinel(int(lens.sum()) + 64)
    status, decoded, hashed = rt.read_ranges_verified(d_blobs, [r for r, _, _ in ranges], [b for _, b, _ in ranges], lens, region)
    want = [_lib.E_DIGEST if row == 0 and n else 0 for row, _, n in ranges]
    assert list(status) == want, (tag, status)
    got = region.cpu().numpy()
    at = 0
    for (row, begin, n), st in zip(ranges, want):
        piece = got[at:at + n]
        assert (piece == SENTINEL).all() if st else piece.tobytes() == rows[row][begin:begin + n], (tag, row, begin)
        at += n
    assert (got[at:] == SENTINEL).all()
    rt.close()


def test_whole_route_without_accepted_entries(gpu_ctx, auth_rows):
    R = auth_rows
    whole_route(gpu_ctx, R["rows"][:2], R["frames"][:2], R["ck"][:2], "no tree", install=False)


def test_whole_route_foreign_frames(gpu_ctx, foreign_rows):
    F = foreign_rows
    whole_route(gpu_ctx, F["rows"][:2], F["A"]["frames"][:2], F["A"]["ck"][:2], "libzstd -19", install=True)


def test_whole_route_window_frames(gpu_ctx, oracle):
    rows = [gen.incompressible(8, 100_000) * 3, gen.pseudo_text(50_000, seed=6) * 6]
    whole_route(gpu_ctx, rows, tr.own_frames(19, rows, window_log=17), digests(oracle, rows), "window 17", install=True)


def test_whole_route_late_rows(gpu_ctx, oracle):
    cases = tr.synth_frames()
    rows, frames = [c for c, _ in cases], [f for _, f in cases]
    ck = digests(oracle, rows)
    rt, d_blobs, _ = tr.table_of(gpu_ctx, frames, rows, checksum=ck)
    assert (rt.set_block_tree(b3_tree.table_tree(rows)) == 0).all()
    verified_and_check(rt, d_blobs, rows, [(0, 1_000, 4096), (1, 70_500, 100)], "block 0", want=(2 * BLK, 2 * BLK))   # by blocks
    assert "range_decode_rows_late" not in dict(gpu_ctx.kernel_times())
    verified_and_check(rt, d_blobs, rows, [(0, BLK + 50, 4096), (1, 2 * BLK - 1, 1)], "block 1", want=(4 * BLK, 4 * BLK))
    assert "range_decode_rows_late" in dict(gpu_ctx.kernel_times())
    rt.close()
    whole_route(gpu_ctx, rows, frames, ck, "late", install=False)


def test_damaged_frame_keeps_its_decode_code(gpu_ctx, oracle):
    from znippy_amd import _lib, hip
    rows = [gen.pseudo_text(300_001, seed=140), gen.pseudo_text(300_001, seed=141)]
    frames = tr.own_frames(19, rows)
    bs = np.array([len(frames[0]), len(frames[1]) - 1], np.uint64)   # row 1: cut by one byte
    bo = np.array([0, len(frames[0])], np.uint64)
    us = np.array([300_001, 300_001], np.uint64)
    d_blobs = tr.to_dev(b"".join(frames))
    plain = hip.RowTable(gpu_ctx, bo, bs, us, np.array([0, 300_001], np.uint64), None, None)
    _, want = plain.decode(d_blobs, tr.sentinel(600_002 + 64))
    want = want.copy()
    plain.close()
    assert want[1] < 0 and want[1] != _lib.E_DIGEST
    rt = hip.RowTable(gpu_ctx, bo, bs, us, None, None, digests(oracle, rows))
    for tree in (None, b3_tree.table_tree(rows)):
        rt.set_block_tree(tree)
        region = tr.sentinel(1024)
        status, _, _ = rt.read_ranges_verified(d_blobs, [0, 1], [100, 2 * BLK + 5], [300, 300], region)
        assert list(status) == [0, want[1]], status
        got = region.cpu().numpy()
        assert got[:300].tobytes() == rows[0][100:400] and (got[300:] == SENTINEL).all()
    rt.close()


# ---- 6. validation and "not a run" -------------------------------------------------------------------------------------------

def test_validation_on_the_host(gpu_ctx, oracle):
    from znippy_amd import _lib, hip
    rows = [gen.pseudo_text(300_001, seed=31), gen.incompressible(2, 1000), gen.pseudo_text(9_000, seed=32)]
    frames = tr.own_frames(3, [rows[0]]) + [rows[1]] + tr.own_frames(3, [rows[2]])
    bs = np.array([len(f) for f in frames], np.uint64)
    bo = (np.cumsum(bs) - bs).astype(np.uint64)
    us = np.array([len(r) for r in rows], np.uint64)
    rt = hip.RowTable(gpu_ctx, bo, bs, us, None, np.packbits(np.array([1, 0, 1], bool), bitorder="little"), digests(oracle, rows))
    assert (rt.set_block_tree(b3_tree.table_tree(rows)) == 0).all()
    d_blobs = tr.to_dev(b"".join(frames))
    blob_cap = int(bo[2]) + int(bs[2]) - 1                      # the last row's blob ends one byte outside
    good = [(0, 200_000, 777), (1, 10, 99)]
    cases = [((3, 0, 1), _lib.E_INVAL), ((0, 300_000, 2), _lib.E_INVAL), ((0, 5, (1 << 64) - 3), _lib.E_INVAL),
             ((0, 300_002, 0), _lib.E_INVAL), ((1, 0, 50), _lib.E_DST_SMALL), ((2, 0, 10), _lib.E_CORRUPT)]
    cap = 4000
    for (row, begin, n), code in cases:
        region = tr.sentinel(cap + 64)
        at = cap - 20 if code == _lib.E_DST_SMALL else 2000
        status, decoded, hashed = rt.read_ranges_verified(d_blobs, [good[0][0], row, good[1][0]], [good[0][1], begin, good[1][1]],
                                                          [good[0][2], n, good[1][2]], region, out_offsets=[1, at, 1000], out_cap=cap, blob_cap=blob_cap)
        assert list(status) == [0, code, 0], ((row, begin, n), status)
        want = np.full(cap + 64, SENTINEL, np.uint8)
        want[1:778] = np.frombuffer(rows[0][200_000:200_777], np.uint8)
        want[1000:1099] = np.frombuffer(rows[1][10:109], np.uint8)
        assert np.array_equal(region.cpu().numpy(), want), (row, begin, n)
        assert (decoded, hashed) == (BLK, BLK + 1000)
    # ranges without bytes verify nothing
    region = tr.sentinel(64)
    status, decoded, hashed = rt.read_ranges_verified(d_blobs, [0, 1], [300_001, 0], [0, 0], region, blob_cap=blob_cap)
    assert list(status) == [0, 0] and (decoded, hashed) == (0, 0) and bool((region == SENTINEL).all().item())
    rt.close()


def test_abi_arguments(gpu_ctx, oracle):
    import torch
    from znippy_amd import _lib
    L = _lib.lib()
    E = _lib.E_INVAL
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    raw = gen.incompressible(3, 300_001)
    d = tr.to_dev(raw)
    out = tr.sentinel(256)
    dp, op = C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr())
    bitmap = (C.c_uint8 * 1)(0)
    ck = (C.c_uint8 * 32).from_buffer_copy(oracle.blake3(raw))
    rows, bare = C.c_void_p(), C.c_void_p()
    assert L.znippy_rows_create(gpu_ctx.h, u64(0), u64(300_001), bitmap, u64(300_001), None, ck, 0, 1, C.byref(rows)) == 0
    assert L.znippy_rows_create(gpu_ctx.h, u64(0), u64(300_001), bitmap, u64(300_001), None, None, 0, 1, C.byref(bare)) == 0
    st = (C.c_int32 * 2)(7, 7)
    dec, hsh, n = C.c_uint64(99), C.c_uint64(99), C.c_uint64(99)
    first = u64(9, 9)
    tree = (C.c_uint8 * 96)()
    read = lambda ctx, t, blobs, rr, rb, rl, k, o: L.znippy_rows_read_ranges_verified(ctx, t, blobs, 0, rr, rb, rl, None, k, o, 256, st, C.byref(dec), C.byref(hsh))
    assert read(None, rows, dp, u64(0), u64(0), u64(4), 1, op) == E
    assert read(gpu_ctx.h, None, dp, u64(0), u64(0), u64(4), 1, op) == E
    assert read(gpu_ctx.h, rows, None, u64(0), u64(0), u64(4), 1, op) == E
    assert read(gpu_ctx.h, rows, dp, None, u64(0), u64(4), 1, op) == E
    assert read(gpu_ctx.h, rows, dp, u64(0), None, u64(4), 1, op) == E
    assert read(gpu_ctx.h, rows, dp, u64(0), u64(0), None, 1, op) == E
    assert read(gpu_ctx.h, rows, dp, u64(0), u64(0), u64(4), 1, None) == E
    assert read(gpu_ctx.h, bare, dp, u64(0), u64(0), u64(4), 1, op) == E                         # no checksum column
    assert read(gpu_ctx.h, rows, None, None, None, None, 0, None) == 0 and (dec.value, hsh.value) == (0, 0)   # no ranges
    assert bool((out == SENTINEL).all().item())
    assert L.znippy_rows_block_tree_layout(None, rows, C.byref(n), first) == E
    assert L.znippy_rows_block_tree_layout(gpu_ctx.h, None, C.byref(n), first) == E
    assert L.znippy_rows_block_tree_layout(gpu_ctx.h, rows, None, first) == E
    assert L.znippy_rows_block_tree_layout(gpu_ctx.h, rows, C.byref(n), None) == 0 and n.value == 3
    assert L.znippy_rows_block_tree_layout(gpu_ctx.h, rows, C.byref(n), first) == 0 and list(first) == [0, 3]
    assert L.znippy_rows_block_tree_build(None, rows, dp, 0, tree, st) == E
    assert L.znippy_rows_block_tree_build(gpu_ctx.h, None, dp, 0, tree, st) == E
    assert L.znippy_rows_block_tree_build(gpu_ctx.h, rows, None, 0, tree, st) == E
    assert L.znippy_rows_block_tree_build(gpu_ctx.h, rows, dp, 0, None, st) == E
    assert L.znippy_rows_block_tree_build(gpu_ctx.h, rows, dp, 0, tree, None) == 0               # the status is optional
    assert bytes(tree) == b3_tree.entries(raw).tobytes()
    assert L.znippy_rows_block_tree_build(gpu_ctx.h, bare, dp, 0, tree, st) == 0 and st[0] == 0  # works without a checksum column
    assert L.znippy_rows_set_block_tree(None, rows, tree, st) == E
    assert L.znippy_rows_set_block_tree(gpu_ctx.h, None, tree, st) == E
    assert L.znippy_rows_set_block_tree(gpu_ctx.h, bare, tree, st) == E
    assert L.znippy_rows_set_block_tree(gpu_ctx.h, rows, tree, None) == 0
    assert read(gpu_ctx.h, rows, dp, u64(0, 0), u64(7, 200_000), u64(5, 3), 2, op) == 0          # packed; status, decoded and hashed filled
    assert [st[0], st[1]] == [0, 0] and (dec.value, hsh.value) == (0, 2 * BLK)
    assert out[:8].cpu().numpy().tobytes() == raw[7:12] + raw[200_000:200_003] and bool((out[8:] == SENTINEL).all().item())
    assert L.znippy_rows_read_ranges_verified(gpu_ctx.h, rows, dp, 0, u64(0), u64(1), u64(2), u64(40), 1, op, 256, None, None, None) == 0
    assert out[40:42].cpu().numpy().tobytes() == raw[1:3]
    assert L.znippy_rows_set_block_tree(gpu_ctx.h, rows, None, st) == 0                          # NULL removes
    other = C.c_void_p()
    assert L.znippy_ctx_create(0, None, C.byref(other)) == 0
    assert read(other, rows, dp, u64(0), u64(0), u64(4), 1, op) == E                             # a table of another context
    assert L.znippy_rows_set_block_tree(other, rows, tree, st) == E
    assert L.znippy_rows_block_tree_build(other, rows, dp, 0, tree, st) == E
    assert L.znippy_rows_block_tree_layout(other, rows, C.byref(n), None) == E
    t2 = C.c_void_p()
    assert L.znippy_rows_create(other, u64(0), u64(300_001), bitmap, u64(300_001), None, ck, 0, 1, C.byref(t2)) == 0
    L.znippy_ctx_destroy(other)                                                                   # closed, kept alive by its table
    assert read(other, t2, dp, u64(0), u64(0), u64(4), 1, op) == E
    assert L.znippy_rows_set_block_tree(other, t2, tree, st) == E
    assert L.znippy_rows_block_tree_build(other, t2, dp, 0, tree, st) == E
    assert L.znippy_rows_block_tree_layout(other, t2, C.byref(n), None) == E
    L.znippy_rows_destroy(t2)
    L.znippy_rows_destroy(rows)
    L.znippy_rows_destroy(bare)
    torch.cuda.synchronize()


def test_not_a_run(gpu_ctx, oracle):
    import torch
    rows = [gen.pseudo_text(300_001, seed=51), gen.incompressible(9, 270_000), gen.text(10_240), gen.pseudo_text(2 * BLK, seed=52)]
    comp = [1, 0, 1, 1]
    frames = [f if c else r for f, r, c in zip(tr.own_frames(19, rows), rows, comp)]
    ck = digests(oracle, rows)
    ck[2] ^= 1                                                   # one checksum mismatch, so that the corrupt list has an entry
    tree = b3_tree.table_tree(rows)
    total = sum(len(r) for r in rows)
    ranges = [(0, 250_000, 4097), (3, 131_000, 200), (1, 5, 777)]

    def between(rt, d_blobs, tag):
        assert (rt.set_block_tree(tree) == 0).all()
        built, status = rt.build_block_tree(d_blobs)
        assert np.array_equal(built, tree) and (status == 0).all()
        verified_and_check(rt, d_blobs, rows, ranges, tag, want=(3 * BLK, 4 * BLK))     # one block of row 0, two of row 3; and one of the stored row

    def sequence(with_calls):
        rt, d_blobs, _ = tr.table_of(gpu_ctx, frames, rows, comp=comp, checksum=ck)
        outs = [tr.sentinel(total + 64) for _ in range(2)]
        rt.decode_verify_async(d_blobs, outs[0])
        if with_calls:
            between(rt, d_blobs, "between two runs")
        rt.decode_verify_async(d_blobs, outs[1])
        a = rt.results_lagged(1)
        if with_calls:
            between(rt, d_blobs, "between a run and its results")
        b, corrupt, status = rt.results()
        res = (a, b, list(corrupt), status.copy(), rt.digests().copy(), outs[0].cpu().numpy(), outs[1].cpu().numpy())
        if with_calls:
            between(rt, d_blobs, "behind the runs")
        v = rt.verify(d_blobs)
        res += (v[0], list(v[1]), v[2].copy(), rt.digests().copy())
        rt.close()
        return res

    plain, mixed_in = sequence(False), sequence(True)
    assert plain[0]["corrupt_rows"] == 1 and plain[2] == [2]
    for k, (x, y) in enumerate(zip(plain, mixed_in)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, k
    torch.cuda.synchronize()
