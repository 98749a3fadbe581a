"""No result depends on what recycled device memory held (api.hip, above tmalloc).

A table's device arrays come from a per-context recycler that hands back whatever the previous table left in them, the context's
grow-only pools are shared by every table and run and never cleared, and page-locked mirrors are recycled the same way.  The rest of
the suite builds almost every table on fresh memory and zeroed outputs, on a session-wide context whose history depends on the tests
selected.  Here every case runs on contexts created with ZNIPPY_POISON — every recycled or pooled buffer filled with one byte before
it is handed out, and every pool again in front of every run and batch call — with the fill bytes 0x00, 0xFF (reads as the code's
own sentinels: 0xFFFFFFFF skip entries, RX_NONE, LDM_NONE) and 0x5A (large junk), and on two clean contexts created under the same
other switches.  The caller's output regions hold a guard byte, not zeros.

Every case asserts:
 - oracle agreement (inside the scenario, on every context): bytes, statuses, digests, counters, the corrupt list; guard bytes
   untouched wherever the oracle writes nothing;
 - the same route as the clean context: RowTable.foreign_stats (the pool counters: bytes of the literal pool, sequence records,
   frames decoded by the parallel parsers, blocks given up and why — what a speculative kernel that read junk and handed its row to
   the fallback would change), RowTable.checksum_stats, the counters, and the set of kernel names of every run or call;
 - the same answer for every fill byte, and the clean contexts': all five records are equal.

Route fields are compared only where the two clean contexts agree with each other; a field on which they do not must be named in
UNSTABLE below, with the reason, or the case fails.  Left out of the records altogether:
 - the digest rows of rows whose status is negative (RowTable.digests() hands out the whole column; a row that was not decoded has
   no digest, and nothing writes its 32 bytes);
 - the bytes INSIDE the output range of a row whose status is negative, in the comparison with the oracle only (a decoder may have
   written a part of the row before it failed; the five contexts must still agree on them);
 - Context.run_lane_stats: with the switch on, the context waits for all of its streams in front of every run, so runs that
   otherwise stand beside each other stand behind each other (timing may change, results may not);
 - the kernel times themselves.

Under ZNIPPY_FZ_ONLY the oracle agreement is one-sided (ReadCase.check_without_fallback): the switch takes the serial decoder away, so
what the parallel paths leave comes out corrupt by design and the oracle cannot say which rows those are.
"""
import zlib

import numpy as np
import pytest

import b3_tree
import gen
import gpu_cases
import gunzip_checks as GZ
import inflate_checks as IN
import range_checks as RC
import targz_checks as TZ
import zstd_synth_cases as K
from deflate_build import block_kind_cases, rejection_cases
from gpu_cases import build_archive, frame_table, make_ctx, oracle_rows

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0x5A)
GUARD = 0xA5
TAIL = 64  # guard bytes behind the last row of every output image

# Route fields on which two clean contexts may differ: "<run>/<group>/<field>" -> why.  (None so far: pool offsets are handed out
# by atomic adds in whatever order the waves arrive, but the totals the statistics report do not depend on the order.)
UNSTABLE = {}

SWITCH_SETS = [
    ("default", {}),
    ("roles_min_1", {"ZNIPPY_ROLES_MIN": "1"}),
    ("no_bx", {"ZNIPPY_NO_BX": "1"}),
    ("no_bx+no_fz", {"ZNIPPY_NO_BX": "1", "ZNIPPY_NO_FZ": "1"}),
    ("no_rx", {"ZNIPPY_NO_RX": "1"}),
    ("fz_only", {"ZNIPPY_FZ_ONLY": "1"}),
]


# ---- contexts -----------------------------------------------------------------------------------------------------------------

class Ctxs:
    """Two clean contexts and one per fill byte, all under the same other switches."""

    def __init__(self, env):
        self.env = dict(env)
        self.all = [("clean_a", make_ctx(env)), ("clean_b", make_ctx(env))]
        self.all += [(f"poison_{v:#04x}", make_ctx(dict(env, ZNIPPY_POISON=f"{v:#04x}"))) for v in FILLS]

    def close(self):
        for _, c in self.all:
            c.close()


@pytest.fixture(scope="module", params=SWITCH_SETS, ids=[s for s, _ in SWITCH_SETS])
def ctxs(request):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    name, env = request.param
    c = Ctxs(env)
    c.name = name
    yield c
    c.close()


@pytest.fixture(scope="module")
def default_ctxs():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = Ctxs({})
    c.name = "default"
    yield c
    c.close()


# ---- records and their comparison ---------------------------------------------------------------------------------------------

def differences(a, b, path=""):
    """Paths at which two records (nested dicts / lists / arrays / scalars) differ."""
    if isinstance(a, dict) and isinstance(b, dict):
        out = [f"{path}/{k}" for k in set(a) ^ set(b)]
        for k in sorted(set(a) & set(b), key=str):
            out += differences(a[k], b[k], f"{path}/{k}")
        return out
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b):
            return [path + "/len"]
        out = []
        for i, (x, y) in enumerate(zip(a, b)):
            out += differences(x, y, f"{path}/{i}")
        return out
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or not np.array_equal(a, b):
            at = "" if a.shape != b.shape else f"@{int(np.flatnonzero(a.reshape(-1) != b.reshape(-1))[0])}"
            return [path + at]
        return []
    return [] if a == b else [f"{path} ({a!r} != {b!r})"]


def strip(paths):
    return {p.split(" (")[0].split("@")[0].lstrip("/") for p in paths}


def everywhere(ctxs, scenario):
    """The scenario on every context (it asserts oracle agreement itself and returns {"results": ..., "route": ...}), then the
    three comparisons of the module docstring."""
    recs = [(name, scenario(ctx)) for name, ctx in ctxs.all]
    (_, ca), (_, cb) = recs[0], recs[1]
    d = differences(ca["results"], cb["results"])
    assert not d, ("two clean contexts give different results", ctxs.name, d[:8])
    unstable = strip(differences(ca["route"], cb["route"]))
    assert unstable <= set(UNSTABLE), ("route fields on which two clean contexts differ, not named in UNSTABLE", ctxs.name, sorted(unstable))
    for name, p in recs[2:]:
        d = differences(ca["results"], p["results"])
        assert not d, ("results differ from the clean context's", ctxs.name, name, d[:8])
        d = [x for x in differences(ca["route"], p["route"]) if not strip([x]) <= unstable]
        assert not d, ("the route differs from the clean context's", ctxs.name, name, d[:8])
    for (na, a), (nb, b) in zip(recs[2:], recs[3:]):   # (follows from the above; stated because it is what the fill bytes are for)
        assert not differences(a["results"], b["results"]), (na, nb)
    return ca


def kernel_names(ctx):
    return sorted(set(n for n, _ in ctx.kernel_times()))


def guard_buf(n):
    import torch
    return torch.full((n,), GUARD, dtype=torch.uint8, device="cuda")


# ---- read side: archives ------------------------------------------------------------------------------------------------------

class ReadCase:
    """An archive with the oracle's read loop over it: counters, corrupt list and the output image over a guard-filled region.
    lenient: rows the oracle rejects may be decoded by the library to the intended bytes (hand-built invalid frames: the rule of
    gpu_cases.fuzz_run) — bytes are then compared with the oracle's only in rows that are clean on both sides."""

    def __init__(self, oracle, arch, extent=None, lenient=False, batch_checksums=0):
        self.arch = arch
        self.n = len(arch["usize"])
        ends = arch["out_off"].astype(np.int64) + arch["usize"].astype(np.int64)
        self.extent = (int(ends.max()) if self.n else 0) + TAIL if extent is None else extent
        self.want, wc, self.img = oracle_rows(oracle, arch, extent=self.extent, fill=GUARD)
        self.want_corrupt = sorted(int(x) for x in wc)
        self.lenient = lenient
        self.batch_checksums = batch_checksums
        self.bitmap = np.packbits(arch["compressed"].astype(bool), bitorder="little")
        self.blobs = np.concatenate([arch["blobs"], np.zeros(32, np.uint8)])

    def table(self, ctx):
        from znippy_amd import hip
        a = self.arch
        return hip.RowTable(ctx, a["blob_offset"], a["blob_size"], a["usize"], a["out_off"], self.bitmap, a["checksum"])

    def row_mask(self, rows):
        m = np.zeros(self.extent, bool)
        for i in rows:
            o = int(self.arch["out_off"][i])
            m[o:o + int(self.arch["usize"][i])] = True
        return m

    def check_without_fallback(self, tag, kind, counters, corrupt, status, img, digests, left):
        """ZNIPPY_FZ_ONLY: the switch takes the serial decoder away, and what the parallel paths leave — damaged frames, frames they
        decline — comes out as a row that was neither written nor hashed, on the corrupt list by design.  The oracle cannot say which
        rows those are, so the agreement is one-sided: every row the run reports clean holds the oracle's bytes and the oracle's
        digest, no row the oracle finds corrupt is reported clean, and the counters add up over the clean rows.  `left`: the corrupt
        list of the scenario's first decode + verify run, which stands in for the list a decode-only run does not make."""
        a = self.arch
        failed = [int(i) for i in np.flatnonzero(status < 0)]
        listed = list(left) if kind == "plain" else corrupt
        assert set(self.want_corrupt) <= set(listed) | set(failed), (tag, listed, self.want_corrupt)
        clean = np.ones(self.n, bool)
        clean[failed + listed] = False
        assert counters["total_chunks"] == self.n and counters["decode_errors"] == len(failed), (tag, counters)
        if kind != "plain":
            assert counters["corrupt_rows"] == len(corrupt) and counters["verified_bytes"] == int(a["usize"][clean].sum()), (tag, counters)
        if img is not None:
            skip = self.row_mask(failed + listed)
            ok = (img == self.img) | skip
            assert ok.all(), (tag, "first byte that differs from the oracle's image", int(np.flatnonzero(~ok)[0]))
        if digests is not None:
            assert np.array_equal(digests[clean], a["checksum"][clean]), tag

    def check(self, tag, kind, counters, corrupt, status, img, digests):
        """kind: "full" (decode + verify), "plain" (decode-only: the oracle's counters without what a checksum column adds) or
        "verify" (no output)."""
        want = self.want
        failed = [int(i) for i in np.flatnonzero(status < 0)]
        assert len(failed) == want["decode_errors"], (tag, len(failed), want)
        if kind == "plain":
            assert (counters["total_chunks"], counters["decode_errors"], counters["corrupt_rows"], counters["total_written_bytes"]) == \
                   (want["total_chunks"], want["decode_errors"], 0, want["total_written_bytes"]), (tag, counters, want)
        else:
            assert counters == want, (tag, counters, want)
            assert corrupt == self.want_corrupt, (tag, corrupt, self.want_corrupt)
        if img is not None:
            skip = self.row_mask(failed + (self.want_corrupt + corrupt if self.lenient else []))
            ok = (img == self.img) | skip
            assert ok.all(), (tag, "first byte that differs from the oracle's image", int(np.flatnonzero(~ok)[0]))
        if digests is not None:
            good = status >= 0
            good[self.want_corrupt] = False
            assert np.array_equal(digests[good], self.arch["checksum"][good]), tag

    def scenario(self, ctx, fallback=True):
        """Three decode + verify runs on one table (full, then the lean repeats), a decode-only run and a verify-only run on tables of
        their own.  fallback=False: the context has no serial decoder (check_without_fallback)."""
        import torch
        ctx.set_batch_checksums(self.batch_checksums)
        d_blobs = torch.from_numpy(self.blobs).cuda()
        res, route = {}, {}
        left = []

        def check(tag, kind, counters, corrupt, status, img, digests):
            if fallback:
                return self.check(tag, kind, counters, corrupt, status, img, digests)
            if kind == "full" and tag[1] == 0:
                left.extend(corrupt)
            return self.check_without_fallback(tag, kind, counters, corrupt, status, img, digests, left)

        def note(key, rt, counters, corrupt, status, img, digests):
            has = status >= 0
            if not fallback:   # (a row that was left has no digest: nothing wrote its 32 bytes)
                has[sorted(set(corrupt) | set(left))] = False
            res[key] = dict(counters=dict(counters), corrupt=corrupt, status=status.copy(), img=img,
                            digests=None if digests is None else digests[has].copy())
            route[key] = dict(kernels=names, counters=dict(counters), foreign=rt.foreign_stats(), checksum=rt.checksum_stats())

        rt = self.table(ctx)
        for rep in range(3):
            d_out = guard_buf(self.extent)
            counters, corrupt, status = rt.decode_verify(d_blobs, d_out)
            names = kernel_names(ctx)
            corrupt, img, dig = sorted(int(x) for x in corrupt), d_out.cpu().numpy(), rt.digests()
            check(("decode_verify", rep), "full", counters, corrupt, status, img, dig)
            note(f"decode_verify_{rep}", rt, counters, corrupt, status, img, dig)
        rt.close()
        rt = self.table(ctx)
        d_out = guard_buf(self.extent)
        counters, status = rt.decode(d_blobs, d_out)
        names = kernel_names(ctx)
        img = d_out.cpu().numpy()
        check("decode_rows", "plain", counters, [], status, img, None)
        note("decode_rows", rt, counters, [], status, img, None)
        rt.close()
        rt = self.table(ctx)
        counters, corrupt, status = rt.verify(d_blobs)
        names = kernel_names(ctx)
        corrupt, dig = sorted(int(x) for x in corrupt), rt.digests()
        check("verify_rows", "verify", counters, corrupt, status, None, dig)
        note("verify_rows", rt, counters, corrupt, status, None, dig)
        rt.close()
        return dict(results=res, route=route)


def _frames_arch(A, n):
    return dict(blobs=A["blobs"], blob_offset=A["bo"], blob_size=A["bs"], usize=A["us"], out_off=A["oo"], checksum=A["ck"],
                compressed=np.ones(n, np.uint8))


def _own_archive(oracle, entries):
    """entries written by this library's encoder (a clean context of its own); the checksum column is the oracle's."""
    import torch
    from znippy_amd import hip
    ctx = make_ctx({})
    src = np.frombuffer(b"".join(entries) + bytes(64), dtype=np.uint8)
    lens = np.array([len(e) for e in entries], dtype=np.uint64)
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    rounds = hip.RoundTable(ctx, offs, lens)
    d_blob = torch.zeros(rounds.blob_bound() + 64, dtype=torch.uint8, device="cuda")
    enc = rounds.encode_hash(torch.from_numpy(src.copy()).cuda(), d_blob)
    arch = dict(blobs=d_blob[:int(enc["blob_bytes"])].cpu().numpy(), blob_offset=enc["blob_offset"].copy(), blob_size=enc["blob_size"].copy(),
                usize=lens, out_off=offs, compressed=np.ones(len(entries), np.uint8),
                checksum=np.stack([np.frombuffer(oracle.blake3(e), dtype=np.uint8) for e in entries]))
    rounds.close()
    ctx.close()
    return arch


def _synth_arch(oracle, cases):
    A = frame_table(oracle, [c.want for c in cases], [c.frame for c in cases])
    return _frames_arch(A, len(cases))


def _build_read_case(name, oracle):
    if name == "random":
        return ReadCase(oracle, gpu_cases.random_case(oracle)[0])
    if name == "mixed":
        return ReadCase(oracle, gpu_cases.mixed_case(oracle)[0])
    if name == "foreign":
        return ReadCase(oracle, gpu_cases.foreign_case(oracle)[0])
    if name == "store":
        S = gpu_cases.store_case(oracle)
        arch = dict(blobs=S["blobs"], blob_offset=S["bo"], blob_size=S["bs"], usize=S["bs"], out_off=S["oo"], checksum=S["ck"],
                    compressed=np.zeros(len(S["sizes"]), np.uint8))
        case = ReadCase(oracle, arch, extent=S["total"])
        assert GUARD == 0xA5 and np.array_equal(case.img, S["want"]) and case.want_corrupt == [S["bad_row"]]   # the builder's own image, same guard byte
        return case
    if name == "big_rows":
        return ReadCase(oracle, _own_archive(oracle, gpu_cases.big_rows_entries()))
    if name == "periodic_rows":
        return ReadCase(oracle, build_archive(oracle, gpu_cases.periodic_rows_entries(), level=19))
    valid = [c for c in K.valid_cases() if not c.no_size]
    if name == "synth_valid":
        return ReadCase(oracle, _synth_arch(oracle, valid))
    if name == "synth_valid+batch_checksums":
        return ReadCase(oracle, _synth_arch(oracle, valid), batch_checksums=1)
    if name == "synth_invalid":   # the invalid frames between valid ones, so that the kernels' waves hold both
        bad = K.invalid_cases()
        rows = []
        for i, c in enumerate(bad):
            rows += [c, valid[i % len(valid)]]
        return ReadCase(oracle, _synth_arch(oracle, rows), lenient=True)
    raise KeyError(name)


READ_CASES = ["random", "mixed", "foreign", "store", "big_rows", "periodic_rows", "synth_valid", "synth_valid+batch_checksums", "synth_invalid"]
_read_cases = {}


@pytest.fixture(scope="module")
def read_case(oracle):
    """Cases by name, each built once per module (oracle side) and left unchanged."""
    def get(name):
        if name not in _read_cases:
            _read_cases[name] = _build_read_case(name, oracle)
        return _read_cases[name]
    return get


@pytest.mark.parametrize("name", READ_CASES)
def test_read_side(ctxs, read_case, name):
    case = read_case(name)
    rec = everywhere(ctxs, (lambda ctx: case.scenario(ctx, fallback=False)) if ctxs.name == "fz_only" else case.scenario)
    # the case is what it is meant to be on this switch set (a clean context's record: all five are equal)
    first = rec["route"]["decode_verify_0"]["kernels"]
    if name in ("foreign", "synth_valid") and ctxs.name in ("default", "roles_min_1"):
        assert "zstd_batch_execute" in first and "zstd_resolve_expand" in first, first
    if name == "foreign" and ctxs.name == "no_bx":
        assert "zstd_foreign_entropy" in first, first
    if name == "big_rows" and ctxs.name == "default":
        assert "decode_verify_fused_blocks" in first, first
    if name == "periodic_rows" and ctxs.name == "roles_min_1":
        assert "decode_verify_roles" in first, first
    if name == "synth_valid+batch_checksums" and ctxs.name == "default":
        assert rec["route"]["decode_verify_0"]["checksum"]["verified"] > 0


# ---- read side: byte ranges and the block tree --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def range_rows(oracle):
    rows = [gen.pseudo_text(n, seed=40 + i) for i, n in enumerate(RC.ROW_SIZES[:-1])] + [gpu_cases.mixed(RC.ROW_SIZES[-1], seed=9)]
    A = gpu_cases.foreign_archive(oracle, [gen.pseudo_text(300_001, seed=3), gen.pseudo_text(200_000, seed=4)], 19)
    return dict(rows=rows, frames=RC.own_frames(19, rows), ck=np.stack([np.frombuffer(oracle.blake3(r), np.uint8) for r in rows]),
                tree=b3_tree.table_tree(rows), foreign=A, foreign_rows=[gen.pseudo_text(300_001, seed=3), gen.pseudo_text(200_000, seed=4)])


def test_ranges_and_block_tree(ctxs, range_rows):
    """znippy_rows_read_ranges, _block_tree_build, _set_block_tree and _read_ranges_verified on the rows of test_gpu_ranges.py: the
    block pass and the whole-row passes share the range scratch, and every call builds and destroys private tables."""
    R = range_rows
    ranges = RC.boundary_ranges(RC.ROW_SIZES)
    all_bytes = sum(RC.ROW_SIZES)

    def scenario(ctx):
        from znippy_amd import hip
        res, route = {}, {}
        rt, d_blobs, _ = RC.table_of(ctx, R["frames"], R["rows"], checksum=R["ck"])
        res["decoded"] = RC.read_and_check(rt, d_blobs, R["rows"], ranges, "ranges", want_decoded=all_bytes)
        route["read_ranges"] = kernel_names(ctx)
        tree, status = rt.build_block_tree(d_blobs)
        route["build"] = kernel_names(ctx)
        assert (status == 0).all() and np.array_equal(tree, R["tree"])     # the reference is tests/b3_tree.py: nothing of the library
        assert (rt.set_block_tree(tree) == 0).all()
        route["set"] = kernel_names(ctx)
        res["verified"] = RC.verified_and_check(rt, d_blobs, R["rows"], ranges, "verified", want=(all_bytes, all_bytes))
        route["verified"] = kernel_names(ctx)
        few = [(4, 300_000, 1), (4, 262_144, 5), (2, 131_072, 1), (0, 17, 3)]
        res["few"] = RC.verified_and_check(rt, d_blobs, R["rows"], few, "few", guard=1, want=((300_001 - 2 * RC.BLK) + 1 + 5_000,) * 2)
        rt.close()
        A = R["foreign"]   # foreign frames: every range through the whole-row pass
        rt = hip.RowTable(ctx, A["bo"], A["bs"], A["us"], A["oo"], None, A["ck"])
        fr = [(0, 0, 1), (0, 300_000, 1), (1, 131_071, 2), (1, 140_000, 4097), (0, 140_000, 4097)]
        res["foreign"] = RC.read_and_check(rt, RC.to_dev(A["blobs"]), R["foreign_rows"], fr, "foreign", want_decoded=500_001)
        route["foreign"] = kernel_names(ctx)
        rt.close()
        return dict(results=res, route=route)

    rec = everywhere(ctxs, scenario)
    assert {"range_scan", "range_decode_blocks", "range_decode_rows", "range_copy"} <= set(rec["route"]["read_ranges"]), rec["route"]["read_ranges"]


# ---- table order on one poisoned context --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def table_order(read_case, oracle):
    """(the cases in order, each one's record on a fresh clean context)"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    many = read_case("foreign")
    A = many.arch
    few_rows = [150, 151, 160, 163]   # three small frames and a big one of the same archive, as a table of its own
    few = ReadCase(oracle, dict(blobs=A["blobs"], blob_offset=A["blob_offset"][few_rows], blob_size=A["blob_size"][few_rows], usize=A["usize"][few_rows],
                                out_off=(np.cumsum(A["usize"][few_rows]) - A["usize"][few_rows]).astype(np.uint64), checksum=A["checksum"][few_rows],
                                compressed=np.ones(len(few_rows), np.uint8)))
    order = [many, few, read_case("store"), read_case("big_rows"), many]
    want = []
    for case in order[:4]:
        ctx = make_ctx({})
        want.append(case.scenario(ctx))
        ctx.close()
    want.append(want[0])
    return order, want


@pytest.mark.parametrize("fill", FILLS, ids=[f"{v:#04x}" for v in FILLS])
def test_table_order_on_one_context(table_order, fill):
    """The shape of both historic faults: a table with many item slots, then one with few, then ones of other paths (no compressed
    row; this library's own multi-block frames), then the first again, each destroyed before the next is made — so each is carved
    from what its predecessors left — on ONE poisoned context.  Every result equals that table's result on a fresh clean context."""
    order, want = table_order
    ctx = make_ctx({"ZNIPPY_POISON": f"{fill:#04x}"})
    try:
        for k, (case, w) in enumerate(zip(order, want)):
            got = case.scenario(ctx)
            assert not differences(w["results"], got["results"]), (k, differences(w["results"], got["results"])[:8])
            d = [x for x in differences(w["route"], got["route"]) if not strip([x]) <= set(UNSTABLE)]
            assert not d, (k, d[:8])
    finally:
        ctx.close()


# ---- write side ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def write_case(oracle):
    entries, skip, digests = gpu_cases.write_case(oracle)
    return dict(entries=entries, skip=np.array(skip, np.uint8), digests=digests, tree=b3_tree.table_tree(entries),
                first=b3_tree.row_first([len(e) for e in entries]))


WRITE_RUNS = [  # name, level, window_log, store_incompressible + blob_align 128 + emit_block_tree
    ("level_1", 1, 0, False),
    ("level_19", 19, 0, False),
    ("level_19_window_23", 19, 23, False),
    ("level_19_options", 19, 0, True),
]


@pytest.mark.parametrize("run", WRITE_RUNS, ids=[r[0] for r in WRITE_RUNS])
def test_write_side(default_ctxs, write_case, oracle, run):
    """gpu_cases.write_case encoded twice on one table: frames decode by the oracle's decoder (libzstd), digests are the oracle's,
    stored rounds are their input, nothing is written behind the blob bytes; offsets, sizes, flags, trees and blob bytes are
    identical on all five contexts."""
    _, level, window_log, options = run
    W = write_case
    entries = W["entries"]
    lens = np.array([len(e) for e in entries], np.uint64)
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    src = np.frombuffer(b"".join(entries) + bytes(64), np.uint8).copy()

    def scenario(ctx):
        import torch
        from znippy_amd import hip
        ctx.set_level(level)
        ctx.set_window_log(window_log)
        d_src = torch.from_numpy(src).cuda()
        rt = hip.RoundTable(ctx, offs, lens, W["skip"])
        if options:
            rt.set_store_incompressible(True)
            rt.set_blob_align(128)
            rt.emit_block_tree(True)
        bound = rt.blob_bound()
        res, route = {}, {}
        for rep in range(2):
            d_blob = guard_buf(bound + 4096)
            enc = rt.encode_hash(d_src, d_blob)
            names = kernel_names(ctx)
            img = d_blob.cpu().numpy()
            bo, bs, comp, total = enc["blob_offset"].copy(), enc["blob_size"].copy(), enc["compressed"].copy(), int(enc["blob_bytes"])
            assert total <= bound and (img[total:] == GUARD).all(), ("a byte behind the blob bytes was written", rep)
            used = np.zeros(total, bool)
            for i, e in enumerate(entries):
                o, n = int(bo[i]), int(bs[i])
                used[o:o + n] = True
                f = img[o:o + n].tobytes()
                assert enc["checksum"][i].tobytes() == W["digests"][i], (rep, i)
                assert (o % 128 == 0) if options else (o == (int(bo[i - 1] + bs[i - 1]) if i else 0)), (rep, i, o)
                if comp[i]:
                    assert not W["skip"][i] and oracle.libzstd_decompress(f, max(len(e), 1)) == e, (rep, i, len(e))
                else:
                    assert (W["skip"][i] or options) and f == e, (rep, i)
            assert (img[:total][~used] == 0).all(), "the gaps between aligned payloads are zeros"
            res[rep] = dict(blob_offset=bo, blob_size=bs, compressed=comp, checksum=enc["checksum"].copy(), total=total, img=img)
            if options:
                tree = rt.block_tree()
                assert np.array_equal(tree, W["tree"]), rep                # tests/b3_tree.py: nothing of the library
                res[rep]["tree"] = tree
            route[rep] = names
        rt.close()
        return dict(results=res, route=route)

    rec = everywhere(default_ctxs, scenario)
    if options:
        assert (rec["results"][0]["compressed"][W["skip"] == 0] == 0).any(), "no round was stored by the opt-in pass: the case does not reach it"
    if window_log:
        assert "ldm_index" in rec["route"][0], rec["route"][0]


def test_hash_rounds(default_ctxs, oracle):
    """znippy_hash_rounds on the ragged table of test_gpu_blake3.py (twice on one table: the tile CVs of the first call are still there)."""
    offs, sizes, buf = gpu_cases.ragged_rounds()
    want = np.stack([np.frombuffer(oracle.blake3(buf[o:o + s]), np.uint8) for o, s in zip(offs, sizes)])

    def scenario(ctx):
        import torch
        from znippy_amd import hip
        d = torch.from_numpy(buf.copy()).cuda()
        rt = hip.RoundTable(ctx, offs, sizes)
        res, route = {}, {}
        for rep in range(2):
            got = rt.hash(d)
            assert np.array_equal(got, want), (rep, int(np.flatnonzero((got != want).any(axis=1))[0]))
            res[rep], route[rep] = got.copy(), kernel_names(ctx)
        rt.close()
        return dict(results=res, route=route)

    everywhere(default_ctxs, scenario)


# ---- the DEFLATE batch calls --------------------------------------------------------------------------------------------------

def test_inflate_batch(default_ctxs):
    """The small accept and reject cases of znippy_inflate_batch (tests/inflate_checks.py asserts zlib's verdicts, bytes, CRCs and the
    guard bytes), rejected items between clean ones."""
    accept = block_kind_cases()
    reject = rejection_cases()
    clean = accept[1]
    mixed_in = []
    for c in reject:
        mixed_in += [c, clean]

    def scenario(ctx):
        res, route = {}, {}
        res["accept"] = np.array(IN.check(ctx, accept, "packed", accept_only=True))
        route["accept"] = kernel_names(ctx)
        res["reject"] = np.array(IN.check(ctx, mixed_in, "reversed"))
        route["reject"] = kernel_names(ctx)
        assert (res["reject"][0::2] == IN.E_CORRUPT).all() and (res["reject"][1::2] == IN.OK).all()
        return dict(results=res, route=route)

    everywhere(default_ctxs, scenario)


def test_gunzip_batch(default_ctxs):
    """znippy_gunzip_batch: single members, several members, flush segments (tests/gunzip_checks.py asserts the model's contents,
    members and segments, and the guard bytes), then damaged files and rooms one byte short beside clean ones."""
    t = gen.pseudo_text(30_000, seed=2)
    flush = GZ.flushed([t[:10_000], t[10_000:20_000], t[20_000:]], zlib.Z_FULL_FLUSH)
    three = GZ.gz(gen.text(5000)) + GZ.gz(b"") + GZ.gz(gen.pseudo_text(9000, seed=5), 9)
    small = GZ.gz(gen.text(500))
    valid = [three, flush, GZ.bgzf(gen.pseudo_text(5 * 3000, seed=8), 3000), small, GZ.gz(b"")]
    flip = lambda s, at: s[:at] + bytes([s[at] ^ 0x10]) + s[at + 1:]   # noqa: E731
    bad = [(flush, GZ.OK, 30_000), (flip(flush, len(flush) - 8), GZ.E_CHECKSUM, 30_000), (flush[:len(flush) // 2], GZ.E_CORRUPT, 30_000),
           (small, GZ.OK, 500), (small[:-1], GZ.E_CORRUPT, 500), (flush, GZ.E_DST_SMALL, 29_999), (three + b"x", GZ.E_CORRUPT, 14_000), (small, GZ.OK, 777)]

    def scenario(ctx):
        res, route = {}, {}
        want, segments, names = GZ.check_valid(ctx, valid, seg_min=1)
        res["valid"], route["valid"] = [segments, [w[1:] for w in want]], sorted(set(names))
        status, got, members, segments, names = GZ.run_batch(ctx, [b[0] for b in bad], [b[2] for b in bad], seg_min=1)
        assert status == [b[1] for b in bad], status
        res["bad"], route["bad"] = [status, got, members, segments], sorted(set(names))
        return dict(results=res, route=route)

    rec = everywhere(default_ctxs, scenario)
    assert {"gunzip_probe", "gunzip_inflate", "gunzip_crc"} <= set(rec["route"]["valid"]), rec["route"]["valid"]


def test_targz_find_batch(default_ctxs):
    """znippy_targz_find_batch: the valid tars and the malformed files of test_gpu_targz.py (tests/targz_checks.py asserts the model's
    statuses and members, and the guard bytes)."""
    from test_tar_rules_cpu import make_tar
    items = [TZ.gz(t, 6, name="pkg-1.0.crate" if i & 1 else None) for i, t in enumerate(TZ.valid_tars())]
    b = make_tar("gnu", [("pkg-1.0/Cargo.toml", b"second member")])
    odd = [TZ.gz(b, 6), b"PK\x03\x04" + bytes(60), b"\x1f\x8b\x07" + bytes(60), b"", TZ.gz(b, 6)[:40], TZ.gz(b, 6, name="a-file-name.crate")]

    def scenario(ctx):
        res, route = {}, {}
        want, status, scanned = TZ.check(ctx, items, b"/Cargo.toml")
        res["valid"], route["valid"] = [status, scanned], kernel_names(ctx)
        want, status, scanned = TZ.check(ctx, odd, b"/Cargo.toml")
        res["odd"], route["odd"] = [status, scanned], kernel_names(ctx)
        assert status[0] == 0 and status[-1] == 0 and all(s != 0 for s in status[1:-1]), status
        return dict(results=res, route=route)

    everywhere(default_ctxs, scenario)


# ---- found under this module: ZNIPPY_FZ_ONLY and the digest of a row that was left ---------------------------------------------

def test_fz_only_row_that_is_left_is_corrupt_whatever_its_digest_slot_held():
    """ZNIPPY_FZ_ONLY promises that a row the parallel paths leave shows up as a corrupt row.  Such a row is never hashed, and the
    verify kernel compared whatever its digest slot held: the whole suite in one process showed two clean contexts disagreeing on a
    damaged archive, one of them reporting left rows verified — their slots held the rows' right digests from an earlier context's
    table.  Built deliberately here, with the poison switch off: a first table of good frames, run twice, leaves the right digests
    in both digest slots; a second table of the same rows is carved from those buffers, and one of its frames has a skippable frame
    in front, which the batch path declines as a whole (tests/test_gpu_synth.py: DECLINED).  The row must be on the corrupt list
    and its bytes unwritten, in every run."""
    import torch
    from znippy_amd import hip
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import workloads
    data = gpu_cases.py_corpus(200_000)
    entries = [data[i * 10240:(i + 1) * 10240] for i in range(12)]
    frames = [workloads.libzstd_compress(e, 19) for e in entries]
    left = 5
    prefixed = list(frames)
    prefixed[left] = bytes.fromhex("502a4d18") + (4).to_bytes(4, "little") + b"skip" + frames[left]
    ctx = make_ctx({"ZNIPPY_FZ_ONLY": "1"})
    setup = make_ctx({})
    ck = np.stack([np.frombuffer(setup.blake3(e), np.uint8) for e in entries])
    setup.close()
    total = 12 * 10240
    try:
        for k, fr in enumerate((frames, prefixed)):
            bs = np.array([len(f) for f in fr], np.uint64)
            bo = (np.cumsum(bs) - bs).astype(np.uint64)
            us = np.full(12, 10240, np.uint64)
            oo = (np.cumsum(us) - us).astype(np.uint64)
            d_blobs = torch.from_numpy(np.frombuffer(b"".join(fr) + bytes(64), np.uint8).copy()).cuda()
            rt = hip.RowTable(ctx, bo, bs, us, oo, None, ck)
            for rep in range(2):
                d_out = guard_buf(total + TAIL)
                c, corrupt, status = rt.decode_verify(d_blobs, d_out)
                img = d_out.cpu().numpy()
                want = np.concatenate([np.frombuffer(b"".join(entries), np.uint8), np.full(TAIL, GUARD, np.uint8)])
                if k == 0:
                    assert (status == 0).all() and c["corrupt_rows"] == 0 and np.array_equal(img, want), (rep, c)
                    assert np.array_equal(rt.digests(), ck)
                else:
                    want[left * 10240:(left + 1) * 10240] = GUARD
                    assert [int(x) for x in corrupt] == [left] and c["corrupt_rows"] == 1 and c["verified_bytes"] == total - 10240, (rep, c, list(corrupt))
                    assert np.array_equal(img, want), rep
            rt.close()
    finally:
        ctx.close()


# ---- the switch itself --------------------------------------------------------------------------------------------------------

def test_the_switch_is_read_as_documented():
    """Unset, empty and malformed values leave the switch off; 0 is a fill byte like any other; decimal and 0x.. both work.  Seen from
    outside through the one place where a caller can read memory that nothing wrote: RowTable.digests() hands out the whole digest
    column, and the rows of rows that were not decoded are never written.  A first table of two good rows, run twice, leaves its
    digests in both digest slots and in its checksum column; a second table of the same shape, whose rows both fail, is carved from
    those buffers: with the switch off it shows the first table's digests, with the switch on the fill byte."""
    import torch
    from znippy_amd import hip
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rows = [gen.text(100), gen.binary(100)]
    setup = make_ctx({})
    frames = [setup.compress(r) for r in rows]
    ck = np.stack([np.frombuffer(setup.blake3(r), np.uint8) for r in rows])
    setup.close()
    bs = np.array([len(f) for f in frames], np.uint64)
    bo = (np.cumsum(bs) - bs).astype(np.uint64)
    us, oo = np.array([100, 100], np.uint64), np.array([0, 100], np.uint64)
    good = torch.from_numpy(np.frombuffer(b"".join(frames) + bytes(64), np.uint8).copy()).cuda()
    zeros = torch.zeros(good.numel(), dtype=torch.uint8, device="cuda")   # no magic number: both rows fail

    def second_table_digests(env):
        ctx = make_ctx(env)
        rt = hip.RowTable(ctx, bo, bs, us, oo, None, ck)
        for _ in range(2):
            c, corrupt, status = rt.decode_verify(good, guard_buf(264))
            assert (status == 0).all() and c["corrupt_rows"] == 0
        assert np.array_equal(rt.digests(), ck)
        rt.close()
        rt = hip.RowTable(ctx, bo, bs, us, oo, None, ck)
        c, corrupt, status = rt.decode_verify(zeros, guard_buf(264))
        assert (status < 0).all() and c["decode_errors"] == 2
        d = rt.digests().copy()
        rt.close()
        ctx.close()
        return d

    for value, byte in (("0x5a", 0x5A), ("90", 0x5A), ("090", 0x5A), ("0", 0), ("0x00", 0), ("255", 0xFF), ("0xFF", 0xFF), ("0XA7", 0xA7)):
        assert (second_table_digests({"ZNIPPY_POISON": value}) == byte).all(), value
    for env in ({}, {"ZNIPPY_POISON": ""}, {"ZNIPPY_POISON": "256"}, {"ZNIPPY_POISON": "-1"}, {"ZNIPPY_POISON": "0x100"}, {"ZNIPPY_POISON": "5a"},
                {"ZNIPPY_POISON": "on"}):
        assert np.array_equal(second_table_digests(env), ck), env
