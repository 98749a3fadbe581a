"""Verify-only runs (znippy_verify_rows: the read loop with save_data=false, decompress.rs:L186-189 / index.rs:L550-553)
against the oracle's restated read loop: a verify run reports exactly what a decode run of the same table over the same blobs
reports — counters, corrupt list, status column, digests — takes its place in the table's run sequence like any other run, and
writes no row that no kernel has to read back.  Every case runs on a default context and on contexts created under the switch
sets that change which kernels a run launches."""
import ctypes as C

import numpy as np
import pytest

import gen
import workloads
from gpu_cases import (build_archive, frame_table, make_ctx, mixed_archive_entries, oracle_rows, py_corpus, random_archive,
                       random_mutants)

pytestmark = pytest.mark.gpu

SWITCH_SETS = [
    ("default", {}),
    ("roles_min_1", {"ZNIPPY_ROLES_MIN": "1"}),
    ("no_roles", {"ZNIPPY_NO_ROLES": "1"}),
    ("no_lean", {"ZNIPPY_NO_LEAN": "1"}),
    ("no_bx", {"ZNIPPY_NO_BX": "1"}),
    ("no_bx+no_fz", {"ZNIPPY_NO_BX": "1", "ZNIPPY_NO_FZ": "1"}),
    ("no_rx", {"ZNIPPY_NO_RX": "1"}),
    ("store_g_2", {"ZNIPPY_STORE_G": "2"}),
    ("no_stored_only", {"ZNIPPY_NO_STORED_ONLY": "1"}),
    ("no_block_items", {"ZNIPPY_NO_BLOCK_ITEMS": "1"}),
    ("no_fused_blocks", {"ZNIPPY_NO_FUSED_BLOCKS": "1"}),
]


@pytest.fixture(scope="module", params=SWITCH_SETS, ids=[s for s, _ in SWITCH_SETS])
def sw(request):
    """(name, switch set, context created under it)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    name, env = request.param
    ctx = make_ctx(env)
    yield name, env, ctx
    ctx.close()


def _names(ctx):
    return set(dict(ctx.kernel_times()))


class _DevMem:
    """Device memory at a raw address as something torch.as_tensor takes (no copy)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def scratch_tensor(ctx, rt):
    """The table's part of the context's verify scratch as a uint8 CUDA tensor (None: the table takes none), its slots."""
    import torch
    ctx.sync()
    base, nbytes, off = rt.verify_scratch()
    if not nbytes:
        return None, nbytes, off
    return torch.as_tensor(_DevMem(base, nbytes), device="cuda"), nbytes, off


def to_dev(blobs, pad=0):
    import torch
    return torch.from_numpy(np.concatenate([np.zeros(pad, np.uint8), blobs, np.zeros(64, np.uint8)])).cuda()


def make_table(ctx, arch, pad=0, out=True):
    from znippy_amd import hip
    bitmap = np.packbits(arch["compressed"].astype(bool), bitorder="little")
    return hip.RowTable(ctx, arch["blob_offset"] + np.uint64(pad), arch["blob_size"], arch["usize"],
                        arch["out_off"] if out else None, bitmap, arch["checksum"])


def check_run(arch, want, want_corrupt, counters, corrupt, status, rt, tag):
    """One run's results against the oracle's read loop: counters, corrupt list, status, every good row's digest."""
    assert counters == want, (tag, counters, want)
    assert sorted(int(x) for x in corrupt) == sorted(int(x) for x in want_corrupt), tag
    ok = status >= 0
    assert int((~ok).sum()) == want["decode_errors"], tag
    good = ok.copy()
    good[[int(x) for x in want_corrupt]] = False
    assert np.array_equal(rt.digests()[good], arch["checksum"][good]), tag
    return ok


def check_decoded_bytes(arch, ok, out, want_out, tag):
    for i in np.nonzero(ok)[0]:
        a, b = int(arch["out_off"][i]), int(arch["out_off"][i] + arch["usize"][i])
        assert np.array_equal(out[a:b], want_out[a:b]), (tag, int(i))


# ---- cases (oracle side: once per module) ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def random_cases(oracle):
    out = []
    for seed in (4, 5, 6):
        arch = random_archive(oracle, seed=seed, n_rows=700)
        out.append((arch, oracle_rows(oracle, arch)))
    return out


@pytest.fixture(scope="module")
def mixed_case(oracle):
    entries, skip = mixed_archive_entries()
    arch = build_archive(oracle, entries, level=3, skip=skip)
    return arch, oracle_rows(oracle, arch)


@pytest.fixture(scope="module")
def foreign_case(oracle):
    """libzstd -19 frames of real text: 10 KiB ones (batch path), 64-256 KiB ones and one above 256 KiB (resolve path),
    three of them damaged."""
    data = py_corpus(3 << 20)
    entries = [data[i * 10240:(i + 1) * 10240] for i in range(160)]
    entries += [data[2_000_000:2_000_000 + n] for n in (65_537, 100_000, 180_000, 262_143)] + [data[1_700_000:1_700_000 + 300_001]]
    frames = [workloads.libzstd_compress(e, 19) for e in entries]
    A = frame_table(oracle, entries, frames)
    blobs = A["blobs"].copy()
    rng = np.random.default_rng(8)
    for i in (17, 161, 164):
        blobs[int(A["bo"][i]) + int(rng.integers(8, int(A["bs"][i]) - 4))] ^= 0x5A
    arch = dict(blobs=blobs, blob_offset=A["bo"], blob_size=A["bs"], usize=A["us"], out_off=A["oo"], checksum=A["ck"],
                compressed=np.ones(len(entries), np.uint8))
    return arch, oracle_rows(oracle, arch)


@pytest.fixture(scope="module")
def big_case(oracle):
    """Big rows of this build's own multi-block frames — periodic text (periodic blocks), incompressible bytes (raw blocks),
    binary and word soup (blocks for the block decoder), a short last block — beside a big stored row; one frame damaged."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import hip
    rows = [gen.text(4 * 131072), gen.incompressible(21, 3 * 131072), gen.binary(4 * 131072), gen.pseudo_text(2 * 131072 + 5000, seed=3),
            gen.text(6 * 131072), gen.incompressible(22, 2 * 131072 + 77), gen.incompressible(23, 5 * 131072 + 1)]
    comp = np.array([1, 1, 1, 1, 1, 1, 0], np.uint8)
    ctx0 = hip.Context(0)
    frames = [ctx0.compress(r) if c else r for r, c in zip(rows, comp)]
    ctx0.close()
    bs = np.array([len(f) for f in frames], np.uint64)
    bo = (np.cumsum(bs) - bs).astype(np.uint64)
    us = np.array([len(r) for r in rows], np.uint64)
    oo = (np.cumsum(us) - us).astype(np.uint64)
    ck = np.stack([np.frombuffer(oracle.blake3(r), dtype=np.uint8) for r in rows])
    blobs = np.frombuffer(b"".join(frames), dtype=np.uint8).copy()
    blobs[int(bo[4]) + 40] ^= 0x7F
    arch = dict(blobs=blobs, blob_offset=bo, blob_size=bs, usize=us, out_off=oo, checksum=ck, compressed=comp)
    return arch, oracle_rows(oracle, arch)


@pytest.fixture(scope="module")
def store_case(oracle):
    """No compressed row: ragged rows, 64-leaf rows, big rows, empty and tiny rows, one damaged."""
    rng = np.random.default_rng(31)
    sizes = [65536, 200_000, 65536, 65537, 3 * 65536, (1 << 20) + 1] + [int(x) for x in rng.integers(0, 30000, 120)]
    sizes += [10240] * 40 + [0, 1, 15, 16, 17, 1023, 1024, 1025]
    rows = [gen.incompressible(900 + i, n) for i, n in enumerate(sizes)]
    arch = build_archive(oracle, rows, level=3, skip=np.ones(len(rows), np.uint8))
    blobs = arch["blobs"].copy()
    blobs[int(arch["blob_offset"][9]) + 7] ^= 0x10
    arch["blobs"] = blobs
    return arch, oracle_rows(oracle, arch)


@pytest.fixture(scope="module")
def c2_case(oracle):
    """A C2-shaped table: 2,048 tiles of six 10 KiB text rows (libzstd -19 frames), every blob in a slot wide enough for the
    frame that replaces one of them later."""
    n = 6 * 2048
    data = gen.text(10240)
    frame = oracle.libzstd_compress(data, 19)
    other = gen.pseudo_text(10240, seed=5)                    # same size, another content, not of the recognised shape
    other_frame = oracle.libzstd_compress(other, 3)
    assert len(other_frame) > len(frame)
    slot = len(other_frame) + 7
    blob = np.zeros(n * slot + 64, np.uint8)
    blob[:n * slot].reshape(n, slot)[:, :len(frame)] = np.frombuffer(frame, np.uint8)
    return dict(n=n, data=data, frame=frame, other_frame=other_frame, slot=slot, blob=blob,
                bo=np.arange(n, dtype=np.uint64) * np.uint64(slot), bs=np.full(n, len(frame), np.uint64),
                us=np.full(n, 10240, np.uint64), oo=np.arange(n, dtype=np.uint64) * np.uint64(10240),
                ck=np.tile(np.frombuffer(oracle.blake3(data), dtype=np.uint8), (n, 1)))


# ---- 1. parity with the oracle's read loop --------------------------------------------------------------------------

def _verify_decode_verify_verify(ctx, arch, want, want_corrupt, want_out, pad):
    import torch
    total = int(arch["usize"].sum())
    d_blobs = to_dev(arch["blobs"], pad)
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    rt = make_table(ctx, arch, pad)
    ok = None
    for step, mode in enumerate(("verify", "decode", "verify", "verify")):
        if mode == "verify":
            counters, corrupt, status = rt.verify(d_blobs)
        else:
            counters, corrupt, status = rt.decode_verify(d_blobs, d_out)
        ok = check_run(arch, want, want_corrupt, counters, corrupt, status.copy(), rt, (step, mode))
    check_decoded_bytes(arch, ok, d_out.cpu().numpy(), want_out, "bytes of the decode run, after the verify runs around it")
    rt.close()


def test_random_archives_match_the_oracle(sw, random_cases):
    name, env, ctx = sw
    for k, (arch, (want, want_corrupt, want_out)) in enumerate(random_cases):
        _verify_decode_verify_verify(ctx, arch, want, want_corrupt, want_out, pad=3 + k)


def test_mixed_archive_matches_the_oracle(sw, mixed_case):
    name, env, ctx = sw
    arch, (want, want_corrupt, want_out) = mixed_case
    assert want["corrupt_rows"] == 0 and want["decode_errors"] == 0
    _verify_decode_verify_verify(ctx, arch, want, want_corrupt, want_out, pad=5)


# ---- 2. every path, 3. no row is written that need not be -----------------------------------------------------------

def test_c2_table_full_lean_and_changed_blobs(sw, c2_case):
    """The first verify run of a C2-shaped table is a full one, the second a lean one (the role-split kernel and the verify);
    then one row's blob becomes a frame the kernel does not recognise and another is damaged: the flagged lean verify run
    reports what a context without lean runs reports.  The table's scratch, filled with a pattern after the first run, still
    holds the pattern after the second: every row is of the recognised shape, so not one row may be materialised."""
    import torch
    from znippy_amd import hip
    name, env, _ = sw
    S = c2_case
    n, slot = S["n"], S["slot"]

    def run(extra):
        ctx = make_ctx(dict(env, **extra))
        d_blobs = torch.from_numpy(S["blob"].copy()).cuda()
        rt = hip.RowTable(ctx, S["bo"], S["bs"], S["us"], None, None, S["ck"])
        seen, untouched = [], None
        for step in range(5):
            if step == 3:
                d_blobs[1234 * slot:1234 * slot + len(S["other_frame"])] = torch.from_numpy(np.frombuffer(S["other_frame"], np.uint8).copy()).cuda()
                d_blobs[77 * slot + 20] ^= 0x55
                torch.cuda.synchronize()
            if step == 1:
                t, nbytes, off = scratch_tensor(ctx, rt)
                assert nbytes == n * 10240 and (off == np.arange(n, dtype=np.uint64) * np.uint64(10240)).all()
                t.fill_(0xA5)
                torch.cuda.synchronize()
            c, corrupt, status = rt.verify(d_blobs)
            kt = _names(ctx)
            if step == 1:
                t, _, _ = scratch_tensor(ctx, rt)
                untouched = bool((t == 0xA5).all().item())
            seen.append((dict(c), sorted(int(x) for x in corrupt), status.copy(), rt.digests().copy(), "blake3_hash_only" in kt, kt))
        rt.close(); ctx.close()
        return seen, untouched

    (lean, untouched), (full, _) = run({}), run({"ZNIPPY_NO_LEAN": "1"})
    assert all(s[4] for s in full)
    roles = "ZNIPPY_NO_ROLES" not in env
    if roles:
        assert "verify_roles" in lean[0][5] and "decode_verify_roles" not in lean[0][5], sorted(lean[0][5])
    else:
        assert "verify_small" in lean[0][5] and "verify_roles" not in lean[0][5], sorted(lean[0][5])
    assert untouched, "a verify run of recognised rows wrote into the scratch"
    if roles and "ZNIPPY_NO_LEAN" not in env:
        assert lean[0][4] and not lean[1][4] and not lean[2][4], [s[4] for s in lean]   # full, then lean
    for a, b in zip(lean, full):
        assert a[0] == b[0] and a[1] == b[1] and (a[2] == b[2]).all() and (a[3] == b[3]).all()
    for s in lean[:3]:
        assert s[0]["corrupt_rows"] == 0 and s[0]["decode_errors"] == 0 and s[0]["verified_bytes"] == n * 10240 and (s[3] == S["ck"]).all()
        assert s[0]["total_written_bytes"] == n * 10240   # counted whatever save_data is (decompress.rs:L168-169)
    assert lean[3][0]["corrupt_rows"] + lean[3][0]["decode_errors"] == 2, lean[3][0]
    assert lean[4][0] == lean[3][0]


def test_big_rows_of_own_frames_and_a_big_stored_row(sw, big_case):
    name, env, ctx = sw
    arch, (want, want_corrupt, want_out) = big_case
    assert want["corrupt_rows"] + want["decode_errors"] == 1
    d_blobs = to_dev(arch["blobs"])
    rt = make_table(ctx, arch, out=False)
    for rep in range(3):
        counters, corrupt, status = rt.verify(d_blobs)
        check_run(arch, want, want_corrupt, counters, corrupt, status.copy(), rt, rep)
        if rep == 0:
            names = _names(ctx)
            assert "decode_verify_fused_blocks" not in names and "blake3_second_pass" not in names, sorted(names)
            assert ("verify_blocks" in names) == (name not in ("no_block_items", "no_fused_blocks")), sorted(names)
            assert "blake3_hash_only" in names, sorted(names)
    t, nbytes, off = scratch_tensor(ctx, rt)
    assert off[6] == 2**64 - 1 and (off[:6] % 16 == 0).all() and nbytes >= int(arch["usize"][:6].sum())
    rt.close()


def test_foreign_frames_land_in_their_scratch_slots(sw, foreign_case):
    name, env, ctx = sw
    arch, (want, want_corrupt, want_out) = foreign_case
    d_blobs = to_dev(arch["blobs"])
    rt = make_table(ctx, arch, out=False)
    for rep in range(2):
        counters, corrupt, status = rt.verify(d_blobs)
        ok = check_run(arch, want, want_corrupt, counters, corrupt, status.copy(), rt, rep)
        if rep == 0:
            names = _names(ctx)
            if name.startswith("no_bx"):
                assert "zstd_batch_execute" not in names, sorted(names)
            else:
                assert "zstd_batch_execute" in names, sorted(names)
                assert ("zstd_resolve_expand" in names) == (name != "no_rx"), sorted(names)
    # these rows go through real decoders: every good row's slot holds the oracle's decoded bytes
    t, nbytes, off = scratch_tensor(ctx, rt)
    host = t.cpu().numpy()
    assert (off % 16 == 0).all()
    good = ok.copy()
    good[[int(x) for x in want_corrupt]] = False
    for i in np.nonzero(good)[0]:
        a, b = int(arch["out_off"][i]), int(arch["out_off"][i] + arch["usize"][i])
        assert np.array_equal(host[int(off[i]):int(off[i]) + (b - a)], want_out[a:b]), int(i)
    rt.close()


def test_table_without_a_compressed_row_takes_no_scratch(sw, store_case):
    name, env, ctx = sw
    arch, (want, want_corrupt, want_out) = store_case
    assert want["corrupt_rows"] == 1 and list(want_corrupt) == [9]
    d_blobs = to_dev(arch["blobs"], 1)
    rt = make_table(ctx, arch, pad=1, out=False)
    for rep in range(2):
        counters, corrupt, status = rt.verify(d_blobs)
        check_run(arch, want, want_corrupt, counters, corrupt, status.copy(), rt, rep)
        names = _names(ctx)
        assert "blake3_hash_only" in names and "blake3_second_pass" not in names, sorted(names)
        assert ("verify_small" in names) == (name == "no_stored_only"), sorted(names)
    base, nbytes, off = rt.verify_scratch()
    assert nbytes == 0 and (off == 2**64 - 1).all()
    rt.close()


def test_verify_run_leaves_an_earlier_decode_runs_output_alone(sw, mixed_case):
    """The bytes in d_out belong to the caller once the decode run's results were read: a verify run queued afterwards on the
    same table writes nothing there."""
    import torch
    name, env, ctx = sw
    arch, (want, want_corrupt, want_out) = mixed_case
    total = int(arch["usize"].sum())
    d_blobs = to_dev(arch["blobs"])
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    rt = make_table(ctx, arch)
    counters, corrupt, status = rt.decode_verify(d_blobs, d_out)
    assert counters == want and np.array_equal(d_out[:total].cpu().numpy(), want_out)
    d_out.fill_(0x3C)
    torch.cuda.synchronize()
    for rep in range(2):
        counters, corrupt, status = rt.verify(d_blobs)
        check_run(arch, want, want_corrupt, counters, corrupt, status.copy(), rt, rep)
    assert bool((d_out == 0x3C).all().item())
    rt.close()


# ---- 4. pipeline ----------------------------------------------------------------------------------------------------

def test_pipeline_of_alternating_verify_and_decode_runs(sw, oracle):
    """Four runs queued on one table, verify and decode in turn over two output buffers, read one run behind; another row is
    damaged before each run: every run's counters are its own."""
    import torch
    name, env, ctx = sw
    rng = np.random.default_rng(2)
    entries = [gen.text(int(rng.integers(1024, 12000))) for _ in range(500)] + [gen.incompressible(40 + i, (1 << 19) + 777 * i) for i in range(2)]
    arch = build_archive(oracle, entries, level=19, skip=[0] * 500 + [1] * 2)
    total = int(arch["usize"].sum())
    blobs = arch["blobs"].copy()
    d_blobs = to_dev(blobs)
    outs = [torch.zeros(total + 64, dtype=torch.uint8, device="cuda") for _ in range(2)]
    rt = make_table(ctx, arch)
    wants, got = [], []
    for k in range(4):
        row = (37, 501, 250, 499)[k]
        at = int(arch["blob_offset"][row]) + int(arch["blob_size"][row]) // 2
        blobs[at] ^= 0x21
        torch.cuda.synchronize()
        d_blobs[at] ^= 0x21
        torch.cuda.synchronize()
        a = dict(arch, blobs=blobs.copy())
        wants.append(oracle_rows(oracle, a))
        if k % 2 == 0:
            rt.verify_async(d_blobs)
        else:
            rt.decode_verify_async(d_blobs, outs[(k >> 1) & 1])
        if k >= 1:
            got.append(rt.results_lagged(1))
    got.append(rt.results_lagged(0))
    assert got == [w[0] for w in wants], (got, [w[0] for w in wants])
    assert got[0] != got[3] and got[3]["corrupt_rows"] + got[3]["decode_errors"] >= 2, got
    ctx.sync()
    for k in (1, 3):   # the decode runs' bytes: every row that decoded (a damaged stored row is written as it is)
        want, want_corrupt, want_out = wants[k]
        out = outs[(k >> 1) & 1].cpu().numpy()
        bad = set(int(x) for x in want_corrupt)
        for i in range(len(entries)):
            o, l = int(arch["out_off"][i]), int(arch["usize"][i])
            if i not in bad and i not in (37, 501, 250, 499):
                assert np.array_equal(out[o:o + l], want_out[o:o + l]), (k, i)
    rt.close()


# ---- 6. damaged input -----------------------------------------------------------------------------------------------

def test_mutated_frames_in_verify_mode(gpu_ctx, oracle):
    """The mutant scheme of the decode suite (gpu_cases.fuzz_run) at a reduced count, verified without an output: a mutant the
    oracle accepts is accepted and flagged exactly when its content changed; one the oracle rejects is rejected or flagged;
    none is reported verified with a digest other than the index's.  Rows whose index points outside the blob region are
    ZNIPPY_E_CORRUPT."""
    import torch
    from znippy_amd import _lib, hip
    rng = np.random.default_rng(2024)
    bases = [(gen.text(10240), 19), (gen.binary(10240), 19), (gen.pseudo_text(6000, 3), 3), (gen.pseudo_text(70000, 5), 3),
             (gen.random_lcg(3000), 3), (bytes(5000), 3), (gen.pseudo_text(300_000, 11), 3), (gen.incompressible(6, 270_000), 1)]
    frames, sizes, originals = [], [], []
    for data, lvl in bases:
        for base in (oracle.libzstd_compress(data, lvl), gpu_ctx.compress(data)):
            frames.append(base); sizes.append(len(data)); originals.append(data)
            for m in random_mutants(base, rng, 30):
                frames.append(m); sizes.append(len(data)); originals.append(data)
    n = len(frames)
    bs = np.array([len(f) for f in frames] + [100, 9], dtype=np.uint64)
    bo = np.concatenate([[0], np.cumsum(bs[:n])[:-1], [0, 0]]).astype(np.uint64)
    blob = b"".join(frames)
    bo[n] = len(blob) + 64 - 50            # runs over the end of the region
    bo[n + 1] = np.uint64(2**64 - 4)       # offset + size wraps
    us = np.array(sizes + [1000, 20], dtype=np.uint64)
    dig = {}
    for d in originals:
        if d not in dig:
            dig[d] = np.frombuffer(oracle.blake3(d), dtype=np.uint8)
    ck = np.stack([dig[d] for d in originals] + [np.zeros(32, np.uint8)] * 2)
    d_blobs = torch.from_numpy(np.frombuffer(blob + bytes(64), dtype=np.uint8).copy()).cuda()
    rt = hip.RowTable(gpu_ctx, bo, bs, us, None, None, ck)
    counters, corrupt, status = rt.verify(d_blobs)
    digests = rt.digests()
    corrupt = set(int(x) for x in corrupt)
    assert status[n] == _lib.E_CORRUPT and status[n + 1] == _lib.E_CORRUPT
    n_ok = n_rej = n_flagged = 0
    for i in range(n):
        try:
            want = oracle.zstd_decompress(frames[i], cap=sizes[i])
            oracle_ok = len(want) == sizes[i]
        except ValueError:
            oracle_ok = False
        if oracle_ok:
            assert status[i] == 0, (i, status[i])
            assert digests[i].tobytes() == oracle.blake3(want), i
            assert (i in corrupt) == (want != originals[i]), i
            n_ok += 1
        elif status[i] < 0:
            n_rej += 1
        else:
            assert i in corrupt or digests[i].tobytes() == ck[i].tobytes(), i
            n_flagged += 1
    assert counters["total_chunks"] == n + 2 and counters["decode_errors"] == int((status < 0).sum())
    assert n_ok >= 16 and n_rej >= 40, (n_ok, n_rej)
    print(f"mutants: {n} rows, oracle-accepted {n_ok}, rejected by both {n_rej}, gpu-decoded-but-flagged {n_flagged}")
    rt.close()


# ---- 7. the ABI through ctypes --------------------------------------------------------------------------------------

def test_abi_of_the_verify_entry_points(gpu_ctx, oracle):
    import torch
    from znippy_amd import _lib
    from znippy_amd._lib import VerifyCounters
    L = _lib.lib()
    E_INVAL = _lib.E_INVAL
    for sym in ("znippy_verify_rows", "znippy_verify_rows_async", "znippy_rows_verify_scratch"):
        assert hasattr(L, sym), sym
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    data = gen.text(10240)
    frame = oracle.libzstd_compress(data, 19)
    ck = (C.c_uint8 * 32).from_buffer_copy(oracle.blake3(data))
    d = torch.from_numpy(np.frombuffer(frame + bytes(64), np.uint8).copy()).cuda()
    dp = C.c_void_p(d.data_ptr())
    # a table created without output offsets verifies, and refuses a decode call; every other NULL stays an error
    rows = C.c_void_p()
    assert L.znippy_rows_create(gpu_ctx.h, u64(0), u64(len(frame)), None, u64(10240), None, ck, 0, 1, C.byref(rows)) == 0
    assert L.znippy_rows_create(gpu_ctx.h, None, u64(len(frame)), None, u64(10240), None, ck, 0, 1, C.byref(C.c_void_p())) == E_INVAL
    assert L.znippy_rows_create(gpu_ctx.h, u64(0), None, None, u64(10240), None, ck, 0, 1, C.byref(C.c_void_p())) == E_INVAL
    assert L.znippy_rows_create(gpu_ctx.h, u64(0), u64(len(frame)), None, None, None, ck, 0, 1, C.byref(C.c_void_p())) == E_INVAL
    out = torch.zeros(10240 + 64, dtype=torch.uint8, device="cuda")
    assert L.znippy_decode_verify_rows_async(gpu_ctx.h, rows, dp, 0, C.c_void_p(out.data_ptr()), 10240) == E_INVAL
    c = VerifyCounters()
    st = (C.c_int32 * 1)()
    assert L.znippy_verify_rows_async(gpu_ctx.h, rows, None, 0) == E_INVAL          # NULL blobs with rows
    assert L.znippy_verify_rows(gpu_ctx.h, rows, None, 0, C.byref(c), None, 0, st) == E_INVAL
    assert L.znippy_verify_rows(None, rows, dp, 0, C.byref(c), None, 0, st) == E_INVAL
    assert L.znippy_verify_rows(gpu_ctx.h, None, dp, 0, C.byref(c), None, 0, st) == E_INVAL
    assert L.znippy_verify_rows(gpu_ctx.h, rows, dp, 0, C.byref(c), None, 0, st) == 0
    assert c.as_dict() == dict(total_chunks=1, total_written_bytes=10240, verified_bytes=10240, corrupt_bytes=0, corrupt_rows=0,
                               decode_errors=0) and st[0] == 0
    digest = (C.c_uint8 * 32)()
    assert L.znippy_rows_digests(gpu_ctx.h, rows, digest) == 0 and bytes(digest) == oracle.blake3(data)
    base, nbytes, off = C.c_void_p(), C.c_uint64(), u64(7)
    assert L.znippy_rows_verify_scratch(gpu_ctx.h, rows, C.byref(base), C.byref(nbytes), off) == 0
    assert nbytes.value == 10240 and off[0] == 0 and base.value
    assert L.znippy_rows_verify_scratch(gpu_ctx.h, rows, None, C.byref(nbytes), None) == E_INVAL
    assert L.znippy_rows_verify_scratch(gpu_ctx.h, rows, C.byref(base), C.byref(nbytes), None) == 0
    L.znippy_rows_destroy(rows)
    # an empty table is fine
    empty = C.c_void_p()
    assert L.znippy_rows_create(gpu_ctx.h, u64(0), u64(0), None, u64(0), None, None, 0, 0, C.byref(empty)) == 0
    assert L.znippy_verify_rows(gpu_ctx.h, empty, None, 0, C.byref(c), None, 0, None) == 0 and c.total_chunks == 0
    L.znippy_rows_destroy(empty)
    # a table of another context, and a closed context
    ctx = C.c_void_p()
    assert L.znippy_ctx_create(0, None, C.byref(ctx)) == 0
    rows = C.c_void_p()
    assert L.znippy_rows_create(ctx, u64(0), u64(len(frame)), None, u64(10240), None, ck, 0, 1, C.byref(rows)) == 0
    assert L.znippy_verify_rows_async(gpu_ctx.h, rows, dp, 0) == E_INVAL
    L.znippy_ctx_destroy(ctx)                      # the table is alive: the context is closed, not freed
    assert L.znippy_verify_rows_async(ctx, rows, dp, 0) == E_INVAL
    assert L.znippy_verify_rows(ctx, rows, dp, 0, C.byref(c), None, 0, st) == E_INVAL
    assert L.znippy_rows_verify_scratch(ctx, rows, C.byref(base), C.byref(nbytes), None) == E_INVAL
    L.znippy_rows_destroy(rows)


def test_python_tables_without_output_offsets(gpu_ctx, oracle):
    import torch
    from znippy_amd import hip
    from znippy_amd._lib import ZnippyError
    entries = [gen.text(10240), gen.incompressible(1, 3000), b"", gen.pseudo_text(20000, 3)]
    arch = build_archive(oracle, entries, level=3, skip=[0, 1, 0, 0])
    d_blobs = to_dev(arch["blobs"])
    rt = make_table(gpu_ctx, arch, out=False)
    c, corrupt, status = rt.verify(d_blobs)
    assert c["verified_bytes"] == sum(len(e) for e in entries) and (status == 0).all() and len(corrupt) == 0
    assert np.array_equal(rt.digests(), arch["checksum"])
    with pytest.raises(ZnippyError):
        rt.decode_verify(d_blobs, torch.zeros(40000, dtype=torch.uint8, device="cuda"))
    c2, _, _ = rt.verify(d_blobs)                  # the refused call queued nothing and broke nothing
    assert c2 == c
    base, nbytes, off = rt.verify_scratch()
    assert off[1] == 2**64 - 1 and off[2] == 2**64 - 1 and off[0] == 0 and off[3] == 10240
    rt.close()


def test_recognised_rows_with_ragged_leaves_are_not_written_either(sw, oracle):
    """Rows of the recognised shape whose length is not a whole number of KiB (nearly every real row), six to a tile: the
    small-row kernel hashes them from their windows through the generic leaf path, so the scratch keeps its pattern; a tile
    that also holds a stored row and a row for the scalar decoder is right as well."""
    import torch
    name, env, ctx = sw
    sizes = [10000, 9999, 10241, 11111, 64 * 1024 - 1, 20000, 12345, 30001, 10000, 10000, 10001] * 40   # ten leaves or more: <= 6 rows per tile
    entries = [gen.text(n) for n in sizes]
    arch = build_archive(oracle, entries, level=19)
    want, want_corrupt, want_out = oracle_rows(oracle, arch)
    d_blobs = to_dev(arch["blobs"], 1)
    rt = make_table(ctx, arch, pad=1, out=False)
    counters, corrupt, status = rt.verify(d_blobs)
    check_run(arch, want, want_corrupt, counters, corrupt, status.copy(), rt, "first")
    t, nbytes, off = scratch_tensor(ctx, rt)
    t.fill_(0xA5)
    torch.cuda.synchronize()
    counters, corrupt, status = rt.verify(d_blobs)
    check_run(arch, want, want_corrupt, counters, corrupt, status.copy(), rt, "second")
    assert (status == 0).all() and counters["corrupt_rows"] == 0
    t, _, _ = scratch_tensor(ctx, rt)
    assert bool((t == 0xA5).all().item()), "a recognised row with a ragged leaf was written"
    rt.close()
    # short ragged rows, more than six to a tile: those beyond the sixth go through the pre-pass and their scratch slots
    sizes = [65, 1023, 1025, 3000, 4097, 7777, 100, 2049] * 60
    entries = [gen.text(n) for n in sizes]
    arch = build_archive(oracle, entries, level=19)
    want, want_corrupt, want_out = oracle_rows(oracle, arch)
    d_blobs = to_dev(arch["blobs"], 2)
    rt = make_table(ctx, arch, pad=2, out=False)
    for rep in range(2):
        counters, corrupt, status = rt.verify(d_blobs)
        check_run(arch, want, want_corrupt, counters, corrupt, status.copy(), rt, ("short", rep))
    assert (status == 0).all() and counters["corrupt_rows"] == 0
    rt.close()
    # mixed tile: recognised ragged rows beside a stored row and a word-soup row (scalar decoder / handed over)
    entries = [gen.text(10000), gen.incompressible(3, 5000), gen.pseudo_text(3000, 7), gen.text(9000), b"", gen.text(12345)] * 30
    arch = build_archive(oracle, entries, level=3, skip=[0, 1, 0, 0, 0, 0] * 30)
    want, want_corrupt, want_out = oracle_rows(oracle, arch)
    d_blobs = to_dev(arch["blobs"])
    rt = make_table(ctx, arch, out=False)
    for rep in range(2):
        counters, corrupt, status = rt.verify(d_blobs)
        check_run(arch, want, want_corrupt, counters, corrupt, status.copy(), rt, rep)
    assert counters["corrupt_rows"] == 0 and (status == 0).all()
    rt.close()
