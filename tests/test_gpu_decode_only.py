"""Decode-only runs (znippy_decode_rows: the extract path, which never looks at the checksum column — archive.rs:L144-168).
The reference of every case is twofold: the oracle's bytes, and a decode + verify run on the same context of a table built
from the same columns with checksum=None.  Counters and status are identical to that run, the whole output region is byte-
identical to that run's — the 0xA5 sentinel in the gaps between rows and behind the last row included — and no kernel of the
run hashes.  Every row is checked.  The cases run on a default context and on contexts created under the switch sets that
change which kernels a run launches."""
import ctypes as C

import numpy as np
import pytest

import gen
import workloads
import zstd_synth as zs
from gpu_cases import build_archive, frame_table, make_ctx, mixed_archive_entries, oracle_rows, py_corpus, random_archive

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
HASHING = {"decode_verify_roles", "decode_verify_fused", "decode_verify_fused_blocks", "blake3_second_pass", "blake3_merge_big",
           "blake3_hash_only"}
SENTINEL = 0xA5


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


def assert_no_hash_kernel(names, tag=""):
    bad = sorted(n for n in names if n in HASHING or n.startswith("verify"))
    assert not bad, (tag, bad, sorted(names))


def to_dev(blobs, pad=0):
    import torch
    return torch.from_numpy(np.concatenate([np.zeros(pad, np.uint8), blobs, np.zeros(64, np.uint8)])).cuda()


def make_table(ctx, arch, pad=0, checksum=True):
    from znippy_amd import hip
    bitmap = np.packbits(arch["compressed"].astype(bool), bitorder="little")
    return hip.RowTable(ctx, arch["blob_offset"] + np.uint64(pad), arch["blob_size"], arch["usize"], arch["out_off"], bitmap,
                        arch["checksum"] if checksum else None)


def out_region(total, shift):
    """total + 64 bytes of sentinel, starting `shift` bytes into a tensor."""
    import torch
    base = torch.full((total + 64 + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    return base[shift:shift + total + 64]


def extent(arch):
    return int((arch["out_off"] + arch["usize"]).max()) if len(arch["usize"]) else 0


def check_case(ctx, arch, oracle_res, pad=0, shift=0, tag="", reps=2):
    """A decode + verify run of the table without a checksum column, then decode-only runs of the table WITH the column (which
    must not be read): same counters, same status, same bytes in the whole region; the oracle's bytes in every decoded row."""
    want, want_corrupt, want_out = oracle_res
    total = extent(arch)
    d_blobs = to_dev(arch["blobs"], pad)
    ref_out = out_region(total, shift)
    rt_ref = make_table(ctx, arch, pad, checksum=False)
    c_ref, corrupt_ref, st_ref = rt_ref.decode_verify(d_blobs, ref_out)
    st_ref = st_ref.copy()
    ref_host = ref_out.cpu().numpy()
    rt_ref.close()
    assert len(corrupt_ref) == 0 and c_ref["verified_bytes"] == c_ref["total_written_bytes"]
    rt = make_table(ctx, arch, pad, checksum=True)
    names = set()
    for rep in range(reps):
        out = out_region(total, shift)
        counters, status = rt.decode(d_blobs, out)
        names |= _names(ctx)
        assert counters == c_ref, (tag, rep, counters, c_ref)
        assert np.array_equal(status, st_ref), (tag, rep, np.nonzero(status != st_ref)[0][:8])
        host = out.cpu().numpy()
        if not np.array_equal(host, ref_host):
            at = int(np.nonzero(host != ref_host)[0][0])
            row = int(np.searchsorted(arch["out_off"], at, side="right")) - 1
            raise AssertionError((tag, rep, "first differing byte", at, "row", row, int(arch["usize"][row]) if row >= 0 else None))
        assert bool((host[total:] == SENTINEL).all()), (tag, rep)
    assert_no_hash_kernel(names, tag)
    assert "count_rows" in names or not len(arch["usize"]), (tag, sorted(names))
    # the oracle's bytes, every decoded row; its counters without what a checksum column adds
    ok = st_ref >= 0
    assert int((~ok).sum()) == want["decode_errors"] and c_ref["total_chunks"] == want["total_chunks"], (tag, c_ref, want)
    assert c_ref["total_written_bytes"] == want["total_written_bytes"] and c_ref["corrupt_rows"] == 0, (tag, c_ref, want)
    for i in np.nonzero(ok)[0]:
        a, b = int(arch["out_off"][i]), int(arch["out_off"][i] + arch["usize"][i])
        assert np.array_equal(ref_host[a:b], want_out[a:b]), (tag, int(i))
    rt.close()
    return names


# ---- cases (oracle side: once per module) ---------------------------------------------------------------------------

def _want(oracle, arch):
    """oracle_rows for layouts with gaps: the output region spans to the last row's end."""
    n = len(arch["usize"])
    bitmap = np.packbits(arch["compressed"].astype(bool), bitorder="little")
    want_out = np.zeros(extent(arch), dtype=np.uint8)
    want, want_corrupt = oracle.decompress_rows(arch["blobs"], arch["blob_offset"], arch["blob_size"], arch["usize"], arch["out_off"],
                                                bitmap, arch["checksum"], 0, n, out=want_out)
    return want, want_corrupt, want_out


USIZES = [0, 1, 15, 16, 17, 127, 128, 129, 1023, 1024, 1025, 10240, 65535]
PERIODS = [1, 2, 3, 7, 16, 45, 64, 127, 128, 129, 1000]
PREFIXES = [0, 1, 200]


def periodic_frame(oracle, prefix, period, usize, seed):
    """(content, frame): `prefix` literal bytes, then `period` bytes repeated to the end.  Where the row is long enough, the frame is
    hand-built in the shape the small-row kernel recognises — raw literals (prefix + one period) and ONE overlapping match to the
    end; shorter rows are libzstd's frames of the same bytes."""
    rng = np.random.default_rng(seed)
    head = rng.integers(0, 256, prefix, dtype=np.uint8).tobytes()
    per = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
    data = (head + per * ((usize // period) + 2))[:usize]
    L0 = prefix + period
    if usize >= L0 + 64:
        frame = zs.write_frame([zs.Comp(data[:L0], [(L0, usize - L0, period + 3)], lit=dict(type="raw"))], content=data)
    else:
        frame = oracle.libzstd_compress(data, 19)
    return data, frame


@pytest.fixture(scope="module")
def periodic_cases(oracle):
    """Two layouts of the same rows: packed back to back (most rows start at odd addresses), and with 0-3 byte gaps."""
    entries, frames, comp = [], [], []
    k = 0
    for prefix in PREFIXES:
        for period in PERIODS:
            for usize in USIZES:
                data, frame = periodic_frame(oracle, prefix, period, usize, 7000 + k)
                assert oracle.zstd_decompress(frame, cap=max(usize, 1)) == data, (prefix, period, usize)
                entries.append(data); frames.append(frame); comp.append(1)
                if k % 3 == 0:  # a stored row of the same size beside it
                    raw = gen.incompressible(k, usize)
                    entries.append(raw); frames.append(raw); comp.append(0)
                k += 1
    A = frame_table(oracle, entries, frames)
    rng = np.random.default_rng(5)
    out = []
    for gaps in (False, True):
        oo = A["oo"].copy()
        if gaps:
            oo = oo + np.cumsum(rng.integers(0, 4, len(entries))).astype(np.uint64)
        arch = dict(blobs=A["blobs"], blob_offset=A["bo"], blob_size=A["bs"], usize=A["us"], out_off=oo, checksum=A["ck"],
                    compressed=np.array(comp, np.uint8))
        out.append((arch, _want(oracle, arch)))
    return out


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
def store_case(oracle):
    """No compressed row (the stored_only plan): ragged rows, 64-leaf rows, big rows, empty and tiny rows."""
    rng = np.random.default_rng(31)
    sizes = [65536, 200_000, 65536, 65537, 3 * 65536, (1 << 20) + 1] + [int(x) for x in rng.integers(0, 30000, 120)]
    sizes += [10240] * 40 + [0, 1, 15, 16, 17, 1023, 1024, 1025]
    rows = [gen.incompressible(900 + i, n) for i, n in enumerate(sizes)]
    arch = build_archive(oracle, rows, level=3, skip=np.ones(len(rows), np.uint8))
    return arch, oracle_rows(oracle, arch)


@pytest.fixture(scope="module")
def foreign_case(oracle):
    """libzstd -19 frames of real text: 160 of 10 KiB (batch path), five of 64-300 KiB (batch and resolve paths), three damaged."""
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
    """Big rows of this build's own multi-block frames — periodic text, incompressible bytes, binary, a short last block — beside
    big stored rows of 64 KiB + 1 and 1 MiB; one frame damaged."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import hip
    rows = [gen.text(4 * 131072), gen.incompressible(21, 3 * 131072), gen.binary(4 * 131072), gen.pseudo_text(2 * 131072 + 5000, seed=3),
            gen.text(6 * 131072), gen.incompressible(22, 2 * 131072 + 77), gen.incompressible(23, 65537), gen.incompressible(24, 1 << 20),
            gen.text(3 * 131072 + 1)]
    comp = np.array([1, 1, 1, 1, 1, 1, 0, 0, 1], np.uint8)
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


# ---- 1. periodic small rows at the edges of the line-store path ------------------------------------------------------

@pytest.mark.parametrize("shift", [0, 1, 15])
def test_periodic_small_rows_any_period_any_row_start(gpu_ctx, periodic_cases, shift):
    for k, (arch, res) in enumerate(periodic_cases):
        names = check_case(gpu_ctx, arch, res, pad=k, shift=shift, tag=("periodic", "gaps" if k else "packed", shift), reps=1)
        assert "decode_small" in names, sorted(names)


# ---- 2. the cases under every switch set ----------------------------------------------------------------------------

def test_existing_archive_fixtures(sw, mixed_case, random_cases, store_case):
    name, env, ctx = sw
    arch, res = mixed_case
    assert res[0]["decode_errors"] == 0
    names = check_case(ctx, arch, res, pad=5, tag="mixed")
    assert {"decode_small", "copy_stored"} <= names, sorted(names)
    for k, (arch, res) in enumerate(random_cases):
        check_case(ctx, arch, res, pad=3 + k, shift=k, tag=("random", k))
    arch, res = store_case
    names = check_case(ctx, arch, res, pad=1, tag="stored only")
    assert "copy_stored" in names and ("decode_small" in names) == (name == "no_stored_only"), sorted(names)


def test_periodic_rows_under_every_switch_set(sw, periodic_cases):
    name, env, ctx = sw
    arch, res = periodic_cases[1]
    check_case(ctx, arch, res, pad=2, shift=1, tag="periodic, gaps", reps=1)


def test_foreign_frames(sw, foreign_case):
    name, env, ctx = sw
    arch, res = foreign_case
    assert res[0]["decode_errors"] >= 1
    names = check_case(ctx, arch, res, tag="foreign")
    if name.startswith("no_bx"):
        assert "zstd_batch_execute" not in names, sorted(names)
    else:
        assert "zstd_batch_execute" in names, sorted(names)
        assert ("zstd_resolve_expand" in names) == (name != "no_rx"), sorted(names)


def test_big_rows(sw, big_case):
    name, env, ctx = sw
    arch, res = big_case
    assert res[0]["decode_errors"] + res[0]["corrupt_rows"] == 1
    names = check_case(ctx, arch, res, pad=1, tag="big")
    assert ("decode_blocks" in names) == (name not in ("no_block_items", "no_fused_blocks")), sorted(names)
    assert "copy_stored" in names, sorted(names)


# ---- 3. the run sequence --------------------------------------------------------------------------------------------

def lean_table(ctx):
    """240 rows of the 10 KiB text chunk (40 tiles: the role-split kernel takes them on a ZNIPPY_ROLES_MIN=1 context, so the second
    decode run is a lean one), and a frame of the same length with other content that the small-row kernels hand over: a
    skippable frame in front of the frame of 10 KiB of zeros."""
    import torch
    from znippy_amd import hip
    n = 6 * 40
    data = gen.text(10240)
    frame = workloads.libzstd_compress(data, 19)
    other = bytes(10240)
    zf = workloads.libzstd_compress(other, 19)
    pad = len(frame) - 8 - len(zf)
    assert pad >= 0
    other_frame = (0x184D2A50).to_bytes(4, "little") + pad.to_bytes(4, "little") + bytes(pad) + zf
    fl = len(frame)
    blob = np.concatenate([np.tile(np.frombuffer(frame, np.uint8), n), np.zeros(64, np.uint8)])
    ck = np.tile(np.frombuffer(ctx.blake3(data), dtype=np.uint8), (n, 1))
    total = n * 10240
    d_blobs = torch.from_numpy(blob).cuda()
    rt = hip.RowTable(ctx, np.arange(n, dtype=np.uint64) * np.uint64(fl), np.full(n, fl, np.uint64), np.full(n, 10240, np.uint64),
                      np.arange(n, dtype=np.uint64) * np.uint64(10240), None, ck)
    clean = dict(total_chunks=n, total_written_bytes=total, verified_bytes=total, corrupt_bytes=0, corrupt_rows=0, decode_errors=0)
    want = np.tile(np.frombuffer(data, np.uint8), n)
    want9 = want.copy()
    want9[9 * 10240:10 * 10240] = 0

    def change_row_9():
        d_blobs[9 * fl:10 * fl] = torch.from_numpy(np.frombuffer(other_frame, np.uint8).copy()).cuda()
        torch.cuda.synchronize()
    return rt, d_blobs, total, clean, want, want9, change_row_9


def test_run_sequence_of_every_kind_with_a_flagged_lean_run():
    """One table of a ZNIPPY_ROLES_MIN=1 context: decode (full), decode (lean), decode-only, verify-only, decode-only, decode — two
    buffers in turn, two runs in flight, read one run behind.  Before the last two runs one row's blob is damaged, so that the
    lean decode at the end comes back flagged and is repeated (and the decode-only run before it, as a decode-only run).  Every
    run's counters are its own, both buffers end complete, and a decode-only run writes only the buffer it was given."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = make_ctx({"ZNIPPY_ROLES_MIN": "1"})
    rt, d_blobs, total, clean, _, want9, change_row_9 = lean_table(ctx)
    bufs = [torch.full((total + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    kinds = ["decode", "decode", "plain", "verify", "plain", "decode"]
    got, names = [], []
    for k, kind in enumerate(kinds):
        if k == 4:
            ctx.sync()
            change_row_9()
        if k == 1:  # the second decode run is lean only if the first one's results have been seen
            got.append(rt.results_lagged(0))
        buf = bufs[k & 1]
        if kind == "decode":
            rt.decode_verify_async(d_blobs, buf)
        elif kind == "plain":
            rt.decode_async(d_blobs, buf)
        else:
            rt.verify_async(d_blobs)
        names.append(_names(ctx))
        if k >= 2:
            got.append(rt.results_lagged(1))
    got.append(rt.results_lagged(0))
    ctx.sync()
    assert len(got) == 6
    assert "decode_verify_roles" in names[0] and "blake3_second_pass" in names[0], sorted(names[0])
    assert "blake3_second_pass" not in names[1], sorted(names[1])                    # the lean run
    for k in (2, 4):
        assert_no_hash_kernel(names[k], k)
        assert "decode_small" in names[k], sorted(names[k])
    assert got[0] == got[1] == got[2] == got[3] == clean, got
    # row 9 now holds other content: the decode-only run reports what a table without checksums reports — everything decoded
    assert got[4] == clean, got[4]
    # ... and the decode run after it finds the mismatch (the row decodes, its digest is not the index's)
    assert got[5] == dict(clean, verified_bytes=total - 10240, corrupt_bytes=10240, corrupt_rows=1), got[5]
    h0, h1 = bufs[0].cpu().numpy(), bufs[1].cpu().numpy()
    assert np.array_equal(h0[:total], want9) and np.array_equal(h1[:total], want9)   # runs 4 and 5, both after the change
    assert bool((h0[total:] == SENTINEL).all()) and bool((h1[total:] == SENTINEL).all())
    # a decode-only run never writes a buffer it was not given
    bufs[1].fill_(0x3C)
    torch.cuda.synchronize()
    c, st = rt.decode(d_blobs, bufs[0])
    assert c == clean and (st == 0).all() and bool((bufs[1] == 0x3C).all().item())
    rt.close(); ctx.close()


def test_decode_only_run_is_repeated_as_one_behind_a_flagged_lean_run():
    """lean decode (flagged by a changed blob) with a decode-only run queued behind it, read with lag 1: rows_settle repeats both,
    the second again as a decode-only run — its counters stay a decode-only run's and digests() stays refused."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import _lib
    ctx = make_ctx({"ZNIPPY_ROLES_MIN": "1"})
    rt, d_blobs, total, clean, _, want9, change_row_9 = lean_table(ctx)
    bufs = [torch.full((total + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    assert rt.decode_verify(d_blobs, bufs[0])[0] == clean
    change_row_9()
    rt.decode_verify_async(d_blobs, bufs[0])      # lean: comes back flagged
    assert "blake3_second_pass" not in _names(ctx)
    rt.decode_async(d_blobs, bufs[1])
    a = rt.results_lagged(1)
    assert a == dict(clean, verified_bytes=total - 10240, corrupt_bytes=10240, corrupt_rows=1), a
    assert_no_hash_kernel(_names(ctx), "the repeat of the latest run")
    assert rt.results_lagged(0) == clean
    with pytest.raises(_lib.ZnippyError):
        rt.digests()
    for b in bufs:
        assert np.array_equal(b.cpu().numpy()[:total], want9)
    rt.close(); ctx.close()


# ---- 4. the ABI through ctypes --------------------------------------------------------------------------------------

def test_abi_of_the_decode_only_entry_points(gpu_ctx, oracle):
    import torch
    from znippy_amd import _lib
    from znippy_amd._lib import VerifyCounters
    L = _lib.lib()
    E_INVAL = _lib.E_INVAL
    for sym in ("znippy_decode_rows", "znippy_decode_rows_async"):
        assert hasattr(L, sym), sym
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    data = gen.text(10240)
    frame = oracle.libzstd_compress(data, 19)
    ck = (C.c_uint8 * 32).from_buffer_copy(oracle.blake3(data))
    d = torch.from_numpy(np.frombuffer(frame + bytes(64), np.uint8).copy()).cuda()
    dp = C.c_void_p(d.data_ptr())
    out = torch.full((2 * 10240 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    op = C.c_void_p(out.data_ptr())
    c = VerifyCounters()
    st = (C.c_int32 * 2)()
    clean1 = dict(total_chunks=1, total_written_bytes=10240, verified_bytes=10240, corrupt_bytes=0, corrupt_rows=0, decode_errors=0)
    # a table without output offsets is refused
    rows = C.c_void_p()
    assert L.znippy_rows_create(gpu_ctx.h, u64(0), u64(len(frame)), None, u64(10240), None, ck, 0, 1, C.byref(rows)) == 0
    assert L.znippy_decode_rows_async(gpu_ctx.h, rows, dp, 0, op, 10240) == E_INVAL
    assert L.znippy_decode_rows(gpu_ctx.h, rows, dp, 0, op, 10240, C.byref(c), st) == E_INVAL
    L.znippy_rows_destroy(rows)
    # NULL arguments; then the run, digests() refused after it and back after the next decode run
    rows = C.c_void_p()
    assert L.znippy_rows_create(gpu_ctx.h, u64(0), u64(len(frame)), None, u64(10240), u64(0), ck, 0, 1, C.byref(rows)) == 0
    assert L.znippy_decode_rows_async(gpu_ctx.h, rows, None, 0, op, 10240) == E_INVAL
    assert L.znippy_decode_rows_async(gpu_ctx.h, rows, dp, 0, None, 10240) == E_INVAL
    assert L.znippy_decode_rows(None, rows, dp, 0, op, 10240, C.byref(c), st) == E_INVAL
    assert L.znippy_decode_rows(gpu_ctx.h, None, dp, 0, op, 10240, C.byref(c), st) == E_INVAL
    assert L.znippy_decode_rows(gpu_ctx.h, rows, dp, 0, op, 10240, C.byref(c), st) == 0
    assert c.as_dict() == clean1 and st[0] == 0
    host = out.cpu().numpy()
    assert host[:10240].tobytes() == data and bool((host[10240:] == SENTINEL).all())
    digest = (C.c_uint8 * 32)()
    assert L.znippy_rows_digests(gpu_ctx.h, rows, digest) == E_INVAL
    assert L.znippy_decode_rows(gpu_ctx.h, rows, dp, 0, op, 10240, None, None) == 0      # counters and status are optional
    assert L.znippy_decode_verify_rows(gpu_ctx.h, rows, dp, 0, op, 10240, C.byref(c), None, 0, st) == 0
    assert L.znippy_rows_digests(gpu_ctx.h, rows, digest) == 0 and bytes(digest) == oracle.blake3(data)
    L.znippy_rows_destroy(rows)
    # out_cap one byte short, and a blob region that ends inside a row: the rows a decode run refuses, with its codes
    two = torch.from_numpy(np.frombuffer(frame + frame + bytes(64), np.uint8).copy()).cuda()
    tp = C.c_void_p(two.data_ptr())
    n = len(frame)
    for out_cap, blob_cap in ((2 * 10240 - 1, None), (2 * 10240, 2 * n - 1), (2 * 10240, 2 * n)):
        res = []
        for plain in (False, True):
            rows = C.c_void_p()
            assert L.znippy_rows_create(gpu_ctx.h, u64(0, n), u64(n, n), None, u64(10240, 10240), u64(0, 10240), None, 0, 2, C.byref(rows)) == 0
            if blob_cap is not None:
                assert L.znippy_rows_set_blob_cap(rows, blob_cap) == 0
            out.fill_(SENTINEL)
            torch.cuda.synchronize()
            if plain:
                assert L.znippy_decode_rows(gpu_ctx.h, rows, tp, 0, op, out_cap, C.byref(c), st) == 0
            else:
                assert L.znippy_decode_verify_rows(gpu_ctx.h, rows, tp, 0, op, out_cap, C.byref(c), None, 0, st) == 0
            res.append((c.as_dict(), [st[0], st[1]], out.cpu().numpy().copy()))
            L.znippy_rows_destroy(rows)
        assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and np.array_equal(res[0][2], res[1][2]), (out_cap, blob_cap, res[0][:2], res[1][:2])
        want_st = [0, _lib.E_DST_SMALL] if out_cap < 2 * 10240 else ([0, _lib.E_CORRUPT] if blob_cap == 2 * n - 1 else [0, 0])
        assert res[1][1] == want_st, (out_cap, blob_cap, res[1][1])
        assert bool((res[1][2][10240 if want_st[1] else 20480:] == SENTINEL).all())
    # an empty table works
    empty = C.c_void_p()
    assert L.znippy_rows_create(gpu_ctx.h, u64(0), u64(0), None, u64(0), u64(0), None, 0, 0, C.byref(empty)) == 0
    assert L.znippy_decode_rows(gpu_ctx.h, empty, None, 0, None, 0, C.byref(c), None) == 0 and c.total_chunks == 0
    L.znippy_rows_destroy(empty)
    # a table of another context, and a closed context
    ctx = C.c_void_p()
    assert L.znippy_ctx_create(0, None, C.byref(ctx)) == 0
    rows = C.c_void_p()
    assert L.znippy_rows_create(ctx, u64(0), u64(len(frame)), None, u64(10240), u64(0), ck, 0, 1, C.byref(rows)) == 0
    assert L.znippy_decode_rows_async(gpu_ctx.h, rows, dp, 0, op, 10240) == E_INVAL
    L.znippy_ctx_destroy(ctx)                      # the table is alive: the context is closed, not freed
    assert L.znippy_decode_rows_async(ctx, rows, dp, 0, op, 10240) == E_INVAL
    assert L.znippy_decode_rows(ctx, rows, dp, 0, op, 10240, C.byref(c), st) == E_INVAL
    L.znippy_rows_destroy(rows)


def test_python_table_keeps_the_buffers_of_its_last_two_decode_only_runs(gpu_ctx, oracle):
    import torch
    entries = [gen.text(10240), gen.incompressible(1, 3000), b"", gen.pseudo_text(20000, 3)]
    arch = build_archive(oracle, entries, level=3, skip=[0, 1, 0, 0])
    total = extent(arch)
    d_blobs = to_dev(arch["blobs"])
    rt = make_table(gpu_ctx, arch)
    outs = [torch.zeros(total + 64, dtype=torch.uint8, device="cuda") for _ in range(3)]
    for o in outs:
        rt.decode_async(d_blobs, o)
    assert sorted(rt._runs) == [1, 2] and rt._runs[2][1] is outs[2] and rt._runs[1][0] is d_blobs
    c = rt.results_lagged(1)
    assert sorted(rt._runs) == [2]
    c2, _, status = rt.results()
    assert rt._runs == {} and c == c2 and (status == 0).all() and c["verified_bytes"] == total
    for o in outs:
        assert o[:total].cpu().numpy().tobytes() == b"".join(entries)
    rt.close()
