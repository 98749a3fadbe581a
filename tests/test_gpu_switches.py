"""Every kernel-path switch (api.hip: read_switches) through the same cases.  The read side picks its kernels at run time —
size thresholds, the ZNIPPY_* switches a context reads when it is created, hints a table learns from its previous run — and
the default suite checks one point of that matrix.  Here a context is created under each switch set (the way the conftest
fixtures do it) and runs: a random damaged archive three times on one table (the later runs use what the first learned), the
mixed archive, foreign frames of the batch and resolve paths with damaged ones among them, a table without a compressed row,
a random write-side round table, and four lagged runs over two output buffers.  Expected results come from the oracle's read
and write loops (decompress.rs:L135-190, stream_packer.rs:L217-284) and do not depend on the switch.

Left out on purpose: ZNIPPY_FZ_ONLY (changes verdicts by design), NOHASH, the diagnostics (DBG, EDBG, TDBG, TRACE),
KTIME and LDS_PAD."""
import numpy as np
import pytest

import gen
import gpu_cases
from gpu_cases import build_archive, check_random_archive_run, make_ctx, oracle_rows, run_gpu

pytestmark = pytest.mark.gpu

SWITCH_SETS = [
    ("roles_min_1", {"ZNIPPY_ROLES_MIN": "1"}),
    ("roles_min_0", {"ZNIPPY_ROLES_MIN": "0"}),
    ("no_roles", {"ZNIPPY_NO_ROLES": "1"}),
    ("store_g_1", {"ZNIPPY_STORE_G": "1"}),
    ("store_g_2", {"ZNIPPY_STORE_G": "2"}),
    ("store_g_2+roles_min_1", {"ZNIPPY_STORE_G": "2", "ZNIPPY_ROLES_MIN": "1"}),
    ("no_lean", {"ZNIPPY_NO_LEAN": "1"}),
    ("no_bx", {"ZNIPPY_NO_BX": "1"}),
    ("no_bx+no_fz", {"ZNIPPY_NO_BX": "1", "ZNIPPY_NO_FZ": "1"}),
    ("no_fz", {"ZNIPPY_NO_FZ": "1"}),
    ("no_rx", {"ZNIPPY_NO_RX": "1"}),
    ("bx_big_1", {"ZNIPPY_BX_BIG": "1"}),
    ("no_pack", {"ZNIPPY_NO_PACK": "1"}),
    ("no_stored_only", {"ZNIPPY_NO_STORED_ONLY": "1"}),
    ("no_block_items", {"ZNIPPY_NO_BLOCK_ITEMS": "1"}),
    ("no_fused_blocks", {"ZNIPPY_NO_FUSED_BLOCKS": "1"}),
    ("no_fused_store", {"ZNIPPY_NO_FUSED_STORE": "1"}),
    ("no_fuse_hash", {"ZNIPPY_NO_FUSE_HASH": "1"}),
    ("gen_share_1", {"ZNIPPY_GEN_SHARE": "1"}),
    ("gen_share_4", {"ZNIPPY_GEN_SHARE": "4"}),
    ("ddbg", {"ZNIPPY_DDBG": "1"}),
]


@pytest.fixture(scope="module", params=SWITCH_SETS, ids=[s for s, _ in SWITCH_SETS])
def sw(request):
    """(name, context created under the switch set)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    name, env = request.param
    ctx = make_ctx(env)
    yield name, ctx
    ctx.close()


def _names(ctx):
    return set(dict(ctx.kernel_times()))


# ---- cases: built once per module (oracle side) -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def random_case(oracle):
    return gpu_cases.random_case(oracle)


@pytest.fixture(scope="module")
def mixed_case(oracle):
    return gpu_cases.mixed_case(oracle)


@pytest.fixture(scope="module")
def foreign_case(oracle):
    return gpu_cases.foreign_case(oracle)


@pytest.fixture(scope="module")
def store_case(oracle):
    return gpu_cases.store_case(oracle)


@pytest.fixture(scope="module")
def write_case(oracle):
    return gpu_cases.write_case(oracle)


@pytest.fixture(scope="module")
def pipeline_case(oracle):
    """Small text rows beside big stored rows, clean."""
    rng = np.random.default_rng(2)
    entries = [gen.text(int(rng.integers(1024, 12000))) for _ in range(700)] + [gen.incompressible(40 + i, (1 << 19) + 777 * i) for i in range(3)]
    skip = [0] * 700 + [1] * 3
    arch = build_archive(oracle, entries, level=19, skip=skip)
    return arch, oracle_rows(oracle, arch)


# ---- the matrix -------------------------------------------------------------------------------------------------------

def test_random_archive_three_runs_one_table(sw, random_case, oracle):
    name, ctx = sw
    arch, (want, want_corrupt, want_out) = random_case
    rt = None
    for rep in range(3):
        counters, corrupt, status, out, rt = run_gpu(ctx, arch, pad_blobs=3, rt=rt)
        names = _names(ctx)
        check_random_archive_run(arch, want, want_corrupt, want_out, counters, corrupt, status, out, rt, rep)
        dig = rt.digests()
        for i in [int(x) for x in want_corrupt]:   # a corrupt row's digest is the BLAKE3 of the bytes it decoded to
            a, b = int(arch["out_off"][i]), int(arch["out_off"][i] + arch["usize"][i])
            assert dig[i].tobytes() == oracle.blake3(want_out[a:b].tobytes()), (rep, i)
        if rep == 0 and "roles_min_1" in name:
            assert "decode_verify_roles" in names, sorted(names)
        if name in ("roles_min_0", "no_roles"):
            assert "decode_verify_roles" not in names, sorted(names)
    rt.close()


def test_mixed_archive(sw, mixed_case):
    name, ctx = sw
    arch, (want, want_corrupt, want_out) = mixed_case
    counters, corrupt, status, out, rt = run_gpu(ctx, arch, pad_blobs=5)
    assert (status == 0).all()
    assert counters == want
    assert len(corrupt) == 0 and len(want_corrupt) == 0
    assert np.array_equal(out, want_out)
    assert np.array_equal(out, arch["src"][:len(out)])
    assert np.array_equal(rt.digests(), arch["checksum"])
    rt.close()


def test_foreign_frames(sw, foreign_case):
    name, ctx = sw
    arch, (want, want_corrupt, want_out) = foreign_case
    rt = None
    for rep in range(2):
        counters, corrupt, status, out, rt = run_gpu(ctx, arch, rt=rt)
        names = _names(ctx)
        assert counters == want, (rep, counters, want)
        assert sorted(int(x) for x in corrupt) == sorted(int(x) for x in want_corrupt), rep
        ok = status >= 0
        assert int((~ok).sum()) == want["decode_errors"]
        for i in np.nonzero(ok)[0]:
            a, b = int(arch["out_off"][i]), int(arch["out_off"][i] + arch["usize"][i])
            assert np.array_equal(out[a:b], want_out[a:b]), (rep, int(i))
        good = ok.copy(); good[[int(x) for x in want_corrupt]] = False
        assert np.array_equal(rt.digests()[good], arch["checksum"][good]), rep
        if rep == 0:
            if name.startswith("no_bx"):
                assert "zstd_batch_execute" not in names, sorted(names)
                assert ("zstd_foreign_entropy" in names) == (name == "no_bx"), sorted(names)
            else:
                assert "zstd_batch_execute" in names, sorted(names)
                assert ("zstd_resolve_expand" in names) == (name != "no_rx"), sorted(names)
    rt.close()


def test_store_path(sw, store_case):
    import torch
    from znippy_amd import hip
    name, ctx = sw
    S = store_case
    d_blobs = torch.from_numpy(S["blobs"].copy()).cuda()
    bitmap = np.zeros((len(S["sizes"]) + 7) // 8, np.uint8)
    rt = hip.RowTable(ctx, S["bo"], S["bs"], S["bs"], S["oo"], bitmap, S["ck"])
    for rep in range(2):
        d_out = torch.full((S["total"],), 0xA5, dtype=torch.uint8, device="cuda")
        counters, corrupt, status = rt.decode_verify(d_blobs, d_out)
        assert (status == 0).all() and list(corrupt) == [S["bad_row"]], (rep, list(corrupt))
        assert counters["corrupt_rows"] == 1 and counters["verified_bytes"] == sum(S["sizes"]) - S["sizes"][S["bad_row"]]
        assert np.array_equal(d_out.cpu().numpy(), S["want"]), rep
        good = np.ones(len(S["sizes"]), bool); good[S["bad_row"]] = False
        assert np.array_equal(rt.digests()[good], S["ck"][good]), rep
        assert ("decode_verify_fused" in _names(ctx)) == (name == "no_stored_only")
    rt.close()


def test_write_side_round_table(sw, write_case, oracle):
    import torch
    from znippy_amd import hip
    name, ctx = sw
    entries, skip, digests = write_case
    lens = np.array([len(e) for e in entries], np.uint64)
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    total = int(lens.sum())
    d_src = torch.from_numpy(np.frombuffer(b"".join(entries) + bytes(64), np.uint8).copy()).cuda()
    rt = hip.RoundTable(ctx, offs, lens, np.array(skip, np.uint8))
    d_blob = torch.zeros(rt.blob_bound() + 64, dtype=torch.uint8, device="cuda")
    first = None
    for rep in range(2):
        d_blob.zero_()
        enc = rt.encode_hash(d_src, d_blob)
        hb = d_blob.cpu().numpy()
        got = (enc["blob_offset"].copy(), enc["blob_size"].copy(), enc["checksum"].copy(), hb[:int(enc["blob_bytes"])].copy())
        if first is None:
            first = got
            for i, e in enumerate(entries):
                f = hb[int(enc["blob_offset"][i]):int(enc["blob_offset"][i] + enc["blob_size"][i])].tobytes()
                assert enc["checksum"][i].tobytes() == digests[i], i
                if enc["compressed"][i]:
                    assert oracle.libzstd_decompress(f, max(len(e), 1)) == e, (i, len(e))
                else:
                    assert f == e, i
        else:
            assert all((a == b).all() for a, b in zip(got, first)), "the second run wrote something else"
    rows = hip.RowTable(ctx, enc["blob_offset"], enc["blob_size"], lens, offs,
                        np.packbits(enc["compressed"].astype(bool), bitorder="little"), enc["checksum"])
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    c, corrupt, st = rows.decode_verify(d_blob, d_out)
    names = _names(ctx)
    assert c["corrupt_rows"] == 0 and c["decode_errors"] == 0 and c["verified_bytes"] == total
    assert torch.equal(d_out[:total], d_src[:total])
    if name == "no_fused_blocks":
        assert "decode_verify_fused_blocks" not in names, sorted(names)
    if name == "no_block_items":
        assert "zstd_block_scan" not in names and "decode_verify_fused_blocks" not in names, sorted(names)
    rows.close()
    rt.close()


def test_lagged_pipeline(sw, pipeline_case):
    import torch
    from znippy_amd import hip
    name, ctx = sw
    arch, (want, want_corrupt, want_out) = pipeline_case
    total = int(arch["usize"].sum())
    d_blobs = torch.from_numpy(np.concatenate([arch["blobs"], np.zeros(64, np.uint8)])).cuda()
    outs = [torch.zeros(total + 64, dtype=torch.uint8, device="cuda") for _ in range(2)]
    rt = hip.RowTable(ctx, arch["blob_offset"], arch["blob_size"], arch["usize"], arch["out_off"],
                      np.packbits(arch["compressed"].astype(bool), bitorder="little"), arch["checksum"])
    got, full = [], []
    for k in range(4):
        outs[k & 1].zero_()
        rt.decode_verify_async(d_blobs, outs[k & 1])
        names = _names(ctx)
        full.append("zstd_decode_general" in names or "zstd_decode_fallback" in names)
        if k >= 1:
            got.append(rt.results_lagged(1))
            assert np.array_equal(outs[(k - 1) & 1][:total].cpu().numpy(), want_out), k - 1
    got.append(rt.results_lagged(0))
    assert np.array_equal(outs[1][:total].cpu().numpy(), want_out)
    assert got == [want] * 4, got
    if name == "no_lean":
        assert all(full), full
    rt.close()
