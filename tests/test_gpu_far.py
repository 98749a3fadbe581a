"""Offsets beyond 4 GiB on the read and write paths.  The C ABI takes 64-bit byte offsets everywhere (blob_offset, blob_base,
out_offset, out_cap, src_offset, the running blob_offset the write side returns) and the kernels carry many of them between
lanes as two 32-bit halves; the rest of the suite never hands a kernel an offset whose upper half is not zero.  Here the small
cases of test_gpu_switches.py / test_gpu_decode.py run again with the same bytes placed far away (gpu_cases.place): in two
device regions of 4 GiB + 96 MiB that are never initialised whole, with the 4 GiB line above, inside or at the start of a row
chosen for the kernel path it takes.  Expected results are the oracle's (layout-free); besides them the bytes around the line
are compared with the expected image and the bytes at the place a truncated offset would land (offset mod 4 GiB) must keep
their guard value.  L1 (a blob_base above 2^40, nothing big) runs in tests of its own, in front of everything far.
Far output (L2, L4) takes every placement for the stored-only tables and the placement above the line for tables with
compressed rows."""
import numpy as np
import pytest

import gpu_cases
from gpu_cases import FAR_LINE as T
from gpu_cases import make_ctx, oracle_rows, place

pytestmark = pytest.mark.gpu

FAR_BYTES = T + (96 << 20)
GUARD = 0xA5
HIGH_BASE = (1 << 40) + 12345
MIB = 1 << 20


# ---- regions, contexts ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def room():
    """Without room for the far regions every test that needs them is skipped."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    free, _ = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip(f"the far regions need 12 GiB of free device memory, {free >> 20} MiB are free")


@pytest.fixture(scope="module")
def far(room):
    """far_a, far_b: two uninitialised device regions of 4 GiB + 96 MiB."""
    import torch
    a = torch.empty(FAR_BYTES, dtype=torch.uint8, device="cuda")
    b = torch.empty(FAR_BYTES, dtype=torch.uint8, device="cuda")
    yield a, b
    del a, b
    torch.cuda.empty_cache()


CONTEXTS = {
    "default": {},
    "roles_min_1": {"ZNIPPY_ROLES_MIN": "1"},
    "no_bx": {"ZNIPPY_NO_BX": "1"},
    "no_bx+no_fz": {"ZNIPPY_NO_BX": "1", "ZNIPPY_NO_FZ": "1"},
    "no_rx": {"ZNIPPY_NO_RX": "1"},
    "store_g_1": {"ZNIPPY_STORE_G": "1"},
    "store_g_2": {"ZNIPPY_STORE_G": "2"},
    "no_stored_only": {"ZNIPPY_NO_STORED_ONLY": "1"},
    "no_pack": {"ZNIPPY_NO_PACK": "1"},
}


@pytest.fixture(scope="module")
def ctxs():
    """name -> context created under that switch set, one per module."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = {}

    def get(name):
        if name not in made:
            made[name] = make_ctx(CONTEXTS[name])
        return made[name]
    yield get
    for c in made.values():
        c.close()


# ---- cases: the oracle side, built once per module ----------------------------------------------------------------------

class Case:
    """arch: the columns and blobs; want / want_corrupt: the oracle's counters and corrupt list; img: the oracle's output
    image from offset 0 (guard value where no row lies); picks: label -> row chosen for the kernel path it takes."""

    def __init__(self, oracle, arch, picks):
        self.arch = arch
        us, oo = arch["usize"], arch["out_off"]
        self.n = len(us)
        self.extent = int((oo + us).max())
        self.want, self.want_corrupt, self.img = oracle_rows(oracle, arch, extent=self.extent, fill=GUARD)
        self.want_corrupt = sorted(int(x) for x in self.want_corrupt)
        self.corrupt_digest = {i: oracle.blake3(self.img[int(oo[i]):int(oo[i] + us[i])].tobytes()) for i in self.want_corrupt}
        self.failed = [i for i in range(self.n) if arch["compressed"][i] and not self._decodes(oracle, i)]   # per row, by the oracle's decoder
        assert len(self.failed) == self.want["decode_errors"]
        self.has_compressed = bool(arch["compressed"].any())
        self.W = max(self.extent, len(arch["blobs"])) + MIB
        assert self.extent < 40 * MIB
        self.picks = {k: int(v) for k, v in picks.items()}
        self.bitmap = np.packbits(arch["compressed"].astype(bool), bitorder="little")
        self._dev = None

    def _decodes(self, oracle, i):
        A = self.arch
        frame = A["blobs"][int(A["blob_offset"][i]):int(A["blob_offset"][i] + A["blob_size"][i])].tobytes()
        try:
            return len(oracle.zstd_decompress(frame, cap=int(A["usize"][i]))) == int(A["usize"][i])
        except ValueError:
            return False

    def dev(self):
        """(blobs + 64 zero bytes, image) on the device."""
        import torch
        if self._dev is None:
            blobs = np.concatenate([self.arch["blobs"], np.zeros(64, np.uint8)])
            self._dev = torch.from_numpy(blobs).cuda(), torch.from_numpy(self.img.copy()).cuda()
        return self._dev

    def back_to_back(self):
        """Rows and blobs each behind the one before: the table zn_rows_pack32 accepts (the device rebuilds its columns)."""
        A = self.arch
        return (self.n >= 64 and np.array_equal(A["blob_offset"][1:], (A["blob_offset"] + A["blob_size"])[:-1]) and
                np.array_equal(A["out_off"][1:], (A["out_off"] + A["usize"])[:-1]))


def _first(mask, what):
    idx = np.nonzero(mask)[0]
    assert len(idx), f"the case holds no {what}"
    return int(idx[0])


def _own_archive(oracle, ctx, entries):
    """entries written by this library's encoder; the checksum column is the oracle's."""
    import torch
    from znippy_amd import hip
    src = np.frombuffer(b"".join(entries) + bytes(64), dtype=np.uint8)
    lens = np.array([len(e) for e in entries], dtype=np.uint64)
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    rounds = hip.RoundTable(ctx, offs, lens)
    d_blob = torch.zeros(rounds.blob_bound() + 64, dtype=torch.uint8, device="cuda")
    enc = rounds.encode_hash(torch.from_numpy(src.copy()).cuda(), d_blob)
    arch = dict(blobs=d_blob[:int(enc["blob_bytes"])].cpu().numpy(), blob_offset=enc["blob_offset"].copy(),
                blob_size=enc["blob_size"].copy(), usize=lens, out_off=offs, compressed=np.ones(len(entries), np.uint8),
                checksum=np.stack([np.frombuffer(oracle.blake3(e), dtype=np.uint8) for e in entries]))
    rounds.close()
    return arch


def _build_case(name, oracle, ctxs):
    if name == "random":
        arch, _ = gpu_cases.random_case(oracle)
        c, us = arch["compressed"].astype(bool), arch["usize"]
        case = Case(oracle, arch, {})
        clean = np.ones(case.n, bool); clean[case.want_corrupt] = False
        case.picks = dict(small_compressed=_first(c & (us == 10240) & clean, "10 KiB compressed row"),
                          small_stored=_first(~c & (us >= 256) & (us < 65536) & clean, "small stored row"),
                          big_stored=_first(~c & (us > 65536), "stored row above 64 KiB"),
                          damaged=_first(~clean & (us >= 256), "damaged row"))
        return case
    if name == "mixed":
        arch, _ = gpu_cases.mixed_case(oracle)
        c, us = arch["compressed"].astype(bool), arch["usize"]
        return Case(oracle, arch, dict(multi_block=_first(c & (us >= 2 * MIB), "multi-block frame"),
                                       big_stored=_first(~c & (us > 65536), "stored row above 64 KiB")))
    if name == "foreign":
        arch, _ = gpu_cases.foreign_case(oracle)
        us = arch["usize"]
        return Case(oracle, arch, dict(libzstd_10k=_first(us == 10240, "10 KiB libzstd row"),
                                       foreign_mid=_first((us > 65536) & (us <= 131072), "foreign row of 64-256 KiB"),
                                       libzstd_multi_block=_first((us > 131072) & (us < 262144), "libzstd multi-block row"),
                                       foreign_big=_first(us >= 262144, "foreign row of 256 KiB or more")))
    if name == "store":
        S = gpu_cases.store_case(oracle)
        arch = dict(blobs=S["blobs"], blob_offset=S["bo"], blob_size=S["bs"], usize=S["bs"], out_off=S["oo"],
                    compressed=np.zeros(len(S["sizes"]), np.uint8), checksum=S["ck"])
        case = Case(oracle, arch, dict(small_stored=_first(S["bs"] == 10240, "small stored row"),
                                       big_stored=_first(S["bs"] > MIB, "stored row above 64 KiB"), damaged=S["bad_row"]))
        assert np.array_equal(case.img, S["want"][:case.extent]) and case.want_corrupt == [S["bad_row"]]
        return case
    if name == "store_packed":      # the same stored rows back to back: a stored-only table that zn_rows_pack32 accepts
        S = gpu_cases.store_case(oracle)
        arch = dict(blobs=S["blobs"], blob_offset=S["bo"], blob_size=S["bs"], usize=S["bs"], out_off=S["bo"].copy(),
                    compressed=np.zeros(len(S["sizes"]), np.uint8), checksum=S["ck"])
        case = Case(oracle, arch, dict(small_stored=_first(S["bs"] == 10240, "small stored row"),
                                       big_stored=_first(S["bs"] > MIB, "stored row above 64 KiB"), damaged=S["bad_row"]))
        assert case.back_to_back() and case.want_corrupt == [S["bad_row"]]
        return case
    if name == "big_rows":
        entries = gpu_cases.big_rows_entries()
        arch = _own_archive(oracle, ctxs("default"), entries)
        ent = [i for i, e in enumerate(entries) if e == gpu_cases.gen.pseudo_text(3 * gpu_cases.BLK + 5, seed=10)]
        return Case(oracle, arch, dict(periodic_blocks=_first(arch["usize"] == 8 * gpu_cases.BLK, "multi-block periodic row"),
                                       entropy_blocks=ent[0]))
    if name == "periodic":
        entries = gpu_cases.periodic_rows_entries()
        arch = gpu_cases.build_archive(oracle, entries, level=19)
        us = arch["usize"]
        per = np.arange(len(entries)) < 46
        case = Case(oracle, arch, dict(periodic_leaves=_first(per & (us % 1024 == 0) & (us >= 4096), "whole-leaf periodic row"),
                                       periodic_ragged=_first(per & (us % 1024 != 0) & (us >= 4096), "ragged periodic row"),
                                       text_10k=_first(us == 10240, "10 KiB text row")))
        assert case.back_to_back()
        return case
    raise KeyError(name)


@pytest.fixture(scope="module")
def cases(oracle, ctxs):
    built = {}

    def get(name):
        if name not in built:
            built[name] = _build_case(name, oracle, ctxs)
        return built[name]
    return get


# (context, case, kernel names the first run must show, names it must not show)
PAIRS = [
    ("default", "random", {"decode_verify_fused"}, set()),
    ("default", "mixed", {"decode_verify_fused", "blake3_second_pass"}, set()),
    ("default", "foreign", {"zstd_batch_execute", "zstd_resolve_expand"}, set()),
    ("default", "store", {"blake3_second_pass"}, {"decode_verify_fused"}),
    ("default", "big_rows", {"decode_verify_fused_blocks", "zstd_block_scan", "zstd_decode_blocks"}, set()),
    ("default", "periodic", {"decode_verify_fused"}, set()),
    ("roles_min_1", "random", {"decode_verify_roles"}, set()),
    ("roles_min_1", "periodic", {"decode_verify_roles"}, set()),
    ("no_bx", "foreign", {"zstd_foreign_entropy", "zstd_foreign_execute"}, {"zstd_batch_execute"}),
    ("no_bx+no_fz", "foreign", {"zstd_decode_general"}, {"zstd_batch_execute", "zstd_foreign_entropy"}),
    ("no_bx+no_fz", "big_rows", {"zstd_decode_general"}, {"zstd_batch_execute", "zstd_foreign_entropy"}),
    ("no_rx", "foreign", {"zstd_batch_execute"}, {"zstd_resolve_expand"}),
    ("store_g_1", "store", {"blake3_second_pass"}, {"decode_verify_fused"}),
    ("store_g_2", "store", {"blake3_second_pass"}, {"decode_verify_fused"}),
    ("no_stored_only", "store", {"decode_verify_fused"}, set()),
    ("no_pack", "periodic", {"decode_verify_fused"}, set()),
    ("default", "store_packed", {"blake3_second_pass"}, {"decode_verify_fused"}),   # the unpack kernels with far output (oo0, running sum)
    ("no_pack", "store_packed", {"blake3_second_pass"}, {"decode_verify_fused"}),
]
PAIR_IDS = [f"{c}-{k}" for c, k, _, _ in PAIRS]


# ---- one layout: a table, five runs, every check ------------------------------------------------------------------------

def _u64(col, add):
    return (col.astype(np.uint64) + np.uint64(add)).astype(np.uint64)


def _diff_at(got, exp):
    return int((got != exp).nonzero()[0][0])


def _gpu(what, fn):
    """A HIP error ends the session: after a GPU fault nothing more is started on that GPU."""
    from znippy_amd._lib import E_HIP, ZnippyError
    try:
        return fn()
    except ZnippyError as e:
        if e.code == E_HIP:
            pytest.exit(f"{what}: {e}", returncode=3)
        raise


def _run_layout(ctx, case, far, tag, out_shift, blob_shift, base, need, never):
    """out_shift / blob_shift None: that side in an ordinary buffer of its own size.  Returns the first run's kernel names."""
    import torch
    from znippy_amd import hip
    from znippy_amd._lib import E_INVAL, ZnippyError
    A, W, ext = case.arch, case.W, case.extent
    d_near_blobs, d_img = case.dev()
    nb = d_near_blobs.numel()
    far_a, far_b = far if far is not None else (None, None)
    us, oo0 = A["usize"], A["out_off"]
    if blob_shift is None:
        d_blobs, bshift = d_near_blobs, 0
    else:
        assert T - W <= blob_shift and blob_shift + nb <= T + W, tag
        far_b[blob_shift:blob_shift + nb] = d_near_blobs
        d_blobs, bshift = far_b, blob_shift
    if out_shift is None:
        d_out, oshift, pos = torch.empty(ext + 64, dtype=torch.uint8, device="cuda"), 0, 0
        exp = torch.full((ext + 64,), GUARD, dtype=torch.uint8, device="cuda")
    else:
        assert T - W <= out_shift and out_shift + ext <= T + W, tag
        d_out, oshift, pos = far_a, out_shift, out_shift - (T - W)
        exp = torch.full((2 * W,), GUARD, dtype=torch.uint8, device="cuda")
    exp[pos:pos + ext] = d_img
    guard_w = torch.full((W,), GUARD, dtype=torch.uint8, device="cuda")
    rt = hip.RowTable(ctx, _u64(A["blob_offset"], base + bshift), A["blob_size"], us, _u64(oo0, oshift), case.bitmap, A["checksum"])

    def prep():
        if out_shift is None:
            d_out.fill_(GUARD)
        else:
            far_a[0:W].fill_(GUARD)
            far_a[T - W:T + W].fill_(GUARD)
        if blob_shift is not None:
            far_b[0:W].zero_()

    def check_bytes(status, what, written=True):
        got = d_out if out_shift is None else far_a[T - W:T + W]
        want_img = exp if written else torch.full_like(exp, GUARD)
        if written:
            for i in np.nonzero(status < 0)[0]:      # a row that failed to decode: its own bytes are not compared, its neighbours' are
                a = pos + int(oo0[i])
                got[a:a + int(us[i])] = exp[a:a + int(us[i])]
        if not torch.equal(got, want_img):
            at = _diff_at(got, want_img)
            where = at if out_shift is None else T - W + at
            raise AssertionError(f"{tag} {what}: output differs from the expected image at byte {where} (line at {T})")
        if out_shift is not None and not torch.equal(far_a[0:W], guard_w):
            at = _diff_at(far_a[0:W], guard_w)
            raise AssertionError(f"{tag} {what}: stray write at byte {at}, where an offset cut to 32 bits lands")

    def check_results(counters, corrupt, status, what, want):
        assert counters == want, (tag, what, counters, want)
        assert sorted(int(x) for x in corrupt) == (case.want_corrupt if want is case.want else []), (tag, what)
        assert [int(i) for i in np.nonzero(status < 0)[0]] == case.failed, (tag, what)   # the rows the oracle could not decode

    def check_digests(status, what):
        dig = rt.digests()
        good = status >= 0
        good[case.want_corrupt] = False
        assert np.array_equal(dig[good], A["checksum"][good]), (tag, what)
        for i, d in case.corrupt_digest.items():      # a corrupt row's digest is the BLAKE3 of the bytes it decoded to
            assert dig[i].tobytes() == d, (tag, what, i)

    def run(what, fn):
        return _gpu(f"{tag} {what}", fn)

    kw = dict(blob_base=base, blob_cap=d_blobs.numel())
    names, status0 = None, None
    for rep in range(3):                              # the second and third are lean runs where the table allows
        prep()
        counters, corrupt, status = run(f"run {rep}", lambda: rt.decode_verify(d_blobs, d_out, out_cap=d_out.numel(), **kw))
        status = status.copy()
        if rep == 0:
            names, status0 = set(dict(ctx.kernel_times())), status
            assert need <= names and not (never & names), (tag, sorted(names))
        assert np.array_equal(status, status0), (tag, rep)
        check_results(counters, corrupt, status, f"run {rep}", case.want)
        check_digests(status, f"run {rep}")
        check_bytes(status, f"run {rep}")
    prep()                                            # verify-only: the results of a decode run, and no output
    counters, corrupt, status = run("verify-only", lambda: rt.verify(d_blobs, **kw))
    assert np.array_equal(status, status0), tag
    check_results(counters, corrupt, status, "verify-only", case.want)
    check_digests(status.copy(), "verify-only")
    check_bytes(status, "verify-only", written=False)
    prep()                                            # decode-only: the same bytes, the counters of a table without checksums
    counters, status = run("decode-only", lambda: rt.decode(d_blobs, d_out, out_cap=d_out.numel(), **kw))
    assert np.array_equal(status, status0), tag
    plain = dict(case.want, verified_bytes=case.want["total_written_bytes"], corrupt_bytes=0, corrupt_rows=0)
    check_results(counters, [], status, "decode-only", plain)
    check_bytes(status.copy(), "decode-only")
    with pytest.raises(ZnippyError) as ei:
        rt.digests()
    assert ei.value.code == E_INVAL
    rt.close()
    return names


def _straddle_row(sizes, k):
    """k, or the nearest row long enough to hold the line (place needs 256 bytes)."""
    ok = np.nonzero(sizes >= 256)[0]
    return int(ok[np.argmin(np.abs(ok - k))])


def _modes(case, offsets, sizes):
    """(tag, shift) of every placement of one offset column: above, then the line inside and at the start of every pick,
    then — where rows are not aligned — the line exactly at the start of the nearest row whose offset allows it."""
    out = [("above", place(offsets, sizes, "above"))]
    for label, k in case.picks.items():
        out.append((f"straddle({label})", place(offsets, sizes, "straddle", _straddle_row(sizes, k))))
        out.append((f"start_at_line({label})", place(offsets, sizes, "start_at_line", k)))
    k0 = next(iter(case.picks.values()))
    if int(offsets[k0]) % 128:
        al = np.nonzero((offsets % np.uint64(128) == 0) & (sizes > 0))[0]
        if len(al):
            k = int(al[np.argmin(np.abs(al - k0))])
            out.append((f"start_at_line(row {k}, exact)", place(offsets, sizes, "start_at_line", k)))
    return out


@pytest.mark.parametrize("ctx_name,case_name,need,never", PAIRS, ids=PAIR_IDS)
def test_read_high_base(ctxs, cases, oracle, ctx_name, case_name, need, never):
    """L1: blob_base = 2^40 + 12345 added to every blob_offset, nothing else moves (offA - baseA on its own)."""
    case = cases(case_name)
    names = _run_layout(ctxs(ctx_name), case, None, f"{ctx_name}/{case_name} L1", None, None, HIGH_BASE, need, never)
    print(f"FAR {ctx_name}/{case_name}: L1 high base; kernels {sorted(names)}")


@pytest.mark.parametrize("ctx_name,case_name,need,never", PAIRS, ids=PAIR_IDS)
def test_read_far(far, ctxs, cases, oracle, ctx_name, case_name, need, never):
    """L2 far output, L3 far blobs, L4 both with L1's base — every placement of the case's picks (far output of tables
    with compressed rows: above the line)."""
    case, ctx = cases(case_name), ctxs(ctx_name)
    if ctx_name == "no_pack" or case_name in ("periodic", "store_packed"):
        assert case.back_to_back()
    A = case.arch
    ran = []
    for tag, s in _modes(case, A["out_off"], A["usize"])[:1 if case.has_compressed else None]:
        _run_layout(ctx, case, far, f"{ctx_name}/{case_name} L2 {tag}", s, None, 0, need, never)
        ran.append(f"L2 {tag}")
    for tag, s in _modes(case, A["blob_offset"], A["blob_size"]):
        names = _run_layout(ctx, case, far, f"{ctx_name}/{case_name} L3 {tag}", None, s, 0, need, never)
        ran.append(f"L3 {tag}")
    label, k = next(iter(case.picks.items()))
    both = [("above", place(A["out_off"], A["usize"], "above"), place(A["blob_offset"], A["blob_size"], "above")),
            (f"straddle({label})", place(A["out_off"], A["usize"], "straddle", _straddle_row(A["usize"], k)),
             place(A["blob_offset"], A["blob_size"], "straddle", _straddle_row(A["blob_size"], k)))]
    for tag, so, sb in both[:1 if case.has_compressed else None]:
        names = _run_layout(ctx, case, far, f"{ctx_name}/{case_name} L4 {tag}", so, sb, HIGH_BASE, need, never)
        ran.append(f"L4 {tag}")
    print(f"FAR {ctx_name}/{case_name}: {len(ran)} layouts: {'; '.join(ran)}; kernels {sorted(names)}")


# ---- write side ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wcase(oracle):
    entries, skip, digests = gpu_cases.write_case(oracle)
    lens = np.array([len(e) for e in entries], np.uint64)
    offs = (np.cumsum(lens) - lens).astype(np.uint64)
    src = np.frombuffer(b"".join(entries) + bytes(64), np.uint8).copy()
    return dict(entries=entries, skip=np.array(skip, np.uint8), digests=np.stack([np.frombuffer(d, np.uint8) for d in digests]),
                lens=lens, offs=offs, src=src, total=int(lens.sum()))


def _near_encode(ctx, wc, oracle, d_src):
    """The write case with its source at offset 0: columns, blob bytes (device), every frame checked against its entry."""
    import torch
    from znippy_amd import hip
    rt = hip.RoundTable(ctx, wc["offs"], wc["lens"], wc["skip"])
    d_blob = torch.zeros(rt.blob_bound() + 64, dtype=torch.uint8, device="cuda")
    enc = _gpu("near encode", lambda: rt.encode_hash(d_src, d_blob))
    bo, bs, ck, comp, nbytes = (enc["blob_offset"].copy(), enc["blob_size"].copy(), enc["checksum"].copy(), enc["compressed"].copy(),
                                int(enc["blob_bytes"]))
    rt.close()
    assert np.array_equal(ck, wc["digests"])
    assert np.array_equal(bo, np.cumsum(bs) - bs) and nbytes == int(bs.sum())
    hb = d_blob[:nbytes].cpu().numpy()
    for i, e in enumerate(wc["entries"]):
        f = hb[int(bo[i]):int(bo[i] + bs[i])].tobytes()
        if comp[i]:
            assert oracle.libzstd_decompress(f, max(len(e), 1)) == e, (i, len(e))
        else:
            assert f == e, i
    return bo, bs, comp, d_blob[:nbytes].clone()


@pytest.mark.parametrize("level,window_log", [(1, 0), (19, 0), (19, 23)], ids=["level1", "level19", "level19-window23"])
def test_write_far_source(far, wcase, oracle, level, window_log):
    """src_offset beyond the line: digests, columns and blob bytes are those of the same rounds with the source at 0."""
    import torch
    from znippy_amd import hip
    _, far_b = far
    wc = wcase
    ctx = make_ctx({})
    ctx.set_level(level)
    ctx.set_window_log(window_log)
    d_src = torch.from_numpy(wc["src"]).cuda()
    bo, bs, comp, near = _near_encode(ctx, wc, oracle, d_src)
    lens, offs, skip = wc["lens"], wc["offs"], wc["skip"]
    W = wc["total"] + MIB
    k_enc = _first((skip == 0) & (lens > 128 * 1024), "encoded multi-block round")
    k_store = _first((skip == 1) & (lens >= 256), "store-path round")
    for tag, s in (("above", place(offs, lens, "above")), ("straddle(encoded)", place(offs, lens, "straddle", k_enc)),
                   ("straddle(stored)", place(offs, lens, "straddle", k_store))):
        far_b[0:W].zero_()
        far_b[s:s + d_src.numel()] = d_src
        rt = hip.RoundTable(ctx, _u64(offs, s), lens, skip)
        d_blob = torch.zeros(rt.blob_bound() + 64, dtype=torch.uint8, device="cuda")
        enc = _gpu(f"far source {tag} level {level}", lambda: rt.encode_hash(far_b, d_blob))
        assert np.array_equal(enc["checksum"], wc["digests"]), tag
        assert np.array_equal(enc["blob_offset"], bo) and np.array_equal(enc["blob_size"], bs), tag
        assert int(enc["blob_bytes"]) == near.numel() and torch.equal(d_blob[:near.numel()], near), tag
        assert not d_blob[near.numel():].any(), tag
        assert np.array_equal(_gpu(f"far hash {tag}", lambda: rt.hash(far_b)), wc["digests"]), tag
        rt.close()
    print(f"FAR write source level {level} window_log {window_log}: above; straddle(encoded round {k_enc}); straddle(stored round {k_store})")
    ctx.close()


FILL = 64 * MIB


@pytest.mark.parametrize("how", ["straddle", "start_at_line"])
def test_write_far_blob_and_read_back(far, wcase, oracle, how):
    """The running blob_offset crosses the line: 64 store-path rounds over one 64 MiB slice push the write case's frames up to
    it, one frame lies across it (or begins on it).  Then the frames are read back from there: blob_offset beyond the line,
    output in the other far region above the line."""
    import torch
    from znippy_amd import hip
    far_a, far_b = far
    wc = wcase
    ctx = make_ctx({})
    lens, offs, skip, total = wc["lens"], wc["offs"], wc["skip"], wc["total"]
    filler = np.random.default_rng(77).integers(0, 256, FILL, dtype=np.uint8)
    d_src = torch.from_numpy(np.concatenate([filler, wc["src"]])).cuda()
    bo, bs, comp, near = _near_encode(ctx, wc, oracle, d_src[FILL:])
    j = _first((skip == 0) & (lens > 128 * 1024) & (bo > 0), "encoded multi-block round")
    X = int(bo[j]) + (int(bs[j]) // 2 if how == "straddle" else 0)
    assert 0 < X < FILL
    ln = np.concatenate([np.full(63, FILL, np.uint64), [np.uint64(FILL - X)], lens]).astype(np.uint64)
    so = np.concatenate([np.zeros(64, np.uint64), _u64(offs, FILL)]).astype(np.uint64)
    sk = np.concatenate([np.ones(64, np.uint8), skip])
    rt = hip.RoundTable(ctx, so, ln, sk)
    assert rt.blob_bound() <= far_a.numel()
    far_a[T - FILL:].fill_(GUARD)
    enc = _gpu(f"far blob output {how}", lambda: rt.encode_hash(d_src, far_a))
    ebo, ebs, eck, nbytes = enc["blob_offset"].copy(), enc["blob_size"].copy(), enc["checksum"].copy(), int(enc["blob_bytes"])
    rt.close()
    assert np.array_equal(ebs, np.concatenate([ln[:64], bs])) and np.array_equal(ebo, np.cumsum(ebs) - ebs)
    assert nbytes == T - X + near.numel() and nbytes > T
    assert int(ebo[64 + j]) < T < int(ebo[64 + j] + ebs[64 + j]) if how == "straddle" else int(ebo[64 + j]) == T
    whole, cut = oracle.blake3(filler.tobytes()), oracle.blake3(filler[:FILL - X].tobytes())
    assert all(eck[i].tobytes() == whole for i in range(63)) and eck[63].tobytes() == cut
    assert np.array_equal(eck[64:], wc["digests"])
    for i in range(63):
        assert torch.equal(far_a[i * FILL:(i + 1) * FILL], d_src[:FILL]), i
    assert torch.equal(far_a[63 * FILL:T - X], d_src[:FILL - X])
    assert torch.equal(far_a[T - X:nbytes], near), "the frames around the line differ from the near run's"
    assert bool((far_a[nbytes:] == GUARD).all()), "bytes behind blob_bytes were written"
    # close the loop: read the frames back from beyond the line
    bitmap = np.packbits(comp.astype(bool), bitorder="little")
    s, W = place(offs, lens, "above"), total + MIB
    far_b[0:W].fill_(GUARD)
    far_b[T:T + W].fill_(GUARD)
    rows = hip.RowTable(ctx, ebo[64:], ebs[64:], lens, _u64(offs, s), bitmap, eck[64:])
    c, corrupt, status = _gpu(f"read back {how}", lambda: rows.decode_verify(far_a, far_b))
    assert (status == 0).all() and len(corrupt) == 0
    assert c["corrupt_rows"] == 0 and c["decode_errors"] == 0 and c["verified_bytes"] == total
    assert np.array_equal(rows.digests(), wc["digests"])
    assert torch.equal(far_b[s:s + total], d_src[FILL:FILL + total])
    assert bool((far_b[T:s] == GUARD).all()) and bool((far_b[s + total:T + W] == GUARD).all())
    assert bool((far_b[0:W] == GUARD).all()), "stray write where an offset cut to 32 bits lands"
    names = sorted(dict(ctx.kernel_times()))
    rows.close()
    print(f"FAR write blob {how}: X={X}, frame {j} at {int(ebo[64 + j])}+{int(ebs[64 + j])}, blob_bytes={nbytes}; read back: {names}")
    ctx.close()
