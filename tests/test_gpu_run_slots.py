"""Two runs in flight on two slots of per-run device state (csrc/api.hip: control block, digest column and corrupt list per
slot; a lean run's verify queued on the auxiliary stream beside the next run, run_verify).  Every case runs with the default
ordering and with the switch that gives the in-line ordering back (ZNIPPY_NO_FORK_VERIFY), on the smallest tables that reach
the code: 48 rows of the recognised
periodic shape (8 tiles of the 6 x 10 shape: two groups of the role-split kernel, forced by ZNIPPY_ROLES_MIN=1) and the
same table with a 3-leaf row and a stored row mixed in (never lean: full runs).  Expected counters, corrupt lists and bytes
are the oracle's restated read loop's (decompress.rs:L113-192) over the same blobs."""
import numpy as np
import pytest

import gen
from gpu_cases import make_ctx

pytestmark = pytest.mark.gpu

SZ = 10240
SWITCHES = [{}, {"ZNIPPY_NO_FORK_VERIFY": "1"}]
IDS = ["default", "no_fork_verify"]


class Arch:
    """Rows in blob slots of one size (a row can be damaged and restored in place); the oracle's results per blob image."""

    def __init__(self, oracle, entries, comp):
        self.O = oracle
        self.entries, self.n = entries, len(entries)
        self.frames = [oracle.libzstd_compress(e, 19) if c else e for e, c in zip(entries, comp)]
        self.slot = max(len(f) for f in self.frames) + 9
        self.bo = np.arange(self.n, dtype=np.uint64) * np.uint64(self.slot)
        self.bs = np.array([len(f) for f in self.frames], np.uint64)
        self.us = np.array([len(e) for e in entries], np.uint64)
        self.oo = (np.cumsum(self.us) - self.us).astype(np.uint64)
        self.comp = np.array(comp, np.uint8)
        self.bitmap = np.packbits(self.comp.astype(bool), bitorder="little")
        dig = {}
        for e in entries:
            if e not in dig:
                dig[e] = np.frombuffer(oracle.blake3(e), dtype=np.uint8)
        self.ck = np.stack([dig[e] for e in entries])
        self.total = int(self.us.sum())
        self.blob = np.zeros(self.n * self.slot + 64, np.uint8)
        for i, f in enumerate(self.frames):
            self.blob[i * self.slot:i * self.slot + len(f)] = np.frombuffer(f, np.uint8)
        self.clean_bytes = np.frombuffer(b"".join(entries), np.uint8)
        # a frame of another shape (entropy-coded literals and sequences): the role-split kernel's recogniser refuses it
        self.other = np.frombuffer(oracle.libzstd_compress(gen.pseudo_text(SZ, seed=5), 3), np.uint8)
        self._want = {}

    def damage_at(self, row):  # a byte of the row's sequence section (stored rows: of its content)
        return row * self.slot + 20

    def foreign(self, row):  # (where, bytes): the row's blob as the head of the other frame — as long as the table says the blob is
        assert len(self.other) > int(self.bs[row])
        return row * self.slot, self.other[:int(self.bs[row])]

    def want(self, damaged=(), n_rows=None, onto=None, foreign=()):
        """Oracle over the blobs with the given rows damaged / replaced by the other frame: (counters, sorted corrupt list,
        output image).  The image starts as `onto` (what a buffer held before the run; default: the clean rows)."""
        key = (tuple(damaged), n_rows, None if onto is None else onto.tobytes(), tuple(foreign))
        if key not in self._want:
            blob = self.blob.copy()
            for r in damaged:
                blob[self.damage_at(r)] ^= 0x55
            for r in foreign:
                at, b = self.foreign(r)
                blob[at:at + len(b)] = b
            out = (self.clean_bytes if onto is None else onto).copy()
            c, corrupt = self.O.decompress_rows(blob, self.bo, self.bs, self.us, self.oo, self.bitmap, self.ck, 0,
                                                self.n if n_rows is None else n_rows, out=out)
            self._want[key] = (dict(c), [int(x) for x in corrupt], out)
        return self._want[key]

    def table(self, ctx):
        from znippy_amd import hip
        return hip.RowTable(ctx, self.bo, self.bs, self.us, self.oo, self.bitmap, self.ck)

    def d_blob(self):
        import torch
        return torch.from_numpy(self.blob.copy()).cuda()

    def d_out(self, fill=0):
        import torch
        return torch.full((self.total + 64,), fill, dtype=torch.uint8, device="cuda")


@pytest.fixture(scope="module")
def periodic(oracle):
    return Arch(oracle, [gen.text(SZ)] * 48, [1] * 48)


@pytest.fixture(scope="module")
def mixed(oracle):
    entries = [gen.text(SZ)] * 48
    comp = [1] * 48
    entries.insert(13, gen.text(3072)); comp.insert(13, 1)            # a 3-leaf row
    entries.insert(31, gen.incompressible(7, 5000)); comp.insert(31, 0)  # a stored row
    return Arch(oracle, entries, comp)


@pytest.fixture(params=SWITCHES, ids=IDS)
def ctx(request):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = make_ctx(dict(ZNIPPY_ROLES_MIN="1", **request.param))
    yield c
    c.close()


def _flip(ctx, d_blob, at):
    """Damage or restore a blob byte with nothing in flight."""
    import torch
    ctx.sync()
    d_blob[at] ^= 0x55
    torch.cuda.synchronize()


def _put(ctx, d_blob, at, b):
    """Overwrite blob bytes with nothing in flight."""
    import torch
    ctx.sync()
    d_blob[at:at + len(b)] = torch.from_numpy(np.ascontiguousarray(b).copy()).cuda()
    torch.cuda.synchronize()


def _lean(ctx):
    return "blake3_second_pass" not in dict(ctx.kernel_times())


@pytest.mark.parametrize("which", ["periodic", "mixed"])
def test_pipeline_with_alternating_buffers(ctx, request, which):
    """Ten runs into alternating buffers, each read with lag 1.  A row is damaged before run 4 (its blob becomes the head of a
    frame the role-split kernel hands over: on the periodic table run 4 is a lean run and comes back flagged) and another
    before run 7 (a flipped byte), each restored once that run's results have been read (a flagged run is repeated over the
    blobs as they are then: the caller keeps them until it has read the run), so runs 4, 5 and 7, 8 see a damaged row.  Every
    lagged read returns that run's counters;
    after the last read, status, corrupt list and digests describe run 9; both buffers hold the oracle's bytes of the last run
    written into them."""
    A = request.getfixturevalue(which)
    rt = A.table(ctx)
    d_blob, outs = A.d_blob(), [A.d_out(), A.d_out()]
    dmg = {4: dict(foreign=(5,)), 5: dict(foreign=(5,)), 7: dict(damaged=(40,)), 8: dict(damaged=(40,))}
    got, lean = [], []
    for k in range(10):
        if k == 4:
            _put(ctx, d_blob, *A.foreign(5))
        if k == 7:
            _flip(ctx, d_blob, A.damage_at(40))
        rt.decode_verify_async(d_blob, outs[k & 1])
        lean.append(_lean(ctx))
        if k >= 1:
            got.append(rt.results_lagged(1))
            if k == 5:
                _put(ctx, d_blob, 5 * A.slot, A.blob[5 * A.slot:6 * A.slot])
            if k == 8:
                _flip(ctx, d_blob, A.damage_at(40))
    got.append(rt.results_lagged(0))
    assert lean[4] == (which == "periodic") and not any(lean[6:]), lean   # (a flagged run: the table runs in full from then on)
    for k in range(10):
        assert got[k] == A.want(**dmg.get(k, {}))[0], (k, got[k])
    assert sum(c["corrupt_rows"] + c["decode_errors"] for c in (got[4], got[7])) == 2  # (the damage is seen at all)
    counters, corrupt, status = rt.results()
    want9 = A.want(())
    assert counters == want9[0] and list(corrupt) == want9[1] and (status == 0).all()
    assert np.array_equal(rt.digests(), A.ck)
    ctx.sync()
    assert np.array_equal(outs[1][:A.total].cpu().numpy(), want9[2])                      # run 9
    assert np.array_equal(outs[0][:A.total].cpu().numpy(), A.want((40,), onto=want9[2])[2])  # run 8, over run 6's clean bytes
    rt.close()


def test_flagged_lean_runs(ctx, periodic):
    """After three lean runs two rows become frames the role-split kernel's recogniser refuses (the head of an entropy-coded
    frame of other content, cut where the table says the blob ends), for two runs in flight: both come back complete with
    their own counters, and the next run is a full one."""
    import torch
    A = periodic
    rt = A.table(ctx)
    d_blob, outs = A.d_blob(), [A.d_out(), A.d_out()]
    lean = []
    for k in range(4):  # a full run (nothing is known yet), then lean ones
        rt.decode_verify_async(d_blob, outs[k & 1])
        lean.append(_lean(ctx))
        assert rt.results_lagged(0) == A.want(())[0], k
    assert lean == [False, True, True, True], lean
    ctx.sync()
    for r in (7, 44):
        at, b = A.foreign(r)
        d_blob[at:at + len(b)] = torch.from_numpy(b.copy()).cuda()
    torch.cuda.synchronize()
    rt.decode_verify_async(d_blob, outs[0])
    assert _lean(ctx)
    rt.decode_verify_async(d_blob, outs[1])
    assert _lean(ctx)
    c4, c5 = rt.results_lagged(1), rt.results_lagged(0)
    w2 = A.want(foreign=(7, 44))
    assert c4 == w2[0] and c5 == w2[0], (c4, c5, w2[0])
    assert c4["corrupt_rows"] + c4["decode_errors"] == 2
    counters, corrupt, status = rt.results()
    assert counters == w2[0] and list(corrupt) == w2[1]
    assert sorted(np.nonzero(status < 0)[0].tolist() + w2[1]) == [7, 44]
    ctx.sync()
    for o in outs:
        assert np.array_equal(o[:A.total].cpu().numpy(), w2[2])
    rt.decode_verify_async(d_blob, outs[0])
    assert not _lean(ctx)
    assert rt.results_lagged(0) == w2[0]
    rt.close()


def test_preset_run_in_the_steady_state(ctx, periodic):
    """A run whose last row lies outside the declared blob region, between lean runs with two in flight: that row reports
    ZNIPPY_E_CORRUPT and no kernel touches its bytes; the runs in front of it and behind it are what they always are."""
    from znippy_amd import _lib
    A = periodic
    rt = A.table(ctx)
    d_blob = A.d_blob()
    outs = [A.d_out(), A.d_out(), A.d_out(0xCD)]
    cap_all, cap_cut = d_blob.numel(), int(A.bo[-1]) + 5      # the last row's blob passes the short region's end
    short = A.want((), n_rows=A.n - 1)[0]
    want_preset = dict(short, total_chunks=short["total_chunks"] + 1, decode_errors=short["decode_errors"] + 1)
    got = {}
    for k in range(8):
        rt.decode_verify_async(d_blob, outs[2] if k == 4 else outs[k & 1], blob_cap=cap_cut if k == 4 else cap_all)
        if k >= 1:
            got[k - 1] = rt.results_lagged(1)
        if k == 4:
            counters, corrupt, status = rt.results()
            want_status = np.zeros(A.n, np.int32); want_status[-1] = _lib.E_CORRUPT
            assert counters == want_preset and len(corrupt) == 0 and np.array_equal(status, want_status)
    got[7] = rt.results_lagged(0)
    for k in range(8):
        assert got[k] == (want_preset if k == 4 else A.want(())[0]), (k, got[k])
    counters, corrupt, status = rt.results()
    assert counters == A.want(())[0] and (status == 0).all() and np.array_equal(rt.digests(), A.ck)
    ctx.sync()
    host = outs[2].cpu().numpy()
    assert np.array_equal(host[:A.total - SZ], A.clean_bytes[:A.total - SZ]) and (host[A.total - SZ:] == 0xCD).all()
    for o in outs[:2]:
        assert np.array_equal(o[:A.total].cpu().numpy(), A.clean_bytes)
    rt.close()


def test_mixed_run_kinds(ctx, mixed):
    """Decode + verify, verify-only and decode-only runs interleaved on one table with two in flight (one row damaged
    throughout): every run's counters equal the synchronous call of its kind on a fresh table — and, for the two kinds that
    verify, the oracle's."""
    A = mixed
    d_blob = A.d_blob()
    d_blob[A.damage_at(20)] ^= 0x55
    w = A.want((20,), onto=np.zeros(A.total, np.uint8))
    fresh = {}
    for kind in "DVP":
        rt0, o = A.table(ctx), A.d_out()
        if kind == "D": fresh[kind] = rt0.decode_verify(d_blob, o)[0]
        elif kind == "V": fresh[kind] = rt0.verify(d_blob)[0]
        else: fresh[kind] = rt0.decode(d_blob, o)[0]
        rt0.close()
    assert fresh["D"] == w[0] and fresh["V"] == w[0]
    assert fresh["D"]["corrupt_rows"] + fresh["D"]["decode_errors"] == 1
    rt = A.table(ctx)
    outs = [A.d_out(), A.d_out()]
    kinds = "DVPVDPDDVP"
    got = []
    for k, kind in enumerate(kinds):
        if kind == "D": rt.decode_verify_async(d_blob, outs[k & 1])
        elif kind == "V": rt.verify_async(d_blob)
        else: rt.decode_async(d_blob, outs[k & 1])
        if k >= 1:
            got.append(rt.results_lagged(1))
    got.append(rt.results_lagged(0))
    for k, kind in enumerate(kinds):
        assert got[k] == fresh[kind], (k, kind, got[k])
    ctx.sync()
    for o in outs:
        assert np.array_equal(o[:A.total].cpu().numpy(), w[2])
    rt.close()


def test_two_tables_on_one_context(ctx, periodic, mixed):
    """Two tables queued alternately on one context, each read with lag 1: the oracle's results for each.  Then a clean run,
    znippy_ctx_sync, and the output read directly — complete before any results call — then the results."""
    tabs = [(periodic, (3,)), (mixed, (31,))]   # one damaged row each (the mixed table's: its stored row)
    rts, blobs, outs = [], [], []
    for A, bad in tabs:
        rts.append(A.table(ctx))
        b = A.d_blob()
        for r in bad:
            b[A.damage_at(r)] ^= 0x55
        blobs.append(b)
        outs.append([A.d_out(), A.d_out()])
    for k in range(6):
        for i, (A, bad) in enumerate(tabs):
            rts[i].decode_verify_async(blobs[i], outs[i][k & 1])
            if k >= 1:
                assert rts[i].results_lagged(1) == A.want(bad, onto=np.zeros(A.total, np.uint8))[0], (k, i)
    for i, (A, bad) in enumerate(tabs):
        w = A.want(bad, onto=np.zeros(A.total, np.uint8))
        counters, corrupt, status = rts[i].results()
        assert counters == w[0] and list(corrupt) == w[1], i
        assert counters["corrupt_rows"] + counters["decode_errors"] == 1
        ctx.sync()
        for o in outs[i]:
            assert np.array_equal(o[:A.total].cpu().numpy(), w[2]), i
    for i, (A, bad) in enumerate(tabs):      # sync, read the output, then the results
        for r in bad:
            _flip(ctx, blobs[i], A.damage_at(r))
        fresh = A.d_out(0xEE)
        rts[i].decode_verify_async(blobs[i], fresh)
        ctx.sync()
        assert np.array_equal(fresh[:A.total].cpu().numpy(), A.clean_bytes), i
        counters, corrupt, status = rts[i].results()
        assert counters == A.want(())[0] and len(corrupt) == 0 and (status == 0).all(), i
        assert np.array_equal(rts[i].digests(), A.ck), i
    for rt in rts:
        rt.close()
