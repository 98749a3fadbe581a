"""Lean runs in the read loop's pipeline (api.hip: rows_settle).  A table whose last run left nothing behind its main kernel is
run without the kernels behind it; a run that meets changed blobs comes back flagged and is repeated in full inside the first
results call that reads it.  Here a reader keeps two runs in flight over two blob and two output buffers, as the header says
it may (run k + 1 queued before run k's results are read; a buffer refilled only after the results of the run that used it
have been read), and every run meets its own damage.  Each run's counters, its output buffer at the moment its results are
returned, and the table's status / corrupt list / digests after the loop must be what the oracle's read loop
(decompress.rs:L135-190) and a context without lean runs (ZNIPPY_NO_LEAN=1) say — for all three kinds of lean run."""
import gc
import weakref

import numpy as np
import pytest

import gen
from gpu_cases import make_ctx

pytestmark = pytest.mark.gpu


def _flip(oracle, frame, data, kind):
    """(position, xor) of a one-byte change of `frame` after which the oracle reports `kind`: 'error' (the frame does not
    decode to its size) or 'mismatch' (it decodes to other bytes of the same size: a checksum mismatch).  An error is made
    in the first block's literals header if it can be (the frame is then of a shape no lean kernel takes: it is handed over
    and the run comes back flagged), else from the frame's end; mismatches are looked for from the frame's middle."""
    n = len(frame)
    fhd = frame[4]
    single = (fhd >> 5) & 1
    lit_hdr = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if single else 0), 2, 4, 8)[fhd >> 6] + 3
    order = [lit_hdr] + list(range(n - 1, 3, -1)) if kind == "error" else list(range(n // 2, n)) + list(range(4, n // 2))
    for p in order:
        for x in (0x02, 0x01, 0x55, 0x80):
            b = bytearray(frame)
            b[p] ^= x
            try:
                d = oracle.zstd_decompress(bytes(b), cap=len(data))
                got = "mismatch" if len(d) == len(data) and d != data else ("error" if len(d) != len(data) else "same")
            except ValueError:
                got = "error"
            if got == kind:
                return p, x
    raise AssertionError(f"no one-byte change gives {kind}")


def _table(oracle, kind):
    """Index columns, pristine blob region and the switches of one of the three lean kinds (the shapes of the
    test_lean_runs_of_*_notice_changed_blobs tests in test_gpu_roles.py)."""
    from znippy_amd import hip
    env, bm = {}, None
    if kind == "lean":            # small rows the role-split kernel takes whole
        env = {"ZNIPPY_ROLES_MIN": "1"}
        n = 6 * 500
        datas = [gen.text(10240)] * n
        frames = [oracle.libzstd_compress(datas[0], 19)] * n
        comp_rows = list(range(n))
        marker = lambda names: "blake3_second_pass" in names
    elif kind == "lean_blocks":   # big multi-block rows only, every block written and hashed by the fused block kernel
        n, size = 24, 4 * 131072
        datas = [gen.text(size) if i % 3 else gen.binary(size) for i in range(n)]
        ctx0 = hip.Context(0)
        by = {d: ctx0.compress(d) for d in set(datas)}
        ctx0.close()
        frames = [by[d] for d in datas]
        comp_rows = list(range(n))
        marker = lambda names: "zstd_decode_blocks" in names
    else:                         # lean_mixed: small compressed rows beside big stored rows
        rng = np.random.default_rng(11)
        small = [gen.text(int(rng.integers(1024, 8192))) for _ in range(900)]
        big = [gen.incompressible(20 + i, (1 << 20) + 4096 * i) for i in range(6)]
        datas = small + big
        ctx0 = hip.Context(0)
        frames = [ctx0.compress(e) for e in small] + big
        ctx0.close()
        comp = np.array([1] * len(small) + [0] * len(big), np.uint8)
        bm = np.packbits(comp.astype(bool), bitorder="little")
        comp_rows = list(range(len(small)))
        marker = lambda names: "zstd_decode_general" in names or "zstd_decode_fallback" in names
    n = len(datas)
    bs = np.array([len(f) for f in frames], np.uint64)
    bo = (np.cumsum(bs) - bs).astype(np.uint64)
    us = np.array([len(d) for d in datas], np.uint64)
    oo = (np.cumsum(us) - us).astype(np.uint64)
    dig = {d: np.frombuffer(oracle.blake3(d), np.uint8) for d in set(datas)}
    ck = np.stack([dig[d] for d in datas])
    blob = np.frombuffer(b"".join(frames) + bytes(64), np.uint8).copy()
    src = np.frombuffer(b"".join(datas), np.uint8)
    return dict(kind=kind, env=env, n=n, bo=bo, bs=bs, us=us, oo=oo, ck=ck, bm=bm, blob=blob, src=src, frames=frames,
                datas=datas, comp_rows=comp_rows, full_marker=marker, total=int(us.sum()))


# Damage of run k: (fraction of the compressed rows, kind).  Every damaged run has its own count; errors come from the
# frame's sequence section (the lean kernels hand such a row over: the run is flagged), mismatches decode to other bytes.
SCHEDULES = {
    # 1, 2 and 3 damaged rows in a row (run 5 stands behind flagged run 4 and is flagged itself), a clean run, one more, a
    # clean last run
    "counts": [[], [], [], [], [(0.014, "error")], [(0.3, "mismatch"), (0.97, "error")],
               [(0.001, "error"), (0.5, "mismatch"), (0.8, "error")], [], [(0.6, "error")], []],
    # the run before the last one is flagged, the last one is clean: the table's status and digests must be the last run's
    "last_clean": [[], [], [], [], [(0.25, "error"), (0.7, "mismatch")], []],
}


class _Runs:
    """The blob region of every run of a schedule and the oracle's read loop over it."""

    def __init__(self, oracle, T, schedule):
        self.T, self.oracle = T, oracle
        self.flips, self.bad = [], []
        cache = {}
        for damage in schedule:
            fl, bad = [], set()
            for frac, kind in damage:
                r = T["comp_rows"][min(int(frac * len(T["comp_rows"])), len(T["comp_rows"]) - 1)]
                key = (T["frames"][r], kind)
                if key not in cache:
                    cache[key] = _flip(oracle, T["frames"][r], T["datas"][r], kind)
                p, x = cache[key]
                fl.append((int(T["bo"][r]) + p, x))
                bad.add(r)
            self.flips.append(fl)
            self.bad.append(bad)
        self._want = {}

    def blob(self, k):
        b = self.T["blob"].copy()
        for p, x in self.flips[k]:
            b[p] ^= x
        return b

    def want(self, k):
        """(counters, sorted corrupt rows, bytes) of the oracle's read loop over run k's blobs."""
        key = tuple(self.flips[k])
        if key not in self._want:
            T = self.T
            comp = np.ones(T["n"], np.uint8) if T["bm"] is None else np.unpackbits(T["bm"], bitorder="little")[:T["n"]]
            bitmap = np.packbits(comp.astype(bool), bitorder="little")
            out = np.zeros(T["total"], np.uint8)
            c, corrupt = self.oracle.decompress_rows(self.blob(k), T["bo"], T["bs"], T["us"], T["oo"], bitmap, T["ck"], 0,
                                                     T["n"], out=out)
            self._want[key] = (dict(c), sorted(int(x) for x in corrupt), out)
        return self._want[key]

    def good_bytes(self, k):
        """Mask of the output bytes that belong to rows run k did not damage."""
        m = np.ones(self.T["total"], bool)
        for r in self.bad[k]:
            m[int(self.T["oo"][r]):int(self.T["oo"][r] + self.T["us"][r])] = False
        return m


class _Reader:
    """One context (lean runs or none) running a schedule as the read loop does: two blob and two output buffers."""

    def __init__(self, T, no_lean):
        import torch
        from znippy_amd import hip
        self.ctx = make_ctx(dict(T["env"], **({"ZNIPPY_NO_LEAN": "1"} if no_lean else {})))
        self.T = T
        self.blobs = [torch.zeros(len(T["blob"]), dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.outs = [torch.zeros(T["total"] + 64, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.rt = hip.RowTable(self.ctx, T["bo"], T["bs"], T["us"], T["oo"], T["bm"], T["ck"])
        self.counters, self.full_queued, self.full_after_read = [], [], []

    def queue(self, k, blob):
        import torch
        self.blobs[k & 1].copy_(torch.from_numpy(blob))      # the run that used this buffer last has been read
        self.outs[k & 1].fill_(0)
        self.rt.decode_verify_async(self.blobs[k & 1], self.outs[k & 1])
        self.full_queued.append(self.T["full_marker"](dict(self.ctx.kernel_times())))

    def read(self, lag):
        self.counters.append(self.rt.results_lagged(lag))
        self.full_after_read.append(self.T["full_marker"](dict(self.ctx.kernel_times())))

    def out(self, k):
        return self.outs[k & 1][:self.T["total"]].cpu().numpy()

    def close(self):
        self.rt.close()
        self.ctx.close()


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("kind", ["lean", "lean_blocks", "lean_mixed"])
def test_lean_pipeline_every_run_is_its_own(oracle, kind, schedule):
    T = _table(oracle, kind)
    R = _Runs(oracle, T, SCHEDULES[schedule])
    nruns = len(SCHEDULES[schedule])
    lean, full = _Reader(T, False), _Reader(T, True)
    try:
        def check_out(k):   # run k's results have just been returned by both contexts
            a, b = lean.out(k), full.out(k)
            m = R.good_bytes(k)
            assert np.array_equal(a[m], T["src"][m]), (k, "an undamaged row of the lean context's buffer is not its source")
            assert np.array_equal(b[m], T["src"][m]), (k, "an undamaged row of the NO_LEAN buffer is not its source")
            assert np.array_equal(a, b), (k, int(np.nonzero(a != b)[0][0]))

        for k in range(nruns):
            blob = R.blob(k)
            for rd in (lean, full):
                rd.queue(k, blob)
            if k >= 1:
                for rd in (lean, full):
                    rd.read(1)
                check_out(k - 1)
        for rd in (lean, full):
            rd.read(0)
        check_out(nruns - 1)

        want = [R.want(k)[0] for k in range(nruns)]
        assert len(full.counters) == nruns and full.counters == want
        assert len(lean.counters) == nruns
        assert lean.counters == want, [(k, c, w) for k, (c, w) in enumerate(zip(lean.counters, want)) if c != w]
        assert all(full.full_queued) and all(full.full_after_read)
        assert not any(lean.full_queued[2:5]), lean.full_queued      # lean runs were queued, damaged ones among them
        assert any(lean.full_after_read), "no flagged run was repeated"

        # the table's own outputs describe the latest run, as the NO_LEAN context reports them
        c_want, corrupt_want, _ = R.want(nruns - 1)
        res = {}
        for name, rd in (("lean", lean), ("full", full)):
            c, corrupt, status = rd.rt.results()
            res[name] = (dict(c), sorted(int(x) for x in corrupt), status.copy(), rd.rt.digests().copy())
        for name in res:
            assert res[name][0] == c_want, name
            assert res[name][1] == corrupt_want, name
            assert int((res[name][2] < 0).sum()) == c_want["decode_errors"], name
        assert np.array_equal(res["lean"][2], res["full"][2]), np.nonzero(res["lean"][2] != res["full"][2])[0][:8]
        assert np.array_equal(res["lean"][3], res["full"][3]), np.nonzero((res["lean"][3] != res["full"][3]).any(1))[0][:8]
        good = res["full"][2] >= 0
        good[corrupt_want] = False
        assert np.array_equal(res["full"][3][good], T["ck"][good])
    finally:
        lean.close()
        full.close()


@pytest.mark.parametrize("kind", ["lean", "lean_blocks", "lean_mixed"])
def test_sync_then_results_completes_a_flagged_lean_run(oracle, kind):
    """A flagged lean run, then znippy_ctx_sync, then a results call: the results call completes d_out (the run is repeated
    there), to the bytes a NO_LEAN context wrote, with the oracle's counters."""
    T = _table(oracle, kind)
    R = _Runs(oracle, T, [[], [], [], [(0.4, "error"), (0.9, "mismatch")]])
    lean, full = _Reader(T, False), _Reader(T, True)
    try:
        for k in range(4):
            for rd in (lean, full):
                rd.queue(k, R.blob(k))
                if k < 3:
                    rd.read(0)
        assert not lean.full_queued[3] and full.full_queued[3]
        for rd in (lean, full):
            rd.ctx.sync()
            rd.out(3)                                  # the caller looks at d_out before reading the results ...
        c_want, corrupt_want, _ = R.want(3)
        for rd in (lean, full):
            c, corrupt, status = rd.rt.results()       # ... and reads them now: d_out is complete after this call
            assert dict(c) == c_want and sorted(int(x) for x in corrupt) == corrupt_want
        a, b = lean.out(3), full.out(3)
        m = R.good_bytes(3)
        assert np.array_equal(a[m], T["src"][m])
        assert np.array_equal(a, b), int(np.nonzero(a != b)[0][0])
    finally:
        lean.close()
        full.close()


def test_row_table_keeps_queued_buffers_until_read(gpu_ctx, oracle):
    """RowTable holds the tensors of a queued run (the library may run it again from a later results call): a caller that
    drops its references does not free them until the run's results have been read; then they go.  The latest run's
    buffers also stay while the run before it is unread (reading that one may repeat the latest run too)."""
    import torch
    from znippy_amd import hip
    data = gen.text(10240)
    frame = np.frombuffer(oracle.libzstd_compress(data, 19), np.uint8)
    n = 64
    rt = hip.RowTable(gpu_ctx, np.arange(n, dtype=np.uint64) * len(frame), np.full(n, len(frame), np.uint64),
                      np.full(n, 10240, np.uint64), np.arange(n, dtype=np.uint64) * 10240, None,
                      np.tile(np.frombuffer(oracle.blake3(data), np.uint8), (n, 1)))
    blob_host = np.concatenate([np.tile(frame, n), np.zeros(64, np.uint8)])

    def queue():
        b = torch.from_numpy(blob_host.copy()).cuda()
        o = torch.zeros(n * 10240 + 64, dtype=torch.uint8, device="cuda")
        rt.decode_verify_async(b, o)
        return weakref.ref(b), weakref.ref(o)

    def alive(refs):
        gc.collect()
        return [r() is not None for r in refs]

    r0 = queue()
    assert alive(r0) == [True, True]
    c, _, _ = rt.results()
    assert c["verified_bytes"] == n * 10240
    assert alive(r0) == [False, False]

    # two in flight, read in order: each pair goes with its own read
    r1 = queue()
    r2 = queue()
    assert alive(r1 + r2) == [True] * 4
    assert rt.results_lagged(1)["verified_bytes"] == n * 10240
    assert alive(r1 + r2) == [False, False, True, True]
    assert rt.results_lagged(0)["verified_bytes"] == n * 10240
    assert alive(r2) == [False, False]

    # the latest run read first: it stays until the run before it is read as well
    r3 = queue()
    r4 = queue()
    rt.digests()
    assert alive(r3 + r4) == [True] * 4
    assert rt.results_lagged(1)["verified_bytes"] == n * 10240
    assert alive(r3 + r4) == [False] * 4
    rt.close()
