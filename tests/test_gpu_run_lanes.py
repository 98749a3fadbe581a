"""Run lanes (csrc/api.hip: lane_begin; the rule: csrc/host/run_overlap.cc): consecutive lean runs queued on two run streams,
left unordered when neither can see the other.  Every case runs on a context with lanes (default), with the switch that puts
every run back in queue order (ZNIPPY_NO_RUN_LANES) and without the forked verify (ZNIPPY_NO_FORK_VERIFY: no lanes either), on
the smallest table that runs lean through the role-split kernel: 48 rows of the recognised periodic 10 KiB shape under
ZNIPPY_ROLES_MIN=1 (8 tiles, two groups).  A second archive of the same layout holds another text.  Expected counters,
corrupt lists and bytes are the oracle's restated read loop's (decompress.rs:L113-192) over the same blobs; what the context
decided comes from its lane counters (Context.run_lane_stats)."""
import numpy as np
import pytest

import gen
from gpu_cases import make_ctx

pytestmark = pytest.mark.gpu

SZ = 10240
# (the first says "0" and not nothing: the suite is also run with ZNIPPY_NO_RUN_LANES=1 exported, and this case is the one with lanes)
SWITCHES = [{"ZNIPPY_NO_RUN_LANES": "0"}, {"ZNIPPY_NO_RUN_LANES": "1"}, {"ZNIPPY_NO_FORK_VERIFY": "1"}]
IDS = ["default", "no_run_lanes", "no_fork_verify"]


class Arch:
    """Rows in blob slots of one size; the oracle's results per blob image."""

    def __init__(self, oracle, entries, comp):
        self.O = oracle
        self.entries, self.n = entries, len(entries)
        made = {}
        for e, c in zip(entries, comp):
            if c and e not in made:
                made[e] = oracle.libzstd_compress(e, 19)
        self.frames = [made[e] if c else e for e, c in zip(entries, comp)]
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

    def foreign(self, row):  # (where, bytes): the row's blob as the head of the other frame, as long as the table says the blob is
        assert len(self.other) > int(self.bs[row])
        return row * self.slot, self.other[:int(self.bs[row])]

    def want(self, blob=None, onto=None, foreign=()):
        """Oracle over this table's columns and a blob image (default: its own; `foreign`: rows replaced by the other frame):
        (counters, sorted corrupt list, output image over `onto`, default zeros)."""
        key = (None if blob is None else blob.tobytes(), None if onto is None else onto.tobytes(), tuple(foreign))
        if key not in self._want:
            img = (self.blob if blob is None else blob).copy()
            for r in foreign:
                at, b = self.foreign(r)
                img[at:at + len(b)] = b
            out = (np.zeros(self.total, np.uint8) if onto is None else onto).copy()
            c, corrupt = self.O.decompress_rows(img, self.bo, self.bs, self.us, self.oo, self.bitmap, self.ck, 0, self.n, out=out)
            self._want[key] = (dict(c), [int(x) for x in corrupt], out)
        return self._want[key]

    def table(self, ctx):
        from znippy_amd import hip
        return hip.RowTable(ctx, self.bo, self.bs, self.us, self.oo, self.bitmap, self.ck)

    def d_blob(self, image=None):
        import torch
        return torch.from_numpy((self.blob if image is None else image).copy()).cuda()

    def d_out(self, fill=0, extra=64):
        import torch
        return torch.full((self.total + extra,), fill, dtype=torch.uint8, device="cuda")


def _other_text():
    return (gen.PHRASE.swapcase() * (SZ // len(gen.PHRASE) + 1))[:SZ]


@pytest.fixture(scope="module")
def periodic(oracle):
    return Arch(oracle, [gen.text(SZ)] * 48, [1] * 48)


@pytest.fixture(scope="module")
def periodic_b(oracle):
    """The same layout with another text in every row (its frames are as long as the first archive's)."""
    return Arch(oracle, [_other_text()] * 48, [1] * 48)


@pytest.fixture(scope="module")
def mixed(oracle):
    entries = [gen.text(SZ)] * 48
    comp = [1] * 48
    entries.insert(13, gen.text(3072)); comp.insert(13, 1)               # a 3-leaf row
    entries.insert(31, gen.incompressible(7, 5000)); comp.insert(31, 0)  # a stored row
    return Arch(oracle, entries, comp)


@pytest.fixture(params=SWITCHES, ids=IDS)
def ctx(request):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = make_ctx(dict(ZNIPPY_ROLES_MIN="1", **request.param))
    c.lanes = request.param.get("ZNIPPY_NO_RUN_LANES") == "0"
    yield c
    c.close()


def _lean(ctx):
    """Was the last run lean?  By its kernel times."""
    return "blake3_second_pass" not in dict(ctx.kernel_times())


def _n_lean(ctx):
    """Lean runs queued on the context so far: each is counted once, beside its predecessor, behind it, or off the lanes (the
    counters are read without going through the context's entry: nothing is ordered by asking)."""
    st = ctx.run_lane_stats()
    return st["unordered"] + st["ordered"] + st["off_lanes"]


def _delta(ctx, since):
    return {k: v - since[k] for k, v in ctx.run_lane_stats().items()}


def _warm(ctx, rt, d_blob, d_out):
    """A full run, then two lean ones, each read before the next is queued: the table's next run is lean, nothing is in flight and
    nothing but lane runs has been queued since the last of them.  -> the lane counters now."""
    n0 = _n_lean(ctx)
    for k in range(3):
        rt.decode_verify_async(d_blob, d_out)
        rt.results_lagged(0)
    assert _n_lean(ctx) == n0 + 2
    return ctx.run_lane_stats()


def _host(t, n):
    return t[:n].cpu().numpy()


def test_pipeline_identical_arguments(ctx, periodic):
    """Twelve runs of one table over one pair of buffers, each read with lag 1: every run's counters, the bytes after the drain.
    With lanes every lean run but the first is queued beside its predecessor (the first stands behind the full runs: one mark, no
    predecessor to run beside); without, none is on a lane."""
    A = periodic
    rt = A.table(ctx)
    d_blob, d_out = A.d_blob(), A.d_out(0xEE)
    want = A.want()
    lean = []
    for k in range(12):
        n0 = _n_lean(ctx)
        rt.decode_verify_async(d_blob, d_out)
        lean.append(_n_lean(ctx) == n0 + 1)
        if k:
            assert rt.results_lagged(1) == want[0], k
    assert rt.results_lagged(0) == want[0]
    counters, corrupt, status = rt.results()
    assert counters == want[0] and list(corrupt) == want[1] and (status == 0).all()
    assert np.array_equal(rt.digests(), A.ck)
    ctx.sync()
    assert np.array_equal(_host(d_out, A.total), A.clean_bytes)
    assert lean[0] is False and all(lean[2:]), lean   # (the second run is lean only if the first had ended when it was queued)
    n_lean = sum(lean)
    st = ctx.run_lane_stats()
    print("lane counters", st, "lean runs", n_lean)
    if ctx.lanes:
        assert st == dict(unordered=n_lean - 1, ordered=1, marks=1, off_lanes=0), st
    else:
        assert st == dict(unordered=0, ordered=0, marks=0, off_lanes=n_lean), st
    rt.close()


def test_alternating_buffer_pairs(ctx, periodic, periodic_b):
    """One table, two blob buffers with different rows, each decoded into its own output buffer, alternating: the output regions
    are disjoint and no run reads where another writes, so the runs go unordered; each buffer ends up with its own archive's bytes
    (the second archive's rows do not match the table's checksums: the oracle says what a run over them reports)."""
    A = periodic
    rt = A.table(ctx)
    blobs = [A.d_blob(), A.d_blob(periodic_b.blob)]
    outs = [A.d_out(0xEE), A.d_out(0xEE)]
    wants = [A.want(), A.want(blob=periodic_b.blob)]
    assert wants[1][0]["corrupt_rows"] == A.n and np.array_equal(wants[1][2], periodic_b.clean_bytes)
    s0 = _warm(ctx, rt, blobs[0], outs[0])
    for k in range(8):
        rt.decode_verify_async(blobs[k & 1], outs[k & 1])
        if k:
            assert rt.results_lagged(1) == wants[(k - 1) & 1][0], k
    assert rt.results_lagged(0) == wants[1][0]
    d = _delta(ctx, s0)   # (every run is counted once: all eight were lean)
    assert d == (dict(unordered=8, ordered=0, marks=0, off_lanes=0) if ctx.lanes else dict(unordered=0, ordered=0, marks=0, off_lanes=8)), d
    ctx.sync()
    for i in range(2):
        assert np.array_equal(_host(outs[i], A.total), wants[i][2]), i
    rt.close()


@pytest.mark.parametrize("n_runs", [2, 3, 6, 7])
def test_two_blob_buffers_into_one_output(ctx, periodic, periodic_b, n_runs):
    """Two blob buffers with different rows decoded alternately into ONE output buffer: the runs write different bytes to the same
    place, so each is ordered behind its predecessor, and after the drain the buffer holds the last queued run's bytes exactly."""
    A = periodic
    rt = A.table(ctx)
    blobs = [A.d_blob(), A.d_blob(periodic_b.blob)]
    d_out = A.d_out(0xEE)
    wants = [A.want(), A.want(blob=periodic_b.blob)]
    s0 = _warm(ctx, rt, blobs[0], d_out)
    for k in range(n_runs):
        rt.decode_verify_async(blobs[k & 1], d_out)
        if k:
            assert rt.results_lagged(1) == wants[(k - 1) & 1][0], k
    assert rt.results_lagged(0) == wants[(n_runs - 1) & 1][0]
    d = _delta(ctx, s0)
    # (the first run of the pipeline has the same arguments as the last warm-up run: that pair alone may go side by side)
    assert d == (dict(unordered=1, ordered=n_runs - 1, marks=0, off_lanes=0) if ctx.lanes else dict(unordered=0, ordered=0, marks=0, off_lanes=n_runs)), d
    ctx.sync()
    assert np.array_equal(_host(d_out, A.total), wants[(n_runs - 1) & 1][2])
    rt.close()


def test_blobs_inside_the_previous_output(ctx, periodic, periodic_b):
    """A run whose blob region lies inside the output region of the run in front of it (the frames of the second archive, placed
    in the buffer's tail with nothing in flight), alternating with that run: every run is ordered — the reader behind the writer of
    the region it reads from, the writer behind the reader — and the bytes are right."""
    A, B = periodic, periodic_b
    rt = A.table(ctx)
    d_blob = A.d_blob()
    tail = (A.total + 255) // 256 * 256
    big = A.d_out(0xEE, extra=tail - A.total + len(B.blob) + 64)
    big[tail:tail + len(B.blob)] = B.d_blob()
    out2 = A.d_out(0xEE)
    wants = [A.want(), A.want(blob=B.blob)]
    s0 = _warm(ctx, rt, big[tail:], out2)
    for k in range(6):
        if k & 1:
            rt.decode_verify_async(big[tail:], out2)   # reads the tail of `big`
        else:
            rt.decode_verify_async(d_blob, big)        # its output region is all of `big`
        if k:
            assert rt.results_lagged(1) == wants[(k - 1) & 1][0], k
    assert rt.results_lagged(0) == wants[1][0]
    d = _delta(ctx, s0)
    assert d == (dict(unordered=0, ordered=6, marks=0, off_lanes=0) if ctx.lanes else dict(unordered=0, ordered=0, marks=0, off_lanes=6)), d
    ctx.sync()
    assert np.array_equal(_host(big, A.total), wants[0][2])
    assert np.array_equal(big[tail:tail + len(B.blob)].cpu().numpy(), B.blob)
    assert np.array_equal(_host(out2, A.total), wants[1][2])
    rt.close()


def test_main_stream_work_behind_a_lane_run(ctx, periodic):
    """A hash of the rows where a lean run writes them, queued on the context at once behind the run: it sees the run's bytes."""
    from znippy_amd import hip
    A = periodic
    rt = A.table(ctx)
    rounds = hip.RoundTable(ctx, A.oo, A.us)
    d_blob, warm = A.d_blob(), A.d_out()
    _warm(ctx, rt, d_blob, warm)
    for k in range(4):   # runs on both lanes
        fresh = A.d_out(0xEE)
        s0 = ctx.run_lane_stats()
        rt.decode_verify_async(d_blob, fresh)
        d = _delta(ctx, s0)
        assert d["unordered"] + d["ordered"] == (1 if ctx.lanes else 0) and d["off_lanes"] == (0 if ctx.lanes else 1), d
        assert np.array_equal(rounds.hash(fresh), A.ck), k
        assert rt.results_lagged(0) == A.want()[0]
    rounds.close()
    rt.close()


def test_main_stream_work_in_front_of_a_lane_run(ctx, periodic, mixed):
    """A full run of another table (main-stream work), directly behind it a lean run whose blobs live in the buffer the full run
    writes into (elsewhere in it), then a lean run behind a range read on its own table: each lean run stands behind a mark on the
    main stream, and every result is right."""
    A, M = periodic, mixed
    rt, rm = A.table(ctx), M.table(ctx)
    d_blob_m = M.d_blob()
    at = (M.total + 255) // 256 * 256
    big = M.d_out(0xEE, extra=at - M.total + len(A.blob) + 64)
    big[at:at + len(A.blob)] = A.d_blob()
    d_out = A.d_out(0xEE)
    s0 = _warm(ctx, rt, big[at:], d_out)
    n0 = _n_lean(ctx)
    rm.decode_verify_async(d_blob_m, big, out_cap=M.total)   # full: never lean
    assert _n_lean(ctx) == n0
    rt.decode_verify_async(big[at:], d_out)
    wm = M.want()
    assert rm.results_lagged(0) == wm[0] and rt.results_lagged(0) == A.want()[0]
    d1 = _delta(ctx, s0)
    # a range read on the lean table, then a lean run
    small = A.d_out(0xEE)
    status, _ = rt.read_ranges(big[at:], [5, 40], [100, 0], [300, SZ], small)
    assert (status == 0).all()
    assert np.array_equal(small[:300].cpu().numpy(), A.clean_bytes[5 * SZ + 100:5 * SZ + 400])
    assert np.array_equal(small[300:300 + SZ].cpu().numpy(), A.clean_bytes[40 * SZ:41 * SZ])
    rt.decode_verify_async(big[at:], d_out)
    assert rt.results_lagged(0) == A.want()[0]
    d2 = _delta(ctx, s0)
    if ctx.lanes:
        assert d1 == dict(unordered=0, ordered=1, marks=1, off_lanes=0), d1
        assert d2 == dict(unordered=0, ordered=2, marks=2, off_lanes=0), d2
    else:
        assert d2 == dict(unordered=0, ordered=0, marks=0, off_lanes=2), d2
    ctx.sync()
    assert np.array_equal(_host(big, M.total), wm[2])
    assert np.array_equal(_host(d_out, A.total), A.clean_bytes)
    rm.close()
    rt.close()


def test_flagged_runs_in_a_pipeline(ctx, periodic):
    """Two rows become frames the role-split kernel's recogniser refuses, between runs of a pipeline, for two runs in flight (the
    pattern of test_gpu_run_slots.test_flagged_lean_runs): both come back complete with what a full run reports, and the next run
    is a full one."""
    import torch
    A = periodic
    rt = A.table(ctx)
    d_blob, outs = A.d_blob(), [A.d_out(), A.d_out()]
    clean = A.want()
    for k in range(5):   # a pipeline of lean runs, two in flight
        rt.decode_verify_async(d_blob, outs[k & 1])
        if k:
            assert rt.results_lagged(1) == clean[0], k
    assert rt.results_lagged(0) == clean[0]   # (nothing in flight: every run has been read)
    for r in (7, 44):
        at, b = A.foreign(r)
        d_blob[at:at + len(b)] = torch.from_numpy(b.copy()).cuda()
    torch.cuda.synchronize()
    s0 = ctx.run_lane_stats()
    rt.decode_verify_async(d_blob, outs[1])
    rt.decode_verify_async(d_blob, outs[0])
    d = _delta(ctx, s0)   # both were queued lean
    assert d == (dict(unordered=2, ordered=0, marks=0, off_lanes=0) if ctx.lanes else dict(unordered=0, ordered=0, marks=0, off_lanes=2)), d
    c5, c6 = rt.results_lagged(1), rt.results_lagged(0)
    w2 = A.want(foreign=(7, 44), onto=A.clean_bytes)
    assert c5 == w2[0] and c6 == w2[0], (c5, c6, w2[0])
    assert c5["corrupt_rows"] + c5["decode_errors"] == 2
    counters, corrupt, status = rt.results()
    assert counters == w2[0] and list(corrupt) == w2[1]
    assert sorted(np.nonzero(status < 0)[0].tolist() + w2[1]) == [7, 44]
    ctx.sync()
    for o in outs:
        assert np.array_equal(_host(o, A.total), w2[2])
    rt.decode_verify_async(d_blob, outs[0])
    assert not _lean(ctx)
    assert rt.results_lagged(0) == w2[0]
    rt.close()


def test_two_lean_tables_interleaved(ctx, periodic, periodic_b):
    """Two tables on one context, both lean, queued A, B, A, B with lag-1 reads: counters and bytes per table."""
    tabs = [periodic, periodic_b]
    rts = [T.table(ctx) for T in tabs]
    blobs = [T.d_blob() for T in tabs]
    outs = [[T.d_out(0xEE), T.d_out(0xEE)] for T in tabs]
    for i in range(2):
        _warm(ctx, rts[i], blobs[i], outs[i][0])
    s0 = ctx.run_lane_stats()
    for k in range(6):
        for i, T in enumerate(tabs):
            rts[i].decode_verify_async(blobs[i], outs[i][k & 1])
            if k:
                assert rts[i].results_lagged(1) == T.want()[0], (k, i)
    d = _delta(ctx, s0)
    if ctx.lanes:   # (A, B, A, B goes to lanes 1, 1, 0, 0: every second run stands behind its predecessor on its own stream)
        assert d == dict(unordered=6, ordered=6, marks=0, off_lanes=0), d
    else:
        assert d == dict(unordered=0, ordered=0, marks=0, off_lanes=12), d
    for i, T in enumerate(tabs):
        counters, corrupt, status = rts[i].results()
        assert counters == T.want()[0] and len(corrupt) == 0 and (status == 0).all(), i
        assert np.array_equal(rts[i].digests(), T.ck), i
    ctx.sync()
    for i, T in enumerate(tabs):
        for o in outs[i]:
            assert np.array_equal(_host(o, T.total), T.clean_bytes), i
    for rt in rts:
        rt.close()


N_BIG = 60_000   # 10,000 tiles: the role-split kernel runs for ~0.3 ms, several times what it takes to queue three more runs


@pytest.fixture(scope="module")
def big_pair(oracle):
    """A table whose kernel fills the chip for a while, and the same layout with the other text in every row."""
    a, b = Arch(oracle, [gen.text(SZ)] * N_BIG, [1] * N_BIG), Arch(oracle, [_other_text()] * N_BIG, [1] * N_BIG)
    assert a.slot == b.slot and np.array_equal(a.bs, b.bs)
    return a, b


def test_a_run_behind_an_older_run_of_its_table(ctx, big_pair, periodic_b):
    """A, B, B, A with no read in between: a big table's run on lane 1, two runs of a small table (lanes 0 and 1), then the big
    table again on lane 0 with OTHER blobs into the SAME output.  The last run's predecessor is a run of the small table, which it
    may run beside; the run it must not run beside is two runs older and on the other stream.  It waits for it: the output holds
    the last run's bytes exactly, and the context counts the wait."""
    A, A2 = big_pair
    B = periodic_b
    ra, rb = A.table(ctx), B.table(ctx)
    blobs = [A.d_blob(), A.d_blob(A2.blob)]
    d_out = A.d_out(0xEE)
    b_blob, b_outs = B.d_blob(), [B.d_out(0xEE), B.d_out(0xEE)]
    wants = [A.want(), A.want(blob=A2.blob)]
    _warm(ctx, ra, blobs[0], d_out)          # three runs: the next is the table's slot 1
    _warm(ctx, rb, b_blob, b_outs[0])
    rb.decode_verify_async(b_blob, b_outs[1])  # a fourth: the next is the table's slot 0
    assert rb.results_lagged(0) == B.want()[0]
    s0, w0 = ctx.run_lane_stats(), ctx.run_lane_older_waits()
    ra.decode_verify_async(blobs[0], d_out)
    rb.decode_verify_async(b_blob, b_outs[0])
    rb.decode_verify_async(b_blob, b_outs[1])
    ra.decode_verify_async(blobs[1], d_out)
    d, w = _delta(ctx, s0), ctx.run_lane_older_waits() - w0
    assert ra.results_lagged(1) == wants[0][0] and ra.results_lagged(0) == wants[1][0]
    assert rb.results_lagged(1) == B.want()[0] and rb.results_lagged(0) == B.want()[0]
    ctx.sync()
    assert np.array_equal(_host(d_out, A.total), wants[1][2])
    for o in b_outs:
        assert np.array_equal(_host(o, B.total), B.clean_bytes)
    print("lane counters", d, "older waits", w)
    if ctx.lanes:
        # the first stands on the stream of the small table's last run; the others each go beside their predecessor
        assert d == dict(unordered=3, ordered=1, marks=0, off_lanes=0), d
        assert w == 1, (w, "0: the big run had ended before the fourth run was queued (three queue calls took > 0.3 ms)")
    else:
        assert d == dict(unordered=0, ordered=0, marks=0, off_lanes=4) and w == 0, (d, w)
    ra.close()
    rb.close()


def test_context_on_a_callers_stream(periodic):
    """A context created on a caller's stream never uses lanes, and a copy queued on that stream behind an async call reads the
    decoded bytes."""
    import os
    import torch
    from znippy_amd import hip
    A = periodic
    s = torch.cuda.Stream()
    old = os.environ.get("ZNIPPY_ROLES_MIN")
    os.environ["ZNIPPY_ROLES_MIN"] = "1"
    try:
        c = hip.Context(0, stream=s.cuda_stream)
    finally:
        if old is None:
            del os.environ["ZNIPPY_ROLES_MIN"]
        else:
            os.environ["ZNIPPY_ROLES_MIN"] = old
    rt = A.table(c)
    d_blob, warm = A.d_blob(), A.d_out()
    _warm(c, rt, d_blob, warm)
    for k in range(3):
        fresh = A.d_out(0xEE)
        torch.cuda.synchronize()
        rt.decode_verify_async(d_blob, fresh)
        with torch.cuda.stream(s):
            copy = fresh.clone()
        s.synchronize()
        assert np.array_equal(_host(copy, A.total), A.clean_bytes), k
        assert rt.results_lagged(0) == A.want()[0]
    st = c.run_lane_stats()
    assert st == dict(unordered=0, ordered=0, marks=0, off_lanes=5), st   # (every run but the first was lean)
    rt.close()
    c.close()


KINDS = "DDVDVVDPDVDDPVD"
_kinds_ref = {}


def _run_kinds(c, A, d_blob, outs):
    rt = A.table(c)
    got = []
    for k, kind in enumerate(KINDS):
        if kind == "D": rt.decode_verify_async(d_blob, outs[k & 1])
        elif kind == "V": rt.verify_async(d_blob)
        else: rt.decode_async(d_blob, outs[k & 1])
        if k:
            got.append(rt.results_lagged(1))
    got.append(rt.results_lagged(0))
    c.sync()
    res = (got, [_host(o, A.total).copy() for o in outs])
    rt.close()
    return res


def test_run_kinds_mixed_into_a_lean_pipeline(ctx, periodic):
    """Verify-only and decode-only runs mixed into a lean pipeline on one table: the
    results are those of the same sequence on a context without lanes, and the oracle's."""
    A = periodic
    d_blob = A.d_blob()
    if not _kinds_ref:
        c0 = make_ctx(dict(ZNIPPY_ROLES_MIN="1", ZNIPPY_NO_RUN_LANES="1"))
        _kinds_ref["ref"] = _run_kinds(c0, A, d_blob, [A.d_out(), A.d_out()])
        c0.close()
    ref = _kinds_ref["ref"]
    s0 = ctx.run_lane_stats()
    got = _run_kinds(ctx, A, d_blob, [A.d_out(), A.d_out()])
    assert got[0] == ref[0]
    for k, kind in enumerate(KINDS):
        if kind != "P":
            assert got[0][k] == A.want()[0], (k, kind)
    for o, r in zip(got[1], ref[1]):
        assert np.array_equal(o, r) and np.array_equal(o, A.clean_bytes)
    d = _delta(ctx, s0)
    if ctx.lanes:
        assert d["unordered"] >= 4 and d["marks"] >= 2 and d["off_lanes"] == 0, d   # (D and V runs side by side; marks behind the P runs)
    else:
        assert d["unordered"] == 0 and d["ordered"] == 0, d


def test_destroy_with_lane_runs_queued(ctx, periodic):
    """A table destroyed, and a context closed, with two lean runs queued and unread: the process goes on and a fresh context on
    the device works."""
    A = periodic
    d_blob, outs = A.d_blob(), [A.d_out(), A.d_out()]
    rt = A.table(ctx)
    _warm(ctx, rt, d_blob, outs[0])
    rt.decode_verify_async(d_blob, outs[1])
    rt.decode_verify_async(d_blob, outs[0])
    rt.close()
    rt = A.table(ctx)   # (takes the destroyed table's buffers from the context's pool)
    s0 = _warm(ctx, rt, d_blob, outs[0])
    rt.decode_verify_async(d_blob, outs[1])
    rt.decode_verify_async(d_blob, outs[0])
    if ctx.lanes:
        assert _delta(ctx, s0)["unordered"] == 2
    ctx.close()
    c = make_ctx(dict(ZNIPPY_ROLES_MIN="1"))
    rt = A.table(c)
    fresh = A.d_out(0xEE)
    counters, corrupt, status = rt.decode_verify(d_blob, fresh)
    assert counters == A.want()[0] and len(corrupt) == 0 and (status == 0).all()
    assert np.array_equal(_host(fresh, A.total), A.clean_bytes)
    rt.close()
    c.close()
