"""Content checksums on the batch and resolve paths (znippy_ctx_set_batch_checksums): with the context's switch
on, zstd frames that end with an XXH64 trailer go through the lane-per-block kernels and the resolve stages like any other
foreign frame, and the checksum stage (zstd_batch_checksum) checks the trailer; a frame whose trailer differs goes to the
serial decoder, which reports ZNIPPY_E_CHECKSUM.  The switch is off by default, and then nothing changes.

Every checksummed frame has a TWIN: the same bytes with the Content_Checksum bit of the frame header cleared and the last four
bytes dropped — the frame the batch path has always taken.  Routing is compared with the twin's."""
import numpy as np
import pytest

import gen
import workloads
import zstd_synth
from gpu_cases import frame_table, make_ctx, py_corpus

pytestmark = pytest.mark.gpu

E_CHECKSUM = -7
HIGH_BASE = (1 << 40) + 12345


def twin(frame):
    assert frame[4] & 4
    return frame[:4] + bytes([frame[4] & ~4]) + frame[5:-4]


def flagged(frame):
    return len(frame) > 4 and frame[:4] == zstd_synth.MAGIC and bool(frame[4] & 4)


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = make_ctx({})
    assert c.batch_checksums() == 0  # off by default
    yield c
    c.close()


class Table:
    """Entries and their frames as one row table of a context; run() is one run of it with the switch as given."""

    def __init__(self, ctx, oracle, entries, frames, blob_base=0):
        import torch
        from znippy_amd import hip
        self.ctx, self.entries, self.frames, self.base = ctx, entries, frames, blob_base
        self.A = A = frame_table(oracle, entries, frames)
        self.d_blobs = torch.from_numpy(A["blobs"].copy()).cuda()
        self.total = int(A["us"].sum())
        self.d_out = torch.zeros(self.total + 64, dtype=torch.uint8, device="cuda")
        self.rt = hip.RowTable(ctx, A["bo"] + np.uint64(blob_base), A["bs"], A["us"], A["oo"], None, A["ck"])

    def run(self, on, kind="decode_verify"):
        self.ctx.set_batch_checksums(on)
        try:
            self.d_out.zero_()
            kw = dict(blob_base=self.base, blob_cap=self.d_blobs.numel())
            if kind == "decode_verify":
                c, corrupt, status = self.rt.decode_verify(self.d_blobs, self.d_out, **kw)
            elif kind == "decode":
                self.rt.decode_async(self.d_blobs, self.d_out, **kw)
                c, corrupt, status = self.rt.results()
            else:
                c, corrupt, status = self.rt.verify(self.d_blobs, **kw)
            return dict(c=dict(c), corrupt=sorted(int(x) for x in corrupt), status=status.copy(), out=self.d_out[:self.total].cpu().numpy(),
                        fs=self.rt.foreign_stats(), cs=self.rt.checksum_stats(), kt=dict(self.ctx.kernel_times()),
                        dig=self.rt.digests().copy() if kind != "decode" else None)
        finally:
            self.ctx.set_batch_checksums(0)

    def row(self, res, i):
        a = int(self.A["oo"][i])
        return res["out"][a:a + int(self.A["us"][i])].tobytes()

    def close(self):
        self.rt.close()


def clean(t, res, rows=None):
    """Every row (or `rows`) decoded to its source, nothing corrupt, no error."""
    rows = range(len(t.entries)) if rows is None else rows
    assert all(res["status"][i] == 0 for i in rows), [(i, int(res["status"][i])) for i in rows if res["status"][i] != 0][:8]
    assert not set(res["corrupt"]) & set(rows), res["corrupt"][:8]
    for i in rows:
        assert t.row(res, i) == t.entries[i], i


# ---- routing and parity -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def routing_rows():
    """Pseudo-text of every length 0..99, 240 rows of 2-30 KiB of real text with odd lengths, three multi-block rows (the last two
    above RX_MIN); levels 3 and 19 mixed.  -> entries, checksummed frames."""
    rng = np.random.default_rng(20240)
    text = py_corpus(6 << 20)
    entries = [gen.pseudo_text(n, seed=n + 1) for n in range(100)]
    at = 0
    for _ in range(240):
        n = int(rng.integers(2048, 30 * 1024)) | 1
        entries.append(text[at:at + n])
        at += n
    for n in (131_073, 262_145, 300_001):
        entries.append(text[at:at + n])
        at += n
    assert at <= len(text) and all(len(e) == n for e, n in zip(entries[-3:], (131_073, 262_145, 300_001)))
    frames = [workloads.libzstd_compress_adv(e, level=(3, 19)[i % 2], checksum=True) for i, e in enumerate(entries)]
    for e, f in zip(entries[:100:7] + entries[-3:], frames[:100:7] + frames[-3:]):  # the trailer is what zstd_synth.xxh64 says
        assert int.from_bytes(f[-4:], "little") == zstd_synth.xxh64(e) & 0xFFFFFFFF
    return entries, frames


def _routing(ctx, oracle, entries, frames, label):
    """Twins with the switch off, then the checksummed table on / off / on: every run clean and alike.  -> N0 (the twins the batch
    path decoded), the first run with the switch on."""
    assert all(flagged(f) for f in frames)
    tw = Table(ctx, oracle, entries, [twin(f) for f in frames])
    r0 = tw.run(0)
    clean(tw, r0)
    n0 = r0["fs"]["frames"]
    assert r0["cs"] == dict(verified=0, mismatched=0, bytes=0) and "zstd_batch_checksum" not in r0["kt"]
    tw.close()
    t = Table(ctx, oracle, entries, frames)
    on = t.run(1)
    off = t.run(0)
    on2 = t.run(1)
    print(f"routing ({label}): rows {len(frames)}; twins through the batch path {n0}; checksummed, switch on: frames {on['fs']['frames']} "
          f"checksum {on['cs']}; switch off: frames {off['fs']['frames']} checksum {off['cs']}")
    for res in (on, off, on2):
        clean(t, res)
        assert res["c"]["decode_errors"] == 0 and res["c"]["corrupt_rows"] == 0
        assert np.array_equal(res["dig"], t.A["ck"])
    assert "zstd_batch_checksum" in on["kt"] and "zstd_resolve_store" in on["kt"]
    # with the switch off the batch path decodes what the parent's does: the frames without the flag, of which this table has none
    assert off["fs"]["frames"] == sum(not flagged(f) for f in frames) == 0
    assert off["cs"] == dict(verified=0, mismatched=0, bytes=0) and "zstd_batch_checksum" not in off["kt"]
    assert on2["cs"] == on["cs"] and on2["fs"]["frames"] == on["fs"]["frames"]
    assert (on["status"] == off["status"]).all() and on["c"] == off["c"] and (on["out"] == off["out"]).all()
    t.close()
    return n0, on


def test_routing_and_parity_with_twins(ctx, oracle, routing_rows):
    """The rows above 99 bytes: the batch path decodes a checksummed frame exactly when it decodes the twin, and checks each."""
    entries, frames = routing_rows[0][100:], routing_rows[1][100:]
    n0, on = _routing(ctx, oracle, entries, frames, "rows above 99 bytes")
    assert n0 == len(frames)
    assert on["fs"]["frames"] == n0, (on["fs"], n0)
    assert on["cs"] == dict(verified=n0, mismatched=0, bytes=sum(len(e) for e in entries)), (on["cs"], n0)


def test_routing_with_tiny_rows(ctx, oracle, routing_rows):
    """The whole table, rows of 0..99 bytes included.  Most of those are one raw block, a shape the small-row kernels decode by
    themselves when the frame has no trailer: such a twin never reaches the batch path, its checksummed frame (which those
    kernels hand over, as ever) does.  So here the batch path's count with the switch on is NOT the twins' N0 — measured on an
    MI355X: 343 rows, N0 = 256, with the switch on 343 frames decoded and 343 trailers checked.  What holds, and is asserted, is
    the stronger half: every checksummed row — the N0 and the rest — is decoded and checked by the batch path, none is left to the
    serial decoder."""
    entries, frames = routing_rows
    n0, on = _routing(ctx, oracle, entries, frames, "all rows")
    assert n0 <= len(frames)
    assert on["fs"]["frames"] == len(frames), (on["fs"], n0)
    assert on["cs"] == dict(verified=len(frames), mismatched=0, bytes=sum(len(e) for e in entries)), (on["cs"], n0)


def test_big_frames_resolve_and_checksum(ctx, oracle):
    """Two frames of 600,001 bytes: a table small enough that every frame above 64 KiB is resolved."""
    text = py_corpus(2 << 20)
    entries = [text[:600_001], text[700_000:700_000 + 600_001]]
    frames = [workloads.libzstd_compress_adv(e, level=lv, checksum=True) for e, lv in zip(entries, (19, 3))]
    tw = Table(ctx, oracle, entries, [twin(f) for f in frames])
    n0 = tw.run(0)["fs"]["frames"]
    tw.close()
    t = Table(ctx, oracle, entries, frames)
    on, off = t.run(1), t.run(0)
    clean(t, on); clean(t, off)
    assert n0 == 2 and on["fs"]["frames"] == n0 and off["fs"]["frames"] == 0
    assert on["cs"] == dict(verified=2, mismatched=0, bytes=1_200_002)
    assert "zstd_resolve_store" in on["kt"] and "zstd_batch_checksum" in on["kt"]
    assert off["cs"]["verified"] == 0 and "zstd_batch_checksum" not in off["kt"]
    t.close()


# ---- wave packing -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_rows():
    text = py_corpus(1 << 20)
    entries = [text[3000 * i + i:3000 * i + i + 3071 + (i % 5)] for i in range(65)]
    frames = [workloads.libzstd_compress_adv(e, level=(3, 19)[i % 2], checksum=True) for i, e in enumerate(entries)]
    return entries, frames


@pytest.mark.parametrize("n", [1, 15, 16, 17, 64, 65])
def test_wave_packing(ctx, oracle, small_rows, n):
    entries, frames = small_rows[0][:n], small_rows[1][:n]
    t = Table(ctx, oracle, entries, frames)
    on = t.run(1)
    clean(t, on)
    assert on["cs"] == dict(verified=n, mismatched=0, bytes=sum(len(e) for e in entries)), on["cs"]
    assert on["fs"]["frames"] == n
    t.close()


def test_checksummed_and_plain_frames_alternate(ctx, oracle, small_rows):
    entries, frames = small_rows
    mixed = [f if i % 2 else twin(f) for i, f in enumerate(frames)]
    n_ck = sum(flagged(f) for f in mixed)
    t = Table(ctx, oracle, entries, mixed)
    on, off = t.run(1), t.run(0)
    clean(t, on); clean(t, off)
    assert on["cs"] == dict(verified=n_ck, mismatched=0, bytes=sum(len(e) for e, f in zip(entries, mixed) if flagged(f)))
    assert on["fs"]["frames"] == len(mixed) and off["fs"]["frames"] == len(mixed) - n_ck  # the parent's count: the frames without the flag
    assert off["cs"]["verified"] == 0
    t.close()


# ---- a mismatch only the checksum can see ----------------------------------------------------------------------------------------

def _flip(frame, at):
    b = bytearray(frame)
    b[at] ^= 0x21
    return bytes(b)


@pytest.mark.parametrize("size", [5 * 1024, 300_001])
def test_payload_damage_is_the_checksums_to_find(ctx, oracle, size):
    """Random bytes become raw blocks: a flipped payload byte decodes without complaint, only the content differs."""
    rng = np.random.default_rng(size)
    entries = [rng.integers(0, 256, size, dtype=np.uint8).tobytes() for _ in range(5)]
    frames = [workloads.libzstd_compress_adv(e, level=3, checksum=True) for e in entries]
    assert all(len(f) >= size for f in frames)  # stored as raw blocks
    bad = [_flip(f, len(f) // 2 + 7) if i in (1, 3) else f for i, f in enumerate(frames)]
    for i in (1, 3):  # libzstd's verdict on these mutants and on their twins
        with pytest.raises(RuntimeError):
            workloads.libzstd_decompress(bad[i], size)
        assert workloads.libzstd_decompress(twin(bad[i]), size) != entries[i]
    t = Table(ctx, oracle, entries, bad)
    on = t.run(1)
    assert [int(s) for s in on["status"]] == [0, E_CHECKSUM, 0, E_CHECKSUM, 0], on["status"]
    assert on["c"]["decode_errors"] == 2 and on["c"]["corrupt_rows"] == 0
    assert on["cs"]["mismatched"] == 2 and on["cs"]["verified"] == 3, on["cs"]
    clean(t, on, rows=(0, 2, 4))
    assert "zstd_batch_checksum" in on["kt"]
    off = t.run(0)
    assert (off["status"] == on["status"]).all() and off["c"] == on["c"]
    t.close()
    # the same mutants of the twins: nothing the decoder can see, two rows the BLAKE3 verify flags — the -7 above is the stage's doing
    tw = Table(ctx, oracle, entries, [twin(f) for f in bad])
    r = tw.run(1)
    assert (r["status"] == 0).all() and r["corrupt"] == [1, 3] and r["c"]["corrupt_rows"] == 2
    assert r["cs"] == dict(verified=0, mismatched=0, bytes=0)
    tw.close()


def test_damaged_trailers(ctx, oracle, small_rows):
    entries, frames = small_rows[0][:6], list(small_rows[1][:6])
    frames[1] = _flip(frames[1], len(frames[1]) - 1)      # a trailer byte
    frames[2] = _flip(frames[2], len(frames[2]) - 4)
    frames[4] = frames[4][:-2]                             # a truncated trailer
    lits = gen.pseudo_text(700, seed=9)
    entries = entries + [lits, lits]
    frames += [zstd_synth.write_frame([zstd_synth.Raw(lits)], checksum=True, bad_checksum=True),
               zstd_synth.write_frame([zstd_synth.Raw(lits[:300]), zstd_synth.Raw(lits[300:])], checksum=True)]
    t = Table(ctx, oracle, entries, frames)
    on, off = t.run(1), t.run(0)
    for i in (1, 2, 6):
        assert on["status"][i] == E_CHECKSUM, (i, on["status"])
    with pytest.raises(ValueError):
        oracle.zstd_decompress(frames[4], cap=len(entries[4]))
    assert on["status"][4] < 0 and on["status"][4] == off["status"][4]  # the serial decoder's verdict on the truncation, as ever
    clean(t, on, rows=(0, 3, 5, 7))
    assert (on["status"] == off["status"]).all() and on["c"] == off["c"] and on["c"]["decode_errors"] == 4
    assert on["cs"]["mismatched"] == 3 and on["cs"]["verified"] == 4, on["cs"]
    t.close()


# ---- verdict parity on damaged frames ----------------------------------------------------------------------------------------------

MUTANT_SEED = 77001


def _mutants():
    """200 single-byte mutants, anywhere in three checksummed frames in turn -> the rows' sources, the damaged frames."""
    text = py_corpus(1 << 20)
    bases = [(text[:6 * 1024], 19), (text[100_000:100_000 + 262_145], 19), (text[500_000:500_000 + 20 * 1024], 3)]
    base_frames = [workloads.libzstd_compress_adv(data, level=lv, checksum=True) for data, lv in bases]
    rng = np.random.default_rng(MUTANT_SEED)
    entries, frames = [], []
    for k in range(200):
        f = bytearray(base_frames[k % 3])
        f[int(rng.integers(0, len(f)))] ^= int(rng.integers(1, 256))
        entries.append(bases[k % 3][0]); frames.append(bytes(f))
    return entries, frames


def test_mutants_agree_with_oracle(ctx, oracle):
    entries, frames = _mutants()
    verdict = []
    for e, f in zip(entries, frames):
        try:
            w = oracle.zstd_decompress(f, cap=len(e))
            verdict.append(w if len(w) == len(e) else None)
        except ValueError:
            verdict.append(None)
    n_rej = sum(v is None for v in verdict)
    assert n_rej >= 150, n_rej
    t = Table(ctx, oracle, entries, frames)
    on = t.run(1)
    print(f"mutants: {len(frames)} rows, rejected by the oracle {n_rej}, checksum stage {on['cs']}, batch frames {on['fs']['frames']}")
    for i, v in enumerate(verdict):
        assert (on["status"][i] >= 0) == (v is not None), (i, int(on["status"][i]))
        if v is not None:
            assert t.row(on, i) == v, i
            assert (i in on["corrupt"]) == (v != entries[i]), i  # never reported verified with other bytes
    assert on["c"]["decode_errors"] == n_rej
    off = t.run(0)
    assert (on["status"] == off["status"]).all() and on["c"] == off["c"] and on["corrupt"] == off["corrupt"]
    t.close()


# ---- run kinds ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["decode", "verify"])
def test_decode_only_and_verify_only_runs(ctx, oracle, routing_rows, kind):
    entries, frames = list(routing_rows[0]), list(routing_rows[1])
    entries.append(entries[150]); frames.append(_flip(frames[150], len(frames[150]) - 2))  # one damaged trailer
    bad = len(frames) - 1
    t = Table(ctx, oracle, entries, frames)
    on = t.run(1, kind)
    off = t.run(0, kind)
    good = list(range(bad))
    assert on["status"][bad] == E_CHECKSUM and (on["status"][:bad] == 0).all(), on["status"][on["status"] != 0]
    assert on["c"]["decode_errors"] == 1 and on["c"]["corrupt_rows"] == 0  # an error, not a verified row, in either kind
    assert on["c"] == off["c"] and (on["status"] == off["status"]).all()
    assert on["cs"]["mismatched"] == 1 and on["cs"]["verified"] > 0 and "zstd_batch_checksum" in on["kt"]
    assert off["cs"] == dict(verified=0, mismatched=0, bytes=0) and "zstd_batch_checksum" not in off["kt"]
    assert on["c"]["verified_bytes"] == sum(len(e) for e in entries[:bad])  # (the damaged row is not among the rows a run counts as done)
    if kind == "decode":
        clean(t, on, rows=good)
    else:
        assert np.array_equal(on["dig"][:bad], t.A["ck"][:bad])
    t.close()


# ---- the switch ---------------------------------------------------------------------------------------------------------------

def test_setter_getter_and_environment(ctx):
    from znippy_amd import hip
    assert ctx.batch_checksums() == 0
    ctx.set_batch_checksums(1)
    assert ctx.batch_checksums() == 1
    for v in (2, -1):
        assert ctx.L.znippy_ctx_set_batch_checksums(ctx.h, v) == -1  # ZNIPPY_E_INVAL
        with pytest.raises(Exception):
            ctx.set_batch_checksums(v)
    assert ctx.batch_checksums() == 1
    ctx.set_batch_checksums(0)
    assert ctx.batch_checksums() == 0
    c1 = make_ctx({"ZNIPPY_BX_CHECKSUM": "1"})
    c0 = make_ctx({"ZNIPPY_BX_CHECKSUM": "0"})
    assert c1.batch_checksums() == 1 and c0.batch_checksums() == 0
    c1.close(); c0.close()
    c = make_ctx({})
    h, L = c.h, c.L
    rt = hip.RowTable(c, np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint64), None, np.zeros((1, 32), np.uint8))
    c._tables.discard(rt)
    L.znippy_ctx_destroy(h)  # a table keeps it alive: closed
    assert L.znippy_ctx_set_batch_checksums(h, 1) == -1 and L.znippy_ctx_set_batch_checksums(h, 0) == -1
    assert L.znippy_ctx_batch_checksums(h) == -1
    rt.close()  # the last table: the context is released
    c.h = None


def test_no_serial_fallback_context(oracle):
    """ZNIPPY_FZ_ONLY: nothing behind the batch path.  A row with a damaged trailer is left over — never hashed, so it shows as a
    corrupt row like everything that path leaves —, and the valid checksummed table decodes there.  (Rows of this test's own, the
    damaged table first: a row that is not hashed keeps whatever its digest slot held.)"""
    c = make_ctx({"ZNIPPY_FZ_ONLY": "1", "ZNIPPY_BX_CHECKSUM": "1"})
    try:
        assert c.batch_checksums() == 1
        entries = [gen.pseudo_text(3001 + 13 * i, seed=9100 + i) for i in range(20)]
        frames = [workloads.libzstd_compress_adv(e, level=(3, 19)[i % 2], checksum=True) for i, e in enumerate(entries)]
        bad = list(frames)
        bad[7] = _flip(bad[7], len(bad[7]) - 3)
        t = Table(c, oracle, entries, bad)
        on = t.run(1)
        assert on["corrupt"] == [7] and on["cs"]["mismatched"] == 1 and on["cs"]["verified"] == 19, (on["corrupt"], on["cs"])
        clean(t, on, rows=[i for i in range(20) if i != 7])
        t.close()
        t = Table(c, oracle, entries, frames)
        on = t.run(1)
        clean(t, on)
        assert on["c"]["corrupt_rows"] == 0 and on["cs"] == dict(verified=20, mismatched=0, bytes=sum(len(e) for e in entries))
        t.close()
    finally:
        c.close()


# ---- far offsets ---------------------------------------------------------------------------------------------------------------

def test_blob_base_above_2_40(ctx, oracle, small_rows, routing_rows):
    entries = small_rows[0][:17] + routing_rows[0][:40] + routing_rows[0][-2:]
    frames = small_rows[1][:17] + routing_rows[1][:40] + routing_rows[1][-2:]
    mixed = [f if i % 3 else twin(f) for i, f in enumerate(frames)]
    t = Table(ctx, oracle, entries, mixed, blob_base=HIGH_BASE)
    on = t.run(1)
    clean(t, on)
    near = Table(ctx, oracle, entries, mixed)
    want = near.run(1)
    assert on["cs"] == want["cs"] and on["cs"]["verified"] > 0 and on["cs"]["mismatched"] == 0
    assert on["fs"]["frames"] == want["fs"]["frames"] and on["c"] == want["c"]
    t.close(); near.close()
