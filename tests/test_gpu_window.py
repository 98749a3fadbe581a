"""The encoder's opt-in cross-block match window (znippy_ctx_set_window_log).

Window 0 (the default) keeps every 128 KiB block self-contained; 17..27 lets the higher effort tier reach up to
2^window_log bytes back inside the round: the near window (the 64 KiB in front of a block, through the LDS buckets)
and the far window (long-distance matches through k_ldm_index).  What is checked here: far and near repeats shrink,
the frames are valid for two independent decoders and for every read path of this build, nothing changes with the
window off (or where it cannot apply), the output is deterministic and independent of how rounds are batched, and
every layer of the interface carries the setting.  All inputs come from seeded generators below."""
import os
import subprocess
import sys

import numpy as np
import pytest

import workloads
from gpu_cases import make_ctx

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
BLOCK = 128 * KiB


# ---- inputs --------------------------------------------------------------------------------------------------------

def far_round(seed=1):
    """8 MiB: 2 MiB of random bytes, then three copies of them with ~0.1 % of the bytes flipped."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, 2 * MiB, dtype=np.uint8)
    parts = [base]
    for _ in range(3):
        c = base.copy()
        idx = rng.choice(c.size, c.size // 1000, replace=False)
        c[idx] ^= rng.integers(1, 256, idx.size, dtype=np.uint8)
        parts.append(c)
    return np.concatenate(parts).tobytes()


def near_round(seed, n=4 * MiB):
    """Random blocks; every block but the first starts with 16 KiB copied from 20-40 KiB in front of it."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, n, dtype=np.uint8)
    for s in range(BLOCK, n, BLOCK):
        back = int(rng.integers(20 * KiB, 40 * KiB + 1))
        d[s:s + 16 * KiB] = d[s - back:s - back + 16 * KiB]
    return d.tobytes()


def mixed(n, seed):
    """Zipf-word text, binary-like records and runs, with some segments repeated (changed a little) from far behind."""
    rng = np.random.default_rng(seed)
    vocab = [bytes(rng.integers(97, 123, int(rng.integers(2, 10)), dtype=np.uint8)) for _ in range(3000)]
    zipf = 1.0 / np.arange(1, len(vocab) + 1)
    zipf /= zipf.sum()
    out, size = [], 0
    while size < n:
        kind = rng.integers(0, 4)
        ln = int(rng.integers(1 * KiB, 48 * KiB))
        if kind == 0:
            words = rng.choice(len(vocab), ln // 5 + 1, p=zipf)
            seg = b" ".join(vocab[w] for w in words)[:ln]
        elif kind == 1:
            k = ln // 24 + 1
            rec = np.zeros((k, 24), np.uint8)
            rec[:, 0:4] = np.arange(k, dtype=np.uint32).view(np.uint8).reshape(k, 4)
            rec[:, 4:6] = rng.integers(0, 4, (k, 2), dtype=np.uint8)
            rec[:, 8:16] = rng.integers(0, 256, (k, 8), dtype=np.uint8)
            rec[:, 16:24] = np.frombuffer(b"RECORD\x00\x01", np.uint8)
            seg = rec.tobytes()[:ln]
        elif kind == 2:
            seg = bytes([int(rng.integers(0, 256))]) * ln
        else:
            blob = b"".join(out)
            if len(blob) < 64 * KiB:
                continue
            st = int(rng.integers(0, len(blob) - 16 * KiB))
            seg = bytearray(blob[st:st + ln])
            for i in rng.integers(0, len(seg), len(seg) // 2000 + 1):
                seg[int(i)] ^= 0x5A
            seg = bytes(seg)
        out.append(seg)
        size += len(seg)
    return b"".join(out)[:n]


SIZES = [0, 1, 4095, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1, MiB + 7, 3 * MiB, 9 * MiB]


def mixed_rounds(seed=7):
    return [mixed(n, seed + i) for i, n in enumerate(SIZES)]


# ---- helpers -------------------------------------------------------------------------------------------------------

def encode(ctx, rounds, level=19, window_log=None):
    """Frames of `rounds` encoded as one table (znippy_encode_hash_rounds) and their digests."""
    import torch
    from znippy_amd import hip
    ctx.set_level(level)
    if window_log is not None:
        ctx.set_window_log(window_log)
    lens = np.array([len(r) for r in rounds], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    src = np.frombuffer(b"".join(rounds) + bytes(64), np.uint8)
    rt = hip.RoundTable(ctx, offs, lens)
    d_src = torch.from_numpy(src.copy()).cuda()
    d_out = torch.zeros(rt.blob_bound() + 64, dtype=torch.uint8, device="cuda")
    res = rt.encode_hash(d_src, d_out)
    bo, bs, ck = res["blob_offset"].copy(), res["blob_size"].copy(), res["checksum"].copy()
    blob = d_out[:res["blob_bytes"]].cpu().numpy().tobytes()
    rt.close()
    assert (res["compressed"] == 1).all()
    return [blob[int(o):int(o) + int(s)] for o, s in zip(bo, bs)], ck


def blocks(frame):
    """(type, size, last) of every block of one single-segment frame (RFC 8878 3.1.1)."""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    fhd = frame[4]
    assert fhd & 0x20 and not fhd & 0x04 and not fhd & 0x03  # single segment, no checksum, no dictionary
    fcs = {0: 1, 1: 2, 2: 4, 3: 8}[fhd >> 6]
    p, out = 5 + fcs, []
    while True:
        h = frame[p] | frame[p + 1] << 8 | frame[p + 2] << 16
        t, sz, last = (h >> 1) & 3, h >> 3, h & 1
        out.append((t, sz, last))
        p += 3 + (1 if t == 1 else sz)
        if last:
            break
    assert p == len(frame)
    return out


def tail_marked(frame):
    b = blocks(frame)
    return len(b) > 1 and b[-1] == (0, 0, 1)


def check_decoders(oracle, rounds, frames):
    for r, f in zip(rounds, frames):
        assert workloads.libzstd_decompress(f, len(r)) == r
        assert oracle.zstd_decompress(f) == r


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = make_ctx({})
    yield c
    c.close()


@pytest.fixture(scope="module")
def far_data():
    return far_round()


@pytest.fixture(scope="module")
def near_data():
    return [near_round(11), near_round(12)]


@pytest.fixture(scope="module")
def mixed_data():
    return mixed_rounds()


@pytest.fixture(scope="module")
def windowed(ctx, far_data, near_data, mixed_data):
    """One table of every input at level 19, window 23: what the read paths are given."""
    rounds = mixed_data + near_data + [far_data]
    frames, ck = encode(ctx, rounds, 19, 23)
    ctx.set_window_log(0)
    return rounds, frames, ck


# ---- 1, 2: ratio ---------------------------------------------------------------------------------------------------

def test_far_repeats_shrink(ctx, oracle, far_data):
    (f23,), _ = encode(ctx, [far_data], 19, 23)
    (f0,), _ = encode(ctx, [far_data], 19, 0)
    n = len(far_data)
    print(f"far repeats: window 0 {len(f0) / n:.4f}, window 23 {len(f23) / n:.4f}")
    assert len(f23) / n <= 0.35
    assert len(f0) / n >= 0.95
    check_decoders(oracle, [far_data], [f23])


def test_near_window_shrinks(ctx, oracle, near_data):
    f17, _ = encode(ctx, near_data, 19, 17)
    f0, _ = encode(ctx, near_data, 19, 0)
    b17, b0 = sum(map(len, f17)), sum(map(len, f0))
    print(f"near window: window 0 {b0} B, window 17 {b17} B ({1 - b17 / b0:.1%} fewer)")
    assert b17 <= 0.9 * b0
    check_decoders(oracle, near_data, f17)


# ---- 3: frames are valid -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [4, 19, 22])
@pytest.mark.parametrize("window_log", [17, 23, 27])
def test_frames_decode_with_two_decoders(ctx, oracle, mixed_data, level, window_log):
    frames, _ = encode(ctx, mixed_data, level, window_log)
    for r, f in zip(mixed_data, frames):
        blocks(f)  # plain single-segment frames, no checksum, no dictionary
        assert len(f) <= ctx.compress_bound(len(r))
    check_decoders(oracle, mixed_data, frames)
    ctx.set_window_log(0)


def test_windowed_table_decodes_with_two_decoders(oracle, windowed):
    rounds, frames, _ = windowed
    check_decoders(oracle, rounds, frames)


# ---- 4: every read path ---------------------------------------------------------------------------------------------

READ_PATHS = [
    ("default", {}),
    ("no_bx", {"ZNIPPY_NO_BX": "1"}),
    ("no_fz", {"ZNIPPY_NO_FZ": "1"}),
    ("no_bx+no_fz", {"ZNIPPY_NO_BX": "1", "ZNIPPY_NO_FZ": "1"}),
    ("no_rx", {"ZNIPPY_NO_RX": "1"}),
    ("no_block_items", {"ZNIPPY_NO_BLOCK_ITEMS": "1"}),
    ("no_fused_blocks", {"ZNIPPY_NO_FUSED_BLOCKS": "1"}),
]


@pytest.mark.parametrize("env", [e for _, e in READ_PATHS], ids=[n for n, _ in READ_PATHS])
def test_every_read_path_decodes_windowed_frames(oracle, windowed, env):
    import torch
    from znippy_amd import hip
    rounds, frames, ck = windowed
    rc = make_ctx(env)
    try:
        us = np.array([len(r) for r in rounds], np.uint64)
        oo = np.concatenate([[0], np.cumsum(us)[:-1]]).astype(np.uint64)
        bs = np.array([len(f) for f in frames], np.uint64)
        bo = np.concatenate([[0], np.cumsum(bs)[:-1]]).astype(np.uint64)
        want_ck = np.stack([np.frombuffer(oracle.blake3(r), np.uint8) for r in rounds])
        assert (ck == want_ck).all()  # the write side's digests
        d_blobs = torch.from_numpy(np.frombuffer(b"".join(frames) + bytes(64), np.uint8).copy()).cuda()
        total = int(us.sum())
        d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        rt = hip.RowTable(rc, bo, bs, us, oo, None, want_ck)
        for _ in range(2):  # the second run uses what the table learned from the first
            d_out.zero_()
            counters, corrupt, status = rt.decode_verify(d_blobs, d_out)
            assert counters["corrupt_rows"] == 0 and counters["decode_errors"] == 0, (counters, corrupt[:8])
            assert (status == 0).all()
            assert counters["verified_bytes"] == total
            assert d_out[:total].cpu().numpy().tobytes() == b"".join(rounds)
            assert (rt.digests() == want_ck).all()
        rt.close()
    finally:
        rc.close()


# ---- 5: off means unchanged ----------------------------------------------------------------------------------------

def test_new_context_has_no_window():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = make_ctx({})
    try:
        assert c.window_log == 0
    finally:
        c.close()


def test_default_equals_explicit_zero(mixed_data):
    a = make_ctx({})
    try:
        f_default, _ = encode(a, mixed_data, 19)
    finally:
        a.close()
    b = make_ctx({})
    try:
        f_zero, _ = encode(b, mixed_data, 19, 0)
    finally:
        b.close()
    assert f_default == f_zero


def test_single_block_rounds_ignore_the_window(ctx, mixed_data):
    rounds = [r for r in mixed_data if len(r) <= BLOCK] + [near_round(5, BLOCK), far_round(3)[:BLOCK]]
    assert len(rounds) >= 6
    f23, _ = encode(ctx, rounds, 19, 23)
    f0, _ = encode(ctx, rounds, 19, 0)
    assert f23 == f0


@pytest.mark.parametrize("level", [1, 2, 3])
def test_fast_tier_ignores_the_window(ctx, mixed_data, far_data, level):
    rounds = mixed_data[-4:] + [far_data]
    f23, _ = encode(ctx, rounds, level, 23)
    assert ctx.window_log == 23  # kept, not used
    f0, _ = encode(ctx, rounds, level, 0)
    assert f23 == f0


def test_tail_mark_only_without_window(ctx, mixed_data, far_data):
    rounds = [r for r in mixed_data if len(r) > BLOCK] + [far_data]
    f0, _ = encode(ctx, rounds, 19, 0)
    f23, _ = encode(ctx, rounds, 19, 23)
    ctx.set_window_log(0)
    assert all(tail_marked(f) for f in f0)
    assert not any(tail_marked(f) for f in f23)


# ---- 6: determinism ------------------------------------------------------------------------------------------------

def test_deterministic_and_independent_of_batching(ctx, mixed_data, far_data, near_data):
    rounds = mixed_data + [far_data] + near_data
    a, _ = encode(ctx, rounds, 19, 23)
    b, _ = encode(ctx, rounds, 19, 23)
    assert a == b
    k = 5
    c1, _ = encode(ctx, rounds[k:], 19, 23)
    c2, _ = encode(ctx, rounds[:k], 19, 23)
    ctx.set_window_log(0)
    assert c2 + c1 == a


# ---- 7: interfaces -------------------------------------------------------------------------------------------------

def test_invalid_values_and_closed_context(ctx):
    from znippy_amd import hip
    from znippy_amd._lib import ZnippyError
    for v in (-1, 1, 16, 28, 31, 100):
        with pytest.raises(ZnippyError):
            ctx.set_window_log(v)
        assert ctx.window_log == 0
    for v in (17, 20, 27, 0):
        ctx.set_window_log(v)
        assert ctx.window_log == v
    c = make_ctx({})
    h, L = c.h, c.L
    rt = hip.RoundTable(c, np.zeros(1, np.uint64), np.ones(1, np.uint64))
    c._tables.discard(rt)
    L.znippy_ctx_destroy(h)  # a table keeps it alive: closed
    assert L.znippy_ctx_set_window_log(h, 17) == -1
    assert L.znippy_ctx_set_window_log(h, 0) == -1
    assert L.znippy_ctx_window_log(h) == -1
    rt.close()  # the last table: the context is released
    c.h = None


def test_codec_compress_ctx(ctx, oracle, far_data):
    from znippy_amd import codec
    cc = codec.CompressCtx(19, ctx=ctx, window_log=23)
    f = cc.compress(far_data)
    assert ctx.window_log == 23
    assert codec.decompress_frame(f, ctx=ctx) == far_data
    assert oracle.zstd_decompress(f) == far_data
    f0 = codec.CompressCtx(19, ctx=ctx).compress(far_data)
    assert ctx.window_log == 0
    assert len(f) < 0.5 * len(f0)


def _stream_archive(tmp_path, name, ents, window_log):
    from znippy_amd.stream_packer import compress_stream
    c = compress_stream(str(tmp_path / (name + ".tmp")), False, window_log=window_log)
    for e in ents:
        c.sender().send(e)
    c.finish()
    return tmp_path / (name + ".znippy")


def test_compress_stream_window(tmp_path, far_data, mixed_data):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd.decompress import decompress_archive
    from znippy_amd.stream_packer import ArchiveEntry
    ents = [ArchiveEntry("far.bin", far_data), ArchiveEntry("mixed.bin", mixed_data[-2]), ArchiveEntry("small.txt", mixed_data[3])]
    a23 = _stream_archive(tmp_path, "w23", ents, 23)
    a0 = _stream_archive(tmp_path, "w0", ents, 0)
    assert a23.stat().st_size < a0.stat().st_size - len(far_data) // 2
    for a, d in ((a23, "out23"), (a0, "out0")):
        rep = decompress_archive(a, True, tmp_path / d)
        assert rep.corrupt_files == 0 and rep.total_files == len(ents)
        for e in ents:
            assert (tmp_path / d / e.relative_path).read_bytes() == e.data


CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
from znippy_amd import host
from znippy_amd.stream_packer import ArchiveEntry
c = host.compress_stream(sys.argv[1], False)
c.sender().send(ArchiveEntry("far.bin", open(sys.argv[2], "rb").read()))
c.finish()
"""


def test_host_layer_reads_window_from_environment(tmp_path, far_data):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd.decompress import decompress_archive
    here = os.path.dirname(os.path.abspath(__file__))
    script = CHILD.format(root=os.path.dirname(here), tests=here)
    (tmp_path / "far.bin").write_bytes(far_data)
    sizes = {}
    for wl in ("23", "0"):
        env = dict(os.environ, ZNIPPY_WINDOW_LOG=wl)
        p = subprocess.run([sys.executable, "-c", script, str(tmp_path / f"w{wl}.tmp"), str(tmp_path / "far.bin")],
                           env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        a = tmp_path / f"w{wl}.znippy"
        sizes[wl] = a.stat().st_size
        rep = decompress_archive(a, True, tmp_path / f"out{wl}")
        assert rep.corrupt_files == 0 and rep.total_files == 1
        assert (tmp_path / f"out{wl}" / "far.bin").read_bytes() == far_data
    assert sizes["23"] < sizes["0"] // 2
