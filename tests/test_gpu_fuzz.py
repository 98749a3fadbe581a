"""Robustness: mutated frames through the batch decoder.  Every mutant is one index row; one
launch decodes them all.  Contract (decompress.rs:L159-162): a frame that fails to decode is a
per-row error, never a fault or a hang.  Cross-check with the oracle: whenever the oracle accepts
a mutant the GPU must accept it too and produce the same bytes; whenever the oracle rejects it,
the GPU must either reject it or (checksum-less frames carry no integrity) produce bytes the
BLAKE3 verify then flags — it must never report a verified row with different bytes.
"""
import numpy as np
import pytest

import gen
from gpu_cases import fuzz_run as _run

pytestmark = pytest.mark.gpu


def test_mutated_frames_never_fault_and_agree_with_oracle(gpu_ctx, oracle):
    bases = [(gen.text(10240), 19), (gen.binary(10240), 19), (gen.pseudo_text(6000, 3), 3), (gen.pseudo_text(6000, 4), 19),
             (gen.pseudo_text(70000, 5), 3), (gen.random_lcg(3000), 3), (bytes(5000), 3)]
    _run(gpu_ctx, oracle, bases, 120, 2024, 15, 200)


def test_mutated_multi_block_frames(gpu_ctx, oracle):
    """Frames of several blocks: the block-item path (header scan, speculative per-block decode, per-frame
    fallback), Huffman-coded literals and dense sequence sections written by this encoder, raw blocks, and
    libzstd's chained blocks — damaged anywhere, including block headers and sizes."""
    bases = [(gen.pseudo_text(300_000, 11), 3), (gen.binary(280_000), 19), (gen.text(400_000), 3),
             (gen.incompressible(6, 270_000), 1), (gen.pseudo_text(131_073, 12), 19)]
    _run(gpu_ctx, oracle, bases, 50, 77, 10, 60)


def _all_bit_flips(frame: bytes, rng, limit):
    """Every single-bit flip of the first `limit` bytes and of the last 16 (headers, literals, sequence section)."""
    n = len(frame)
    pos = sorted(set(range(min(n, limit))) | set(range(max(0, n - 16), n)))
    out = []
    for p in pos:
        for bit in range(8):
            b = bytearray(frame); b[p] ^= 1 << bit
            out.append(bytes(b))
    return out


def _periodic(period, n, seed):
    rng = np.random.default_rng(seed)
    p = rng.integers(32, 127, size=period, dtype=np.uint8).tobytes()
    return (p * (n // period + 1))[:n]


def test_every_bit_of_recognised_small_frames(gpu_ctx, oracle):
    """The lane-parallel recogniser of the fused kernel (parse_fast) against the oracle, exhaustively: every
    single-bit flip of whole small frames of the shape it takes (literals + one periodic match) — frame header,
    block header, literals header, the literals, sequence count, modes, bitstream."""
    bases = [(gen.text(10240), 19), (gen.text(10240), 1), (_periodic(7, 4096, 1), 3), (_periodic(200, 20480, 2), 19),
             (_periodic(1, 2048, 3), 3), (gen.binary(10240), 3)]
    _run(gpu_ctx, oracle, bases, 400, 5, 100, 300, mutants=_all_bit_flips)


def test_every_bit_of_block_heads_in_big_frames(gpu_ctx, oracle):
    """Same for the block half of the recogniser (fused block kernel): every bit of the first 96 bytes (frame
    header + first block) and of the tail of multi-block frames of periodic and raw data."""
    bases = [(_periodic(45, 3 * 128 * 1024, 4), 3), (gen.incompressible(8, 2 * 128 * 1024 + 5000), 1)]
    _run(gpu_ctx, oracle, bases, 96, 6, 20, 100, mutants=_all_bit_flips)


def test_every_bit_of_entropy_headers_in_text_frames(gpu_ctx, oracle):
    """The general decoder's table readers against the oracle, exhaustively: every single-bit flip of the first 220 bytes
    (Huffman tree description with FSE-compressed or direct weights, stream sizes, sequence count, modes, the three FSE
    table descriptions, the start of the bitstreams) and of the last 16 of single-block frames of non-periodic text —
    libzstd's at two levels and this build's own higher-tier ones.  The tree is read and the tables are built by whole
    waves (huf_read_tree_wave, fse_build_wave): every verdict has to equal the one-lane oracle's."""
    bases = [(gen.pseudo_text(6000, 21), 19), (gen.pseudo_text(20000, 22), 3), (gen.pseudo_text(3000, 23), 19),
             (bytes(np.random.default_rng(24).integers(0, 256, 9000, dtype=np.uint8) // 3 * 3), 19)]
    _run(gpu_ctx, oracle, bases, 220, 9, 200, 1500, mutants=_all_bit_flips)


def test_mutant_table_is_decoded_the_same_every_time(gpu_ctx, oracle):
    """The exhaustive single-bit table (role-split kernel + its left-over list + general decoder in one run) ten times
    over: the digests, statuses and counters of every run equal the first one's.  (A wrong digest for one valid row in
    ~30 % of runs is how a race in the left-over path showed; a single run of the parity test above can miss it.)"""
    import torch
    from znippy_amd import hip
    bases = [(gen.text(10240), 19), (gen.text(10240), 1), (_periodic(200, 20480, 2), 19), (gen.binary(10240), 3)]
    rng = np.random.default_rng(5)
    frames, sizes, originals = [], [], []
    for data, lvl in bases:
        for base in (oracle.libzstd_compress(data, lvl), gpu_ctx.compress(data)):
            frames.append(base); sizes.append(len(data)); originals.append(data)
            for m in _all_bit_flips(base, rng, 400):
                frames.append(m); sizes.append(len(data)); originals.append(data)
    n = len(frames)
    bs = np.array([len(f) for f in frames], dtype=np.uint64)
    bo = np.concatenate([[0], np.cumsum(bs)[:-1]]).astype(np.uint64)
    us = np.array(sizes, dtype=np.uint64)
    oo = np.concatenate([[0], np.cumsum(us)[:-1]]).astype(np.uint64)
    ck = np.stack([np.frombuffer(oracle.blake3(d), dtype=np.uint8) for d in originals])
    d_blobs = torch.from_numpy(np.frombuffer(b"".join(frames) + bytes(64), dtype=np.uint8).copy()).cuda()
    d_out = torch.zeros(int(us.sum()) + 64, dtype=torch.uint8, device="cuda")
    rt = hip.RowTable(gpu_ctx, bo, bs, us, oo, None, ck)
    first = None
    for rep in range(10):
        counters, corrupt, status = rt.decode_verify(d_blobs, d_out)
        got = (dict(counters), sorted(int(x) for x in corrupt), status.copy(), rt.digests()[status >= 0].copy())
        if first is None:
            first = got
            assert n > 4000
        else:
            assert got[0] == first[0], (rep, got[0], first[0])
            assert got[1] == first[1], (rep, sorted(set(got[1]) ^ set(first[1]))[:8])
            assert (got[2] == first[2]).all() and (got[3] == first[3]).all(), rep
