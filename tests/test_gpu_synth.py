"""GPU parity: the hand-built RFC 8878 frames of tests/zstd_synth_cases.py on every foreign-frame read path.

The read side parses the format in several separately written places (the serial decoder, the two-phase path, the batch
path with lane = block and wave = block sequence decoders, the resolve path, the fused kernels' recognisers), and a row
reaches one of them by its size, the table around it and the context's switches.  Every other foreign frame of the suite
comes out of libzstd; these come out of a writer that is told what to write: tables dominated by "less than 1" symbols or
at the maximum accuracy log, blocks that open with rep0 - 1, Repeat_Mode across RLE blocks, non-minimal headers, 128 KiB
matches.  Expected bytes come from the reference executor (tests/zstd_synth.py), digests from the oracle's BLAKE3,
verdicts from the oracle (test_zstd_synth.py pins executor, oracle and libzstd against each other without a GPU).

A context is created under each switch set and runs (a) a table of all valid cases, (b) the valid cases shuffled among a few
hundred libzstd frames of real text plus every invalid case: a corner case must neither disturb the 63 other blocks of its
wave nor be disturbed by them.  The default context also runs every valid case through the single-frame ABI.  A context
without a serial decoder behind the parallel paths (ZNIPPY_FZ_ONLY) shows which cases those paths decline, and the test
carries that list; every context's statistics show which kernels ran on these frames, on how many of them, and that no
block was handed on to the serial decoder.

What the valid table notices was tried with three one-line changes to the kernels, one build each:
  - bx_fse_spread without its `pos >= high` step: the spread no longer ends at cell 0, so the batch path gives up 26
    blocks (every table with a "less than 1" symbol) to the serial decoder, which decodes them.  Caught by the
    blocks_given_up assertion in all seven contexts with the batch path, and by 15 more declined frames (mode_*_fse,
    mode_*repeat*, fse_*less_than_1*, fse_max_log_9_8_9) under ZNIPPY_FZ_ONLY; no_bx and no_bx+no_fz pass.
  - k_bx_fse with `o = r0` for `o = r0 + 1`: wrong bytes in rep_ll0_opens_* and rep_rep0_minus_1_chain_opens_* (next block,
    after a raw block, after a zero-sequence block; _fse_offsets), rep_minus_1_chain_opens_three_blocks_running_fse_offsets
    and rep_minus_1_chain_opens_block_above_128k, in the six contexts where the lane = block decoder runs; bx_big_1 (every
    block to the wave decoder), no_bx and no_bx+no_fz pass.  The rep_* cases without _fse_offsets pass it everywhere: with
    predefined tables and raw literals the fused kernels decode them and the batch path never sees them, which is why
    the _fse_offsets twins exist.
  - fz_lit_header with the 4-byte and 5-byte formats swapped: 13 blocks given up in the batch contexts and 3 in no_bx
    (lit_huf_4byte_and_5byte_formats_above_128k, the one such frame the two-phase path takes), 11 more declined frames
    under ZNIPPY_FZ_ONLY (lit_huf_4streams_[45]byte*, treeless_4streams_behind_fse_weights,
    len_128k_huffman_literals_zero_sequences, the frame above); no_bx+no_fz passes."""
import numpy as np
import pytest

import workloads
import zstd_synth_cases as K
from gpu_cases import decode_table, frame_table, make_ctx, py_corpus

pytestmark = pytest.mark.gpu

# (name, switches, frames of the valid table that the parallel parsers decode: the batch path, or the two-phase path where the
# batch path is off; RowTable.foreign_stats()["frames"]).  The valid table has 157 rows.  The others are decoded whole by the
# fused kernels (predefined or RLE tables over raw or RLE literals, up to 64 KiB) or by the serial decoder; of the default
# context's 59, the serial decoder has the 4 of DECLINED and the fused kernels 55.  no_block_items: one more frame, which the
# fused block kernel otherwise takes.
PATHS = [
    ("default", {}, 98),
    ("no_bx", {"ZNIPPY_NO_BX": "1"}, 14),
    ("no_bx+no_fz", {"ZNIPPY_NO_BX": "1", "ZNIPPY_NO_FZ": "1"}, 0),
    ("no_fz", {"ZNIPPY_NO_FZ": "1"}, 98),
    ("no_rx", {"ZNIPPY_NO_RX": "1"}, 98),
    ("bx_big_1", {"ZNIPPY_BX_BIG": "1"}, 98),
    ("bx_big_huge", {"ZNIPPY_BX_BIG": "1000000000"}, 98),
    ("no_block_items", {"ZNIPPY_NO_BLOCK_ITEMS": "1"}, 99),
    ("roles_min_1", {"ZNIPPY_ROLES_MIN": "1"}, 98),
]
BATCH_KERNELS = {"zstd_batch_scan", "zstd_batch_tables", "zstd_batch_huffman", "zstd_batch_sequences", "zstd_batch_sequences_long",
                 "zstd_batch_execute"}
TWO_PHASE_KERNELS = {"zstd_foreign_entropy", "zstd_foreign_execute"}
RESOLVE_KERNELS = {"zstd_resolve_plan", "zstd_resolve_jump", "zstd_resolve_expand", "zstd_resolve_store"}

# Valid cases the parallel paths leave to the serial decoder, each with the line that declines it.  With ZNIPPY_FZ_ONLY
# (no serial decoder behind them) exactly these come back as corrupt rows; every context with a serial decoder decodes
# them.  Value: (the line that declines it, blocks the batch path counts as given up for it).  All four are declined as
# whole frames, before any block is looked at, so none of them shows in blocks_given_up.
#
# None of the four is declined at one of the three places where the parallel parsers give up a block by design: an offset
# code above 27 (`ofb > 27`, k_bx_fse), more than 64 symbols in a lane's table scratch (`s >= 64`, bx_read_ncount) and a
# symbolic repeat offset that runs out of its field (`(o & 0x3FFFFFF) == 0x3FFFFFF`).  No valid case of the corpus reaches
# any of them: the largest offset code is 22, the widest description in a lane's scratch has 53 symbols (ML), and the
# longest run of rep0 - 1 is four.  They are covered by the fuzz tests alone.
_CHECKSUM = "zstd_batch.hip k_bx_scan: `!((fhd >> 2) & 1)` -- a checksum trailer is the serial decoder's"
DECLINED = {
    "hdr_checksum": (_CHECKSUM, 0),
    "hdr_checksum_window_multiblock": (_CHECKSUM, 0),
    "hdr_skippable_in_front": ("zstd_batch.hip k_bx_scan: the magic number is looked for at byte 0; the serial decoder steps "
                               "over skippable frames", 0),
    "extreme_codes_offset_code_22_above_4_mib": ("zstd_batch.hip fz_exec_frame / k_rx_plan: `fcs >= (1u << 20) && seqs * 2048 < "
                                                 "fcs` -- a few very long copies go to the serial decoder's wide variant", 0),
}
N_GIVEN_UP = sum(n for _, n in DECLINED.values())


@pytest.fixture(scope="module", params=PATHS, ids=[p[0] for p in PATHS])
def path(request):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    name, env, frames = request.param
    ctx = make_ctx(env)
    yield name, ctx, frames
    ctx.close()


def build_valid_table(oracle):
    """Every valid case that declares its content size (the row loop asks the frame for its size first)."""
    cases = [c for c in K.valid_cases() if not c.no_size]
    return cases, frame_table(oracle, [c.want for c in cases], [c.frame for c in cases])


@pytest.fixture(scope="module")
def valid_table(oracle):
    return build_valid_table(oracle)


def build_mixed_table(oracle):
    """(rows, table, the oracle's counters and corrupt list): rows are (kind, name, intended bytes, frame), kind one of
    "valid", "libzstd", "invalid"; a valid case without a content size counts as invalid here (the size query fails)."""
    data = py_corpus(4 << 20)
    rng = np.random.default_rng(77)
    rows, pos = [], 0
    for i in range(240):
        n = int(rng.integers(2048, 30 * 1024))
        e = data[pos:pos + n]
        pos += n
        rows.append(("libzstd", f"libzstd_{i}", e, workloads.libzstd_compress(e, 19 if i % 2 else 3)))
    rows += [("invalid" if c.no_size else "valid", c.name, c.want, c.frame) for c in K.valid_cases()]
    rows += [("invalid", c.name, c.want, c.frame) for c in K.invalid_cases()]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    A = frame_table(oracle, [r[2] for r in rows], [r[3] for r in rows])
    n = len(rows)
    want, want_corrupt = oracle.decompress_rows(A["blobs"], A["bo"], A["bs"], A["us"], A["oo"], np.full((n + 7) // 8, 255, np.uint8),
                                                A["ck"], 0, n)
    return rows, A, want, sorted(int(x) for x in want_corrupt)


@pytest.fixture(scope="module")
def mixed_table(oracle):
    return build_mixed_table(oracle)


def _row_bytes(A, out, i):
    return out[int(A["oo"][i]):int(A["oo"][i] + A["us"][i])].tobytes()


def _wrong_rows(names, wants, A, status, out, corrupt, digests):
    """Names of the rows that are not: status 0, not corrupt, the intended bytes, the oracle's digest."""
    bad = []
    for i, (name, want) in enumerate(zip(names, wants)):
        if status[i] != 0 or i in corrupt or _row_bytes(A, out, i) != want or not np.array_equal(digests[i], A["ck"][i]):
            bad.append((name, int(status[i]), i in corrupt))
    return bad


def _path_report(tag, st, kt):
    print(f"[synth] {tag}: frames={st['frames']} blocks_given_up={st['blocks_given_up']} "
          f"(error={st['given_up_error']} table_far={st['given_up_table_far']} pool={st['given_up_pool']} range={st['given_up_range']}) "
          f"kernels={sorted(k for k in kt if k.startswith(('zstd_', 'decode_verify')))}")


def test_valid_table(path, valid_table):
    """(a) all valid cases, nothing else: status 0 everywhere, no corrupt row, the executor's bytes, the oracle's digests;
    two runs agree (decode_table)."""
    name, ctx, frames = path
    cases, A = valid_table
    c, status, out, st, kt, corrupt, digests = decode_table(ctx, A, full=True)
    _path_report(f"{name} valid table", st, kt)
    bad = _wrong_rows([x.name for x in cases], [x.want for x in cases], A, status, out, set(corrupt), digests)
    assert not bad, bad
    total = int(A["us"].sum())
    assert c["total_chunks"] == len(cases) and c["decode_errors"] == 0 and c["corrupt_rows"] == 0 and c["verified_bytes"] == total, c
    # The parallel parsers decoded the frames they are meant to, and finished every block they began: a block they give
    # up goes to the serial decoder, which would decode it right and say nothing about them.
    assert st["frames"] == frames and st["blocks_given_up"] == N_GIVEN_UP, st
    ran = set(kt)
    if name.startswith("no_bx"):
        assert not (BATCH_KERNELS | RESOLVE_KERNELS) & ran, sorted(ran)
        assert (TWO_PHASE_KERNELS <= ran) if name == "no_bx" else not TWO_PHASE_KERNELS & ran, sorted(ran)
        assert "zstd_decode_general" in ran, sorted(ran)
    else:
        assert BATCH_KERNELS <= ran and not TWO_PHASE_KERNELS & ran, sorted(ran)
        assert (RESOLVE_KERNELS <= ran) if name != "no_rx" else not RESOLVE_KERNELS & ran, sorted(ran)


def test_mixed_table(path, mixed_table, oracle):
    """(b) the valid cases among libzstd frames and the invalid cases.  Valid and libzstd rows as in (a).  A row the oracle
    rejects has status < 0, or is on the corrupt list, or holds the intended bytes (the rule of gpu_cases.fuzz_run); a row
    the oracle accepts holds the oracle's bytes.  The counters are those of the oracle's read loop over the same columns."""
    name, ctx, _ = path
    rows, A, want, want_corrupt = mixed_table
    c, status, out, st, kt, corrupt, digests = decode_table(ctx, A, full=True)
    _path_report(f"{name} mixed table", st, kt)
    corrupt = set(corrupt)
    good = [i for i, r in enumerate(rows) if r[0] != "invalid"]
    bad = _wrong_rows([rows[i][1] for i in good], [rows[i][2] for i in good],
                      {k: (v[good] if k in ("oo", "us", "ck") else v) for k, v in A.items()}, status[good], out,
                      {good.index(i) for i in corrupt if i in good}, digests[good])
    assert not bad, bad
    wrong = []
    for i, (kind, rname, intended, frame) in enumerate(rows):
        if kind != "invalid":
            continue
        try:
            accepted = oracle.zstd_decompress(frame)
            oracle_ok = len(accepted) == len(intended)
        except ValueError:
            oracle_ok = False
        got = _row_bytes(A, out, i)
        if oracle_ok:
            if status[i] != 0 or got != accepted or (i in corrupt) != (accepted != intended):
                wrong.append((rname, int(status[i]), "differs from the oracle's bytes"))
        elif not (status[i] < 0 or i in corrupt or got == intended):
            wrong.append((rname, int(status[i]), "verified with wrong bytes"))
    assert not wrong, wrong
    assert c == want, (c, want, [(rows[i][1], int(status[i])) for i in range(len(rows)) if status[i] != 0],
                       [rows[i][1] for i in sorted(corrupt)], [rows[i][1] for i in want_corrupt])
    assert sorted(corrupt) == want_corrupt


def test_single_frame_abi(gpu_ctx, valid_table):
    """(c) znippy_decompress and the size query on every valid case that declares a content size."""
    from znippy_amd import hip
    cases, _ = valid_table
    bad = []
    for c in cases:
        if hip.get_decompressed_size(c.frame) != len(c.want) or gpu_ctx.decompress(c.frame) != c.want:
            bad.append(c.name)
    assert not bad, bad


def test_parallel_paths_decline_only_what_they_say(gpu_ctx_fz_only, gpu_ctx, valid_table):
    """No serial decoder behind the parallel paths: a frame they do not finish is a corrupt row.  Exactly the cases of
    DECLINED come back that way, every other row is right, and the default context decodes the declined ones."""
    cases, A = valid_table
    c, status, out, st, kt, corrupt, digests = decode_table(gpu_ctx_fz_only, A, full=True)
    _path_report("fz_only valid table", st, kt)
    bad = _wrong_rows([x.name for x in cases], [x.want for x in cases], A, status, out, set(corrupt), digests)
    assert sorted(b[0] for b in bad) == sorted(DECLINED), bad
    assert all(b[1] == 0 and b[2] for b in bad), bad             # declined = decoded to something else and flagged, not an error
    assert st["frames"] == PATHS[0][2] and st["blocks_given_up"] == N_GIVEN_UP, st
    idx = [i for i, x in enumerate(cases) if x.name in DECLINED]
    if idx:
        sub = [cases[i] for i in idx]
        B = {k: (v[idx] if k in ("us", "ck") else v) for k, v in A.items()}
        B["bo"], B["bs"] = A["bo"][idx], A["bs"][idx]
        B["oo"] = (np.cumsum(B["us"]) - B["us"]).astype(np.uint64)
        c2, status2, out2, st2, kt2, corrupt2, digests2 = decode_table(gpu_ctx, B, full=True)
        assert not _wrong_rows([x.name for x in sub], [x.want for x in sub], B, status2, out2, set(corrupt2), digests2)
