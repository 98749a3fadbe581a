"""The named corpus of hand-built frames (not a test module).  Every case is written by tests/zstd_synth.py from a
description; its expected bytes come from the reference executor there.  Deterministic: fixed seeds only.

    valid_cases()    -> [Case]: frames every decoder must decode to Case.want
    invalid_cases()  -> [Case]: one deliberate violation each; Case.want is what the frame was meant to say (the bytes a
                        decoder may at most produce), Case.why the rule that is broken

Case.promise says what the name promises about the bytes of the frame (checked by the writer's self-checks in
test_zstd_synth.py): keys are read by `test_frame_holds_what_its_name_promises` there.  Case.no_size marks a frame
without a content size: valid to a decoder that is told the size, a decode error to the row loop (the size query comes
first)."""
import functools

import numpy as np

import zstd_synth as Z
from zstd_synth import Comp, Raw, Rle


class Case:
    def __init__(self, name, blocks, want, frame, promise=None, why=None, no_size=False):
        self.name, self.blocks, self.want, self.frame = name, blocks, want, frame
        self.promise, self.why, self.no_size = promise or {}, why, no_size

    def __repr__(self):
        return self.name


def _text(n, seed, alpha=20):
    """n bytes over a small skewed alphabet (letters): literals a Huffman code is worth writing for."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, alpha + 1)
    return (rng.choice(alpha, size=n, p=p / p.sum()) + 97).astype(np.uint8).tobytes()


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def pack(items, first=None, **comp_kw):
    """[(literal bytes, match length, offset value)] -> compressed blocks of at most 128 KiB each (a trailing item with
    match length 0 is literals only).  comp_kw goes to every block."""
    blocks, lits, seqs, size = ([first] if first is not None else []), bytearray(), [], 0
    for lb, ml, ov in items:
        if size + len(lb) + ml > Z.BLOCK_MAX:
            blocks.append(Comp(lits, seqs, **comp_kw))
            lits, seqs, size = bytearray(), [], 0
        lits += lb
        size += len(lb) + ml
        if ml:
            seqs.append((len(lb), ml, ov))
    if size or not blocks:
        blocks.append(Comp(lits, seqs, **comp_kw))
    return blocks


# a first block that leaves the offset history at (30, 20, 12): three explicit offsets over 64 literal bytes
def _hist_block(seed=1, **kw):
    t = _text(64, seed)
    return Comp(t, [(40, 5, 12 + 3), (10, 6, 20 + 3), (14, 7, 30 + 3)], **kw)


REP_LL0 = [(0, 4, 1), (0, 5, 2), (0, 6, 3), (0, 4, 3), (0, 7, 1)]             # ll = 0: rep1, rep2, rep0-1, rep0-1, rep1
REP_LL1 = [(2, 4, 1), (1, 5, 2), (3, 6, 3), (1, 4, 1), (2, 5, 3), (1, 4, 2)]  # ll > 0: rep0, rep1, rep2, ...
REP_MINUS = [(0, 4, 3), (0, 5, 3), (0, 6, 3), (0, 7, 3), (1, 4, 1)]           # rep0-1 four times in a row, then rep0


def _rep_block(seqs, seed, **kw):
    return Comp(_text(sum(s[0] for s in seqs) + 5, seed), seqs, **kw)


def _match_items(offsets, lengths, seed):
    """One match per (offset, length), 1-3 fresh bytes in front of each, behind a 5000-byte opening."""
    items = [(_text(5000, seed, alpha=26), 0, 0)]
    k = 0
    for ml in lengths:
        for off in offsets:
            items.append((_noise(1 + k % 3, seed * 1000 + k), ml, off + 3))
            k += 1
    items[0] = (items[0][0], 3, 9 + 3)
    return items


LL_LOW = ("fse", [-1] * 20 + [6, 6], 5)     # 20 of 32 cells belong to "less than 1" symbols


@functools.lru_cache(maxsize=1)
def valid_cases():
    C = []

    def add(name, blocks, promise=None, no_size=False, **fkw):
        want = Z.execute(blocks)
        C.append(Case(name, blocks, want, Z.write_frame(blocks, content=want, **fkw), promise, no_size=no_size))

    small = lambda s=3: [Comp(_text(60, s), [(10, 5, 7 + 3), (3, 4, 1), (20, 9, 2)])]
    pad = lambda n: [Rle(0x41, n)] + small()

    # ---- frame header ------------------------------------------------------------------------------------------------
    add("hdr_single_fcs1", small(), dict(fhd=0x20))
    add("hdr_single_fcs2_at_256", pad(256 - 78), dict(fhd=0x60, fcs_raw=0))
    add("hdr_single_fcs2", pad(1000), dict(fhd=0x60))
    add("hdr_single_fcs4_wide", small(), dict(fhd=0xA0), fcs_bytes=4)
    add("hdr_single_fcs8_wide", small(), dict(fhd=0xE0), fcs_bytes=8)
    add("hdr_window_no_size", small(), dict(fhd=0x00), single=False, window_log=10, no_size=True)
    add("hdr_window_fcs2", pad(1000), dict(fhd=0x40), single=False, window_log=11, fcs_bytes=2)
    add("hdr_window_fcs4", small(), dict(fhd=0x80), single=False, window_log=17, fcs_bytes=4)
    add("hdr_window_fcs8", small(), dict(fhd=0xC0), single=False, window_log=23, fcs_bytes=8)
    for nb in (1, 2, 4):
        add(f"hdr_dict_id_zero_{nb}byte", small(), dict(fhd=0x20 | {1: 1, 2: 2, 4: 3}[nb]), did=(nb, 0))
    add("hdr_checksum", small(), dict(fhd=0x24), checksum=True)
    add("hdr_checksum_window_multiblock", [_hist_block(), Raw(_noise(40, 2)), _rep_block(REP_LL1, 3)], dict(fhd=0x84),
        checksum=True, single=False, window_log=10, fcs_bytes=4)
    add("hdr_skippable_in_front", small(), dict(skippable=2), skippable=[b"hello world", b""])

    # ---- blocks ------------------------------------------------------------------------------------------------------
    add("blk_raw_only", [Raw(_noise(100, 1))], dict(types=[0]))
    add("blk_rle_only", [Rle(7, 1000)], dict(types=[1]))
    add("blk_empty_frame", [Raw(b"")], dict(types=[0]))
    add("blk_empty_last_raw_behind_predefined", small(), dict(types=[2, 0], modes={0: 0}), empty_last=True)
    add("blk_raw_128k", [Raw(_noise(Z.BLOCK_MAX, 2))], dict(types=[0], sizes=[Z.BLOCK_MAX]))
    add("blk_rle_128k_then_compressed", [Rle(9, Z.BLOCK_MAX)] + small(), dict(types=[1, 2], sizes={0: Z.BLOCK_MAX}))
    add("blk_raw_rle_compressed_mix",
        [Raw(_text(50, 1)), Rle(66, 300), _hist_block(), Rle(67, 1), Raw(b""), _rep_block(REP_LL0, 5)],
        dict(types=[0, 1, 2, 1, 0, 2]))

    # frames of ceil(size / 128 KiB) blocks whose first block is in the plain style (predefined tables): what the read
    # side's block scan takes for a frame whose blocks stand alone at multiples of 128 KiB
    full = Comp(_text(64, 9), [(64, Z.BLOCK_MAX - 64, 7 + 3)])
    add("blk_looks_standalone_uneven_split", small() + [Comp(b"", [(0, Z.BLOCK_MAX, 5 + 3)])], dict(types=[2, 2]))
    add("blk_looks_standalone_second_reaches_back", [full, Comp(_text(30, 8), [(10, 50, 100 + 3), (5, 9, 1)])],
        dict(types=[2, 2]))
    add("blk_looks_standalone_second_opens_with_repeat", [full, Comp(_text(30, 8), [(10, 50, 1), (5, 9, 8 + 3)])],
        dict(types=[2, 2]))
    add("blk_looks_standalone_and_is", [full, Comp(_text(30, 8), [(10, 50, 4 + 3), (5, 9, 1)]), ], dict(types=[2, 2]))

    # ---- raw and RLE literals in every header form -------------------------------------------------------------------
    for typ in ("raw", "rle"):
        for fmt, n, tag in ((0, 20, "1byte"), (2, 31, "1byte_alt"), (1, 700, "2byte"), (1, 5, "2byte_wide"),
                            (3, 5000, "3byte"), (3, 6, "3byte_wide")):
            lits = _text(n, n) if typ == "raw" else b"q" * n
            seqs = [(2, 4, 2 + 3), (1, 3, 1)] if n >= 5 else []
            add(f"lit_{typ}_{tag}", [Comp(lits, seqs, lit=dict(type=typ, fmt=fmt))],
                dict(lit={0: (0 if typ == "raw" else 1, fmt, n)}))

    # ---- Huffman literals --------------------------------------------------------------------------------------------
    for wdesc in ("direct", "fse"):
        for fmt, n, tag in ((0, 300, "1stream"), (1, 900, "4streams_3byte"), (2, 900, "4streams_4byte_wide"),
            (2, 9000, "4streams_4byte"),
                            (3, 900, "4streams_5byte_wide"), (3, 20000, "4streams_5byte")):
            add(f"lit_huf_{tag}_{wdesc}", [Comp(_text(n, n + 1), [(50, 8, 33 + 3), (0, 5, 2), (100, 40, 1)],
                                               lit=dict(type="huf", fmt=fmt, wdesc=wdesc))],
                dict(lit={0: (2, fmt, n)}, tree={0: wdesc}))
    abc = bytes(np.random.default_rng(5).integers(0, 3, 200, dtype=np.uint8) + 120)
    add("lit_huf_1stream_3_symbols", [Comp(abc, [(100, 30, 50 + 3)], lit=dict(type="huf", fmt=0))],
        dict(lit={0: (2, 0, 200)}, nweights={0: 122}))

    # the 4-byte and the 5-byte format in a frame of two blocks by its size (above 128 KiB): the two-phase path reads
    # these headers only in such frames, the batch path in every frame
    add("lit_huf_4byte_and_5byte_formats_above_128k",
        [Comp(_text(9000, 77), [(9000, Z.BLOCK_MAX - 9000, 7 + 3)], lit=dict(type="huf", fmt=2)),
         Comp(_text(20000, 78), [(50, 8, 33 + 3), (0, 5, 2), (100, 40, 1)], lit=dict(type="huf", fmt=3)),
         Comp(_text(900, 79), [(50, 8, 33 + 3)], lit=dict(type="treeless", fmt=2))],
        dict(types=[2, 2, 2], lit={0: (2, 2, 9000), 1: (2, 3, 20000), 2: (3, 2, 900)}))

    def with_weights(name, weights, n, seed, wdesc="direct", fmt=0, promise=None):
        syms = [s for s, w in enumerate(weights) if w]
        p = np.array([float(1 << weights[s]) for s in syms])
        rng = np.random.default_rng(seed)
        lits = bytes(syms) + np.array(syms, np.uint8)[rng.choice(len(syms), size=n - len(syms),
            p=p / p.sum())].tobytes()
        add(name, [Comp(lits, [(n // 2, 9, 40 + 3), (5, 4, 1)], lit=dict(type="huf", fmt=fmt, weights=weights,
            wdesc=wdesc))],
            dict(tree={0: wdesc}, **(promise or {})))

    with_weights("huf_max_code_length_11_last_weight_largest", [1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], 600, 1,
        promise=dict(huf_bits={0: 11}, last_weight={0: 11}))
    with_weights("huf_max_code_length_11_fse_weights", [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1], 600, 2, "fse",
        promise=dict(huf_bits={0: 11}, last_weight={0: 1}))
    with_weights("huf_max_code_length_11_4streams", [0, 0, 11, 10, 9, 8, 7, 6, 5, 4, 0, 3, 2, 1, 0, 0, 1], 1000, 3,
        fmt=1, promise=dict(huf_bits={0: 11}))
    with_weights("huf_two_symbols", [1, 1], 100, 4, promise=dict(nweights={0: 1}, huf_bits={0: 1}))
    with_weights("huf_two_symbols_far_apart", [1] + [0] * 99 + [1], 100, 5,
        promise=dict(nweights={0: 100}, huf_bits={0: 1}))
    with_weights("huf_zero_weights_in_the_middle", [2, 0, 0, 1, 0, 0, 0, 1], 200, 6, promise=dict(nweights={0: 7}))
    with_weights("huf_symbol_255_fse_weights", [1] + [0] * 254 + [1], 150, 7, "fse", promise=dict(nweights={0: 255}))
    with_weights("huf_128_direct_weights", [1] * 128 + [8], 800, 9, promise=dict(nweights={0: 128}, last_weight={0: 8}))
    with_weights("huf_127_direct_weights_4streams", [1] * 64 + [0] * 62 + [7, 8], 800, 10, fmt=1,
        promise=dict(nweights={0: 127}))

    # ---- treeless literals -------------------------------------------------------------------------------------------
    hb = lambda seed, n=300, **k: Comp(_text(n, seed, alpha=8), [(50, 8, 33 + 3), (0, 5, 2)], lit=dict(type="huf", **k))
    tl = lambda seed, n=200, fmt=0, **k: Comp(_text(n, seed, alpha=8), [(20, 8, 1), (3, 5, 2)],
        lit=dict(type="treeless", fmt=fmt), **k)
    add("treeless_next_block", [hb(1), tl(2)], dict(lit={1: (3, 0, 200)}))
    add("treeless_4streams_behind_fse_weights", [hb(3, wdesc="fse"), tl(4, n=1000, fmt=1), tl(5, n=1000, fmt=2)],
        dict(lit={1: (3, 1, 1000), 2: (3, 2, 1000)}))
    add("treeless_across_raw_literal_block", [hb(6), Comp(_noise(40, 1), [(10, 4, 1)]), tl(7)],
        dict(lit={1: (0, 1, 40), 2: (3, 0, 200)}))
    add("treeless_across_rle_literal_block", [hb(6), Comp(b"z" * 40, [(10, 4, 1)], lit=dict(type="rle")), tl(7)],
        dict(lit={2: (3, 0, 200)}))
    add("treeless_across_raw_block", [hb(8), Raw(_noise(33, 3)), tl(9)], dict(types=[2, 0, 2], lit={2: (3, 0, 200)}))
    add("treeless_across_rle_block", [hb(10), Rle(1, 77), tl(11)], dict(types=[2, 1, 2], lit={2: (3, 0, 200)}))
    add("treeless_and_repeat_tables_behind_raw_block",
        [Comp(_text(300, 12, alpha=8), [(50, 8, 33 + 3), (0, 5, 2), (9, 4, 12 + 3)], lit=dict(type="huf"),
            ll=("fse", Z.spread_norm([0, 3, 9, 18, 24], 5), 5),
              of=("fse", Z.spread_norm([0, 1, 3, 5], 5), 5), ml=("fse", Z.spread_norm([1, 2, 5], 5), 5)),
                  Raw(_noise(20, 4)), tl(13, ll="rep", of="rep", ml="rep")],
        dict(types=[2, 0, 2], lit={2: (3, 0, 200)}, modes={0: 0xA8, 2: 0xFC}))
    add("treeless_zero_sequences", [hb(14), Comp(_text(100, 15, alpha=8), [], lit=dict(type="treeless"))],
        dict(lit={1: (3, 0, 100)}, nseq={1: (1, 0)}))

    # ---- sequence count forms ----------------------------------------------------------------------------------------
    for typ in ("raw", "rle", "huf"):
        add(f"seq_count_zero_{typ}_literals", [Comp(b"w" * 90 if typ == "rle" else _text(90, 4), [],
            lit=dict(type=typ))], dict(nseq={0: (1, 0)}))
    add("seq_count_1byte_127", pack([(_text(2, i), 3, 1 + 3 + i % 5) for i in range(127)]), dict(nseq={0: (1, 127)}))
    add("seq_count_2byte_128", pack([(_text(2, i), 3, 1 + 3 + i % 5) for i in range(128)]), dict(nseq={0: (2, 128)}))
    add("seq_count_2byte_non_minimal_5", [Comp(_text(30, 1), [(3, 4, 1 + 3), (2, 3, 1), (1, 5, 2), (4, 3, 9 + 3),
        (0, 4, 1)], nseq_form=2)], dict(nseq={0: (2, 5)}))
    add("seq_count_2byte_0x7eff", pack([(b"ab"[i & 1:][:1] if i % 3 == 0 else b"", 3,
        4 + i % 7) for i in range(0x7EFF)], first=Raw(_text(16, 2))), dict(nseq={1: (2, 0x7EFF)}))
    add("seq_count_3byte_exactly_0x7f00", pack([(b"", 3, 4 + i % 11) for i in range(0x7F00)],
        first=Raw(_text(16, 3))), dict(nseq={1: (3, 0x7F00)}))
    add("seq_count_3byte_above_0x7f00_3byte_matches",
        pack([(b"x" if i % 64 == 0 else b"", 3, 4 + (i * 7) % 13) for i in range(0x7F00 + 1500)],
        first=Raw(_text(16, 4))),
        dict(nseq={1: (3, 0x7F00 + 1500)}))
    add("seq_count_3byte_fse_tables",
        pack([(b"x" if i % 5 == 0 else b"", 3 + (i % 3 == 0), 4 + (i * 7) % 13) for i in range(0x7F00 + 77)],
             first=Raw(_text(16, 5)), ll=("fse", [24, 8], 5), of=("fse", Z.spread_norm([2, 3, 4], 6), 6),
             ml=("fse", [20, 6, 6], 5)),
        dict(nseq={1: (3, 0x7F00 + 77)}, modes={1: 0xA8}))

    # ---- table modes: each of LL, OF, ML in each mode, the other two predefined --------------------------------------
    same = [(4, 5, 4 + 3)] * 6                        # one code each: what RLE mode can say
    T = _text(64, 21)
    fse_for = {"ll": ("fse", Z.spread_norm([4], 5, low=[0, 9]), 5), "of": ("fse", Z.spread_norm([2], 5, low=[0, 1]),
        5), "ml": ("fse", Z.spread_norm([2], 5, low=[7]), 5)}
    shift = {"ll": 6, "of": 4, "ml": 2}
    for kind in ("ll", "of", "ml"):
        add(f"mode_{kind}_rle", [Comp(T, same, **{kind: "rle"})], dict(modes={0: 1 << shift[kind]}))
        add(f"mode_{kind}_fse", [Comp(T, same, **{kind: fse_for[kind]})], dict(modes={0: 2 << shift[kind]}))
        for first, tag in (("pre", "predefined"), ("rle", "rle"), (fse_for[kind], "fse")):
            add(f"mode_{kind}_repeat_of_{tag}", [Comp(T, same, **{kind: first}),
                Comp(T, same, **{kind: "rep"})], dict(modes={1: 3 << shift[kind]}))
    add("mode_all_rle", [Comp(T, same, ll="rle", of="rle", ml="rle")], dict(modes={0: 0x54}))
    add("mode_all_fse_then_all_repeat", [Comp(T, same, **fse_for), Comp(T, same, ll="rep", of="rep", ml="rep")],
        dict(modes={0: 0xA8, 1: 0xFC}))
    add("mode_all_predefined_then_all_repeat", [Comp(T, same), Comp(T, same, ll="rep", of="rep", ml="rep")],
        dict(modes={0: 0, 1: 0xFC}))
    add("mode_mixed_fse_rle_pre_then_rep_rep_fse", [Comp(T, same, ll=fse_for["ll"], of="rle"),
        Comp(T, same, ll="rep", of="rep", ml=fse_for["ml"])], dict(modes={0: 0x90, 1: 0xF8}))
    for mid, tag in ((Comp(_text(30, 2), []), "zero_sequence_block"), (Rle(5, 40), "rle_block"),
                     (Raw(_noise(40, 6)), "raw_block")):
        add(f"mode_repeat_across_{tag}",
            [Comp(T, same, ll=LL_LOW, of="rle", ml=("fse", Z.spread_norm([1, 2, 3], 5), 5)), mid,
             Comp(T, REP_LL1, ll="rep", of=("fse", Z.spread_norm([0, 1], 5), 5), ml="rep"), mid,
             Comp(T, same, ll="rep", of="rle", ml="rep")],
            dict(modes={0: 0x98, 2: 0xEC, 4: 0xDC}))
    add("mode_repeat_of_rle_across_rle_block", [Comp(T, same, ll="rle", of="rle", ml="rle"), Rle(0, 9),
        Comp(T, same, ll="rep", of="rep", ml="rep")], dict(modes={2: 0xFC}))

    # ---- shapes of FSE table descriptions ----------------------------------------------------------------------------
    varied = [(24, 3, 5), (28, 9, 30 + 3), (0, 60, 1), (24, 3, 2), (28, 9, 3),
        (0, 60, 40 + 3)]      # LL codes 20, 21, 0; ML 0, 6, 39; OF 0..5
    V = _text(200, 31)
    add("fse_ll_dominated_by_less_than_1", [Comp(V, [(24, 5, 7), (28, 6, 1), (24, 7, 1)], ll=LL_LOW)],
        dict(fse={0: {"ll": (5, 20)}}))
    add("fse_all_three_dominated_by_less_than_1",
        [Comp(V, varied, ll=("fse", [-1] * 20 + [6, 6], 5), of=("fse", [-1] * 6 + [0] * 3 + [-1] * 20 + [6], 5),
              ml=("fse", [-1] * 39 + [15] + [-1] * 10, 6))],
        dict(fse={0: {"ll": (5, 20), "of": (5, 26), "ml": (6, 49)}}))
    add("fse_min_log_5", [Comp(V, varied, ll=("fse", Z.spread_norm([0, 20, 21], 5), 5),
        of=("fse", Z.spread_norm(range(6), 5), 5), ml=("fse", Z.spread_norm([0, 6, 39], 5), 5))],
        dict(fse={0: {"ll": (5, 0), "of": (5, 0), "ml": (5, 0)}}))
    add("fse_max_log_9_8_9", [Comp(V, varied, ll=("fse", Z.spread_norm([0, 20, 21], 9, low=[35]), 9),
        of=("fse", Z.spread_norm(range(6), 8, low=[28, 31]), 8),
                                   ml=("fse", Z.spread_norm([0, 6, 39], 9, low=[52]),
                                       9))], dict(fse={0: {"ll": (9, 1), "of": (8, 2), "ml": (9, 1)}}))
    add("fse_max_log_every_symbol", [Comp(V, varied, ll=("fse", Z.spread_norm(range(36), 9), 9),
        of=("fse", Z.spread_norm(range(32), 8), 8), ml=("fse", Z.spread_norm(range(53), 9), 9))],
        dict(fse={0: {"ll": (9, 0), "of": (8, 0), "ml": (9, 0)}}))
    add("fse_one_symbol_holds_almost_all", [Comp(V, varied, ll=("fse", [509] + [0] * 19 + [1, 2], 9),
        of=("fse", [251, 1, 1, 1, 1, 1], 8), ml=("fse", [1] + [0] * 5 + [1] + [0] * 32 + [510], 9))],
        dict(fse={0: {"ll": (9, 0), "of": (8, 0), "ml": (9, 0)}}))
    add("fse_long_zero_runs", [Comp(V, [(24, 3, 4), (0, 300, 4), (41, 3, 4)],
        ll=("fse", [16] + [0] * 19 + [8, 0, 0, 8], 5), of=("fse", [0, 0, 16] + [0] * 19 + [16], 5),
                                    ml=("fse", [16] + [0] * 43 + [16], 5))], dict(zero_runs={0: {"of": 6, "ml": 14}}))
    add("fse_less_than_1_at_high_logs_many_sequences",
        pack([(_text(i % 4, i), 3 + i % 40, 4 + (i * 5) % 60) for i in range(3000)], first=Raw(_text(64, 6)),
             ll=("fse", Z.spread_norm(range(4), 7, low=range(4, 36)), 7),
             of=("fse", Z.spread_norm(range(2, 6), 6, low=[0, 1] + list(range(6, 32))), 6),
             ml=("fse", Z.spread_norm(range(33), 8, low=range(33, 53)), 8)),
        dict(fse={1: {"ll": (7, 32), "of": (6, 28), "ml": (8, 20)}}))

    # ---- repeat offsets ----------------------------------------------------------------------------------------------
    add("rep_first_block_from_1_4_8", [Comp(_text(60, 41), [(9, 4, 1), (2, 5, 2), (3, 6, 3), (0, 4, 1), (0, 5, 2),
        (1, 4, 3), (0, 4, 3), (0, 6, 2)])])
    add("rep_first_block_rep0_minus_1_chain", [Comp(_text(60, 42), [(9, 4, 3), (0, 4, 3), (0, 5, 3), (0, 6, 3),
        (0, 7, 3), (2, 4, 1)])])
    mids = ((None, "next_block"), (Raw(_noise(50, 7)), "after_raw_block"), (Rle(3, 50), "after_rle_block"),
            (Comp(_text(50, 8), []), "after_zero_sequence_block"))
    openings = ((REP_LL0, "ll0"), (REP_LL1, "ll_positive"), (REP_MINUS, "rep0_minus_1_chain"))
    for mid, tag in mids:
        for seqs, what in openings:
            add(f"rep_{what}_opens_{tag}", [_hist_block()] + ([mid] if mid else []) + [_rep_block(seqs, 43)])
    add("rep_minus_1_chain_opens_three_blocks_running",
        [_hist_block()] + [_rep_block(REP_MINUS, 44 + i) for i in range(3)])
    add("rep_chain_many_small_blocks", [_hist_block()] + [x for i in range(40) for x in (_rep_block((REP_LL0,
        REP_LL1, REP_MINUS)[i % 3][:2 + i % 3] + ([(3, 4, 25 + i + 3)] if i % 3 == 2 else []), 50 + i),
        ) + ((Rle(i, 3),) if i % 4 == 0 else ())])
    # The same openings with one FSE-compressed table in the opening block.  A frame of predefined or RLE tables over
    # raw or RLE literals is decoded whole by the fused kernels' own recogniser; a compressed table sends it to the
    # parallel parsers, where the opening repeat codes are carried as "incoming entry k minus d" (k_bx_fse,
    # fz_wave_sequences).
    of_rep = ("fse", Z.spread_norm([0, 1], 5), 5)      # offset codes 0 and 1: every repeat code
    for mid, tag in mids:
        for seqs, what in openings:
            add(f"rep_{what}_opens_{tag}_fse_offsets",
                [_hist_block()] + ([mid] if mid else []) + [_rep_block(seqs, 43, of=of_rep)],
                dict(modes={(2 if mid else 1): 0x20}))
    add("rep_minus_1_chain_opens_three_blocks_running_fse_offsets",
        [_hist_block(), _rep_block(REP_MINUS, 44, of=of_rep)] + [_rep_block(REP_MINUS, 45 + i,
            of="rep") for i in range(2)],
        dict(modes={1: 0x20, 2: 0x30, 3: 0x30}))
    # ... and in a frame of two blocks by its size (above 128 KiB), which the two-phase path takes when the batch path
    # is off
    add("rep_minus_1_chain_opens_block_above_128k", [full, _rep_block(REP_MINUS, 46)], dict(types=[2, 2]))
    add("rep_minus_1_down_to_1",
        [Comp(_text(40, 45), [(20, 4, 5 + 3), (0, 4, 3), (0, 4, 3), (0, 4, 3), (0, 4, 3), (3, 4, 1)])])

    # ---- extra-bit extremes and long lengths -------------------------------------------------------------------------
    seed4k = Raw(_noise(4096, 9))
    add("len_one_sequence_longest_match", [seed4k, Comp(b"", [(0, Z.BLOCK_MAX, 1000 + 3)])], dict(nseq={1: (1, 1)}))
    add("len_128k_rle_literals_zero_sequences", [Comp(b"L" * Z.BLOCK_MAX, [], lit=dict(type="rle"))],
        dict(lit={0: (1, 3, Z.BLOCK_MAX)}, nseq={0: (1, 0)}))
    bits = np.random.default_rng(3).integers(0, 4, Z.BLOCK_MAX, dtype=np.uint8)
    add("len_128k_huffman_literals_zero_sequences", [Comp(bytes(bits + 48), [], lit=dict(type="huf", fmt=3))],
        dict(lit={0: (2, 3, Z.BLOCK_MAX)}, nseq={0: (1, 0)}))
    add("len_ll_code_35", [seed4k, Comp(b"r" * 65600, [(65536 + 60, 40000, 4000 + 3), (0, 3, 1)],
        lit=dict(type="rle"))], dict(max_codes={1: dict(ll=35)}))
    long_blocks = [seed4k] + [Comp(b"", [(0, Z.BLOCK_MAX, 4096 - 17 * i + 3)]) for i in range(2)]
    add("extreme_codes_few_hundred_kib", long_blocks + [Comp(b"t" * 65536, [(65536, 65536, 262144 + 2000 + 3)],
        lit=dict(type="rle")), Comp(b"", [(0, 65539 + 65533, 262144 + 70000 + 3)])],
        dict(max_codes={3: dict(ll=35, of=18), 4: dict(ml=52, of=18)}))
    big = [seed4k] + [Comp(b"", [(0, Z.BLOCK_MAX, 4096 - 3 * i + 3)] if i % 5 else [(0, Z.BLOCK_MAX - 10,
        4096 - 100 - i + 3), (0, 10, 1)]) for i in range(34)]
    big += [Comp(b"u" * 65536, [(65536, 65536, (1 << 22) + 9999 + 3)], lit=dict(type="rle")),
        Comp(b"", [(0, 65539 + 65533, (1 << 22) + 123456)]), Comp(_text(100, 1),
        [(50, 1000, 4400000 + 3), (0, 5000, 2)])]
    add("extreme_codes_offset_code_22_above_4_mib", big, dict(max_codes={35: dict(ll=35, of=22),
        36: dict(ml=52, of=22)}), fcs_bytes=8)

    # ---- matches: short periods, thresholds of the copy loops, on frames of each executor's size ---------------------
    offs = [1, 2, 3, 7, 8, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097]
    add("match_matrix_under_64k_one_block", pack(_match_items(offs, [3, 4, 15, 16, 17, 63, 64, 65, 255, 256], 1)))
    add("match_matrix_under_64k_several_blocks",
        [b for ch in range(4) for b in pack(_match_items(offs[:11] if ch else offs, [15 + ch, 64 - ch, 65 + ch],
        2 + ch))])
    add("match_matrix_resolve_small_table", pack(_match_items(offs, [16, 64, 8191, 8192], 6)))
    add("match_matrix_above_256k", pack(_match_items(offs, [17, 63, 8191, 8192, 8193, 16383], 7)))
    add("match_matrix_long_periods_above_256k", pack(_match_items([1, 2, 3, 7, 8, 15, 16, 17, 4096, 4097],
        [16384, 16385, 40000], 8)))
    add("match_exactly_65537_bytes", [Raw(_text(1537, 3))] + pack([(b"ab", 15998, 1 + 3 + i) for i in range(4)]))
    add("match_exactly_262144_bytes", [Raw(_text(2144, 4))] + pack([(b"", 65000, 17 + 3 + i) for i in range(4)]))
    add("match_from_previous_block_into_own_literals", [Raw(_text(100, 5)),
        Comp(_text(40, 6), [(10, 30, 15 + 3), (5, 60, 2), (10, 90, 40 + 3)])])
    add("match_overlap_across_block_boundary", [Comp(_text(40, 7), [(30, 5, 9 + 3)]),
        Comp(b"", [(0, 500, 3 + 3), (0, 70, 1 + 3)]), Rle(8, 5), Comp(b"k", [(0, 300, 2 + 3), (1, 65, 7 + 3)]),
        Raw(b"xy"),
                                                Comp(b"", [(0, 20000, 1 + 3), (0, 9000, 16 + 3)])])
    add("match_overlap_across_block_boundary_above_64k", [Raw(_text(17, 8))] + [Comp(b"",
        [(0, 30000 + i, (1, 2, 3, 7, 8, 15, 16, 17)[i] + 3)]) for i in range(8)])
    add("match_overlap_across_block_boundary_above_256k", [Raw(_text(17, 9))] + [Comp(b"",
        [(0, 100000 + i, (1, 2, 3, 7, 8, 15, 16, 17)[i % 8] + 3)]) for i in range(3)])
    return C


@functools.lru_cache(maxsize=1)
def invalid_cases():
    C = []

    def add(name, blocks, want, why, **fkw):
        C.append(Case(name, blocks, want, Z.write_frame(blocks, content=want, **fkw), why=why))

    T = _text(64, 71)
    ok = [Comp(T, [(10, 5, 7 + 3), (3, 4, 1), (20, 9, 2)])]
    okw = Z.execute(ok)
    add("inv_offset_zero_from_rep0_minus_1", [Comp(T, [(5, 4, 1 + 3), (0, 4, 3)])],
        Z.execute([Comp(T, [(5, 4, 1 + 3), (0, 4, 1 + 3)])]), "3.1.1.5: rep0 - 1 = 0 is not a distance")
    add("inv_offset_beyond_frame_start_first_block", [Comp(T, [(5, 4, 6 + 3)])], bytes(68),
        "a distance of 6 behind 5 bytes")
    add("inv_offset_beyond_frame_start_later_block", ok + [Raw(b"abc"), Comp(T, [(5, 4, len(okw) + 9 + 3)])],
        bytes(len(okw) + 3 + 68), "a distance past the frame's first byte")
    add("inv_offset_code_31", [Comp(T, [(5, 4, (1 << 31) + 12345)])], bytes(68),
        "a distance of 2 GiB in a frame of 68 bytes")
    add("inv_treeless_first_block", [Comp(T, [(5, 4, 1 + 3)],
        lit=dict(type="treeless", tree=Z.HufTree(Z.huf_weights(T))))], Z.execute([Comp(T, [(5, 4, 1 + 3)])]),
        "treeless literals with no tree before them")
    for kind in ("ll", "of", "ml"):
        add(f"inv_repeat_mode_first_block_{kind}", [Comp(T, [(10, 5, 7 + 3)], **{kind: "rep-of-nothing"})],
            Z.execute([Comp(T, [(10, 5, 7 + 3)])]), "Repeat_Mode with no table before it")
    add("inv_repeat_mode_behind_zero_sequence_block_only",
        [Comp(T, []), Comp(T, [(10, 5, 7 + 3)], ll="rep-of-nothing")], T + Z.execute([Comp(T, [(10, 5, 7 + 3)])]),
        "Repeat_Mode with no table before it")
    hw = dict(type="huf", check=False)
    lit4 = bytes([0, 1, 2, 3] * 10)
    add("inv_weights_not_a_power_of_two", [Comp(lit4, [], lit=dict(weights=[2, 1, 1, 1, 1], **hw))], lit4,
        "4.2.1: weights 2,1,1,1 sum to 5, no last weight completes them")
    l12 = bytes(range(13)) * 3
    add("inv_code_length_12", [Comp(l12, [], lit=dict(weights=[1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], **hw))],
        l12, "4.2.1: Max_Number_of_Bits is 11")
    short = [1] * 35 + [28]        # 36 symbols, one cell short of 64
    add("inv_counts_below_table_size", [Comp(T, [(10, 5, 7 + 3)], ll=("fse", short, 6, False))],
        Z.execute([Comp(T, [(10, 5, 7 + 3)])]), "4.1.1: the counts of all 36 symbols sum to 63 of 64")
    add("inv_accuracy_log_above_max_ll", [Comp(T, [(10, 5, 7 + 3)], ll=("fse", Z.spread_norm([10, 3], 10), 10))],
        Z.execute([Comp(T, [(10, 5, 7 + 3)])]), "LL accuracy log 10 > 9")
    add("inv_accuracy_log_above_max_of", [Comp(T, [(10, 5, 7 + 3)], of=("fse", Z.spread_norm([3, 1], 9), 9))],
        Z.execute([Comp(T, [(10, 5, 7 + 3)])]), "OF accuracy log 9 > 8")
    add("inv_accuracy_log_above_max_ml", [Comp(T, [(10, 5, 7 + 3)], ml=("fse", Z.spread_norm([2, 1], 10), 10))],
        Z.execute([Comp(T, [(10, 5, 7 + 3)])]), "ML accuracy log 10 > 9")
    for kind, sym in (("ll", 36), ("ml", 53), ("of", 32)):
        add(f"inv_symbol_above_alphabet_{kind}_{sym}", [Comp(T, [(10, 5, 7 + 3)], **{kind: ("rle", sym)})],
            Z.execute([Comp(T, [(10, 5, 7 + 3)])]), f"{kind.upper()} code {sym} does not exist")
    add("inv_ll_symbol_36_in_table_description",
        [Comp(T, [(10, 5, 7 + 3)], ll=("fse", [16] + [0] * 9 + [8] + [0] * 25 + [8], 5))],
        Z.execute([Comp(T, [(10, 5, 7 + 3)])]), "a count for LL symbol 36")
    add("inv_bitstream_bits_left_over", [Comp(T, [(10, 5, 7 + 3), (3, 4, 1)], pad_bits=3)],
        Z.execute([Comp(T, [(10, 5, 7 + 3), (3, 4, 1)])]), "3 bits left when the last sequence is decoded")
    add("inv_bitstream_a_byte_left_over", [Comp(T, [(10, 5, 7 + 3), (3, 4, 1)], pad_bits=8)],
        Z.execute([Comp(T, [(10, 5, 7 + 3), (3, 4, 1)])]), "8 bits left when the last sequence is decoded")
    add("inv_bitstream_runs_out", [Comp(T, [(10, 5, 7 + 3), (3, 40, 100 + 3 - 90)], drop_bits=5)],
        Z.execute([Comp(T, [(10, 5, 7 + 3), (3, 40, 13)])]), "the last fields want 5 bits more than there are")
    add("inv_literal_lengths_beyond_literals", [Comp(T[:20], [(10, 5, 7 + 3), (15, 4, 1)])], bytes(20 + 9),
        "literal lengths 10 + 15 over 20 literals")
    over = [Raw(T), Comp(b"y" * 10, [(10, Z.BLOCK_MAX - 2, 1 + 3)], lit=dict(type="rle"))]
    add("inv_block_regenerates_more_than_128k", over, T + b"y" * (Z.BLOCK_MAX + 8),
        "3.1.1.2.4: a block of 131080 bytes")
    add("inv_content_size_smaller", ok, okw, "the header declares one byte less than the blocks hold",
        fcs_value=len(okw) - 1)
    add("inv_content_size_larger", ok, okw, "the header declares one byte more than the blocks hold",
        fcs_value=len(okw) + 1)
    add("inv_wrong_checksum", ok, okw, "the checksum's lowest bit is flipped", checksum=True, bad_checksum=True)
    add("inv_reserved_frame_header_bit", ok, okw, "3.1.1.1.1: the reserved bit must be zero", reserved=1)
    add("inv_dictionary_id_5", ok, okw, "a dictionary the decoder does not have", did=(1, 5))
    add("inv_reserved_compression_modes_bits", [Comp(T, [(10, 5, 7 + 3)], modes_reserved=1)],
        Z.execute([Comp(T, [(10, 5, 7 + 3)])]), "3.1.1.3.2.1: the reserved bits must be zero")
    return C
