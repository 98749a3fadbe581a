"""The hand-built frames of tests/zstd_synth_cases.py against two CPU judges, and the writer against itself.

Every foreign frame elsewhere in the suite comes out of libzstd; these come out of a writer that takes every choice RFC 8878
leaves to an encoder as an argument.  Here, without a GPU:
  - every valid case decodes, by the system's libzstd and by the oracle, to exactly the bytes of the reference executor;
  - every invalid case is rejected by the oracle; where libzstd accepts one, the case is "disputed" and the list of those
    is written down below with the reason (a libzstd upgrade shows up as a diff of that list);
  - every case is parsed back with a small header walker and holds what its name promises, so that the corpus cannot
    silently stop covering a corner."""
import functools

import pytest

import workloads
import zstd_synth as Z
import zstd_synth_cases as K

VALID = {c.name: c for c in K.valid_cases()}
INVALID = {c.name: c for c in K.invalid_cases()}

# invalid to the RFC and to the oracle, accepted by libzstd 1.4.8 -- and why it accepts
DISPUTED = {
    "inv_offset_zero_from_rep0_minus_1": "libzstd forces an offset of 0 to 1 (ZSTD_decodeSequence: offset += !offset)",
    "inv_code_length_12": "libzstd's Huffman reader allows HUF_TABLELOG_MAX = 12 bits, one more than the format's 11",
    "inv_bitstream_bits_left_over": "libzstd 1.4.8 does not require the sequence bitstream to be consumed to its last bit",
    "inv_bitstream_a_byte_left_over": "libzstd 1.4.8 does not require the sequence bitstream to be consumed to its last bit",
    "inv_block_regenerates_more_than_128k": "libzstd bounds a block's output by the destination, not by Block_Maximum_Size",
    "inv_reserved_compression_modes_bits": "libzstd ignores the two reserved bits of Compression_Modes",
}


# ---- the two judges ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(VALID))
def test_valid_case_decodes_to_the_executors_bytes(oracle, name):
    c = VALID[name]
    assert workloads.libzstd_decompress(c.frame, len(c.want) + 16) == c.want
    assert oracle.zstd_decompress(c.frame, cap=len(c.want) + 16) == c.want
    if not c.no_size:
        assert oracle.zstd_decompressed_size(c.frame) == len(c.want)
        assert oracle.zstd_decompress(c.frame) == c.want


def _libzstd_accepts(c):
    try:
        workloads.libzstd_decompress(c.frame, len(c.want) + 16)
        return True
    except RuntimeError:
        return False


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_case_is_rejected(oracle, name):
    c = INVALID[name]
    assert c.why
    with pytest.raises(ValueError):
        oracle.zstd_decompress(c.frame, cap=len(c.want) + 16)
    assert _libzstd_accepts(c) == (name in DISPUTED), DISPUTED.get(name, "libzstd accepts a frame the oracle rejects")


def test_disputed_list_is_exact():
    assert sorted(n for n, c in INVALID.items() if _libzstd_accepts(c)) == sorted(DISPUTED)


def test_executor_tells_invalid_descriptions():
    for name, msg in (("inv_offset_zero_from_rep0_minus_1", "zero"), ("inv_offset_beyond_frame_start_first_block", "beyond the start"),
                      ("inv_offset_beyond_frame_start_later_block", "beyond the start"), ("inv_offset_code_31", "beyond the start"),
                      ("inv_literal_lengths_beyond_literals", "beyond the literals"), ("inv_block_regenerates_more_than_128k", "128 KiB")):
        with pytest.raises(Z.SynthError, match=msg):
            Z.execute(INVALID[name].blocks)
    # the rules of 3.1.1.5 on a case small enough to follow by hand: history 1, 4, 8
    lits = b"abcdefghijkl"
    got = Z.execute([Z.Comp(lits, [(9, 2, 3), (0, 2, 3), (1, 2, 1), (0, 3, 1)])])
    #   "abcdefghi" | rep2 = 8: "bc" | ll=0, value 3: rep0-1 = 7: "ef" | "j", rep0 = 7: "hi" | ll=0, value 1: rep1 = 8: "ibc"
    assert got == b"abcdefghi" + b"bc" + b"ef" + b"j" + b"hi" + b"ibc" + b"kl"


def test_xxh64_of_the_writer(oracle):
    for n in (0, 1, 3, 4, 8, 31, 32, 33, 100, 1000):
        d = bytes((i * 7 + n) & 255 for i in range(n))
        assert Z.xxh64(d) == oracle.xxh64(d), n
    c = VALID["hdr_checksum"]
    assert Z.write_frame(c.blocks, checksum=True, xxh=oracle.xxh64) == c.frame


def test_corpus_size():
    assert 100 <= len(VALID) + len(INVALID) <= 400
    assert sum(len(c.want) for c in VALID.values()) < 40 << 20
    assert [n for n, c in VALID.items() if len(c.want) > 1 << 20] == ["extreme_codes_offset_code_22_above_4_mib"]
    assert max(len(c.want) for c in VALID.values()) <= 8 << 20


# ---- the header walker ------------------------------------------------------------------------------------------------

class _Fwd:
    def __init__(self, b, at):
        self.v, self.pos = int.from_bytes(b[at:at + 80], "little"), 0

    def read(self, n):
        r = (self.v >> self.pos) & ((1 << n) - 1)
        self.pos += n
        return r


def _read_ncount(b, at, max_sym):
    """-> (counts, accuracy log, bytes used, [lengths of the chains of repeat flag 3])."""
    r = _Fwd(b, at)
    log = 5 + r.read(4)
    remaining, norm, chains = 1 << log, [], []
    while remaining > 0 and len(norm) <= max_sym:
        bits = (remaining + 1).bit_length()
        low_mask, threshold = (1 << (bits - 1)) - 1, (1 << bits) - 1 - (remaining + 1)
        v = r.read(bits)
        if (v & low_mask) < threshold:
            r.pos -= 1
            v &= low_mask
        elif v > low_mask:
            v -= threshold
        norm.append(v - 1)
        remaining -= abs(v - 1)
        if v == 1:
            chain = 0
            while True:
                rep = r.read(2)
                norm += [0] * rep
                if rep != 3:
                    break
                chain += 1
            chains.append(chain)
    assert remaining == 0
    return norm, log, (r.pos + 7) // 8, chains


def _fse_table(norm, log):
    """(symbol, number of bits, baseline) per state: the decoding table of section 4.1.1, built here."""
    size = 1 << log
    sym, high, nxt = [0] * size, size, {}
    for s, p in enumerate(norm):
        if p == -1:
            high -= 1
            sym[high] = s
            nxt[s] = 1
    pos = 0
    for s, p in enumerate(norm):
        for _ in range(max(p, 0)):
            sym[pos] = s
            pos = (pos + (size >> 1) + (size >> 3) + 3) & (size - 1)
            while pos >= high:
                pos = (pos + (size >> 1) + (size >> 3) + 3) & (size - 1)
        if p > 0:
            nxt[s] = p
    nb, base = [0] * size, [0] * size
    for i in range(size):
        ns = nxt[sym[i]]
        nxt[sym[i]] += 1
        nb[i] = log - (ns.bit_length() - 1)
        base[i] = (ns << nb[i]) - size
    return sym, nb, base, log


def _fse_weights(b, at, n):
    """The weights of an FSE-compressed tree description (section 4.2.1.2)."""
    norm, log, used, _ = _read_ncount(b, at, 12)
    sym, nb, base, log = _fse_table(norm, log)
    stream = int.from_bytes(b[at + used:at + n], "little")
    left = stream.bit_length() - 1

    def read(k):
        nonlocal left
        left -= k
        return (stream >> left) & ((1 << k) - 1) if left >= 0 else 0
    s1, s2, out = read(log), read(log), []
    while True:
        out.append(sym[s1])
        s1 = base[s1] + read(nb[s1])
        if left < 0:
            out.append(sym[s2])
            break
        out.append(sym[s2])
        s2 = base[s2] + read(nb[s2])
        if left < 0:
            out.append(sym[s1])
            break
    return out


@functools.lru_cache(maxsize=None)
def _walk(frame):
    """The frame's header fields and, per block, what its section headers say."""
    p, skippable = 0, 0
    while int.from_bytes(frame[p:p + 4], "little") & 0xFFFFFFF0 == 0x184D2A50:
        p += 8 + int.from_bytes(frame[p + 4:p + 8], "little")
        skippable += 1
    assert frame[p:p + 4] == Z.MAGIC
    fhd = frame[p + 4]
    single, did_bytes = (fhd >> 5) & 1, (0, 1, 2, 4)[fhd & 3]
    fcs_bytes = (1 << (fhd >> 6)) if fhd >> 6 else single
    p += 5 + (0 if single else 1)
    did = int.from_bytes(frame[p:p + did_bytes], "little")
    p += did_bytes
    fcs_raw = int.from_bytes(frame[p:p + fcs_bytes], "little")
    p += fcs_bytes
    F = dict(skippable=skippable, fhd=fhd, did=did, fcs_raw=fcs_raw, fcs_bytes=fcs_bytes, blocks=[])
    tabs = {}
    while True:
        bh = int.from_bytes(frame[p:p + 3], "little")
        B = dict(type=(bh >> 1) & 3, size=bh >> 3, last=bh & 1)
        F["blocks"].append(B)
        p += 3
        if B["type"] == 2:
            _walk_block(frame, p, B, tabs)
        p += 1 if B["type"] == 1 else B["size"]
        if B["last"]:
            break
    assert p + (4 if fhd & 4 else 0) == len(frame)
    return F


def _walk_block(f, p, B, tabs):
    end = p + B["size"]
    lt, sf = f[p] & 3, (f[p] >> 2) & 3
    h = int.from_bytes(f[p:p + 5], "little")
    if lt <= 1:
        hl = 1 if sf in (0, 2) else (2 if sf == 1 else 3)
        regen = (h & 0xFF) >> 3 if hl == 1 else (h & ((1 << (8 * hl)) - 1)) >> 4
        q = p + hl + (regen if lt == 0 else 1)
    else:
        hl, nb = {0: (3, 10), 1: (3, 10), 2: (4, 14), 3: (5, 18)}[sf]
        regen, comp = (h >> 4) & ((1 << nb) - 1), (h >> (4 + nb)) & ((1 << nb) - 1)
        q = p + hl + comp
        if lt == 2:
            hb = f[p + hl]
            if hb >= 128:
                n = hb - 127
                ws = [(f[p + hl + 1 + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(n)]
                kind = "direct"
            else:
                ws, kind = _fse_weights(f, p + hl + 1, hb), "fse"
            total = sum(1 << (w - 1) for w in ws if w)
            bits = total.bit_length()
            left = (1 << bits) - total
            assert left & (left - 1) == 0
            B["tree"] = dict(kind=kind, header=hb, nweights=len(ws), bits=bits, last_weight=left.bit_length(), weights=ws)
    B["lit"] = (lt, sf, regen)
    s0 = f[q]
    if s0 < 128:
        B["nseq"], q = (1, s0), q + 1
    elif s0 < 255:
        B["nseq"], q = (2, ((s0 - 128) << 8) + f[q + 1]), q + 2
    else:
        B["nseq"], q = (3, f[q + 1] + (f[q + 2] << 8) + 0x7F00), q + 3
    if B["nseq"][1]:
        B["modes"] = f[q]
        q += 1
        B["fse"], B["chains"] = {}, {}
        for kind, shift in (("ll", 6), ("of", 4), ("ml", 2)):
            mode = (B["modes"] >> shift) & 3
            if mode == 0:
                tabs[kind] = _fse_table(*Z.DEFAULTS[kind])
            elif mode == 1:
                tabs[kind] = ([f[q]], [0], [0], 0)
                q += 1
            elif mode == 2:
                norm, log, used, chains = _read_ncount(f, q, Z.MAX_SYM[kind])
                B["fse"][kind] = (log, sum(1 for x in norm if x == -1))
                B["chains"][kind] = chains
                tabs[kind] = _fse_table(norm, log)
                q += used
        assert q < end
        # the codes of every sequence, read from the bitstream (section 3.1.1.3.2.1.1)
        left = 8 * (end - q) - 9 + f[end - 1].bit_length()      # bits under the closing 1 bit

        def read(k):
            nonlocal left
            left -= k
            assert left >= 0
            at = q + (left >> 3)
            return (int.from_bytes(f[at:at + 8], "little") >> (left & 7)) & ((1 << k) - 1)
        (sl, nl, bl, logl), (so, no, bo, logo), (sm, nm, bm, logm) = tabs["ll"], tabs["of"], tabs["ml"]
        xl, xo, xm = read(logl), read(logo), read(logm)
        mx = dict(ll=0, of=0, ml=0)
        for i in range(B["nseq"][1]):
            cl, co, cm = sl[xl], so[xo], sm[xm]
            mx = dict(ll=max(mx["ll"], cl), of=max(mx["of"], co), ml=max(mx["ml"], cm))
            read(co), read(Z.ML_BITS[cm]), read(Z.LL_BITS[cl])
            if i + 1 < B["nseq"][1]:
                xl = bl[xl] + read(nl[xl])
                xm = bm[xm] + read(nm[xm])
                xo = bo[xo] + read(no[xo])
        assert left == 0
        B["max_codes"] = mx
    else:
        assert q == end


# ---- the writer's self-checks -------------------------------------------------------------------------------------------

def _opens_with(block, ovs, ll0):
    return len(block.seqs) >= len(ovs) and all(s[2] == ov and (s[0] == 0) == ll0 for s, ov in zip(block.seqs, ovs))


@pytest.mark.parametrize("name", sorted(VALID))
def test_frame_holds_what_its_name_promises(name):
    c = VALID[name]
    F = _walk(c.frame)
    B = F["blocks"]
    want_types = [0 if isinstance(b, Z.Raw) else (1 if isinstance(b, Z.Rle) else 2) for b in c.blocks]
    assert [b["type"] for b in B][:len(want_types)] == want_types and len(B) - len(want_types) in (0, 1)
    for b, d in zip(B, c.blocks):
        if b["type"] == 2:
            assert b["nseq"][1] == len(d.seqs) and b["lit"][2] == len(d.lits)
    assert (F["fcs_bytes"] == 0) == c.no_size
    if not c.no_size:
        assert F["fcs_raw"] + (256 if F["fcs_bytes"] == 2 else 0) == len(c.want)
    P = dict(c.promise)
    group = name.split("_")[0]
    assert P or group in ("rep", "match"), "a case that promises nothing"
    for key, val in P.items():
        if key == "fhd":
            assert F["fhd"] == val and F["did"] == 0
        elif key in ("fcs_raw", "skippable"):
            assert F[key] == val
        elif key == "types":
            assert [b["type"] for b in B] == val
        elif key == "sizes":
            for i, v in (val.items() if isinstance(val, dict) else enumerate(val)):
                assert B[i]["size"] == v
        elif key in ("modes", "lit", "nseq", "fse"):
            for i, v in val.items():
                assert B[i][key] == v, (key, i, B[i].get(key), v)
        elif key == "tree":
            for i, v in val.items():
                assert B[i]["tree"]["kind"] == v
        elif key in ("nweights", "last_weight"):
            for i, v in val.items():
                assert B[i]["tree"][key] == v, (key, B[i]["tree"])
        elif key == "huf_bits":
            for i, v in val.items():
                assert B[i]["tree"]["bits"] == v
        elif key == "zero_runs":
            for i, kinds in val.items():
                for kind, n in kinds.items():
                    assert n in B[i]["chains"][kind], (kind, B[i]["chains"])
        elif key == "max_codes":
            for i, v in val.items():
                assert all(B[i]["max_codes"][k] == x for k, x in v.items()), (i, B[i]["max_codes"], v)
        else:
            raise AssertionError(f"unknown promise {key}")
    if "128_direct_weights" in name:
        assert B[0]["tree"]["kind"] == "direct" and B[0]["tree"]["header"] == 255
    if "symbol_255" in name:
        assert 255 in c.blocks[0].lits
    if "zero_weights_in_the_middle" in name:
        assert B[0]["tree"]["weights"] == [2, 0, 0, 1, 0, 0, 0]
    if group == "rep":
        later = [b for b in c.blocks[1:] if isinstance(b, Z.Comp) and b.seqs]
        first = c.blocks[0]
        if "first_block" in name or name == "rep_minus_1_down_to_1":
            assert any(s[2] <= 3 for s in first.seqs)
        else:
            assert later and all(b.seqs[0][2] <= 3 for b in later)
        if "rep0_minus_1_chain" in name or "rep_minus_1_chain" in name:
            blocks = later or [Z.Comp(b"", first.seqs[1:])]
            assert all(_opens_with(b, [3, 3, 3], True) for b in blocks)
        if "_ll0_" in name:
            assert _opens_with(later[0], [1, 2, 3], True)
        if "_ll_positive_" in name:
            assert _opens_with(later[0], [1, 2, 3], False)
        for tag, cls in (("after_raw_block", Z.Raw), ("after_rle_block", Z.Rle)):
            if tag in name:
                assert isinstance(c.blocks[1], cls)
        if "after_zero_sequence_block" in name:
            assert B[1]["type"] == 2 and B[1]["nseq"] == (1, 0)
    if group == "match":
        n = len(c.want)
        if "under_64k" in name:
            assert n < 65536 and (len(B) == 1) == ("one_block" in name)
        elif "resolve_small_table" in name or "above_64k" in name:
            assert 65537 <= n < 262144
        elif "above_256k" in name:
            assert n >= 262144
        elif "exactly" in name:
            assert n == int(name.split("_")[2])
        if "matrix" in name:
            dists = {s[2] - 3 for b in c.blocks for s in b.seqs}
            assert {1, 2, 3, 7, 8, 15, 16, 17} <= dists
        if "overlap" in name:
            assert all(b.seqs[0][0] == 0 and b.seqs[0][1] > b.seqs[0][2] - 3 for b in c.blocks[1:] if isinstance(b, Z.Comp))


def test_every_writer_choice_is_taken_somewhere():
    """The list of section 1 of the writer's brief, counted over the whole valid corpus."""
    seen = set()
    for c in VALID.values():
        F = _walk(c.frame)
        seen.add(("fcs", F["fcs_bytes"]))
        seen.add(("single", (F["fhd"] >> 5) & 1))
        seen.add(("did_bytes", (0, 1, 2, 4)[F["fhd"] & 3]))
        seen.add(("checksum", (F["fhd"] >> 2) & 1))
        seen.add(("skippable", F["skippable"] > 0))
        for b in F["blocks"]:
            seen.add(("block", b["type"]))
            if b["type"] == 0 and b["size"] == 0 and b["last"] and len(F["blocks"]) > 1:
                seen.add("empty last raw block")
            if b["type"] != 2:
                continue
            seen.add(("lit", b["lit"][0], b["lit"][1]))
            if "tree" in b:
                seen.add(("tree", b["tree"]["kind"]))
            seen.add(("nseq", b["nseq"][0]))
            if "modes" in b:
                for kind, shift in (("ll", 6), ("of", 4), ("ml", 2)):
                    seen.add((kind, (b["modes"] >> shift) & 3))
                for kind, (log, low) in b["fse"].items():
                    seen.add((kind, "log", log))
    want = {("fcs", n) for n in (0, 1, 2, 4, 8)} | {("single", 0), ("single", 1), ("checksum", 0), ("checksum", 1), ("skippable", True)}
    want |= {("did_bytes", n) for n in (0, 1, 2, 4)} | {("block", t) for t in (0, 1, 2)} | {"empty last raw block"}
    want |= {("lit", t, f) for t in (0, 1) for f in (0, 1, 2, 3)} | {("lit", t, f) for t in (2, 3) for f in (0, 1, 2)} | {("lit", 2, 3)}
    want |= {("tree", "direct"), ("tree", "fse")} | {("nseq", n) for n in (1, 2, 3)}
    want |= {(k, m) for k in ("ll", "of", "ml") for m in (0, 1, 2, 3)}
    want |= {("ll", "log", 5), ("of", "log", 5), ("ml", "log", 5), ("ll", "log", 9), ("of", "log", 8), ("ml", "log", 9)}
    assert not want - seen, sorted(map(str, want - seen))
