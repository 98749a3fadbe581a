"""The corpus of scripted encoder inputs (not a test module).  Every case is ONE round, written by tests/enc_inputs.py from a script
of literals and planted copies, placed inside a buffer whose bytes in front of and behind the round are chosen too (where a case
asks for it the bytes behind the round's end CONTINUE the last copy's source: a match length one too long shows).  A case names
the encoder line it aims at (znippy_amd/csrc/zstd_encode.hip) and carries coverage predicates pred(trace, case) over the trace
(oracle.zstd_trace) of the frame the encoder wrote, per route: level 1 (fast tier), level 19 (higher tier), "win" (level 19 with
window_log 17).  A predicate is a condition on the frame, not a measurement: it says that the boundary was reached.

What shapes every script (all three matchers, zstd_encode.hip:1188-1193, :1456-1460, :1566-1570): the 64 lanes of a window read
their hash cells before any of them writes, so a copy is found at its first byte only if its source lies in an EARLIER window.
Scripts therefore keep distances at 64 or more, or start an overlapping copy on a window's first lane (a multiple of 64 while
nothing has matched yet), where the source's last byte belongs to the window before.  Positions a long match covers are never
inserted (base jumps to the match's end), which keeps a far source alive: 65,536 bytes of fresh literals would push it out of
its bucket (8 ways x 1024 buckets, one way x 8192 cells on the fast tier), a 65,000-byte run of period 7 inserts one window.

Left out, with the line that makes each unreachable:
  * a 3-byte sequence count: MAX_SEQ = 16384 < 0x7F00 (:1103, :1678);
  * a Huffman stream above 65,535 bytes: a block holds 131,072 literals, a stream a quarter of them at 11 bits at most, 45 KiB (:726);
  * a 1-bit Huffman code: a symbol share above 0.25 is out of the builder's reach (enc_inputs.py);
  * rlen 0 and 1 WITH a planted copy, and a copy of 4-7 bytes that ends at the round's end: positions from nq - 7 on are never
    probed (scan_end, :1134); the cases are there, their predicate is that the bytes go out as literals;
  * the sequence budget n / 8 met exactly by 8-byte records: the last record's copy starts at nq - 4, behind scan_end; the case
    reaches 16,372 of 16,384 (96 bytes of lead), and the budget is SPENT by 7-byte records (3 literals + 4 copied: 18,710 in a block)
    instead of 4-byte ones: a copy that follows a copy needs a source whose neighbours differ, and with 4-byte copies only, every
    source is a copy again;
  * `room` clipping a back-extension against the previous match (:1358) has no case of its own: copy_across_128k_line meets it with
    the window, where the bytes in front of the second block agree with those in front of the source and room is what is left of
    the block."""
import functools

import numpy as np

import enc_inputs as E

KIB = 1024
BLOCK = 128 * KIB


class Case:
    def __init__(self, name, aim, buf, off, n, script, tail, preds, plants=None, window=False, exact_parse=True):
        self.name, self.aim, self.buf, self.off, self.n = name, aim, buf, off, n
        self.script, self.tail, self.preds, self.plants, self.window, self.exact_parse = script, tail, preds, plants, window, exact_parse

    @property
    def data(self):
        return self.buf[self.off:self.off + self.n]

    def __repr__(self):
        return self.name


# ---- reading a trace ----------------------------------------------------------------------------------------------------------

def blocks(T):
    return T["frames"][0]["blocks"]


def seqs(T, block=None):
    """[(ll, ml, resolved distance)] of one block, or of all blocks one behind the other."""
    bs = blocks(T) if block is None else [blocks(T)[block]]
    return [(int(s[0]), int(s[1]), int(s[3])) for b in bs if b["type"] == 2 for s in b["seqs"]]


def has(T, ll=None, ml=None, dist=None, block=None):
    return any((ll is None or s[0] == ll) and (ml is None or s[1] == ml) and (dist is None or s[2] == dist) for s in seqs(T, block))


def script(c):
    return [tuple(s) for s in c.script]


def exact(T, c):
    """The frame's sequences are the planted script, copy for copy."""
    return seqs(T) == script(c)


def header(n):
    return (0x20, 1) if n < 256 else ((0x60, 2) if n < 65792 else (0xA0, 4))


def header_ok(T, c):
    F = T["frames"][0]
    return (F["fhd"], F["fcs_bytes"]) == header(c.n) and F["content_size"] == c.n


def hib(v):
    return v.bit_length() - 1


def model_norm(counts, tl):
    """fse_build's normalisation (:295-312), restated: -> (normalised counts, 'remainder' or 'excess')."""
    total, ts = sum(counts), 1 << tl
    norm = [max(1, (c * ts + (total >> 1)) // total) if c else 0 for c in counts]
    s = sum(norm)
    if s <= ts:
        big = max(range(len(counts)), key=lambda i: (counts[i], i))
        norm[big] += ts - s
        return norm, "remainder"
    excess = s - ts
    while excess:
        k = max(range(len(norm)), key=lambda i: (norm[i], i) if norm[i] > 1 else (0, 0))
        take = min(max(norm[k] >> 2, 1), excess, norm[k] - 1)
        norm[k] -= take
        excess -= take
    return norm, "excess"


def code_counts(T, kind, block=0):
    import zstd_synth as Z
    b = blocks(T)[block]
    f = {"ll": lambda s: Z.ll_code(int(s[0]))[0], "ml": lambda s: Z.ml_code(int(s[1]))[0], "of": lambda s: Z.of_code(int(s[2]))[0]}[kind]
    c = [0] * 64
    for s in b["seqs"]:
        c[f(s)] += 1
    return c


def table_is_model(T, kind, branch=None, block=0):
    """The traced counts of a compressed table are what fse_build's rule gives for the block's own histogram (and took `branch`)."""
    b = blocks(T)[block]
    t = b["tables"][kind]
    if t["mode"] != 2:
        return False
    c = code_counts(T, kind, block)
    norm, br = model_norm(c, t["log"])
    while norm and norm[-1] == 0:
        norm.pop()
    return t["norm"] == norm and (branch is None or br == branch)


def zero_runs(norm):
    runs, k = [], 0
    for i, x in enumerate(norm):
        if x == 0:
            k += 1
        elif k:
            runs.append((i - k, k))
            k = 0
    return runs


def custom_logs_ok(T, nseq, block=0):
    b = blocks(T)[block]
    tl = min(max(hib(nseq) - 2, 6), 8)
    return b["modes"] != 0 and all(t["mode"] in (1, 2) and (t["mode"] == 1 or t["log"] == tl) for t in b["tables"].values())


# ---- scripts ------------------------------------------------------------------------------------------------------------------

def chain(recs, lead=192, piece=24, min_dist=70):
    """[(ll, ml)] -> a script in which copy i reads from the start of a stretch of fresh literals at least min_dist back: the
    lead's pieces first, then the literal stretches of earlier records in order (each used once, so no two copies share their first
    bytes and the nearest candidate is the planted one).  Returns the script; the first record's literals include the lead."""
    starts = list(range(0, lead - lead % piece, piece)) + [lead]
    pos, script = lead, []
    for i, (ll, ml) in enumerate(recs):
        p = pos + ll
        assert p - starts[i] >= min_dist and ll >= 3, (i, p, starts[i])
        assert ml <= starts[i + 1] - starts[i], "a source that runs into the next one: two copies would share bytes"
        script.append((ll + (lead if i == 0 else 0), ml, p - starts[i]))
        pos = p + ml
        starts.append(pos)
    return script


def own(n, seed, ll=(70, 90), ml=(8, 20)):
    """n records whose copy reads from its OWN literal stretch (64 bytes or more back, never beyond the stretch's start): every
    source is fresh, lies in an earlier window and shares no byte with another."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        l = int(rng.integers(ll[0], ll[1] + 1))
        out.append((l, int(rng.integers(ml[0], ml[1] + 1)), int(rng.integers(64, l + 1))))
    return out


def hash4(data, q, log):
    return ((int.from_bytes(data[q:q + 4], "little") * 2654435761) & 0xFFFFFFFF) >> (32 - log)


def survives(b, logs=(11, 13)):
    """Would every planted copy find its source's first position in a ONE-way table of 2^log cells (the fast tier's, :1459, :1569)?
    No position between the source and the copy may hash to the source's cell; positions inside a planted copy beyond its first
    64 bytes are not counted (the matcher jumps over them)."""
    skip = np.zeros(len(b.data) + 4, bool)
    for s, ml, d in b.plants:
        skip[s + 64:s + ml] = True
    for s, ml, d in b.plants:
        for log in logs:
            h = hash4(b.data, s - d, log)
            if any(not skip[q] and hash4(b.data, q, log) == h for q in range(s - d + 1, s)):
                return False
    return True


def build_clean(script, seeds, **kw):
    """E.build from the first seed whose planted sources all survive in a one-way table: the fast tier then finds every copy at its
    first byte, as the higher tier's eight ways do anyhow."""
    for _ in range(40):
        b = E.build(script, seed=next(seeds), **kw)
        if survives(b):
            return b
    raise E.BuildError("no seed keeps every source in a one-way table")


def varied(n, seed, ll=(4, 10), ml=(8, 12)):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(ll[0], ll[1] + 1)), int(rng.integers(ml[0], ml[1] + 1))) for _ in range(n)]


def clip(plants, off, n, min_match=4):
    """The script of the round [off, off + n) of a buffer: copies cut at the round's ends; a piece shorter than min_match, or one whose
    source starts in front of the round, is literals.  -> (script, tail)."""
    script, anchor = [], off
    for s, ml, d in plants:
        a, e = max(s, off), min(s + ml, off + n)
        if e - a >= min_match and a - d >= off:
            script.append((a - anchor, e - a, d))
            anchor = e
    return script, off + n - anchor


@functools.lru_cache(maxsize=1)
def cases():
    C = []

    def add(name, aim, built, preds, off=0, n=None, window=False, exact_parse=True):
        n = len(built.data) - off if n is None else n
        sc, tail = clip(built.plants, off, n)
        C.append(Case(name, aim, built.data, off, n, sc, tail, preds, built.plants, window, exact_parse))

    both = lambda p: {1: p, 19: p}
    seed = iter(range(1000, 100000, 37))
    types = lambda T: [b["type"] for b in blocks(T)]
    b0 = lambda T: blocks(T)[0]
    modes3 = lambda T: [b0(T)["tables"][k]["mode"] for k in ("ll", "of", "ml")]

    # ---- 1. frame header forms (:1749-1752), a last block below scan_end (:1134), a copy across the 128 KiB line --------------
    big = E.build(chain(varied(9000, 1)), tail=400, seed=next(seed))
    assert len(big.data) > BLOCK + 9
    for n in (0, 1, 255, 256, 257, 65791, 65792, 65793):
        add(f"hdr_rlen_{n}", ":1749-1752", big, both(lambda T, c: header_ok(T, c) and (c.n < 255 or b0(T)["type"] == 2)), n=n)
    for k in (1, 3, 7, 8, 9):
        def p(mark, k=k):
            want = [(2, None), (0, k)] + ([(0, 0)] if mark else [])
            return lambda T, c: header_ok(T, c) and len(blocks(T)) == len(want) and \
                all(b["type"] == t and (sz is None or b["size"] == sz) for b, (t, sz) in zip(blocks(T), want))
        add(f"hdr_rlen_128k_plus_{k}", ":1134 scan_end of a last block of k bytes; :1730 the closing mark", big,
            {1: p(False), 19: p(True), "win": p(False)}, n=BLOCK + k, window=True)   # (:1730 a.tail_mark is off with the window)
    recs, at = [], 0
    for r in own(2000, 2):
        if at + r[0] + r[1] > BLOCK - 40 - 400:
            break
        recs.append(r)
        at += r[0] + r[1]
    assert 400 <= BLOCK - 40 - at < 600
    line = E.build(recs + [(BLOCK - 40 - at, 100, 350)], tail=300, seed=next(seed))
    assert line.plants[-1] == (BLOCK - 40, 100, 350)
    cut = lambda T, c: seqs(T, 0)[-1][1:] == (40, 350) and sum(s[0] + s[1] for s in seqs(T, 0)) == BLOCK and not has(T, dist=350, block=1)
    add("copy_across_128k_line", ":1096 cut at the block's end; :1126 PRE, :1358 room: with the window the rest is (0, 60, 350)", line,
        {1: cut, 19: cut, "win": lambda T, c: seqs(T, 0)[-1][1:] == (40, 350) and seqs(T, 1)[:1] == [(0, 60, 350)]}, window=True)

    # ---- 2. match extension (:1218-1275 per lane, :1362-1399 cooperative, the scalar tail at mpos + o + 16 > nq) --------------
    # the last copy ends exactly at the round's end; the 40 bytes behind it continue its source
    ext_L = [4, 5, 6, 7, 8, 15, 16, 17, 63, 64, 65, 79, 80, 81] + [64 + 1024 * q + d for q in (1, 2, 4) for d in (-1, 0, 1, 15, 16, 17)]
    # (a first copy of 30 bytes lets the block shrink: a block that does not goes out raw, :1723; 340 literals send the round to the
    # higher tier's matcher at level 19, :1639; at level 1 the small variant has it, and the wide one behind a run of 17,024 bytes)
    for L in ext_L:
        b = build_clean([(300, 30, 100), (40, L + 40, 110)], seed, tail=24)
        if L < 8:
            add(f"ext_ends_at_round_end_{L}", ":1134 scan_end: a copy that starts in the last 7 bytes is never probed", b,
                both(lambda T, c: seqs(T) == [(300, 30, 100)]), n=370 + L)
        else:
            add(f"ext_ends_at_round_end_{L}", ":1218 lim = nq - pos; :1369/:1380 the piece that holds the round's end", b,
                both(lambda T, c, L=L: seqs(T) == [(300, 30, 100), (40, L, 110)]), n=370 + L)
    for L in (8, 63, 64, 65, 1087, 1088, 1089):
        b = build_clean([(128, 17024, 7), (300, 30, 100), (40, L + 40, 110)], seed, tail=24)
        add(f"ext_wide_ends_at_round_end_{L}", ":1468 lim, :1510/:1521 in the fast tier's wide variant", b,
            both(lambda T, c, L=L: seqs(T) == [(128, 17024, 7), (300, 30, 100), (40, L, 110)]), n=128 + 17024 + 370 + L)
    far = E.build([(192, 29800, 7), (8, 70040, 30000)], tail=24, seed=next(seed))
    add("ext_70000_at_distance_30000", ":427 ML code 52; :1394 whole 1 KiB quarters", far, both(lambda T, c: has(T, ml=70000, dist=30000)),
        n=30000 + 70000)
    # back-extension: a copy that starts k bytes in front of a window's first lane is hit on that lane; its source at block position
    # s: candidate s + k.  At 8 or more the k bytes in front are taken over; below 8 they are not looked at (cand >= 8, :1323)
    for s in (0, 1, 4, 7, 8, 9):
        for k in (1, 4, 7, 8):
            P = 64 - k
            want = [(P, 30, P - s)] if s + k >= 8 else [(64, 30 - k, P - s)]
            # (two lanes of a window that write one bucket leave one position: the candidate s + k must have its bucket alone)
            b = next(b for b in (E.build([(P, 30, P - s)], tail=300, seed=next(seed)) for _ in range(40))
                     if all(hash4(b.data, q, 10) != hash4(b.data, s + k, 10) for q in range(64) if q != s + k))
            add(f"back_source_at_{s}_hit_{k}_late", ":1323 cand >= 8; :1242 bk from the first load", b,
                {19: lambda T, c, want=want: seqs(T) == want})

    # ---- 3. distances ----------------------------------------------------------------------------------------------------------
    for d in (1, 2, 3, 4, 7):      # the copy starts on lane 0 of the third window
        add(f"dist_overlap_{d}", ":1255 candidates that read what the copy writes", E.build([(128, 300, d)], tail=300, seed=next(seed)),
            both(exact))
    for D in (65535, 65536, 65537):
        G = D - 128 - 24
        b = E.build([(128, G, 7), (24, 40, D)], tail=300, seed=next(seed))
        add(f"dist_{D}", ":1210-1212, :1462-1464 c -= 0x10000: 65536 is the farthest a 16-bit position names", b,
            both(exact if D <= 65536 else (lambda T, c, G=G: seqs(T) == [(128, G, 7)])), exact_parse=D <= 65536)
    for ml, D in ((4, 2048), (4, 2049), (5, 32768), (5, 32769)):
        G = D - 128 - 24
        b = E.build([(128, G, 7), (24, ml, D)], tail=300, seed=next(seed))
        add(f"gate_ml{ml}_at_{D}", ":1283 mlen == 4 && off > 2048, mlen == 5 && off > 32768", b,
            {19: exact if D in (2048, 32768) else (lambda T, c, G=G: seqs(T) == [(128, G, 7)])})

    # ---- 4. code table bounds (:426-427, :1699-1700) -----------------------------------------------------------------------------
    for ll in (63, 64, 65):
        add(f"ll_{ll}", ":426 ll < 64: the table or hib(ll) + 19", build_clean([(128, 12, 100), (ll, 12, 64)], seed, tail=300), both(exact))
    for ml in (130, 131, 132):
        add(f"ml_{ml}", ":427 mlb < 128: the table or hib(mlb) + 36", build_clean([(192, ml, 160)], seed, tail=300), both(exact))
    for extra in (0, 1, 700):      # LL code 35; the run crosses every step of the miss acceleration and store_tail's bulk copy
        run = 65536 + extra
        add(f"literal_run_{run}", ":426 LL code 35; :1342 acceleration; :1178 emitted < base",
            E.build([(100, 12, 80), (run, 1100, 1024)], tail=200, seed=next(seed)),
            both(lambda T, c: any(s[0] >= 65536 and s[1] >= 4 for s in seqs(T))))
    for k in (1, 2, 16, 17, 96):
        for d in (-1, 1):
            run = 64 * k + d
            add(f"literal_run_{run}", ":1342 base += 64 * (1 + (misses >> 4)); :1339 store_tail only for the first two misses",
                E.build([(700, 12, 80), (run, 600, 712 + run - 50)], tail=100, seed=next(seed)),
                {1: lambda T, c, run=run: any(s[0] >= run and s[1] >= 4 for s in seqs(T)),
                 19: exact if k <= 2 else (lambda T, c, run=run: any(s[0] >= run and s[1] >= 4 for s in seqs(T)))})
    add("given_up_after_96_windows", ":1341, :1489 nseq == 0 && misses >= 96: the block goes out raw",
        E.build([(30000, 600, 1024), (20, 600, 2000)], tail=100, seed=next(seed)), both(lambda T, c: types(T) == [0]))

    # ---- 5. repeat offsets, higher tier (:1409-1420) ----------------------------------------------------------------------------
    # every source lies in the 350 fresh literals in front of its copy (or of the copies it follows with ll == 0)
    rep6 = [(400, 10, 300), (350, 10, 200), (350, 10, 100), (350, 10, 100), (350, 10, 200), (350, 10, 300), (0, 10, 200), (0, 10, 100),
            (0, 10, 99), (350, 10, 99)]
    r0_1 = [(128, 300, 1), (0, 10, 408)]

    def six_forms(block):
        def p(T, c):
            got = {(int(s[2]), int(s[0]) > 0) for s in blocks(T)[block]["seqs"] if int(s[2]) <= 3}
            return got == {(v, z) for v in (1, 2, 3) for z in (True, False)} and seqs(T, block) == rep6
        return p
    filler = [(192, BLOCK - 192, 7)]
    add("rep_six_forms", ":1409-1420 all six forms", E.build(rep6, tail=300, seed=next(seed)), {19: six_forms(0)})
    add("rep_r0_is_1_ll_0", ":1418 r0 > 1: no code for distance 0", E.build(r0_1, tail=300, seed=next(seed)),
        {19: lambda T, c: seqs(T) == r0_1 and [int(s[2]) for s in b0(T)["seqs"]] == [4, 411]})
    add("rep_six_forms_second_block", ":1147 the history starts unknown in every block", E.build(filler + rep6, tail=300, seed=next(seed)),
        {19: six_forms(1)}, window=True)
    add("rep_r0_is_1_ll_0_second_block", ":1418, in a second block", E.build(filler + r0_1, tail=300, seed=next(seed)),
        {19: lambda T, c: seqs(T, 1) == r0_1}, window=True)

    # ---- 6. sequence counts (:1689 nseq > 8, the 64-sequence batches, :1678 the count's form, :431 tl, the budgets :1102) ------
    for N in (0, 1, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 511, 512, 1023, 1024):
        b = E.build(own(N, 100 + N), tail=300 if N else 396, seed=next(seed))

        def count(T, N=N):
            return b0(T)["type"] == 0 or b0(T)["nseq"] == 0 if N == 0 else (b0(T)["nseq"], b0(T)["nseq_bytes"]) == (N, 1 if N < 128 else 2)
        add(f"nseq_{N}", ":1678 count form; :1688-1690 which writer; :431-432 tl", b,
            {1: lambda T, c, N=N, count=count: count(T) and (N == 0 or b0(T)["modes"] == 0),
             19: lambda T, c, N=N, count=count: count(T) and (N == 0 or (custom_logs_ok(T, N) if N >= 128 else b0(T)["modes"] == 0))})
    n8 = (BLOCK - 96) // 8
    add("budget_8_byte_records", ":1102-1103 max_seq = n / 8: 16,372 records in a block whose budget is 16,384",
        E.build(chain([(4, 4)] * n8, lead=96, piece=8), seed=next(seed)), {19: lambda T, c: b0(T)["nseq"] >= n8 - 1})
    n7 = (BLOCK - 96) // 7
    rec7 = E.build(chain([(3, 4)] * n7, lead=96, piece=8), tail=BLOCK - 96 - 7 * n7, seed=next(seed))
    assert len(rec7.data) == BLOCK and n7 > BLOCK // 8
    add("budget_spent_7_byte_records", ":1173 nseq < max_seq: the rest of the block is literals", rec7,
        {19: lambda T, c: b0(T)["nseq"] == BLOCK // 8 and sum(x[0] + x[1] for x in seqs(T)) < BLOCK - 8192})
    hand = E.build(chain(varied(600, 7, ll=(4, 8), ml=(8, 12))), tail=40, seed=next(seed))
    assert len(hand.data) <= 16 * KIB
    add("handed_over_600_copies_in_16k", ":1638-1647 the small variant's budget n / 40 spent: the wide variant encodes the block", hand,
        both(lambda T, c: b0(T)["nseq"] == 600))

    # ---- 7. tables: fse_build (:295-312 both branches, :369-375 zero-run flags), RLE mode (:441) -----------------------------------
    # every record's copy reads from the record's own literals: LL codes 25 / 26 (64..255 literals), distances 64..ll
    add("rle_all_three", ":441 one symbol present: RLE_Mode", E.build([(80, 8, 72 - 2 * (i % 4)) for i in range(130)], tail=300, seed=next(seed)),
        {19: lambda T, c: modes3(T) == [1, 1, 1] and exact(T, c)})
    rng = np.random.default_rng(5)
    add("rle_ll_only", ":441", E.build([(100, int(rng.integers(8, 41)), 72 - 2 * (i // 2 % 4)) for i in range(130)], tail=300, seed=next(seed)),
        {19: lambda T, c: modes3(T) == [1, 2, 2] and exact(T, c)})
    add("rle_ml_only", ":441", E.build([(int(rng.integers(70, 201)), 10, 68 - 2 * (i // 2 % 3)) for i in range(130)], tail=300, seed=next(seed)),
        {19: lambda T, c: modes3(T) == [2, 2, 1] and exact(T, c)})
    add("rle_of_only", ":441", E.build([(int(rng.integers(70, 201)), int(rng.integers(8, 41)), 70 - 2 * (i % 4)) for i in range(130)], tail=300,
                                       seed=next(seed)), {19: lambda T, c: modes3(T) == [2, 1, 2] and exact(T, c)})
    # one length per ML code 2..43; distances 141..149 change from record to record (no repeat codes: one OF code).  No copy of 4
    # bytes: it has one position to be found at, and that position's bucket may have gone to another lane of its window
    up = list(range(5, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 70, 84, 99, 140]
    rec = lambda ms: [(150, m, 141 + (i * 2) % 9) for i, m in enumerate(ms)]
    add("ml_42_codes_counts_of_3", ":301-311 sum > ts: the excess comes off a quarter at a time",
        E.build(rec(up * 3 + [5, 6]), tail=300, seed=next(seed)),
        {19: lambda T, c: b0(T)["nseq"] == 128 and table_is_model(T, "ml", "excess") and exact(T, c)})
    add("ml_42_codes_counts_of_1_and_2", ":298-300 sum <= ts: the remainder goes to the most frequent symbol",
        E.build(rec(up + up + [5] * 43 + [6, 7, 8]), tail=300, seed=next(seed)),
        {19: lambda T, c: b0(T)["nseq"] == 130 and table_is_model(T, "ml", "remainder") and
         all(table_is_model(T, k) for k in ("ll", "of") if b0(T)["tables"][k]["mode"] == 2) and exact(T, c)})
    zr = [5, 7, 11, 16, 23, 31]                                                      # ML codes 2, 4, 8, 13, 20, 28
    add("ml_zero_runs_1_2_3_4_6_7", ":369-375 repeat flags: more % 3, more / 3, a run that starts at symbol 0",
        E.build(rec([zr[i % 6] for i in range(132)]), tail=300, seed=next(seed)),
        {19: lambda T, c: zero_runs(b0(T)["tables"]["ml"]["norm"]) == [(0, 2), (3, 1), (5, 3), (9, 4), (14, 6), (21, 7)]
         and table_is_model(T, "ml") and exact(T, c)})

    # ---- 8. Huffman literals (:564 HUF_MIN_LITS, :647 streams, :724 size format, :619-641 the clamp, :890 direct or FSE weights) ----
    # a run of period 7 lifts the block above 16 KiB: below, the fast tier's small variant leaves literals raw
    def lit_case(name, aim, total, alphabet, weights, preds):
        # (a short copy behind thousands of literals would be stepped over by the miss acceleration: the literals come last)
        b = build_clean([(128, 17024, 7), (40, 12, 17172)], seed, tail=total - 168, alphabet=alphabet, weights=weights)
        add(name, aim, b, preds)
        return b
    lits, huf = (lambda T: b0(T)["lits"]), (lambda T: b0(T)["huf"])
    for total in (255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385):
        def p(T, c, total=total):
            if lits(T)["regen"] != total:
                return False
            if total < 256:
                return lits(T)["type"] == 0
            want = (2, 1, 0) if total < 1024 else (2, 4, 2 if total <= 16383 else 3)
            return (lits(T)["type"], lits(T)["streams"], lits(T)["size_format"]) == want and huf(T)["kind"] == "direct" and len(huf(T)["weights"]) == 113
        lit_case(f"huf_{total}_literals_16_symbols", ":564 HUF_MIN_LITS, :647 n < 1024, :724 n <= 16383", total, bytes(range(97, 113)), None, both(p))
    for top in (126, 127, 128, 255):
        lit_case(f"huf_highest_symbol_{top}", ":648, :891 tree_bytes = 1 + (last + 1) / 2, both parities; :586 symbols >= 128 stay raw on the fast "
                 "tier; :890 FSE-compressed weights", 600, bytes(range(40, 55)) + bytes([top]), None,
                 {1: lambda T, c, top=top: lits(T)["type"] == (2 if top < 128 else 0) and lits(T)["regen"] == 600,
                  19: lambda T, c, top=top: lits(T)["type"] == 2 and huf(T)["kind"] == ("direct" if top < 128 else "fse") and
                  len(huf(T)["weights"]) == top + 1 and lits(T)["regen"] == 600})
    skew = lit_case("huf_256_symbols_clamped_to_11_bits", ":619-641, :830-861 lengths above 11 clamped, both Kraft repair loops", 60000,
                    bytes(range(256)), E.zipf(256, 2.0),
                    {19: lambda T, c: lits(T)["type"] == 2 and huf(T)["longest"] == 11 and huf(T)["kind"] == "fse"})
    cnt = np.bincount(np.frombuffer(skew.data, np.uint8), minlength=256)
    assert cnt.min() > 0 and (int(cnt.min()) << 11) < 60000         # a symbol whose Shannon length is above 11
    return C
