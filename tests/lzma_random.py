"""Random scripts for lzma_build.Writer (not a test module): script(seed) draws the properties, a legal plan of LZMA2 chunks and the
operations of every LZMA chunk, and is valid by construction — it keeps the count of bytes since the dictionary reset and
rep0..3 itself and names no distance beyond them or beyond the declared dictionary.  The Writer codes every operation as given, so
what a script reaches (an operation in a state, a length class at a pos-state, a distance slot, a dictionary reset at an odd
position) is what a decoder has to follow.  tests/test_lzma_random_cpu.py holds every file of corpus() against liblzma and asserts
what the corpus covers; tests/test_gpu_unxz_random.py runs it on the device."""
import functools
import random

import lzma_build as L
import xz_build as X
import xz_cases as K

LZMA_KINDS = (0xE0, 0xC0, 0xA0, 0x80)
KINDS = LZMA_KINDS + (1, 2)
PROPS = [(lc, lp, pb) for lc in range(5) for lp in range(5 - lc) for pb in range(5)]   # the 15 lc + lp <= 4 pairs x pb 0..4
BIASED_LENGTHS = (2, 3, 9, 10, 17, 18, 19, 273)
OPS_PER_CHUNK = 400
CORPUS = 120
FAR_LEAD = 4 * 65536        # uncompressed bytes in front of a "far" script: distances up to slot 35


def legal_next(kind, need_props):
    """the chunk kinds that may follow `kind`, and whether the next LZMA chunk must still bring properties (liblzma's rule: a dictionary
    reset asks for properties, an uncompressed chunk changes nothing)"""
    if kind == 1:
        need_props = True
    elif kind >= 0xC0:
        need_props = False
    return [k for k in KINDS if not (need_props and k in (0xA0, 0x80))], need_props


def legal_pairs():
    """every ordered pair of chunk kinds that stands somewhere in a legal sequence"""
    pairs, seen, todo = set(), set(), [(k, True) for k in (0xE0, 1)]
    while todo:
        kind, need = todo.pop()
        if (kind, need) in seen:
            continue
        seen.add((kind, need))
        nxt, need = legal_next(kind, need)
        for k in nxt:
            pairs.add((kind, k))
            todo.append((k, need))
    return pairs


class Track:
    """what the generator knows of the decoder: the bytes since the dictionary reset and rep0..3 (0-based)"""

    def __init__(self):
        self.n, self.reps = 0, [0, 0, 0, 0]


def _length(rnd):
    return rnd.choice(BIASED_LENGTHS) if rnd.random() < 0.6 else rnd.randrange(2, 274)


def _ops(w, t, rnd, count, dict_size, want_exact):
    """`count` operations, drawn one at a time: the Writer has coded the ones before, so w.hist holds the byte a matched literal is
    compared with (only the choice of a literal's value looks at it; validity rests on `t` alone)"""
    run = 0   # literals still to come in a long run
    for _ in range(count):
        r = rnd.random()
        if t.n == 0 or run:
            kind = "lit"
            run = max(run - 1, 0)
        elif want_exact[0] and t.n >= dict_size:
            kind = "exact"
        elif r < 0.45:
            kind = "lit"
        elif r < 0.47:
            kind, run = "lit", rnd.choice((61, 62, 63, 64, 65, 126, 127, 128, 129))
        elif r < 0.70:
            kind = "match"
        elif r < 0.80:
            kind = "shortrep"
        else:
            kind = "rep"
        if kind in ("rep", "shortrep"):
            ks = [k for k in range(4) if t.reps[k] < t.n] if kind == "rep" else [0] * (t.reps[0] < t.n)
            if not ks:
                kind = "lit"
        if kind == "lit":
            r = rnd.random()
            if w.state >= 7 and r < 0.5 and t.reps[0] < len(w.hist):
                mb = w.hist[-t.reps[0] - 1]
                byte = mb if r < 0.25 else mb ^ (1 << rnd.randrange(8))
            elif r < 0.75:
                byte = rnd.randrange(256)
            else:
                byte = rnd.choice(b"abcd")
            t.n += 1
            yield ("lit", byte)
        elif kind in ("match", "exact"):
            most = min(t.n, dict_size)
            if kind == "exact":
                dist, want_exact[0] = dict_size, False
                w.exact_dict += 1
            else:
                dist = rnd.randint(1, min(most, 1 << rnd.randrange(most.bit_length() + 1)))
            length = _length(rnd)
            t.reps = [dist - 1] + t.reps[:3]
            t.n += length
            yield ("match", dist, length)
        elif kind == "shortrep":
            t.n += 1
            yield ("shortrep",)
        else:
            k, length = rnd.choice(ks), _length(rnd)
            t.reps = [t.reps[k]] + t.reps[:k] + t.reps[k + 1:]
            t.n += length
            yield ("rep", k, length)


def script(seed):
    """A Writer holding the chunks of one block.  w.prop is the dictionary byte its block header has to declare, w.check the check the
    file gets, w.exact_dict how many matches reach back exactly the declared 4 KiB."""
    rnd = random.Random(seed)
    far = seed % 40 == 20
    small = seed % 4 == 3                       # one in four declares the 4 KiB dictionary
    want_exact = [small and seed % 16 == 15]    # and one in four of those places a match at exactly 4,096
    dict_size = 4096 if small else 1 << 20
    # the first 75 seeds take the 75 property triples in turn; the later ones keep to pb = 4 and lp = 4, whose masks see the most of a
    # position, and reset the dictionary more often
    keen = seed >= len(PROPS)
    some = [p for p in PROPS if p[2 - seed % 2] == 4] if keen else PROPS
    w = L.Writer(*(rnd.choice(some) if keen else PROPS[seed]))
    w.prop, w.check, w.exact_dict = (0 if small else K.PROP_1M), (X.CHECK_CRC32 if seed & 1 else X.CHECK_CRC64), 0
    t = Track()
    if far:     # a lead-in that only shifts the history: the plan behind it resets no dictionary
        for i in range(FAR_LEAD // 65536):
            w.stored(rnd.randbytes(65536), i == 0)
        t.n = FAR_LEAD
        kind, need = 2, True
    else:
        kind, need = None, True
    for _ in range(rnd.randrange(5 if keen else 3, 9)):
        if kind is None:
            kind = rnd.choice((0xE0, 1))
        else:
            nxt, need = legal_next(kind, need)
            kind = rnd.choice([k for k in nxt if not (far and k in (0xE0, 1))] + [k for k in (0xE0, 1) if keen and not far] * 2)
        if kind in (1, 2):
            data = rnd.randbytes(rnd.randrange(1, 41))
            w.stored(data, kind == 1)
            t.n = len(data) if kind == 1 else t.n + len(data)
            continue
        if kind >= 0xC0 and rnd.random() < 0.3 and any(c[0] >= 0x80 for c in w.chunks):
            w.lc, w.lp, w.pb = rnd.choice(some)    # new properties inside the block
        if kind == 0xE0:
            t.n = 0
        if kind >= 0xA0:
            t.reps = [0, 0, 0, 0]
        w.lzma(_ops(w, t, rnd, rnd.randrange(OPS_PER_CHUNK // 2, OPS_PER_CHUNK * 3 // 2), dict_size, want_exact), control=kind)
        assert t.n == len(w.hist) and t.reps == w.reps, seed
    return w


@functools.lru_cache(None)
def corpus():
    """[(seed, file, content, writer)]"""
    out = []
    for seed in range(CORPUS):
        w = script(seed)
        f, content = K.scripted_file(w, check=w.check, prop=w.prop)
        out.append((seed, f, content, w))
    return out
