"""Scripted inputs for the encoder (not a test module: pytest does not collect it).  Pure Python + numpy.

An input is written from a script in zstd_synth's vocabulary, literals and copies [(literal_length, match_length, distance)], and
built so that the ONLY repeats a match finder can find in it are the planted copies:

    no_repeat_stream(n, alphabet, weights, seed)   n bytes over a weighted alphabet in which no 4-gram occurs twice
    build(script, ...)                             literals drawn the same way + the planted copies -> Built(data, plants)
    check_invariant(data, plants)                  brute force: every 4-gram that occurs twice lies wholly inside a planted copy,
                                                   its earlier occurrence at the planted distance
    greedy_parse(data)                             plain greedy longest-match parse (64 KiB window, matches of 4 bytes or more,
                                                   the nearest of equally long candidates) -> (script, trailing literals)

How a byte is drawn: by weight; if the 4-gram it would close has been seen, among the symbols whose 4-gram has not; if there is
none, one step back (the byte before is drawn again without the symbol it had).  The guard bytes around a copy come for free:
a literal behind a copy that would lengthen it closes the 4-gram that lies behind the copy's source, which has been seen, and is
drawn again; the last literal in front of a copy is drawn with the copy's first three bytes already in view, so that none of the
three 4-grams that straddle the copy's start has been seen (a copy that could start a byte earlier would make one).  Where a copy
follows a copy with no literal between them (ll == 0) the straddling 4-grams are given by bytes already written; if one of them has
been seen the build starts again from the next seed (the source cannot be moved: the distance is the script's).  Overlapping copies
(distance < length: distances 1, 2, 3, 4, 7 in the corpus) are planted on purpose; the 4-grams inside their own span, period
included, are exempt from the invariant.

What this builder cannot reach: a symbol share above about 0.25 (1/i^2 over 256 symbols gives 0.24 with half of all draws forced;
beyond that the stream cannot avoid repeating 4-grams), so a 1-bit Huffman code is out of its reach; and 16 symbols have only 65,536
4-grams, so such a stream ends below 64 KiB.

Measured: the whole corpus of tests/enc_edge_cases.py (154 cases, 3.2 MB in rounds) builds in 4.2 s on one CPU core while the rest
of the suite runs beside it (test_enc_inputs_cpu.py measures it again and holds it below a minute); it is cached per process."""
import numpy as np


class BuildError(ValueError):
    pass


class _Retry(Exception):
    pass


def zipf(n, s):
    w = 1.0 / np.arange(1, n + 1) ** s
    return w / w.sum()


class _Drawer:
    """Draws symbols by weight, in chunks; `among` draws among an allowed subset with the weights renormalised."""

    def __init__(self, alphabet, weights, seed):
        self.alpha = list(bytes(alphabet))
        w = np.ones(len(self.alpha)) if weights is None else np.asarray(weights, float)
        assert len(w) == len(self.alpha) and len(set(self.alpha)) == len(self.alpha)
        self.w = w / w.sum()
        self.wl = self.w.tolist()
        self.rng = np.random.default_rng(seed)
        self.buf, self.at = [], 0
        self.forced = 0

    def draw(self):
        if self.at == len(self.buf):
            self.buf = np.asarray(self.alpha, np.uint8)[self.rng.choice(len(self.alpha), size=4096, p=self.w)].tolist()
            self.at = 0
        self.at += 1
        return self.buf[self.at - 1]

    def among(self, ok):
        self.forced += 1
        idx = [i for i, s in enumerate(self.alpha) if ok(s)]
        if not idx:
            return None
        p = np.array([self.wl[i] for i in idx])
        return self.alpha[idx[int(self.rng.choice(len(idx), p=p / p.sum()))]]


def no_repeat_stream(n, alphabet=bytes(range(256)), weights=None, seed=0, stats=None):
    """n bytes over the weighted alphabet, no 4-gram twice.  stats (a dict) receives forced draws and steps back."""
    D = _Drawer(alphabet, weights, seed)
    out, seen, banned, back = bytearray(), set(), {}, 0
    while len(out) < n:
        p = len(out)
        if p < 3:
            out.append(D.draw())
            continue
        t = (out[p - 3] << 24) | (out[p - 2] << 16) | (out[p - 1] << 8)
        ban = banned.get(p, ())
        s = D.draw()
        if (t | s) in seen or s in ban:
            s = D.among(lambda x: (t | x) not in seen and x not in ban)
        if s is None:                                       # dead end: the byte before is drawn again without its symbol
            if p <= 3:
                raise BuildError("the alphabet is too small for a stream without repeats")
            back += 1
            banned.pop(p, None)
            last = out.pop()
            seen.discard((out[p - 4] << 24) | (out[p - 3] << 16) | (out[p - 2] << 8) | last)
            banned.setdefault(p - 1, set()).add(last)
            continue
        seen.add(t | s)
        out.append(s)
    if stats is not None:
        stats.update(forced=D.forced, back=back)
    return bytes(out)


class Built:
    """data: the bytes; plants: [(start, length, distance)] of the copies in order; script: [(ll, ml, distance)] as given;
    tail: literals behind the last copy."""

    def __init__(self, data, plants, script, tail):
        self.data, self.plants, self.script, self.tail = data, plants, script, tail


def _head(out, extra, dist, k):
    """The first k bytes of a copy at `dist` behind out + extra (the copy may read what it writes)."""
    n, res = len(out) + len(extra), []
    for i in range(k):
        j = n + i - dist
        res.append(out[j] if j < len(out) else (extra[j - len(out)] if j < n else res[j - n]))
    return res


def _build_once(script, tail, alphabet, weights, seed, prefix):
    D = _Drawer(alphabet, weights, seed)
    out, seen, plants = bytearray(), set(), []

    def gram_at(i):
        return (out[i - 3] << 24) | (out[i - 2] << 16) | (out[i - 1] << 8) | out[i]

    def push(b):
        out.append(b)
        if len(out) >= 4:
            seen.add(gram_at(len(out) - 1))

    for b in prefix:
        push(b)

    def straddle_ok(extra, dist, ml):
        """Would a copy at `dist` behind out + extra start clean: the (up to) three 4-grams across its start unseen?"""
        h = _head(out, extra, dist, min(3, ml))
        s = list(out[-3:]) + list(extra) + h
        e = len(s) - len(h)                      # index of the copy's first byte in s
        new = set()
        for j in range(max(3, e), len(s)):       # 4-grams ending at the copy's bytes 0..2 (they hold a byte from before it)
            if j - 3 < 0:
                continue
            g = (s[j - 3] << 24) | (s[j - 2] << 16) | (s[j - 1] << 8) | s[j]
            if g in seen or g in new:
                return False
            new.add(g)
        return True

    def literal(nxt):
        """One literal; nxt = (distance, length) of a copy that starts right behind it, or None."""
        p = len(out)
        if p < 3:
            s = D.draw()
            if nxt and not straddle_ok([s], *nxt):
                s = D.among(lambda x: straddle_ok([x], *nxt))
                if s is None:
                    raise _Retry
            push(s)
            return
        t = (out[p - 3] << 24) | (out[p - 2] << 16) | (out[p - 1] << 8)
        ok = (lambda x: (t | x) not in seen and straddle_ok([x], *nxt)) if nxt else (lambda x: (t | x) not in seen)
        s = D.draw()
        if not ok(s):
            s = D.among(ok)
            if s is None:
                raise _Retry
        push(s)

    done = []
    for ll, ml, dist in script:
        if not isinstance(dist, int):                       # alternatives: the first one whose copy starts clean (ll == 0 only)
            assert ll == 0
            dist = next((d for d in dist if straddle_ok([], d, ml)), None)
            if dist is None:
                raise _Retry
        done.append((ll, ml, dist))
        if dist > len(out) + ll or dist < 1 or ml < 1:
            raise BuildError(f"a copy at distance {dist} behind {len(out) + ll} bytes")
        for i in range(ll):
            literal((dist, ml) if i == ll - 1 else None)
        if ll == 0 and len(out) and not straddle_ok([], dist, ml):
            raise _Retry
        start = len(out)
        if dist >= ml:
            chunk = bytes(out[start - dist:start - dist + ml])
        else:
            pat = bytes(out[start - dist:])
            chunk = (pat * (ml // dist + 1))[:ml]
        for b in chunk:
            push(b)
        plants.append((start, ml, dist))
    for _ in range(tail):
        literal(None)
    return Built(bytes(out), plants, done, tail), D.forced


def build(script, tail=0, alphabet=bytes(range(256)), weights=None, seed=0, prefix=b"", stats=None):
    """The bytes of the script: per item `ll` fresh literals, then `ml` bytes copied from `distance` back; `tail` literals
    behind the last copy.  prefix: bytes that stand in front (they count as seen)."""
    for attempt in range(50):
        try:
            built, forced = _build_once(script, tail, alphabet, weights, seed + 7919 * attempt, prefix)
            if stats is not None:
                stats.update(forced=forced, attempts=attempt + 1)
            return built
        except _Retry:
            continue
    raise BuildError("no seed in 50 gave a clean build: alphabet too small for this script?")


def check_invariant(data, plants):
    """Brute force over every 4-gram of data.  Returns the list of violations (empty = the invariant holds): a 4-gram at q that
    occurred before must lie wholly inside a planted copy (start <= q, q + 4 <= start + length) whose source has it
    (data[q - distance : q - distance + 4] equal), or wholly inside the span of an overlapping copy and its period."""
    a = np.frombuffer(data, np.uint8).astype(np.uint32)
    if len(a) < 4:
        return []
    g = (a[:-3] << 24) | (a[1:-2] << 16) | (a[2:-1] << 8) | a[3:]
    order = np.argsort(g, kind="stable")
    gs = g[order]
    dup = np.zeros(len(g), bool)
    dup[order[1:][gs[1:] == gs[:-1]]] = True                # every occurrence but the first
    cover = np.zeros(len(g), np.int64) - 1                  # the planted copy a position lies wholly inside
    exempt = np.zeros(len(g), bool)
    for k, (s, ml, d) in enumerate(plants):
        if ml >= 4:
            cover[s:s + ml - 3] = k
        if d < ml:
            exempt[max(s - d, 0):s + ml - 3] = True
    bad = []
    for q in np.nonzero(dup & ~exempt)[0].tolist():
        k = int(cover[q])
        if k < 0:
            bad.append((q, "outside every copy"))
            continue
        d = plants[k][2]
        if data[q - d:q - d + 4] != data[q:q + 4]:
            bad.append((q, "not its source"))
    return bad


def greedy_parse(data, window=65536, min_match=4):
    """[(ll, ml, distance)], trailing literals: at every position the longest match of at least min_match bytes that starts
    within `window` bytes back (the nearest of equally long ones), taken at once; positions inside a match are indexed too."""
    n = len(data)
    table, seqs, anchor, p, ins = {}, [], 0, 0, 0
    mv = memoryview(data)

    def insert_upto(e):
        nonlocal ins
        while ins < e and ins + 4 <= n:
            table.setdefault(bytes(mv[ins:ins + 4]), []).append(ins)
            ins += 1

    def common(a, b):
        k, step = 0, 64
        while b + k < n:
            m = min(step, n - b - k)
            if mv[a + k:a + k + m] == mv[b + k:b + k + m]:
                k += m
                step = min(step * 2, 1 << 16)
                continue
            while mv[a + k] == mv[b + k]:
                k += 1
            break
        return k

    while p + min_match <= n:
        insert_upto(p)
        best, bc = 0, -1
        for c in reversed(table.get(bytes(mv[p:p + 4]), ())[-16:]):
            if p - c > window:
                break
            k = common(c, p)
            if k > best:
                best, bc = k, c
        if best >= min_match:
            seqs.append((p - anchor, best, p - bc))
            p += best
            anchor = p
        else:
            p += 1
    return seqs, n - anchor
