"""The encoder (znippy_amd/csrc/zstd_encode.hip) driven by scripted inputs onto its format and matcher edges: the corpus of
tests/enc_edge_cases.py, every case one round whose only repeats are the copies its script plants (tests/enc_inputs.py), every
frame read back with the oracle's trace (oracle.zstd_trace, tests/test_zstd_trace_cpu.py).

Routes.  Every case is encoded at level 1 and level 19, the cases above one block also at level 19 with window_log 17; on each route
alone (Context.compress), in one table of all the route's cases in shuffled order, and (cases of at most 16 KiB) in a table of small
rounds only, which takes the small variant with the hash fused.  The three frames of a case must be the same bytes.  In the tables
a round lies inside its case's buffer: what stands behind its end continues the last copy's source where the case says so.

Judges, for every frame: libzstd decodes it to the round; the oracle's strict decoder does; executing the traced description
(zstd_synth.execute) gives the round; it is no longer than compress_bound; the table's digest is the oracle's BLAKE3; and every
table comes back through RowTable.decode_verify with no corrupt row, no decode error and equal bytes.

Coverage.  On the routes a case names, its predicate over the trace must hold: the frame shows that the boundary the case aims at
(Case.aim, a line of zstd_encode.hip) was reached, mostly by holding exactly the planted sequences.

All GPU work happens once, in the module's fixture: a handful of tables and a few hundred small compress calls."""
import numpy as np
import pytest

import enc_edge_cases as K
import zstd_synth as Z

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in K.cases()}
ROUTES = (1, 19, "win")
SMALL = 16 * 1024


def route_cases(route):
    return [c for c in CASES.values() if route != "win" or c.window]


def staging():
    """Every case's buffer once, 64 bytes apart -> (bytes, {buffer id: offset})."""
    out, at = bytearray(), {}
    for c in CASES.values():
        if id(c.buf) not in at:
            at[id(c.buf)] = len(out)
            out += c.buf + bytes(64)
    return bytes(out), at


def run_table(ctx, d_src, base, cases, oracle):
    """One RoundTable of the cases' rounds: -> {name: frame}, {name: digest}, what decode_verify said."""
    import torch
    from znippy_amd import hip
    so = np.array([base[id(c.buf)] + c.off for c in cases], np.uint64)
    ln = np.array([c.n for c in cases], np.uint64)
    rt = hip.RoundTable(ctx, so, ln)
    d_blob = torch.zeros(rt.blob_bound() + 64, dtype=torch.uint8, device="cuda")
    enc = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in rt.encode_hash(d_src, d_blob).items()}
    rt.close()
    hb = d_blob.cpu().numpy()
    frames = {c.name: hb[int(enc["blob_offset"][i]):int(enc["blob_offset"][i] + enc["blob_size"][i])].tobytes() for i, c in enumerate(cases)}
    digests = {c.name: bytes(enc["checksum"][i]) for i, c in enumerate(cases)}
    oo = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    total = int(ln.sum())
    rows = hip.RowTable(ctx, enc["blob_offset"], enc["blob_size"], ln, oo, None, enc["checksum"])
    d_out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    counters, corrupt, status = rows.decode_verify(d_blob, d_out)
    rows.close()
    back = d_out[:total].cpu().numpy().tobytes() == b"".join(c.data for c in cases)
    return frames, digests, dict(counters=counters, total=total, equal=back, compressed=[int(x) for x in enc["compressed"]])


def collect(oracle):
    """{route: {"alone" / "all" / "small": {name: frame}, "digest": {name: bytes}, "tables": {which: decode_verify's word}}}"""
    import torch
    from znippy_amd import hip
    data, base = staging()
    d_src = torch.from_numpy(np.frombuffer(data + bytes(64), np.uint8).copy()).cuda()
    out = {}
    for route in ROUTES:
        ctx = hip.Context(0)
        try:
            ctx.set_level(1 if route == 1 else 19)
            if route == "win":
                ctx.set_window_log(17)
            cs = route_cases(route)
            r = dict(alone={c.name: ctx.compress(c.data) for c in cs}, bound={c.name: ctx.compress_bound(c.n) for c in cs}, tables={})
            order = np.random.default_rng(11).permutation(len(cs))
            r["all"], r["digest"], r["tables"]["all"] = run_table(ctx, d_src, base, [cs[i] for i in order], oracle)
            small = [c for c in cs if c.n <= SMALL]
            if small:
                r["small"], dg, r["tables"]["small"] = run_table(ctx, d_src, base, small, oracle)
                r["digest_small"] = dg
            out[route] = r
        finally:
            ctx.close()
    return out


@pytest.fixture(scope="module")
def runs(oracle):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return collect(oracle)


def judge(oracle, c, frame, bound):
    """Judges 1-4 on one frame; -> the trace."""
    data = c.data
    assert len(frame) <= bound, (c.name, len(frame), bound)
    assert oracle.libzstd_decompress(frame, max(c.n, 1)) == data, (c.name, "libzstd")
    assert oracle.zstd_decompress(frame, cap=c.n) == data, (c.name, "oracle")
    T = oracle.zstd_trace(frame, cap=c.n)
    assert len(T["frames"]) == 1 and T["content"] == data
    assert Z.execute(Z.blocks_of_trace(T["frames"][0], T["content"])) == data, (c.name, "execute(trace)")
    return T


def describe(T, c):
    got = K.seqs(T)
    want = K.script(c)
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    B = K.blocks(T)
    return dict(case=c.name, aim=c.aim, nseq=[b.get("nseq") for b in B], types=[b["type"] for b in B], first_diff=k,
                got=got[max(k - 1, 0):k + 3], want=want[max(k - 1, 0):k + 3], n_got=len(got), n_want=len(want),
                lits=[(b["lits"]["type"], b["lits"]["size_format"], b["lits"]["streams"], b["lits"]["regen"]) for b in B if b["type"] == 2],
                modes=[b.get("modes") for b in B])


@pytest.mark.parametrize("name,route", [(c.name, route) for route in ROUTES for c in route_cases(route)])
def test_case(runs, oracle, name, route):
    c = CASES[name]
    r = runs[route]
    frame = r["alone"][name]
    assert r["all"][name] == frame, (name, route, "the frame alone and in the table of all cases differ")
    if c.n <= SMALL:
        assert r["small"][name] == frame, (name, route, "the frame alone and in the table of small rounds differ")
        assert r["digest_small"][name] == oracle.blake3(c.data)
    assert r["digest"][name] == oracle.blake3(c.data), (name, route, "digest")
    T = judge(oracle, c, frame, r["bound"][name])
    pred = c.preds.get(route)
    if pred is not None:
        assert pred(T, c), describe(T, c)


@pytest.mark.parametrize("route", ROUTES)
def test_tables_come_back_through_the_read_path(runs, route):
    for which, t in runs[route]["tables"].items():
        cn = t["counters"]
        assert cn["corrupt_rows"] == 0 and cn["decode_errors"] == 0 and cn["verified_bytes"] == t["total"] and t["equal"], (route, which, cn)


def test_what_was_traced(runs, oracle):
    frames = seqs = 0
    for route in ROUTES:
        for name, f in runs[route]["alone"].items():
            T = oracle.zstd_trace(f, cap=CASES[name].n)
            frames += 1 + (name in runs[route]["all"]) + (name in runs[route].get("small", {}))
            seqs += sum(b["nseq"] for b in K.blocks(T) if b["type"] == 2)
    print(f"encoder edges: {len(CASES)} cases, {frames} frames, {seqs} sequences traced")
    assert frames >= 2 * len(CASES)
