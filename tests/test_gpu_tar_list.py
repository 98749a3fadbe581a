"""znippy_tar_list_batch against the Python listing (tests/tar_list_model.py, pinned to `tarfile` and to the C++ listing by
tests/test_tar_list_cpu.py): valid tars, the chain lengths around the wave and round boundaries, candidates off the chain, every cut
and a mutation sample of one small tar, items at odd addresses, filters, caps, the host's validation and an item across the 4 GiB
line.  One batch per test; every call has guard bytes around all it may write (tests/tar_list_checks.py)."""
import ctypes as C

import numpy as np
import pytest

import tar_list_model as M
from gpu_cases import FAR_LINE
from tar_list_checks import call, expect, run_batch
from test_tar_list_cpu import END, MEMBER, entry, many, mutation_sample, valid_tars
from test_tar_rules_cpu import header, make_tar, octal, pax, small

pytestmark = pytest.mark.gpu

SKIP = entry(b"g", pax(b"comment", b"c"))


def false_candidates():
    """tars with valid headers that the chain does not reach"""
    a = header(b"a", octal(1), b"0") + b"A" + bytes(511)
    return [valid_tars()["nested-gnu"], valid_tars()["nested-pax"],
            header(b"zeros", octal(4096), b"0") + bytes(4096) + a + END,                                        # a member of eight zero blocks
            header(b"trap", octal(512), b"0") + header(b"far", octal(1 << 30), b"0") + a + END,                  # data that is a header with a size far beyond the tar
            header(b"trap2", octal(1024), b"0") + entry(b"L", b"n" * 9000)[:1024] + a + END,                     # data that is an unsupported header
            a + END + a + a + END,                                                                              # valid headers behind the two zero blocks
            a + bytes(512) + a + END]                                                                           # (one zero block is stepped over)


def status_tars():
    """tars that end in a status, and edge cases of the extended headers"""
    return [entry(b"x", pax(b"path", b"p/Cargo.toml") + pax(b"size", b"2")) + MEMBER + END, entry(b"x", pax(b"size", b"3")) + MEMBER + END,
            entry(b"x", pax(b"size", b"1")) + header(b"d", octal(0), b"5") + MEMBER + END, entry(b"L", b"n" * 8193) + MEMBER + END,
            entry(b"L", b"n" * 8192) + MEMBER + END, header(b"sparse", octal(0), b"S") + MEMBER + END, entry(b"x", pax(b"GNU.sparse.major", b"1")) + MEMBER + END,
            entry(b"L", b"name\0") + END, entry(b"L", b"name\0"), entry(b"L", b"name\0") + bytes(512) + MEMBER + END, entry(b"x", b"12 path=a\n") + MEMBER + END,
            header(b"././@LongLink", octal(600), b"L") + b"n" * 512, entry(b"L", b"first/Cargo.toml\0") + entry(b"x", pax(b"path", b"second")) + MEMBER + MEMBER + END,
            entry(b"x", pax(b"path", b"one") + pax(b"path", b"two")) + entry(b"K", b"link\0") + entry(b"g", pax(b"path", b"g")) + MEMBER + END,
            entry(b"L", b"a/long/dir\0") + header(b"d", octal(0), b"5") + MEMBER + END, b"", bytes(512), bytes(511), bytes(1024), MEMBER, MEMBER[:1023],
            b"this is a text file named .crate, and it is longer than a block" * 10, header(b"big", octal(1 << 32), b"0") + bytes(2048),
            # runs of extended headers: 64 are looked back over, the 65th is unsupported
            entry(b"L", b"the/first/name\0") + SKIP * 63 + MEMBER + MEMBER + END, SKIP * 64 + MEMBER + SKIP * 64 + MEMBER + bytes(512) + SKIP * 64 + END,
            SKIP * 65 + MEMBER + END, entry(b"L", b"n\0") + SKIP * 64 + MEMBER + END, MEMBER + SKIP * 65, SKIP * 64 + entry(b"K", b"k\0") + b"junk" * 128,
            SKIP * 300 + MEMBER + END]


def test_valid_tars(gpu_ctx):
    tars = list(valid_tars().values())
    want = expect(tars)
    assert want[0] == [0] * len(tars) and want[1][-1] > 3000
    got = run_batch(gpu_ctx, tars)
    assert got == want
    names = [n for n, _ in gpu_ctx.kernel_times()]
    assert names == ["tar_scan", "tar_chain", "tar_emit", "tar_emit_write", "tar_gather"], names
    m = run_batch(gpu_ctx, tars, measure=True)
    assert (m[0], m[1], m[5], m[6], m[7]) == (want[0], want[1], want[5], want[6], 0)
    # the same without contents, and at aligned addresses
    assert run_batch(gpu_ctx, tars, contents=False) == expect(tars, contents=False)
    assert run_batch(gpu_ctx, tars, odd=False) == want


def test_chain_edges(gpu_ctx):
    tars = [many(n) for n in (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 3000)]
    want = expect(tars)
    assert [want[1][i + 1] - want[1][i] for i in range(len(tars))] == [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 3000]
    assert run_batch(gpu_ctx, tars) == want


def test_false_candidates_and_statuses(gpu_ctx):
    tars = false_candidates() + status_tars()
    want = expect(tars)
    assert want[0][:len(false_candidates())] == [0] * len(false_candidates())
    assert {M.OK, M.E_CORRUPT, M.E_UNSUPPORTED} == set(want[0])
    assert run_batch(gpu_ctx, tars) == want
    m = run_batch(gpu_ctx, tars, measure=True)
    assert (m[0], m[1], m[5], m[6]) == (want[0], want[1], want[5], want[6])


def test_every_cut(gpu_ctx):
    data = small()
    tars = [data[:k] for k in range(len(data) + 1)]
    want = expect(tars, contents=False)
    assert set(want[0]) == {M.OK, M.E_CORRUPT}
    assert run_batch(gpu_ctx, tars, contents=False) == want


def test_a_mutation_sample(gpu_ctx):
    data = small()
    tars = []
    for off, x in mutation_sample(data):
        mut = bytearray(data)
        mut[off] ^= x
        tars.append(bytes(mut))
    want = expect(tars, contents=False)
    assert want[0].count(M.E_CORRUPT) == 19659 and want[0].count(M.OK) == 825
    assert run_batch(gpu_ctx, tars, contents=False) == want


def test_filters(gpu_ctx):
    tars = [valid_tars()[k] for k in ("standard-gnu-first", "standard-pax-last", "standard-ustar-absent", "long-gnu", "long-pax", "utf8-pax", "nested-gnu")]
    for prefix, suffix in [(b"pkg-1.0/src/", b""), (b"", b".rs"), (b"pkg-1.0/src/f5", b"3.rs"), (b"", b"/Cargo.toml"), (b"pkg-1.0/" + b"d" * 60, b"notes.txt"),
                           (b"pkg-1.0/" + b"x" * 50, b"Cargo.toml"), (b"no such", b""), (b"", b"z" * 400), (b"pkg-1.0/a.txt", b"pkg-1.0/a.txt")]:
        want = expect(tars, prefix, suffix)
        assert run_batch(gpu_ctx, tars, prefix, suffix) == want, (prefix, suffix)
    assert expect(tars, b"no such")[1][-1] == 0 and expect(tars, b"", b".rs")[1][-1] > 10


def test_caps_one_short_for_the_middle_item(gpu_ctx):
    tars = [make_tar("gnu", [("a/one", b"1" * 700), ("a/two", b"22")]), valid_tars()["standard-gnu-first"], make_tar("gnu", [("c/three", b"3" * 5)])]
    st, first, members, names, out = M.batch(tars)[:5]
    per = [(first[i + 1] - first[i], sum(len(m[4]) for m in members if m[0] == i), sum(m[3] for m in members if m[0] == i)) for i in range(3)]
    for which, key in enumerate(("members_cap", "names_cap", "out_cap")):
        caps = {"members_cap": first[3], "names_cap": len(names), "out_cap": len(out)}
        caps[key] = per[0][which] + per[1][which] - 1
        want = expect(tars, **caps)
        assert want[0] == [0, M.E_DST_SMALL, 0] and want[1] == [0, per[0][0], per[0][0], per[0][0] + per[2][0]]
        assert run_batch(gpu_ctx, tars, **caps) == want, key
    # exact caps hold everything; caps of nothing hold the empty tar alone
    assert run_batch(gpu_ctx, tars, members_cap=first[3], names_cap=len(names), out_cap=len(out)) == expect(tars)
    tars.append(make_tar("gnu", []))
    assert run_batch(gpu_ctx, tars, members_cap=0, names_cap=0, out_cap=0)[0] == [M.E_DST_SMALL] * 3 + [0]


def test_host_validation(gpu_ctx):
    import torch
    from znippy_amd._lib import np_ptr
    ctx = gpu_ctx
    t = make_tar("gnu", [("a", b"A")])
    d = torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda()
    # per item: outside tar_cap, an offset that wraps, 4 GiB
    got = call(ctx, d, [0, 1, (1 << 64) - 8, 0], [len(t), len(t), 16, 0])
    assert got[0] == [0, M.E_INVAL, M.E_INVAL, 0] and got[1] == [0, 1, 1, 1, 1] and got[2][0][4] == b"a"
    got = call(ctx, d, [0, 0], [len(t), 1 << 32], tar_cap=1 << 33, measure=True)
    assert got[0] == [0, M.E_UNSUPPORTED] and got[1] == [0, 1, 1]
    # the call
    off, ln = np.array([0], dtype=np.uint64), np.array([len(t)], dtype=np.uint64)
    first = np.zeros(2, dtype=np.uint64)
    nb, ob = C.c_uint64(), C.c_uint64()
    st = np.zeros(1, dtype=np.int32)
    big = b"x" * (1 << 16)

    def raw(d_tar=C.c_void_p(d.data_ptr()), o=np_ptr(off), l=np_ptr(ln), n=1, prefix=b"", suffix=b"", members=None, m_cap=0, names=None, n_cap=0, out=None,
            o_cap=0, f=np_ptr(first), pnb=C.byref(nb), pob=C.byref(ob)):
        return ctx.L.znippy_tar_list_batch(ctx.h, d_tar, d.numel(), o, l, n, prefix, len(prefix), suffix, len(suffix), members, m_cap, names, n_cap, out, o_cap, f,
                                           pnb, pob, np_ptr(st))

    assert raw() == 0 and first[1] == 1
    assert raw(n=0) == 0 and raw(n=0, d_tar=None, o=None, l=None) == 0
    for bad in (dict(d_tar=None), dict(o=None), dict(l=None), dict(f=None), dict(pnb=None), dict(pob=None), dict(prefix=big), dict(suffix=big), dict(m_cap=1),
                dict(n_cap=1), dict(o_cap=1), dict(names=np_ptr(st), n_cap=4), dict(out=C.c_void_p(d.data_ptr()), o_cap=1)):
        assert raw(**bad) == M.E_INVAL, bad
    assert raw(prefix=big[:-1]) == 0 and first[1] == 0
    # the Python wrapper measures and lists
    st2, first2, members, names, nb2, ob2 = ctx.tar_list_batch(d, [0], [len(t)])
    assert list(st2) == [0] and list(first2) == [0, 1] and names == b"a" and (nb2, ob2) == (1, 1) and int(members[0]["data_off"]) == 512


def test_an_item_across_the_4_gib_line(gpu_ctx):
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip(f"the far region needs 6 GiB of free device memory, {free >> 20} MiB are free")
    region = torch.empty(FAR_LINE + (16 << 20), dtype=torch.uint8, device="cuda")
    try:
        tars = [many(300), valid_tars()["standard-pax-first"], many(65)]
        offs = [FAR_LINE - len(tars[0]) // 2 + 1, FAR_LINE + (1 << 20) + 3, 5]  # across the line, above it, below it
        for t, o in zip(tars, offs):
            region[o:o + len(t)] = torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda()
        got = call(gpu_ctx, region, offs, [len(t) for t in tars])
        assert got == expect(tars)
    finally:
        del region
        torch.cuda.empty_cache()
