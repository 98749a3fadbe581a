"""znippy_targz_find_batch: one member of gzip-compressed tars found and extracted on the device, against the model of
tests/targz_model.py — zlib fed one byte at a time gives the prefix of the tar that the input determines, the tar walk (pinned to
`tarfile` and to the C++ walker by tests/test_tar_rules_cpu.py) runs on it.  One batch per test."""
import ctypes as C
import io
import tarfile
import zlib

import numpy as np
import pytest

import gen
import targz_model as M
from test_tar_rules_cpu import make_tar
from targz_checks import GUARD, SCAN, check, gz, run_batch, valid_tars

pytestmark = pytest.mark.gpu


# ---- 1. valid streams ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_valid_streams(gpu_ctx, level):
    items = [gz(t, level, name="pkg-1.0.crate" if i & 1 else None) for i, t in enumerate(valid_tars())]
    want, status, scanned = check(gpu_ctx, items, b"/Cargo.toml")
    assert status.count(0) >= 11 and status.count(M.E_NOENT) >= 4, status
    # other filters on the same files: a prefix only; a name behind a long-name entry; nothing matches
    check(gpu_ctx, items, b"", prefix=b"pkg-1.0/src/f51")
    check(gpu_ctx, items, b"z.txt")
    want, status, _ = check(gpu_ctx, items, b"/no-such-member")
    assert set(status) == {M.E_NOENT}


def test_early_stop(gpu_ctx):
    # the answer lies in front of 300 KB of text: the walk stops behind the member, not at the end of the stream
    tar = make_tar("gnu", [("pkg-1.0/.cargo_vcs_info.json", b"{}" * 40), ("pkg-1.0/Cargo.toml", b"[package]\n" * 30), ("pkg-1.0/src/lib.rs", gen.pseudo_text(300_000, seed=3))])
    want, status, scanned = check(gpu_ctx, [gz(tar, 6)], b"/Cargo.toml")
    assert status == [0] and scanned[0] < 4096, scanned


# ---- 2. every cut of one stream ------------------------------------------------------------------------------------------------

def fixture_tar():
    return make_tar("gnu", [("pkg-1.0/.cargo_vcs_info.json", (b'{"git":{"sha1":"%040x"},"path_in_vcs":""}' % 7).ljust(80)[:80]),
                            ("pkg-1.0/Cargo.toml", (b"[package]\nname = \"pkg\"\nversion = \"1.0.0\"\n" + gen.pseudo_text(300, seed=9))[:300]),
                            ("pkg-1.0/src/lib.rs", gen.pseudo_text(2000, seed=11))])


def fixture():
    return gz(fixture_tar(), 6)


def test_every_cut(gpu_ctx):
    tar = make_tar("gnu", [("pkg-1.0/.cargo_vcs_info.json", b"{}".ljust(80)), ("pkg-1.0/Cargo.toml", gen.pseudo_text(300, seed=9)),
                           ("pkg-1.0/src/lib.rs", gen.pseudo_text(700, seed=11))])
    full = gz(tar, 6)
    assert 500 <= len(full) <= 1000, len(full)
    items = [full[:k] for k in range(len(full) + 1)]
    for whole in (0, 1):
        want, status, _ = check(gpu_ctx, items, b"/Cargo.toml", whole=[whole] * len(items))
        other = M.E_CORRUPT if whole else M.E_MORE
        assert set(status) == {0, other}
        first_ok = status.index(0)
        assert status[:first_ok] == [other] * first_ok and status[first_ok:] == [0] * (len(items) - first_ok)   # one switch, where the model names it
    # a file without the member whose tar ends behind its last member's block, with no zero blocks: the end of the stream is the
    # answer only when a following gzip member could have been seen
    none = gz(make_tar("gnu", [("pkg-1.0/README", b"nothing")])[:1024], 6)
    items = [none[:k] for k in range(len(none) - 12, len(none) + 1)] + [none + bytes(k) for k in (1, 9, 10, 30)]
    want, status, _ = check(gpu_ctx, items, b"/Cargo.toml", whole=[0] * len(items))
    assert status[-2:] == [M.E_NOENT] * 2 and status[-5:-2] == [M.E_MORE] * 3, status
    want, status, _ = check(gpu_ctx, items, b"/Cargo.toml", whole=[1] * len(items))
    assert status[-5:] == [M.E_NOENT] * 5, status


# ---- 3. scan_cap and out_cap ---------------------------------------------------------------------------------------------------

def test_scan_cap_and_out_cap(gpu_ctx):
    tar = fixture_tar()
    with tarfile.open(fileobj=io.BytesIO(tar)) as tf:
        ti = tf.getmember("pkg-1.0/Cargo.toml")
        end = ti.offset_data + ti.size
        want = tf.extractfile(ti).read()
    for level in (0, 6):
        src = gz(tar, level)
        status, got, _ = run_batch(gpu_ctx, [src], b"/Cargo.toml", scan_cap=end)
        assert status == [0] and got == [want]
        assert M.find(src, 1, b"", b"/Cargo.toml", end)[0] == 0
        status, got, _ = run_batch(gpu_ctx, [src], b"/Cargo.toml", scan_cap=end - 1)
        assert status == [M.E_DST_SMALL] == [M.find(src, 1, b"", b"/Cargo.toml", end - 1)[0]]
        # a cap in front of the member's header: the item ends when the walk asks for the header
        status, got, scanned = run_batch(gpu_ctx, [src], b"/Cargo.toml", scan_cap=1024)
        assert status == [M.E_DST_SMALL] and scanned[0] <= 1024
    # out_cap fits all but the second member: it takes no room and the third follows the first
    src = gz(tar, 6)
    lib = gz(make_tar("gnu", [("pkg-1.0/Cargo.toml", b"x" * 301)]), 6)
    status, got, _ = run_batch(gpu_ctx, [src, lib, src], b"/Cargo.toml", out_cap=600)
    assert status == [0, M.E_DST_SMALL, 0] and got == [want, b"", want]
    status, got, _ = run_batch(gpu_ctx, [src, src], b"/Cargo.toml", out_cap=0)
    assert status == [M.E_DST_SMALL] * 2


# ---- 4. other inputs -----------------------------------------------------------------------------------------------------------

def test_two_members_and_bad_headers(gpu_ctx):
    a, b = make_tar("gnu", [("pkg-1.0/README", b"first member")]), make_tar("gnu", [("pkg-1.0/Cargo.toml", b"second member")])
    two = gz(a[:1024], 6) + gz(a[1024:] + b, 6)          # a tar split over two gzip members, as `cat a.gz b.gz` makes
    items = [two, gz(b, 6) + gz(a, 6), b"PK\x03\x04" + bytes(60), b"\x1f\x8b\x07" + bytes(60), b"\x1f\x8b\x08\xe0" + bytes(60), b"", b"\x1f\x8b\x08\x08" + b"n" * 40,
             gz(b, 6, name="a-file-name.crate")]
    want, status, _ = check(gpu_ctx, items, b"/Cargo.toml")
    assert status == [M.E_UNSUPPORTED, 0, M.E_CORRUPT, M.E_UNSUPPORTED, M.E_UNSUPPORTED, M.E_CORRUPT, M.E_CORRUPT, 0], status
    want, status, _ = check(gpu_ctx, items, b"/Cargo.toml", whole=[0] * len(items))
    assert status[5] == status[6] == M.E_MORE


def test_host_validation_and_call_rules(gpu_ctx):
    import torch
    from znippy_amd import _lib
    L = _lib.lib()
    s = fixture()
    d_src = torch.from_numpy(np.frombuffer(bytes(7) + s, np.uint8).copy()).cuda()
    d_out = torch.full((4096,), GUARD, dtype=torch.uint8, device="cuda")
    big = (1 << 64) - 4
    status, off, ln, scanned = gpu_ctx.targz_find_batch(d_src, [7, 7, big, 7], [len(s), len(s) + 1, 8, len(s)], d_out, b"/Cargo.toml")
    assert list(status) == [0, M.E_INVAL, M.E_INVAL, 0] and list(off) == [0, 0, 0, 300] and list(ln) == [300, 0, 0, 300]
    img = d_out.cpu().numpy()
    assert img[:300].tobytes() == img[300:600].tobytes() and (img[600:] == GUARD).all()
    # a source of 4 GiB or more is refused before any kernel (the region only has to be declared that big)
    status, off, ln, _ = gpu_ctx.targz_find_batch(d_src, [0, 7], [1 << 32, len(s)], d_out, b"/Cargo.toml", src_cap=1 << 33)
    assert list(status) == [M.E_UNSUPPORTED, 0] and list(ln) == [0, 300]
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)   # noqa: E731
    st = (C.c_int32 * 1)(99)
    oo, ol = u64(9), u64(9)
    sp, op = C.c_void_p(d_src.data_ptr()), C.c_void_p(d_out.data_ptr())

    def call(h, dsrc, so, sl, n, scan=SCAN, suffix=b"/Cargo.toml", oo=oo, ol=ol):
        return L.znippy_targz_find_batch(h, dsrc, d_src.numel(), so, sl, None, n, b"", 0, suffix, len(suffix) if suffix else 11, scan, op, d_out.numel(), oo, ol, st, None)
    assert call(gpu_ctx.h, None, None, None, 0) == 0                                     # n == 0
    assert call(gpu_ctx.h, sp, u64(7), u64(len(s)), 1) == 0 and st[0] == 0 and (oo[0], ol[0]) == (0, 300)
    assert call(gpu_ctx.h, sp, u64(7), u64(len(s)), 1, scan=511) == M.E_INVAL            # scan_cap below one header
    assert call(gpu_ctx.h, sp, u64(7), u64(len(s)), 1, scan=512) == 0 and st[0] == M.E_DST_SMALL
    for args in [(None, u64(7), u64(len(s))), (sp, None, u64(len(s))), (sp, u64(7), None)]:
        assert call(gpu_ctx.h, *args, 1) == M.E_INVAL
    assert call(gpu_ctx.h, sp, u64(7), u64(len(s)), 1, suffix=None) == M.E_INVAL
    assert call(gpu_ctx.h, sp, u64(7), u64(len(s)), 1, oo=None) == M.E_INVAL and call(gpu_ctx.h, sp, u64(7), u64(len(s)), 1, ol=None) == M.E_INVAL
    assert call(None, sp, u64(7), u64(len(s)), 1) == M.E_INVAL
    assert call(gpu_ctx.h, sp, u64(7), u64(len(s)), (1 << 32) - 16) == M.E_INVAL
    # a batch whose scratch would pass 16 GiB is refused with nothing queued
    n = 20
    assert L.znippy_targz_find_batch(gpu_ctx.h, sp, 1 << 40, u64(*[0] * n), u64(*[1 << 30] * n), None, n, b"", 0, b"x", 1, 1 << 30, op, d_out.numel(),
                                     u64(*[0] * n), u64(*[0] * n), None, None) == M.E_NOMEM
    torch.cuda.synchronize()


def test_not_a_run_and_kernel_times(gpu_ctx, oracle):
    from test_gpu_ranges import own_frames, sentinel, table_of
    rows = [gen.pseudo_text(300_001, seed=51), gen.incompressible(9, 70_000), gen.text(10_240)]
    comp = [1, 0, 1]
    frames = [f if c else r for f, r, c in zip(own_frames(19, rows), rows, comp)]
    ck = np.stack([np.frombuffer(oracle.blake3(r), np.uint8) for r in rows])
    ck[2] ^= 1                                                  # one mismatch, so that the corrupt list has an entry
    total = sum(len(r) for r in rows)
    items = [fixture(), gz(make_tar("gnu", [("pkg-1.0/README", b"no manifest")]), 6)]

    def sequence(mixed_in):
        rt, d_blobs, _ = table_of(gpu_ctx, frames, rows, comp=comp, checksum=ck)
        out = sentinel(total + 64)
        rt.decode_verify_async(d_blobs, out)
        if mixed_in:
            status, got, _ = run_batch(gpu_ctx, items, b"/Cargo.toml")
            assert status == [0, M.E_NOENT] and len(got[0]) == 300
            names = [k for k, _ in gpu_ctx.kernel_times()]
            assert names == ["targz_find", "targz_gather"], names
        counters, corrupt, status = rt.results()
        res = (counters, list(corrupt), status.copy(), rt.digests().copy(), out.cpu().numpy())
        rt.close()
        return res
    plain, mixed = sequence(False), sequence(True)
    assert plain[0]["corrupt_rows"] == 1 and plain[1] == [2]
    for k, (x, y) in enumerate(zip(plain, mixed)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, k


# ---- 5. damage -----------------------------------------------------------------------------------------------------------------

def cpu_walker(tar, suffix):
    """the C++ walker (host/tar_walk.cc, compiled into the library) on the whole tar"""
    from znippy_amd import _lib
    L = _lib.lib()
    L.znippy_tar_find_member.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64] + [C.POINTER(C.c_uint64)] * 3
    off, size, need = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = L.znippy_tar_find_member(tar, len(tar), 1, b"", 0, suffix, len(suffix), C.byref(off), C.byref(size), C.byref(need))
    return rc, tar[off.value:off.value + size.value] if rc == 0 else b""


def test_tar_level_damage(gpu_ctx):
    """single-byte mutants of the three headers, made before compression: the DEFLATE stream stays valid"""
    tar = fixture_tar()
    headers = (0, 1024, 2048)
    assert all(tar[h + 257:h + 262] == b"ustar" for h in headers)
    rng = np.random.default_rng(5)
    muts = []
    for h in headers:
        for k in range(512):
            m = bytearray(tar)
            m[h + k] ^= int(rng.integers(1, 256)) if k % 7 else 0xFF
            muts.append(bytes(m))
    # a single byte changed and the checksum made to fit again: the type of the wanted member's header (a sparse member; a directory,
    # whose data is then read as a header; a long name for the member behind it; an unknown type), its name
    for at, value in [(1024 + 156, b"S"), (1024 + 156, b"5"), (1024 + 156, b"L"), (1024 + 156, b"Z"), (1024 + 8, b"X")]:
        m = bytearray(tar)
        m[at:at + 1] = value
        m[1024 + 148:1024 + 156] = b"        "
        m[1024 + 148:1024 + 156] = b"%06o\0 " % sum(m[1024:1536])
        muts.append(bytes(m))
    items = [gz(m, 1) for m in muts]
    status, got, _ = run_batch(gpu_ctx, items, b"/Cargo.toml")
    want = [cpu_walker(m, b"/Cargo.toml") for m in muts]
    assert [(s, g) for s, g in zip(status, got)] == want
    assert status[-5:] == [M.E_UNSUPPORTED, M.E_CORRUPT, M.E_NOENT, M.E_NOENT, M.E_NOENT] and 0 in status and M.E_CORRUPT in status, status[-5:]


def flip_fixture(lib_bytes, strategy):
    """The fixture of the bit-flip tests: .cargo_vcs_info.json (80 B), Cargo.toml (300 B) and src/lib.rs of word soup in a GNU-format
    tar, at level 6, as a gzip member."""
    tar = make_tar("gnu", [("pkg-1.0/.cargo_vcs_info.json", (b'{"git":{"sha1":"%040x"},"path_in_vcs":""}' % 7).ljust(80)[:80]),
                           ("pkg-1.0/Cargo.toml", (b"[package]\nname = \"pkg\"\nversion = \"1.0.0\"\n" + gen.pseudo_text(300, seed=9))[:300]),
                           ("pkg-1.0/src/lib.rs", gen.pseudo_text(lib_bytes, seed=11))])
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strategy)
    return b"\x1f\x8b\x08\0\0\0\0\0\x02\xff" + c.compress(tar) + c.flush() + zlib.crc32(tar).to_bytes(4, "little") + (len(tar) & 0xFFFFFFFF).to_bytes(4, "little")


def flip_mutants(src, at):
    """every single-bit flip of the DEFLATE bytes of src: (files, what zlib fed one byte at a time makes of each: M.inflate_prefix).
    A mutant that zlib accepts to the end of its input gives the same prefix however it is fed, so it is fed at once from a saved
    state in front of the flip; only a refused one is fed again byte by byte."""
    body, n = src[at:], len(src) - at - 8
    step = 64
    states, outs, d, out = [], [], zlib.decompressobj(-15), []
    for c in range(0, n, step):
        states.append(d.copy())
        outs.append(b"".join(out))
        out.append(d.decompress(body[c:c + step]))
    items, infl = [], []
    for k in range(n):
        c = k // step
        for bit in range(8):
            m = bytearray(body)
            m[k] ^= 1 << bit
            m = bytes(m)
            d = states[c].copy()
            try:
                P = outs[c] + d.decompress(m[c * step:])
                res = (P, "end", d.unused_data) if d.eof else (P, "input", b"")
            except zlib.error:
                d, out = states[c].copy(), [outs[c]]
                res = None
                for i in range(c * step, len(m)):
                    try:
                        out.append(d.decompress(m[i:i + 1]))
                    except zlib.error:
                        res = (b"".join(out), "error", b"")
                        break
                assert res is not None
            items.append(src[:at] + m)
            infl.append(res)
    return items, infl


def flips_against_the_model(ctx, src):
    """(mutants, those of the loose class, those of the loose class that give the model's answer all the same)"""
    st, at = M.gzip_header(src)
    assert st == 0 and at == 10
    items, infl = flip_mutants(src, at)
    scan = 64 << 10   # (a flipped stream may inflate to anything: the scratch of the batch stays small)
    status, got, _ = run_batch(ctx, items, b"/Cargo.toml", scan_cap=scan, out_cap=len(items) * 300 + 4096)
    loose = agree = 0
    for i, (s, g, (P, why, tail)) in enumerate(zip(status, got, infl)):
        want = M.find(items[i], 1, b"", b"/Cargo.toml", scan, inflated=(P, why, tail))
        if why != "error":
            assert (s, g) == want[:2], (i, why, s, want[0])
            continue
        cap = M.item_cap(len(items[i]), scan)
        wst, _, _, need = M.walk(P[:cap], False, b"", b"/Cargo.toml")
        if wst != M.E_MORE or need > cap:
            assert (s, g) == want[:2], (i, "verdict inside the prefix", s, want[0])
        elif need - len(P) > 1032:
            assert s == M.E_CORRUPT, (i, s, need, len(P))
        else:
            loose += 1
            agree += (s, g) == want[:2]
    print(f"{loose} of {len(items)} mutants end within 1,032 bytes of the walk's need ({100 * loose / len(items):.2f} %); {agree} of them give the model's answer")
    return len(items), loose, agree


def test_every_single_bit_flip_of_the_stream(gpu_ctx):
    """Every single-bit flip of the DEFLATE bytes of the fixture, in one batch.  Against the model: exactly its answer where zlib accepts
    the mutant whole, or where it rejects it behind the walk's verdict; ZNIPPY_E_CORRUPT where zlib rejects it and the walk still wants
    more than 1,032 bytes beyond the prefix (one input byte completes at most four 258-byte matches); any status in between, which
    may be no more than 2 % of the mutants.  No mutant writes outside its scratch and destination: the guard bytes are checked.

    The fixture.  The loose class is the flips in front of the answer that zlib refuses at once — the walk's need is then a header or
    the 300-byte member away, never 1,032 bytes.  Counted with the model alone: a gzip level-6 stream of the tar with 2,000 bytes of
    lib.rs opens with a dynamic block whose description refuses nearly every flip, 840 of 6,840 mutants (12.3 %); with the fixed codes
    (Z_FIXED, still level 6) 491 of 8,128 (6.0 %), and the 491 do not grow with the file.  So lib.rs has 12,000 bytes here and the
    stream uses the fixed codes: 491 of 28,672 (1.7 %).  The dynamic stream is the next test's."""
    n, loose, _ = flips_against_the_model(gpu_ctx, flip_fixture(12000, zlib.Z_FIXED))
    assert 25000 <= n <= 32000, n
    assert loose <= 0.02 * n, (loose, n)


def test_every_single_bit_flip_of_a_dynamic_block(gpu_ctx):
    """The same comparison on the stream gzip itself makes of the small fixture (one dynamic block), where flips of the block's
    description are refused at once: the three exact classes and the guard bytes are asserted; the share of the loose class (12.3 %
    by the model alone) is what the fixture of the test above was changed for, and is printed, not bounded."""
    src = flip_fixture(2000, zlib.Z_DEFAULT_STRATEGY)
    assert src[10:] == fixture()[10:]
    n, loose, _ = flips_against_the_model(gpu_ctx, src)
    assert 5000 <= n <= 8000, n
