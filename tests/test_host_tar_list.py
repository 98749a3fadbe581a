"""znippy_archive_list_tar_members (the compiled host layer): a directory holding a .tar, a .tar.gz, a .crate, a .tar.bz2, a damaged
tar and a text file is archived, and the members of every tar come back from one call — the files gathered on the device, gzip and
bzip2 files decompressed there by their first bytes, one znippy_tar_list_batch over all of them — against `tarfile`, through
ZnippyArchive.list_tar_members and the C function: with and without contents, with a filter, and with a cap that leaves one file out."""
import bz2
import ctypes as C
import gzip
import io
import tarfile

import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_DST_SMALL, E_CORRUPT = 0, -1, -4, -5
FORMATS = {"ustar": tarfile.USTAR_FORMAT, "gnu": tarfile.GNU_FORMAT, "pax": tarfile.PAX_FORMAT}


def make(fmt, members, dirs=()):
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=FORMATS[fmt]) as tf:
        for d in dirs:
            ti = tarfile.TarInfo(d)
            ti.type = tarfile.DIRTYPE
            tf.addfile(ti)
        for name, data in members:
            ti = tarfile.TarInfo(name)
            ti.size = len(data)
            tf.addfile(ti, io.BytesIO(data))
    return b.getvalue()


def files():
    plain = make("gnu", [("plain/a.txt", gen.text(700)), ("plain/" + "d" * 120 + "/b.rs", gen.pseudo_text(40_000, seed=3)), ("plain/empty", b"")], dirs=["plain"])
    sdist = make("pax", [("pkg-2.0/setup.py", gen.text(900)), ("pkg-2.0/café/naïve.py", gen.pseudo_text(5000, seed=4))] +
                 [("pkg-2.0/src/m%d.py" % k, gen.pseudo_text(30_000 + 77 * k, seed=50 + k)) for k in range(6)])
    crate = make("ustar", [("crate-0.1.0/Cargo.toml", b"[package]\nname = \"crate\"\n"), ("crate-0.1.0/src/lib.rs", gen.pseudo_text(12_345, seed=5))])
    old = make("gnu", [("old-1.0/m%d.c" % k, gen.pseudo_text(50_000 + k, seed=60 + k)) for k in range(4)])
    damaged = bytearray(plain)
    damaged[512 + 150] ^= 1  # the checksum field of the second header
    two = gzip.compress(crate[:1024], 6) + gzip.compress(crate[1024:], 6)  # two members: ISIZE names only the last
    return {"t/plain.tar": plain, "t/sdist.tar.gz": gzip.compress(sdist, 6), "t/crate-0.1.0.crate": gzip.compress(crate, 9), "t/two.tgz": two,
            "t/old.tar.bz2": bz2.compress(old, 1), "t/damaged.tar": bytes(damaged), "t/notes.txt": gen.text(3000), "t/empty.tar": b""}


def tars(f):
    return {"t/plain.tar": f["t/plain.tar"], "t/sdist.tar.gz": gzip.decompress(f["t/sdist.tar.gz"]), "t/crate-0.1.0.crate": gzip.decompress(f["t/crate-0.1.0.crate"]),
            "t/two.tgz": gzip.decompress(f["t/two.tgz"]), "t/old.tar.bz2": bz2.decompress(f["t/old.tar.bz2"]), "t/empty.tar": b""}


def expected(f, prefix=b"", suffix=b""):
    """per path: (status, [(name, size, bytes)]) by tarfile"""
    want = {"t/damaged.tar": (E_CORRUPT, []), "t/notes.txt": (E_CORRUPT, []), "t/empty.tar": (OK, [])}
    for p, t in tars(f).items():
        if not t:
            continue
        ms = []
        with tarfile.open(fileobj=io.BytesIO(t), mode="r:") as tf:
            for ti in tf:
                name = ti.name.encode("utf-8", "surrogateescape")
                if ti.isreg() and name.startswith(prefix) and name.endswith(suffix):
                    ms.append((name, ti.size, t[ti.offset_data:ti.offset_data + ti.size]))
        want[p] = (OK, ms)
    return want


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import host
    d = tmp_path_factory.mktemp("host_tar_list")
    for k, v in files().items():
        p = d / "in" / k
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(v)
    out = d / "a.znippy"
    host.compress_dir(d / "in", out)
    a = host.ZnippyArchive.open(out)
    yield a
    a.close()


def test_list_tar_members(archive):
    f = files()
    want = expected(f)
    assert [len(want[p][1]) for p in ("t/plain.tar", "t/sdist.tar.gz", "t/crate-0.1.0.crate", "t/two.tgz", "t/old.tar.bz2")] == [3, 8, 2, 2, 4]
    paths = sorted(f) + ["t/unknown.tar"]
    got = archive.list_tar_members(paths, contents=True)
    for p, g in zip(paths, got):
        assert g == want.get(p, (E_INVAL, [])), (p, g[0])
    # plain tars alone are listed where they were gathered; one compressed file among them moves all into one region
    for sel in (["t/plain.tar", "t/damaged.tar", "t/notes.txt", "t/empty.tar", "t/plain.tar"], ["t/plain.tar", "t/two.tgz", "t/empty.tar", "t/plain.tar"],
                ["t/empty.tar"], ["t/old.tar.bz2", "t/plain.tar"]):
        assert archive.list_tar_members(sel, contents=True) == [want[p] for p in sel], sel
    # without contents
    got = archive.list_tar_members(paths)
    for p, g in zip(paths, got):
        w = want.get(p, (E_INVAL, []))
        assert g == (w[0], [(name, size, None) for name, size, _ in w[1]]), p
    # a filter
    for prefix, suffix in [(b"", b".py"), (b"pkg-2.0/src/", b""), (b"crate-0.1.0/", b"Cargo.toml"), (b"nothing", b"")]:
        wantf = expected(f, prefix, suffix)
        got = archive.list_tar_members(paths, suffix=suffix, prefix=prefix, contents=True)
        for p, g in zip(paths, got):
            assert g == wantf.get(p, (E_INVAL, [])), (prefix, suffix, p)
    assert sum(len(m) for _, m in archive.list_tar_members(paths, suffix=b".py")) == 8
    # a cap one byte short of all the contents: the last file with contents is left out, the ones in front of it are not
    good = [p for p in sorted(f) if want[p][0] == OK]
    total = sum(size for p in good for _, size, _ in want[p][1])
    assert archive.list_tar_members(good, contents=True, cap=total) == [want[p] for p in good]
    got = archive.list_tar_members(good, contents=True, cap=total - 1)
    last = max(k for k, p in enumerate(good) if any(size for _, size, _ in want[p][1]))
    assert [g[0] for g in got] == [E_DST_SMALL if k == last else OK for k in range(len(good))]
    assert [g for k, g in enumerate(got) if k != last] == [want[p] for k, p in enumerate(good) if k != last] and got[last][1] == []
    assert archive.list_tar_members([]) == []


def test_the_c_function(archive):
    from znippy_amd import hip, host
    L = host.lib()
    f = files()
    want = expected(f)
    paths = sorted(f)
    n = len(paths)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    vp = C.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    first = np.full(n + 1, 99, dtype=np.uint64)
    st = np.full(n, 99, dtype=np.int32)
    nb, ob = C.c_uint64(99), C.c_uint64(99)
    # measured
    assert L.znippy_archive_list_tar_members(archive.h, arr, n, None, None, None, 0, None, 0, None, 0, ptr(first), C.byref(nb), C.byref(ob), ptr(st)) == OK
    counts = [len(want[p][1]) for p in paths]
    assert [int(first[k + 1] - first[k]) for k in range(n)] == counts and [int(s) for s in st] == [want[p][0] for p in paths]
    assert nb.value == sum(len(name) for p in paths for name, _, _ in want[p][1]) and ob.value == sum(size for p in paths for _, size, _ in want[p][1])
    # listed, with guard entries and bytes behind what the caps allow
    m_cap, n_cap, o_cap = int(first[n]), nb.value, ob.value
    members = np.frombuffer(b"\xA5" * (hip.TAR_MEMBER.itemsize * (m_cap + 2)), dtype=hip.TAR_MEMBER).copy()
    names = np.full(n_cap + 32, 0xA5, dtype=np.uint8)
    buf = np.full(o_cap + 32, 0xA5, dtype=np.uint8)
    assert L.znippy_archive_list_tar_members(archive.h, arr, n, b"", b"", ptr(members), m_cap, ptr(names), n_cap, ptr(buf), o_cap, ptr(first), C.byref(nb),
                                             C.byref(ob), ptr(st)) == OK
    assert (members[m_cap:].view(np.uint8) == 0xA5).all() and (names[n_cap:] == 0xA5).all() and (buf[o_cap:] == 0xA5).all()
    t = tars(f)
    for k, p in enumerate(paths):
        assert int(st[k]) == want[p][0], p
        ms = members[int(first[k]):int(first[k + 1])]
        assert len(ms) == len(want[p][1])
        for m, (name, size, data) in zip(ms, want[p][1]):
            assert names[int(m["name_off"]):int(m["name_off"]) + int(m["name_len"])].tobytes() == name and int(m["size"]) == size
            assert buf[int(m["out_off"]):int(m["out_off"]) + size].tobytes() == data
            assert t[p][int(m["data_off"]):int(m["data_off"]) + size] == data and int(m["data_off"]) == int(m["header_off"]) + 512
    # the members table one entry short: the last file with members is left out
    assert L.znippy_archive_list_tar_members(archive.h, arr, n, b"", b"", ptr(members), m_cap - 1, ptr(names), n_cap, None, 0, ptr(first), C.byref(nb),
                                             C.byref(ob), ptr(st)) == OK
    last = max(k for k in range(n) if counts[k])
    assert [int(s) for s in st] == [E_DST_SMALL if k == last else want[p][0] for k, p in enumerate(paths)] and int(first[n]) == m_cap - counts[last]
    # the status array is optional; NULL required arguments are refused
    a = (archive.h, arr, n, b"", b"", ptr(members), m_cap, ptr(names), n_cap, ptr(buf), o_cap, ptr(first), C.byref(nb), C.byref(ob), None)
    assert L.znippy_archive_list_tar_members(*a) == OK
    for k in (0, 1, 11, 12, 13):
        bad = list(a)
        bad[k] = None
        assert L.znippy_archive_list_tar_members(*bad) == E_INVAL, k
    for k in (5, 7, 9):  # a cap without its buffer
        bad = list(a)
        bad[k] = None
        assert L.znippy_archive_list_tar_members(*bad) == E_INVAL, k
