"""znippy_archive_unxz_files and the xz path of znippy_archive_list_tar_members (the compiled host layer): a directory holding a .xz,
a two-block .tar.xz, a .txz and an unrelated file is archived; the whole content of every xz file comes back from one batch — the
files gathered on the device, their rooms from the sizes their indexes claim, znippy_unxz_batch on them there — against
lzma.decompress, and the members of the tars inside against tarfile."""
import ctypes as C
import io
import lzma
import tarfile

import numpy as np
import pytest

import gen
import xz_build as X

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_DST_SMALL, E_CORRUPT, E_CHECKSUM = 0, -1, -4, -5, -7


def tar_of(n, seed):
    b = io.BytesIO()
    members = []
    with tarfile.open(fileobj=b, mode="w", format=tarfile.GNU_FORMAT) as tf:
        for k in range(n):
            data = gen.pseudo_text(20_000 + 777 * k, seed=seed + k)
            ti = tarfile.TarInfo(f"pkg-1.0/src/m{k}.py")
            ti.size = len(data)
            tf.addfile(ti, io.BytesIO(data))
            members.append((ti.name.encode(), len(data), data))
    return b.getvalue(), members


def files():
    t1, _ = tar_of(4, 40)
    t2, _ = tar_of(2, 50)
    text = gen.pseudo_text(50_000, seed=31)
    plain = lzma.compress(text)
    damaged = X.stream([X.Block(text, X.CHECK_CRC64, check_bytes=bytes(8))], X.CHECK_CRC64)   # a check field that differs
    half = len(t1) // 2 + 5
    return {"data/log.xz": plain, "data/two.xz": lzma.compress(gen.text(4000), check=lzma.CHECK_CRC32) + lzma.compress(b"") + lzma.compress(gen.binary(3000)),
            "dist/pkg-1.0.tar.xz": X.xz([t1[:half], t1[half:]], check=X.CHECK_CRC32), "dist/pkg-0.9.txz": lzma.compress(t2), "data/empty.xz": lzma.compress(b""),
            "data/damaged.xz": bytes(damaged), "data/notes.txt": gen.text(3000)}


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import host
    d = tmp_path_factory.mktemp("host_unxz")
    for k, v in files().items():
        p = d / "in" / k
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(v)
    out = d / "a.znippy"
    host.compress_dir(d / "in", out)
    rows = host.read_index(out)[0]
    assert not any(r["compressed"] for r in rows if r["relative_path"].endswith("xz")), "xz files are stored rows"
    a = host.ZnippyArchive.open(out)
    yield a
    a.close()


def expected(f):
    want = {k: (OK, lzma.decompress(v)) for k, v in f.items() if k not in ("data/damaged.xz", "data/notes.txt")}
    want["data/damaged.xz"] = (E_CHECKSUM, None)
    want["data/notes.txt"] = (E_CORRUPT, None)
    return want


def test_unxz_files(archive):
    f = files()
    want = expected(f)
    assert len(want["data/two.xz"][1]) == 7000 and want["data/empty.xz"][1] == b"" and len(want["dist/pkg-1.0.tar.xz"][1]) > 80_000
    with pytest.raises(lzma.LZMAError):
        lzma.decompress(f["data/damaged.xz"])
    paths = sorted(f) + ["data/unknown.xz"]
    got, st = archive.unxz_files(paths)
    for p, g, s in zip(paths, got, st):
        assert (s, g) == want.get(p, (E_INVAL, None)), (p, s)
    assert st.count(OK) == 5
    # the result buffer one byte short of the last content: that file is left out, the ones in front of it are not
    good = [p for p in sorted(f) if want[p][0] == OK]
    total = sum(len(want[p][1]) for p in good)
    got, st = archive.unxz_files(good, cap=total)
    assert st == [OK] * 5 and got == [want[p][1] for p in good]
    got, st = archive.unxz_files(good, cap=total - 1)
    assert st == [OK] * 4 + [E_DST_SMALL] and got[:4] == [want[p][1] for p in good[:4]] and got[4] is None
    assert archive.unxz_files([]) == ([], [])


def test_list_tar_members_of_xz_tarballs(archive):
    _, m1 = tar_of(4, 40)
    _, m2 = tar_of(2, 50)
    got = archive.list_tar_members(["dist/pkg-1.0.tar.xz", "data/log.xz", "dist/pkg-0.9.txz", "data/damaged.xz"], contents=True)
    assert got[0] == (OK, m1) and got[2] == (OK, m2)
    assert got[1][0] == E_CORRUPT and got[1][1] == []      # an xz file that holds no tar
    assert got[3] == (E_CHECKSUM, [])
    got = archive.list_tar_members(["dist/pkg-0.9.txz", "dist/pkg-1.0.tar.xz"], suffix=b"m1.py")
    assert got == [(OK, [(m2[1][0], m2[1][1], None)]), (OK, [(m1[1][0], m1[1][1], None)])]


def test_the_c_function(archive):
    from znippy_amd import host
    L = host.lib()
    f = files()
    want = expected(f)
    paths = sorted(f)
    n = len(paths)
    arr = (C.c_char_p * n)(*[p.encode() for p in paths])
    cap = 1 << 20
    buf = np.empty(cap, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    st = np.full(n, 99, dtype=np.int32)
    vp = C.c_void_p
    assert L.znippy_archive_unxz_files(archive.h, arr, n, buf.ctypes.data_as(vp), cap, off.ctypes.data_as(vp), st.ctypes.data_as(vp)) == OK
    for k, p in enumerate(paths):
        assert int(st[k]) == want[p][0], (p, st[k])
        piece = buf[int(off[k]):int(off[k + 1])].tobytes()
        assert piece == (want[p][1] if want[p][0] == OK else b""), p
    # without a buffer: the sizes the indexes claim (no block is read, so the damaged file counts)
    sizes = np.zeros(n + 1, dtype=np.uint64)
    assert L.znippy_archive_unxz_files(archive.h, arr, n, None, 0, sizes.ctypes.data_as(vp), st.ctypes.data_as(vp)) == OK
    lens = [int(sizes[k + 1] - sizes[k]) for k in range(n)]
    assert lens == [50_000 if p == "data/damaged.xz" else 0 if p == "data/notes.txt" else len(want[p][1]) for p in paths]
    # the status array is optional; NULL required arguments are refused
    assert L.znippy_archive_unxz_files(archive.h, arr, n, buf.ctypes.data_as(vp), cap, off.ctypes.data_as(vp), None) == OK
    assert L.znippy_archive_unxz_files(archive.h, arr, n, buf.ctypes.data_as(vp), cap, None, st.ctypes.data_as(vp)) == E_INVAL
    assert L.znippy_archive_unxz_files(archive.h, None, n, buf.ctypes.data_as(vp), cap, off.ctypes.data_as(vp), st.ctypes.data_as(vp)) == E_INVAL
    assert L.znippy_archive_unxz_files(None, arr, n, buf.ctypes.data_as(vp), cap, off.ctypes.data_as(vp), st.ctypes.data_as(vp)) == E_INVAL
    assert L.znippy_archive_unxz_files(archive.h, arr, n, None, cap, off.ctypes.data_as(vp), st.ctypes.data_as(vp)) == E_INVAL
