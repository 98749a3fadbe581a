"""znippy_archive_bunzip2_files (the compiled host layer): a directory holding .bz2 and .tar.bz2 files and an unrelated file is
archived, and the whole content of every bzip2 file comes back from one batch — the files gathered on the device, their rooms from a
measuring pass, znippy_bunzip2_batch on them there — against bz2.decompress, through ZnippyArchive.bunzip2_files and the C function."""
import bz2
import ctypes as C
import io
import tarfile

import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_DST_SMALL, E_CORRUPT, E_CHECKSUM = 0, -1, -4, -5, -7


def files():
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=tarfile.GNU_FORMAT) as tf:
        for k in range(4):
            data = gen.pseudo_text(60_000 + 777 * k, seed=40 + k)
            ti = tarfile.TarInfo(f"pkg-1.0/src/m{k}.py")
            ti.size = len(data)
            tf.addfile(ti, io.BytesIO(data))
    plain = bz2.compress(gen.pseudo_text(50_000, seed=31), 9)
    damaged = bytearray(plain)
    damaged[12] ^= 0x40                                        # the block CRC
    return {"logs/access.log.bz2": plain, "logs/rotated.bz2": bz2.compress(gen.text(4000), 1) + bz2.compress(b"") + bz2.compress(gen.binary(3000), 5),
            "sdist/pkg-1.0.tar.bz2": bz2.compress(b.getvalue(), 1), "sdist/old.tbz2": bz2.compress(bytes(300_000), 9), "logs/empty.bz2": bz2.compress(b""),
            "logs/damaged.bz2": bytes(damaged), "logs/notes.txt": gen.text(3000)}


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import host
    d = tmp_path_factory.mktemp("host_bunzip2")
    for k, v in files().items():
        p = d / "in" / k
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(v)
    out = d / "a.znippy"
    host.compress_dir(d / "in", out)
    rows = host.read_index(out)[0]
    assert not any(r["compressed"] for r in rows if r["relative_path"].endswith(".bz2")), "bzip2 files are stored rows"
    a = host.ZnippyArchive.open(out)
    yield a
    a.close()


def expected(f):
    want = {k: (OK, bz2.decompress(v)) for k, v in f.items() if k not in ("logs/damaged.bz2", "logs/notes.txt")}
    want["logs/damaged.bz2"] = (E_CHECKSUM, None)
    want["logs/notes.txt"] = (E_CORRUPT, None)
    return want


def test_bunzip2_files(archive):
    f = files()
    want = expected(f)
    assert len(want["logs/rotated.bz2"][1]) == 7000 and want["logs/empty.bz2"][1] == b"" and len(want["sdist/pkg-1.0.tar.bz2"][1]) > 240_000
    paths = sorted(f) + ["logs/unknown.bz2"]
    got, st = archive.bunzip2_files(paths)
    for p, g, s in zip(paths, got, st):
        assert (s, g) == want.get(p, (E_INVAL, None)), (p, s)
    assert st.count(OK) == 5
    # the result buffer one byte short of the last content: that file is left out, the ones in front of it are not
    good = [p for p in sorted(f) if want[p][0] == OK]
    total = sum(len(want[p][1]) for p in good)
    got, st = archive.bunzip2_files(good, cap=total)
    assert st == [OK] * 5 and got == [want[p][1] for p in good]
    got, st = archive.bunzip2_files(good, cap=total - 1)
    assert st == [OK] * 4 + [E_DST_SMALL] and got[:4] == [want[p][1] for p in good[:4]] and got[4] is None
    assert archive.bunzip2_files([]) == ([], [])


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
    assert L.znippy_archive_bunzip2_files(archive.h, arr, n, buf.ctypes.data_as(vp), cap, off.ctypes.data_as(vp), st.ctypes.data_as(vp)) == OK
    for k, p in enumerate(paths):
        assert int(st[k]) == want[p][0], (p, st[k])
        piece = buf[int(off[k]):int(off[k + 1])].tobytes()
        assert piece == (want[p][1] if want[p][0] == OK else b""), p
    # without a buffer: the sizes alone (no CRC is looked at, so the damaged file counts)
    sizes = np.zeros(n + 1, dtype=np.uint64)
    assert L.znippy_archive_bunzip2_files(archive.h, arr, n, None, 0, sizes.ctypes.data_as(vp), st.ctypes.data_as(vp)) == OK
    lens = [int(sizes[k + 1] - sizes[k]) for k in range(n)]
    assert lens == [len(bz2.decompress(f[p])) if p != "logs/notes.txt" and p != "logs/damaged.bz2" else (50_000 if p == "logs/damaged.bz2" else 0) for p in paths]
    # the status array is optional; NULL required arguments are refused
    assert L.znippy_archive_bunzip2_files(archive.h, arr, n, buf.ctypes.data_as(vp), cap, off.ctypes.data_as(vp), None) == OK
    assert L.znippy_archive_bunzip2_files(archive.h, arr, n, buf.ctypes.data_as(vp), cap, None, st.ctypes.data_as(vp)) == E_INVAL
    assert L.znippy_archive_bunzip2_files(archive.h, None, n, buf.ctypes.data_as(vp), cap, off.ctypes.data_as(vp), st.ctypes.data_as(vp)) == E_INVAL
    assert L.znippy_archive_bunzip2_files(None, arr, n, buf.ctypes.data_as(vp), cap, off.ctypes.data_as(vp), st.ctypes.data_as(vp)) == E_INVAL
    assert L.znippy_archive_bunzip2_files(archive.h, arr, n, None, cap, off.ctypes.data_as(vp), st.ctypes.data_as(vp)) == E_INVAL
