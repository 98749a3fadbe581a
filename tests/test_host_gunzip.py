"""znippy_archive_gunzip_files (the compiled host layer): the whole content of every archived gzip file in one batch — the files
gathered on the device, their rooms from ISIZE, znippy_gunzip_batch on them there, the files of several members once more with a
larger room — against gzip.decompress, through ZnippyArchive.gunzip_files and through the C function."""
import ctypes as C
import gzip
import io
import tarfile
import zlib

import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_DST_SMALL, E_CORRUPT, E_CHECKSUM = 0, -1, -4, -5, -7


def files():
    plain = gzip.compress(gen.pseudo_text(50_000, seed=31), 6, mtime=0)
    # ISIZE names the last member only (100 bytes): the first room is too small by far
    multi = b"".join(gzip.compress(gen.pseudo_text(n, seed=n), 6, mtime=0) for n in (40_000, 0, 30_000, 100))
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=tarfile.GNU_FORMAT) as tf:
        for k in range(4):
            data = gen.pseudo_text(30_000 + 777 * k, seed=40 + k)
            ti = tarfile.TarInfo(f"pkg-1.0/src/m{k}.py")
            ti.size = len(data)
            tf.addfile(ti, io.BytesIO(data))
    tar = b.getvalue()
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    flushed = b"".join(c.compress(tar[at:at + 32_768]) + c.flush(zlib.Z_FULL_FLUSH) for at in range(0, len(tar), 32_768)) + c.flush()
    damaged = bytearray(plain)
    damaged[-6] ^= 0x40                                        # the CRC-32
    return {"logs/access.log.gz": plain, "logs/rotated.gz": multi, "sdist/pkg-1.0.tar.gz": flushed, "logs/empty.gz": gzip.compress(b"", 6, mtime=0),
            "logs/damaged.gz": bytes(damaged), "logs/notes.gz": gen.text(3000)}


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import host
    from znippy_amd.stream_packer import ArchiveEntry
    p = tmp_path_factory.mktemp("host_gunzip") / "a.znippy"
    c = host.compress_stream(str(p), False)
    for k, v in files().items():
        c.send(ArchiveEntry(k, v))
    c.finish()
    rows = host.read_index(p)[0]
    assert not any(r["compressed"] for r in rows if r["relative_path"].endswith(".gz")), "gzip files are stored rows"
    a = host.ZnippyArchive.open(p)
    yield a
    a.close()


def expected(f):
    want = {k: (OK, gzip.decompress(v)) for k, v in f.items() if k not in ("logs/damaged.gz", "logs/notes.gz")}
    want["logs/damaged.gz"] = (E_CHECKSUM, None)
    want["logs/notes.gz"] = (E_CORRUPT, None)
    return want


def test_gunzip_files(archive):
    f = files()
    want = expected(f)
    assert len(want["logs/rotated.gz"][1]) == 70_100 and want["logs/empty.gz"][1] == b""
    paths = sorted(f) + ["logs/unknown.gz"]
    got, st = archive.gunzip_files(paths)
    for p, g, s in zip(paths, got, st):
        assert (s, g) == want.get(p, (E_INVAL, None)), (p, s)
    assert st.count(OK) == 4
    # the result buffer one byte short of the last content: that file is left out, the ones in front of it are not
    good = [p for p in sorted(f) if want[p][0] == OK]
    total = sum(len(want[p][1]) for p in good)
    got, st = archive.gunzip_files(good, cap=total)
    assert st == [OK] * 4 and got == [want[p][1] for p in good]
    got, st = archive.gunzip_files(good, cap=total - 1)
    assert st == [OK] * 3 + [E_DST_SMALL] and got[:3] == [want[p][1] for p in good[:3]] and got[3] is None
    assert archive.gunzip_files([]) == ([], [])


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
    assert L.znippy_archive_gunzip_files(archive.h, arr, n, buf.ctypes.data_as(vp), cap, off.ctypes.data_as(vp), st.ctypes.data_as(vp)) == OK
    for k, p in enumerate(paths):
        assert int(st[k]) == want[p][0], (p, st[k])
        piece = buf[int(off[k]):int(off[k + 1])].tobytes()
        assert piece == (want[p][1] if want[p][0] == OK else b""), p
    # the status array is optional; NULL required arguments are refused
    assert L.znippy_archive_gunzip_files(archive.h, arr, n, buf.ctypes.data_as(vp), cap, off.ctypes.data_as(vp), None) == OK
    assert L.znippy_archive_gunzip_files(archive.h, arr, n, buf.ctypes.data_as(vp), cap, None, st.ctypes.data_as(vp)) == E_INVAL
    assert L.znippy_archive_gunzip_files(archive.h, None, n, buf.ctypes.data_as(vp), cap, off.ctypes.data_as(vp), st.ctypes.data_as(vp)) == E_INVAL
    assert L.znippy_archive_gunzip_files(None, arr, n, buf.ctypes.data_as(vp), cap, off.ctypes.data_as(vp), st.ctypes.data_as(vp)) == E_INVAL
    assert L.znippy_archive_gunzip_files(archive.h, arr, n, None, cap, off.ctypes.data_as(vp), st.ctypes.data_as(vp)) == E_INVAL
