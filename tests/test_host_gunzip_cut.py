"""The compiled host layer with ZNIPPY_GZ_CUT in the environment: an archive opened with the block-start search on must give, for a
.tar.gz of a few MiB that has no flush point, for a crate-like file and for damaged ones, exactly what the same archive opened without
it gives — through gunzip_files and through list_tar_members."""
import gzip
import io
import os
import tarfile

import pytest

import gen

pytestmark = pytest.mark.gpu


def files():
    b = io.BytesIO()
    with tarfile.open(fileobj=b, mode="w", format=tarfile.GNU_FORMAT) as tf:
        for k in range(12):
            data = gen.pseudo_text(250_000 + 7777 * k, seed=60 + k)
            ti = tarfile.TarInfo(f"pkg-2.0/src/m{k}.py")
            ti.size = len(data)
            tf.addfile(ti, io.BytesIO(data))
    tar = b.getvalue()
    assert len(tar) > 3 << 20
    sdist = gzip.compress(tar, 6, mtime=0)                      # one member, no flush
    damaged = bytearray(sdist)
    damaged[len(sdist) // 2] ^= 0x08
    return {"sdist/pkg-2.0.tar.gz": sdist, "crates/pkg-2.0.crate": gzip.compress(tar[:700_000] + bytes(1024), 9, mtime=0), "sdist/damaged.tar.gz": bytes(damaged),
            "logs/short.gz": gzip.compress(gen.text(50), 6, mtime=0)}


@pytest.fixture(scope="module")
def archive_path(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import host
    from znippy_amd.stream_packer import ArchiveEntry
    p = tmp_path_factory.mktemp("host_gunzip_cut") / "a.znippy"
    c = host.compress_stream(str(p), False)
    for k, v in files().items():
        c.send(ArchiveEntry(k, v))
    c.finish()
    return p


def answers(path, cut):
    from znippy_amd import host
    old = os.environ.get("ZNIPPY_GZ_CUT")
    if cut is None:
        os.environ.pop("ZNIPPY_GZ_CUT", None)
    else:
        os.environ["ZNIPPY_GZ_CUT"] = str(cut)
    try:
        a = host.ZnippyArchive.open(path)
        try:
            paths = sorted(files())
            tars = [p for p in paths if not p.startswith("logs/")]
            return a.gunzip_files(paths), a.list_tar_members(tars, contents=True), a.list_tar_members(tars, suffix=b"m3.py")
        finally:
            a.close()
    finally:
        if old is None:
            os.environ.pop("ZNIPPY_GZ_CUT", None)
        else:
            os.environ["ZNIPPY_GZ_CUT"] = old


def test_same_answers_with_the_search_on(archive_path):
    f = files()
    off = answers(archive_path, None)
    (got, st), listed, one = off
    paths = sorted(f)
    at = paths.index("sdist/pkg-2.0.tar.gz")
    assert st[at] == 0 and got[at] == gzip.decompress(f["sdist/pkg-2.0.tar.gz"]) and st[paths.index("sdist/damaged.tar.gz")] != 0
    assert st[paths.index("logs/short.gz")] == 0 and len(listed[2][1]) == 12 and len(one[2][1]) == 1
    for cut in (64, 16384):
        assert answers(archive_path, cut) == off, cut
