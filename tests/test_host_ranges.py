"""znippy_archive_read_range (the compiled host layer) against slices of extract_file: pread semantics over an archive whose
files span several chunks — compressed multi-block chunks of this library (the partial route), stored chunks, small files."""
import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu

SLICE = 8 << 20
FILES = {"big.txt": gen.pseudo_text(2 * SLICE + 300_001, seed=3), "stored.jar": gen.incompressible(7, SLICE + 70_001),
         "small.txt": gen.text(5_000), "empty": b""}


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import host
    from znippy_amd.stream_packer import ArchiveEntry
    assert hasattr(host.lib(), "znippy_archive_read_range")
    p = tmp_path_factory.mktemp("host_ranges") / "a.znippy"
    c = host.compress_stream(str(p), False)
    for k, v in FILES.items():
        c.send(ArchiveEntry(k, v))
    c.finish()
    a = host.ZnippyArchive.open(p)
    yield a, p
    a.close()


def shapes(n):
    return [(0, 1), (10, 4096), (131_071, 2), (SLICE - 1, 2), (SLICE - 5, 4097), (SLICE, 1), (100, 2 * SLICE + 70_000), (0, n), (0, n + 99),
            (n - 1, 1), (n - 1, 50), (n, 10), (n + 10 ** 9, 10), (5, 0)]


def test_read_range_against_extract_file(archive):
    archive, _ = archive
    for name, data in FILES.items():
        whole = archive.extract_file(name)
        assert whole == data
        for off, n in shapes(len(data)):
            assert archive.read_range(name, off, n) == whole[off:off + n], (name, off, n)
    with pytest.raises(KeyError):
        archive.read_range("nope", 0, 1)


def test_python_archive_reads_ranges_through_the_device(archive):
    """The Python ZnippyArchive over the same file: HipBackend.read_ranges, batched."""
    from znippy_amd.archive import ZnippyArchive
    _, p = archive
    a = ZnippyArchive.open(p)
    req = [("big.txt", SLICE - 5, 4097), ("nope", 0, 1), ("stored.jar", SLICE - 1, 70_000), ("big.txt", 2 * SLICE + 299_000, 5_000),
           ("small.txt", 4_000, 5_000), ("empty", 0, 1), ("big.txt", 7, 0)]
    got = a.read_ranges(req)
    assert isinstance(got[1], KeyError)
    for (name, off, n), g in zip(req, got):
        if name != "nope":
            assert g == FILES[name][off:off + n], (name, off, n)
