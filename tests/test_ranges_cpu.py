"""ZnippyArchive.read_range / read_ranges without a GPU: the mapping of a file-level range to its chunks by fdata_offset, the
pread semantics, and what goes down to the backend.  The archive is written through the oracle double with a small split size,
so that files have several chunks; the double has no read_ranges, so the archive decodes the touched chunks whole and slices —
a recording double with the method shows what a backend that has it is handed."""
import numpy as np
import pytest

import gen
from znippy_amd import stream_packer
from znippy_amd.archive import ZnippyArchive
from znippy_amd.stream_packer import ArchiveEntry, compress_stream

SPLIT = 4096
FILES = {"big.txt": gen.pseudo_text(3 * SPLIT + 1500, seed=1), "two.txt": gen.pseudo_text(SPLIT + 1, seed=2), "small.txt": gen.text(777),
         "stored.jar": gen.incompressible(4, 2 * SPLIT + 9), "empty": b""}


@pytest.fixture(scope="module")
def archive_path(oracle, tmp_path_factory):
    from oracle_backend import OracleBackend
    p = tmp_path_factory.mktemp("ranges") / "a.znippy"
    mp = pytest.MonkeyPatch()
    mp.setattr(stream_packer, "SLICE_SIZE", SPLIT)
    try:
        c = compress_stream(p, False, backend=OracleBackend())
        for k, v in FILES.items():
            c.sender().send(ArchiveEntry(k, v))
        c.finish()
    finally:
        mp.undo()
    return p


@pytest.fixture()
def archive(archive_path):
    from oracle_backend import OracleBackend
    a = ZnippyArchive.open(archive_path, backend=OracleBackend())
    assert len(a.file_index["big.txt"]) == 4 and len(a.file_index["stored.jar"]) == 3
    return a


SHAPES = [(10, 100), (SPLIT - 1, 1), (SPLIT - 1, 2), (SPLIT, 1), (SPLIT - 50, 100), (100, 2 * SPLIT), (0, 10 ** 9), (3 * SPLIT + 1400, 100),
          (3 * SPLIT + 1400, 101), (3 * SPLIT + 1499, 50), (3 * SPLIT + 1500, 10), (10 ** 7, 10), (5, 0), (0, 0)]


def test_read_range_is_pread(archive):
    for name in ("big.txt", "stored.jar", "two.txt", "small.txt", "empty"):
        data = FILES[name]
        for off, n in SHAPES:
            assert archive.read_range(name, off, n) == data[off:off + n], (name, off, n)
    assert archive.read_range("big.txt", 0, len(FILES["big.txt"])) == archive.extract_file("big.txt")
    with pytest.raises(KeyError):
        archive.read_range("nope", 0, 1)


def test_read_ranges_over_several_files(archive):
    req = [("big.txt", SPLIT - 3, 2 * SPLIT), ("nope", 0, 5), ("stored.jar", 8000, 5000), ("small.txt", 700, 500), ("big.txt", 1, 2),
           ("empty", 0, 4), ("two.txt", SPLIT, 100)]
    got = archive.read_ranges(req)
    assert isinstance(got[1], KeyError)
    for (name, off, n), g in zip(req, got):
        if name != "nope":
            assert g == FILES[name][off:off + n], (name, off, n)
    assert archive.read_ranges([]) == []


class Recording:
    """A backend with read_ranges: records what it is handed and answers from the files' bytes."""

    def __init__(self, archive):
        self.a, self.calls = archive, []

    def read_ranges(self, blobs, blob_base, blob_offset, blob_size, usize, compressed, range_row, range_begin, range_len):
        self.calls.append(dict(blobs=np.array(blobs), base=blob_base, bo=np.array(blob_offset), bs=np.array(blob_size), us=np.array(usize),
                               comp=np.array(compressed), rr=np.array(range_row), rb=np.array(range_begin), rl=np.array(range_len)))
        return np.zeros(len(range_row), np.int32), np.zeros(int(np.asarray(range_len).sum()), np.uint8), 0


def test_only_the_touched_chunks_go_down(archive, archive_path):
    rec = Recording(archive)
    a = ZnippyArchive.open(archive_path, backend=rec)
    c = a._c
    big, jar = a.file_index["big.txt"], a.file_index["stored.jar"]
    out = a.read_ranges([("big.txt", SPLIT + 10, SPLIT), ("stored.jar", 2 * SPLIT + 1, 100), ("big.txt", 2 * SPLIT - 1, 3)])
    assert [len(x) for x in out] == [SPLIT, 8, 3] and len(rec.calls) == 1
    k = rec.calls[0]
    touched = [big[1], big[2], jar[2]]                     # chunks 1 and 2 of big.txt (twice), the last chunk of the jar
    assert list(k["bs"]) == [int(c["blob_size"][r]) for r in touched]
    assert list(k["us"]) == [int(a._rlen[r]) for r in touched] and list(k["comp"]) == [True, True, False]
    assert list(k["rr"]) == [0, 1, 2, 0, 1] and list(k["rb"]) == [10, 0, 1, SPLIT - 1, 0] and list(k["rl"]) == [SPLIT - 10, 10, 8, 1, 2]
    # the bytes read from the file lie between the first and the last touched blob (read_spans reads close neighbours in one go), and
    # every row's slice of the buffer is its blob in the file
    raw = archive_path.read_bytes()
    lo = min(int(c["blob_offset"][r]) for r in touched)
    hi = max(int(c["blob_offset"][r] + c["blob_size"][r]) for r in touched)
    assert sum(int(c["blob_size"][r]) for r in touched) <= len(k["blobs"]) <= hi - lo < len(raw) - 1000
    for i, r in enumerate(touched):
        lo = int(k["bo"][i]) - k["base"]
        assert k["blobs"][lo:lo + int(k["bs"][i])].tobytes() == raw[int(c["blob_offset"][r]):int(c["blob_offset"][r] + c["blob_size"][r])]
    # nothing to read: no call at all
    assert a.read_ranges([("big.txt", 10 ** 6, 5), ("empty", 0, 1), ("big.txt", 7, 0)]) == [b"", b"", b""] and len(rec.calls) == 1
