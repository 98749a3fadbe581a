"""The compiled host layer's read plans (csrc/host/read_plan.cc) through the library, on an archive that holds one path twice with a
stored entry of 3 MiB between the two: the two rows of the path are scattered, so a read of the file takes the pack branch of
plan_rows_read (one pread per blob instead of the span between them), and they overlap, both beginning at byte 0 of the file."""
import pytest

import gen

gpu = pytest.mark.gpu
DUP = "a/dup.txt"


def test_rank_range_of_the_largest_world(tmp_path, oracle):
    """The second finding: split_rows kept `world + 1` cuts in a vector sized in 32 bits, so world = 2^32 - 1 made a vector of no
    elements and wrote behind it.  Only the rank's own two cuts are computed now.  (A rank with no rows needs no GPU: the archive
    comes from the Python mirror with the checker backend.)"""
    from oracle_backend import OracleBackend
    from znippy_amd import host
    from znippy_amd.stream_packer import ArchiveEntry, compress_stream
    c = compress_stream(tmp_path / "a.znippy", False, backend=OracleBackend())
    for i in range(5):
        c.sender().send(ArchiveEntry(f"f{i}.txt", gen.pseudo_text(4000 + i, seed=i)))
    c.finish()
    for rank in (1, 2 ** 31):                                            # (the first cuts of so many ranks over five rows are all row 0)
        rep = host.decompress_archive(tmp_path / "a.znippy", False, tmp_path / "none", rank=rank, world=2 ** 32 - 1)
        assert (rep.total_files, rep.chunks, rep.corrupt_rows) == (5, 0, [])


@pytest.fixture(scope="module")
def dup_archive(tmp_path_factory):
    from znippy_amd import host
    from znippy_amd.stream_packer import ArchiveEntry
    d = tmp_path_factory.mktemp("read_plan")
    first, jar, second = gen.pseudo_text(5000, seed=1), gen.incompressible(7, 3 * 1024 * 1024 + 17), gen.pseudo_text(7000, seed=2)
    c = host.compress_stream(d / "dup.tmp", False)
    for e in (ArchiveEntry(DUP, first), ArchiveEntry("lib.jar", jar), ArchiveEntry(DUP, second)):
        c.sender().send(e)
    rep = c.finish()
    assert (rep.total_files, rep.uncompressed_files, rep.chunks) == (3, 1, 3)
    return d / "dup.znippy", first, jar, second


@gpu
def test_scattered_rows_of_one_file_are_packed(dup_archive, tmp_path):
    from znippy_amd import host
    archive, first, jar, second = dup_archive
    rows, _, _ = host.read_index(archive)
    assert [r["relative_path"] for r in rows] == [DUP, "lib.jar", DUP] and not rows[1]["compressed"]
    blobs = rows[0]["blob_size"] + rows[2]["blob_size"]
    span = rows[2]["blob_offset"] + rows[2]["blob_size"] - rows[0]["blob_offset"]
    assert span > 2 * blobs + (1 << 20)                                    # the rule of the pack branch
    a = host.ZnippyArchive.open(archive)
    assert a.extract_file(DUP) == first + second                          # both entries, in index order (as before this module)
    assert a.extract_file(DUP, verify=True) == first + second
    assert a.extract_file("lib.jar") == jar
    rep = host.decompress_archive(archive, False, tmp_path / "none")
    assert rep.corrupt_rows == [] and rep.corrupt_files == 0 and rep.chunks == 3
    rep = host.decompress_archive(archive, True, tmp_path / "out")
    assert rep.corrupt_rows == [] and rep.corrupt_files == 0 and rep.total_files == 2
    assert (tmp_path / "out" / "lib.jar").read_bytes() == jar
    assert (tmp_path / "out" / DUP).read_bytes() == second                # the later, longer entry over the earlier one


@gpu
def test_range_read_of_overlapping_chunks_stays_inside_the_request(dup_archive):
    """The finding of tests/test_read_plan_cpu.py: both rows of the path begin at byte 0 of the file, so a range touches both, and
    the bytes of both used to be copied into a buffer of `length` bytes.  A chunk now gives what the chunks in front of it have
    left of the request."""
    from znippy_amd import host
    archive, first, _, second = dup_archive
    a = host.ZnippyArchive.open(archive)
    for read in (a.read_range, a.read_range_verified):
        assert read(DUP, 0, 4000) == first[:4000]
        assert read(DUP, 1000, 4000) == first[1000:]                       # (the first entry ends at 5000: it fills the request)
        assert read(DUP, 0, 6000) == first + second[:1000]
        assert read(DUP, 6000, 5000) == second[6000:]
        assert read(DUP, 7000, 10) == b""
