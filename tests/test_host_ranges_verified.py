"""znippy_archive_read_range_verified (the compiled host layer): pread with every returned byte covered by a hash that
chains to the index checksum.  Slices of extract_file on a clean archive; on a damaged one, ZNIPPY_E_CHECKSUM for the
blocks a read touches and for the first touch of the chunk by a fresh handle."""
import numpy as np
import pytest

import gen

pytestmark = pytest.mark.gpu

BLK = 128 * 1024
FILES = {"big.txt": gen.pseudo_text(300_001, seed=3), "stored.jar": gen.incompressible(7, 300_001), "small.txt": gen.text(5_000)}
E_CHECKSUM = "rc=-7"


@pytest.fixture(scope="module")
def archive_path(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import host
    from znippy_amd.stream_packer import ArchiveEntry
    assert hasattr(host.lib(), "znippy_archive_read_range_verified")
    p = tmp_path_factory.mktemp("host_ranges_verified") / "a.znippy"
    c = host.compress_stream(str(p), False)
    for k, v in FILES.items():
        c.send(ArchiveEntry(k, v))
    c.finish()
    return p


def shapes(n):
    return [(0, 1), (10, 4096), (131_071, 2), (BLK, 1), (2 * BLK - 5, 4097), (100, n - 200), (0, n), (0, n + 99), (n - 1, 1), (n - 1, 50),
            (n, 10), (n + 10 ** 9, 10), (5, 0)]


def test_verified_reads_against_extract_file(archive_path):
    from znippy_amd import host
    a = host.ZnippyArchive.open(archive_path)
    rows, _, _ = host.read_index(archive_path)
    jar = [r for r in rows if r["relative_path"] == "stored.jar"]
    assert len(jar) == 1 and not jar[0]["compressed"] and jar[0]["blob_size"] == 300_001   # one stored chunk of three blocks
    for name, data in FILES.items():
        whole = a.extract_file(name)
        assert whole == data
        for off, n in shapes(len(data)):
            assert a.read_range_verified(name, off, n) == whole[off:off + n], (name, off, n)
    with pytest.raises(KeyError):
        a.read_range_verified("nope", 0, 1)
    a.close()


def test_damage_between_two_reads_and_on_a_fresh_handle(archive_path, tmp_path):
    from znippy_amd import host
    rows, _, _ = host.read_index(archive_path)
    (jar,) = [r for r in rows if r["relative_path"] == "stored.jar"]
    p = tmp_path / "damaged.znippy"
    p.write_bytes(archive_path.read_bytes())
    a = host.ZnippyArchive.open(p)
    data = FILES["stored.jar"]
    assert a.read_range_verified("stored.jar", 1000, 4096) == data[1000:5096]              # builds the chunk's entries
    at = BLK + 4321                                                                         # inside block 1
    with open(p, "r+b") as f:
        f.seek(jar["blob_offset"] + at)
        f.write(bytes([data[at] ^ 0x40]))
    assert a.read_range("stored.jar", at, 1) == bytes([data[at] ^ 0x40])                   # the unverified read returns the damage
    assert a.read_range_verified("stored.jar", 1000, 4096) == data[1000:5096]              # block 0 is still what the index says
    assert a.read_range_verified("stored.jar", 2 * BLK + 5, 100) == data[2 * BLK + 5:2 * BLK + 105]
    for off, n in [(at, 1), (BLK - 10, 20), (at - 100, 4096), (0, 300_001)]:
        with pytest.raises(host.HostError) as e:
            a.read_range_verified("stored.jar", off, n)
        assert E_CHECKSUM in str(e.value), (off, n, str(e.value))
    assert a.read_range_verified("big.txt", BLK - 5, 4097) == FILES["big.txt"][BLK - 5:BLK + 4092]   # other files are untouched
    a.close()
    fresh = host.ZnippyArchive.open(p)                                                      # no cache: the first touch builds, and fails
    with pytest.raises(host.HostError) as e:
        fresh.read_range_verified("stored.jar", 1000, 4096)
    assert E_CHECKSUM in str(e.value)
    assert fresh.read_range_verified("small.txt", 100, 200) == FILES["small.txt"][100:300]
    fresh.close()
