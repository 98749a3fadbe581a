"""The block tree sidecar `<archive>.b3t` on the compiled host layer: written by compress_stream / compress_dir under
ZNIPPY_HOST_BLOCK_TREE=1 from the trees the encode runs emit, read by znippy_archive_open and offered — never trusted — on the
first verified touch of a multi-block chunk.  The files are those of test_host_ranges_verified.py; the reference is
tests/b3_tree.py."""
import os

import numpy as np
import pytest

import b3_tree
from test_host_ranges_verified import BLK, E_CHECKSUM, FILES, shapes

pytestmark = pytest.mark.gpu

MULTI = [k for k, v in FILES.items() if len(v) > BLK]  # one chunk each, of three blocks


class BlockTreeEnv:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("ZNIPPY_HOST_BLOCK_TREE")
        if self.value is None:
            os.environ.pop("ZNIPPY_HOST_BLOCK_TREE", None)
        else:
            os.environ["ZNIPPY_HOST_BLOCK_TREE"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("ZNIPPY_HOST_BLOCK_TREE", None)
        else:
            os.environ["ZNIPPY_HOST_BLOCK_TREE"] = self.old


def write_stream(path, value, files=FILES):
    from znippy_amd import host
    from znippy_amd.stream_packer import ArchiveEntry
    with BlockTreeEnv(value):
        c = host.compress_stream(str(path), False)
        for k, v in files.items():
            c.send(ArchiveEntry(k, v))
        c.finish()


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    """(archive with a sidecar, the same archive written without the variable), through compress_stream."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import block_tree, host
    assert hasattr(host.lib(), "znippy_archive_block_tree_stats") and callable(block_tree.read_sidecar)
    d = tmp_path_factory.mktemp("host_tree_sidecar")
    (d / "on").mkdir()
    (d / "off").mkdir()
    write_stream(d / "on" / "a.znippy", "1")
    write_stream(d / "off" / "a.znippy", None)
    return d / "on" / "a.znippy", d / "off" / "a.znippy"


def check_sidecar(archive, files):
    """The sidecar parses, counts the index's rows and holds b3_tree's entries per chunk, in index order."""
    from znippy_amd import block_tree, host
    rows, _, _ = host.read_index(archive)
    n_rows, entries = block_tree.read_sidecar(block_tree.sidecar_path(archive))
    assert n_rows == len(rows)
    want = []
    for r in rows:
        data = files[r["relative_path"]]
        chunk = data[r["fdata_offset"]:r["fdata_offset"] + (r["uncompressed_size"] if r["compressed"] else r["blob_size"])]
        want.append(b3_tree.entries(chunk))
    want = np.concatenate(want)
    assert entries.shape == want.shape and want.shape[0] == 3 * len(MULTI)
    assert np.array_equal(entries, want)
    assert os.path.getsize(block_tree.sidecar_path(archive)) == 32 + 32 * want.shape[0]
    return entries


def test_written_by_compress_stream(archives, tmp_path):
    on, off = archives
    check_sidecar(on, FILES)
    assert on.read_bytes() == off.read_bytes()                      # the archive does not depend on the variable
    assert not os.path.exists(str(off) + ".b3t")
    write_stream(tmp_path / "zero.znippy", "0")
    assert (tmp_path / "zero.znippy").read_bytes() == on.read_bytes() and not (tmp_path / "zero.znippy.b3t").exists()
    stale = tmp_path / "zero.znippy.b3t"                            # off: a sidecar that is there is not touched either
    stale.write_bytes(b"left alone")
    write_stream(tmp_path / "zero.znippy", None)
    assert stale.read_bytes() == b"left alone"


def test_written_by_compress_dir(archives, tmp_path):
    from znippy_amd import host
    src = tmp_path / "in"
    (src / "sub").mkdir(parents=True)
    files = {"big.txt": FILES["big.txt"], "sub/stored.jar": FILES["stored.jar"], "sub/small.txt": FILES["small.txt"], "empty": b""}
    for k, v in files.items():
        (src / k).write_bytes(v)
    with BlockTreeEnv("1"):
        host.compress_dir(src, tmp_path / "d.znippy")
    with BlockTreeEnv(None):
        host.compress_dir(src, tmp_path / "plain.znippy")
    check_sidecar(tmp_path / "d.znippy", files)
    assert (tmp_path / "d.znippy").read_bytes() == (tmp_path / "plain.znippy").read_bytes()
    assert not (tmp_path / "plain.znippy.b3t").exists()
    a = host.ZnippyArchive.open(tmp_path / "d.znippy")
    assert a.block_tree_stats() == [6, 0, 0, 0]
    assert a.read_range_verified("sub/stored.jar", BLK + 7, 4096) == files["sub/stored.jar"][BLK + 7:BLK + 7 + 4096]
    assert a.block_tree_stats() == [6, 1, 0, 0]
    a.close()


def test_reads_with_a_sidecar(archives):
    from znippy_amd import host
    on, _ = archives
    a = host.ZnippyArchive.open(on)
    assert a.block_tree_stats() == [3 * len(MULTI), 0, 0, 0]
    touched = 0
    for name, data in FILES.items():
        whole = a.extract_file(name)
        assert whole == data
        for off, n in shapes(len(data)):
            assert a.read_range_verified(name, off, n) == whole[off:off + n], (name, off, n)
        touched += name in MULTI
        assert a.block_tree_stats() == [3 * len(MULTI), touched, 0, 0], name   # accepted once per chunk, never built
    a.close()


def test_damaged_sidecar_costs_a_build(archives, tmp_path):
    from znippy_amd import block_tree, host
    on, _ = archives
    p = tmp_path / "a.znippy"
    p.write_bytes(on.read_bytes())
    rows, _, _ = host.read_index(p)
    n_rows, entries = block_tree.read_sidecar(str(on) + ".b3t")
    first = block_tree.layout([r["uncompressed_size"] if r["compressed"] else r["blob_size"] for r in rows])[1]
    (jar,) = [i for i, r in enumerate(rows) if r["relative_path"] == "stored.jar"]
    entries[int(first[jar]) + 1, 9] ^= 0x10                          # one byte of one entry of the jar
    block_tree.write_sidecar(str(p) + ".b3t", n_rows, entries)
    a = host.ZnippyArchive.open(p)
    assert a.block_tree_stats() == [6, 0, 0, 0]
    data = FILES["stored.jar"]
    assert a.read_range_verified("stored.jar", 1000, 4096) == data[1000:5096]
    assert a.block_tree_stats() == [6, 0, 1, 1]                      # rejected, then built by a whole decode
    for off, n in shapes(len(data)):
        assert a.read_range_verified("stored.jar", off, n) == data[off:off + n], (off, n)
    assert a.block_tree_stats() == [6, 0, 1, 1]
    assert a.read_range_verified("big.txt", BLK - 5, 4097) == FILES["big.txt"][BLK - 5:BLK + 4092]
    assert a.block_tree_stats() == [6, 1, 1, 1]                      # the other chunk's entries are good
    a.close()


def test_mismatched_sidecar_is_ignored(archives, tmp_path):
    from znippy_amd import block_tree, host
    on, _ = archives
    good = (on.parent / (on.name + ".b3t")).read_bytes()
    write_stream(tmp_path / "other.znippy", "1", {"x.txt": FILES["big.txt"], "y.jar": FILES["stored.jar"]})   # two rows, not three
    other = (tmp_path / "other.znippy.b3t").read_bytes()
    assert block_tree.read_sidecar(tmp_path / "other.znippy.b3t")[0] == 2
    shapes_ = {"truncated": good[:-32], "cut": good[:-1], "short": good[:20], "other archive": other, "magic": b"ZNPYB3T9" + good[8:],
               "fewer entries": good[:24] + (5).to_bytes(8, "little") + good[32:-32]}
    for i, (what, raw) in enumerate(shapes_.items()):
        p = tmp_path / f"m{i}.znippy"
        p.write_bytes(on.read_bytes())
        (tmp_path / (p.name + ".b3t")).write_bytes(raw)
        a = host.ZnippyArchive.open(p)
        assert a.block_tree_stats() == [0, 0, 0, 0], what
        assert a.read_range_verified("stored.jar", BLK + 1, 4096) == FILES["stored.jar"][BLK + 1:BLK + 4097], what
        assert a.block_tree_stats() == [0, 0, 0, 1], what            # as without one: built by a whole decode
        a.close()


def test_damaged_blob_with_a_valid_sidecar(archives, tmp_path):
    from znippy_amd import host
    on, _ = archives
    p = tmp_path / "a.znippy"
    p.write_bytes(on.read_bytes())
    (tmp_path / "a.znippy.b3t").write_bytes((on.parent / (on.name + ".b3t")).read_bytes())
    rows, _, _ = host.read_index(p)
    (jar,) = [r for r in rows if r["relative_path"] == "stored.jar"]
    data = FILES["stored.jar"]
    at = BLK + 4321                                                   # inside block 1
    with open(p, "r+b") as f:
        f.seek(jar["blob_offset"] + at)
        f.write(bytes([data[at] ^ 0x40]))
    a = host.ZnippyArchive.open(p)                                   # a fresh handle
    assert a.read_range_verified("stored.jar", 1000, 4096) == data[1000:5096]       # block 0: only the touched blocks are hashed
    assert a.read_range_verified("stored.jar", 2 * BLK + 5, 100) == data[2 * BLK + 5:2 * BLK + 105]
    for off, n in [(at, 1), (BLK - 10, 20), (0, 300_001)]:
        with pytest.raises(host.HostError) as e:
            a.read_range_verified("stored.jar", off, n)
        assert E_CHECKSUM in str(e.value), (off, n, str(e.value))
    assert a.block_tree_stats() == [6, 1, 0, 0]
    a.close()
