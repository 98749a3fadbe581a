"""ZNIPPY_HOST_BLOB_ALIGN in the compiled host layer: every slot's rounds table gets the alignment and every slot is written at
an aligned out_cursor, so every blob_offset of the archive is a multiple of it; the holes read as zeros.  The read side needs
nothing: the same archive goes through znippy_decompress_archive with and without save_data and through the verified extract."""
import numpy as np
import pytest

import gen
from znippy_amd.stream_packer import ArchiveEntry

pytestmark = pytest.mark.gpu

ALIGN = 4096
FILES = {f"t/{i:02}.txt": gen.pseudo_text(900 + 7919 * i, seed=i) for i in range(24)}
FILES.update({
    "big.bin": gen.binary(20 * 1024 * 1024 + 5),            # three chunks, more than two 8 MiB slots
    "stored_big.png": gen.incompressible(6, 9 * 1024 * 1024 + 1),
    "stored.jar": gen.incompressible(5, 70001),
    "one.gz": gen.incompressible(7, 1),
    "empty": b"",
    "last.txt": gen.text(10241),
})


@pytest.fixture()
def host_env(monkeypatch):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setenv("ZNIPPY_HOST_BLOB_ALIGN", str(ALIGN))
    monkeypatch.setenv("ZNIPPY_HOST_SLOT_MB", "1")           # a slot holds one 8 MiB round at least: several slots
    from znippy_amd import host
    return host


def check_archive(host, p, tmp_path, n_rows_min):
    rows, _, _ = host.read_index(p)
    assert len(rows) >= n_rows_min
    assert all(r["blob_offset"] % ALIGN == 0 for r in rows)
    rows.sort(key=lambda r: r["blob_offset"])
    raw = np.frombuffer(p.read_bytes(), np.uint8)
    end = rows[-1]["blob_offset"] + rows[-1]["blob_size"]
    gap = np.ones(end, bool)
    for r in rows:
        gap[r["blob_offset"]:r["blob_offset"] + r["blob_size"]] = False
    assert gap.any() and not raw[:end][gap].any(), "bytes between blobs are not zero"
    for a, b in zip(rows, rows[1:]):                          # no more room than the alignment asks for
        assert b["blob_offset"] - (a["blob_offset"] + a["blob_size"]) < ALIGN
    saved = host.decompress_archive(p, True, tmp_path / "out")
    dry = host.decompress_archive(p, False, tmp_path / "unused")
    assert saved.corrupt_files == 0 and dry.corrupt_files == 0 and saved.corrupt_rows == [] and dry.corrupt_rows == []
    assert (saved.total_files, saved.verified_files, saved.total_bytes, saved.verified_bytes, saved.chunks) == \
           (dry.total_files, dry.verified_files, dry.total_bytes, dry.verified_bytes, dry.chunks)
    assert saved.verified_bytes == sum(len(v) for v in FILES.values())
    for k, v in FILES.items():
        assert (tmp_path / "out" / k).read_bytes() == v, k
    return rows


def test_compress_stream_aligned(host_env, tmp_path, monkeypatch):
    host = host_env
    p = tmp_path / "a.znippy"
    c = host.compress_stream(p)
    for k, v in FILES.items():
        c.send(ArchiveEntry(k, v))
    rep = c.finish()
    assert rep.total_files == len(FILES) and rep.chunks == len(FILES) + 2 + 1
    check_archive(host, p, tmp_path, rep.chunks)
    a = host.ZnippyArchive.open(p)
    assert a.extract_file("big.bin", verify=True) == FILES["big.bin"]      # a multi-chunk file
    assert a.extract_file("stored_big.png", verify=True) == FILES["stored_big.png"]
    assert a.extract_file("t/05.txt") == FILES["t/05.txt"]
    a.close()
    # the packed archive of the same entries: same payload sizes, a shorter file
    monkeypatch.setenv("ZNIPPY_HOST_BLOB_ALIGN", "3")         # not a power of two: treated as 1
    q = tmp_path / "p.znippy"
    c = host.compress_stream(q)
    for k, v in FILES.items():
        c.send(ArchiveEntry(k, v))
    packed = c.finish()
    prow, _, _ = host.read_index(q)
    prow.sort(key=lambda r: r["blob_offset"])
    assert prow[0]["blob_offset"] == 0 and all(b["blob_offset"] == a_["blob_offset"] + a_["blob_size"] for a_, b in zip(prow, prow[1:]))
    for f in ("total_files", "compressed_files", "uncompressed_files", "chunks", "total_bytes_in", "compressed_bytes", "uncompressed_bytes"):
        assert getattr(rep, f) == getattr(packed, f), f
    assert rep.total_bytes_out > packed.total_bytes_out


def test_compress_dir_aligned(host_env, tmp_path):
    host = host_env
    src = tmp_path / "in"
    for k, v in FILES.items():
        (src / k).parent.mkdir(parents=True, exist_ok=True)
        (src / k).write_bytes(v)
    rep = host.compress_dir(src, tmp_path / "d")
    assert rep.total_files == len(FILES)
    check_archive(host, tmp_path / "d.znippy", tmp_path, rep.chunks)
