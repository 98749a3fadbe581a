"""verify (decompress_archive with save_data=false, index.rs:L550-553 / decompress.rs:L186-189) through both host layers: with
a backend that can check rows without writing them the rows go through a verify-only run, with ZNIPPY_NO_VERIFY_ONLY=1 (or a
backend without `verify`) they are decoded and thrown away — the VerifyReport and the corrupt rows are the same either way."""
import dataclasses

import pytest

import gen
from znippy_amd.decompress import decompress_archive, verify_archive_integrity
from znippy_amd.stream_packer import ArchiveEntry, compress_stream

gpu = pytest.mark.gpu


def _entries():
    return [ArchiveEntry("a/text.txt", gen.text(10240 * 30)), ArchiveEntry("a/words.txt", gen.pseudo_text(70000, 4)),
            ArchiveEntry("b/pic.png", gen.incompressible(3, 50000)), ArchiveEntry("b/bin.dat", gen.binary(300000)),
            ArchiveEntry("b/big.jar", gen.incompressible(4, 700000)), ArchiveEntry("empty", b"")] + \
           [ArchiveEntry(f"c/f{i:03}.txt", gen.text(10240)) for i in range(40)]


def _damage(path, needle):
    raw = bytearray(path.read_bytes())
    i = bytes(raw).find(needle)
    assert i >= 0
    raw[i + 9] ^= 0x40
    path.write_bytes(bytes(raw))


def test_python_route_with_a_backend_that_cannot_verify_only(tmp_path, oracle):
    """The CPU checker double has no `verify`: save_data=false still decodes through decode_verify and reports the same."""
    from oracle_backend import OracleBackend
    backend = OracleBackend()
    assert not hasattr(backend, "verify")
    p = tmp_path / "a.znippy"
    c = compress_stream(p, False, backend=backend)
    for e in _entries():
        c.sender().send(e)
    c.finish()
    _damage(p, gen.incompressible(3, 50000)[:64])
    rep = verify_archive_integrity(p, backend=backend)
    assert (rep.total_files, rep.corrupt_files, rep.verified_files, rep.corrupt_bytes) == (46, 1, 45, 50000)
    assert len(rep.corrupt_rows) == 1
    assert rep == decompress_archive(p, True, tmp_path / "o", backend=backend)


def test_python_route_uses_verify_when_the_backend_has_it(tmp_path, oracle, monkeypatch):
    """... and a backend that has `verify` is asked for it with save_data=false only, unless the environment says otherwise."""
    from oracle_backend import OracleBackend

    class Counting(OracleBackend):
        calls = 0

        def verify(self, blobs, blob_base, blob_offset, blob_size, usize, compressed, checksum):
            import numpy as np
            type(self).calls += 1
            usz = np.asarray(usize, np.uint64)
            off = (np.cumsum(usz) - usz).astype(np.uint64)
            return self.decode_verify(blobs, blob_base, blob_offset, blob_size, usize, off, compressed, checksum, int(usz.sum()))[:3]

    backend = Counting()
    p = tmp_path / "a.znippy"
    c = compress_stream(p, False, backend=backend)
    for e in _entries():
        c.sender().send(e)
    c.finish()
    _damage(p, gen.incompressible(3, 50000)[:64])
    monkeypatch.delenv("ZNIPPY_NO_VERIFY_ONLY", raising=False)
    full = decompress_archive(p, True, tmp_path / "o", backend=backend)
    assert Counting.calls == 0
    rep = verify_archive_integrity(p, backend=backend)
    assert Counting.calls >= 1 and rep == full
    monkeypatch.setenv("ZNIPPY_NO_VERIFY_ONLY", "1")
    n = Counting.calls
    assert verify_archive_integrity(p, backend=backend) == full and Counting.calls == n


@gpu
def test_both_host_layers_report_the_same_with_and_without_verify_only(tmp_path, monkeypatch):
    """An archive written by the compiled host layer, one blob damaged: compiled znippy_decompress_archive(save_data=0) and
    Python verify_archive_integrity, each with the feature on and with ZNIPPY_NO_VERIFY_ONLY=1 — four equal reports."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from znippy_amd import host
    from znippy_amd.backend import HipBackend
    p = tmp_path / "a.znippy"
    c = host.compress_stream(p, False)
    for e in _entries():
        c.send(e)
    c.finish()
    _damage(p, gen.incompressible(4, 700000)[:64])
    backend = HipBackend()
    assert hasattr(backend, "verify")
    reports = {}
    for mode in ("on", "off"):
        if mode == "off":
            monkeypatch.setenv("ZNIPPY_NO_VERIFY_ONLY", "1")
        else:
            monkeypatch.delenv("ZNIPPY_NO_VERIFY_ONLY", raising=False)
        reports["cpp", mode] = host.decompress_archive(p, False, tmp_path / "unused")
        reports["py", mode] = verify_archive_integrity(p, backend=backend)
    first = reports["cpp", "on"]
    assert (first.total_files, first.corrupt_files, first.verified_files, first.corrupt_bytes) == (46, 1, 45, 700000)
    assert len(first.corrupt_rows) == 1
    for k, r in reports.items():
        assert dataclasses.asdict(r) == dataclasses.asdict(first), k
    # and what a run that extracts reports
    monkeypatch.delenv("ZNIPPY_NO_VERIFY_ONLY", raising=False)
    assert dataclasses.asdict(host.decompress_archive(p, True, tmp_path / "o")) == dataclasses.asdict(first)
    assert not (tmp_path / "unused").exists()
    backend.ctx.close()
