"""The unverified extract (ZnippyArchive::extract_file / extract_files, archive.rs:L144-168) in both host layers: a decode-only run
(znippy_decode_rows) by default, the decode + verify run without a checksum column under ZNIPPY_NO_DECODE_ONLY=1 — the same
bytes and the same errors either way; the Python mirror falls back to decode_verify on a backend without a decode()."""
import numpy as np
import pytest

import gen
from znippy_amd.archive import ZnippyArchive
from znippy_amd.stream_packer import ArchiveEntry, compress_stream

gpu = pytest.mark.gpu

FILES = {
    "one.txt": gen.text(10240),                      # one chunk
    "small/words.txt": gen.pseudo_text(5000, 2),
    "big.bin": gen.binary(12 * 1024 * 1024),         # several chunks
    "stored.jar": gen.incompressible(5, 70000),      # stored (skip extension)
    "stored_big.png": gen.incompressible(6, 9 * 1024 * 1024),
    "empty": b"",
}


def write_archive(path, backend=None):
    c = compress_stream(path, False, **({"backend": backend} if backend is not None else {}))
    for k, v in FILES.items():
        c.sender().send(ArchiveEntry(k, v))
    c.finish()


def damage(src, dst, needle_of, at):
    raw = bytearray(src.read_bytes())
    i = bytes(raw).find(needle_of[:64])
    assert i >= 0
    raw[i + at] ^= 0x40
    dst.write_bytes(bytes(raw))


class Spy:
    """A backend that records which read call the archive mirror makes."""

    def __init__(self, inner, with_decode):
        self.inner, self.calls = inner, []
        if with_decode:
            self.decode = self._decode

    def decode_verify(self, *a):
        self.calls.append(("decode_verify", a[7] is not None))
        return self.inner.decode_verify(*a)

    def _decode(self, blobs, blob_base, bo, bs, usz, oo, comp, total):
        self.calls.append(("decode", False))
        if hasattr(self.inner, "decode"):
            return self.inner.decode(blobs, blob_base, bo, bs, usz, oo, comp, total)
        return self.inner.decode_verify(blobs, blob_base, bo, bs, usz, oo, comp, None, total)


# ---- not gpu: the mirror's dispatch, on the oracle backend double ----------------------------------------------------

def test_archive_mirror_still_extracts_with_the_oracle_backend(oracle, tmp_path):
    from oracle_backend import OracleBackend
    b = OracleBackend()
    assert not hasattr(b, "decode")
    p = tmp_path / "a.znippy"
    write_archive(p, b)
    a = ZnippyArchive.open(p, backend=b)
    got = a.extract_files(list(FILES) + ["nope"])
    assert [g for g in got[:-1]] == list(FILES.values()) and isinstance(got[-1], KeyError)
    assert a.extract_file("big.bin", verify=True) == FILES["big.bin"]


def test_archive_mirror_uses_decode_when_the_backend_has_one_and_falls_back_when_not(oracle, tmp_path, monkeypatch):
    from oracle_backend import OracleBackend
    p = tmp_path / "a.znippy"
    write_archive(p, OracleBackend())
    monkeypatch.delenv("ZNIPPY_NO_DECODE_ONLY", raising=False)
    spy = Spy(OracleBackend(), with_decode=True)
    a = ZnippyArchive.open(p, backend=spy)
    assert a.extract_file("big.bin") == FILES["big.bin"] and spy.calls == [("decode", False)]
    assert a.extract_file("one.txt", verify=True) == FILES["one.txt"] and spy.calls[-1] == ("decode_verify", True)   # a verified extract hashes
    monkeypatch.setenv("ZNIPPY_NO_DECODE_ONLY", "1")
    assert a.extract_file("stored.jar") == FILES["stored.jar"] and spy.calls[-1] == ("decode_verify", False)
    monkeypatch.setenv("ZNIPPY_NO_DECODE_ONLY", "0")
    assert a.extract_file("stored.jar") == FILES["stored.jar"] and spy.calls[-1] == ("decode", False)
    spy = Spy(OracleBackend(), with_decode=False)                # no decode(): what it did before
    a = ZnippyArchive.open(p, backend=spy)
    assert a.extract_files(["one.txt", "empty"]) == [FILES["one.txt"], b""] and spy.calls == [("decode_verify", False)]


# ---- gpu --------------------------------------------------------------------------------------------------------------

@pytest.fixture()
def gpu_archive(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p = tmp_path / "g.znippy"
    write_archive(p)
    bad = tmp_path / "bad.znippy"
    damage(p, bad, FILES["stored.jar"], 9)            # a stored chunk: unverified extracts return the bytes as they are
    bad2 = tmp_path / "bad2.znippy"
    a = ZnippyArchive.open(p)
    raw = bytearray(p.read_bytes())
    raw[int(a._c["blob_offset"][a.file_index["one.txt"][0]]) + 2] ^= 0xFF     # the chunk's frame magic: a decode error
    bad2.write_bytes(bytes(raw))
    return p, bad, bad2


@gpu
def test_python_mirror_extracts_the_same_bytes_with_and_without_decode_only(gpu_archive, monkeypatch):
    from znippy_amd.backend import default_backend
    p, bad, bad2 = gpu_archive
    res = {}
    for env in ("0", "1"):
        monkeypatch.setenv("ZNIPPY_NO_DECODE_ONLY", env)
        spy = Spy(default_backend(), with_decode=True)
        a = ZnippyArchive.open(p, backend=spy)
        got = a.extract_files(list(FILES))
        assert got == list(FILES.values()), env
        assert [a.extract_file(k) for k in FILES] == list(FILES.values()), env
        assert a.extract_file("big.bin", verify=True) == FILES["big.bin"]
        assert {c[0] for c in spy.calls if not c[1]} == ({"decode"} if env == "0" else {"decode_verify"}), (env, spy.calls)
        b = ZnippyArchive.open(bad, backend=default_backend())
        flipped = b.extract_file("stored.jar")
        assert flipped != FILES["stored.jar"] and len(flipped) == 70000     # not checked on this path, as in the reference
        with pytest.raises(ValueError, match="checksum mismatch"):
            b.extract_file("stored.jar", verify=True)
        b2 = ZnippyArchive.open(bad2, backend=default_backend())
        with pytest.raises(ValueError) as e:
            b2.extract_file("one.txt")
        assert b2.extract_file("small/words.txt") == FILES["small/words.txt"]
        res[env] = (flipped, str(e.value))
    assert res["0"] == res["1"]
    assert "decompress failed" in res["0"][1]


@gpu
def test_compiled_extract_file_with_and_without_decode_only(gpu_archive, monkeypatch):
    from znippy_amd import host
    p, bad, bad2 = gpu_archive
    res = {}
    for env in ("0", "1"):
        monkeypatch.setenv("ZNIPPY_NO_DECODE_ONLY", env)
        a = host.ZnippyArchive.open(p)
        for k, v in FILES.items():
            assert a.extract_file(k) == v, (env, k)
            assert a.extract_file(k, verify=True) == v, (env, k)
        with pytest.raises(KeyError):
            a.extract_file("nope")
        a.close()
        b = host.ZnippyArchive.open(bad)
        flipped = b.extract_file("stored.jar")
        assert flipped != FILES["stored.jar"] and len(flipped) == 70000
        with pytest.raises(host.HostError):
            b.extract_file("stored.jar", verify=True)
        b.close()
        b2 = host.ZnippyArchive.open(bad2)
        with pytest.raises(host.HostError) as e:
            b2.extract_file("one.txt")
        b2.close()
        res[env] = (flipped, str(e.value))
    assert res["0"] == res["1"], (res["0"][1], res["1"][1])
