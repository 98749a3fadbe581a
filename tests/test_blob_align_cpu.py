"""blob_align in the Python pipelines, without a GPU: the cursor between staging batches, the merge of the ranks' regions, and
the read side over an archive whose blobs do not lie back to back.  The backend is the oracle double behind a wrapper that
lays its payloads out the way znippy_rounds_set_blob_align does."""
import numpy as np
import pytest

import gen
from znippy_amd import index as ix
from znippy_amd import stream_packer
from znippy_amd.archive import ZnippyArchive
from znippy_amd.decompress import decompress_archive, verify_archive_integrity
from znippy_amd.stream_packer import ArchiveEntry, compress_stream, merge_rank_regions


def round_up(v, a):
    return (int(v) + a - 1) // a * a


class AligningOracle:
    """The oracle backend with set_blob_align: the packed payloads moved to aligned offsets inside the batch's region, zero
    gaps, no padding behind the last one."""

    def __init__(self):
        from oracle_backend import OracleBackend
        self.inner, self.align, self.batches = OracleBackend(), 1, 0

    def set_level(self, level):
        self.inner.set_level(level)

    def set_blob_align(self, align):
        self.align = int(align)

    def encode_hash(self, staging, off, length, skip):
        res, blob = self.inner.encode_hash(staging, off, length, skip)
        self.batches += 1
        n = len(off)
        if not n:
            return res, blob
        bo, bs = np.asarray(res["blob_offset"], np.uint64), np.asarray(res["blob_size"], np.uint64)
        new = np.zeros(n, np.uint64)
        for i in range(1, n):
            new[i] = round_up(int(new[i - 1] + bs[i - 1]), self.align)
        out = np.zeros(int(new[-1] + bs[-1]), np.uint8)
        for i in range(n):
            out[int(new[i]):int(new[i] + bs[i])] = blob[int(bo[i]):int(bo[i] + bs[i])]
        res = dict(res, blob_offset=new)
        return res, out

    def decode_verify(self, *a):
        return self.inner.decode_verify(*a)


FILES = {f"t/{i:02}.txt": gen.pseudo_text(700 + 531 * i, seed=i) for i in range(12)}
FILES.update({"stored.jar": gen.incompressible(5, 7001), "empty": b"", "one.png": gen.incompressible(6, 1), "last.txt": gen.text(333)})


def index_rows(path):
    _, batches = ix.read_znippy_index(str(path))
    rows = []
    for b in batches:
        rows += list(zip(b.column(0).to_pylist(), b.column(5).to_pylist(), b.column(6).to_pylist()))
    return rows


def write(path, backend, blob_align):
    c = compress_stream(path, False, backend=backend, blob_align=blob_align)
    for k, v in FILES.items():
        c.sender().send(ArchiveEntry(k, v))
    return c.finish()


def test_stream_packer_aligns_across_batch_borders(oracle, tmp_path, monkeypatch):
    monkeypatch.setattr(stream_packer, "BATCH_BYTES", 4000)  # a few rounds per staging batch
    b = AligningOracle()
    rep = write(tmp_path / "a.znippy", b, 128)
    assert b.batches >= 5 and b.align == 128
    packed = write(tmp_path / "p.znippy", AligningOracle(), 1)
    rows, prows = sorted(index_rows(tmp_path / "a.znippy"), key=lambda r: r[1]), sorted(index_rows(tmp_path / "p.znippy"), key=lambda r: r[1])
    assert len(rows) == len(FILES)
    assert all(o % 128 == 0 for _, o, _ in rows)
    # every blob right behind the one before, rounded up — also where the next one came from another batch
    assert rows[0][1] == 0 and all(rows[i + 1][1] == round_up(rows[i][1] + rows[i][2], 128) for i in range(len(rows) - 1))
    raw = (tmp_path / "a.znippy").read_bytes()
    end = ix.blob_region_end(str(tmp_path / "a.znippy"))
    assert end == rows[-1][1] + rows[-1][2]                      # nothing behind the last blob
    gap = np.ones(end, bool)
    for _, o, s in rows:
        gap[o:o + s] = False
    assert gap.any() and not np.frombuffer(raw[:end], np.uint8)[gap].any()
    # the payloads are the packed archive's, and the report counts payload bytes as before
    praw = (tmp_path / "p.znippy").read_bytes()
    assert [(p, s) for p, _, s in sorted(rows)] == [(p, s) for p, _, s in sorted(prows)]
    for (p, o, s), (_, po, _) in zip(sorted(rows), sorted(prows)):
        assert raw[o:o + s] == praw[po:po + s], p
    for f in ("total_files", "compressed_files", "uncompressed_files", "chunks", "total_bytes_in", "compressed_bytes", "uncompressed_bytes"):
        assert getattr(rep, f) == getattr(packed, f), f
    assert rep.total_bytes_out - packed.total_bytes_out == int(gap.sum())


def test_archive_reads_back(oracle, tmp_path, monkeypatch):
    monkeypatch.setattr(stream_packer, "BATCH_BYTES", 4000)
    b = AligningOracle()
    p = tmp_path / "a.znippy"
    write(p, b, 4096)
    assert all(o % 4096 == 0 for _, o, _ in index_rows(p))
    rep = decompress_archive(p, True, tmp_path / "out", backend=b)
    assert (rep.total_files, rep.corrupt_files, rep.verified_files) == (len(FILES), 0, len(FILES))
    for k, v in FILES.items():
        assert (tmp_path / "out" / k).read_bytes() == v, k
    v = verify_archive_integrity(p, backend=b)
    assert (v.total_files, v.corrupt_files, v.total_bytes) == (len(FILES), 0, sum(len(x) for x in FILES.values()))
    a = ZnippyArchive.open(p, backend=b)
    assert a.extract_files(list(FILES)) == list(FILES.values())
    assert a.extract_file("stored.jar", verify=True) == FILES["stored.jar"]


def test_compress_dir_aligns_every_batch(oracle, tmp_path):
    from znippy_amd.slot_packer import compress_dir
    src = tmp_path / "in"
    for k, v in FILES.items():
        (src / k).parent.mkdir(parents=True, exist_ok=True)
        (src / k).write_bytes(v)
    b = AligningOracle()
    cfg = ix.StrategicConfig(max_core_in_flight=64)
    rep = compress_dir(src, tmp_path / "d", backend=b, config=cfg, blob_align=512)
    assert rep.total_files == len(FILES) and b.batches == 2       # the big pass (the empty files) and the small pass
    assert all(o % 512 == 0 for _, o, _ in index_rows(tmp_path / "d.znippy"))
    out = decompress_archive(tmp_path / "d.znippy", True, tmp_path / "out", backend=b)
    assert out.corrupt_files == 0
    for k, v in FILES.items():
        assert (tmp_path / "out" / k).read_bytes() == v, k


def test_rank_merge_aligns_region_bases():
    def part(sizes, seed):
        sizes = np.array(sizes, np.uint64)
        off = np.zeros(len(sizes), np.uint64)
        for i in range(1, len(sizes)):
            off[i] = round_up(int(off[i - 1] + sizes[i - 1]), 64)
        region = np.random.default_rng(seed).integers(1, 256, int(off[-1] + sizes[-1]), dtype=np.uint8).tobytes()
        cols = dict(blob_offset=off, blob_size=sizes, checksum=np.full((len(sizes), 32), seed, np.uint8), compressed=np.ones(len(sizes), np.uint8))
        return cols, region
    gathered = [part([5, 77, 1], 1), part([64], 2), part([3, 0, 129], 3), part([1000], 4)]
    cols, region = merge_rank_regions(gathered, 64)
    bases, at = [], 0
    for c, r in gathered:
        at = round_up(at, 64)
        bases.append(at)
        assert region[at:at + len(r)] == r                       # the rank's region, whole, at an aligned base
        at += len(r)
    assert len(region) == at and bases == [0, 256, 320, 576]     # odd region sizes: 193, 64, 193, 1000
    assert not any(region[bases[k] - g:bases[k]] != bytes(g) for k, g in ((1, 63), (3, 63)))   # the gaps in front are zero
    assert (cols["blob_offset"] % np.uint64(64) == 0).all()
    assert cols["blob_offset"].tolist() == [0, 64, 192, 256, 320, 384, 384, 576]
    assert cols["blob_size"].tolist() == [5, 77, 1, 64, 3, 0, 129, 1000] and cols["checksum"][:, 0].tolist() == [1, 1, 1, 2, 3, 3, 3, 4]
    # align 1: the running sum, as before
    cols1, region1 = merge_rank_regions(gathered, 1)
    assert region1 == b"".join(r for _, r in gathered)
    assert cols1["blob_offset"].tolist() == [0, 64, 192, 193, 257, 321, 321, 450]


def test_a_backend_without_the_setting_takes_only_1(oracle, tmp_path):
    from oracle_backend import OracleBackend
    from znippy_amd.slot_packer import compress_dir
    b = OracleBackend()
    assert not hasattr(b, "set_blob_align")
    write(tmp_path / "ok.znippy", b, 1)                          # the default still runs on it
    for align in (2, 128, 4096):
        with pytest.raises(ValueError, match="cannot align"):
            write(tmp_path / "no.znippy", b, align)
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "a.txt").write_bytes(b"abc")
    compress_dir(tmp_path / "in", tmp_path / "d1", backend=b)
    with pytest.raises(ValueError, match="cannot align"):
        compress_dir(tmp_path / "in", tmp_path / "d2", backend=b, blob_align=16)
    for bad in (0, 3, 8192):                                     # not a power of two in 1..4096: refused whatever the backend is
        with pytest.raises(ValueError, match="power of two"):
            write(tmp_path / "bad.znippy", AligningOracle(), bad)
