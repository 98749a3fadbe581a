"""ctypes front-end to oracle/liboracle.so — TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this
module; the product path (znippy_amd/) never does.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "liboracle.so")


def build(force=False):
    srcs = [os.path.join(_HERE, f) for f in ("blake3_ref.c", "zstd_ref.c", "loops_ref.c")]
    if (not force and os.path.exists(_SO)
            and all(os.path.getmtime(_SO) >= os.path.getmtime(s) for s in srcs)):
        return _SO
    subprocess.check_call(["make", "-C", _HERE, "-s"])
    return _SO


_lib = None


class VerifyStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("total_chunks", "total_written_bytes", "verified_bytes",
                                          "corrupt_bytes", "corrupt_rows", "decode_errors")]


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_SO)
        L.oracle_blake3.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.oracle_blake3.restype = None
        L.oracle_xxh64.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64]
        L.oracle_xxh64.restype = C.c_uint64
        L.oracle_zstd_get_decompressed_size.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
        L.oracle_zstd_get_decompressed_size.restype = C.c_int
        L.oracle_zstd_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        L.oracle_zstd_decompress.restype = C.c_int64
        L.oracle_zstd_trace.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.oracle_zstd_trace.restype = C.c_int64
        L.oracle_have_libzstd.restype = C.c_int
        L.oracle_libzstd_compress_bound.argtypes = [C.c_size_t]
        L.oracle_libzstd_compress_bound.restype = C.c_size_t
        L.oracle_libzstd_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
        L.oracle_libzstd_compress.restype = C.c_int64
        L.oracle_libzstd_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        L.oracle_libzstd_decompress.restype = C.c_int64
        L.oracle_decompress_rows.argtypes = [C.c_void_p] * 7 + [C.c_uint64, C.c_uint64, C.c_void_p, C.c_int,
                                                               C.c_int, C.POINTER(VerifyStats), C.c_void_p,
                                                               C.c_size_t]
        L.oracle_decompress_rows.restype = C.c_int
        L.oracle_compress_rounds.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_int, C.c_int, C.c_void_p,
                                                               C.c_size_t] + [C.c_void_p] * 4
        L.oracle_compress_rounds.restype = C.c_int64
        _lib = L
    return _lib


def _buf(b):
    """bytes / bytearray / numpy -> (keepalive, void*, nbytes)."""
    a = np.frombuffer(b, dtype=np.uint8) if not isinstance(b, np.ndarray) else b
    a = np.ascontiguousarray(a)
    return a, a.ctypes.data_as(C.c_void_p), a.nbytes


def blake3(data) -> bytes:
    a, p, n = _buf(data)
    out = (C.c_uint8 * 32)()
    lib().oracle_blake3(p, n, out)
    return bytes(out)


def xxh64(data, seed=0) -> int:
    a, p, n = _buf(data)
    return lib().oracle_xxh64(p, n, seed)


def zstd_decompressed_size(frame) -> int:
    a, p, n = _buf(frame)
    v = C.c_uint64()
    rc = lib().oracle_zstd_get_decompressed_size(p, n, C.byref(v))
    if rc:
        raise ValueError(f"oracle getDecompressedSize: error {rc}")
    return v.value


def zstd_decompress(frame, cap=None) -> bytes:
    a, p, n = _buf(frame)
    if cap is None:
        cap = zstd_decompressed_size(frame)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    r = lib().oracle_zstd_decompress(out.ctypes.data_as(C.c_void_p), cap, p, n)
    if r < 0:
        raise ValueError(f"oracle decompress: error {r}")
    return out[:r].tobytes()


_TRACE_KINDS = ("ll", "of", "ml")


def zstd_trace(frame, cap=None) -> dict:
    """What the frame contains, as oracle_zstd_decompress reads it (the same decode, with a recorder).  Returns
    {"content": the decoded bytes, "frames": [frame]}; a frame is a dict of fhd, fcs_bytes, header_bytes, has_size,
    content_size, window, checksum, dict_id, regenerated, checksum_read, blocks; a block is a dict of type (0 raw, 1 RLE,
    2 compressed), size, last, at (position of its first byte in the content) and, for a compressed block:
      lits    type, size_format, streams (0 for raw and RLE literals), regen, comp, header_bytes, bytes (the literals)
      huf     None or kind ("direct" / "fse"), desc_bytes, max_bits (the table's log), weights (as read, then the implied
              last one), longest (the longest code: max_bits + 1 - the smallest weight)
      nseq, nseq_bytes, modes (None without sequences)
      tables  {"ll" / "of" / "ml": mode, log, rle_symbol (None unless RLE_Mode), norm (the counts as read, [] otherwise)}
      seqs    uint64 array [nseq, 4]: literal length, match length, Offset_Value, resolved distance.
    Skippable frames are listed under "skippable" as (magic, size).  Raises ValueError where the decoder does."""
    a, p, n = _buf(frame)
    if cap is None:
        cap = zstd_decompressed_size(frame)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    need = np.zeros(3, dtype=np.uint64)
    ev, sq, lit = np.empty(4096, np.int64), np.empty((1024, 4), np.uint64), np.empty(max(cap, 1), np.uint8)
    for _ in range(2):
        r = lib().oracle_zstd_trace(out.ctypes.data_as(C.c_void_p), cap, p, n, ev.ctypes.data_as(C.c_void_p), len(ev),
                                    sq.ctypes.data_as(C.c_void_p), len(sq), lit.ctypes.data_as(C.c_void_p), len(lit),
                                    need.ctypes.data_as(C.c_void_p))
        if r < 0:
            raise ValueError(f"oracle trace: error {r}")
        if need[0] <= len(ev) and need[1] <= len(sq) and need[2] <= len(lit):
            break
        ev, sq = np.empty(max(int(need[0]), 1), np.int64), np.empty((max(int(need[1]), 1), 4), np.uint64)
        lit = np.empty(max(int(need[2]), 1), np.uint8)
    else:
        raise AssertionError("the recorder asked for more room twice")
    content = out[:r].tobytes()
    sq = sq[:int(need[1])]
    frames, skippable, blk, i, end = [], [], None, 0, int(need[0])
    evl = ev[:end].tolist()
    while i < end:
        tag, k = evl[i], evl[i + 1]
        v = evl[i + 2:i + 2 + k]
        i += 2 + k
        if tag == 1:
            frames.append(dict(zip(("fhd", "fcs_bytes", "header_bytes", "has_size", "content_size", "window", "checksum",
                                    "dict_id"), v), blocks=[]))
        elif tag == 2:
            blk = dict(type=v[0], size=v[1], last=v[2], at=v[3])
            if v[0] == 2:
                blk.update(lits=None, huf=None, nseq=0, nseq_bytes=0, modes=None, tables={}, seqs=sq[:0], _sq=0)
            frames[-1]["blocks"].append(blk)
        elif tag == 3:
            blk["lits"] = dict(type=v[0], size_format=v[1], streams=v[2], regen=v[3], comp=v[4], header_bytes=v[5],
                               bytes=lit[v[6]:v[6] + v[3]].tobytes())
        elif tag == 4:
            w = v[4:] + [v[3]]
            blk["huf"] = dict(kind="fse" if v[0] else "direct", desc_bytes=v[1], max_bits=v[2], weights=w,
                              longest=v[2] + 1 - min(x for x in w if x))
        elif tag == 5:
            blk["nseq"], blk["nseq_bytes"], blk["_sq"] = v[0], v[1], v[2]
        elif tag == 6:
            blk["modes"] = v[0]
        elif tag == 7:
            blk["tables"][_TRACE_KINDS[v[0]]] = dict(mode=v[1], log=v[2], rle_symbol=v[3] if v[1] == 1 else None, norm=v[4:])
        elif tag == 8:
            skippable.append((v[0], v[1]))
        elif tag == 9:
            frames[-1]["regenerated"], frames[-1]["checksum_read"] = v[0], (None if v[1] < 0 else v[1])
    for f in frames:
        for b in f["blocks"]:
            if b["type"] == 2:
                b["seqs"] = sq[b["_sq"]:b["_sq"] + b["nseq"]]
                del b["_sq"]
    return dict(content=content, frames=frames, skippable=skippable)


def have_libzstd() -> bool:
    return bool(lib().oracle_have_libzstd())


def libzstd_compress(data, level=19) -> bytes:
    a, p, n = _buf(data)
    cap = lib().oracle_libzstd_compress_bound(n)
    out = np.empty(cap, dtype=np.uint8)
    r = lib().oracle_libzstd_compress(out.ctypes.data_as(C.c_void_p), cap, p, n, level)
    if r < 0:
        raise RuntimeError(f"libzstd compress failed {r}")
    return out[:r].tobytes()


def libzstd_decompress(frame, cap) -> bytes:
    a, p, n = _buf(frame)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    r = lib().oracle_libzstd_decompress(out.ctypes.data_as(C.c_void_p), cap, p, n)
    if r < 0:
        raise ValueError(f"libzstd decompress failed {r}")
    return out[:r].tobytes()


def decompress_rows(blobs, blob_offset, blob_size, uncompressed_size, out_offset, compressed_bitmap,
                    checksum, row_begin, row_end, out=None, n_threads=1, use_libzstd=False,
                    corrupt_cap=1024):
    """Restated read loop (decompress.rs:L113-192) over in-memory columns."""
    ks = []

    def ptr(x, dt):
        arr = np.ascontiguousarray(np.asarray(x, dtype=dt))
        ks.append(arr)
        return arr.ctypes.data_as(C.c_void_p)

    st = VerifyStats()
    corrupt = np.zeros(corrupt_cap, dtype=np.uint64)
    rc = lib().oracle_decompress_rows(
        ptr(blobs, np.uint8), ptr(blob_offset, np.uint64), ptr(blob_size, np.uint64),
        ptr(uncompressed_size, np.uint64), ptr(out_offset, np.uint64), ptr(compressed_bitmap, np.uint8),
        ptr(checksum, np.uint8), row_begin, row_end,
        out.ctypes.data_as(C.c_void_p) if out is not None else None, n_threads, int(use_libzstd),
        C.byref(st), corrupt.ctypes.data_as(C.c_void_p), corrupt_cap)
    if rc:
        raise RuntimeError(f"oracle_decompress_rows rc={rc}")
    stats = {n: getattr(st, n) for n, _ in VerifyStats._fields_}
    return stats, np.sort(corrupt[:min(st.corrupt_rows, corrupt_cap)])


def compress_rounds(src, off, length, skip, level=19, n_threads=1):
    """Restated write loop (stream_packer.rs:L215-284). Returns dict of per-round columns."""
    src = np.ascontiguousarray(np.asarray(src, dtype=np.uint8))
    off = np.ascontiguousarray(np.asarray(off, dtype=np.uint64))
    length = np.ascontiguousarray(np.asarray(length, dtype=np.uint64))
    skip = np.ascontiguousarray(np.asarray(skip, dtype=np.uint8))
    n = len(off)
    # ZSTD_compressBound(n) = n + n/256 + (n < 128 KiB ? (128 KiB - n)/2048 : 0), summed over rounds
    ln = length.astype(np.int64)
    cap = int(np.sum(ln + (ln >> 8) + np.where(ln < (128 << 10), ((128 << 10) - ln) >> 11, 0))) + 64
    blob = np.empty(max(cap, 1), dtype=np.uint8)
    bo = np.zeros(n, dtype=np.uint64)
    bs = np.zeros(n, dtype=np.uint64)
    ck = np.zeros((n, 32), dtype=np.uint8)
    cm = np.zeros(n, dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    r = lib().oracle_compress_rounds(vp(src), vp(off), vp(length), vp(skip), n, level, n_threads,
                                     vp(blob), cap, vp(bo), vp(bs), vp(ck), vp(cm))
    if r < 0:
        raise RuntimeError(f"oracle_compress_rounds rc={r}")
    return dict(blobs=blob[:r], blob_offset=bo, blob_size=bs, checksum=ck, compressed=cm)
