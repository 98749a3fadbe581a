"""ctypes binding of the compiled host layer (include/znippy_host.h, csrc/host/*.cpp)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import index as ix

vp = C.c_void_p


class _CR(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("total_files", "compressed_files", "uncompressed_files", "total_dirs",
                                          "total_bytes_in", "total_bytes_out", "compressed_bytes", "uncompressed_bytes",
                                          "chunks")] + [("compression_ratio", C.c_float)]


class _VR(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("total_files", "verified_files", "corrupt_files", "total_bytes",
                                          "verified_bytes", "corrupt_bytes", "chunks")]


class _ME(C.Structure):
    _fields_ = [("pkg_type", C.c_int8), ("repo", C.c_char_p), ("module_name", C.c_char_p), ("index_offset", C.c_uint64),
                ("index_len", C.c_uint64), ("row_count", C.c_uint64)]


HOST_EXPORTS = [
    "znippy_host_last_error", "znippy_compress_stream", "znippy_stream_send", "znippy_stream_send_packed", "znippy_stream_finish",
    "znippy_compress_dir", "znippy_decompress_archive", "znippy_archive_open", "znippy_archive_file_count", "znippy_archive_file_size",
    "znippy_archive_extract_file", "znippy_archive_extract_file_verified", "znippy_archive_read_range", "znippy_archive_read_range_verified", "znippy_archive_block_tree_stats", "znippy_archive_extract_zip_entries", "znippy_archive_extract_tar_members", "znippy_archive_gunzip_files", "znippy_archive_bunzip2_files", "znippy_archive_unxz_files", "znippy_archive_list_tar_members", "znippy_zip_end_of_directory", "znippy_zip_find_entry", "znippy_zip_local_data_offset", "znippy_archive_close", "znippy_index_open", "znippy_index_rows",
    "znippy_index_manifest_len", "znippy_index_manifest_entry", "znippy_index_row", "znippy_index_metadata",
    "znippy_index_close", "znippy_interpret_footer", "znippy_write_manifest_bytes",
]

_L = None


def lib():
    global _L
    if _L is None:
        L = _lib.lib()
        L.znippy_host_last_error.restype = C.c_char_p
        L.znippy_compress_stream.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
        L.znippy_stream_send.argtypes = [vp, C.c_char_p, vp, C.c_size_t, C.c_int, C.c_char_p]
        L.znippy_stream_send_packed.argtypes = [vp, C.c_uint64, vp, vp, vp, vp, vp, C.c_char_p]
        L.znippy_stream_finish.argtypes = [vp, C.POINTER(_CR)]
        L.znippy_compress_dir.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(_CR)]
        L.znippy_decompress_archive.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32,
                                                C.POINTER(_VR), vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.znippy_archive_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
        L.znippy_archive_file_count.argtypes = [vp]
        L.znippy_archive_file_count.restype = C.c_uint64
        L.znippy_archive_file_size.argtypes = [vp, C.c_char_p]
        L.znippy_archive_file_size.restype = C.c_int64
        L.znippy_archive_extract_file.argtypes = [vp, C.c_char_p, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.znippy_archive_extract_file_verified.argtypes = [vp, C.c_char_p, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.znippy_archive_read_range.argtypes = [vp, C.c_char_p, C.c_uint64, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.znippy_archive_read_range_verified.argtypes = [vp, C.c_char_p, C.c_uint64, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.znippy_archive_block_tree_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.znippy_archive_close.argtypes = [vp]
        L.znippy_archive_extract_zip_entries.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint64, C.c_char_p, C.c_char_p, vp, C.c_size_t, vp, vp]
        L.znippy_archive_extract_tar_members.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint64, C.c_char_p, C.c_char_p, C.c_uint64, vp, C.c_size_t, vp, vp]
        L.znippy_archive_gunzip_files.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint64, vp, C.c_size_t, vp, vp]
        if hasattr(L, "znippy_archive_bunzip2_files"):  # (a library built before the call existed still loads)
            L.znippy_archive_bunzip2_files.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint64, vp, C.c_size_t, vp, vp]
        if hasattr(L, "znippy_archive_unxz_files"):  # (likewise)
            L.znippy_archive_unxz_files.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint64, vp, C.c_size_t, vp, vp]
        if hasattr(L, "znippy_archive_list_tar_members"):  # (likewise)
            L.znippy_archive_list_tar_members.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint64, C.c_char_p, C.c_char_p, vp, C.c_uint64, vp, C.c_uint64, vp,
                                                          C.c_size_t, vp, vp, vp, vp]
        L.znippy_zip_end_of_directory.argtypes = [vp, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.znippy_zip_find_entry.argtypes = [vp, C.c_size_t, C.c_uint64, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, vp]
        L.znippy_zip_local_data_offset.argtypes = [vp, C.c_size_t, C.POINTER(C.c_uint64)]
        L.znippy_archive_close.restype = None
        L.znippy_index_open.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.znippy_index_rows.argtypes = [vp]
        L.znippy_index_rows.restype = C.c_uint64
        L.znippy_index_manifest_len.argtypes = [vp]
        L.znippy_index_manifest_len.restype = C.c_uint64
        L.znippy_index_manifest_entry.argtypes = [vp, C.c_uint64, C.POINTER(_ME)]
        L.znippy_index_row.argtypes = [vp, C.c_uint64, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64), C.POINTER(C.POINTER(C.c_uint8))]
        L.znippy_index_metadata.argtypes = [vp, C.c_char_p]
        L.znippy_index_metadata.restype = C.c_char_p
        L.znippy_index_close.argtypes = [vp]
        L.znippy_index_close.restype = None
        L.znippy_interpret_footer.argtypes = [vp, C.c_size_t, C.POINTER(C.c_uint64)]
        L.znippy_write_manifest_bytes.argtypes = [C.POINTER(_ME), C.c_size_t, vp, C.c_size_t]
        L.znippy_write_manifest_bytes.restype = C.c_size_t
        _L = L
    return _L


class HostError(RuntimeError):
    pass


def _chk(rc, what):
    if rc:
        raise HostError(f"{what}: rc={rc} {lib().znippy_host_last_error().decode()}")


class StreamCompressor:
    """compress_stream(&output, no_skip) on the compiled host layer."""

    def __init__(self, output, no_skip=False, device=0):
        self.h = vp()
        _chk(lib().znippy_compress_stream(str(output).encode(), int(no_skip), device, C.byref(self.h)), "compress_stream")

    def sender(self):
        return self

    def send(self, entry):
        data = bytes(entry.data)
        _chk(lib().znippy_stream_send(self.h, entry.relative_path.encode(), data, len(data),
                                      -1 if entry.pkg_type is None else int(entry.pkg_type),
                                      None if entry.repo is None else entry.repo.encode()), "stream_send")

    def send_packed(self, paths, data, data_off, pkg_type=None, repo=None):
        """n entries in one call: `paths` a list of str, `data` one contiguous buffer (bytes / numpy uint8), `data_off`
        n + 1 offsets into it.  The per-entry work (chunking, the one copy into staging) is the same as send()'s; what goes
        away is n trips through the binding."""
        import numpy as np
        enc = [p.encode() for p in paths]
        n = len(enc)
        poff = np.zeros(n + 1, np.uint64)
        np.cumsum([len(p) for p in enc], out=poff[1:])
        pblob = b"".join(enc)
        doff = np.ascontiguousarray(np.asarray(data_off, dtype=np.uint64))
        assert doff.size == n + 1
        buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        assert int(doff[-1]) <= buf.size
        pk = None if pkg_type is None else np.ascontiguousarray(np.asarray(pkg_type, dtype=np.int32))
        _chk(lib().znippy_stream_send_packed(self.h, n, pblob, poff.ctypes.data_as(vp), buf.ctypes.data_as(vp), doff.ctypes.data_as(vp),
                                             None if pk is None else pk.ctypes.data_as(vp),
                                             None if repo is None else repo.encode()), "stream_send_packed")

    def finish(self) -> ix.CompressionReport:
        r = _CR()
        h, self.h = self.h, None
        _chk(lib().znippy_stream_finish(h, C.byref(r)), "stream_finish")
        return _report(r)


def _report(r) -> ix.CompressionReport:
    return ix.CompressionReport(**{n: (float(getattr(r, n)) if n == "compression_ratio" else int(getattr(r, n)))
                                   for n, _ in _CR._fields_})


def compress_stream(output, no_skip=False, device=0):
    return StreamCompressor(output, no_skip, device)


def compress_dir(input_dir, output, no_skip=False, plugin=None, repo=None, device=0) -> ix.CompressionReport:
    """compress_dir(&input_dir, &output, no_skip, plugin, repo) on the compiled host layer."""
    if plugin is not None:
        raise NotImplementedError("metadata plugins are outside the hot path (SURVEY §2 #12)")
    r = _CR()
    _chk(lib().znippy_compress_dir(str(input_dir).encode(), str(output).encode(), int(no_skip),
                                   None if repo is None else repo.encode(), device, C.byref(r)), "compress_dir")
    return _report(r)


def decompress_archive(index_path, save_data, out_dir, device=0, rank=0, world=1) -> ix.VerifyReport:
    r = _VR()
    cap = 1 << 16
    corrupt = np.zeros(cap, dtype=np.uint64)
    n = C.c_uint64()
    _chk(lib().znippy_decompress_archive(str(index_path).encode(), int(save_data), str(out_dir).encode(), device, rank,
                                         world, C.byref(r), corrupt.ctypes.data_as(vp), cap, C.byref(n)), "decompress_archive")
    return ix.VerifyReport(**{k: int(getattr(r, k)) for k, _ in _VR._fields_},
                           corrupt_rows=[int(x) for x in corrupt[:min(n.value, cap)]])


class ZnippyArchive:
    def __init__(self, path, device=0):
        self.h = vp()
        _chk(lib().znippy_archive_open(str(path).encode(), device, C.byref(self.h)), "archive_open")

    @classmethod
    def open(cls, path, device=0):
        return cls(path, device)

    def file_count(self):
        return int(lib().znippy_archive_file_count(self.h))

    def contains(self, rel):
        return lib().znippy_archive_file_size(self.h, rel.encode()) >= 0

    def file_size(self, rel):
        s = lib().znippy_archive_file_size(self.h, rel.encode())
        return None if s < 0 else int(s)

    def extract_file(self, rel, verify=False) -> bytes:
        """verify=True: every chunk's BLAKE3 is checked against the index (the reference has no such option)."""
        size = self.file_size(rel)
        if size is None:
            raise KeyError(f"file not found in archive: {rel}")
        buf = np.empty(max(size, 1), dtype=np.uint8)
        w = C.c_size_t()
        f = lib().znippy_archive_extract_file_verified if verify else lib().znippy_archive_extract_file
        _chk(f(self.h, rel.encode(), buf.ctypes.data_as(vp), size, C.byref(w)), "extract_file")
        return buf[:w.value].tobytes()

    def read_range(self, rel, offset, length) -> bytes:
        """pread on an archived file: clamped at its end, b"" at or past it; only the touched chunks are read and, of a
        chunk this library wrote, only the blocks the range overlaps are decoded."""
        if not self.contains(rel):
            raise KeyError(f"file not found in archive: {rel}")
        buf = np.empty(max(int(length), 1), dtype=np.uint8)
        w = C.c_size_t()
        _chk(lib().znippy_archive_read_range(self.h, rel.encode(), int(offset), buf.ctypes.data_as(vp), int(length), C.byref(w)),
             "read_range")
        return buf[:w.value].tobytes()

    def read_range_verified(self, rel, offset, length) -> bytes:
        """read_range where every byte returned was covered by a hash that chains to the index checksum: block by block
        (128 KiB) once the handle has built a chunk's block tree, which the first verified read of the chunk does.  A
        mismatch raises with ZNIPPY_E_CHECKSUM."""
        if not self.contains(rel):
            raise KeyError(f"file not found in archive: {rel}")
        buf = np.empty(max(int(length), 1), dtype=np.uint8)
        w = C.c_size_t()
        _chk(lib().znippy_archive_read_range_verified(self.h, rel.encode(), int(offset), buf.ctypes.data_as(vp), int(length), C.byref(w)),
             "read_range_verified")
        return buf[:w.value].tobytes()

    def extract_zip_entries(self, paths, suffix, prefix="", cap=None):
        """For every archived ZIP container of `paths` (jars, wars, wheels): the content of its first entry whose name starts with
        `prefix` and ends with `suffix` — what the reference's ingest plugins ask of ljar::decompress_jar_filter per container, for
        all of them in one batch: three range-read passes (tails, central directories, local headers + compressed bytes), one
        upload, one znippy_inflate_batch against the directories' CRC-32s, one copy back.  cap: bytes of the result buffer of the
        one call made.  None: the first call gets 16 KiB per file + 1 MiB, and the files that did not fit (ZNIPPY_E_DST_SMALL) go
        through the call again with eight times the room, until they fit or the room is what DEFLATE can expand their containers
        to.  Returns (list of bytes, or None where the status is not 0; statuses: 0 or ZNIPPY_E_*)."""
        paths = [str(p) for p in paths]
        n = len(paths)
        out, status = [None] * n, [0] * n
        todo = list(range(n))
        room = int(cap) if cap is not None else (16 << 10) * n + (1 << 20)
        while todo:
            m = len(todo)
            arr = (C.c_char_p * m)(*[paths[i].encode() for i in todo])
            buf = np.empty(max(room, 1), dtype=np.uint8)
            off = np.zeros(m + 1, dtype=np.uint64)
            st = np.zeros(m, dtype=np.int32)
            _chk(lib().znippy_archive_extract_zip_entries(self.h, arr, m, prefix.encode(), suffix.encode(), buf.ctypes.data_as(vp), room,
                                                          off.ctypes.data_as(vp), st.ctypes.data_as(vp)), "extract_zip_entries")
            again = []
            for k, i in enumerate(todo):
                status[i] = int(st[k])
                if st[k] == 0:
                    out[i] = buf[int(off[k]):int(off[k + 1])].tobytes()
                elif st[k] == _lib.E_DST_SMALL:
                    again.append(i)
            # (DEFLATE expands at most 1032-fold: more room than that for the containers left cannot help)
            most = sum(1032 * (self.file_size(paths[i]) or 0) + 64 for i in again)
            if cap is not None or room >= most:
                break
            todo, room = again, min(8 * room, most)
        return out, status

    def extract_tar_members(self, paths, suffix, prefix="", scan_cap=8 << 20, cap=None):
        """For every archived gzip-compressed tar of `paths` (.crate files, .tar.gz sdists): the content of its first regular member
        whose name starts with `prefix` and ends with `suffix` — the Cargo.toml of a batch of crates — found on the device: the first
        64 KiB of every file (ZNIPPY_HOST_TARGZ_HEAD overrides) are gathered there and inflated only until the tar answers, the files
        whose head did not hold the answer go through once more whole, and only the members come back.  scan_cap: the most inflated
        bytes one file may take.  cap: bytes of the result buffer of the one call made.  None: the first call gets 16 KiB per file +
        1 MiB, and the files that did not fit (ZNIPPY_E_DST_SMALL) go through the call again with eight times the room, until they
        fit or the room is what scan_cap lets them come to.  Returns (list of bytes, or None where the status is not 0; statuses)."""
        paths = [str(p) for p in paths]
        n = len(paths)
        out, status = [None] * n, [0] * n
        todo = list(range(n))
        room = int(cap) if cap is not None else (16 << 10) * n + (1 << 20)
        while todo:
            m = len(todo)
            arr = (C.c_char_p * m)(*[paths[i].encode() for i in todo])
            buf = np.empty(max(room, 1), dtype=np.uint8)
            off = np.zeros(m + 1, dtype=np.uint64)
            st = np.zeros(m, dtype=np.int32)
            _chk(lib().znippy_archive_extract_tar_members(self.h, arr, m, prefix.encode(), suffix.encode(), int(scan_cap), buf.ctypes.data_as(vp), room,
                                                          off.ctypes.data_as(vp), st.ctypes.data_as(vp)), "extract_tar_members")
            again = []
            for k, i in enumerate(todo):
                status[i] = int(st[k])
                if st[k] == 0:
                    out[i] = buf[int(off[k]):int(off[k + 1])].tobytes()
                elif st[k] == _lib.E_DST_SMALL:
                    again.append(i)
            most = sum(min(int(scan_cap), 1032 * (self.file_size(paths[i]) or 0) + 512) for i in again)
            if cap is not None or room >= most:
                break
            todo, room = again, min(8 * room, most)
        return out, status

    def gunzip_files(self, paths, cap=None):
        """The whole content of every archived gzip file of `paths` (.gz logs, .tar.gz sdists, .crate files, BGZF files), all members
        concatenated, inflated on the device in one batch: the files are gathered there whole, their rooms come from each file's ISIZE
        (its last four bytes), members and flush segments are decoded in parallel and every member's CRC-32 and ISIZE are checked; a
        file of several members goes through again with eight times the room.  cap: bytes of the result buffer of the one call made.
        None: the first call gets four times the files' sizes + 1 MiB, and the files that did not fit (ZNIPPY_E_DST_SMALL) go through
        the call again with eight times the room, until they fit or the room is what DEFLATE can expand them to.  Returns (list of
        bytes, or None where the status is not 0; statuses)."""
        paths = [str(p) for p in paths]
        n = len(paths)
        out, status = [None] * n, [0] * n
        todo = list(range(n))
        room = int(cap) if cap is not None else 4 * sum(self.file_size(p) or 0 for p in paths) + (1 << 20)
        while todo:
            m = len(todo)
            arr = (C.c_char_p * m)(*[paths[i].encode() for i in todo])
            buf = np.empty(max(room, 1), dtype=np.uint8)
            off = np.zeros(m + 1, dtype=np.uint64)
            st = np.zeros(m, dtype=np.int32)
            _chk(lib().znippy_archive_gunzip_files(self.h, arr, m, buf.ctypes.data_as(vp), room, off.ctypes.data_as(vp), st.ctypes.data_as(vp)),
                 "gunzip_files")
            again = []
            for k, i in enumerate(todo):
                status[i] = int(st[k])
                if st[k] == 0:
                    out[i] = buf[int(off[k]):int(off[k + 1])].tobytes()
                elif st[k] == _lib.E_DST_SMALL:
                    again.append(i)
            most = sum(1032 * (self.file_size(paths[i]) or 0) + 512 for i in again)
            if cap is not None or room >= most:
                break
            todo, room = again, min(8 * room, most)
        return out, status

    def bunzip2_files(self, paths, cap=None):
        """The whole content of every archived bzip2 file of `paths` (.bz2, .tar.bz2, .tbz, .tbz2), all streams concatenated,
        decoded on the device in one batch: the files are gathered there whole, a measuring pass gives their rooms (bzip2 names no
        size), then their blocks are decoded in parallel and every block CRC and combined CRC is checked.  cap: bytes of the result
        buffer.  None: the sizes are measured first (a call without a buffer) and the buffer holds exactly the clean files.  Returns
        (list of bytes, or None where the status is not 0; statuses)."""
        return self._measured_files(lib().znippy_archive_bunzip2_files, "bunzip2_files", paths, cap)

    def unxz_files(self, paths, cap=None):
        """The whole content of every archived xz file of `paths` (.xz, .tar.xz, .txz), all streams concatenated, decoded on the
        device in one batch: the files are gathered there whole, a measuring pass reads the sizes their indexes claim, then every
        block of every file is decoded in one launch, a wave per block, and CRC32 and CRC64 checks are verified (blocks with no
        check or SHA-256 are delivered unverified).  cap: as in bunzip2_files.  Returns (list of bytes, or None where the status
        is not 0; statuses)."""
        return self._measured_files(lib().znippy_archive_unxz_files, "unxz_files", paths, cap)

    def _measured_files(self, call, what, paths, cap):
        paths = [str(p) for p in paths]
        n = len(paths)
        arr = (C.c_char_p * n)(*[p.encode() for p in paths])
        off = np.zeros(n + 1, dtype=np.uint64)
        st = np.zeros(max(n, 1), dtype=np.int32)
        if cap is None:
            _chk(call(self.h, arr, n, None, 0, off.ctypes.data_as(vp), st.ctypes.data_as(vp)), what)
            cap = int(off[n])
        room = int(cap)
        buf = np.empty(max(room, 1), dtype=np.uint8)
        _chk(call(self.h, arr, n, buf.ctypes.data_as(vp), room, off.ctypes.data_as(vp), st.ctypes.data_as(vp)), what)
        out = [buf[int(off[i]):int(off[i + 1])].tobytes() if st[i] == 0 else None for i in range(n)]
        return out, [int(v) for v in st[:n]]

    def list_tar_members(self, paths, suffix=b"", prefix=b"", contents=False, cap=None):
        """Every regular member of the tar in every archived file of `paths` (.tar, .tar.gz / .tgz / .crate, .tar.bz2, .tar.xz / .txz) whose name starts
        with `prefix` and ends with `suffix` (bytes without NUL; empty = all), listed on the device in one batch: the files are gathered
        there whole, gzip, bzip2 and xz files are decompressed there (chosen by their first bytes), and one znippy_tar_list_batch walks all
        the tars.  contents: the members' bytes come back as well.  cap: bytes of the buffer for the contents.  None: the tars are
        measured first (a call without buffers) and the buffers hold exactly what is listed.  Returns, per file,
        (status, [(name, size, bytes | None), ...]); a file whose status is not 0 lists nothing."""
        from .hip import TAR_MEMBER
        paths = [str(p) for p in paths]
        n = len(paths)
        arr = (C.c_char_p * n)(*[p.encode() for p in paths])
        prefix, suffix = bytes(prefix), bytes(suffix)
        first = np.zeros(n + 1, dtype=np.uint64)
        st = np.zeros(max(n, 1), dtype=np.int32)
        nb, ob = C.c_uint64(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data_as(vp)  # noqa: E731
        _chk(lib().znippy_archive_list_tar_members(self.h, arr, n, prefix, suffix, None, 0, None, 0, None, 0, ptr(first), C.byref(nb), C.byref(ob), ptr(st)),
             "list_tar_members")
        members = np.zeros(max(int(first[n]), 1), dtype=TAR_MEMBER)
        names = np.zeros(max(nb.value, 1), dtype=np.uint8)
        room = (ob.value if cap is None else int(cap)) if contents else 0
        buf = np.empty(max(room, 1), dtype=np.uint8) if contents else None
        _chk(lib().znippy_archive_list_tar_members(self.h, arr, n, prefix, suffix, ptr(members), int(first[n]), ptr(names), nb.value,
                                                   ptr(buf) if contents else None, room, ptr(first), C.byref(nb), C.byref(ob), ptr(st)), "list_tar_members")
        nm = names.tobytes()
        out = []
        for i in range(n):
            ms = []
            for m in members[int(first[i]):int(first[i + 1])]:
                no, oo, size = int(m["name_off"]), int(m["out_off"]), int(m["size"])
                ms.append((nm[no:no + int(m["name_len"])], size, buf[oo:oo + size].tobytes() if contents else None))
            out.append((int(st[i]), ms))
        return out

    def block_tree_stats(self):
        """[entries loaded from the sidecar `<path>.b3t` at open, chunks whose sidecar entries were accepted, chunks whose
        sidecar entries were rejected, chunks whose block tree was built by a whole decode]."""
        st = (C.c_uint64 * 4)()
        _chk(lib().znippy_archive_block_tree_stats(self.h, st), "block_tree_stats")
        return [int(v) for v in st]

    def close(self):
        if self.h:
            lib().znippy_archive_close(self.h)
            self.h = None

    __del__ = close


def read_index(path):
    """-> (rows: list of dicts, manifest: list[ManifestEntry], metadata getter) via the C++ Arrow IPC reader."""
    h = vp()
    _chk(lib().znippy_index_open(str(path).encode(), C.byref(h)), "index_open")
    try:
        L = lib()
        rows = []
        for i in range(L.znippy_index_rows(h)):
            p = C.c_char_p(); seq = C.c_uint32(); fo = C.c_uint64(); cm = C.c_int(); us = C.c_uint64()
            bo = C.c_uint64(); bs = C.c_uint64(); ck = C.POINTER(C.c_uint8)()
            L.znippy_index_row(h, i, C.byref(p), C.byref(seq), C.byref(fo), C.byref(cm), C.byref(us), C.byref(bo),
                               C.byref(bs), C.byref(ck))
            rows.append(dict(relative_path=p.value.decode(), chunk_seq=seq.value, fdata_offset=fo.value,
                             compressed=bool(cm.value), uncompressed_size=us.value, blob_offset=bo.value,
                             blob_size=bs.value, checksum=bytes(ck[:32])))
        manifest = []
        for i in range(L.znippy_index_manifest_len(h)):
            e = _ME()
            L.znippy_index_manifest_entry(h, i, C.byref(e))
            manifest.append(ix.ManifestEntry(e.pkg_type, e.repo.decode(), e.module_name.decode(), e.index_offset,
                                             e.index_len, e.row_count))
        keys = ["znippy_format_version", "max_core_in_flight", "max_core_in_compress", "max_mem_allowed",
                "min_free_memory_ratio", "file_split_block_size", "max_chunks", "compression_level",
                "zstd_output_buffer_size", "checksum_group_0"]
        md = {}
        for k in keys:
            v = L.znippy_index_metadata(h, k.encode())
            if v is not None:
                md[k] = v.decode()
        return rows, manifest, md
    finally:
        lib().znippy_index_close(h)


def write_manifest_bytes(entries) -> bytes:
    arr = (_ME * max(len(entries), 1))()
    keep = []
    for i, e in enumerate(entries):
        r, m = e.repo.encode(), e.module_name.encode()
        keep += [r, m]
        arr[i] = _ME(e.pkg_type, r, m, e.index_offset, e.index_len, e.row_count)
    n = lib().znippy_write_manifest_bytes(arr, len(entries), None, 0)
    buf = np.zeros(n, dtype=np.uint8)
    lib().znippy_write_manifest_bytes(arr, len(entries), buf.ctypes.data_as(vp), n)
    return buf.tobytes()


def interpret_footer(tail: bytes):
    off = C.c_uint64()
    multi = lib().znippy_interpret_footer(tail, len(tail), C.byref(off))
    return ("multi" if multi else "single", off.value)
