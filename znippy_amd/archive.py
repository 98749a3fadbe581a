"""ZnippyArchive — host-side mirror of znippy-common/src/archive.rs (random-access reads).

open() loads only the index; extract_file(path) preads that file's blobs, decodes compressed
chunks on the GPU and concatenates them in fdata_offset order.  Like the reference, no checksum
verification happens on this path by default (archive.rs:L144-168); `verify=True` adds the check the
reference lacks: every chunk's BLAKE3 against the index's checksum column."""
import os

import numpy as np

from . import index as ix
from .decompress import _columns, read_spans, row_lengths


class ZnippyArchive:
    def __init__(self, path, backend=None):
        self.path = str(path)
        self._backend = backend
        _, batches = ix.read_znippy_index(self.path)
        c = _columns(batches)
        self._c = c
        self._rlen = row_lengths(c)
        self.file_index = {}
        for row, p in enumerate(c["paths"]):
            self.file_index.setdefault(p, []).append(row)
        for p, rows in self.file_index.items():  # chunks sorted by fdata_offset (L131-133)
            rows.sort(key=lambda r: int(c["fdata_offset"][r]))

    @classmethod
    def open(cls, path, backend=None):
        return cls(path, backend)

    def file_count(self):
        return len(self.file_index)

    def list_files(self):
        return list(self.file_index.keys())

    def contains(self, relative_path):
        return relative_path in self.file_index

    def file_size(self, relative_path):
        rows = self.file_index.get(relative_path)
        return None if rows is None else int(sum(int(self._c["usize"][r]) for r in rows))

    def extract_file(self, relative_path, verify=False) -> bytes:
        out = self.extract_files([relative_path], verify=verify)[0]
        if isinstance(out, Exception):
            raise out
        return out

    def extract_files(self, paths, verify=False):
        """Batch extract: all requested files' chunks go to the GPU as one row set.  Only the requested rows' blobs
        are read (rows that sit next to each other in the archive in one read), not the span between them."""
        from .backend import default_backend
        c = self._c
        rows, spans, results = [], [], []
        for p in paths:
            r = self.file_index.get(p)
            if r is None:
                spans.append(None)
                continue
            spans.append((len(rows), len(rows) + len(r)))
            rows.extend(r)
        if rows:
            rows_np = np.asarray(rows)
            bs, usz = c["blob_size"][rows_np], self._rlen[rows_np]
            with open(self.path, "rb") as f:
                blobs, bo = read_spans(f, os.path.getsize(self.path), c["blob_offset"][rows_np], bs)
            out_off = np.concatenate([[0], np.cumsum(usz)[:-1]]).astype(np.uint64)
            backend = self._backend or default_backend()
            # an unverified extract never looks at the checksum column (archive.rs:L144-168): a decode-only run, which does not hash
            # (ZNIPPY_NO_DECODE_ONLY=1 in the environment: the decode + verify run without a checksum, as before — for A/B runs)
            if not verify and hasattr(backend, "decode") and os.environ.get("ZNIPPY_NO_DECODE_ONLY", "0") in ("", "0"):
                _, corrupt, status, out = backend.decode(blobs, 0, bo, bs, usz, out_off, c["compressed"][rows_np], int(usz.sum()))
            else:
                _, corrupt, status, out = backend.decode_verify(blobs, 0, bo, bs, usz, out_off, c["compressed"][rows_np],
                                                                c["checksum"][rows_np] if verify else None, int(usz.sum()))
            corrupt = set(int(x) for x in corrupt)
        for p, sp in zip(paths, spans):
            if sp is None:
                results.append(KeyError(f"file not found in archive: {p}"))
                continue
            a, b = sp
            if (status[a:b] < 0).any():
                results.append(ValueError(f"decompress failed for {p}: status {int(status[a:b].min())}"))
                continue
            if verify and any(k in corrupt for k in range(a, b)):
                results.append(ValueError(f"checksum mismatch in {p}"))
                continue
            start = int(out_off[a])
            end = int(out_off[b - 1] + usz[b - 1])
            results.append(out[start:end].tobytes())
        return results

    def read_range(self, relative_path, offset, length) -> bytes:
        """pread on an archived file: bytes [offset, offset + length) of it, clamped at its end (an offset at or past the
        end gives b"").  Only the chunks the range touches are read from disk, and of a chunk this library wrote only the
        128 KiB blocks it overlaps are decoded.  No checksum is looked at, as for extract_file."""
        out = self.read_ranges([(relative_path, offset, length)])[0]
        if isinstance(out, Exception):
            raise out
        return out

    def read_ranges(self, requests):
        """Batch of (relative_path, offset, length): every request's chunk pieces go to the backend as one call.  An
        unknown path gives a KeyError in its place, a chunk that fails to decode a ValueError."""
        from .backend import default_backend
        c = self._c
        chunk_rows, chunk_at = [], {}  # archive rows the requests touch, in first-touch order; archive row -> its place there
        rr, rb, rl, spans = [], [], [], []
        for p, offset, length in requests:
            rows = self.file_index.get(p)
            if rows is None:
                spans.append(None)
                continue
            offset, length = int(offset), int(length)
            if offset < 0 or length < 0:
                raise ValueError(f"negative offset or length for {p}")
            first = len(rr)
            for row in rows:  # (sorted by fdata_offset)
                lo, n = int(c["fdata_offset"][row]), int(self._rlen[row])
                a, b = max(offset, lo), min(offset + length, lo + n)
                if a >= b:
                    continue
                if row not in chunk_at:
                    chunk_at[row] = len(chunk_rows)
                    chunk_rows.append(row)
                rr.append(chunk_at[row]); rb.append(a - lo); rl.append(b - a)
            spans.append((first, len(rr)))
        status = np.zeros(0, np.int32)
        pieces = []
        if rr:
            rows_np = np.asarray(chunk_rows)
            bs, usz, comp = c["blob_size"][rows_np], self._rlen[rows_np], c["compressed"][rows_np]
            with open(self.path, "rb") as f:
                blobs, bo = read_spans(f, os.path.getsize(self.path), c["blob_offset"][rows_np], bs)
            rr, rb, rl = np.asarray(rr, np.uint64), np.asarray(rb, np.uint64), np.asarray(rl, np.uint64)
            backend = self._backend or default_backend()
            if hasattr(backend, "read_ranges"):
                status, out, _ = backend.read_ranges(blobs, 0, bo, bs, usz, comp, rr, rb, rl)
                at = np.concatenate([[0], np.cumsum(rl)]).astype(np.uint64)
                pieces = [out[int(at[i]):int(at[i + 1])] for i in range(len(rr))]
            else:  # a backend without range reads: the touched chunks decoded whole, then sliced
                out_off = np.concatenate([[0], np.cumsum(usz)[:-1]]).astype(np.uint64)
                if hasattr(backend, "decode"):
                    _, _, st, out = backend.decode(blobs, 0, bo, bs, usz, out_off, comp, int(usz.sum()))
                else:
                    _, _, st, out = backend.decode_verify(blobs, 0, bo, bs, usz, out_off, comp, None, int(usz.sum()))
                status = np.asarray(st)[rr.astype(np.int64)]
                pieces = [out[int(out_off[int(k)] + b):int(out_off[int(k)] + b + n)] for k, b, n in zip(rr, rb, rl)]
        results = []
        for (p, _, _), sp in zip(requests, spans):
            if sp is None:
                results.append(KeyError(f"file not found in archive: {p}"))
                continue
            a, b = sp
            if b > a and (status[a:b] < 0).any():
                results.append(ValueError(f"range read failed for {p}: status {int(status[a:b].min())}"))
                continue
            results.append(b"".join(x.tobytes() for x in pieces[a:b]))
        return results
