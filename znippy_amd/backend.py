"""The device backend the host-side pipelines drive: host buffers in, host buffers out, all
compute through libznippy_hip.so (C ABI).  There is no CPU implementation in the product; the
CPU tests inject a checker double from tests/ to exercise the host logic without a GPU."""
import numpy as np


class HipBackend:
    def __init__(self, device=None, ctx=None):
        import torch
        from . import hip
        if not torch.cuda.is_available():
            raise RuntimeError("znippy_amd: no GPU visible — the codec/hash path has no CPU fallback")
        self.torch = torch
        self.hip = hip
        self.device = torch.cuda.current_device() if device is None else device
        self.ctx = ctx or hip.Context(self.device)
        self.blob_align = 1

    def set_level(self, level):
        """CompressCtx::new(compression_level), codec.rs:L16-28."""
        self.ctx.set_level(level)

    def set_window_log(self, window_log):
        """Cross-block match window of later encode calls (0 = off, 17..27; znippy_ctx_set_window_log)."""
        self.ctx.set_window_log(window_log)

    def set_batch_checksums(self, on):
        """Frames with a content checksum through the batch path of later read runs (0 = off; znippy_ctx_set_batch_checksums)."""
        self.ctx.set_batch_checksums(on)

    def set_gunzip_cut(self, cut_bytes):
        """Later gunzip calls cut files without flush points at found block starts (0 = off, 64 .. 2^30 source bytes per kept
        candidate; znippy_ctx_set_gunzip_cut)."""
        self.ctx.set_gunzip_cut(cut_bytes)

    @property
    def gunzip_cut(self):
        return self.ctx.gunzip_cut

    def gunzip_cut_stats(self):
        """The counters of the context's last gunzip call (znippy_ctx_gunzip_cut_stats)."""
        return self.ctx.gunzip_cut_stats()

    def set_blob_align(self, align):
        """Blob offsets of later encode_hash calls are multiples of `align` inside their region (a power of two, 1 .. 4096;
        znippy_rounds_set_blob_align on every table built from here on)."""
        self.blob_align = check_blob_align(align)

    def _to_dev(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a))
        return t.to(f"cuda:{self.device}", non_blocking=False)

    # write side: Rounds over one staging buffer -> packed blobs + per-round metadata
    def encode_hash(self, staging, off, length, skip):
        n = len(off)
        if n == 0:
            return dict(blob_offset=np.zeros(0, np.uint64), blob_size=np.zeros(0, np.uint64),
                        checksum=np.zeros((0, 32), np.uint8), compressed=np.zeros(0, np.uint8)), np.zeros(0, np.uint8)
        d_src = self._to_dev(np.concatenate([staging, np.zeros(64, np.uint8)]))
        rt = self.hip.RoundTable(self.ctx, off, length, skip)
        if self.blob_align > 1:
            rt.set_blob_align(self.blob_align)
        d_blob = self.torch.empty(rt.blob_bound() + 64, dtype=self.torch.uint8, device=f"cuda:{self.device}")
        res = rt.encode_hash(d_src, d_blob)
        res = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in res.items()}  # views die with the table
        blob = d_blob[:res["blob_bytes"]].cpu().numpy()
        rt.close()
        return res, blob

    # read side: rows of the index over a blob region -> decoded bytes + counters
    def decode_verify(self, blobs, blob_base, blob_offset, blob_size, usize, out_offset, compressed, checksum, out_total):
        n = len(blob_offset)
        if n == 0:
            return dict(total_chunks=0, total_written_bytes=0, verified_bytes=0, corrupt_bytes=0, corrupt_rows=0,
                        decode_errors=0), np.zeros(0, np.uint64), np.zeros(0, np.int32), np.zeros(0, np.uint8)
        d_blobs = self._to_dev(np.concatenate([blobs, np.zeros(64, np.uint8)]))
        d_out = self.torch.empty(out_total + 64, dtype=self.torch.uint8, device=f"cuda:{self.device}")
        bitmap = np.packbits(np.asarray(compressed, dtype=bool), bitorder="little")
        rt = self.hip.RowTable(self.ctx, blob_offset, blob_size, usize, out_offset, bitmap, checksum)
        counters, corrupt, status = rt.decode_verify(d_blobs, d_out, blob_base=blob_base, out_cap=out_total,
                                                     blob_cap=len(blobs))
        out = d_out[:out_total].cpu().numpy()
        rt.close()
        return counters, corrupt, status, out

    # read side, decode only (the extract path, archive.rs:L144-168): the bytes, counters and status — nothing is hashed
    def decode(self, blobs, blob_base, blob_offset, blob_size, usize, out_offset, compressed, out_total):
        n = len(blob_offset)
        if n == 0:
            return dict(total_chunks=0, total_written_bytes=0, verified_bytes=0, corrupt_bytes=0, corrupt_rows=0,
                        decode_errors=0), np.zeros(0, np.uint64), np.zeros(0, np.int32), np.zeros(0, np.uint8)
        d_blobs = self._to_dev(np.concatenate([blobs, np.zeros(64, np.uint8)]))
        d_out = self.torch.empty(out_total + 64, dtype=self.torch.uint8, device=f"cuda:{self.device}")
        bitmap = np.packbits(np.asarray(compressed, dtype=bool), bitorder="little")
        rt = self.hip.RowTable(self.ctx, blob_offset, blob_size, usize, out_offset, bitmap, None)
        counters, status = rt.decode(d_blobs, d_out, blob_base=blob_base, out_cap=out_total, blob_cap=len(blobs))
        status = status.copy()  # (a view of the table's host buffer)
        out = d_out[:out_total].cpu().numpy()
        rt.close()
        return counters, np.zeros(0, np.uint64), status, out

    # read side, byte ranges of rows (znippy_rows_read_ranges): range i is bytes [range_begin[i], + range_len[i]) of row range_row[i] of the
    # given columns.  -> (status per range, the ranges' bytes packed back to back in array order, content bytes the decoders produced)
    def read_ranges(self, blobs, blob_base, blob_offset, blob_size, usize, compressed, range_row, range_begin, range_len):
        n = len(range_row)
        if n == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.uint8), 0
        total = sum(int(x) for x in range_len)  # (a table without rows included: the call rules on every range)
        d_blobs = self._to_dev(np.concatenate([blobs, np.zeros(64, np.uint8)]))
        d_out = self.torch.empty(total + 64, dtype=self.torch.uint8, device=f"cuda:{self.device}")
        bitmap = np.packbits(np.asarray(compressed, dtype=bool), bitorder="little")
        rt = self.hip.RowTable(self.ctx, blob_offset, blob_size, usize, None, bitmap, None)
        status, decoded = rt.read_ranges(d_blobs, range_row, range_begin, range_len, d_out, blob_base=blob_base, out_cap=total,
                                         blob_cap=len(blobs))
        out = d_out[:total].cpu().numpy()
        rt.close()
        return status, out, decoded

    # read side, verify only (decompress.rs save_data=false): counters, corrupt rows and status, no bytes — nothing is
    # allocated for an output and nothing comes back over the bus
    def verify(self, blobs, blob_base, blob_offset, blob_size, usize, compressed, checksum):
        n = len(blob_offset)
        if n == 0:
            return dict(total_chunks=0, total_written_bytes=0, verified_bytes=0, corrupt_bytes=0, corrupt_rows=0,
                        decode_errors=0), np.zeros(0, np.uint64), np.zeros(0, np.int32)
        d_blobs = self._to_dev(np.concatenate([blobs, np.zeros(64, np.uint8)]))
        bitmap = np.packbits(np.asarray(compressed, dtype=bool), bitorder="little")
        rt = self.hip.RowTable(self.ctx, blob_offset, blob_size, usize, None, bitmap, checksum)
        counters, corrupt, status = rt.verify(d_blobs, blob_base=blob_base, blob_cap=len(blobs))
        corrupt, status = corrupt.copy(), status.copy()  # (views of the table's host buffers)
        rt.close()
        return counters, corrupt, status


def apply_window_log(backend, window_log):
    """The pipelines' window_log keyword: set on every backend that has the setting (the CPU test double has not, and
    takes only 0)."""
    if hasattr(backend, "set_window_log"):
        backend.set_window_log(window_log)
    elif window_log:
        raise ValueError(f"backend {type(backend).__name__} has no cross-block window")


def check_blob_align(align):
    align = int(align)
    if not 1 <= align <= 4096 or align & (align - 1):
        raise ValueError(f"blob_align must be a power of two in 1..4096, not {align}")
    return align


def apply_blob_align(backend, blob_align):
    """The pipelines' blob_align keyword: set on every backend that has the setting; one that has not takes only 1."""
    blob_align = check_blob_align(blob_align)
    if hasattr(backend, "set_blob_align"):
        backend.set_blob_align(blob_align)
    elif blob_align > 1:
        raise ValueError(f"backend {type(backend).__name__} cannot align blob offsets")
    return blob_align


def round_up(v, align):
    return (int(v) + align - 1) // align * align


_default = None


def default_backend():
    global _default
    if _default is None:
        _default = HipBackend()
    return _default
