"""Object wrappers over the C ABI (include/znippy_hip.h).  Device buffers are torch uint8 CUDA
tensors (PyTorch-ROCm is only the allocator/stream provider); every compute call goes through
libznippy_hip.so."""
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import VerifyCounters, ZnippyError, as_np, np_ptr, vp


# znippy_tar_member of include/znippy_hip.h
TAR_MEMBER = np.dtype([("header_off", "<u8"), ("data_off", "<u8"), ("size", "<u8"), ("name_off", "<u8"), ("out_off", "<u8"), ("name_len", "<u4"),
                       ("typeflag", "<u4")])


def _pinned(shape, dtype):
    """Host result buffer; pinned when torch can (direct DMA on D2H), reused across calls."""
    try:
        import torch
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        t = torch.empty(max(n, 1), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        return t.numpy()[:n].view(dtype).reshape(shape), t
    except Exception:  # no torch / no pinning: plain numpy
        return np.zeros(shape, dtype=dtype), None


def _dptr(t):
    if t is None:
        return None
    if isinstance(t, int):
        return vp(t)
    assert t.is_cuda and t.is_contiguous(), "device buffers must be contiguous CUDA tensors"
    # The context runs on its own non-blocking stream: whatever torch still has queued on ITS stream for this
    # buffer (a torch.zeros fill, a copy) must have landed before our kernels touch it.
    import torch
    ts = torch.cuda.current_stream(t.device)
    if not ts.query():
        ts.synchronize()
    return vp(t.data_ptr())


class Context:
    """One per worker / GPU — the analogue of one CompressCtx per thread (codec.rs:L8-28)."""

    def __init__(self, device=0, stream=None):
        self.L = _lib.lib()
        h = vp()
        rc = self.L.znippy_ctx_create(int(device), vp(stream) if stream else None, C.byref(h))
        if rc:
            raise ZnippyError(rc, "znippy_ctx_create")
        self.h = h
        self.device = int(device)
        self._tables = weakref.WeakSet()  # row / round tables created on this context: they die before it does

    def close(self):
        if getattr(self, "h", None):
            for t in list(getattr(self, "_tables", ())):  # a table destroyed after its context is a use-after-free in C
                t.close()
            self.L.znippy_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc, what):
        if rc:
            raise ZnippyError(rc, what, (self.L.znippy_last_error(self.h) or b"").decode())

    def sync(self):
        self._chk(self.L.znippy_ctx_sync(self.h), "znippy_ctx_sync")

    def kernel_times(self):
        names = (C.c_char_p * 48)()
        ms = (C.c_float * 48)()
        n = self.L.znippy_last_kernel_times(self.h, names, ms, 48)
        return [(names[i].decode(), float(ms[i])) for i in range(n)]

    def run_lane_stats(self):
        """Run lanes (znippy_hip.h): lean runs queued beside their predecessor / behind it / in front of which a main-stream
        mark was recorded / kept off the lanes, since the context was created."""
        st = (C.c_uint64 * 4)()
        self._chk(self.L.znippy_ctx_run_lane_stats(self.h, st), "znippy_ctx_run_lane_stats")
        return dict(zip(("unordered", "ordered", "marks", "off_lanes"), (int(v) for v in st)))

    def run_lane_older_waits(self):
        """Test introspection: lane runs made to wait for a run older than their predecessor that had not ended (znippy_hip.h)."""
        v = C.c_uint64()
        self._chk(self.L.znippy_ctx_run_lane_older_waits(self.h, C.byref(v)), "znippy_ctx_run_lane_older_waits")
        return int(v.value)

    def set_level(self, level):
        """CompressCtx::new(compression_level), codec.rs:L16-28: levels 1-3 fast tier, 4-22 higher effort tier."""
        self._chk(self.L.znippy_ctx_set_level(self.h, int(level)), "znippy_ctx_set_level")

    @property
    def level(self):
        return int(self.L.znippy_ctx_level(self.h))

    def set_window_log(self, window_log):
        """Opt-in cross-block match window of later encode calls: 0 (default, self-contained blocks) or 17..27
        (matches up to 2^window_log bytes back inside their round; levels 4-22 only).  See znippy_hip.h."""
        self._chk(self.L.znippy_ctx_set_window_log(self.h, int(window_log)), "znippy_ctx_set_window_log")

    @property
    def window_log(self):
        return int(self.L.znippy_ctx_window_log(self.h))

    def set_batch_checksums(self, on):
        """Opt-in: zstd frames with a content checksum (XXH64 trailer) go through the batch and resolve paths of later read
        runs, and a stage of its own checks the trailer; a mismatch is handed to the serial decoder, which reports it.
        0 (default) or 1.  See znippy_hip.h."""
        self._chk(self.L.znippy_ctx_set_batch_checksums(self.h, int(on)), "znippy_ctx_set_batch_checksums")

    def batch_checksums(self):
        return int(self.L.znippy_ctx_batch_checksums(self.h))

    def set_kernel_timing(self, level):
        """2 = HIP events around every kernel (default), 1 = around the dominant read kernels only, 0 = none."""
        self._chk(self.L.znippy_ctx_set_kernel_timing(self.h, int(level)), "znippy_ctx_set_kernel_timing")

    def blake3_pass_ns(self):
        """Measured VALU floor: ns per 64-lane compress pass per SIMD (compressions only, nothing else running)."""
        v, g = C.c_float(), C.c_float()
        self._chk(self.L.znippy_measure_blake3_pass_ns(self.h, C.byref(v), C.byref(g)), "znippy_measure_blake3_pass_ns")
        self.ubench_ghz = float(g.value)
        return float(v.value)

    def last_shader_ghz(self):
        """Shader clock one wave of the small-row read kernel saw in the last run (context created with ZNIPPY_DBG & 32768)."""
        g = C.c_float()
        self._chk(self.L.znippy_last_shader_ghz(self.h, C.byref(g)), "znippy_last_shader_ghz")
        return float(g.value)

    def roles_wait_stats(self, max_waves=1 << 14):
        """Diagnostic (znippy_hip.h): the role-split read kernel's geometry as a dict, and the last run's per-wave wait
        counters as an array [waves, 8] (empty unless the context was created with ZNIPPY_DBG & 32768)."""
        import numpy as np
        g = (C.c_uint32 * 8)()
        buf = np.zeros((max_waves, 8), dtype=np.uint64)
        n = C.c_uint64()
        self._chk(self.L.znippy_roles_wait_stats(self.h, g, buf.ctypes.data, buf.size, C.byref(n)), "znippy_roles_wait_stats")
        keys = ("waves", "slots", "per_cu", "lds_per_workgroup", "registers", "lds_per_cu", "fork_verify", "run_lanes")
        return dict(zip(keys, (int(v) for v in g))), buf[:int(n.value) // 8]

    # ---- single-chunk shims (codec.rs semantics, host buffers) ----
    def compress_bound(self, n):
        return int(self.L.znippy_compress_bound(n))

    def blake3(self, data) -> bytes:
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        out = (C.c_uint8 * 32)()
        self._chk(self.L.znippy_blake3(self.h, np_ptr(a) if a.size else None, a.size, out), "znippy_blake3")
        return bytes(out)

    def decompress(self, frame) -> bytes:
        a = np.frombuffer(frame, dtype=np.uint8)
        n = get_decompressed_size(frame)
        out = np.empty(max(n, 1), dtype=np.uint8)
        w = C.c_size_t()
        self._chk(self.L.znippy_decompress(self.h, np_ptr(a), a.size, np_ptr(out), n, C.byref(w)), "znippy_decompress")
        return out[:w.value].tobytes()

    def compress(self, data) -> bytes:
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        cap = self.compress_bound(a.size)
        out = np.empty(cap, dtype=np.uint8)
        w = C.c_size_t()
        self._chk(self.L.znippy_compress(self.h, np_ptr(a) if a.size else None, a.size, np_ptr(out), cap, C.byref(w)),
                  "znippy_compress")
        return out[:w.value].tobytes()

    # ---- raw DEFLATE of ZIP entries held in device memory ----
    def inflate_batch(self, d_src, src_off, src_len, d_out, out_len, out_off=None, method=None, crc32=None, src_cap=None, out_cap=None):
        """znippy_inflate_batch: item i is the raw DEFLATE stream (method 8; 0 = a copy) d_src[src_off[i] .. + src_len[i]) and must
        decode to exactly out_len[i] bytes at d_out + out_off[i] (None: packed back to back in array order).  crc32: the CRC-32 each
        content must have (None: nothing is compared).  Synchronous and not a run.  Returns (status per item: 0 or ZNIPPY_E_*,
        CRC-32 per item as computed on the device — defined for status 0 and ZNIPPY_E_CHECKSUM)."""
        so, sl, ol = as_np(src_off, np.uint64), as_np(src_len, np.uint64), as_np(out_len, np.uint64)
        oo = as_np(out_off, np.uint64) if out_off is not None else None
        me = as_np(method, np.uint8) if method is not None else None
        cr = as_np(crc32, np.uint32) if crc32 is not None else None
        n = len(so)
        assert len(sl) == n and len(ol) == n and all(a is None or len(a) == n for a in (oo, me, cr)), "item arrays differ in length"
        src_cap = d_src.numel() if src_cap is None else src_cap
        out_cap = d_out.numel() if out_cap is None else out_cap
        status = np.zeros(max(n, 1), dtype=np.int32)
        crc = np.zeros(max(n, 1), dtype=np.uint32)
        opt = lambda a: np_ptr(a) if a is not None else None  # noqa: E731
        self._chk(self.L.znippy_inflate_batch(self.h, _dptr(d_src), int(src_cap), np_ptr(so), np_ptr(sl), opt(me), _dptr(d_out), int(out_cap),
                                              opt(oo), np_ptr(ol), opt(cr), n, np_ptr(status), np_ptr(crc)), "znippy_inflate_batch")
        return status[:n], crc[:n]

    # ---- one tar member out of gzip-compressed tars held in device memory ----
    def targz_find_batch(self, d_src, src_off, src_len, d_out, suffix, prefix=b"", whole=None, scan_cap=8 << 20, src_cap=None, out_cap=None):
        """znippy_targz_find_batch: item i is the gzip member d_src[src_off[i] .. + src_len[i]) of a tar (whole[i] = 0: only the head of
        its file; None: all whole).  Each is inflated only until the first regular member whose name starts with `prefix` and ends with
        `suffix` (bytes) is complete; the members found are packed back to back into d_out in array order.  scan_cap: the most
        inflated bytes one item may take.  Synchronous and not a run.  Returns (status per item: 0 or ZNIPPY_E_* — ZNIPPY_E_MORE asks
        for more of the file —, out_off, out_len, bytes inflated per item)."""
        so, sl = as_np(src_off, np.uint64), as_np(src_len, np.uint64)
        wh = as_np(whole, np.uint8) if whole is not None else None
        n = len(so)
        assert len(sl) == n and (wh is None or len(wh) == n), "item arrays differ in length"
        prefix, suffix = bytes(prefix), bytes(suffix)
        src_cap = d_src.numel() if src_cap is None else src_cap
        out_cap = d_out.numel() if out_cap is None else out_cap
        status = np.zeros(max(n, 1), dtype=np.int32)
        oo, ol, sc = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(3))
        self._chk(self.L.znippy_targz_find_batch(self.h, _dptr(d_src), int(src_cap), np_ptr(so), np_ptr(sl), np_ptr(wh) if wh is not None else None, n,
                                                 prefix, len(prefix), suffix, len(suffix), int(scan_cap), _dptr(d_out), int(out_cap),
                                                 np_ptr(oo), np_ptr(ol), np_ptr(status), np_ptr(sc)), "znippy_targz_find_batch")
        return status[:n], oo[:n], ol[:n], sc[:n]

    # ---- whole gzip files held in device memory ----
    def gunzip_batch(self, d_src, src_off, src_len, d_out, out_room, out_off=None, seg_min=0, src_cap=None, out_cap=None):
        """znippy_gunzip_batch: item i is the whole gzip file d_src[src_off[i] .. + src_len[i]); the content of all its members goes to
        d_out + out_off[i] (None: the rooms lie back to back in array order) and may take out_room[i] bytes — for a file of one member
        its last four bytes, ISIZE, say how many.  Members and the pieces between flush points are decoded in parallel; seg_min: the
        least distance in source bytes between two flush points that are used (0: the default).  CRC-32 and ISIZE of every member are
        checked.  Synchronous and not a run.  Returns (status per item: 0 or ZNIPPY_E_*, out_off, out_len — 0 unless the status is 0 —,
        members, segments: the pieces of the item that a wave of its own decoded)."""
        so, sl, room = as_np(src_off, np.uint64), as_np(src_len, np.uint64), as_np(out_room, np.uint64)
        n = len(so)
        assert len(sl) == n and len(room) == n and (out_off is None or len(out_off) == n), "item arrays differ in length"
        oo = as_np(out_off, np.uint64) if out_off is not None else np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.uint64)
        src_cap = d_src.numel() if src_cap is None else src_cap
        out_cap = d_out.numel() if out_cap is None else out_cap
        status = np.zeros(max(n, 1), dtype=np.int32)
        ol = np.zeros(max(n, 1), dtype=np.uint64)
        mem, seg = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(2))
        self._chk(self.L.znippy_gunzip_batch(self.h, _dptr(d_src), int(src_cap), np_ptr(so), np_ptr(sl), n, _dptr(d_out), int(out_cap),
                                             np_ptr(oo) if out_off is not None else None, np_ptr(room), int(seg_min), np_ptr(ol), np_ptr(status),
                                             np_ptr(mem), np_ptr(seg)), "znippy_gunzip_batch")
        return status[:n], oo[:n], ol[:n], mem[:n], seg[:n]

    GUNZIP_CUT_STATS = ("tested", "passed", "kept", "landed", "marker_pieces", "direct_pieces", "markers_resolved", "passes")

    def set_gunzip_cut(self, cut_bytes):
        """Opt-in: later gunzip_batch calls cut files at DEFLATE block starts found on the device, beside their members and flush points,
        and decode the pieces in parallel.  0 (default, off) or 64 .. 2^30, the window in source bytes that keeps one block candidate.
        Status, content and members are those of the value 0; segments counts the pieces.  See znippy_ctx_set_gunzip_cut in znippy_hip.h."""
        self._chk(self.L.znippy_ctx_set_gunzip_cut(self.h, int(cut_bytes)), "znippy_ctx_set_gunzip_cut")

    @property
    def gunzip_cut(self):
        return int(self.L.znippy_ctx_gunzip_cut(self.h))

    def gunzip_cut_stats(self):
        """The eight counters of the last gunzip_batch call (znippy_ctx_gunzip_cut_stats), in the order of GUNZIP_CUT_STATS."""
        st = (C.c_uint64 * 8)()
        self._chk(self.L.znippy_ctx_gunzip_cut_stats(self.h, st), "znippy_ctx_gunzip_cut_stats")
        return [int(v) for v in st]

    # ---- whole bzip2 files held in device memory ----
    def bunzip2_batch(self, d_src, src_off, src_len, d_out, out_room, out_off=None, slot_cap=0, src_cap=None, out_cap=None):
        """znippy_bunzip2_batch: item i is the whole bzip2 file d_src[src_off[i] .. + src_len[i]); the content of all its streams goes
        to d_out + out_off[i] (None: the rooms lie back to back in array order) and may take out_room[i] bytes (bunzip2_sizes says
        how many it needs).  Blocks are found by their magic and decoded in parallel, at most slot_cap per pass (0: what fits the
        scratch budget); every block CRC and combined CRC is checked.  Synchronous and not a run.  Returns (status per item: 0 or
        ZNIPPY_E_*, out_off, out_len — 0 unless the status is 0 —, streams, blocks)."""
        so, sl, room = as_np(src_off, np.uint64), as_np(src_len, np.uint64), as_np(out_room, np.uint64)
        n = len(so)
        assert len(sl) == n and len(room) == n and (out_off is None or len(out_off) == n), "item arrays differ in length"
        oo = as_np(out_off, np.uint64) if out_off is not None else np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.uint64)
        src_cap = d_src.numel() if src_cap is None else src_cap
        out_cap = d_out.numel() if out_cap is None else out_cap
        status = np.zeros(max(n, 1), dtype=np.int32)
        ol = np.zeros(max(n, 1), dtype=np.uint64)
        streams, blocks = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(2))
        self._chk(self.L.znippy_bunzip2_batch(self.h, _dptr(d_src), int(src_cap), np_ptr(so), np_ptr(sl), n, _dptr(d_out), int(out_cap),
                                              np_ptr(oo) if out_off is not None else None, np_ptr(room), int(slot_cap), np_ptr(ol), np_ptr(status),
                                              np_ptr(streams), np_ptr(blocks)), "znippy_bunzip2_batch")
        return status[:n], oo[:n], ol[:n], streams[:n], blocks[:n]

    def bunzip2_sizes(self, d_src, src_off, src_len, slot_cap=0, src_cap=None):
        """znippy_bunzip2_batch in measure mode (no output buffer): nothing is written and no CRC is checked.  Returns (status per
        item, the size each item's content has — 0 unless the status is 0 —, streams, blocks)."""
        so, sl = as_np(src_off, np.uint64), as_np(src_len, np.uint64)
        n = len(so)
        assert len(sl) == n, "item arrays differ in length"
        src_cap = d_src.numel() if src_cap is None else src_cap
        status = np.zeros(max(n, 1), dtype=np.int32)
        ol = np.zeros(max(n, 1), dtype=np.uint64)
        streams, blocks = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(2))
        self._chk(self.L.znippy_bunzip2_batch(self.h, _dptr(d_src), int(src_cap), np_ptr(so), np_ptr(sl), n, None, 0, None, None, int(slot_cap),
                                              np_ptr(ol), np_ptr(status), np_ptr(streams), np_ptr(blocks)), "znippy_bunzip2_batch")
        return status[:n], ol[:n], streams[:n], blocks[:n]

    # ---- whole xz files held in device memory ----
    def unxz_batch(self, d_src, src_off, src_len, d_out, out_room, out_off=None, src_cap=None, out_cap=None):
        """znippy_unxz_batch: item i is the whole xz file d_src[src_off[i] .. + src_len[i]); the content of all its streams goes to
        d_out + out_off[i] (None: the rooms lie back to back in array order) and may take out_room[i] bytes (unxz_sizes says how
        many the file claims).  Every block of every item is decoded in one launch, a wave per block, straight into its place; CRC32
        and CRC64 checks are verified.  Synchronous and not a run.  Returns (status per item: 0 or ZNIPPY_E_*, out_off, out_len — 0
        unless the status is 0 —, streams, blocks, unverified: the blocks whose check is none, SHA-256 or a reserved id)."""
        so, sl, room = as_np(src_off, np.uint64), as_np(src_len, np.uint64), as_np(out_room, np.uint64)
        n = len(so)
        assert len(sl) == n and len(room) == n and (out_off is None or len(out_off) == n), "item arrays differ in length"
        oo = as_np(out_off, np.uint64) if out_off is not None else np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.uint64)
        src_cap = d_src.numel() if src_cap is None else src_cap
        out_cap = d_out.numel() if out_cap is None else out_cap
        status = np.zeros(max(n, 1), dtype=np.int32)
        ol = np.zeros(max(n, 1), dtype=np.uint64)
        streams, blocks, unverified = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        self._chk(self.L.znippy_unxz_batch(self.h, _dptr(d_src), int(src_cap), np_ptr(so), np_ptr(sl), n, _dptr(d_out), int(out_cap),
                                           np_ptr(oo) if out_off is not None else None, np_ptr(room), np_ptr(ol), np_ptr(status),
                                           np_ptr(streams), np_ptr(blocks), np_ptr(unverified)), "znippy_unxz_batch")
        return status[:n], oo[:n], ol[:n], streams[:n], blocks[:n], unverified[:n]

    def unxz_sizes(self, d_src, src_off, src_len, src_cap=None):
        """znippy_unxz_batch in measure mode (no output buffer): the container walk alone — no block is read, nothing is written.
        Returns (status per item, the size each file's indexes claim — 0 unless the status is 0 —, streams, blocks, unverified)."""
        so, sl = as_np(src_off, np.uint64), as_np(src_len, np.uint64)
        n = len(so)
        assert len(sl) == n, "item arrays differ in length"
        src_cap = d_src.numel() if src_cap is None else src_cap
        status = np.zeros(max(n, 1), dtype=np.int32)
        ol = np.zeros(max(n, 1), dtype=np.uint64)
        streams, blocks, unverified = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        self._chk(self.L.znippy_unxz_batch(self.h, _dptr(d_src), int(src_cap), np_ptr(so), np_ptr(sl), n, None, 0, None, None, np_ptr(ol),
                                           np_ptr(status), np_ptr(streams), np_ptr(blocks), np_ptr(unverified)), "znippy_unxz_batch")
        return status[:n], ol[:n], streams[:n], blocks[:n], unverified[:n]

    # ---- the members of tars held in device memory ----
    def tar_list_batch(self, d_tar, tar_off, tar_len, suffix=b"", prefix=b"", d_out=None, members_cap=None, names_cap=None, tar_cap=None, out_cap=None,
                       measure=False):
        """znippy_tar_list_batch: item i is the (decompressed) tar d_tar[tar_off[i] .. + tar_len[i]).  Every regular member whose name
        starts with `prefix` and ends with `suffix` (bytes; empty = all) is listed, in stream order; with d_out their contents are
        packed into it.  members_cap / names_cap None: a measuring call first, and caps that hold everything.  measure=True: the
        measuring call alone.  Synchronous and not a run.  Returns (status per item: 0 or ZNIPPY_E_*, member_first — n + 1 —,
        members: a structured array (TAR_MEMBER; offsets relative to the item), names: bytes, names_bytes, out_bytes)."""
        to, tl = as_np(tar_off, np.uint64), as_np(tar_len, np.uint64)
        n = len(to)
        assert len(tl) == n, "item arrays differ in length"
        prefix, suffix = bytes(prefix), bytes(suffix)
        tar_cap = d_tar.numel() if tar_cap is None else tar_cap
        status = np.zeros(max(n, 1), dtype=np.int32)
        first = np.zeros(n + 1, dtype=np.uint64)
        nb, ob = C.c_uint64(0), C.c_uint64(0)

        def call(members, m_cap, names, n_cap, out, o_cap):
            self._chk(self.L.znippy_tar_list_batch(self.h, _dptr(d_tar), int(tar_cap), np_ptr(to), np_ptr(tl), n, prefix, len(prefix), suffix, len(suffix),
                                                   np_ptr(members) if members is not None else None, int(m_cap),
                                                   np_ptr(names) if names is not None else None, int(n_cap), _dptr(out) if out is not None else None,
                                                   int(o_cap), np_ptr(first), C.byref(nb), C.byref(ob), np_ptr(status)), "znippy_tar_list_batch")

        if measure or members_cap is None or names_cap is None:
            call(None, 0, None, 0, None, 0)
            if measure:
                return status[:n], first, np.zeros(0, dtype=TAR_MEMBER), b"", nb.value, ob.value
            members_cap = int(first[n]) if members_cap is None else members_cap
            names_cap = nb.value if names_cap is None else names_cap
        members = np.zeros(max(int(members_cap), 1), dtype=TAR_MEMBER)
        names = np.zeros(max(int(names_cap), 1), dtype=np.uint8)
        out_cap = (d_out.numel() if d_out is not None else 0) if out_cap is None else out_cap
        call(members, members_cap, names, names_cap, d_out, out_cap)
        return status[:n], first, members[:int(first[n])], names[:nb.value].tobytes(), nb.value, ob.value


def get_decompressed_size(frame) -> int:
    a = np.frombuffer(frame, dtype=np.uint8)
    v = C.c_uint64()
    rc = _lib.lib().znippy_get_decompressed_size(np_ptr(a), a.size, C.byref(v))
    if rc:
        raise ZnippyError(rc, "znippy_get_decompressed_size")
    return v.value


class RowTable:
    """Device-resident slice [row_begin,row_end) of the index columns + its work plan.  out_offset=None: a table that
    can only be verified (verify / verify_async)."""

    def __init__(self, ctx, blob_offset, blob_size, uncompressed_size, out_offset, compressed_bitmap=None,
                 checksum=None, row_begin=0, row_end=None):
        self.ctx = ctx
        bo = as_np(blob_offset, np.uint64)
        bs = as_np(blob_size, np.uint64)
        us = as_np(uncompressed_size, np.uint64)
        oo = as_np(out_offset, np.uint64) if out_offset is not None else None
        n = len(bo)
        row_end = n if row_end is None else row_end
        bm = as_np(compressed_bitmap, np.uint8) if compressed_bitmap is not None else None
        ck = as_np(checksum, np.uint8).reshape(-1) if checksum is not None else None
        h = vp()
        ctx._chk(ctx.L.znippy_rows_create(ctx.h, np_ptr(bo), np_ptr(bs), np_ptr(bm) if bm is not None else None,
                                          np_ptr(us), np_ptr(oo) if oo is not None else None, np_ptr(ck) if ck is not None else None,
                                          row_begin, row_end, C.byref(h)), "znippy_rows_create")
        self.h = h
        ctx._tables.add(self)
        self.row_begin, self.row_end = row_begin, row_end
        self.n = row_end - row_begin
        self._corrupt, self._k1 = _pinned((max(self.n, 1),), np.uint64)
        self._status, self._k2 = _pinned((max(self.n, 1),), np.int32)
        # The library may run a queued run again, with the pointers it was given, inside a later results call (a lean run
        # over changed blobs; znippy_hip.h): the tensors of the last two runs stay referenced here until they are read.
        self._runs = {}  # run number -> [d_blobs, d_out, read]
        self._seq = 0

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                self.ctx.L.znippy_rows_destroy(self.h)
            self.h = None
        self._runs = {}

    __del__ = close

    def decode_verify_async(self, d_blobs, d_out, blob_base=0, out_cap=None, blob_cap=None):
        out_cap = d_out.numel() if out_cap is None else out_cap
        if blob_cap is None and not isinstance(d_blobs, int):
            blob_cap = d_blobs.numel()
        if blob_cap is not None:  # the blob region's size is known: rows pointing outside it become error codes
            self.ctx._chk(self.ctx.L.znippy_rows_set_blob_cap(self.h, int(blob_cap)), "znippy_rows_set_blob_cap")
        self.ctx._chk(self.ctx.L.znippy_decode_verify_rows_async(self.ctx.h, self.h, _dptr(d_blobs), blob_base,
                                                                 _dptr(d_out), out_cap),
                      "znippy_decode_verify_rows_async")
        self._runs[self._seq] = [d_blobs, d_out, False]
        self._seq += 1
        self._runs.pop(self._seq - 3, None)  # the library keeps two runs

    def decode_async(self, d_blobs, d_out, blob_base=0, out_cap=None, blob_cap=None):
        """Queue a decode-only run (the extract path, archive.rs:L144-168): every row is written where a decode run writes
        it and nothing is hashed — the checksum column is not read and digests() is refused while this is the latest run."""
        out_cap = d_out.numel() if out_cap is None else out_cap
        if blob_cap is None and not isinstance(d_blobs, int):
            blob_cap = d_blobs.numel()
        if blob_cap is not None:
            self.ctx._chk(self.ctx.L.znippy_rows_set_blob_cap(self.h, int(blob_cap)), "znippy_rows_set_blob_cap")
        self.ctx._chk(self.ctx.L.znippy_decode_rows_async(self.ctx.h, self.h, _dptr(d_blobs), blob_base, _dptr(d_out), out_cap),
                      "znippy_decode_rows_async")
        self._runs[self._seq] = [d_blobs, d_out, False]  # (repeated with these pointers when a flagged run in front of it is)
        self._seq += 1
        self._runs.pop(self._seq - 3, None)

    def decode(self, d_blobs, d_out, blob_base=0, out_cap=None, blob_cap=None):
        """Decode-only run, synchronous: (counters, status)."""
        self.decode_async(d_blobs, d_out, blob_base, out_cap, blob_cap)
        counters, _, status = self.results()
        return counters, status

    def read_ranges(self, d_blobs, rows, begins, lens, d_out, out_offsets=None, blob_base=0, out_cap=None, blob_cap=None):
        """Byte ranges of rows (znippy_rows_read_ranges): range i is bytes [begins[i], begins[i] + lens[i]) of absolute row
        rows[i] and lands at d_out + out_offsets[i] (None: packed back to back in array order).  Of a row this library
        wrote only the 128 KiB blocks a range overlaps are decoded.  Synchronous and not a run: the table's results stay as
        they are.  Returns (status per range: 0 or ZNIPPY_E_*, content bytes the decoders produced)."""
        rr, rb, rl = as_np(rows, np.uint64), as_np(begins, np.uint64), as_np(lens, np.uint64)
        ro = as_np(out_offsets, np.uint64) if out_offsets is not None else None
        n = len(rr)
        assert len(rb) == n and len(rl) == n and (ro is None or len(ro) == n), "range arrays differ in length"
        out_cap = d_out.numel() if out_cap is None else out_cap
        if blob_cap is None and not isinstance(d_blobs, int):
            blob_cap = d_blobs.numel()
        if blob_cap is not None:
            self.ctx._chk(self.ctx.L.znippy_rows_set_blob_cap(self.h, int(blob_cap)), "znippy_rows_set_blob_cap")
        status = np.zeros(max(n, 1), dtype=np.int32)
        decoded = C.c_uint64()
        self.ctx._chk(self.ctx.L.znippy_rows_read_ranges(self.ctx.h, self.h, _dptr(d_blobs), blob_base, np_ptr(rr), np_ptr(rb), np_ptr(rl),
                                                         np_ptr(ro) if ro is not None else None, n, _dptr(d_out), out_cap,
                                                         np_ptr(status), C.byref(decoded)), "znippy_rows_read_ranges")
        return status[:n], int(decoded.value)

    def read_ranges_verified(self, d_blobs, rows, begins, lens, d_out, out_offsets=None, blob_base=0, out_cap=None, blob_cap=None):
        """read_ranges on a table with a checksum column, where a range reports 0 only if every byte it returns was covered
        by a hash that chains to the row's checksum (znippy_rows_read_ranges_verified): block by block for rows whose
        entries are installed and accepted (set_block_tree), whole rows otherwise.  A block or row that fails gives
        ZNIPPY_E_DIGEST to every range that overlaps it, and nothing of such a range is written.  Returns (status per range,
        content bytes decoded, content bytes hashed)."""
        rr, rb, rl = as_np(rows, np.uint64), as_np(begins, np.uint64), as_np(lens, np.uint64)
        ro = as_np(out_offsets, np.uint64) if out_offsets is not None else None
        n = len(rr)
        assert len(rb) == n and len(rl) == n and (ro is None or len(ro) == n), "range arrays differ in length"
        out_cap = d_out.numel() if out_cap is None else out_cap
        if blob_cap is None and not isinstance(d_blobs, int):
            blob_cap = d_blobs.numel()
        if blob_cap is not None:
            self.ctx._chk(self.ctx.L.znippy_rows_set_blob_cap(self.h, int(blob_cap)), "znippy_rows_set_blob_cap")
        status = np.zeros(max(n, 1), dtype=np.int32)
        decoded, hashed = C.c_uint64(), C.c_uint64()
        self.ctx._chk(self.ctx.L.znippy_rows_read_ranges_verified(self.ctx.h, self.h, _dptr(d_blobs), blob_base, np_ptr(rr), np_ptr(rb),
                                                                  np_ptr(rl), np_ptr(ro) if ro is not None else None, n, _dptr(d_out),
                                                                  out_cap, np_ptr(status), C.byref(decoded), C.byref(hashed)),
                      "znippy_rows_read_ranges_verified")
        return status[:n], int(decoded.value), int(hashed.value)

    def block_tree_layout(self):
        """(n_entries, row_first): the table's block tree has one 32-byte entry per 128 KiB block of every row of more than
        one block (and below 4 GiB); row i's entries are [row_first[i], row_first[i + 1])."""
        n = C.c_uint64()
        first = np.zeros(self.n + 1, dtype=np.uint64)
        self.ctx._chk(self.ctx.L.znippy_rows_block_tree_layout(self.ctx.h, self.h, C.byref(n), np_ptr(first)), "znippy_rows_block_tree_layout")
        return int(n.value), first

    def build_block_tree(self, d_blobs, blob_base=0, blob_cap=None):
        """Compute the block tree from the blobs (znippy_rows_block_tree_build): (tree uint8[n_entries, 32], status per row —
        0, a decode error, ZNIPPY_E_CORRUPT for a blob outside the region, ZNIPPY_E_DIGEST when the entries do not fold to the
        row's checksum; such a row's entries are zeros).  Does not install the tree."""
        if blob_cap is None and not isinstance(d_blobs, int):
            blob_cap = d_blobs.numel()
        if blob_cap is not None:
            self.ctx._chk(self.ctx.L.znippy_rows_set_blob_cap(self.h, int(blob_cap)), "znippy_rows_set_blob_cap")
        n, _ = self.block_tree_layout()
        tree = np.zeros((max(n, 1), 32), dtype=np.uint8)
        status = np.zeros(max(self.n, 1), dtype=np.int32)
        self.ctx._chk(self.ctx.L.znippy_rows_block_tree_build(self.ctx.h, self.h, _dptr(d_blobs), blob_base, np_ptr(tree), np_ptr(status)),
                      "znippy_rows_block_tree_build")
        return tree[:n], status[:self.n]

    def set_block_tree(self, tree):
        """Install a block tree (uint8, 32 bytes per entry, from anywhere) or remove it (None).  Every row's entries are
        authenticated against its checksum: status per row is 0 (accepted, or a row without entries) or ZNIPPY_E_DIGEST
        (rejected: the row is verified whole from then on)."""
        status = np.zeros(max(self.n, 1), dtype=np.int32)
        t = None
        if tree is not None:
            t = as_np(tree, np.uint8).reshape(-1)
            n, _ = self.block_tree_layout()
            assert t.size == 32 * n, "the tree has 32 bytes per entry of block_tree_layout()"
            if not t.size:
                t = np.zeros(1, dtype=np.uint8)  # (a table without entries: NULL would mean "remove")
        self.ctx._chk(self.ctx.L.znippy_rows_set_block_tree(self.ctx.h, self.h, np_ptr(t) if t is not None else None, np_ptr(status)),
                      "znippy_rows_set_block_tree")
        return status[:self.n]

    def verify_async(self, d_blobs, blob_base=0, blob_cap=None):
        """Queue a verify-only run (the read loop with save_data=false, decompress.rs:L186-189): same results calls, same
        counters, corrupt list, status and digests as a decode run over these blobs, and no output."""
        if blob_cap is None and not isinstance(d_blobs, int):
            blob_cap = d_blobs.numel()
        if blob_cap is not None:
            self.ctx._chk(self.ctx.L.znippy_rows_set_blob_cap(self.h, int(blob_cap)), "znippy_rows_set_blob_cap")
        self.ctx._chk(self.ctx.L.znippy_verify_rows_async(self.ctx.h, self.h, _dptr(d_blobs), blob_base),
                      "znippy_verify_rows_async")
        self._runs[self._seq] = [d_blobs, None, False]  # (a flagged lean run is repeated over these blobs)
        self._seq += 1
        self._runs.pop(self._seq - 3, None)

    def verify(self, d_blobs, blob_base=0, blob_cap=None):
        self.verify_async(d_blobs, blob_base, blob_cap)
        return self.results()

    def verify_scratch(self):
        """Test / measurement hook: (device address of the context's verify scratch or 0, bytes of this table's slots in
        it, per-row slot offsets with 2**64 - 1 for rows without one).  No contract for consumers."""
        base, nbytes = vp(), C.c_uint64()
        off = np.zeros(max(self.n, 1), dtype=np.uint64)
        self.ctx._chk(self.ctx.L.znippy_rows_verify_scratch(self.ctx.h, self.h, C.byref(base), C.byref(nbytes), np_ptr(off)),
                      "znippy_rows_verify_scratch")
        return int(base.value or 0), int(nbytes.value), off[:self.n]

    def _read(self, lag):
        """Run `lag` before the latest has been read.  A run's buffers go once it has been read and no older run is left
        unread: reading that one may repeat the latest run as well."""
        run = self._runs.get(self._seq - 1 - lag)
        if run is not None:
            run[2] = True
        for k in sorted(self._runs):
            if not self._runs[k][2]:
                break
            del self._runs[k]

    def results(self, want_status=True):
        c = VerifyCounters()
        corrupt, status = self._corrupt, self._status
        self.ctx._chk(self.ctx.L.znippy_rows_results(self.ctx.h, self.h, C.byref(c), np_ptr(corrupt), corrupt.size,
                                                     np_ptr(status) if want_status else None), "znippy_rows_results")
        self._read(0)
        return c.as_dict(), corrupt[:min(c.corrupt_rows, corrupt.size)].copy(), status[:self.n]

    def results_lagged(self, lag=1):
        """Counters of the run `lag` runs before the latest queued one (waits for that run only)."""
        c = VerifyCounters()
        self.ctx._chk(self.ctx.L.znippy_rows_results_lagged(self.ctx.h, self.h, lag, C.byref(c)),
                      "znippy_rows_results_lagged")
        self._read(lag)
        return c.as_dict()

    def foreign_stats(self):
        """Last run's two-phase path for foreign multi-block frames: pool use, frames it decoded, blocks it gave up."""
        st = (C.c_uint64 * 8)()
        self.ctx._chk(self.ctx.L.znippy_rows_foreign_stats(self.ctx.h, self.h, st), "znippy_rows_foreign_stats")
        return dict(lit_pool_bytes=int(st[0]), seq_pool_records=int(st[1]), frames=int(st[2]), blocks_given_up=int(st[3]),
                    given_up_error=int(st[4]), given_up_table_far=int(st[5]), given_up_pool=int(st[6]), given_up_range=int(st[7]))

    def checksum_stats(self):
        """Last run's checksum stage (Context.set_batch_checksums): frames whose trailer it found right / wrong, bytes it hashed."""
        st = (C.c_uint64 * 4)()
        self.ctx._chk(self.ctx.L.znippy_rows_checksum_stats(self.ctx.h, self.h, st), "znippy_rows_checksum_stats")
        return dict(verified=int(st[0]), mismatched=int(st[1]), bytes=int(st[2]))

    def decode_verify(self, d_blobs, d_out, blob_base=0, out_cap=None, blob_cap=None):
        self.decode_verify_async(d_blobs, d_out, blob_base, out_cap, blob_cap)
        return self.results()

    def digests(self):
        out = np.zeros((max(self.n, 1), 32), dtype=np.uint8)
        self.ctx._chk(self.ctx.L.znippy_rows_digests(self.ctx.h, self.h, np_ptr(out)), "znippy_rows_digests")
        self._read(0)
        return out[:self.n]


class RoundTable:
    """Device-resident batch of Rounds (offset,len,skip) over one staging buffer."""

    def __init__(self, ctx, src_offset, length, skip=None):
        self.ctx = ctx
        so = as_np(src_offset, np.uint64)
        ln = as_np(length, np.uint64)
        sk = as_np(skip, np.uint8) if skip is not None else None
        self.n = len(so)
        self._compressed = (1 - sk).astype(np.uint8) if sk is not None else np.ones(self.n, np.uint8)
        h = vp()
        ctx._chk(ctx.L.znippy_rounds_create(ctx.h, np_ptr(so), np_ptr(ln), np_ptr(sk) if sk is not None else None,
                                            self.n, C.byref(h)), "znippy_rounds_create")
        self.h = h
        ctx._tables.add(self)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                self.ctx.L.znippy_rounds_destroy(self.h)
            self.h = None

    __del__ = close

    def set_store_incompressible(self, on=True):
        """Opt-in: rounds whose frame is not smaller than the input are emitted as-is (compressed=0)."""
        self.ctx._chk(self.ctx.L.znippy_rounds_set_store_incompressible(self.h, int(on)), "set_store_incompressible")
        self._store_inc = bool(on)

    def set_blob_align(self, align):
        """Opt-in: every payload of later encode calls starts at a multiple of `align` (a power of two, 1 .. 4096; 1 = packed),
        gaps zero-filled; blob_bound() follows.  See znippy_rounds_set_blob_align in znippy_hip.h."""
        self.ctx._chk(self.ctx.L.znippy_rounds_set_blob_align(self.h, int(align)), "znippy_rounds_set_blob_align")

    def blob_align(self):
        return int(self.ctx.L.znippy_rounds_blob_align(self.h))

    def blob_bound(self):
        return int(self.ctx.L.znippy_rounds_blob_bound(self.h))

    def emit_block_tree(self, on=True):
        """Opt-in: later encode calls also leave the block tree of the rows these rounds become (block_tree()), made from the
        hash's own tile chaining values.  See znippy_rounds_emit_block_tree in znippy_hip.h."""
        self.ctx._chk(self.ctx.L.znippy_rounds_emit_block_tree(self.h, int(on)), "znippy_rounds_emit_block_tree")

    def block_tree_layout(self):
        """(n_entries, round_first): as RowTable.block_tree_layout, with a round's source length as the row's length."""
        n = C.c_uint64()
        first = np.zeros(self.n + 1, dtype=np.uint64)
        self.ctx._chk(self.ctx.L.znippy_rounds_block_tree_layout(self.ctx.h, self.h, C.byref(n), np_ptr(first)),
                      "znippy_rounds_block_tree_layout")
        return int(n.value), first

    def block_tree(self, lag=0):
        """The tree of the run `lag` runs before the latest queued one (uint8 [n_entries, 32]); waits for that run's result
        copy only.  Raises (ZNIPPY_E_INVAL) when that run was queued with emission off."""
        n, _ = self.block_tree_layout()
        tree = np.zeros((max(n, 1), 32), dtype=np.uint8)
        self.ctx._chk(self.ctx.L.znippy_rounds_block_tree(self.ctx.h, self.h, int(lag), np_ptr(tree)), "znippy_rounds_block_tree")
        return tree[:n]

    def hash(self, d_src):
        out = np.zeros((max(self.n, 1), 32), dtype=np.uint8)
        self.ctx._chk(self.ctx.L.znippy_hash_rounds(self.ctx.h, self.h, _dptr(d_src), np_ptr(out)), "znippy_hash_rounds")
        return out[:self.n]

    def encode_hash_async(self, d_src, d_blob_out, blob_cap=None):
        blob_cap = d_blob_out.numel() if blob_cap is None else blob_cap
        self.ctx._chk(self.ctx.L.znippy_encode_hash_rounds_async(self.ctx.h, self.h, _dptr(d_src), _dptr(d_blob_out),
                                                                 blob_cap), "znippy_encode_hash_rounds_async")

    def results(self):
        """Per-round outputs as numpy VIEWS of the table's pinned result mirror (zero-copy; they are
        overwritten by the next encode call on this table — copy what must outlive it)."""
        bo, bs, ck = vp(), vp(), vp()
        total = C.c_uint64()
        self.ctx._chk(self.ctx.L.znippy_rounds_results_view(self.ctx.h, self.h, C.byref(bo), C.byref(bs), C.byref(ck),
                                                            C.byref(total)), "znippy_rounds_results_view")
        k = self.n
        if k == 0:
            return dict(blob_offset=np.zeros(0, np.uint64), blob_size=np.zeros(0, np.uint64),
                        checksum=np.zeros((0, 32), np.uint8), compressed=np.zeros(0, np.uint8), blob_bytes=0)
        mk = lambda p, nbytes, dt: np.frombuffer((C.c_uint8 * nbytes).from_address(p.value), dtype=dt)
        comp = self._compressed
        if getattr(self, "_store_inc", False):  # the device decided per round: take the full (copying) result call
            comp = np.zeros(k, dtype=np.uint8)
            self.ctx._chk(self.ctx.L.znippy_rounds_results(self.ctx.h, self.h, None, None, None, np_ptr(comp), None),
                          "znippy_rounds_results")
        return dict(blob_offset=mk(bo, 8 * k, np.uint64), blob_size=mk(bs, 8 * k, np.uint64),
                    checksum=mk(ck, 32 * k, np.uint8).reshape(k, 32), compressed=comp, blob_bytes=int(total.value))

    def results_lagged(self, lag=1):
        """Views of the results of the run `lag` runs before the latest queued one (compressed[] as known to the host)."""
        bo, bs, ck = vp(), vp(), vp()
        total = C.c_uint64()
        self.ctx._chk(self.ctx.L.znippy_rounds_results_lagged(self.ctx.h, self.h, lag, C.byref(bo), C.byref(bs),
                                                              C.byref(ck), C.byref(total)), "znippy_rounds_results_lagged")
        k = self.n
        mk = lambda p, nbytes, dt: np.frombuffer((C.c_uint8 * nbytes).from_address(p.value), dtype=dt)
        return dict(blob_offset=mk(bo, 8 * k, np.uint64), blob_size=mk(bs, 8 * k, np.uint64),
                    checksum=mk(ck, 32 * k, np.uint8).reshape(k, 32), compressed=self._compressed,
                    blob_bytes=int(total.value))

    def encode_hash(self, d_src, d_blob_out, blob_cap=None):
        self.encode_hash_async(d_src, d_blob_out, blob_cap)
        return self.results()
