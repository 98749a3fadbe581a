"""ctypes binding of libznippy_hip.so (the C ABI in include/znippy_hip.h).

There is NO CPU fallback: if the HIP library is missing or fails to load, importing the
product path raises.  Device memory / streams come from PyTorch-ROCm (plumbing only).
"""
import ctypes as C
import os

import numpy as np

from . import _build

_HERE = os.path.dirname(os.path.abspath(__file__))

OK = 0
E_INVAL, E_HIP, E_NOMEM, E_DST_SMALL, E_CORRUPT, E_UNSUPPORTED, E_CHECKSUM, E_DIGEST, E_NOENT = -1, -2, -3, -4, -5, -6, -7, -8, -9
_ERRNAMES = {E_INVAL: "invalid argument", E_HIP: "HIP runtime error", E_NOMEM: "out of device memory",
             E_DST_SMALL: "destination too small", E_CORRUPT: "corrupt frame",
             E_UNSUPPORTED: "unsupported frame", E_CHECKSUM: "content checksum mismatch",
             E_DIGEST: "BLAKE3 digest mismatch", E_NOENT: "no entry of the container matches"}


class ZnippyError(RuntimeError):
    def __init__(self, code, what, detail=""):
        self.code = code
        super().__init__(f"{what}: {_ERRNAMES.get(code, code)} ({code}) {detail}".strip())


class VerifyCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("total_chunks", "total_written_bytes", "verified_bytes",
                                          "corrupt_bytes", "corrupt_rows", "decode_errors")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


_lib = None
vp = C.c_void_p

EXPORTS = [
    "znippy_ctx_create", "znippy_ctx_destroy", "znippy_last_error", "znippy_ctx_sync",
    "znippy_compress_bound", "znippy_get_decompressed_size", "znippy_decompress", "znippy_compress",
    "znippy_blake3", "znippy_rows_create", "znippy_rows_destroy", "znippy_decode_verify_rows",
    "znippy_decode_verify_rows_async", "znippy_rows_results", "znippy_rows_digests",
    "znippy_rounds_create", "znippy_rounds_destroy", "znippy_rounds_blob_bound",
    "znippy_encode_hash_rounds", "znippy_encode_hash_rounds_async", "znippy_rounds_results",
    "znippy_rounds_results_view", "znippy_rows_results_lagged", "znippy_rows_set_blob_cap", "znippy_rounds_results_lagged", "znippy_rounds_set_store_incompressible", "znippy_hash_rounds", "znippy_last_kernel_times", "znippy_measure_blake3_pass_ns", "znippy_last_shader_ghz", "znippy_ctx_set_kernel_timing", "znippy_rows_foreign_stats", "znippy_ctx_run_lane_stats", "znippy_ctx_run_lane_older_waits", "znippy_ctx_set_level", "znippy_ctx_level",
    "znippy_ctx_set_window_log", "znippy_ctx_window_log",
    "znippy_ctx_set_batch_checksums", "znippy_ctx_batch_checksums", "znippy_rows_checksum_stats",
    "znippy_verify_rows", "znippy_verify_rows_async", "znippy_rows_verify_scratch",
    "znippy_decode_rows", "znippy_decode_rows_async",
    "znippy_rounds_set_blob_align", "znippy_rounds_blob_align",
    "znippy_rows_read_ranges",
    "znippy_rows_block_tree_layout", "znippy_rows_block_tree_build", "znippy_rows_set_block_tree",
    "znippy_rows_read_ranges_verified",
    "znippy_rounds_emit_block_tree", "znippy_rounds_block_tree_layout", "znippy_rounds_block_tree",
    "znippy_inflate_batch", "znippy_targz_find_batch", "znippy_gunzip_batch", "znippy_roles_wait_stats",
    "znippy_bunzip2_batch", "znippy_tar_list_batch", "znippy_unxz_batch",
    "znippy_ctx_set_gunzip_cut", "znippy_ctx_gunzip_cut", "znippy_ctx_gunzip_cut_stats",
]


def lib_path():
    return _build.SO


def lib():
    """Load (never build-on-import on a GPU box: the .so travels with the snapshot)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own libamdhip64; load it FIRST so this library's hip* symbols bind to the
    # same runtime instance (two HIP runtimes in one process: the second one finds no device).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
    L = C.CDLL(path)
    L.znippy_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    L.znippy_ctx_destroy.argtypes = [vp]
    L.znippy_ctx_destroy.restype = None
    L.znippy_last_error.argtypes = [vp]
    L.znippy_last_error.restype = C.c_char_p
    L.znippy_ctx_sync.argtypes = [vp]
    L.znippy_compress_bound.argtypes = [C.c_size_t]
    L.znippy_compress_bound.restype = C.c_size_t
    L.znippy_get_decompressed_size.argtypes = [vp, C.c_size_t, C.POINTER(C.c_uint64)]
    L.znippy_decompress.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.znippy_compress.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.znippy_blake3.argtypes = [vp, vp, C.c_size_t, vp]
    L.znippy_rows_create.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.znippy_rows_destroy.argtypes = [vp]
    L.znippy_rows_destroy.restype = None
    L.znippy_decode_verify_rows.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(VerifyCounters),
                                            vp, C.c_uint64, vp]
    L.znippy_decode_verify_rows_async.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64]
    L.znippy_rows_results.argtypes = [vp, vp, C.POINTER(VerifyCounters), vp, C.c_uint64, vp]
    L.znippy_rows_results_lagged.argtypes = [vp, vp, C.c_uint, C.POINTER(VerifyCounters)]
    L.znippy_rounds_results_lagged.argtypes = [vp, vp, C.c_uint, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                               C.POINTER(C.c_uint64)]
    L.znippy_rows_set_blob_cap.argtypes = [vp, C.c_uint64]
    L.znippy_rows_digests.argtypes = [vp, vp, vp]
    L.znippy_rounds_create.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(vp)]
    L.znippy_rounds_destroy.argtypes = [vp]
    L.znippy_rounds_destroy.restype = None
    L.znippy_rounds_blob_bound.argtypes = [vp]
    L.znippy_rounds_blob_bound.restype = C.c_uint64
    L.znippy_encode_hash_rounds.argtypes = [vp, vp, vp, vp, C.c_uint64, vp, vp, vp, vp, C.POINTER(C.c_uint64)]
    L.znippy_encode_hash_rounds_async.argtypes = [vp, vp, vp, vp, C.c_uint64]
    L.znippy_rounds_results.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(C.c_uint64)]
    L.znippy_rounds_results_view.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.znippy_rounds_set_store_incompressible.argtypes = [vp, C.c_int]
    L.znippy_hash_rounds.argtypes = [vp, vp, vp, vp]
    L.znippy_last_kernel_times.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]
    L.znippy_measure_blake3_pass_ns.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.znippy_last_shader_ghz.argtypes = [vp, C.POINTER(C.c_float)]
    L.znippy_ctx_set_kernel_timing.argtypes = [vp, C.c_int]
    L.znippy_ctx_set_level.argtypes = [vp, C.c_int]
    L.znippy_ctx_level.argtypes = [vp]
    L.znippy_ctx_set_window_log.argtypes = [vp, C.c_int]
    L.znippy_ctx_window_log.argtypes = [vp]
    L.znippy_rows_foreign_stats.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    if hasattr(L, "znippy_ctx_set_batch_checksums"):  # (likewise)
        L.znippy_ctx_set_batch_checksums.argtypes = [vp, C.c_int]
        L.znippy_ctx_batch_checksums.argtypes = [vp]
        L.znippy_rows_checksum_stats.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    if hasattr(L, "znippy_verify_rows"):  # (an older build loaded beside this one for an A/B has not got them: calling them raises)
        L.znippy_verify_rows.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(VerifyCounters), vp, C.c_uint64, vp]
        L.znippy_verify_rows_async.argtypes = [vp, vp, vp, C.c_uint64]
        L.znippy_rows_verify_scratch.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(C.c_uint64), vp]
    if hasattr(L, "znippy_decode_rows"):  # (likewise)
        L.znippy_decode_rows.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(VerifyCounters), vp]
        L.znippy_decode_rows_async.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64]
    if hasattr(L, "znippy_rounds_set_blob_align"):  # (likewise)
        L.znippy_rounds_set_blob_align.argtypes = [vp, C.c_uint32]
        L.znippy_rounds_blob_align.argtypes = [vp]
        L.znippy_rounds_blob_align.restype = C.c_uint32
    if hasattr(L, "znippy_rows_read_ranges"):  # (likewise)
        L.znippy_rows_read_ranges.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp,
                                              C.POINTER(C.c_uint64)]
    if hasattr(L, "znippy_rows_read_ranges_verified"):  # (likewise)
        L.znippy_rows_block_tree_layout.argtypes = [vp, vp, C.POINTER(C.c_uint64), vp]
        L.znippy_rows_block_tree_build.argtypes = [vp, vp, vp, C.c_uint64, vp, vp]
        L.znippy_rows_set_block_tree.argtypes = [vp, vp, vp, vp]
        L.znippy_rows_read_ranges_verified.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp,
                                                       C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if hasattr(L, "znippy_rounds_emit_block_tree"):  # (likewise)
        L.znippy_rounds_emit_block_tree.argtypes = [vp, C.c_int]
        L.znippy_rounds_block_tree_layout.argtypes = [vp, vp, C.POINTER(C.c_uint64), vp]
        L.znippy_rounds_block_tree.argtypes = [vp, vp, C.c_uint, vp]
    if hasattr(L, "znippy_ctx_run_lane_stats"):  # (likewise)
        L.znippy_ctx_run_lane_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.znippy_ctx_run_lane_older_waits.argtypes = [vp, C.POINTER(C.c_uint64)]
    if hasattr(L, "znippy_inflate_batch"):  # (likewise)
        L.znippy_inflate_batch.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, vp]
    if hasattr(L, "znippy_targz_find_batch"):  # (likewise)
        L.znippy_targz_find_batch.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint64,
                                              vp, C.c_uint64, vp, vp, vp, vp]
    if hasattr(L, "znippy_gunzip_batch"):  # (likewise)
        L.znippy_gunzip_batch.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, vp, vp]
    if hasattr(L, "znippy_ctx_set_gunzip_cut"):  # (likewise)
        L.znippy_ctx_set_gunzip_cut.argtypes = [vp, C.c_uint64]
        L.znippy_ctx_gunzip_cut.argtypes = [vp]
        L.znippy_ctx_gunzip_cut.restype = C.c_uint64
        L.znippy_ctx_gunzip_cut_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    if hasattr(L, "znippy_bunzip2_batch"):  # (likewise)
        L.znippy_bunzip2_batch.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, vp, vp]
    if hasattr(L, "znippy_tar_list_batch"):  # (likewise)
        L.znippy_tar_list_batch.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, vp, C.c_uint64,
                                            vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp]
    if hasattr(L, "znippy_unxz_batch"):  # (likewise)
        L.znippy_unxz_batch.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "znippy_roles_wait_stats"):  # (likewise)
        L.znippy_roles_wait_stats.argtypes = [vp, C.POINTER(C.c_uint32), vp, C.c_uint64, C.POINTER(C.c_uint64)]
    _lib = L
    return L


def np_ptr(a):
    return a.ctypes.data_as(vp)


def as_np(x, dtype):
    return np.ascontiguousarray(np.asarray(x, dtype=dtype))
