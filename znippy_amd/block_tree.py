"""The block tree's layout and its sidecar file `<archive path>.b3t` (include/znippy_hip.h, "block tree"; include/znippy_host.h).
Pure functions, no GPU: 32 bytes per 128 KiB block of every row of more than one block and below 4 GiB, rows in index order.

Sidecar, little-endian: `ZNPYB3T1`, u32 block log (17), u32 zero, u64 n_rows, u64 n_entries, then the entries.  No checksum of
its own: the index's checksum column authenticates every row's entries (znippy_rows_set_block_tree)."""
import os
import struct

import numpy as np

MAGIC = b"ZNPYB3T1"
BLOCK_LOG = 17
BLK = 1 << BLOCK_LOG
HEADER = 32
SUFFIX = ".b3t"


def n_entries(length):
    """Entries of a row of `length` content bytes."""
    length = int(length)
    return -(-length // BLK) if BLK < length < (1 << 32) else 0


def layout(lengths):
    """(n_entries of the table, first): row i's entries are [first[i], first[i + 1]); first has len(lengths) + 1 values."""
    first = np.zeros(len(lengths) + 1, dtype=np.uint64)
    if len(lengths):
        first[1:] = np.cumsum([n_entries(n) for n in lengths], dtype=np.uint64)
    return int(first[-1]), first


def sidecar_path(archive_path):
    return os.fspath(archive_path) + SUFFIX


def write_sidecar(path, n_rows, entries):
    """entries: uint8, 32 bytes per entry, in row order."""
    e = np.ascontiguousarray(np.asarray(entries, dtype=np.uint8)).reshape(-1)
    if e.size % 32:
        raise ValueError(f"entries are 32 bytes each, not {e.size} bytes in all")
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<IIQQ", BLOCK_LOG, 0, int(n_rows), e.size // 32))
        f.write(e.tobytes())


def read_sidecar(path):
    """(n_rows, entries uint8 [n_entries, 32]); ValueError names what is malformed."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < HEADER:
        raise ValueError(f"{path}: short file ({len(raw)} bytes, the header has {HEADER})")
    if raw[:8] != MAGIC:
        raise ValueError(f"{path}: wrong magic {raw[:8]!r}")
    log, zero, n_rows, n = struct.unpack("<IIQQ", raw[8:HEADER])
    if log != BLOCK_LOG:
        raise ValueError(f"{path}: block log {log}, not {BLOCK_LOG}")
    if zero:
        raise ValueError(f"{path}: reserved field is {zero}, not zero")
    if len(raw) != HEADER + 32 * n:
        raise ValueError(f"{path}: length {len(raw)} does not match n_entries {n} (expected {HEADER + 32 * n})")
    return n_rows, np.frombuffer(raw, dtype=np.uint8, offset=HEADER).reshape(n, 32).copy()
