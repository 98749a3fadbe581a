"""BLAKE3 in numpy, with the block tree of a row (include/znippy_hip.h, "block tree"): the chunk chaining values of a whole
row in one vectorised pass, the 128 KiB block entries folded from them, and the digest folded from the entries.  Written
from the BLAKE3 specification; uses nothing from the library under test."""
import numpy as np

IV = np.array([0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19], np.uint32)
PERM = [2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8]
CHUNK_START, CHUNK_END, PARENT, ROOT = 1, 2, 4, 8
BLK = 128 * 1024
CHUNKS_PER_BLK = 128


def _rotr(x, n):
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def _g(v, a, b, c, d, mx, my):
    v[a] = v[a] + v[b] + mx
    v[d] = _rotr(v[d] ^ v[a], 16)
    v[c] = v[c] + v[d]
    v[b] = _rotr(v[b] ^ v[c], 12)
    v[a] = v[a] + v[b] + my
    v[d] = _rotr(v[d] ^ v[a], 8)
    v[c] = v[c] + v[d]
    v[b] = _rotr(v[b] ^ v[c], 7)


def compress(cv, m, counter, block_len, flags):
    """N compressions at once: cv [N, 8], m [N, 16], counter / block_len / flags [N] (or scalars) -> new cv [N, 8]."""
    n = cv.shape[0]
    col = lambda x: np.broadcast_to(np.asarray(x, np.uint64), (n,))
    v = [cv[:, i].copy() for i in range(8)] + [np.full(n, IV[i], np.uint32) for i in range(4)]
    v += [(col(counter) & np.uint64(0xFFFFFFFF)).astype(np.uint32), (col(counter) >> np.uint64(32)).astype(np.uint32),
          col(block_len).astype(np.uint32), col(flags).astype(np.uint32)]
    w = [m[:, i] for i in range(16)]
    with np.errstate(over="ignore"):
        for r in range(7):
            _g(v, 0, 4, 8, 12, w[0], w[1]); _g(v, 1, 5, 9, 13, w[2], w[3]); _g(v, 2, 6, 10, 14, w[4], w[5]); _g(v, 3, 7, 11, 15, w[6], w[7])
            _g(v, 0, 5, 10, 15, w[8], w[9]); _g(v, 1, 6, 11, 12, w[10], w[11]); _g(v, 2, 7, 8, 13, w[12], w[13]); _g(v, 3, 4, 9, 14, w[14], w[15])
            w = [w[p] for p in PERM]
    return np.stack([v[i] ^ v[i + 8] for i in range(8)], axis=1)


def chunk_cvs(data, root_if_single=False):
    """Chaining values of all chunks of `data` (counters 0, 1, ...): uint32 [max(1, ceil(len / 1024)), 8]."""
    a = np.frombuffer(bytes(data), np.uint8)
    n = max(1, -(-a.size // 1024))
    padded = np.zeros(n * 1024, np.uint8)
    padded[:a.size] = a
    words = padded.view("<u4").astype(np.uint32).reshape(n, 16, 16)
    lens = np.minimum(1024, np.maximum(0, a.size - 1024 * np.arange(n))).astype(np.int64)
    nblk = np.maximum(1, -(-lens // 64))
    cv = np.tile(IV, (n, 1))
    counter = np.arange(n, dtype=np.uint64)
    for b in range(16):
        on = nblk > b
        if not on.any():
            break
        last = nblk - 1 == b
        blen = np.clip(lens - 64 * b, 0, 64)
        flags = np.where(b == 0, CHUNK_START, 0) | np.where(last, CHUNK_END | (ROOT if root_if_single and n == 1 else 0), 0)
        cv[on] = compress(cv[on], words[on, b], counter[on], blen[on], flags[on])
    return cv


def parents(left, right, root=False):
    m = np.concatenate([left, right], axis=1)
    return compress(np.tile(IV, (left.shape[0], 1)), m, 0, 64, PARENT | (ROOT if root else 0))


def fold(nodes, root):
    """Pairwise fold with the odd node promoted — the left-heavy tree — down to one node; ROOT on the last parent if `root`."""
    nodes = np.asarray(nodes, np.uint32)
    while nodes.shape[0] > 1:
        n = nodes.shape[0]
        top = parents(nodes[0:n - 1:2], nodes[1:n:2], root and n == 2)
        nodes = np.concatenate([top, nodes[n - 1:]]) if n & 1 else top
    return nodes[0]


def n_entries(length):
    return -(-length // BLK) if BLK < length < (1 << 32) else 0


def row_first(lengths):
    return np.concatenate([[0], np.cumsum([n_entries(int(n)) for n in lengths])]).astype(np.uint64)


def entries(data):
    """The row's block tree: uint8 [n_entries(len), 32]."""
    nb = n_entries(len(data))
    if not nb:
        return np.zeros((0, 32), np.uint8)
    cvs = chunk_cvs(data)
    out = np.stack([fold(cvs[CHUNKS_PER_BLK * k:CHUNKS_PER_BLK * (k + 1)], False) for k in range(nb)])
    return out.astype("<u4").view(np.uint8).reshape(nb, 32)


def digest_from_entries(e):
    e = np.ascontiguousarray(e, np.uint8).reshape(-1, 32)
    assert e.shape[0] >= 2, "a row with entries has at least two"
    return fold(e.view("<u4").astype(np.uint32), True).astype("<u4").tobytes()


def blake3(data):
    """Digest of `data` (for the self-check against the known answers)."""
    cvs = chunk_cvs(data, root_if_single=True)
    return (cvs[0] if cvs.shape[0] == 1 else fold(cvs, True)).astype("<u4").tobytes()


def table_tree(rows):
    """Entries of `rows` concatenated in row order: uint8 [sum, 32]."""
    parts = [entries(r) for r in rows]
    return np.concatenate(parts) if parts else np.zeros((0, 32), np.uint8)
