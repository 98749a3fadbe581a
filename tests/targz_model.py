"""A Python model of znippy_targz_find_batch and of the tar walk it runs (znippy_amd/csrc/tar_rules.h), for the GPU tests and the
CPU test of the walker.  Not a test file.

The device decodes a gzip member until the tar it produces answers the question.  The model does the same with zlib: the DEFLATE
bytes go into zlib.decompressobj(-15) one byte at a time, and what the calls returned is the prefix P of the tar that the input
given determines, with the reason it ended (the stream's end, the input's end, an error).  `walk` — a restatement of the C++ walk,
written from tarfile's rules and not from the C++ text — then runs on P.  tests/test_tar_rules_cpu.py pins `walk` to tarfile on
valid archives and the C++ walker to `walk` on damaged ones."""
import zlib

OK, E_INVAL, E_NOMEM, E_DST_SMALL, E_CORRUPT, E_UNSUPPORTED, E_NOENT, E_MORE = 0, -1, -3, -4, -5, -6, -9, -10
BLANKS = b" \t\n\x0b\x0c\r\x1c\x1d\x1e\x1f"
LIMIT = 1 << 62
HIGH = bytes(range(128, 256))


def gzip_header(b):
    """(0, offset of the first DEFLATE byte) | (E_MORE, 0): b ends inside the header | (E_CORRUPT / E_UNSUPPORTED, 0)"""
    if b[:2] != b"\x1f\x8b"[:len(b[:2])]:
        return E_CORRUPT, 0
    if len(b) >= 3 and b[2] != 8:
        return E_UNSUPPORTED, 0
    if len(b) >= 4 and b[3] & 0xE0:
        return E_UNSUPPORTED, 0
    if len(b) < 10:
        return E_MORE, 0
    flg, at = b[3], 10
    if flg & 4:
        if len(b) < at + 2:
            return E_MORE, 0
        at += 2 + (b[at] | b[at + 1] << 8)
        if len(b) < at:
            return E_MORE, 0
    for bit in (8, 16):
        if flg & bit:
            z = b.find(b"\0", at)
            if z < 0:
                return E_MORE, 0
            at = z + 1
    if flg & 2:
        at += 2
        if len(b) < at:
            return E_MORE, 0
    return OK, at


def _number(f):
    if f[0] == 0x80:
        v = int.from_bytes(f[1:], "big")
        return v if v < LIMIT else None
    if f[0] == 0xFF:
        return None
    s = f.split(b"\0", 1)[0].strip(BLANKS)
    if any(c not in b"01234567" for c in s):
        return None
    return int(s, 8) if s else 0


def _pax(p):
    """path and size of a pax payload: (status, path | None, size | None)"""
    pos, path, size = 0, None, None
    while pos < len(p):
        i = pos
        while i < len(p) and i - pos < 10 and 48 <= p[i] <= 57:
            i += 1
        if i == pos or i >= len(p) or p[i] != 32:
            return E_CORRUPT, None, None
        n = int(p[pos:i])
        if n > len(p) - pos or pos + n < i + 3 or p[pos + n - 1] != 10:
            return E_CORRUPT, None, None
        rec = p[i + 1:pos + n - 1]
        key, eq, val = rec.partition(b"=")
        if not eq or not key:
            return E_CORRUPT, None, None
        if key.startswith(b"GNU.sparse."):
            return E_UNSUPPORTED, None, None
        if key == b"path":
            path = val
        if key == b"size":
            if not val or any(not 48 <= c <= 57 for c in val):
                return E_CORRUPT, None, None
            size = 0
            for c in val:
                if size >= LIMIT // 10:
                    return E_CORRUPT, None, None
                size = size * 10 + c - 48
        pos += n
    return OK, path, size


def walk(t, ended, prefix=b"", suffix=b""):
    """The first regular member of the tar prefix `t` whose name starts with prefix and ends with suffix:
    (status, data_off, size, need) — need: for E_MORE (only when not ended), the bytes the walk wants before it goes on, and for a
    verdict the highest offset it looked below."""
    h, zeros, name, size_over = 0, 0, None, None

    def short(need, inside_header_boundary):
        if not ended:
            return E_MORE, 0, 0, need
        return (E_NOENT if inside_header_boundary and len(t) == h and name is None and size_over is None else E_CORRUPT), 0, 0, need

    while True:
        if h >= LIMIT and len(t) >= h + 512:
            return E_CORRUPT, 0, 0, h + 512
        if len(t) < h + 512:
            return short(h + 512, True)
        b = t[h:h + 512]
        if b == bytes(512):
            if name is not None or size_over is not None:
                return E_CORRUPT, 0, 0, h + 512
            zeros += 1
            if zeros == 2:
                return E_NOENT, 0, 0, h + 512
            h += 512
            continue
        zeros = 0
        chk = _number(b[148:156])
        rest = b[:148] + b"        " + b[156:]
        unsigned = sum(rest)
        if chk is None or chk not in (unsigned, unsigned - 256 * (512 - len(rest.translate(None, HIGH)))):  # (the signed sum)
            return E_CORRUPT, 0, 0, h + 512
        size = _number(b[124:136])
        if size is None:
            return E_CORRUPT, 0, 0, h + 512
        typ = b[156:157]
        fname = b[:100].split(b"\0", 1)[0]
        if typ == b"\0" and fname.endswith(b"/"):
            typ = b"5"
        if typ == b"S":
            return E_UNSUPPORTED, 0, 0, h + 512
        if typ in (b"L", b"x", b"X"):
            if size > 8192:
                return E_UNSUPPORTED, 0, 0, h + 512
            if len(t) < h + 512 + size:
                return short(h + 512 + size, False)
            p = t[h + 512:h + 512 + size]
            if typ == b"L":
                if name is None:
                    name = p.split(b"\0", 1)[0]
            else:
                st, path, psize = _pax(p)
                if st:
                    return st, 0, 0, h + 512 + size
                if path is not None and name is None:
                    name = path
                if psize is not None and size_over is None:
                    size_over = psize
            h += 512 + (size + 511) // 512 * 512
            continue
        if typ in (b"g", b"K"):
            h += 512 + (size + 511) // 512 * 512
            continue
        if size_over is not None:
            size = size_over
        if typ in (b"0", b"\0", b"7"):
            pfx = b[345:500].split(b"\0", 1)[0]
            full = name if name is not None else (pfx + b"/" + fname if pfx else fname)
            if full.startswith(prefix) and full.endswith(suffix):
                if len(t) < h + 512 + size:
                    return short(h + 512 + size, False)
                return OK, h + 512, size, h + 512 + size
        name = size_over = None
        h += 512 + (0 if typ in (b"1", b"2", b"3", b"4", b"5", b"6") else (size + 511) // 512 * 512)


def inflate_prefix(deflate):
    """What zlib makes of the raw DEFLATE bytes fed one at a time: (P, why, tail) — why: "end" (the final block ended; tail = the
    bytes behind the stream), "input" (the bytes ran out), "error" (zlib refused a byte; P is what it had handed out before)."""
    d = zlib.decompressobj(-15)
    out = []
    for i in range(len(deflate)):
        try:
            out.append(d.decompress(deflate[i:i + 1]))
        except zlib.error:
            return b"".join(out), "error", b""
        if d.eof:
            return b"".join(out), "end", d.unused_data + deflate[i + 1:]
    return b"".join(out), "input", b""


def item_cap(src_len, scan_cap):
    """the inflated bytes one item may take: min(scan_cap, 1032 * src_len + 512), and below 4 GiB"""
    return min(scan_cap, 1032 * src_len + 512, 0xFFFFFFF0)


def find(src, whole, prefix, suffix, scan_cap, inflated=None):
    """The model of one item: (status, member bytes, member end in the tar, need).  `need` is the walk's last need: with a rejected
    stream, how far beyond the prefix the walk wanted to see."""
    st, at = gzip_header(src)
    if st == E_MORE:
        return (E_CORRUPT if whole else E_MORE), b"", 0, 0
    if st:
        return st, b"", 0, 0
    P, why, tail = inflated if inflated is not None else inflate_prefix(src[at:])
    cap = item_cap(len(src), scan_cap)
    t = P[:cap]
    st, off, size, need = walk(t, False, prefix, suffix)
    if st == OK:
        return OK, t[off:off + size], off + size, need
    if st != E_MORE:
        return st, b"", 0, need
    if need > cap:
        return E_DST_SMALL, b"", 0, need
    # need <= cap and the prefix is shorter: the stream ended, ran out or was refused in front of the answer
    if why == "error":
        return E_CORRUPT, b"", 0, need
    if why == "input":
        return (E_CORRUPT if whole else E_MORE), b"", 0, need
    if len(tail) >= 18 and tail[8:10] == b"\x1f\x8b":
        return E_UNSUPPORTED, b"", 0, need
    if not whole and len(tail) < 18:
        return E_MORE, b"", 0, need  # whether another member follows is behind the bytes given
    return walk(t, True, prefix, suffix)[0], b"", 0, need
