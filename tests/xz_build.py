"""xz containers (xz file format 1.1.0) assembled by hand: streams, blocks with and without the sizes in their headers, any check id,
index, footer, stream padding.  The block data is Python's raw LZMA2 output (lzma.FORMAT_RAW, FILTER_LZMA2) or any bytes a caller
brings (tests/lzma_build.py scripts them).  Every field can be overridden, which is how the damaged cases are made; nothing here
needs the xz tool.  tests/test_xz_build_cpu.py proves against liblzma that what is assembled here is what it claims to be."""
import hashlib
import lzma
import struct
import zlib

HEADER_MAGIC = b"\xfd7zXZ\x00"
FOOTER_MAGIC = b"YZ"
CHECK_NONE, CHECK_CRC32, CHECK_CRC64, CHECK_SHA256 = 0, 1, 4, 10
LZMA2_ID, DELTA_ID, X86_ID = 0x21, 0x03, 0x04
PRESET_DICT = {0: 1 << 18, 1: 1 << 20, 2: 1 << 21, 3: 1 << 22, 4: 1 << 22, 5: 1 << 23, 6: 1 << 23, 7: 1 << 24, 8: 1 << 25, 9: 1 << 26}

_T64 = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0xC96C5795D7870F42 if _c & 1 else _c >> 1
    _T64.append(_c)


def crc64(data):
    c = 0xFFFFFFFFFFFFFFFF
    for b in data:
        c = _T64[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFFFFFFFFFF


def crc32(data):
    return zlib.crc32(data) & 0xFFFFFFFF


def vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


def check_size(check):
    return 0 if check == 0 else 4 << ((check - 1) // 3)


def check_field(check, data):
    if check == CHECK_CRC32:
        return struct.pack("<I", crc32(data))
    if check == CHECK_CRC64:
        return struct.pack("<Q", crc64(data))
    if check == CHECK_SHA256:
        return hashlib.sha256(data).digest()
    return bytes(range(1, check_size(check) + 1))  # a reserved id: nobody can verify it


def dict_prop(dict_size):
    """The LZMA2 property byte of the smallest dictionary that holds dict_size."""
    for p in range(40):
        if (2 | (p & 1)) << (p // 2 + 11) >= dict_size:
            return p
    return 40


def dict_bytes(prop):
    return 0xFFFFFFFF if prop == 40 else (2 | (prop & 1)) << (prop // 2 + 11)


def raw_lzma2(data, preset=6, dict_size=None, **opts):
    """(raw LZMA2 chunks of `data`, the 0x00 end byte included; the dictionary property byte)."""
    ds = dict_size or PRESET_DICT[preset & 15]
    f = dict(id=lzma.FILTER_LZMA2, preset=preset, dict_size=ds, **opts)
    return lzma.compress(data, format=lzma.FORMAT_RAW, filters=[f]), dict_prop(ds)


def chunks_of(raw):
    """The chunks of raw LZMA2 bytes as (control byte, uncompressed size, offset of the chunk, bytes of the chunk); the end byte is the
    last, with size 0."""
    out, p = [], 0
    while True:
        c = raw[p]
        if c == 0:
            out.append((0, 0, p, 1))
            return out
        if c >= 0x80:
            u = ((c & 0x1F) << 16) + (raw[p + 1] << 8) + raw[p + 2] + 1
            n = 5 + (c >= 0xC0) + (raw[p + 3] << 8) + raw[p + 4] + 1
        else:
            u = (raw[p + 1] << 8) + raw[p + 2] + 1
            n = 3 + u
        out.append((c, u, p, n))
        p += n


def block_header(prop=None, comp_size=None, uncomp_size=None, filters=None, flags=None, size_byte=None, padding=None, crc=None):
    """A block header.  filters: [(id, property bytes)], default one LZMA2 filter with the dictionary byte `prop`."""
    if filters is None:
        filters = [(LZMA2_ID, bytes([prop]))]
    if flags is None:
        flags = (len(filters) - 1) | (0x40 if comp_size is not None else 0) | (0x80 if uncomp_size is not None else 0)
    body = bytes([flags])
    if comp_size is not None:
        body += vli(comp_size)
    if uncomp_size is not None:
        body += vli(uncomp_size)
    for fid, props in filters:
        body += vli(fid) + vli(len(props)) + props
    total = (1 + len(body) + 4 + 3) & ~3
    if padding is None:
        padding = bytes(total - 4 - 1 - len(body))
    head = bytes([total // 4 - 1 if size_byte is None else size_byte]) + body + padding
    return head + struct.pack("<I", crc32(head) if crc is None else crc)


class Block:
    """One block: header, compressed data, padding and check field, each replaceable."""

    def __init__(self, content, check, raw=None, prop=None, header_sizes=False, preset=6, dict_size=None, header=None, padding=None,
                 check_bytes=None, **opts):
        self.content = content
        if raw is None:
            raw, prop = raw_lzma2(content, preset, dict_size, **opts)
        self.raw = raw
        self.prop = prop
        self.header = header if header is not None else block_header(prop, len(raw) if header_sizes else None, len(content) if header_sizes else None)
        self.padding = bytes(-(len(self.header) + len(raw)) % 4) if padding is None else padding
        self.check_bytes = check_field(check, content) if check_bytes is None else check_bytes

    @property
    def unpadded(self):
        return len(self.header) + len(self.raw) + len(self.check_bytes)

    @property
    def uncomp(self):
        return len(self.content)

    def bytes(self):
        return self.header + self.raw + self.padding + self.check_bytes


def index(records, count=None, padding=None, crc=None, indicator=0):
    body = bytes([indicator]) + vli(len(records) if count is None else count)
    for unpadded, uncomp in records:
        body += (unpadded if isinstance(unpadded, bytes) else vli(unpadded)) + (uncomp if isinstance(uncomp, bytes) else vli(uncomp))
    body += bytes(-len(body) % 4) if padding is None else padding
    return body + struct.pack("<I", crc32(body) if crc is None else crc)


def stream_header(check, flag0=0, magic=HEADER_MAGIC, crc=None):
    flags = bytes([flag0, check])
    return magic + flags + struct.pack("<I", crc32(flags) if crc is None else crc)


def stream_footer(index_len, check, flag0=0, magic=FOOTER_MAGIC, backward=None, crc=None):
    body = struct.pack("<I", index_len // 4 - 1 if backward is None else backward) + bytes([flag0, check])
    return struct.pack("<I", crc32(body) if crc is None else crc) + body + magic


def stream(blocks, check, records=None, header=None, footer=None, index_bytes=None):
    """A stream of Block objects (or ready block bytes with records given)."""
    body = b"".join(b.bytes() if isinstance(b, Block) else b for b in blocks)
    if records is None:
        records = [(b.unpadded, b.uncomp) for b in blocks]
    ix = index(records) if index_bytes is None else index_bytes
    return (stream_header(check) if header is None else header) + body + ix + (stream_footer(len(ix), check) if footer is None else footer)


def xz(contents, check=CHECK_CRC64, **kw):
    """One stream with a block per entry of `contents`."""
    return stream([Block(c, check, **kw) for c in contents], check)
