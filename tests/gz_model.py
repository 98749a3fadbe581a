"""What znippy_gunzip_batch must say about one gzip file, in Python: the content of all members, how many members, and how many
pieces a wave of its own decodes for a given seg_min.  The arbiter of content and validity is `gzip.decompress`; the header rule
(method, reserved flag bits: ZNIPPY_E_UNSUPPORTED) is that of csrc/tar_rules.h, restated in targz_model.gzip_header.

The piece count rests on two properties of zlib that this module observes rather than assumes:
  - a position inside a member's DEFLATE stream is a block boundary behind a stored block exactly when the stream up to it, with a
    final empty stored block appended, is a complete stream for raw inflate (inside a Huffman block the five appended bytes are
    symbols, inside a stored block they are data: the stream does not end);
  - raw inflate with a fresh window (decompressobj(-15)) started at such a boundary succeeds behind a full flush and fails with
    "invalid distance too far back" where a match reaches in front of the boundary: the piece cannot be decoded alone and joins
    the run in front of it (and that one its predecessor, until the joined run decodes alone).
The candidate rule is the one of include/znippy_hip.h: every position behind 00 00 FF FF and every 1F 8B 08, in position order; a
flush candidate closer than seg_min to the candidate kept before it (byte 0 is one) is dropped; an item without kept candidates, or
with more raw candidates than 16 + len / 256, is decoded by one wave."""
import gzip
import zlib

import targz_model as T

E_DST_SMALL, E_CORRUPT, E_UNSUPPORTED, E_CHECKSUM, E_INVAL = -4, -5, -6, -7, -1
SEG_MIN_DEFAULT = 256
END_BLOCK = b"\x01\x00\x00\xff\xff"


def candidates(data, seg_min):
    """(kept candidates behind byte 0 as (pos, kind) with kind 0 = flush, 1 = member; whether the raw list overflowed)"""
    raw = []
    at = data.find(b"\x00\x00\xff\xff")
    while at >= 0:
        if at + 4 < len(data):
            raw.append((at + 4, 0))
        at = data.find(b"\x00\x00\xff\xff", at + 1)
    at = data.find(b"\x1f\x8b\x08", 1)
    while at >= 0:
        raw.append((at, 1))
        at = data.find(b"\x1f\x8b\x08", at + 1)
    raw.sort()
    kept, last = [], 0
    for pos, kind in raw:
        if kind == 0 and pos - last < seg_min:
            continue
        kept.append((pos, kind))
        last = pos
    return kept, len(raw) > 16 + len(data) // 256


def members_of(data):
    """[(header start, first DEFLATE byte, first byte behind the stream, content)] of a valid file"""
    out, at = [], 0
    while at < len(data):
        rc, off = T.gzip_header(data[at:])
        assert rc == 0, (at, rc)
        d = zlib.decompressobj(-15)
        content = d.decompress(data[at + off:])
        assert d.eof
        end = len(data) - len(d.unused_data)
        out.append((at, at + off, end, content))
        at = end + 8
        while at < len(data) and data[at] == 0:
            at += 1
    return out


def is_boundary(data, start, pos):
    d = zlib.decompressobj(-15)
    try:
        d.decompress(data[start:pos] + END_BLOCK)
    except zlib.error:
        return False
    return d.eof and d.unused_data == b""


def decodes_alone(data, a, b):
    try:
        zlib.decompressobj(-15).decompress(data[a:b])
    except zlib.error as e:
        assert "too far back" in str(e), e
        return False
    return True


def expect(data, seg_min=0):
    """(content, members, segments) of a file that gzip.decompress accepts"""
    content = gzip.decompress(data)
    if not data:
        return content, 0, 0
    mem = members_of(data)
    assert b"".join(m[3] for m in mem) == content
    kept, overflow = candidates(data, seg_min or SEG_MIN_DEFAULT)
    if overflow or not kept:
        return content, len(mem), 1
    flush = [p for p, k in kept if k == 0]
    segments = 0
    for _, start, end, _ in mem:
        cuts = [start] + [p for p in flush if start < p < end and is_boundary(data, start, p)] + [end]
        runs = [start]
        for a, b in zip(cuts[1:-1], cuts[2:]):
            if decodes_alone(data, a, b):
                runs.append(a)
            else:
                while len(runs) > 1 and not decodes_alone(data, runs[-1], b):
                    runs.pop()
        segments += len(runs)
    return content, len(mem), segments


def outcome(data, room):
    """what a possibly damaged file must give in a room of `room` bytes: ("ok", content), ("dst",), ("unsup",) or ("bad",).
    gzip.decompress decides between ok and bad; a header it accepts whose method is not 8 or whose reserved flag bits are set is
    unsup (it reads every member header the way the first one is read here: the walk below goes from member to member as far as
    raw inflate carries it)."""
    at = 0
    while at < len(data):
        rc, off = T.gzip_header(data[at:])
        if rc == E_UNSUPPORTED:
            return ("unsup",)
        if rc != 0:
            break
        d = zlib.decompressobj(-15)
        try:
            d.decompress(data[at + off:])
        except zlib.error:
            break
        if not d.eof:
            break
        at = len(data) - len(d.unused_data) + 8
        while at < len(data) and data[at] == 0:
            at += 1
    try:
        content = gzip.decompress(data)
    except (OSError, EOFError, zlib.error):
        return ("bad",)
    return ("ok", content) if len(content) <= room else ("dst",)
