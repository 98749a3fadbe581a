"""The model (bz_model.py) and the builder (bz_build.py) of the bzip2 tests against Python's bz2: what the GPU tests expect comes
from these two, so they are checked first, on the CPU."""
import bz2
import zlib

import pytest

import bz_build as B
import bz_model as M
import gen


def test_crc_is_the_reflection_of_zlibs():
    for data in (b"", b"a", b"123456789", gen.binary(1000)):
        assert M.crc(data) == M.crc_by_reflection(data)
    assert M.crc(b"123456789") == 0xFC891918  # CRC-32/BZIP2 check value
    assert zlib.crc32(b"123456789") == 0xCBF43926


@pytest.mark.parametrize("data", [b"", b"a", b"a" * 4, b"a" * 5, b"a" * 255, b"a" * 256, b"a" * 259 + b"b", b"aaaa\x00" * 300, b"aaaaaaaaa" + b"\x05" * 3,
                                  bytes(range(256)) * 3, b"ab" * 500, b"abcab" * 200, gen.text(3000), gen.incompressible(3, 2000), bytes(5000)])
def test_model_reads_what_bz2_writes(data):
    c = bz2.compress(data, 1)
    status, content, streams, blocks, records = M.walk(c)
    assert (status, content, streams) == (M.OK, data, 1)
    assert blocks == len(records) == len(M.magic_positions(c))
    assert M.expect(c, len(data))[:2] == (M.OK, data)
    assert M.expect(c, len(data) - 1)[0] == (M.E_DST_SMALL if data else M.OK)


def test_model_reads_several_blocks_and_streams():
    data = gen.pseudo_text(250_000)
    c = bz2.compress(data, 1)
    status, content, streams, blocks, records = M.walk(c)
    assert (status, content, streams, blocks) == (M.OK, data, 1, 3)
    assert [r[0] % 8 for r in records] == [0, 4, 3] or len({r[0] % 8 for r in records}) > 1  # blocks start at any bit
    two = bz2.compress(b"one") + bz2.compress(b"") + bz2.compress(b"three") + b"\0\0rest"
    assert M.walk(two)[:4] == (M.OK, b"onethree", 3, 2)
    assert bz2.decompress(two) == b"onethree"


@pytest.mark.parametrize("data", [b"a", b"hello hello hello", b"a" * 300, bytes(range(256)), gen.text(1500), b"ab" * 300, b"aaaa\x04aaaa"])
def test_builder_writes_what_bz2_reads(data):
    for kw in ({}, {"n_groups": 6}):
        s = B.stream([B.block_fields(data, **kw)])
        assert bz2.decompress(s) == data
        assert M.walk(s)[:4] == (M.OK, data, 1, 1)
    assert B.rle1(data) == B.rle1(M.unrle1(B.rle1(data)))
    assert M.unrle1(B.rle1(data)) == data


def test_builder_fields():
    data = gen.text(700)
    # a code of length 20: the end-of-block symbol's neighbour gets it, the others stay flat
    b = B.block_fields(data)
    alpha = len(b.used) + 2
    lens = B.flat_lens(alpha)
    rare = min(set(range(2, alpha - 1)) - set(b.symbols), default=None)
    if rare is not None:
        lens[rare] = 20
        b.tables = [list(lens), list(lens)]
        assert bz2.decompress(B.stream([b])) == data
    # more selectors than 18002: read and discarded
    b = B.block_fields(data)
    b.n_selectors = 18010
    s = B.stream([b])
    assert bz2.decompress(s) == data and M.walk(s)[:2] == (M.OK, data)
    # a block from symbols
    blk, content = B.block_from_symbols(list(range(1, 255)), [5, 9, 0, 1, 77, 200, 3, 3, 8], orig=3)
    s = B.stream([blk])
    assert bz2.decompress(s) == content and M.walk(s)[:2] == (M.OK, content)
    # (a block that ends in four equal bytes without their count is the one thing the model reads and libbz2 refuses; no writer
    # produces it, and accepted_block() below keeps hand-built blocks away from it)
    blk, content = B.accepted_block(list(range(1, 255)), [5, 9, 0, 1, 77, 200, 3, 3, 8])
    assert bz2.decompress(B.stream([blk])) == content
    # damage
    b = B.block_fields(data)
    b.randomised = 1
    assert M.walk(B.stream([b]))[0] == M.E_UNSUPPORTED
    b = B.block_fields(data)
    b.crc ^= 1
    assert M.walk(B.stream([b]))[0] == M.E_CHECKSUM
    assert M.walk(B.stream([B.block_fields(data)], crc=5))[0] == M.E_CHECKSUM
    assert M.walk(B.stream([B.block_fields(data)], head=b"BZh0"))[0] == M.E_CORRUPT
    assert M.walk(B.stream([B.block_fields(data)])[:-3])[0] == M.E_CORRUPT


def test_header_flips_stay_decidable():
    """the stream of the GPU suite's bit-flip test: at most 2 % of the flips may be beyond the model's step bound"""
    s = bz2.compress(gen.text(2000), 1)
    undecided = 0
    for bit in range(32, 232):
        try:
            st = M.walk(B.flip(s, bit), 2000)[0]
            assert st in (M.OK, M.E_CORRUPT, M.E_UNSUPPORTED, M.E_CHECKSUM, M.E_DST_SMALL)
        except M.Undecided:
            undecided += 1
    assert undecided <= 4
