"""The block tree's definition (include/znippy_hip.h), checked on the CPU: the numpy reference of tests/b3_tree.py against
the oracle's BLAKE3 and the known answers.  The GPU tests compare the library with this reference byte for byte."""
import json
import os

import pytest

import b3_tree
import gen

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [131_073, 132_096, 132_097, 262_144, 262_145, 300_001, 655_361, 8_388_609]


@pytest.mark.parametrize("n", LENGTHS)
def test_entries_fold_to_the_digest(oracle, n):
    x = gen.incompressible(n % 251, n)
    e = b3_tree.entries(x)
    assert e.shape == (-(-n // b3_tree.BLK), 32)
    assert b3_tree.digest_from_entries(e) == oracle.blake3(x)


def test_a_row_of_one_block_has_no_entries():
    assert b3_tree.entries(gen.incompressible(1, 131_072)).shape == (0, 32)
    assert b3_tree.n_entries(131_072) == 0 and b3_tree.n_entries(131_073) == 2 and b3_tree.n_entries(1 << 32) == 0
    assert list(b3_tree.row_first([5_000, 131_073, 131_072, 300_001])) == [0, 0, 2, 2, 5]


def test_entry_depends_on_the_chunk_counter():
    """Two blocks of identical content at different places of a row have different entries."""
    part = gen.incompressible(3, b3_tree.BLK)
    e = b3_tree.entries(part * 3)
    assert len({bytes(e[k]) for k in range(3)}) == 3


def test_reference_reproduces_the_known_answers():
    kat = json.load(open(os.path.join(HERE, "golden", "blake3_kat.json")))
    assert b3_tree.blake3(b"").hex() == kat["empty"]
    assert b3_tree.blake3(b"abc").hex() == kat["abc"]
    for n, h in kat["pattern251"].items():
        assert b3_tree.blake3(gen.binary(int(n))).hex() == h, n
