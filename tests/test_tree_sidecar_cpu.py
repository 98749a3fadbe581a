"""znippy_amd/block_tree.py: the block tree's layout against tests/b3_tree.py, and the sidecar file `<archive>.b3t` — round trip
and every malformed shape read_sidecar has to name.  No GPU."""
import struct

import numpy as np
import pytest

import b3_tree

LENGTHS = [0, 1, 65536, 131072, 131073, 196608, 262145, (1 << 32) - 1, 1 << 32]


def test_layout_against_the_reference():
    from znippy_amd import block_tree as bt
    assert bt.BLK == b3_tree.BLK == 1 << bt.BLOCK_LOG
    for n in LENGTHS:
        assert bt.n_entries(n) == b3_tree.n_entries(n), n
    assert bt.n_entries((1 << 32) - 1) == 32768 and bt.n_entries(1 << 32) == 0
    assert [bt.n_entries(n) for n in LENGTHS[:7]] == [0, 0, 0, 0, 2, 2, 3]
    total, first = bt.layout(LENGTHS)
    assert first.dtype == np.uint64 and np.array_equal(first, b3_tree.row_first(LENGTHS))
    assert total == int(first[-1]) == 2 + 2 + 3 + 32768
    total0, first0 = bt.layout([])
    assert total0 == 0 and first0.tolist() == [0]
    assert bt.layout(np.array([300001, 5], np.uint64))[0] == 3


def test_sidecar_round_trip(tmp_path):
    from znippy_amd import block_tree as bt
    entries = np.random.default_rng(1).integers(0, 256, (7, 32), dtype=np.uint8)
    p = tmp_path / "a.znippy.b3t"
    assert bt.sidecar_path(tmp_path / "a.znippy") == str(p)
    bt.write_sidecar(p, 5, entries)
    raw = p.read_bytes()
    assert len(raw) == 32 + 32 * 7
    assert raw[:8] == b"ZNPYB3T1" and struct.unpack("<IIQQ", raw[8:32]) == (17, 0, 5, 7) and raw[32:] == entries.tobytes()
    n_rows, back = bt.read_sidecar(p)
    assert n_rows == 5 and back.shape == (7, 32) and back.dtype == np.uint8 and np.array_equal(back, entries)
    bt.write_sidecar(p, 3, np.zeros((0, 32), np.uint8))    # an archive of small rows: the header alone
    assert p.stat().st_size == 32
    n_rows, back = bt.read_sidecar(p)
    assert n_rows == 3 and back.shape == (0, 32)
    bt.write_sidecar(p, 1, entries.reshape(-1))            # flat bytes are entries too
    assert np.array_equal(bt.read_sidecar(p)[1], entries)
    with pytest.raises(ValueError):
        bt.write_sidecar(p, 1, np.zeros(33, np.uint8))


def test_read_sidecar_rejects(tmp_path):
    from znippy_amd import block_tree as bt
    entries = np.arange(64, dtype=np.uint8).reshape(2, 32)
    good = tmp_path / "good.b3t"
    bt.write_sidecar(good, 2, entries)
    raw = good.read_bytes()
    cases = {
        "short": (raw[:31], "short"),
        "empty": (b"", "short"),
        "magic": (b"ZNPYB3T2" + raw[8:], "magic"),
        "log": (raw[:8] + struct.pack("<I", 16) + raw[12:], "block log"),
        "long": (raw + bytes(32), "n_entries"),
        "cut": (raw[:-1], "n_entries"),
        "count": (raw[:24] + struct.pack("<Q", 3) + raw[32:], "n_entries"),
    }
    for name, (data, word) in cases.items():
        p = tmp_path / f"{name}.b3t"
        p.write_bytes(data)
        with pytest.raises(ValueError) as e:
            bt.read_sidecar(p)
        assert word in str(e.value), (name, str(e.value))
    assert bt.read_sidecar(good)[0] == 2
