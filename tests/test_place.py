"""gpu_cases.place: where a row lands for each mode of the far layouts (test_gpu_far.py).  No GPU."""
import numpy as np
import pytest

from gpu_cases import FAR_LINE, place

T = FAR_LINE
SIZES = np.array([10240, 0, 300, 65536, 70001, 256, 1 << 20, 17], np.uint64)
PACKED = (np.cumsum(SIZES) - SIZES).astype(np.uint64)                      # back to back: every alignment
GAPPED = (PACKED + np.arange(len(SIZES), dtype=np.uint64) * np.uint64(3) + np.uint64(5))   # odd offsets, 3 bytes between rows
ALIGNED = np.arange(len(SIZES), dtype=np.uint64) * np.uint64(2 << 20)        # every offset a multiple of 128


@pytest.mark.parametrize("offs", [PACKED, GAPPED, ALIGNED], ids=["packed", "gapped", "aligned"])
def test_place_every_mode(offs):
    ends = offs + SIZES
    s = place(offs, SIZES, "above")
    assert s == T + (64 << 10) and s % 128 == 0
    assert all(int(o) + s >= T for o in offs)
    for k in range(len(SIZES)):
        s = place(offs, SIZES, "start_at_line", k)
        assert s % 128 == 0 and 0 < s <= T
        at = int(offs[k]) + s
        assert T <= at < T + 128
        assert (at == T) == (int(offs[k]) % 128 == 0)                       # exactly at the line when its alignment allows
        assert all(int(e) + s <= at for e in ends[:k]) and all(int(o) + s >= T for o in offs[k + 1:])
        if SIZES[k] < 256:
            with pytest.raises(AssertionError):
                place(offs, SIZES, "straddle", k)
            continue
        s = place(offs, SIZES, "straddle", k)
        assert s % 128 == 0 and 0 < s < T
        a, b = int(offs[k]) + s, int(ends[k]) + s
        assert a < T < b                                                     # the line is inside row k ...
        assert abs((T - a) - int(SIZES[k]) // 2) < 128                       # ... near its middle
        assert all(int(e) + s <= T for e in ends[:k]) and all(int(o) + s >= T for o in offs[k + 1:])
        assert all((int(o) + s) % 16 == int(o) % 16 for o in offs)           # alignment classes are kept


def test_place_rejects_unknown_mode():
    with pytest.raises(ValueError):
        place(PACKED, SIZES, "below", 0)
