"""CPU: the launch rule restated in tests/rank_support.py (rows_per_wave, chunk_table_rows) against itself, for every
rows-per-wave choice and compute-unit counts from one to more than any device has."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rank_support import chunk_table_rows, rows_per_wave  # noqa: E402


@pytest.mark.parametrize("cus", [1, 8, 64, 256, 304])
@pytest.mark.parametrize("ch", [64, 32, 16, 8, 4, 2, 1])
def test_chunk_table_rows_selects_its_rows_per_wave(ch, cus):
    n = chunk_table_rows(ch, cus)
    assert rows_per_wave(n, cus) == ch
    if ch > 1:
        assert n % ch                                   # the table ends in a partial chunk
    smallest = n
    while smallest > 1 and rows_per_wave(smallest - 1, cus) == ch:
        smallest -= 1
    assert rows_per_wave(smallest, cus) == ch
    if ch > 1:
        assert rows_per_wave(smallest - 1, cus) == ch // 2 and n - smallest <= 38
    else:
        assert smallest == 1                            # one row per wave is what every short table gets
