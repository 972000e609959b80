"""p-values for the BH tests (helper module, no tests in here): what test_gpu_count_sweeps.py and call_order_fixtures.py
both draw their vectors and column tables from."""
import numpy as np


def bh_values(m, rng):
    """NaN-free p-values: continuous, a tenth exactly 1, zeros, denormals, exact ties, crowds a few ulps below 1"""
    p = rng.random(m) ** 3
    p[rng.random(m) < 0.1] = 1.0
    special = np.r_[0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1e-300, 1.0, 0.5, 0.5,
                    1.0 - np.arange(1, 9) * 2.0 ** -53, np.full(8, 0.03125), np.full(5, 1.0 - 2.0 ** -53)]
    p[: min(m, special.size)] = special[:m]
    if m > 4000:
        p[100:1100] = 0.25                                                    # one value over a whole bucket
        p[2000:2400] = 1.0 - rng.integers(1, 6, size=400) * 2.0 ** -53         # crowd just below 1
        p[3000:3100] = rng.choice([5e-324, 1e-320, 0.0], size=100)
    return p[rng.permutation(m)]


def bh_columns_values(n, cols, rng):
    p = np.stack([bh_values(n, rng) for _ in range(cols)], axis=1)
    if cols > 1:
        p[:, 1] = rng.choice([1.0, 0.5, 0.0286, 0.2, 1e-5, 5e-324], size=n)     # discrete levels: long ties
    return p
