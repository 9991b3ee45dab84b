"""Comparison of doubles as bit patterns (test infrastructure): -0.0 is not +0.0, a NaN equals only the same NaN."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))
