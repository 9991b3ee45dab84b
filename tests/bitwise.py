"""Comparison of doubles as bit patterns (test infrastructure): -0.0 is not +0.0, a NaN equals only the same NaN."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_bits_nan_as_class(got, want):
    """same_bits for results that hold NaN: where `want` is NaN `got` must be a NaN (of any sign and payload -- inf - inf is the
    default NaN with the sign bit set on x86 and clear on the GPU, and an input NaN's payload travels differently), everywhere else the
    bit patterns must be equal, so +-inf and +-0.0 are exact. Returns True, or raises AssertionError with a report: how many elements
    are non-finite in `got` but finite in `want` (a leak) and the reverse, and the first few indices of each."""
    got, want = np.ascontiguousarray(got, dtype=np.float64).ravel(), np.ascontiguousarray(want, dtype=np.float64).ravel()
    assert got.shape == want.shape, ("shapes differ", got.shape, want.shape)
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), bits(got) != bits(want))
    if not bad.any():
        return True
    leaked = np.flatnonzero(~np.isfinite(got) & np.isfinite(want))
    lost = np.flatnonzero(np.isfinite(got) & ~np.isfinite(want))
    other = np.flatnonzero(bad & (np.isfinite(got) == np.isfinite(want)))
    raise AssertionError(f"{int(bad.sum())} of {len(want)} elements differ: {len(leaked)} non-finite where a finite value is wanted (first at "
                         f"{leaked[:8].tolist()}), {len(lost)} finite where a non-finite value is wanted (first at {lost[:8].tolist()}), "
                         f"{len(other)} other bit differences (first at {other[:8].tolist()})")
