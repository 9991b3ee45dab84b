"""The numpy restatement of the solvers' sums (tests/reduction_restatement.py) on the CPU: its geometry against the table derived
from csrc/reduce_device.hpp, and every sum within 1e-13 of sum|terms| of math.fsum -- the suite's bound for a re-ordered fp64 sum
(tests/test_blas1_gpu.py). The GPU tests then hold the device to these functions bit for bit."""
import math

import numpy as np
import pytest

import reduction_restatement as R
from bitwise import same_bits

SUM_TOL = 1e-13
COUNTS = [1, 1024, 1025, 2813, 7813, 65_537]
GEOMETRY = {1: (1, 1), 1024: (1024, 1), 1025: (5, 205), 2813: (11, 256), 7813: (31, 253), 65_537: (257, 256)}
SIZES = [1, 2, 3, 127, 128, 129, 4097]


def close(got, terms):
    terms = np.asarray(terms, dtype=np.float64).ravel()
    return abs(got - math.fsum(terms)) <= SUM_TOL * float(np.sum(np.abs(terms)))


def samples(count, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(count) ** 2, rng.standard_normal(count)  # non-negative, mixed signs


@pytest.mark.parametrize("count", COUNTS)
def test_geometry_is_the_table_of_reduce_device_hpp(count):
    assert R.reduce_geometry(count) == GEOMETRY[count]
    slice_, blocks = R.reduce_geometry(count)
    assert (blocks - 1) * slice_ < count <= blocks * slice_ and blocks <= R.STAGE_BLOCKS  # every slice holds something


@pytest.mark.parametrize("count", COUNTS)
def test_reduce_is_an_accurate_sum(count):
    for v in samples(count, count):
        assert close(R.reduce(v), v)
        assert close(R.reduce_pcg(v, count, 1)[0], v)
        assert close(R.reduce_multi(v), v)
        assert same_bits(R.reduce_pcg(v, count, 1)[0], R.reduce(v))  # the same shape where there are no extras
    extra = samples(16, count + 1)[1]
    v = samples(count, count)[1]
    assert close(R.reduce(v, extra), np.concatenate([v, extra]))
    v0, v1 = samples(count, 7 * count)
    t0, t1 = R.reduce_pcg(np.concatenate([v0, v1]), count, 2)
    assert same_bits(t0, R.reduce(v0)) and same_bits(t1, R.reduce(v1))


def test_extras_enter_the_second_stage_after_the_slice_sums():
    """An order that shows in the result: positions 0 and 256 of the second stage share thread 0. With [slice sum | extras] the
    slice sum 2^60 meets the last extra, -2^60, there and cancels exactly, so the 1.0 in thread 1 survives; with the extras first
    thread 0 adds 1.0 to 2^60 and loses it."""
    big = 2.0 ** 60
    extras = np.zeros(256)
    extras[255] = -big                     # position 256 of [sum | extras]: thread 0's second element
    extras[0] = 1.0                        # position 1: thread 1
    assert R.reduce([big], extras) == 1.0  # thread 0: (0 + 2^60) + -2^60 = 0, then the tree adds thread 1's 1.0
    assert R.workgroup_sum(np.concatenate([extras, [big]])) == 0.0  # extras first: thread 0 holds (0 + 1.0) + 2^60 = 2^60


@pytest.mark.parametrize("n", SIZES)
def test_stream_partials_are_an_accurate_sum(n):
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    for a, b in ((x, y), (x, x)):
        p = R.stream_partials(a, b)
        assert len(p) == R.stream_count(n) == max(1, ((n >> 1) + 63) // 64)
        assert close(R.reduce(p), a * b)
    two = R.stream_partials_two(x, y)
    assert same_bits(two[:len(two) // 2], R.residual_partials(x)) and same_bits(two[len(two) // 2:], R.stream_partials(x, y))
    assert same_bits(R.dot_partials(x, y), R.stream_partials(x, y))


def test_stream_partials_use_a_fused_multiply_add_and_add_the_tail_last():
    """One pair whose second product only survives a fused operation: a1 * b1 = 1 - 2^-60 exactly, which rounds to 1.0 on its
    own; fma(a1, b1, -1.0) keeps -2^-60."""
    a = np.array([1.0, 1.0 + 2.0 ** -30])
    b = np.array([-1.0, 1.0 - 2.0 ** -30])
    assert R.stream_partials(a, b)[0] == -(2.0 ** -60)
    # n = 3: the tail joins lane 0 after the pair: (fma(a1, b1, fma(a0, b0, 0)), then fma(a2, b2, .))
    a3, b3 = np.array([2.0 ** 60, 1.0, 1.0]), np.array([1.0, 1.0, -(2.0 ** 60)])
    assert R.stream_partials(a3, b3)[0] == 0.0  # (2^60 + 1) rounds to 2^60 first; the tail first would leave 1.0


@pytest.mark.parametrize("n", SIZES)
def test_grid_partials_are_an_accurate_sum(n):
    """n columns; three grid rows, so that a slot of the second and third row is in play."""
    rng = np.random.default_rng(100 + n)
    x, s = rng.standard_normal(3 * n), rng.standard_normal(3 * n)
    direct, lds, ell = R.rowdirect_partials(x, s, n), R.rowlds_partials(x, s, n), R.ell_partials(x, s)
    assert len(direct) == 3 * ((n + 255) // 256) and len(lds) == 3 * ((n + 127) // 128) and len(ell) == (3 * n + 255) // 256
    for p in (direct, lds, ell):
        assert close(R.reduce(p), x * s)
    # slot = grid row * blocks + block: the middle row's slots hold the middle row's terms
    per = len(lds) // 3
    assert close(float(np.sum(lds[per:2 * per])), x[n:2 * n] * s[n:2 * n])
    per = len(direct) // 3
    assert close(float(np.sum(direct[per:2 * per])), x[n:2 * n] * s[n:2 * n])


def test_sign_of_zero():
    """Every sum starts at +0.0: all -0.0 terms give +0.0."""
    neg = np.full(300, -0.0)
    for got in (R.reduce(neg), R.reduce(neg[:1], neg[:3]), R.reduce(np.full(1500, -0.0)), R.reduce_multi(neg), R.reduce_pcg(neg, 300, 1)[0],
                R.workgroup_sum(neg)):
        assert same_bits(got, 0.0)
    one = np.array([1.0, 1.0, 1.0])
    for p in (R.stream_partials(-one, 0.0 * one), R.rowdirect_partials(-one, 0.0 * one, 3), R.rowlds_partials(-one, 0.0 * one, 3)):
        assert same_bits(p, np.zeros(len(p)))
    assert same_bits(R.stream_partials([-1.0], [0.0]), [0.0])
