"""Rank selection of the Chebyshev low-rank prepared product (rpgp_lowrank_select, host code of csrc/rpgp_lowrank.hip,
through ctypes; no GPU): monotone in the half-width, rank 1 for a constant kernel, "not served" above the largest rank, and
the claimed tail bound covers the float64 error of the truncated expansion on a dense grid."""
import ctypes

import numpy as np
import pytest


def _select(h, p_max=64, coef=False):
    from rpgp_amd import _lib
    lib = _lib.load()
    p, tail = ctypes.c_int(-1), ctypes.c_double(-1.0)
    c = np.zeros((p_max, p_max), dtype=np.float64) if coef else None
    _lib.check(lib.rpgp_lowrank_select(float(h), p_max, ctypes.byref(p), ctypes.byref(tail),
                                       c.ctypes.data if coef else None), "rpgp_lowrank_select")
    return p.value, tail.value, (c[:p.value, :p.value] if coef else None)


def test_rank_is_monotone_in_the_half_width():
    ranks = [_select(h)[0] for h in np.linspace(0.0, 8.0, 33)]
    assert all(r > 0 for r in ranks)
    assert all(a <= b for a, b in zip(ranks, ranks[1:])), ranks
    assert 30 <= _select(4.61)[0] <= 45                   # the benchmark's C4 range


def test_constant_kernel_is_rank_one():
    p, tail, c = _select(0.0, coef=True)
    assert p == 1 and tail <= 2.0 ** -26
    assert abs(c[0, 0] - 1.0) < 1e-14


def test_not_served_above_the_largest_rank():
    assert _select(12.0)[0] == 0                          # needs more than 64
    assert _select(12.0, p_max=128)[0] > 64
    assert _select(float("nan"))[0] == 0


def _cheb(x, p):
    T = np.empty((p, x.size))
    T[0] = 1.0
    if p > 1:
        T[1] = x
    for m in range(2, p):
        T[m] = 2.0 * x * T[m - 1] - T[m - 2]
    return T


@pytest.mark.parametrize("h", [0.5, 2.0, 4.6, 7.0])
def test_claimed_tail_bounds_the_truncation_error(h):
    p, tail, c = _select(h, coef=True)
    assert 0 < p <= 64 and tail <= 2.0 ** -26
    x = np.linspace(-1.0, 1.0, 801)
    T = _cheb(x, p)
    approx = T.T @ c @ T
    exact = np.exp2(-h * h * (x[:, None] - x[None, :]) ** 2)
    err = np.abs(approx - exact).max()
    assert err <= tail, (h, p, err, tail)
    # ... and the bound is not vacuous: one rank less would not do
    if p > 1:
        approx1 = T[:p - 1].T @ c[:p - 1, :p - 1] @ T[:p - 1]
        assert np.abs(approx1 - exact).max() > 1e-10
