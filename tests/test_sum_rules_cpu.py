"""The two fixed-order sums (tests/sum_rules.py), the numpy side of every bit test: each against its rule written out element by element
with Python scalars, and the `axis` forms against the calls row by row."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sum_rules as SR  # noqa: E402
from distance_cases import _same_bits  # noqa: E402


def _literal(v, parts, tree):
    """The rule, element by element: the list of all partials after the last meeting."""
    part = [np.float32(0)] * parts
    for j in range(len(v)):
        part[j % parts] = part[j % parts] + v[j]
    for s in tree:
        part = [part[i] + part[i ^ s] for i in range(parts)]
    return part


def test_sum1024_is_the_stated_tree():
    """The vectorised sum against the rule written out element by element, and against float64 within the rounding of 1024 + 10 adds."""
    rng = np.random.default_rng(3)
    for N in (1, 63, 1023, 1024, 1025, 2500):
        v = rng.normal(size=N).astype(np.float32)
        part = _literal(v, 1024, (32, 16, 8, 4, 2, 1, 512, 256, 128, 64))
        assert all(_same_bits(np.array([p]), np.array([part[0]])) for p in part)  # every partial ends with the same bits
        assert _same_bits(np.array([SR.sum1024(v)]), np.array([part[0]]))
        assert abs(float(part[0]) - v.astype(np.float64).sum()) <= 16 * 2.0 ** -24 * np.abs(v).sum()


def test_sum64_is_the_stated_tree():
    """Likewise.  An element passes through at most ceil(129 / 64) + 6 = 9 adds, and (1 + u)^9 - 1 < 10 u."""
    rng = np.random.default_rng(4)
    for N in (1, 63, 64, 65, 129):
        v = rng.normal(size=N).astype(np.float32)
        part = _literal(v, 64, (32, 16, 8, 4, 2, 1))
        assert all(_same_bits(np.array([p]), np.array([part[0]])) for p in part)
        assert _same_bits(np.array([SR.sum64(v)]), np.array([part[0]]))
        assert abs(float(part[0]) - v.astype(np.float64).sum()) <= 10 * 2.0 ** -24 * np.abs(v).sum()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rule", [SR.sum64, SR.sum1024])
def test_axis_forms_are_the_calls_row_by_row(rule, dtype):
    rng = np.random.default_rng(5)
    for N in (1, 65, 1030):
        a = rng.normal(size=(3, N, 2)).astype(dtype)
        rows = np.array([[rule(np.ascontiguousarray(a[i, :, j])) for j in range(2)] for i in range(3)])
        got = rule(a, axis=1)
        assert got.dtype == dtype and rule(a[0, :, 0]).dtype == dtype
        assert _same_bits(got, rows)
        assert _same_bits(rule(np.moveaxis(a, 1, -1)), rows) and _same_bits(rule(np.moveaxis(a, 1, 0), axis=0), rows)
