"""The grid-wide LDL^T alone (orbba_debug_ldlt_grid, csrc/ldlt_grid.h) on SPD systems B^T B + I: D = 132 (just past
the LDS path's 128), 258 (no multiple of 16 or 32) and 600 (19 block columns).  The relative residual
|Ax - b| / (|A| |x| + |b|) may be 16 x that of numpy.linalg.solve on the same system (the project's usual factor); a
zero first pivot gives ok == 0; two runs are bit-identical.

With tests/ldlt_ref.py's systems at D = 132 and 258, as tests/test_ldlt_paths_gpu.py holds the other two solves to
them: exact_system comes back bit for bit; a zero pivot at 0, 5, 15, 16 or D - 1 and +inf / nan on the diagonal give
ok == 0 with x untouched, all-negative pivots ok == 1 and the exact x0; on quasi_definite (negative pivots) the forward
error against the longdouble solution is within 16 x that of the float64 restatement."""
import ctypes as C

import numpy as np
import pytest

import ldlt_ref as R
from orb_slam2_refactored_amd._lib import check, lib, ptr

pytestmark = pytest.mark.gpu


def grid_solve(A, b, fill=0.0):
    """x starts as `fill` everywhere: the entry leaves it alone when ok == 0"""
    D = len(b)
    x, ok = np.full(D, float(fill)), np.zeros(1, np.int32)
    check(lib().orbba_debug_ldlt_grid(ptr(np.ascontiguousarray(A)), ptr(np.ascontiguousarray(b)), D, ptr(x), ptr(ok), 0),
          "orbba_debug_ldlt_grid")
    return x, int(ok[0])


def residual(A, x, b, norm_A=None):
    """norm_A: |A|_2 where the caller already has it"""
    nA = np.linalg.norm(A, 2) if norm_A is None else norm_A
    return np.linalg.norm(A @ x - b) / (nA * np.linalg.norm(x) + np.linalg.norm(b))


@pytest.mark.parametrize("D", [132, 258, 600])
def test_residual_against_numpy(D):
    rng = np.random.default_rng(D)
    B = rng.normal(size=(D, D))
    A = B.T @ B + np.eye(D)
    A = 0.5 * (A + A.T)
    b = rng.normal(size=D)
    x, ok = grid_solve(A, b)
    x2, _ = grid_solve(A, b)
    rg, rn = residual(A, x, b), residual(A, np.linalg.solve(A, b), b)
    print(f"D {D}: residual grid {rg:.3g}, numpy {rn:.3g}, ratio {rg / rn:.3g}")
    assert ok == 1 and x.tobytes() == x2.tobytes()
    assert rg <= 16 * rn


def test_zero_pivot():
    rng = np.random.default_rng(1)
    B = rng.normal(size=(132, 132))
    A = B.T @ B + np.eye(132)
    A[0, 0] = 0.0
    x, ok = grid_solve(A, rng.normal(size=132))
    assert ok == 0 and not x.any()


def grid_solve_twice(A, b, fill=0.0):
    x, ok = grid_solve(A, b, fill)
    x2, ok2 = grid_solve(A, b, fill)
    assert ok == ok2 and x.tobytes() == x2.tobytes(), "two runs differ"
    return x, ok


@pytest.mark.parametrize("D", [132, 258])
def test_exact(D):
    A, b, x0 = R.exact_system(D, 0)
    x, ok = grid_solve_twice(A, b)
    assert ok == 1
    assert x.tobytes() == x0.tobytes(), np.flatnonzero(x != x0)


@pytest.mark.parametrize("D", [132, 258])
def test_ok_rule(D):
    A0, b0, _ = R.exact_system(D, 0)
    cases = [(f"zero_at {k}",) + R.exact_system(D, 0, zero_at=k)[:2] for k in (0, 5, 15, 16, D - 1)]
    for k in (0, 16):
        for v in (np.inf, np.nan):
            A = A0.copy()
            A[k, k] = v
            cases.append((f"{v} at {k}", A, b0))
    for label, A, b in cases:
        x, ok = grid_solve_twice(A, b, fill=7.0)
        assert ok == 0 and (x == 7.0).all(), label   # x untouched
    A, b, x0 = R.exact_system(D, 0, signs=(-1,))
    x, ok = grid_solve_twice(A, b)
    assert ok == 1 and x.tobytes() == x0.tobytes()


@pytest.mark.parametrize("D", [132, 259])
def test_forward_error_negative_pivots(D):
    A, b, xld, e64 = R.quasi_definite_reference(D)
    x, ok = grid_solve_twice(A, b)
    eg = R.forward_error(x, xld)
    print(f"grid {D} quasi_definite: device {eg:.3g}, reference {e64:.3g}, ratio {eg / e64:.3g}")
    assert ok == 1
    assert eg <= 16 * e64
