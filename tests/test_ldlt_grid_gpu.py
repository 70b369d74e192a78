"""The grid-wide LDL^T alone (orbba_debug_ldlt_grid, csrc/ldlt_grid.h) on SPD systems B^T B + I: D = 132 (just past
the LDS path's 128), 258 (no multiple of 16 or 32) and 600 (19 block columns).  The relative residual
|Ax - b| / (|A| |x| + |b|) may be 16 x that of numpy.linalg.solve on the same system (the project's usual factor); a
zero first pivot gives ok == 0; two runs are bit-identical."""
import ctypes as C

import numpy as np
import pytest

from orb_slam2_refactored_amd._lib import check, lib, ptr

pytestmark = pytest.mark.gpu


def grid_solve(A, b):
    D = len(b)
    x, ok = np.zeros(D), np.zeros(1, np.int32)
    check(lib().orbba_debug_ldlt_grid(ptr(np.ascontiguousarray(A)), ptr(np.ascontiguousarray(b)), D, ptr(x), ptr(ok), 0),
          "orbba_debug_ldlt_grid")
    return x, int(ok[0])


def residual(A, x, b):
    return np.linalg.norm(A @ x - b) / (np.linalg.norm(A, 2) * np.linalg.norm(x) + np.linalg.norm(b))


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
