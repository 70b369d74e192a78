"""Pins tests/ldlt_ref.py, the references and generators the LDL^T GPU tests (test_ldlt_paths_gpu.py,
test_ldlt_grid_gpu.py) rest on: exact_system really is exact under the float64 factorisation at every size those
tests use, zero_at is found at exactly that pivot, the float64 run agrees with numpy.linalg.solve at residual level,
and the longdouble run really carries more precision than the float64 one."""
import numpy as np
import pytest

import ldlt_ref as R

# every D the GPU tests run exact_system at (LDS, HBM and grid paths)
EXACT_D = [6, 7, 12, 16, 17, 18, 30, 48, 66, 96, 114, 126, 132, 144, 258, 259]


def test_longdouble_is_wider():
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("D", EXACT_D)
def test_exact_system_is_exact(D):
    for kw in ({}, {"signs": (-1,)}, {"d_values": (1,)}):
        A, b, x0 = R.exact_system(D, 0, **kw)
        assert np.array_equal(A, A.T) and np.array_equal(A, np.round(A))
        x, bad = R.ldlt_solve(A, b, np.float64)
        assert bad == -1 and x.tobytes() == x0.tobytes()
        xl, bad = R.ldlt_solve(A, b, np.longdouble)
        assert bad == -1 and np.array_equal(xl, x0)


def test_exact_system_pivots_are_d():
    """The factorisation's pivots are the d the system was built from: all negative when asked for."""
    A, b, x0 = R.exact_system(66, 0, signs=(-1,))
    assert (np.linalg.eigvalsh(A) < 0).all()
    A, _, _ = R.exact_system(66, 0)
    ev = np.linalg.eigvalsh(A)
    assert (ev < 0).any() and (ev > 0).any()


@pytest.mark.parametrize("D", [18, 114, 132, 258, 259])
def test_zero_at_is_reported_there(D):
    for k in (0, 5, 15, 16, D - 1):
        A, b, _ = R.exact_system(D, 0, zero_at=k)
        for dt in (np.float64, np.longdouble):
            x, bad = R.ldlt_solve(A, b, dt)
            assert bad == k and not x.any()


def test_non_finite_pivot_fails():
    for v in (np.inf, np.nan):
        A, b, _ = R.exact_system(18, 0)
        A[16, 16] = v
        assert R.ldlt_solve(A, b)[1] == 16


@pytest.mark.parametrize("D", [17, 114, 259])
def test_float64_matches_numpy_at_residual_level(D):
    from test_ldlt_grid_gpu import residual
    A, b = R.spd(D, 0)
    x, bad = R.ldlt_solve(A, b, np.float64)
    assert bad == -1
    r, rn = residual(A, x, b), residual(A, np.linalg.solve(A, b), b)
    assert r <= 16 * rn
    assert np.linalg.norm(x - np.linalg.solve(A, b)) <= 1e-12 * np.linalg.norm(x)


def test_longdouble_differs_on_ill_conditioned():
    """At cond 1e10 the float64 run loses ~10 of its 16 digits, the longdouble run ~10 of its 19: they differ by far
    more than the longdouble run's own error, which is what makes it a reference."""
    A, b = R.ill_spd(114, 1e10, 0)
    x64, _ = R.ldlt_solve(A, b, np.float64)
    xld, _ = R.ldlt_solve(A, b, np.longdouble)
    e = R.forward_error(x64, xld)
    assert 1e-12 < e < 1e-4
    # the longdouble solution's residual, evaluated in longdouble, is below anything float64 can reach
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    rl = np.linalg.norm(Al @ xld - bl) / np.linalg.norm(bl)
    r64 = np.linalg.norm(Al @ x64.astype(np.longdouble) - bl) / np.linalg.norm(bl)
    assert rl < r64 / 64


@pytest.mark.parametrize("D", [66, 114, 259])
def test_quasi_definite_is_stable_unpivoted(D):
    A, b = R.quasi_definite(D, 0)
    ev = np.linalg.eigvalsh(A)
    assert (ev < 0).sum() == D - D // 2 and (ev > 0).sum() == D // 2
    x64, bad = R.ldlt_solve(A, b, np.float64)
    xld, _ = R.ldlt_solve(A, b, np.longdouble)
    assert bad == -1 and R.forward_error(x64, xld) < 1e-12


def test_debug_entries_refuse_before_any_device_call():
    """orbba_debug_ldlt_lds / _hbm return ORB_EINVAL for sizes their kernels are not written for, and the LDS entry for
    a lambda that cannot be taken off A's diagonal exactly (it would solve another system than A)."""
    from orb_slam2_refactored_amd._lib import lib, ptr
    EINVAL = -1
    A, b, _ = R.exact_system(6, 0)
    x, ok = np.zeros(6), np.zeros(1, np.int32)
    f = lib().orbba_debug_ldlt_lds
    assert f(ptr(A), ptr(b), 5, 0.0, 1024, 1, ptr(x), ptr(ok), 0) == EINVAL     # odd D
    assert f(ptr(A), ptr(b), 0, 0.0, 1024, 1, ptr(x), ptr(ok), 0) == EINVAL
    assert f(ptr(A), ptr(b), 130, 0.0, 1024, 1, ptr(x), ptr(ok), 0) == EINVAL   # beyond the LDS range
    assert f(ptr(A), ptr(b), 6, 0.0, 512, 1, ptr(x), ptr(ok), 0) == EINVAL      # no such kernel
    assert f(ptr(A), ptr(b), 6, 0.0, 1024, 2, ptr(x), ptr(ok), 0) == EINVAL
    assert f(None, ptr(b), 6, 0.0, 1024, 1, ptr(x), ptr(ok), 0) == EINVAL
    assert A[0, 0] != 0
    assert f(ptr(A), ptr(b), 6, 1e300, 1024, 1, ptr(x), ptr(ok), 0) == EINVAL   # (A[0, 0] - 1e300) + 1e300 == 0
    g = lib().orbba_debug_ldlt_hbm
    assert g(ptr(A), ptr(b), 0, ptr(x), ptr(ok), 0) == EINVAL
    assert g(ptr(A), ptr(b), 7 * 511 + 1, ptr(x), ptr(ok), 0) == EINVAL
    assert g(ptr(A), None, 6, ptr(x), ptr(ok), 0) == EINVAL
