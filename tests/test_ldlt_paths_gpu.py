"""The LDS and the single-workgroup HBM LDL^T solves alone (orbba_debug_ldlt_lds: ba_solve_kernel<1024> / <256> of
csrc/orbba_solve.h; orbba_debug_ldlt_hbm: ba_solve_global_kernel -> ldlt_hbm_solve of csrc/ldlt_blocked.h), against
tests/ldlt_ref.py (pinned by tests/test_ldlt_ref.py):

  exact      exact_system: ok == 1 and x == x0 bit for bit, no tolerance (ldlt_ref's docstring has the argument);
  ok rule    a zero pivot at 0, 5, 15, 16 or D - 1 and +inf / nan on the diagonal at 0 or 16 give ok == 0 and x all
             zero; a system whose pivots are all negative gives ok == 1 and the exact x0;
  residual   spd and ill_spd (cond 1e6, 1e10): |Ax - b| / (|A| |x| + |b|) <= 16 x numpy.linalg.solve's own value
             (test_ldlt_grid_gpu.py's helper and factor);
  forward    quasi_definite (negative pivots): |x - x_ld| / |x_ld| <= 16 x the same quantity of the float64
             restatement ldlt_solve, x_ld the longdouble solution.

Sizes.  LDS: 6 (one block, 10 padding rows), 12, 18 (second block nearly all padding), 30, 48 and 96 (no padding),
66, 114 (the benchmark's), 126 (the largest), each with 1024 threads and simd0_helpers 1 and 0 and with 256 threads.
HBM: 6, 7 (one Sim3 vertex), 16, 17, 132 (LocalBA's smallest), 144 (no padding), 259 = 7 x 37, and for the residual
1050 and 3577 = 7 x 511, the limit.  Every solve runs twice and the two x must be byte-identical.  Each ratio is printed
as `path D kind: device r, reference r, ratio`."""
import functools

import numpy as np
import pytest

import ldlt_ref as R
from orb_slam2_refactored_amd._lib import check, lib, ptr
from test_ldlt_grid_gpu import residual

pytestmark = pytest.mark.gpu

LDS_D = [6, 12, 18, 30, 48, 66, 96, 114, 126]
LDS_CFG = [(1024, 1), (1024, 0), (256, 1)]   # (threads, simd0_helpers)
HBM_D = [6, 7, 16, 17, 132, 144, 259]


def _twice(call, D):
    out = []
    for _ in range(2):
        x, ok = np.full(D, 7.0), np.full(1, -5, np.int32)
        call(x, ok)
        out.append((x, int(ok[0])))
    (x, ok), (x2, ok2) = out
    assert ok == ok2 and x.tobytes() == x2.tobytes(), "two runs differ"
    return x, ok


def lds_solve(A, b, cfg=(1024, 1), lam=0.0):
    D = len(b)
    A, b = np.ascontiguousarray(A, np.float64), np.ascontiguousarray(b, np.float64)
    return _twice(lambda x, ok: check(lib().orbba_debug_ldlt_lds(ptr(A), ptr(b), D, float(lam), cfg[0], cfg[1], ptr(x),
                                                                 ptr(ok), 0), "orbba_debug_ldlt_lds"), D)


def hbm_solve(A, b):
    D = len(b)
    A, b = np.ascontiguousarray(A, np.float64), np.ascontiguousarray(b, np.float64)
    return _twice(lambda x, ok: check(lib().orbba_debug_ldlt_hbm(ptr(A), ptr(b), D, ptr(x), ptr(ok), 0),
                                      "orbba_debug_ldlt_hbm"), D)


# the systems and their host-side references, built once
exact = functools.lru_cache(None)(R.exact_system)


@functools.lru_cache(None)
def general(kind, D):
    """(A, b, numpy.linalg.solve's residual, |A|_2)"""
    A, b = R.spd(D, 0) if kind == "spd" else R.ill_spd(D, float(kind[4:]), 0)
    # |A|_2 of a symmetric matrix is its largest |eigenvalue|; at the largest size that is several times cheaper than
    # the singular values numpy.linalg.norm(A, 2) computes, and equal to rounding
    nA = np.abs(np.linalg.eigvalsh(A)).max() if D > 2000 else np.linalg.norm(A, 2)
    return A, b, residual(A, np.linalg.solve(A, b), b, nA), nA


def check_residual(path, kind, D, solve):
    A, b, rn, nA = general(kind, D)
    x, ok = solve(A, b)
    rg = residual(A, x, b, nA)
    print(f"{path} {D} {kind}: device {rg:.3g}, reference {rn:.3g}, ratio {rg / rn:.3g}")
    assert ok == 1
    assert rg <= 16 * rn


def check_forward(path, D, solve):
    A, b, xld, e64 = R.quasi_definite_reference(D)
    x, ok = solve(A, b)
    eg = R.forward_error(x, xld)
    print(f"{path} {D} quasi_definite: device {eg:.3g}, reference {e64:.3g}, ratio {eg / e64:.3g}")
    assert ok == 1
    assert eg <= 16 * e64


def failing_systems(D):
    """(label, A, b): a zero pivot at each index of {0, 5, 15, 16, D - 1} that exists, +inf and nan at (k, k)"""
    for k in sorted({k for k in (0, 5, 15, 16, D - 1) if k < D}):
        A, b, _ = exact(D, 0, zero_at=k)
        yield f"zero_at {k}", A, b
    A0, b, _ = exact(D, 0)
    for k in (0, 16):
        for v in (np.inf, np.nan):
            A = A0.copy()
            A[k, k] = v
            yield f"{v} at {k}", A, b


# ---------------------------------------------------------------- LDS path
@pytest.mark.parametrize("cfg", LDS_CFG, ids=lambda c: f"t{c[0]}h{c[1]}")
@pytest.mark.parametrize("lam", [0.0, 3.0])
@pytest.mark.parametrize("D", LDS_D)
def test_lds_exact(D, lam, cfg):
    A, b, x0 = exact(D, 0)
    x, ok = lds_solve(A, b, cfg, lam)
    assert ok == 1
    assert x.tobytes() == x0.tobytes(), np.flatnonzero(x != x0)


@pytest.mark.parametrize("cfg", LDS_CFG, ids=lambda c: f"t{c[0]}h{c[1]}")
@pytest.mark.parametrize("D", [18, 114])
def test_lds_ok_rule(D, cfg):
    for label, A, b in failing_systems(D):
        x, ok = lds_solve(A, b, cfg)
        assert ok == 0 and not x.any(), label
    A, b, x0 = exact(D, 0, signs=(-1,))
    x, ok = lds_solve(A, b, cfg)
    assert ok == 1 and x.tobytes() == x0.tobytes()


@pytest.mark.parametrize("cfg", LDS_CFG, ids=lambda c: f"t{c[0]}h{c[1]}")
@pytest.mark.parametrize("kind", ["spd", "ill_1e6", "ill_1e10"])
@pytest.mark.parametrize("D", [114, 126])
def test_lds_residual(D, kind, cfg):
    check_residual(f"lds[{cfg[0]},{cfg[1]}]", kind, D, lambda A, b: lds_solve(A, b, cfg))


@pytest.mark.parametrize("cfg", LDS_CFG, ids=lambda c: f"t{c[0]}h{c[1]}")
@pytest.mark.parametrize("D", [66, 114])
def test_lds_forward_error_negative_pivots(D, cfg):
    check_forward(f"lds[{cfg[0]},{cfg[1]}]", D, lambda A, b: lds_solve(A, b, cfg))


# ---------------------------------------------------------------- HBM path
@pytest.mark.parametrize("D", HBM_D)
def test_hbm_exact(D):
    A, b, x0 = exact(D, 0)
    x, ok = hbm_solve(A, b)
    assert ok == 1
    assert x.tobytes() == x0.tobytes(), np.flatnonzero(x != x0)


@pytest.mark.parametrize("D", [132, 259])
def test_hbm_ok_rule(D):
    for label, A, b in failing_systems(D):
        x, ok = hbm_solve(A, b)
        assert ok == 0 and not x.any(), label
    A, b, x0 = exact(D, 0, signs=(-1,))
    x, ok = hbm_solve(A, b)
    assert ok == 1 and x.tobytes() == x0.tobytes()


@pytest.mark.parametrize("kind", ["spd", "ill_1e6", "ill_1e10"])
@pytest.mark.parametrize("D", [132, 259, 1050])
def test_hbm_residual(D, kind):
    check_residual("hbm", kind, D, hbm_solve)


def test_hbm_residual_at_the_limit():
    check_residual("hbm", "spd", 7 * 511, hbm_solve)


@pytest.mark.parametrize("D", [132, 259])
def test_hbm_forward_error_negative_pivots(D):
    check_forward("hbm", D, hbm_solve)
