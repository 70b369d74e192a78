"""Plain references and input generators for the library's three blocked LDL^T solvers (csrc/orbba_solve.h's LDS
kernel, csrc/ldlt_blocked.h's single-workgroup HBM form, csrc/ldlt_grid.h).  numpy only.

ldlt_solve is the unpivoted, unblocked factorisation with both substitutions, in float64 (the restatement of what the
device computes) or in longdouble (64-bit mantissa on x86-64: the high-precision reference).  It applies the device's
rule: a zero or non-finite pivot fails, a negative one does not (Eigen SimplicialLDLT's behaviour).

exact_system builds systems on which every one of the three algorithms is exact in fp64 whatever its blocking and
summation order, so a device answer must equal x0 bit for bit:
  A = L diag(d) L^T with L unit lower triangular and exactly one off-diagonal entry per row, +-1, at a random earlier
  column.  L - I is then the edge list of a tree, so L^-1 (and the inverse of every diagonal block of L) has entries
  in {-1, 0, 1}: entry (i, j) is the signed product along the one path from i up to j.  d is drawn from
  {+-1, +-2, +-4} and x0 from the nonzero integers in [-8, 8]; b = A x0.  U = L_IJ D_J, the Schur complements
  (= L2 D2 L2^T of the remaining rows), Linv, D^-1, z, D^-1 z, vz = Linv^T D^-1 z and every partial sum of the MFMA
  tiles are multiples of 1/4 of modest size: exactly representable, so no sum rounds.  The one step that leans on
  the hardware is 1 / d: v_rcp_f64 of a power of two followed by two Newton steps is exact."""
import functools

import numpy as np


def ldlt_solve(A, b, dtype=np.float64):
    """(x, bad): x solves A x = b by unpivoted LDL^T in `dtype`; bad is the index of the first zero or non-finite
    pivot (x is then all zero), or -1."""
    A = np.array(A, dtype=dtype)
    n = len(b)
    y = np.array(b, dtype=dtype)
    d = np.zeros(n, dtype=dtype)
    for j in range(n):   # right-looking: column j is final, the trailing block loses its outer product
        dj = A[j, j]
        if dj == 0 or not np.isfinite(dj):
            return np.zeros(n, dtype=dtype), j
        d[j] = dj
        u = A[j + 1:, j].copy()   # U = L D
        l = u / dj
        A[j + 1:, j] = l
        A[j + 1:, j + 1:] -= np.outer(l, u)
        y[j + 1:] -= l * y[j]     # forward substitution carried along
    y /= d
    for j in range(n - 1, 0, -1):   # L^T x = t
        y[:j] -= A[j, :j] * y[j]
    return y, -1


def exact_system(D, seed, zero_at=None, d_values=(1, 2, 4), signs=(-1, 1)):
    """(A, b, x0) as the module docstring describes.  zero_at = k: d[k] = 0, so pivot k is exactly zero and no
    earlier one is.  d_values / signs: the magnitudes and signs d is drawn from (signs = (-1,): every pivot
    negative)."""
    rng = np.random.default_rng([D, seed])
    L = np.eye(D)
    for i in range(1, D):
        L[i, rng.integers(0, i)] = rng.choice([-1.0, 1.0])
    d = rng.choice(np.asarray(d_values, float), size=D) * rng.choice(np.asarray(signs, float), size=D)
    if zero_at is not None:
        d[zero_at] = 0.0
    A = (L * d) @ L.T   # integers below 2^53: exact
    # (no zeros in x0: an exact zero comes out as +0 or -0 depending on the order of the sums that cancel)
    x0 = (rng.integers(1, 9, size=D) * rng.choice([-1, 1], size=D)).astype(float)
    return A, A @ x0, x0


def spd(D, seed):
    """(A, b): B^T B + I, symmetrised, as tests/test_ldlt_grid_gpu.py builds it."""
    rng = np.random.default_rng([D, seed])
    B = rng.normal(size=(D, D))
    A = B.T @ B + np.eye(D)
    return 0.5 * (A + A.T), rng.normal(size=D)


def ill_spd(D, cond, seed):
    """(A, b): Q diag(logspace(0, -log10 cond)) Q^T, symmetrised: SPD with condition number cond."""
    rng = np.random.default_rng([D, seed, 1])
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    A = (Q * np.logspace(0, -np.log10(cond), D)) @ Q.T
    return 0.5 * (A + A.T), rng.normal(size=D)


def quasi_definite(D, seed):
    """(A, b): [[H, C], [C^T, -G]] with H, G of the spd kind: the trailing pivots are negative, and the unpivoted
    LDL^T is still stable on it (Vanderbei's symmetric quasi-definite matrices)."""
    n1 = D // 2
    rng = np.random.default_rng([D, seed, 2])
    H, _ = spd(n1, seed)
    G, _ = spd(D - n1, seed + 1)
    Cm = rng.normal(size=(n1, D - n1))
    A = np.block([[H, Cm], [Cm.T, -G]])
    return A, rng.normal(size=D)


@functools.lru_cache(None)
def quasi_definite_reference(D):
    """(A, b, x_ld, e64) of quasi_definite(D, 0), computed once for every test that needs it: the longdouble solution
    and the forward error of the float64 restatement against it."""
    A, b = quasi_definite(D, 0)
    x64, bad = ldlt_solve(A, b, np.float64)
    xld, bad_ld = ldlt_solve(A, b, np.longdouble)
    assert bad == -1 and bad_ld == -1
    for a in (A, b, xld):
        a.setflags(write=False)
    return A, b, xld, forward_error(x64, xld)


def forward_error(x, x_ref):
    """|x - x_ref| / |x_ref| in longdouble (x_ref the longdouble solution)."""
    x_ref = np.asarray(x_ref, np.longdouble)
    return float(np.linalg.norm(np.asarray(x, np.longdouble) - x_ref) / np.linalg.norm(x_ref))
