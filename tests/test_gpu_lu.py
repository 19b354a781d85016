"""-m gpu: the LU fallback solver (ipm_getrf / ipm_getrs: k_lu_pivot, k_lu_update, k_laswp,
k_lu_trsm, the MFMA trailing GEMM, k_lu_solve) at its panel edges, with padded leading dimensions,
on the matrices the engine factors, on pivot ties, zero pivot columns and non-finite input.

Bounds (derived in tests/lu_ref.py from Higham, Accuracy and Stability of Numerical Algorithms,
theorems 9.3 and 9.4; they hold for the device's OWN factors in any order of summation and do not
depend on the conditioning):
    |P A - L U|_ij <= (min(i, j) + 2) eps (|L| |U|)_ij          entry by entry, long double product
    |P b - P A x|_i <= 3 (n + 1) eps (|L| |U| |x|)_i
A non-finite device value anywhere gives a ratio of inf.  Where pivots are decisive
(tests/test_lu_ref.py proves second / first <= 1 - 1e-9 at every step of every such instance, and
that lu_ref's pivots are LAPACK's) the pivot vector must equal LAPACK's exactly.

Layout: A column-major with leading dimension lda -- element (i, j) at A[j * lda + i], so a device
tensor of shape (n, lda) holds column j in its row j; B row-major n x nrhs (ldb).  A's padding is
NaN (a load outside the operand shows in the factors) and must still be NaN afterwards; B's and
piv's padding hold a sentinel that must come back untouched.  Each test prints its worst ratio.
"""
import numpy as np
import pytest
import scipy.linalg

import lu_ref as R
from gpu_util import dev, devnan, getrf, getrs, host

pytestmark = pytest.mark.gpu
IPM_OK, IPM_INVALID_ARG = 0, 2
SENTINEL = 12345.0
PIV_SENTINEL = -777
RHS_LAYOUTS = [(1, 1), (1, 4), (2, 2), (2, 5), (70, 70), (70, 73)]   # (nrhs, ldb): ldb = nrhs, nrhs + 3


def _dev_a(A, lda):
    n = A.shape[0]
    t = devnan((n, lda))
    t[:, :n] = dev(A.T)
    return t


def _dev_b(B, ldb):
    import torch
    t = torch.full((B.shape[0], ldb), SENTINEL, dtype=torch.float64, device="cuda")
    t[:, :B.shape[1]] = dev(B)
    return t


def _dev_piv(n):
    import torch
    return torch.full((n + 2,), PIV_SENTINEL, dtype=torch.int64, device="cuda")


def _factor(A, lda):
    """-> (LU as an ordinary (row, column) array, piv, the device tensors)"""
    n = A.shape[0]
    Ad, pd = _dev_a(A, lda), _dev_piv(n)
    rc, info = getrf(Ad, n, lda, pd)
    assert rc == IPM_OK and info == 0
    mem, piv = host(Ad), pd.cpu().numpy()
    assert np.all(np.isnan(mem[:, n:])), "padding rows of A written"
    assert np.all(piv[n:] == PIV_SENTINEL), "piv written past n"
    return mem[:, :n].T.copy(), piv[:n].copy(), Ad, pd


def _solve(Ad, pd, n, lda, B, ldb):
    Bd = _dev_b(B, ldb)
    assert getrs(Ad, n, lda, pd, Bd, B.shape[1], ldb) == IPM_OK
    mem = host(Bd)
    assert np.all(mem[:, B.shape[1]:] == SENTINEL), "padding columns of B written"
    return mem[:, :B.shape[1]].copy()


def _sweep(name, A, pivots):
    n = A.shape[0]
    worst_f = worst_s = 0.0
    seen, seen_x = None, {}
    for lda in (n, n + 1, n + 7):
        LU, piv, Ad, pd = _factor(A, lda)
        np.testing.assert_array_equal(piv, pivots)
        if seen is None or not np.array_equal(seen, LU):     # (the same bits: the same ratio)
            rf = R.factor_ratio(A, LU, piv)
            assert rf <= 1.0, (name, lda, rf)
            worst_f, seen = max(worst_f, rf), LU
        for nrhs, ldb in RHS_LAYOUTS:
            B = R.rhs(n, nrhs)
            X = _solve(Ad, pd, n, lda, B, ldb)
            if nrhs in seen_x and np.array_equal(seen_x[nrhs], X) and np.array_equal(seen, LU):
                continue
            rs = R.solve_ratio(A, LU, piv, X, B)
            assert rs <= 1.0, (name, lda, nrhs, ldb, rs)
            worst_s, seen_x[nrhs] = max(worst_s, rs), X
    print(f"[lu {name}] worst factor err / bound {worst_f:.3g}, solve residual / bound {worst_s:.3g}")


@pytest.mark.parametrize("cls,n", [(c, n) for n in R.SWEEP_N for c in R.CLASSES if not (c == "kkt" and n < 4)])
def test_lu_sweep(cls, n):
    """n = 1, 2, 63: one partial panel; 64: one full panel; 65: one column into the second; 127,
    128, 129: two panels and one column more; 257: the last panel a single column, k_lu_trsm with
    m = 193, 129, 65, 1; 1100: the 1024-thread pivot search takes a second stride trip, k_lu_update
    has 5 row blocks, k_laswp and k_lu_trsm more than 4 workgroups.  Classes: normal entries; the
    symmetric indefinite KKT matrix [[H, A^T], [A, 0]] (H SPD, diagonal spread 1e-6 .. 1e6, zero
    block n // 4); the Schur complement S = A H^-1 A^T.  lda = n, n + 1, n + 7; nrhs = 1, 2, 70
    (more than one 64-column tile of right-hand sides, the block elimination's nrhs = p) with
    ldb = nrhs and nrhs + 3.  (No KKT class at n = 1, 2: there is no zero block below n = 4.)"""
    A = R.matrix(cls, n)
    _sweep(f"{cls}-{n}", A, scipy.linalg.lu_factor(A)[1])


@pytest.mark.parametrize("cond", R.ILLCOND)
def test_lu_ill_conditioned_symmetric(cond):
    """Q diag(logspace(0, -log10 cond)) Q^T at n = 80, cond 1e8 .. 1e15: the same componentwise
    bounds (they do not depend on the conditioning)."""
    A = R.illcond(80, cond)
    _sweep(f"illcond-{cond:.0e}", A, scipy.linalg.lu_factor(A)[1])


TIE_NAMES = ["trip", "reduce", "s512", "diag0"]


@pytest.mark.parametrize("name", TIE_NAMES)
def test_lu_pivot_ties(name):
    """Equal-magnitude pivot candidates in column 0 of an exact integer matrix, n = 1600 (thread of
    row i in the search of step 0: i % 1024):
      trip    rows 100 and 1124 (opposite signs): one thread, first and second stride trip -- the
              strict > keeps 100
      reduce  rows 700 and 1500: threads 700 and 476 -- the reduction's tie-break returns 700
              although the lower thread holds 1500
      s512    rows 3 and 515 (opposite signs): the partners of the s = 512 reduction step
      diag0   rows 0, 512 and 1024 (both signs): a tie with the diagonal -- no swap, piv[0] = 0
    Elimination is exact in fp64 (tests/test_lu_ref.py), so pivots and both factors equal LAPACK's
    bit for bit."""
    _, A, k, rows, winner = next(t for t in R.tie_instances() if t[0] == name)
    n = A.shape[0]
    lu, p = scipy.linalg.lu_factor(A)
    LU, piv, Ad, pd = _factor(A, n + 1)
    assert piv[k] == winner == p[k]
    np.testing.assert_array_equal(piv, p)
    np.testing.assert_array_equal(LU, lu)
    B = R.rhs(n, 1)
    rs = R.solve_ratio(A, LU, piv, _solve(Ad, pd, n, n + 1, B, 1), B)
    print(f"[lu tie {name}] pivots and factors bitwise LAPACK's; solve residual / bound {rs:.3g}")
    assert rs <= 1.0


def _check_skipped(name, A, k, exact):
    n = A.shape[0]
    LUr, pivr, _, _ = R.getrf(A)
    assert pivr[k] == -1 - k
    worst = 0.0
    for lda in (n, n + 7):
        LU, piv, Ad, pd = _factor(A, lda)
        assert piv[k] == -1 - k
        np.testing.assert_array_equal(piv, pivr)
        assert np.all(LU[k + 1:, k] == 0.0) and not np.any(np.signbit(LU[k + 1:, k]))
        if exact:
            np.testing.assert_array_equal(LU, LUr)
        else:
            rf = R.factor_ratio(A, LU, piv)
            assert rf <= 1.0, (name, lda, rf)
            worst = max(worst, rf)
        for nrhs, ldb in [(1, 1), (2, 5)]:
            B = np.round(R.rhs(n, nrhs) * 8) if exact else R.rhs(n, nrhs)
            X = _solve(Ad, pd, n, lda, B, ldb)
            assert np.all(X[k] == 0.0)
            rs = R.solve_ratio(A, LU, piv, X, B)       # (every row of P A x = P b but the skipped one)
            assert rs <= 1.0, (name, lda, nrhs, rs)
            worst = max(worst, rs)
            Xr = R.getrs(LUr, pivr, B)
            assert np.all(np.isfinite(X)) and np.all(Xr[k] == 0.0)
    print(f"[lu skipped {name}] worst ratio {worst:.3g}")


@pytest.mark.parametrize("k", R.ZERO_COLS)
def test_lu_zero_column(k):
    """An exactly zero column at k = 0 (first), 63 (last of a panel), 64 (first of the next), 65
    (inside the second panel), 129 (last column) of an n = 130 normal matrix: piv[k] = -1 - k, the
    L column exactly 0, info 0 and IPM_OK as documented; every other pivot is lu_ref's, the factors
    lie within the componentwise bound; ipm_getrs returns exactly 0 in component k and satisfies
    every other equation of P A x = P b within the solve bound."""
    _check_skipped(f"zero-{k}", R.zero_column(k), k, exact=False)


@pytest.mark.parametrize("name", ["dup64", "dup70"])
def test_lu_column_zero_after_elimination(name):
    """An exact integer matrix with two equal columns: column 64 (the first of the second panel: it
    becomes zero through the MFMA trailing update) / column 70 (through k_lu_update inside the
    panel) is exactly zero when elimination reaches it.  Factors and pivots bitwise lu_ref's."""
    _, A, c = next(d for d in R.dup_instances() if d[0] == name)
    _check_skipped(name, A, c, exact=True)


NONFINITE = [s[0] for s in R.nonfinite_instances()]


@pytest.mark.parametrize("name", NONFINITE)
def test_lu_nonfinite_input_gives_nonfinite_solution(name):
    """A NaN below the diagonal of column 0, a NaN above the diagonal, an all-NaN column (0, 64 and
    the last, n = 70) and an all-NaN matrix (n = 5, 70): the vector ipm_getrs returns must contain
    a non-finite value, as np.linalg.solve's does (tests/test_lu_ref.py).  A NaN pivot candidate is
    never an exactly-zero column (piv >= 0 where the candidates are NaN)."""
    A = dict(R.nonfinite_instances())[name]
    n = A.shape[0]
    for lda in (n, n + 7):
        Ad, pd = _dev_a(A, lda), _dev_piv(n)
        rc, info = getrf(Ad, n, lda, pd)
        assert rc == IPM_OK and info == 0
        piv = pd.cpu().numpy()[:n]
        b = R.rhs(n, 1)
        x = _solve(Ad, pd, n, lda, b, 1)
        print(f"[lu {name} lda={lda}] finite components {int(np.isfinite(x).sum())} of {n}, "
              f"skipped columns {int((piv < 0).sum())}")
        assert not np.all(np.isfinite(x)), (name, lda)
        if name.startswith("nan-column") or name.startswith("nan-matrix"):
            assert np.all(piv >= 0), piv


def test_lu_invalid_arguments_and_empty_sizes():
    """lda < n, ldb < nrhs, negative n / nrhs and a null piv: IPM_INVALID_ARG, the sentinel outputs
    untouched; n = 0 and nrhs = 0: IPM_OK, nothing touched."""
    import torch
    n = 4
    A = torch.full((n, n), SENTINEL, dtype=torch.float64, device="cuda")
    B = torch.full((n, 3), SENTINEL, dtype=torch.float64, device="cuda")
    piv = _dev_piv(n)
    assert getrf(A, n, n - 1, piv)[0] == IPM_INVALID_ARG
    assert getrf(A, -1, n, piv)[0] == IPM_INVALID_ARG
    assert getrf(A, n, n, None)[0] == IPM_INVALID_ARG
    assert getrs(A, n, n - 1, piv, B, 3, 3) == IPM_INVALID_ARG
    assert getrs(A, n, n, piv, B, 3, 2) == IPM_INVALID_ARG
    assert getrs(A, -1, n, piv, B, 3, 3) == IPM_INVALID_ARG
    assert getrs(A, n, n, piv, B, -1, 3) == IPM_INVALID_ARG
    assert getrs(A, n, n, None, B, 3, 3) == IPM_INVALID_ARG
    assert getrf(A, 0, n, piv) == (IPM_OK, -7)            # (n = 0 returns before *info is written)
    assert getrs(A, 0, n, piv, B, 3, 3) == IPM_OK
    assert getrs(A, n, n, piv, B, 0, 3) == IPM_OK
    assert np.all(host(A) == SENTINEL) and np.all(host(B) == SENTINEL)
    assert np.all(piv.cpu().numpy() == PIV_SENTINEL)
