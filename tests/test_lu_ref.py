"""CPU: lu_ref (the NumPy restatement of the device LU) against LAPACK, and the properties of the
seeded instances that tests/test_gpu_lu.py relies on:
  * every pivot decision of a pivot-equality instance is decisive (second / first <= 1 - 1e-9);
  * every tie instance is exact (integer / dyadic factors, P A == L U exactly), ties where claimed;
  * LAPACK's own factors and solutions stay within the componentwise bounds the GPU tests apply;
  * np.linalg.solve returns non-finite values on the non-finite inputs.
"""
import warnings

import numpy as np
import pytest
import scipy.linalg

import lu_ref as R

SWEEP = list(R.sweep_instances())


@pytest.mark.parametrize("name,A", SWEEP, ids=[s[0] for s in SWEEP])
def test_sweep_instance_decisive_and_matches_lapack(name, A):
    n = A.shape[0]
    LU, piv, ratio, ties = R.getrf(A)
    assert np.all(piv >= 0) and not ties
    assert ratio.max() <= R.DECISIVE, (name, int(ratio.argmax()), ratio.max())
    lu, p = scipy.linalg.lu_factor(A)
    np.testing.assert_array_equal(piv, p)
    # the same pivots, so the same exact factors: both computed pairs lie within the componentwise
    # bound of P A (the GPU test's check), and entry by entry they agree to rounding wherever the
    # leading blocks are well enough conditioned to say so (not the cond 1e8 .. 1e15 family)
    rl = R.factor_ratio(A, lu, p)
    rf = R.factor_ratio(A, LU, piv) if n < 1000 else rl      # (long double products: seconds at n = 1100)
    if not name.startswith("illcond"):
        np.testing.assert_allclose(LU, lu, rtol=1e-6, atol=1e-9 * np.abs(lu).max())
    B = R.rhs(n, 2)
    X, x = R.getrs(LU, piv, B), scipy.linalg.lu_solve((lu, p), B)
    sf, sl = R.solve_ratio(A, LU, piv, X, B), R.solve_ratio(A, lu, p, x, B)
    print(f"[{name}] factor ratio ref {rf:.3g} lapack {rl:.3g}; solve ratio ref {sf:.3g} lapack {sl:.3g}; "
          f"least decisive {ratio.max():.6f}")
    assert max(rf, rl, sf, sl) <= 1.0


@pytest.mark.parametrize("k", R.ZERO_COLS)
def test_zero_column_instance(k):
    A = R.zero_column(k)
    LU, piv, ratio, ties = R.getrf(A)
    assert piv[k] == -1 - k and np.all(np.delete(piv, k) >= 0) and not ties
    assert np.all(LU[k + 1:, k] == 0.0)
    assert ratio.max() <= R.DECISIVE
    assert R.factor_ratio(A, LU, piv) <= 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lu, p = scipy.linalg.lu_factor(A)         # LAPACK: the same elimination, piv[k] = k
    np.testing.assert_array_equal(np.where(piv < 0, np.arange(len(piv)), piv), p)
    B = R.rhs(A.shape[0], 2)
    X = R.getrs(LU, piv, B)
    assert np.all(X[k] == 0.0) and R.solve_ratio(A, LU, piv, X, B) <= 1.0


TIES = list(R.tie_instances())


@pytest.mark.parametrize("name,A,k,rows,winner", TIES, ids=[t[0] for t in TIES])
def test_tie_instance_is_exact(name, A, k, rows, winner):
    assert A.shape == (R.TIE_N, R.TIE_N) and np.all(A == np.round(A))
    LU, piv, ratio, ties = R.getrf(A)
    assert list(ties) == [k] and list(ties[k]) == rows and piv[k] == winner
    assert np.all(piv >= 0)
    others = np.delete(ratio, k)
    assert others.max() <= 0.5                       # every other decision: |l| <= 1/2
    L, U = R.split(LU)
    assert R.is_dyadic(LU) and np.array_equal(R.permute_rows(A, piv), L @ U)   # (L @ U is exact too)
    if k == 0:
        assert len(set(np.abs(A[rows, 0]))) == 1 and A[winner, 0] != 0.0
    lu, p = scipy.linalg.lu_factor(A)
    np.testing.assert_array_equal(piv, p)
    np.testing.assert_array_equal(LU, lu)


def test_ties_include_opposite_signs():
    signs = {name: np.sign(A[rows, 0]) for name, A, k, rows, _ in TIES if k == 0}
    assert signs["trip"][0] == -signs["trip"][1] and signs["s512"][0] == -signs["s512"][1]
    assert signs["reduce"][0] == signs["reduce"][1]
    assert set(signs["diag0"][1:] * signs["diag0"][0]) == {-1.0, 1.0}


DUPS = list(R.dup_instances())


@pytest.mark.parametrize("name,A,c", DUPS, ids=[d[0] for d in DUPS])
def test_equal_columns_instance_is_exact(name, A, c):
    LU, piv, ratio, ties = R.getrf(A)
    assert piv[c] == -1 - c and np.all(np.delete(piv, c) >= 0) and not ties
    L, U = R.split(LU)
    assert R.is_dyadic(LU) and np.array_equal(R.permute_rows(A, piv), L @ U)
    assert np.all(LU[c + 1:, c] == 0.0) and LU[c, c] == 0.0
    B = np.round(R.rhs(A.shape[0], 2) * 8)
    X = R.getrs(LU, piv, B)
    assert np.all(X[c] == 0.0) and np.all(np.isfinite(X))


NONFINITE = list(R.nonfinite_instances())


@pytest.mark.parametrize("name,A", NONFINITE, ids=[s[0] for s in NONFINITE])
def test_numpy_solve_is_nonfinite_on_nonfinite_input(name, A):
    b = R.rhs(A.shape[0], 1)
    try:
        x = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        return                                       # (raising is the visible failure as well)
    assert not np.all(np.isfinite(x))
    LU, piv, _, _ = R.getrf(A)
    assert not np.all(np.isfinite(R.getrs(LU, piv, b)))


def test_skip_rule_on_tiny_cases():
    LU, piv, _, _ = R.getrf(np.zeros((3, 3)))
    np.testing.assert_array_equal(piv, [-1, -2, -3])
    np.testing.assert_array_equal(R.getrs(LU, piv, np.ones(3)), np.zeros(3))
    A = np.array([[0.0, 2.0], [0.0, 1.0]])
    LU, piv, _, _ = R.getrf(A)
    np.testing.assert_array_equal(piv, [-1, 1])
    np.testing.assert_array_equal(R.getrs(LU, piv, np.array([4.0, 1.0])), [0.0, 1.0])   # (row 0's equation is dropped)
