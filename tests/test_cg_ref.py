"""CPU checks for linear_solve_method='cg': the NumPy restatement (tests/cg_ref.py) against
scipy.sparse.linalg.cg bit for bit, the six-iteration margin the GPU test's exact count rests on,
the workspace size of a CG problem, and the reference-run fixtures (tests/golden/cg_*.npz)."""
import ctypes
import os

import numpy as np
import pytest

import cg_ref
from conftest import GOLDEN

CG_FIXTURES = ("cg_qp_n40", "cg_qp_n130", "cg_lp_n40", "cg_socp_n24")


def _scipy_cg():
    return pytest.importorskip("scipy.sparse.linalg").cg


@pytest.mark.parametrize("n", [257, 300])
def test_restatement_equals_scipy_clustered(n):
    """converged solves (six eigenvalue clusters), zero and non-zero x0: x and info bit for bit"""
    cg = _scipy_cg()
    H, _ = cg_ref.clustered(n, seed=n)
    rng = np.random.default_rng(n + 1)
    b = rng.standard_normal(n)
    xc = rng.standard_normal(n)
    x0w = (xc @ b) * xc / (xc @ (H @ xc))          # the warm start's form: a scaled copy of a vector
    for x0 in (None, x0w):
        xs, infos = cg(H, b, x0=None if x0 is None else x0.copy(), maxiter=50)
        xr, infor, _ = cg_ref.cg(H, b, x0=x0, maxiter=50)
        assert infor == infos == 0
        assert np.array_equal(xr, xs)
    # the Newton step's own form: cg(-H, g, x0)
    xs, infos = cg(-H, b, x0=x0w.copy(), maxiter=50)
    xr, infor, _ = cg_ref.cg(-H, b, x0=x0w, maxiter=50)
    assert infor == infos and np.array_equal(xr, xs)


@pytest.mark.parametrize("maxiter", [8, 50])
def test_restatement_equals_scipy_truncated(maxiter):
    """lam = logspace(0, 6, n): the cap truncates the solve; info == maxiter, x bit for bit"""
    cg = _scipy_cg()
    n = 257
    H, _ = cg_ref.ill_conditioned(n, seed=5)
    b = np.random.default_rng(6).standard_normal(n)
    xs, infos = cg(H, b, maxiter=maxiter)
    xr, infor, iters = cg_ref.cg(H, b, maxiter=maxiter)
    assert infor == infos == maxiter and iters == maxiter
    assert np.array_equal(xr, xs)


def test_restatement_edge_cases_equal_scipy():
    """b == 0 -> x = 0 whatever x0; maxiter = 0 -> x0 back with info 0"""
    cg = _scipy_cg()
    H, _ = cg_ref.clustered(64, seed=1)
    x0 = np.random.default_rng(2).standard_normal(64)
    xs, infos = cg(H, np.zeros(64), x0=x0.copy(), maxiter=50)
    xr, infor, iters = cg_ref.cg(H, np.zeros(64), x0=x0, maxiter=50)
    assert infos == infor == 0 and iters == 0 and np.array_equal(xs, xr) and not xr.any()
    b = np.random.default_rng(3).standard_normal(64)
    xs, infos = cg(H, b, x0=x0.copy(), maxiter=0)
    xr, infor, iters = cg_ref.cg(H, b, x0=x0, maxiter=0)
    assert infos == infor == 0 and iters == 0 and np.array_equal(xs, xr) and np.array_equal(xr, x0)


@pytest.mark.parametrize("n", [257, 300])
def test_clustered_matrix_stops_after_exactly_six_iterations(n):
    """The margin behind the GPU test's `iters == 6`: ||r|| / ||b|| is >= 0.1 at the six tests
    before (rtol is 1e-5: four orders away) and <= 1e-9 at the one after the sixth iteration (four
    orders the other way), in float64, in longdouble and with the variables permuted (another
    summation order)."""
    H, _ = cg_ref.clustered(n, seed=n)
    b = np.random.default_rng(n + 1).standard_normal(n)
    perm = np.random.default_rng(n + 2).permutation(n)
    for name, (Hm, bm, dt) in {"f64": (H, b, np.float64), "longdouble": (H, b, np.longdouble),
                               "permuted": (H[np.ix_(perm, perm)], b[perm], np.float64)}.items():
        tr = []
        _, info, iters = cg_ref.cg(Hm, bm, maxiter=50, dtype=dt, trace=tr)
        print(f"[clustered n={n} {name}] ||r||/||b|| at the tests: {['%.2g' % v for v in tr]}")
        assert info == 0 and iters == 6 and len(tr) == 7
        assert min(tr[:6]) >= 0.1 and tr[6] <= 1e-9


def test_cg_problem_workspace_has_no_second_matrix():
    """QP n = 2048, m = 512 with IPM_SOLVE_CG: H, but no eigenvector matrix, Cholesky workspace or
    SYRK split tail -- less than two n x n matrices (the Cholesky problem of test_cabi needs two)."""
    from ipm355 import _lib
    lib = _lib.load_library()
    d = _lib.ProblemDesc()
    d.kind = _lib.KIND_QP
    d.n = 2048
    d.m = 512
    d.C = 1  # non-null marker; only sizes are read
    d.ldc = 2048
    d.solve_method = _lib.SOLVE_CG
    ws = lib.ipm_workspace_bytes(ctypes.byref(d))
    print(f"[cg workspace n=2048] {ws} bytes = {ws / (2048 * 2048 * 8):.3f} n^2 doubles")
    assert 2048 * 2048 * 8 <= ws < 2 * 2048 * 2048 * 8
    d.solve_method = _lib.SOLVE_CHOLESKY
    assert lib.ipm_workspace_bytes(ctypes.byref(d)) >= 2 * 2048 * 2048 * 8   # unchanged (test_cabi)


@pytest.mark.parametrize("name", CG_FIXTURES)
def test_cg_fixture_loads(name):
    """reference-run fixtures: a finite value_tol that holds the reference's own three values"""
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    tol, val = float(z["value_tol"]), float(z["value"])
    assert np.isfinite(tol) and tol >= 1e-9 * abs(val) and tol >= 10 * float(z["ref_spread"])
    assert np.all(np.abs(z["ref_values"] - val) <= tol)
    assert np.all(np.isfinite(z["xstar"])) and int(z["outer_iters"]) > 0 and int(z["max_cg_iters"]) > 0
    assert str(z["kind"]) in ("LP", "QP", "SOCP")
