"""CPU checks for cg_preconditioner='jacobi': the NumPy restatement (tests/pcg_ref.py) against
scipy.sparse.linalg.cg with its M argument bit for bit, its two reductions to known bits (M = I is
cg_ref.cg; (-H, -b, -M) is (H, b, M)), the scale invariance of the Jacobi-preconditioned iteration
count with the margin the GPU test's exact count rests on, and the reference-run fixtures
(tests/golden/pcg_*.npz)."""
import os

import numpy as np
import pytest

import cg_ref
import pcg_ref
from conftest import GOLDEN

PCG_FIXTURES = ("pcg_lp_n40_scaled", "pcg_lp_n200_scaled", "pcg_qp_n130")


def _scipy():
    return pytest.importorskip("scipy.sparse.linalg")


def _scipy_pcg(A, b, minv, x0=None, maxiter=50, rtol=1e-5):
    spla = _scipy()
    n = len(b)
    M = spla.LinearOperator((n, n), matvec=lambda r: minv * r, dtype=np.float64)
    return spla.cg(A, b, x0=None if x0 is None else x0.copy(), M=M, maxiter=maxiter, rtol=rtol)


def _system(n):
    K, lam = cg_ref.clustered(n, seed=n)
    b0 = np.random.default_rng(n + 1).standard_normal(n)
    return K, lam, b0


@pytest.mark.parametrize("n", [257, 300])
def test_restatement_equals_scipy(n):
    """(a) float64 pcg == scipy's cg(..., M=M) bit for bit: zero and non-zero x0 on the clustered
    matrix and on its badly scaled form, b = 0, a truncated run, the Newton step's own call
    (-H, g, -1 / h)"""
    _scipy()
    K, _, b0 = _system(n)
    H, b, _ = pcg_ref.scaled_system(K, b0, n + 3)
    xc = np.random.default_rng(n + 2).standard_normal(n)
    for A, rhs in ((K, b0), (H, b)):
        minv = pcg_ref.jacobi(A)
        x0w = (xc @ rhs) * xc / (xc @ (A @ xc))
        for x0 in (None, x0w):
            xs, infos = _scipy_pcg(A, rhs, minv, x0=x0, maxiter=200)
            xr, infor, _ = pcg_ref.pcg(A, rhs, minv, x0=x0, maxiter=200)
            assert infor == infos == 0
            assert np.array_equal(xr, xs)
        xs, infos = _scipy_pcg(A, np.zeros(n), minv, x0=x0w, maxiter=200)
        xr, infor, iters = pcg_ref.pcg(A, np.zeros(n), minv, x0=x0w, maxiter=200)
        assert infos == infor == 0 and iters == 0 and np.array_equal(xs, xr) and not xr.any()
        xs, infos = _scipy_pcg(A, rhs, minv, maxiter=8)
        xr, infor, iters = pcg_ref.pcg(A, rhs, minv, maxiter=8)
        assert infos == infor == 8 and iters == 8 and np.array_equal(xs, xr)
        xs, infos = _scipy_pcg(-A, rhs, -minv, x0=x0w, maxiter=200)
        xr, infor, _ = pcg_ref.pcg(-A, rhs, -minv, x0=x0w, maxiter=200)
        assert infor == infos == 0 and np.array_equal(xr, xs)


@pytest.mark.parametrize("n", [257, 300])
def test_identity_preconditioner_is_plain_cg(n):
    """(b) minv = ones: z = r, every operation the unpreconditioned one -> cg_ref.cg's bits"""
    K, _, b0 = _system(n)
    H, _ = cg_ref.ill_conditioned(n, seed=5)
    x0 = np.random.default_rng(n + 2).standard_normal(n) * 1e-3
    for A, maxiter in ((K, 50), (H, 8)):
        for start in (None, x0):
            xp, ip, itp = pcg_ref.pcg(A, b0, np.ones(n), x0=start, maxiter=maxiter)
            xc, ic, itc = cg_ref.cg(A, b0, x0=start, maxiter=maxiter)
            assert (ip, itp) == (ic, itc) and np.array_equal(xp, xc)


@pytest.mark.parametrize("n", [257, 300])
def test_sign_symmetry(n):
    """(c) pcg(-H, -b, -minv) == pcg(H, b, minv) bit for bit (negation is exact, r, z, rho, p.q and
    alpha keep their magnitudes): the engine solves H dx = -g with M = 1 / h where the reference
    solves -H dx = g with M = -1 / h"""
    K, _, b0 = _system(n)
    H, b, _ = pcg_ref.scaled_system(K, b0, n + 3)
    minv = pcg_ref.jacobi(H)
    x0 = np.random.default_rng(n + 2).standard_normal(n) * 1e-3
    for start, maxiter in ((None, 200), (x0, 200), (None, 8)):
        xp, ip, itp = pcg_ref.pcg(H, b, minv, x0=start, maxiter=maxiter)
        xm, im, itm = pcg_ref.pcg(-H, -b, -minv, x0=start, maxiter=maxiter)
        assert (ip, itp) == (im, itm) and np.array_equal(xp, xm)
    # and the Newton step's form: (-H, g, -1 / h) == (H, -g, 1 / h)
    xp, ip, itp = pcg_ref.pcg(-H, b, -minv, maxiter=200)
    xm, im, itm = pcg_ref.pcg(H, -b, minv, maxiter=200)
    assert (ip, itp) == (im, itm) and np.array_equal(xp, xm)


@pytest.mark.parametrize("n", [257, 300])
def test_jacobi_iteration_count_is_scale_invariant(n):
    """(d) H = S K S, b = S b0, S = diag(10 ** U(-3, 3)) (cond(H) ~ 1e13): Jacobi-PCG converges in
    it_s iterations, within 2 of the it_0 it takes on K itself (measured 45 / 44 at n = 257, 43 / 43
    at n = 300), while plain CG runs into maxiter = 200.  The last two ||r|| / ||b|| of the PCG run
    are each at least 5 % away from rtol (measured 1.2e-5, 8.7e-6 at n = 257; 1.7e-5, 8.4e-6 at
    n = 300): another summation order moves them by ~1e-10 relative and cannot move the stopping
    iteration -- the GPU test's exact count rests on this."""
    K, _, b0 = _system(n)
    H, b, _ = pcg_ref.scaled_system(K, b0, n + 3)
    tr = []
    _, info_s, it_s = pcg_ref.pcg(H, b, pcg_ref.jacobi(H), maxiter=200, trace=tr)
    _, info_0, it_0 = pcg_ref.pcg(K, b0, pcg_ref.jacobi(K), maxiter=200)
    _, info_p, it_p = cg_ref.cg(H, b, maxiter=200)
    print(f"[pcg scale invariance n={n}] scaled {it_s} unscaled {it_0} plain cg info {info_p}; last two "
          f"||r||/||b|| {tr[-2]:.3g} {tr[-1]:.3g}")
    assert info_s == 0 and info_0 == 0
    assert abs(it_s - it_0) <= 2
    assert info_p == 200 and it_p == 200
    assert len(tr) == it_s + 1
    assert tr[-2] >= 1.05e-5 and tr[-1] <= 0.95e-5


@pytest.mark.parametrize("name", PCG_FIXTURES)
def test_pcg_fixture_loads(name):
    """(e) the conditions test_cg_fixture_loads puts on the cg_* fixtures, and the generator's own:
    plain CG at the same cap is at least 1e4 value_tol away unless the instance waives it"""
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    tol, val = float(z["value_tol"]), float(z["value"])
    assert np.isfinite(tol) and tol >= 1e-9 * abs(val) and tol >= 10 * float(z["ref_spread"])
    assert np.all(np.abs(z["ref_values"] - val) <= tol)
    assert np.all(np.isfinite(z["xstar"])) and int(z["outer_iters"]) > 0 and int(z["max_cg_iters"]) > 0
    assert str(z["kind"]) in ("LP", "QP", "SOCP")
    assert str(z["cg_preconditioner"]) == "jacobi"
    assert bool(z["plain_waived"]) or abs(float(z["plain_value"]) - val) >= 1e4 * tol


def test_scale_variables_keeps_the_problem():
    """problems.scale_variables: y = x / sigma is feasible where x is, with the same objective"""
    from ipm355 import problems
    inst = problems.lp_ineq_box(n=40, m=20, seed=3, with_xf=True)
    sigma = 10.0 ** np.random.default_rng(7).uniform(-2, 2, 40)
    sc = problems.scale_variables(inst, sigma)
    y = sc["xf"]
    assert np.allclose(sc["C"] @ y, inst["C"] @ inst["xf"], rtol=1e-13, atol=1e-13)
    assert np.isclose(sc["c"] @ y, inst["c"] @ inst["xf"], rtol=1e-13)
    assert np.array_equal(sc["d"], inst["d"])
    assert np.array_equal(sc["lower_bound"], -3 / sigma) and np.array_equal(sc["upper_bound"], 3 / sigma)
    assert inst["lower_bound"] == -3 and inst["C"] is not sc["C"]
