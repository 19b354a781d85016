"""-m gpu: full LPSolver(..., linear_solve_method='cholesky_dual') solves against the reference-run
fixtures lp_ineq_box, lp_ineq_box_testkw and cg_lp_n40 (read only), the reference's duals
(lp_ineq_box_duals) and one generated instance against the oracle's Cholesky solve.  Phase 1 runs on
the primal Cholesky, as with every other method; the barrier loop takes dual-form steps (Woodbury
solve plus three rounds of iterative refinement).
"""
import numpy as np
import pytest

import golden_io

pytestmark = pytest.mark.gpu
XSTAR_RTOL = 1e-6     # the project's bar


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _fixture(name):
    z = golden_io.load(name)
    kw = golden_io.solver_kwargs(z)
    kw = {k: (v.item() if isinstance(v, np.ndarray) and v.ndim == 0 else v) for k, v in kw.items()}
    kw.pop("linear_solve_method", None)
    if "x_init" in z:
        kw["x0"] = z["x_init"].copy()
    return z, kw


def _solve(kw, method):
    import ipm355
    kw = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    s = ipm355.LPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method=method, **kw)
    return s, s.solve()


@pytest.mark.parametrize("name", ["lp_ineq_box", "lp_ineq_box_testkw", "cg_lp_n40"])
def test_fixture_solves(name):
    import ipm355
    z, kw = _fixture(name)
    s, val = _solve(kw, "cholesky_dual")
    assert isinstance(s.ns, ipm355.NewtonSolverCholeskyDual) and not s.ns.use_backup
    xr, vr = rel(s.xstar, z["xstar"]), abs(val - float(z["value"]))
    print(f"[{name}] outer {s.outer_iters} inner {s.inner_iters} x* rel {xr:.2e} |value diff| {vr:.2e}")
    assert s.outer_iters == int(z["outer_iters"])
    if "inner_iters" in z:
        assert list(s.inner_iters) == list(z["inner_iters"])
    assert xr <= XSTAR_RTOL
    if "value_tol" in z:
        assert vr <= float(z["value_tol"])
    else:
        assert vr <= 1e-9 * abs(float(z["value"]))


def test_dual_variables():
    """get_dual_variables=True against the reference's lam* within max(1e-6, 4 x sens_lam_star_rel).
    lam* = 1 / (t s(x*)) at t = 1.3e13 needs the active slacks (~1e-14) to six digits: the plain
    Woodbury step misses that by far (4.35e-4 on the device), which is what the step's three rounds of
    iterative refinement are for (1.1e-9; the primal Cholesky: 6.9e-10).  DESIGN.md §11."""
    z, kw = _fixture("lp_ineq_box_duals")
    s, _ = _solve(kw, "cholesky_dual")
    tol = max(1e-6, 4 * float(z["sens_lam_star_rel"]))
    el = rel(s.lam_star, z["lam_star"])
    print(f"[lp_ineq_box_duals] lam* rel {el:.2e} (tol {tol:.1e}) inner {s.inner_iters}")
    assert list(s.inner_iters) == list(z["inner_iters"])
    assert el <= tol


def test_generated_instance_against_the_oracle():
    """n = 1024, m = 256 with the reference's test kwargs: four tiles of S per K chunk and the K split
    of its assembly, inside a whole solve"""
    from ipm355 import problems
    from oracle import ipm_oracle as O
    kw = dict(problems.lp_ineq_box(1024, 256, seed=11), **problems.LP_KWARGS)
    orc = O.LPSolver(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
    orc.solve()
    s, val = _solve(kw, "cholesky_dual")
    xr = rel(s.xstar, orc.xstar)
    print(f"[generated 1024 x 256] inner {s.inner_iters} (oracle {orc.inner_iters}) x* rel {xr:.2e} "
          f"value {val!r} oracle {orc.value!r}")
    assert s.outer_iters == orc.outer_iters
    assert list(s.inner_iters) == list(orc.inner_iters)
    assert xr <= XSTAR_RTOL


def test_cholesky_afterwards_is_untouched():
    """'cholesky' on the same fixture after a dual solve in the same process: the fixture's exact step
    sequence -- nothing shared between the two methods went stale"""
    z, kw = _fixture("lp_ineq_box")
    _solve(kw, "cholesky_dual")
    s, val = _solve(kw, "cholesky")
    steps = [t[0] for t in s.phase1_solver.phase1_ns.trace + s.ns.trace]
    assert list(s.inner_iters) == list(z["inner_iters"])
    np.testing.assert_array_equal(np.array(steps), z["trace_step"])
    assert rel(s.xstar, z["xstar"]) <= XSTAR_RTOL


def test_other_facades_reject_the_method():
    import ipm355
    from ipm355 import problems
    kw = problems.qp_ineq_box(32, 8, seed=1)
    with pytest.raises(ValueError, match="Please enter a valid linear solve method!"):
        ipm355.QPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method="cholesky_dual", **kw)
    sk = problems.socp_cones(n=16, K=2, mi=3, seed=1)
    with pytest.raises(ValueError, match="Please enter a valid linear solve method!"):
        ipm355.SOCPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method="cholesky_dual", **sk)
