"""-m gpu: whole phase-1 solves and LP solves with the dual-form phase 1
(PhaseOneSolver(linear_solve_method='cholesky_dual'), LPSolver(phase1_linear_solve_method='cholesky_dual'))
against the reference-run fixtures (read only) and the oracle.  Every phase-1 Newton step goes through the
bordered m x m system (IPM_SOLVE_CHOLESKY_DUAL_PHASE1); no (n+1) x (n+1) Hessian exists.
"""
import numpy as np
import pytest

import golden_io

pytestmark = pytest.mark.gpu
XSTAR_RTOL = 1e-6     # the project's bar


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _copy(kw):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


def _fixture(name):
    z = golden_io.load(name)
    kw = golden_io.solver_kwargs(z)
    kw = {k: (v.item() if isinstance(v, np.ndarray) and v.ndim == 0 else v) for k, v in kw.items()}
    kw.pop("linear_solve_method", None)
    if "x_init" in z:
        kw["x0"] = z["x_init"].copy()
    return z, kw


def _solve(kw, method, phase1_method="cholesky_dual"):
    import ipm355
    s = ipm355.LPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method=method,
                        phase1_linear_solve_method=phase1_method, **_copy(kw))
    return s, s.solve()


def _oracle(kw):
    from oracle import ipm_oracle as O
    s = O.LPSolver(**_copy(kw))
    return s


def _phase_one(kw):
    """the facade's PhaseOneSolver in dual form, built with the arguments LPSolver passes, and the oracle's
    PhaseOne for the same kwargs (unsolved)"""
    import ipm355
    orc = _oracle(kw)
    g = lambda k, dflt: kw.get(k, dflt)  # noqa: E731
    lb, ub = g("lower_bound", 0), g("upper_bound", None)
    p1 = ipm355.PhaseOneSolver(C=kw["C"].copy(), d=kw["d"].copy(), lower_bound=lb, upper_bound=ub, x0=orc.x.copy(),
                               max_outer_iters=g("max_outer_iters", 20), max_inner_iters=500,
                               epsilon=g("epsilon", 1e-10), inner_epsilon=1e-5, alpha=g("alpha", 0.2),
                               beta=g("beta", 0.6), mu=g("mu", 15), suppress_print=True, n=len(orc.x), tol=0,
                               t0=0.01, linear_solve_method="cholesky_dual")
    return p1, orc


@pytest.mark.parametrize("name", ["lp_ineq_box", "lp_ineq_box_testkw"])
def test_phase_one_solver_keeps_the_fixture_lists(name):
    import ipm355
    z, kw = _fixture(name)
    p1, _ = _phase_one(kw)
    assert isinstance(p1.phase1_ns, ipm355.NewtonSolverCholeskyDual)
    assert p1.phase1_fm.prob.desc.solve_method == ipm355._lib.SOLVE_CHOLESKY_DUAL_PHASE1
    x, s = p1.solve()
    print(f"[{name}] phase 1 inner {p1.inner_iters} s {s:.3g}")
    assert list(p1.inner_iters) == list(z["phase1_inner_iters"])
    assert s < 0 and not p1.phase1_ns.use_backup


def _generated(n, m, lo, hi):
    from ipm355 import problems
    return dict(problems.lp_ineq_box(n, m, seed=11), **problems.LP_KWARGS, lower_bound=lo, upper_bound=hi)


ORACLE_CASES = {"cg_lp_n40": None, "generated-130x127-lb": (130, 127, -3, None), "generated-64x63-ub": (64, 63, None, 3)}


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_phase_one_solver_against_the_oracle(name):
    kw = _fixture(name)[1] if ORACLE_CASES[name] is None else _generated(*ORACLE_CASES[name])
    p1, orc = _phase_one(kw)
    x, s = p1.solve()
    xo, so = orc.phase1.solve()
    xr = rel(x.cpu().numpy(), xo)
    print(f"[{name}] phase 1 inner {p1.inner_iters} (oracle {orc.phase1.inner_iters}) exit x rel {xr:.2e} s {s:.6g} / {so:.6g}")
    assert list(p1.inner_iters) == list(orc.phase1.inner_iters)
    assert xr <= XSTAR_RTOL


@pytest.mark.parametrize("name", ["lp_ineq_box", "lp_ineq_box_testkw", "cg_lp_n40"])
def test_fixture_solves_with_both_phases_dual(name):
    import ipm355
    z, kw = _fixture(name)
    s, val = _solve(kw, "cholesky_dual")
    assert isinstance(s.ns, ipm355.NewtonSolverCholeskyDual) and not s.ns.use_backup
    assert isinstance(s.phase1_solver.phase1_ns, ipm355.NewtonSolverCholeskyDual)
    assert not s.phase1_solver.phase1_ns.use_backup
    xr, vr = rel(s.xstar, z["xstar"]), abs(val - float(z["value"]))
    print(f"[{name}] phase 1 {s.phase1_solver.inner_iters} outer {s.outer_iters} inner {s.inner_iters} "
          f"x* rel {xr:.2e} |value diff| {vr:.2e}")
    assert s.outer_iters == int(z["outer_iters"])
    if "inner_iters" in z:
        assert list(s.inner_iters) == list(z["inner_iters"])
    if "phase1_inner_iters" in z:
        assert list(s.phase1_solver.inner_iters) == list(z["phase1_inner_iters"])
    assert xr <= XSTAR_RTOL
    if "value_tol" in z:
        assert vr <= float(z["value_tol"])
    else:
        assert vr <= 1e-9 * abs(float(z["value"]))


def test_dual_variables():
    z, kw = _fixture("lp_ineq_box_duals")
    s, _ = _solve(kw, "cholesky_dual")
    tol = max(1e-6, 4 * float(z["sens_lam_star_rel"]))
    el = rel(s.lam_star, z["lam_star"])
    print(f"[lp_ineq_box_duals] lam* rel {el:.2e} (tol {tol:.1e}) phase 1 {s.phase1_solver.inner_iters} inner {s.inner_iters}")
    assert list(s.phase1_solver.inner_iters) == list(z["phase1_inner_iters"])
    assert list(s.inner_iters) == list(z["inner_iters"])
    assert el <= tol


def test_generated_instance_against_the_oracle():
    """n = 1024, m = 256 with the reference's test kwargs: both phases in dual form inside a whole solve"""
    kw = _generated(1024, 256, -3, 3)
    orc = _oracle(kw)
    orc.solve()
    s, val = _solve(kw, "cholesky_dual")
    xr = rel(s.xstar, orc.xstar)
    print(f"[generated 1024 x 256] phase 1 {s.phase1_solver.inner_iters} (oracle {orc.phase1_iters}) inner "
          f"{s.inner_iters} (oracle {orc.inner_iters}) x* rel {xr:.2e} value {val!r} oracle {orc.value!r}")
    assert list(s.phase1_solver.inner_iters) == list(orc.phase1_iters) and len(orc.phase1_iters) > 0
    assert s.outer_iters == orc.outer_iters
    assert list(s.inner_iters) == list(orc.inner_iters)
    assert xr <= XSTAR_RTOL


def test_cholesky_barrier_phase_with_dual_phase_one():
    import ipm355
    z, kw = _fixture("lp_ineq_box")
    s, val = _solve(kw, "cholesky")
    assert isinstance(s.ns, ipm355.NewtonSolverCholesky)
    assert isinstance(s.phase1_solver.phase1_ns, ipm355.NewtonSolverCholeskyDual)
    assert list(s.phase1_solver.inner_iters) == list(z["phase1_inner_iters"])
    assert list(s.inner_iters) == list(z["inner_iters"]) and s.outer_iters == int(z["outer_iters"])
    assert rel(s.xstar, z["xstar"]) <= XSTAR_RTOL


def test_cholesky_afterwards_is_untouched():
    """a default 'cholesky' solve on the same fixture after the dual solves in the same process: the
    fixture's exact step sequence -- nothing shared between the methods went stale"""
    z, kw = _fixture("lp_ineq_box")
    _solve(kw, "cholesky_dual")
    s, val = _solve(kw, "cholesky", phase1_method=None)
    steps = [t[0] for t in s.phase1_solver.phase1_ns.trace + s.ns.trace]
    assert list(s.inner_iters) == list(z["inner_iters"])
    np.testing.assert_array_equal(np.array(steps), z["trace_step"])
    assert rel(s.xstar, z["xstar"]) <= XSTAR_RTOL


def test_without_the_keyword_phase_one_stays_on_cholesky():
    import ipm355
    _, kw = _fixture("lp_ineq_box_testkw")
    s = ipm355.LPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method="cholesky_dual", **_copy(kw))
    ns = s.phase1_solver.phase1_ns
    assert type(ns) is ipm355.NewtonSolverCholesky
    assert s.phase1_solver.phase1_fm.prob.desc.solve_method == ipm355._lib.SOLVE_CHOLESKY
