"""-m gpu: full solves of ipm355.QPSolver(P_factor=F, P_diag=rho, linear_solve_method='cholesky_dual').

The solve instances of tests/dual_qp_ref.py end to end against the oracle's dense Cholesky solve (P formed on the
host) and against ipm355.QPSolver(P=dense, 'cholesky'): iteration lists equal on the cases for which
tests/test_dual_qp_ref.py shows the fp64 restatement keeps them, x* within max(1e-6, 4 x the oracle's own spread
under a 1e-15 relative perturbation of q), the value within the solver's epsilon of the oracle's.  The
reference-run fixtures dual_qp_factored / dual_qp_diagonal at the bars of test_gpu_parity.py.  Phase 1 in the dual
form, a bound-free instance, the dual variables, and a dense solve before and after a factored one.
"""
import numpy as np
import pytest

import dual_qp_ref as Q
import golden_io

pytestmark = pytest.mark.gpu
QUIET = dict(check_cvxpy=False, suppress_print=True)


def _factored(kw, **extra):
    import ipm355
    s = ipm355.QPSolver(linear_solve_method="cholesky_dual", **QUIET, **Q.copy_kw(kw), **extra)
    s.solve()
    return s


def _dense(kw, **extra):
    import ipm355
    s = ipm355.QPSolver(linear_solve_method="cholesky", **QUIET, **Q.copy_kw(kw), **extra)
    s.solve()
    return s


@pytest.mark.parametrize("case", Q.SOLVES, ids=Q.solve_id)
def test_solves_against_the_oracle_and_the_dense_device_solver(case):
    import ipm355
    ref = Q.solve_reference(case)
    a = ref["solver"]
    s = _factored(ref["fac"])
    assert isinstance(s.ns, ipm355.NewtonSolverCholeskyDualQP) and s.fm.prob.P is None
    assert s.fm.prob.use_backup is False
    dn = _dense(ref["dense"])
    eps = case[5].get("epsilon", 1e-10)
    for other, x_o, v_o, it_o in (("oracle", a.xstar, a.value, list(a.inner_iters)),
                                  ("dense device", dn.xstar, dn.value, list(dn.inner_iters))):
        xr = float(np.linalg.norm(s.xstar - x_o) / np.linalg.norm(x_o))
        print(f"[{Q.solve_id(case)}] vs {other}: inner {list(s.inner_iters)} ({it_o}) x* rel {xr:.2e} (bar "
              f"{ref['xbar']:.1e}) value {s.value!r} ({v_o!r})")
        assert xr <= ref["xbar"], (other, xr)
        assert abs(s.value - v_o) <= eps * max(1.0, abs(v_o)), other
        if Q.solve_id(case) not in Q.NOT_EXACT:
            assert list(s.inner_iters) == it_o, other
    print(f"[{Q.solve_id(case)}] phase 1 {list(s.phase1_solver.inner_iters) if s.phase1_solver else []} "
          f"(oracle, Cholesky: {list(a.phase1_iters)})")


@pytest.mark.parametrize("name", ["dual_qp_factored", "dual_qp_diagonal"])
def test_reference_fixtures_at_the_parity_bars(name):
    z = golden_io.load(name)
    kw = golden_io.solver_kwargs(z)
    s = _factored(kw)
    xr = float(np.linalg.norm(s.xstar - z["xstar"]) / np.linalg.norm(z["xstar"]))
    vr = abs(s.value - float(z["value"])) / max(1.0, abs(float(z["value"])))
    print(f"[{name}] x* rel {xr:.2e} value rel {vr:.2e} inner {list(s.inner_iters)} (reference {list(z['inner_iters'])})")
    assert xr <= max(1e-6, 4 * float(z["sens_xstar_rel"]))
    assert vr <= max(1e-8, 4 * float(z["sens_value_rel"]))
    if bool(z["sens_iters_stable"]):
        assert list(s.inner_iters) == list(z["inner_iters"]) and s.outer_iters == int(z["outer_iters"])


def test_phase_one_runs_in_the_dual_form():
    """x0 default, C and bounds: phase 1 is needed, and a factored QP builds it with linear_solve_method=
    'cholesky_dual' (IPM_SOLVE_CHOLESKY_DUAL_PHASE1): nothing of size n^2 in either phase"""
    import ipm355
    from ipm355 import _lib as L
    case = (64, 16, 8, "ones", {}, Q.TIGHT)
    ref = Q.solve_reference(case)
    a = ref["solver"]
    assert len(a.phase1_iters) > 0
    s = _factored(ref["fac"])
    p1 = s.phase1_solver
    assert isinstance(p1.phase1_ns, ipm355.NewtonSolverCholeskyDual)
    assert p1.phase1_fm.prob.desc.solve_method == L.SOLVE_CHOLESKY_DUAL_PHASE1
    assert sum(p1.inner_iters) > 0
    # without a bound the dual form of phase 1 is not eligible: the primal Cholesky
    fac = dict(ref["fac"], lower_bound=None, upper_bound=None)
    s2 = ipm355.QPSolver(linear_solve_method="cholesky_dual", **QUIET, **Q.copy_kw(fac))
    assert isinstance(s2.phase1_solver.phase1_ns, ipm355.NewtonSolverCholesky)
    assert s2.phase1_solver.phase1_fm.prob.desc.solve_method == L.SOLVE_CHOLESKY


def test_bound_free_instance_from_a_feasible_start():
    """no bound, rho > 0, x0 = x_f: D = t rho alone"""
    from ipm355 import problems
    n, m, k = 130, 40, 12
    inst = problems.qp_factor_box(n, m, k, seed=7, rho="pow2", with_xf=True)
    xf = inst.pop("xf")
    fac = dict(inst, lower_bound=None, upper_bound=None, **Q.TIGHT)
    F, r = fac["P_factor"], fac["P_diag"]
    P = F.T @ F
    P[np.diag_indices(n)] += r
    dense = {key: v for key, v in fac.items() if key not in ("P_factor", "P_diag")}
    a = Q.oracle_qp(dict(dense, P=P, x0=xf.copy()))
    s = _factored(fac, x0=xf.copy())
    xr = float(np.linalg.norm(s.xstar - a.xstar) / np.linalg.norm(a.xstar))
    print(f"bound-free: inner {list(s.inner_iters)} (oracle {list(a.inner_iters)}) x* rel {xr:.2e}")
    assert xr <= 1e-6          # (DESIGN.md §2's floor of the x* bar)
    assert abs(s.value - a.value) <= 1e-6 * max(1.0, abs(a.value))


def test_dual_variables_track_loss_and_stale_slacks():
    eps = np.finfo(np.float64).eps
    case = (64, 16, 8, "ones", {}, Q.TIGHT)
    fac = Q.generated(case)[0]
    s = _factored(fac, get_dual_variables=True, track_loss=True)
    t_last = 1
    for _ in range(s.outer_iters - 1):          # the barrier loop's own sequence t <- t mu, stopped at the gap test
        t_last = t_last * 15
    assert s.optimality_gap == s.num_constraints / t_last < 1e-6
    s.fm.update_x(s.xstar)
    lam = 1 / (t_last * s.fm.slacks)
    assert lam.shape == (16 + 2 * 64,) and np.all(s.lam_star > 0)
    assert np.all(np.abs(s.lam_star - lam) <= 2 * eps * np.abs(lam))
    assert len(s.objective_vals) == s.outer_iters and min(s.objective_vals) == s.value
    s2 = _factored(fac, update_slacks_every=2)
    assert np.linalg.norm(s2.xstar - s.xstar) <= 1e-6 * np.linalg.norm(s.xstar)


def test_a_dense_solve_before_and_after_gives_the_same_bits():
    case = (64, 16, 8, "ones", {}, Q.TIGHT)
    fac, dense = Q.generated(case)
    a = _dense(dense)
    f1 = _factored(fac)
    b = _dense(dense)
    f2 = _factored(fac)
    assert a.xstar.tobytes() == b.xstar.tobytes() and a.value == b.value
    assert list(a.inner_iters) == list(b.inner_iters)
    assert f1.xstar.tobytes() == f2.xstar.tobytes() and f1.value == f2.value
