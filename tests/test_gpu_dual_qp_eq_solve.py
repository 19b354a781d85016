"""-m gpu: full solves through QPSolver(P_factor=F, P_diag=rho, A=A, b=b, linear_solve_method='cholesky_dual_eq')
(IPM_SOLVE_CHOLESKY_DUAL_QP_EQ).

  * five generated instances (problems.qp_factor_eq_box on the 2^-10 grid: the dense P a test forms is exact)
    against the CPU oracle's Cholesky block elimination on the dense P, x* inside max(1e-6, 4 x the oracle's own
    spread under a 1e-15 perturbation of q and b), inner-iteration counts up to the barrier iteration until which
    that perturbation leaves the oracle's own counts unchanged; and against the device's own dense 'cholesky' QP
    with the same A (the same bars); ||A x* - b|| is reported.  (Beyond the cut the counts may differ: at
    (257, 40, 33, 30), cut 9, the tenth count is 9 for the oracle and the dense device solve and 11 here, with x*
    3e-14 from the oracle's);
  * one solve with both phases in the dual form (an infeasible start: phase 1 runs, ignoring A and P);
  * a rank-deficient A (a duplicated row) raises LinAlgError; the duals nu = v / t come out.
"""
import numpy as np
import pytest

import dual_qp_eq_ref as R

pytestmark = pytest.mark.gpu
QUIET = dict(check_cvxpy=False, suppress_print=True)


@pytest.mark.parametrize("case", R.SOLVES, ids=R.solve_id)
def test_generated_instances_against_the_oracle_and_the_dense_device_solve(case):
    import ipm355
    ref = R.solve_reference(case)
    a, fac, dense = ref["solver"], ref["fac"], ref["dense"]
    s = ipm355.QPSolver(linear_solve_method="cholesky_dual_eq", get_dual_variables=True, **R.Q.copy_kw(fac), **QUIET)
    val = s.solve()
    assert s.fm.prob.desc.solve_method == ipm355._lib.SOLVE_CHOLESKY_DUAL_QP_EQ and s.fm.prob.AT is None
    dev = ipm355.QPSolver(**R.Q.copy_kw(dense), **QUIET)
    vdev = dev.solve()
    nrm = float(np.linalg.norm(a.xstar))
    xr_o = float(np.linalg.norm(s.xstar - a.xstar)) / nrm
    xr_d = float(np.linalg.norm(s.xstar - dev.xstar)) / nrm
    res = float(np.linalg.norm(fac["A"] @ s.xstar - fac["b"]))
    cut = min(ref["cut"], R.CUTS[R.solve_id(case)])     # (the recorded cut, or a shorter one found on this host)
    print(f"[{R.solve_id(case)}] x* rel to the oracle {xr_o:.2e}, to the dense device solve {xr_d:.2e} (bar "
          f"{ref['xbar']:.2e}); value {val:.12g} / oracle {a.value:.12g} / dense {vdev:.12g}; |Ax-b| {res:.2e}; cut "
          f"{cut}; inner {list(s.inner_iters)} oracle {list(a.inner_iters)} dense {list(dev.inner_iters)}")
    assert xr_o <= ref["xbar"] and xr_d <= ref["xbar"]
    assert abs(val - a.value) <= max(1e-8, 4 * ref["spread"]) * max(1.0, abs(a.value))
    assert list(s.inner_iters)[:cut] == list(a.inner_iters)[:cut]
    assert s.v_star.shape == (case[3],) and np.all(np.isfinite(s.v_star))


def test_both_phases_in_the_dual_form():
    """x0 violates C x <= d: phase 1 runs, in its dual form (C and a bound are given), ignoring A and P; the
    barrier phase is method 10"""
    import ipm355
    from ipm355 import _lib as L
    from ipm355 import problems
    n, m, k, p = 96, 24, 12, 8
    inst = problems.qp_factor_eq_box(n, m, k, p, seed=9, grid=True, with_xf=True)
    xf = inst.pop("xf")
    x0 = np.clip(xf + 1.5 * np.sign(inst["C"][0]), -2.9, 2.9)           # inside the box, beyond row 0 of C x <= d
    assert (inst["C"] @ x0 >= inst["d"]).any()
    kw = dict(inst, **problems.QP_KWARGS)
    s = ipm355.QPSolver(linear_solve_method="cholesky_dual_eq", x0=x0.copy(), **kw, **QUIET)
    assert s.phase1_solver is not None and s.phase1_solver.phase1_fm.s >= 1
    assert s.phase1_solver.phase1_fm.prob.desc.solve_method == L.SOLVE_CHOLESKY_DUAL_PHASE1
    s.solve()
    F, rho = inst["P_factor"], inst["P_diag"]
    P = F.T @ F
    P[np.diag_indices(n)] += rho
    dense = {key: v for key, v in kw.items() if key not in ("P_factor", "P_diag")}
    d = ipm355.QPSolver(P=P, x0=x0.copy(), **dense, **QUIET)
    d.solve()
    xr = float(np.linalg.norm(s.xstar - d.xstar) / np.linalg.norm(d.xstar))
    print(f"both phases dual: x* rel to the dense device solve {xr:.2e}, value {s.value:.12g} / {d.value:.12g}, "
          f"phase 1 {list(s.phase1_solver.inner_iters)}, inner {list(s.inner_iters)} / {list(d.inner_iters)}")
    assert xr <= 1e-6
    assert s.fm.prob.desc.solve_method == L.SOLVE_CHOLESKY_DUAL_QP_EQ


def test_rank_deficient_a_raises():
    import ipm355
    inst = ipm355.problems.qp_factor_eq_box(64, 16, 8, 4, seed=5, grid=True)
    inst["A"][3] = inst["A"][0]
    inst["b"][3] = inst["b"][0]
    s = ipm355.QPSolver(linear_solve_method="cholesky_dual_eq", **inst, **ipm355.problems.QP_KWARGS, **QUIET)
    with pytest.raises(np.linalg.LinAlgError, match="cholesky_dual_eq"):
        s.solve()
    assert s.ns.last_result.linalg_error == 1 and not s.ns.last_result.use_backup


@pytest.mark.parametrize("name", ["dual_qp_eq_factored", "dual_qp_eq_budget"])
def test_fixtures_of_the_reference_s_own_runs(name):
    """the reference's QPSolver('cholesky') on the dense P with A, b (tests/golden/make_golden_dual_qp_eq.py):
    x* inside max(1e-6, 4 sens), the value inside max(1e-8, 4 sens), iteration lists where sens_iters_stable"""
    import ipm355
    import golden_io
    z = golden_io.load(name)
    kw = golden_io.solver_kwargs(z)
    s = ipm355.QPSolver(linear_solve_method="cholesky_dual_eq", **kw, **QUIET)
    assert s.fm.prob.desc.solve_method == ipm355._lib.SOLVE_CHOLESKY_DUAL_QP_EQ
    val = s.solve()
    xr = float(np.linalg.norm(s.xstar - z["xstar"]) / np.linalg.norm(z["xstar"]))
    vr = abs(val - float(z["value"])) / max(1.0, abs(float(z["value"])))
    print(f"[{name}] x* rel {xr:.2e} value rel {vr:.2e} inner {list(s.inner_iters)} (fixture {list(z['inner_iters'])}) "
          f"|Ax-b| {np.linalg.norm(kw['A'] @ s.xstar - kw['b']):.2e}")
    assert xr <= max(1e-6, 4 * float(z["sens_xstar_rel"]))
    assert vr <= max(1e-8, 4 * float(z["sens_value_rel"]))
    if bool(z["sens_iters_stable"]):
        assert list(s.inner_iters) == list(z["inner_iters"])
