"""-m gpu: LPSolver(linear_solve_method='cholesky_dual_eq') end to end, against the CPU oracle's Cholesky
solves (oracle/ipm_oracle.py) and the reference-run fixtures.

  * six generated LPs with A x = b, C x <= d and bounds, cut at four barrier iterations (beyond them the
    reference's own infeasible-start trajectory is not reproducible: its iteration lists change under a
    1e-15 input perturbation): iteration lists equal the oracle's, x* within 4 x the oracle's own spread
    (or 1e-9) -- the bar tests/test_dual_eq_ref.py holds the fp64 restatement to;
  * lp_eq_ineq and lp_npy_miplib at the bars of test_gpu_parity.py, with the default phase 1 and with
    phase1_linear_solve_method='cholesky_dual';
  * get_dual_variables, one full-length solve judged by what the algorithm guarantees, 'cholesky' unchanged by
    a dual solve in the same process, QPSolver / SOCPSolver reject the string.
"""
import numpy as np
import pytest

import dual_eq_ref as Q
import golden_io

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
QUIET = dict(check_cvxpy=False, suppress_print=True)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


@pytest.mark.parametrize("shape", Q.SOLVE_SHAPES, ids=lambda s: "n%d-p%d-m%d" % s)
def test_short_solves_keep_the_oracles_trajectory(shape):
    import ipm355
    ref = Q.short_reference(shape)
    a = ref["solver"]
    s = ipm355.LPSolver(linear_solve_method="cholesky_dual_eq", **QUIET, **Q.copy_kw(ref["kw"]))
    s.solve(max_outer_iters=Q.SHORT_OUTER)
    xr = rel(s.xstar, a.xstar)
    print(f"[{shape}] inner {list(s.inner_iters)} (oracle {list(a.inner_iters)}) x* rel {xr:.2e} bar {ref['xbar']:.2e}")
    assert s.ns.use_backup is False
    assert list(s.inner_iters) == list(a.inner_iters)
    assert xr <= ref["xbar"]


def _fixture(name, **extra):
    import ipm355
    z = golden_io.load(name)
    kw = golden_io.solver_kwargs(z)
    kw["x0"] = z["x_init"].copy()
    kw.update(QUIET)
    kw.update(extra)
    s = ipm355.LPSolver(**kw)
    return z, s, s.solve()


@pytest.mark.parametrize("phase1", [None, "cholesky_dual"], ids=["phase1-cholesky", "phase1-dual"])
@pytest.mark.parametrize("name", ["lp_eq_ineq", "lp_npy_miplib"])
def test_fixtures_at_the_parity_bars(name, phase1):
    z, s, v = _fixture(name, linear_solve_method="cholesky_dual_eq", phase1_linear_solve_method=phase1)
    xr = rel(s.xstar, z["xstar"])
    vr = abs(v - float(z["value"])) / max(1.0, abs(float(z["value"])))
    print(f"[{name}, phase 1 {phase1}] x* rel {xr:.2e} value rel {vr:.2e} inner {list(s.inner_iters)} "
          f"(fixture {[int(k) for k in z['inner_iters']]})")
    assert xr <= max(1e-6, 4 * float(z["sens_xstar_rel"]))
    assert vr <= max(1e-8, 4 * float(z["sens_value_rel"]))


def test_dual_variables_of_a_short_solve():
    """v_star = v / t through the shared code, against the oracle's at the x* bar; lam_star positive and
    1 / (t slacks) of this run's own slacks"""
    import ipm355
    from oracle import ipm_oracle as O
    shape = (130, 30, 97)
    ref = Q.short_reference(shape)
    o = O.LPSolver(get_dual_variables=True, **Q.copy_kw(ref["kw"]))
    o.solve(max_outer_iters=Q.SHORT_OUTER)
    s = ipm355.LPSolver(linear_solve_method="cholesky_dual_eq", get_dual_variables=True, **QUIET,
                        **Q.copy_kw(ref["kw"]))
    s.solve(max_outer_iters=Q.SHORT_OUTER)
    assert list(s.inner_iters) == list(o.inner_iters)
    vr = rel(s.v_star, o.v_star)
    print(f"v_star rel {vr:.2e} (bar {ref['xbar']:.2e}), lam_star rel {rel(s.lam_star, o.lam_star):.2e}")
    assert s.v_star.shape == (shape[1],) and vr <= ref["xbar"]
    lam = np.asarray(s.lam_star.cpu() if hasattr(s.lam_star, "cpu") else s.lam_star)
    slacks = np.asarray(s.fm.slacks.cpu() if hasattr(s.fm.slacks, "cpu") else s.fm.slacks)
    kw = ref["kw"]
    t = kw["t0"] * kw["mu"] ** Q.SHORT_OUTER        # four barrier iterations, none stopped by the gap
    assert s.outer_iters == Q.SHORT_OUTER and (lam > 0).all() and lam.shape == slacks.shape
    np.testing.assert_allclose(lam, 1 / (t * slacks), rtol=2 * EPS, atol=0)     # two correctly rounded operations


def test_full_length_solve_by_what_the_algorithm_guarantees():
    """(130, 30, 97) with LP_KWARGS, all ten barrier iterations: not pinned to a trajectory.  The solve
    returns, A x* = b holds to the inner tolerance (or the oracle Cholesky solve's own residual), and the two
    values lie within the final duality gap epsilon of the optimum, so within epsilon of each other
    (the fp64 restatement: 3e-8 and 2.7e-6 against 1e-5 and 1e-4)"""
    import ipm355
    kw = Q.generated(130, 30, 97)
    o = Q.oracle_lp(Q.copy_kw(kw), False)
    s = ipm355.LPSolver(linear_solve_method="cholesky_dual_eq", **QUIET, **Q.copy_kw(kw))
    v = s.solve()
    assert v is not None and np.isfinite(v) and np.all(np.isfinite(s.xstar))
    res, res_o = np.linalg.norm(kw["A"] @ s.xstar - kw["b"]), np.linalg.norm(kw["A"] @ o.xstar - kw["b"])
    print(f"||A x* - b|| {res:.2e} (oracle {res_o:.2e}); value {v:.12g} (oracle {o.value:.12g}, diff {abs(v - o.value):.2e}); "
          f"inner {list(s.inner_iters)} (oracle {list(o.inner_iters)})")
    assert res <= max(s.inner_epsilon, res_o)
    assert abs(v - o.value) <= kw["epsilon"]


def test_cholesky_is_unchanged_by_a_dual_solve_in_the_same_process():
    _, a, va = _fixture("lp_eq_ineq")
    _fixture("lp_eq_ineq", linear_solve_method="cholesky_dual_eq")
    _, b, vb = _fixture("lp_eq_ineq")
    assert va == vb and list(a.inner_iters) == list(b.inner_iters)
    assert a.xstar.tobytes() == b.xstar.tobytes()
    assert [t[0] for t in a.ns.trace] == [t[0] for t in b.ns.trace]


def test_other_facades_reject_the_method():
    import ipm355
    from ipm355 import problems
    kw = problems.qp_ineq_box(32, 8, seed=1)
    with pytest.raises(ValueError, match="Please enter a valid linear solve method!"):
        ipm355.QPSolver(linear_solve_method="cholesky_dual_eq", **QUIET, **kw)
    sk = problems.socp_cones(n=16, K=2, mi=3, seed=1)
    with pytest.raises(ValueError, match="Please enter a valid linear solve method!"):
        ipm355.SOCPSolver(linear_solve_method="cholesky_dual_eq", **QUIET, **sk)
