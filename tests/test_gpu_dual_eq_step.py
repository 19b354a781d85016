"""-m gpu: one Newton step of IPM_SOLVE_CHOLESKY_DUAL_EQ (linear_solve_method='cholesky_dual_eq') through
ipm_newton_solve (max_iters = 1) on LP device problems with equality rows.

The device directions (ipm_fm_last_direction / ipm_fm_last_dual_direction: what the linear solve left, before
the step size) are compared as [dx; v + dv] with the long-double solve of the KKT system
[[H, A^T], [A, 0]] [dx; nu] = [-g; -(A x - b)] within

    B = 64 eps cond2(KKT) ||[dx; nu]||_2

over the grid of tests/dual_eq_ref.py: 10 shapes (m, p and m + p on both sides of the 16-row MFMA block and of
the 64-row tile, the seam between C and A inside and at the edge of a 64-row block, the K split of the
assembly), three bound sets, t in {1, 1e3, 1e6} and points 0, 0.9 and 0.999 of the way to the boundary.
tests/test_dual_eq_ref.py (no GPU) holds the fp64 restatement of the step to B / 4 on the same states.
"""
import numpy as np
import pytest

import dual_eq_ref as Q

pytestmark = pytest.mark.gpu
ALPHA, BETA = 0.2, 0.6
NOT_SUPPORTED = "ipm355 error 4"


def _solver(fm, inst, **kw):
    import ipm355
    from ipm355 import _lib as L
    dual = fm.prob.desc.solve_method == L.SOLVE_CHOLESKY_DUAL_EQ
    cls = ipm355.NewtonSolverCholeskyDualInfeasibleStart if dual else ipm355.NewtonSolverCholeskyInfeasibleStart
    return cls(inst.A, inst.b, inst.C, inst.d, fm, max_iters=1, epsilon=1e-5, alpha=ALPHA, beta=BETA, **kw)


def _step(fm, inst, t, **kw):
    """one Newton step from the instance's point and dual -> (dx, dv, step size, x after, v after)"""
    fm.update_t(t)
    ns = _solver(fm, inst, **kw)
    x, v = inst.x.copy(), inst.v.copy()
    _, _, iters, _, _ = ns.solve(x, t, v0=v)
    assert iters == 1
    return (fm.prob.last_direction().cpu().numpy(), fm.prob.last_dual_direction().cpu().numpy(), ns.trace[0][0], x, v)


GROUPS = [(n, p, m, b) for (n, p, m) in Q.SHAPES for b in Q.BOUNDS]


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"n{g[0]}-p{g[1]}-m{g[2]}-{g[3]}")
def test_direction_within_bound_and_step_size(group):
    """every (t, point) of one (shape, bounds): the device problems are created once per point (their data
    does not depend on t).  The accepted step size must equal the Cholesky problem's on the same state -- and
    the oracle's -- wherever each of the oracle's line-search decisions is at least 1e-9 from flipping."""
    from ipm355 import _lib as L
    n, p, m, b = group
    worst, compared = 0.0, 0
    for frac in Q.FRACS:
        inst = Q.instance(n, p, m, b, frac)
        fm_dual = inst.device(L.SOLVE_CHOLESKY_DUAL_EQ)
        fm_chol = inst.device(L.SOLVE_CHOLESKY)
        for t in Q.TS:
            state = (n, p, m, b, t, frac)
            ref = Q.reference_step(state)
            dx, dv, step, x, v = _step(fm_dual, inst, t)
            assert fm_dual.prob.use_backup is False
            assert np.all(np.isfinite(dx)) and np.all(np.isfinite(dv)) and np.all(np.isfinite(x))
            r = Q.joint_error(dx, dv, ref)
            worst = max(worst, r)
            assert r <= 1.0, (Q.state_id(state), r)
            np.testing.assert_array_equal(x, inst.x + step * dx)
            np.testing.assert_array_equal(v, inst.v + step * dv)
            ls = Q.oracle_line_search(state, ALPHA, BETA)
            if ls["decisive"]:
                _, _, step_c, _, _ = _step(fm_chol, inst, t)
                compared += 1
                assert step == step_c == ls["step"], (Q.state_id(state), step, step_c, ls)
    print(f"[n{n} p{p} m{m} {b}] worst |[dx; nu] - ref| / B {worst:.3g}; step size compared on {compared} of 9 states")


SAME_H = [(17, 3, 15, "both", 1e3, 0.9), (65, 17, 64, "lb", 1e3, 0.9), (257, 65, 129, "ub", 1e6, 0.999)]


@pytest.mark.parametrize("state", SAME_H, ids=Q.state_id)
def test_psd_condition_and_stale_slack_options(state):
    """use_psd_condition = 1: 1e-9 on D (the reference with the same add on H's diagonal: the same system);
    update_slacks_every > 0 changes the line search, not the system of the step: the plain reference"""
    from ipm355 import _lib as L
    n, p, m, b, t, frac = state
    inst = Q.instance(n, p, m, b, frac)
    fm = inst.device(L.SOLVE_CHOLESKY_DUAL_EQ)
    for kw, add in ((dict(use_psd_condition=True), 1e-9), (dict(update_slacks_every=2), 0.0)):
        ref = Q.reference_step(state, add)
        dx, dv, _, _, _ = _step(fm, inst, t, **kw)
        r = Q.joint_error(dx, dv, ref)
        print(f"[{Q.state_id(state)}] {kw}: |[dx; nu] - ref| / B {r:.3g}")
        assert r <= 1.0, (kw, r)
    plain, psd = Q.reference_step(state, 0.0)["sol"], Q.reference_step(state, 1e-9)["sol"]
    assert np.linalg.norm(plain - psd) > 0


@pytest.mark.parametrize("shape", [(17, 3, 15), (129, 64, 64), (520, 130, 127)], ids=lambda s: "n%d-p%d-m%d" % s)
def test_repeat_step_is_bitwise_equal(shape):
    from ipm355 import _lib as L
    inst = Q.instance(*shape, "both", 0.9)
    fm = inst.device(L.SOLVE_CHOLESKY_DUAL_EQ)
    a = _step(fm, inst, 1e3)
    b = _step(fm, inst, 1e3)
    fm2 = inst.device(L.SOLVE_CHOLESKY_DUAL_EQ)
    c = _step(fm2, inst, 1e3)
    for u, w in ((a, b), (a, c)):
        assert u[2] == w[2]
        for i in (0, 1, 3, 4):
            assert u[i].tobytes() == w[i].tobytes()


@pytest.mark.parametrize("where", ["d", "b", "A"])
def test_nan_input_never_gives_a_finite_step(where):
    """a NaN in d, b or A: K or its right-hand side is not finite -- the Cholesky fails (linalg_error ->
    LinAlgError from the Newton class, no fallback) or the step is non-finite; never a finite step"""
    import ipm355
    inst = Q.instance(65, 17, 64, "both", 0.0)
    data = {"d": inst.d.copy(), "b": inst.b.copy(), "A": inst.A.copy()}
    data[where].flat[7] = np.nan
    fm = ipm355.FunctionManagerLP(c=inst.c, A=data["A"], b=data["b"], C=inst.C, d=data["d"], x0=inst.x.copy(),
                                  lower_bound=inst.lb, upper_bound=inst.ub, t=1, try_diag=False,
                                  solve_method=ipm355._lib.SOLVE_CHOLESKY_DUAL_EQ)
    fm.update_t(1.0)
    ns = ipm355.NewtonSolverCholeskyDualInfeasibleStart(data["A"], data["b"], inst.C, data["d"], fm, max_iters=1,
                                                        epsilon=1e-5, alpha=ALPHA, beta=BETA)
    x, v = inst.x.copy(), inst.v.copy()
    try:
        ns.solve(x, 1.0, v0=v)
    except np.linalg.LinAlgError:
        assert ns.last_result.linalg_error == 1 and not ns.last_result.use_backup
        assert fm.prob.use_backup is False
        return
    assert not (np.all(np.isfinite(x)) and np.all(np.isfinite(v)))


def test_no_hessian_to_hand_out():
    from ipm355 import IPMBackendError
    from ipm355 import _lib as L
    fm = Q.instance(17, 3, 15, "both", 0.0).device(L.SOLVE_CHOLESKY_DUAL_EQ)
    with pytest.raises(IPMBackendError, match=NOT_SUPPORTED + ".*IPM_SOLVE_CHOLESKY_DUAL_EQ"):
        fm.hessian()
    assert np.all(np.isfinite(fm.gradient()))      # the rest of the protocol is untouched


def test_dual_direction_needs_equality_rows():
    from ipm355 import IPMBackendError
    from ipm355 import _lib as L
    inst = Q.instance(17, 3, 15, "both", 0.0)
    fm = inst.base.device(L.SOLVE_CHOLESKY)          # the same LP without A
    with pytest.raises(IPMBackendError, match="ipm355 error 2"):
        fm.prob.last_dual_direction()


def test_unsupported_problems_are_rejected_at_create():
    from ipm355 import IPMBackendError
    from ipm355 import _lib as L
    from ipm355.device import DeviceProblem
    inst = Q.instance(17, 3, 15, "both", 0.0)
    n = inst.n
    base = dict(solve_method=L.SOLVE_CHOLESKY_DUAL_EQ, c=inst.c, C=inst.C, d=inst.d, lb=inst.lb, ub=inst.ub,
                A=inst.A, b=inst.b)
    DeviceProblem("LP", n, **base)                                            # the supported form
    DeviceProblem("LP", n, **dict(base, ub=None))                             # a single bound is fine
    bad = {
        "QP": lambda: DeviceProblem("QP", n, **dict(base, c=None, P=np.eye(n), q=inst.c)),
        "phase 1": lambda: DeviceProblem("LP", n, phase1=True, **dict(base, c=None)),
        "p = 0": lambda: DeviceProblem("LP", n, **dict(base, A=None, b=None)),
        "m = 0": lambda: DeviceProblem("LP", n, **dict(base, C=None, d=None)),
        "no bound": lambda: DeviceProblem("LP", n, **dict(base, lb=None, ub=None)),
    }
    for why, make in bad.items():
        with pytest.raises(IPMBackendError, match=NOT_SUPPORTED + ".*IPM_SOLVE_CHOLESKY_DUAL_EQ"):
            make()
    # methods 6 and 7 keep refusing equality rows
    for meth, ph1 in ((L.SOLVE_CHOLESKY_DUAL, False), (L.SOLVE_CHOLESKY_DUAL_PHASE1, True)):
        with pytest.raises(IPMBackendError, match=NOT_SUPPORTED + ".*equality"):
            DeviceProblem("LP", n, phase1=ph1, **dict(base, solve_method=meth, c=None if ph1 else inst.c))
