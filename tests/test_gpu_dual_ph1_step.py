"""-m gpu: one Newton step of IPM_SOLVE_CHOLESKY_DUAL_PHASE1 (the dual-form phase-1 step) through
ipm_newton_solve (max_iters = 1) on LP phase-1 device problems.

The direction d = (dx, ds) the linear solve left (ipm_fm_last_direction) is compared with the long-double
solve of H~ d = -g within the project's Newton-step allowance

    B1 = 64 eps cond2(H~) ||d||_2

and the iterate must be x~ + step d bit for bit.  d is also recovered from the iterate and the accepted
step size, (x~_after - x~) / step; that quotient carries the rounding of x~_after = fl(x~ + step d), up to
eps |x~_after| / step per entry -- 245 x B1 at n33-m31-both-t1000-f0-d0.001, where the line search accepts
step = 8.1e-14, for an EXACT d -- so the recovered d is held to B1 + eps ||x~_after|| / step, the solve's
own d to B1 alone.  The grid is that of tests/dual_ph1_ref.py:
11 shapes, three bound sets, t in {0.01, 1, 1e3}, a feasible and an infeasible x, and s at 1 and at 1e-3
from the boundary of the phase-1 domain.  tests/test_dual_ph1_ref.py (no GPU) holds the fp64 restatement
of the step to B1 / 4 on the same states.
"""
import numpy as np
import pytest

import dual_ph1_ref as P

pytestmark = pytest.mark.gpu
ALPHA, BETA = 0.2, 0.6
NOT_SUPPORTED = "ipm355 error 4"
EPS = np.finfo(np.float64).eps


def _solver(fm, **kw):
    import ipm355
    from ipm355 import _lib as L
    dual = fm.prob.desc.solve_method == L.SOLVE_CHOLESKY_DUAL_PHASE1
    cls = ipm355.NewtonSolverCholeskyDual if dual else ipm355.NewtonSolverCholesky
    kw.setdefault("phase1_flag", False)
    return cls(function_manager=fm, max_iters=1, epsilon=1e-5, alpha=ALPHA, beta=BETA, **kw)


def _step(fm, pt, t, **kw):
    """one Newton step from the point -> (the solve's direction, step size, x~ after the step, solver)"""
    fm.update_t(t)
    ns = _solver(fm, **kw)
    x = pt.x.copy()
    _, _, iters, _, _ = ns.solve(x, t)
    assert iters == 1
    return fm.prob.last_direction().cpu().numpy(), ns.trace[0][0], x, ns


GROUPS = [(n, m, b) for (n, m) in P.SHAPES for b in P.BOUNDS]


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"n{g[0]}-m{g[1]}-{g[2]}")
def test_direction_within_bound_and_step_size(group):
    """every (t, x, s) of one (shape, bounds): the device problems are created once per group (their data
    does not depend on the point).  The accepted step size must equal the Cholesky phase-1 problem's on the
    same state -- and the oracle's -- wherever each of the oracle's line-search decisions is at least 1e-9
    from flipping."""
    from ipm355 import _lib as L
    n, m, b = group
    worst, worst_rec, compared, total = 0.0, 0.0, 0, 0
    pt0 = P.point(n, m, b, P.FRACS[0], P.DELTAS[0])
    fm_dual = pt0.device(L.SOLVE_CHOLESKY_DUAL_PHASE1)
    fm_chol = pt0.device(L.SOLVE_CHOLESKY)
    for frac in P.FRACS:
        for delta in P.DELTAS:
            pt = P.point(n, m, b, frac, delta)
            for t in P.TS:
                state = (n, m, b, t, frac, delta)
                total += 1
                ref = P.reference_step(state)
                d_solve, step, x, ns = _step(fm_dual, pt, t)
                assert fm_dual.prob.use_backup is False and not ns.last_result.linalg_error
                assert np.all(np.isfinite(d_solve)) and np.all(np.isfinite(x)) and step > 0
                np.testing.assert_array_equal(x, pt.x + step * d_solve)
                # d recovered from the iterate and the accepted step size.  Its allowance is B1 plus the rounding
                # of the recovery itself: x = fl(x~ + step d) is off by up to eps |x| / 2 per entry, and the
                # quotient (x - x~) / step magnifies that by 1 / step (step = 8.1e-14 at n33-m31-both-t1000-f0-
                # d0.001: 245 B1 for an exact d).  The check that carries the weight is the pair above and
                # below: the solve's own direction within B1 alone, and x == x~ + step d bit for bit
                d = (x - pt.x) / step
                recov = EPS * float(np.linalg.norm(x)) / step
                r_solve = float(np.linalg.norm(d_solve - ref["d"]) / ref["bound"])
                r = float(np.linalg.norm(d - ref["d"]) / (ref["bound"] + recov))
                worst, worst_rec = max(worst, r_solve), max(worst_rec, r)
                assert r_solve <= 1.0 and r <= 1.0, (P.state_id(state), r_solve, r)
                ls = P.oracle_line_search(state, ALPHA, BETA)
                if ls["decisive"]:
                    _, step_c, _, _ = _step(fm_chol, pt, t)
                    compared += 1
                    assert step == step_c == ls["step"], (P.state_id(state), step, step_c, ls["step"])
    print(f"[n{n} m{m} {b}] worst |d - d_ref| / B1 {worst:.3g} (recovered from the iterate: {worst_rec:.3g} of its "
          f"allowance); step size compared on {compared} of {total} states")


SAME_H = [(17, 15, "both", 1.0, 1.5, 1.0), (65, 64, "lb", 1e3, 1.5, 1e-3), (257, 129, "ub", 0.01, 0.0, 1.0)]


@pytest.mark.parametrize("state", SAME_H, ids=P.state_id)
def test_psd_condition_and_stale_slack_options(state):
    """use_psd_condition = 1: 1e-9 on all n + 1 diagonal entries of H~ (on D and on hss), the reference
    with the same add; update_slacks_every = 2 changes the line search, not the step's system"""
    from ipm355 import _lib as L
    n, m, b, t, frac, delta = state
    pt = P.point(n, m, b, frac, delta)
    fm = pt.device(L.SOLVE_CHOLESKY_DUAL_PHASE1)
    for kw, add in ((dict(use_psd_condition=True), 1e-9), (dict(update_slacks_every=2), 0.0)):
        ref = P.reference_step(state, add)
        d, _, _, _ = _step(fm, pt, t, **kw)
        r = float(np.linalg.norm(d - ref["d"]) / ref["bound"])
        print(f"[{P.state_id(state)}] {kw}: |d - d_ref| / B1 {r:.3g}")
        assert r <= 1.0, (kw, r)
    plain, psd = P.reference_step(state, 0.0)["d"], P.reference_step(state, 1e-9)["d"]
    assert np.linalg.norm(plain - psd) > 0


@pytest.mark.parametrize("shape", [(17, 15), (129, 128), (520, 257)], ids=lambda s: f"n{s[0]}-m{s[1]}")
def test_repeat_step_is_bitwise_equal(shape):
    """fixed-order reductions, no atomics: the same problem twice and a second problem give the same bits"""
    from ipm355 import _lib as L
    n, m = shape
    pt = P.point(n, m, "both", 1.5, 1.0)
    fm = pt.device(L.SOLVE_CHOLESKY_DUAL_PHASE1)
    a = _step(fm, pt, 1.0)
    b = _step(fm, pt, 1.0)
    c = _step(pt.device(L.SOLVE_CHOLESKY_DUAL_PHASE1), pt, 1.0)
    for u, v in ((a, b), (a, c)):
        assert u[0].tobytes() == v[0].tobytes() and u[1] == v[1] and u[2].tobytes() == v[2].tobytes()


def test_phase1_flag_early_exit():
    """a state whose first step crosses s < -phase1_tol: iters = 1, success = 1 (the shared early exit)"""
    from ipm355 import _lib as L
    pt = P.point(17, 15, "both", 0.0, 1.0)          # x feasible: s = 1 - min(slacks) and the step drives it down
    fm = pt.device(L.SOLVE_CHOLESKY_DUAL_PHASE1)
    tol = 0.0
    for t in (1e3, 1.0):
        fm.update_t(t)
        ns = _solver(fm, phase1_flag=True, phase1_tol=tol)
        ns.max_iters = 50
        x = pt.x.copy()
        _, _, iters, stat, ok = ns.solve(x, t)
        if iters == 1 and x[-1] < -tol:
            break
    print(f"early exit at t = {t}: s {pt.x[-1]:.3g} -> {x[-1]:.3g}, iters {iters}")
    assert iters == 1 and ok and x[-1] < -tol and stat is None
    # without the flag the same solve goes on
    ns = _solver(fm, phase1_flag=False)
    ns.max_iters = 50
    x2 = pt.x.copy()
    _, _, iters2, _, _ = ns.solve(x2, t)
    assert iters2 > 1


@pytest.mark.parametrize("where", ["C", "d", "x"])
def test_nan_input_never_gives_a_finite_step(where):
    """a NaN in C, d or x: LinAlgError from the Newton class (linalg_error = 1, no backup) or a non-finite
    iterate; never a finite one"""
    import ipm355
    from ipm355 import _lib as L
    pt = P.point(65, 64, "both", 1.5, 1.0)
    C, d, x = pt.C.copy(), pt.d.copy(), pt.x.copy()
    if where == "C":
        C[7, 11] = np.nan
    elif where == "d":
        d[7] = np.nan
    fm = ipm355.FunctionManagerPhase1(C=C, d=d, x0=pt.inst.x.copy(), lower_bound=pt.lb, upper_bound=pt.ub, t=1,
                                      solve_method=L.SOLVE_CHOLESKY_DUAL_PHASE1)
    if where == "x":
        x[3] = np.nan
    fm.update_x(x.copy())
    fm.update_t(1.0)
    ns = _solver(fm)
    try:
        ns.solve(x, 1.0)
    except np.linalg.LinAlgError:
        assert ns.last_result.linalg_error == 1 and not ns.last_result.use_backup
        return
    assert not np.all(np.isfinite(x))


def test_no_hessian_to_hand_out():
    from ipm355 import IPMBackendError
    from ipm355 import _lib as L
    fm = P.point(17, 15, "both", 1.5, 1.0).device(L.SOLVE_CHOLESKY_DUAL_PHASE1)
    with pytest.raises(IPMBackendError, match=NOT_SUPPORTED + ".*IPM_SOLVE_CHOLESKY_DUAL_PHASE1"):
        fm.hessian()
    assert np.all(np.isfinite(fm.gradient()))      # the rest of the protocol is untouched


def test_unsupported_problems_are_rejected_at_create():
    from ipm355 import IPMBackendError
    from ipm355 import _lib as L
    from ipm355.device import ConeData, DeviceProblem
    import torch
    pt = P.point(17, 15, "both", 0.0, 1.0)
    n = pt.n
    base = dict(solve_method=L.SOLVE_CHOLESKY_DUAL_PHASE1, phase1=True, C=pt.C, d=pt.d, lb=pt.lb, ub=pt.ub)
    DeviceProblem("LP", n, **base)                                            # the supported form
    DeviceProblem("LP", n, **dict(base, ub=None))                             # a single bound is fine
    A, bb = np.ones((2, n)), np.zeros(2)
    rng = np.random.default_rng(0)
    cones = ConeData([rng.normal(size=(3, n))], [rng.normal(size=3)], [rng.normal(size=n)], [1.0], n,
                     torch.device("cuda", 0))
    bad = {
        "phase 1 only": lambda: DeviceProblem("LP", n, **dict(base, phase1=False, c=np.ones(n))),
        "equality rows": lambda: DeviceProblem("LP", n, A=A, b=bb, **base),
        "needs inequality rows": lambda: DeviceProblem("LP", n, **dict(base, C=None, d=None)),
        "needs a lower or an upper bound": lambda: DeviceProblem("LP", n, **dict(base, lb=None, ub=None)),
        "LP phase 1 only": lambda: DeviceProblem("SOCP", n, cones=cones, **base),
    }
    for why, make in bad.items():
        with pytest.raises(IPMBackendError, match=NOT_SUPPORTED + ".*IPM_SOLVE_CHOLESKY_DUAL_PHASE1.*" + why):
            make()
    # and method 6 still refuses phase 1
    with pytest.raises(IPMBackendError, match=NOT_SUPPORTED + ".*IPM_SOLVE_CHOLESKY_DUAL: no phase 1"):
        DeviceProblem("LP", n, **dict(base, solve_method=L.SOLVE_CHOLESKY_DUAL))
