"""-m gpu: one Newton step of IPM_SOLVE_CHOLESKY_DUAL (linear_solve_method='cholesky_dual') through
ipm_newton_solve (max_iters = 1) on LP device problems.

The device direction dx (ipm_fm_last_direction: what the linear solve left, before the step size) is
compared with the long-double solve of H dx = -g within

    B = 64 eps ( cond2(H) ||dx||_2 + || E o (|g| + |C|^T |z|) ||_2 )

over the grid of tests/dual_ref.py: 11 shapes (m < n, m >= n, both sides of the 16-row MFMA block, the
64-row tile and the K split of the S assembly), three bound sets, t in {1, 1e3, 1e6} and points 0, 0.9
and 0.999 of the way to the boundary.  tests/test_dual_ref.py (no GPU) holds the fp64 restatement of
the step to B / 4 on the same states.
"""
import numpy as np
import pytest

import dual_ref as D

pytestmark = pytest.mark.gpu
ALPHA, BETA = 0.2, 0.6
NOT_SUPPORTED = "ipm355 error 4"


def _solver(fm, **kw):
    import ipm355
    from ipm355 import _lib as L
    dual = fm.prob.desc.solve_method == L.SOLVE_CHOLESKY_DUAL
    cls = ipm355.NewtonSolverCholeskyDual if dual else ipm355.NewtonSolverCholesky
    return cls(function_manager=fm, max_iters=1, epsilon=1e-5, alpha=ALPHA, beta=BETA, **kw)


def _step(fm, inst, t, **kw):
    """one Newton step from the instance's point -> (dx, step size, x after the step)"""
    fm.update_t(t)
    ns = _solver(fm, **kw)
    x = inst.x.copy()
    _, _, iters, _, _ = ns.solve(x, t)
    assert iters == 1
    return fm.prob.last_direction().cpu().numpy(), ns.trace[0][0], x


GROUPS = [(n, m, b) for (n, m) in D.SHAPES for b in D.BOUNDS]


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"n{g[0]}-m{g[1]}-{g[2]}")
def test_direction_within_bound_and_step_size(group):
    """every (t, point) of one (shape, bounds): the device problems are created once per point (their
    data does not depend on t).  The accepted step size must equal the Cholesky problem's on the same
    state -- and the oracle's -- wherever each of the oracle's line-search decisions is at least 1e-9
    from flipping."""
    from ipm355 import _lib as L
    n, m, b = group
    worst, compared = 0.0, 0
    for frac in D.FRACS:
        inst = D.instance(n, m, b, frac)
        fm_dual = inst.device(L.SOLVE_CHOLESKY_DUAL)
        fm_chol = inst.device(L.SOLVE_CHOLESKY)
        for t in D.TS:
            state = (n, m, b, t, frac)
            ref = D.reference_step(state)
            dx, step, x = _step(fm_dual, inst, t)
            assert fm_dual.prob.use_backup is False
            assert np.all(np.isfinite(dx)) and np.all(np.isfinite(x))
            r = float(np.linalg.norm(dx - ref["dx"]) / ref["bound"])
            worst = max(worst, r)
            assert r <= 1.0, (D.state_id(state), r)
            np.testing.assert_array_equal(x, inst.x + step * dx)
            ls = D.oracle_line_search(state, ALPHA, BETA)
            if ls["decisive"]:
                _, step_c, _ = _step(fm_chol, inst, t)
                compared += 1
                assert step == step_c == ls["step"], (D.state_id(state), step, step_c, ls)
    print(f"[n{n} m{m} {b}] worst |dx - dx_ref| / B {worst:.3g}; step size compared on {compared} of 9 states")


SAME_H = [(33, 31, "both", 1e3, 0.9), (130, 127, "lb", 1e3, 0.9), (300, 40, "ub", 1.0, 0.999),
          (520, 257, "both", 1e6, 0.9)]


@pytest.mark.parametrize("state", SAME_H, ids=D.state_id)
def test_psd_condition_and_stale_slack_options(state):
    """use_psd_condition = 1: the dual system is built from the primal SYRK's own vectors, 1e-9 on
    the diagonal included (the reference with the same add); update_slacks_every > 0 changes the
    line search, not the Hessian of the step's first evaluation: the plain reference"""
    from ipm355 import _lib as L
    n, m, b, t, frac = state
    inst = D.instance(n, m, b, frac)
    fm = inst.device(L.SOLVE_CHOLESKY_DUAL)
    for kw, add in ((dict(use_psd_condition=True), 1e-9), (dict(update_slacks_every=2), 0.0)):
        ref = D.reference_step(state, add)
        dx, _, _ = _step(fm, inst, t, **kw)
        r = float(np.linalg.norm(dx - ref["dx"]) / ref["bound"])
        print(f"[{D.state_id(state)}] {kw}: |dx - dx_ref| / B {r:.3g}")
        assert r <= 1.0, (kw, r)
    # (the two references are different vectors: the add is part of what is compared)
    plain, psd = D.reference_step(state, 0.0)["dx"], D.reference_step(state, 1e-9)["dx"]
    assert np.linalg.norm(plain - psd) > 0


@pytest.mark.parametrize("shape", [(17, 15), (129, 128), (520, 257)], ids=lambda s: f"n{s[0]}-m{s[1]}")
def test_repeat_step_is_bitwise_equal(shape):
    from ipm355 import _lib as L
    n, m = shape
    inst = D.instance(n, m, "both", 0.9)
    fm = inst.device(L.SOLVE_CHOLESKY_DUAL)
    a = _step(fm, inst, 1e3)
    b = _step(fm, inst, 1e3)
    fm2 = inst.device(L.SOLVE_CHOLESKY_DUAL)
    c = _step(fm2, inst, 1e3)
    for u, v in ((a, b), (a, c)):
        assert u[0].tobytes() == v[0].tobytes() and u[1] == v[1] and u[2].tobytes() == v[2].tobytes()


def test_nan_input_never_gives_a_finite_step():
    """a NaN in d: S is not finite, its Cholesky fails (linalg_error -> LinAlgError from the Newton
    class) or the step is non-finite; never a finite step"""
    import ipm355
    inst = D.instance(65, 64, "both", 0.0)
    d = inst.d.copy()
    d[7] = np.nan
    fm = ipm355.FunctionManagerLP(c=inst.c, C=inst.C, d=d, x0=inst.x.copy(), lower_bound=inst.lb,
                                  upper_bound=inst.ub, t=1, try_diag=False,
                                  solve_method=ipm355._lib.SOLVE_CHOLESKY_DUAL)
    fm.update_t(1.0)
    ns = _solver(fm)
    x = inst.x.copy()
    try:
        ns.solve(x, 1.0)
    except np.linalg.LinAlgError:
        assert ns.last_result.linalg_error == 1 and not ns.last_result.use_backup
        return
    assert not np.all(np.isfinite(x))


def test_no_hessian_to_hand_out():
    from ipm355 import IPMBackendError
    from ipm355 import _lib as L
    fm = D.instance(17, 15, "both", 0.0).device(L.SOLVE_CHOLESKY_DUAL)
    with pytest.raises(IPMBackendError, match=NOT_SUPPORTED):
        fm.hessian()
    assert np.all(np.isfinite(fm.gradient()))      # the rest of the protocol is untouched


def test_unsupported_problems_are_rejected_at_create():
    from ipm355 import IPMBackendError
    from ipm355 import _lib as L
    from ipm355.device import DeviceProblem
    inst = D.instance(17, 15, "both", 0.0)
    n = inst.n
    base = dict(solve_method=L.SOLVE_CHOLESKY_DUAL, c=inst.c, C=inst.C, d=inst.d, lb=inst.lb, ub=inst.ub)
    DeviceProblem("LP", n, **base)                                            # the supported form
    DeviceProblem("LP", n, **dict(base, ub=None))                             # a single bound is fine
    A, bb = np.ones((2, n)), np.zeros(2)
    bad = {
        "QP": lambda: DeviceProblem("QP", n, **dict(base, c=None, P=np.eye(n), q=inst.c)),
        "phase 1": lambda: DeviceProblem("LP", n, phase1=True, **dict(base, c=None)),
        "equality rows": lambda: DeviceProblem("LP", n, A=A, b=bb, **base),
        "m = 0": lambda: DeviceProblem("LP", n, **dict(base, C=None, d=None)),
        "no bound": lambda: DeviceProblem("LP", n, **dict(base, lb=None, ub=None)),
    }
    for why, make in bad.items():
        with pytest.raises(IPMBackendError, match=NOT_SUPPORTED + ".*IPM_SOLVE_CHOLESKY_DUAL"):
            make()
