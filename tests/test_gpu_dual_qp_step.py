"""-m gpu: one Newton step of IPM_SOLVE_CHOLESKY_DUAL_QP (a QP with the factored P = diag(rho) + F^T F) through
ipm_newton_solve (max_iters = 1).

The device direction dx (ipm_fm_last_direction) is compared with the long-double solve of H dx = -g, H formed in
long double from F, rho and C, within

    B = 64 eps ( cond2(H) ||dx||_2 + || E o (|g| + |M|^T |z|) ||_2 ),   M = [C; F], z = W o (M dx)

over the grid of tests/dual_qp_ref.py (12 shapes x bound sets x rho kinds x t x points: 1080 states);
tests/test_dual_qp_ref.py (no GPU) holds the fp64 restatement of the step to B / 4 on the same states.  The
accepted step size must equal the dense 'cholesky' QP problem's (P formed on the host) and the oracle's wherever
the oracle's own decisions are at least 1e-9 from flipping, and the new iterate is x + step dx bit for bit.
"""
import types

import numpy as np
import pytest

import barrier_ref as BR
import dual_qp_ref as Q

pytestmark = pytest.mark.gpu
ALPHA, BETA = 0.2, 0.6
NOT_SUPPORTED = "ipm355 error 4"


def _solver(fm, **kw):
    import ipm355
    from ipm355 import _lib as L
    dual = fm.prob.desc.solve_method == L.SOLVE_CHOLESKY_DUAL_QP
    cls = ipm355.NewtonSolverCholeskyDualQP if dual else ipm355.NewtonSolverCholesky
    return cls(function_manager=fm, max_iters=1, epsilon=1e-5, alpha=ALPHA, beta=BETA, **kw)


def _step(fm, inst, t, **kw):
    """one Newton step from the instance's point -> (dx, step size, x after the step)"""
    fm.update_t(t)
    ns = _solver(fm, **kw)
    x = inst.x.copy()
    _, _, iters, _, _ = ns.solve(x, t)
    assert iters == 1
    return fm.prob.last_direction().cpu().numpy(), ns.trace[0][0], x


@pytest.mark.parametrize("group", Q.groups(), ids=lambda g: "n%d-m%d-k%d-%s-%s" % g)
def test_direction_within_bound_and_step_size(group):
    """every (t, point) of one (shape, bounds, rho): the device problems are created once per point"""
    n, m, k, b, r = group
    worst, compared = 0.0, 0
    for frac in Q.FRACS:
        inst = Q.instance(n, m, k, b, r, frac)
        fm_dual = inst.device(True)
        fm_chol = inst.device(False)
        assert fm_dual.prob.P is None and int(fm_dual.prob.desc.kf) == k
        for t in Q.TS:
            state = (n, m, k, b, r, t, frac)
            ref = Q.reference_step(state)
            dx, step, x = _step(fm_dual, inst, t)
            assert fm_dual.prob.use_backup is False
            assert np.all(np.isfinite(dx)) and np.all(np.isfinite(x))
            e = float(np.linalg.norm(dx - ref["dx"]) / ref["bound"])
            worst = max(worst, e)
            assert e <= 1.0, (Q.state_id(state), e)
            np.testing.assert_array_equal(x, inst.x + step * dx)
            ls = Q.oracle_line_search(state, ALPHA, BETA)
            if ls["decisive"]:
                _, step_c, _ = _step(fm_chol, inst, t)
                compared += 1
                assert step == step_c == ls["step"], (Q.state_id(state), step, step_c, ls)
    print(f"[{group}] worst |dx - dx_ref| / B {worst:.3g}; step size compared on {compared} of 9 states")


PROTOCOL = [g for g in Q.groups() if g[1] > 0 or g[3] != "none"]


@pytest.mark.parametrize("group", PROTOCOL, ids=lambda g: "n%d-m%d-k%d-%s-%s" % g)
def test_protocol_values_within_the_dense_managers_bounds(group):
    """objective, gradient and slacks through ipm_fm_* (P applied through its factors) against the long-double
    values of the dense QP, at the entry-wise bounds tests/barrier_ref.py holds the dense QP manager to"""
    n, m, k, b, r = group
    inst = Q.instance(n, m, k, b, r, 0.9)
    shim = types.SimpleNamespace(kind="qp", n=n, m=m, t=1e3, C=inst.C, d=inst.d, lb=inst.lb, ub=inst.ub,
                                 P=inst.dense_P(), q=inst.q)
    ref = BR.lpqp_reference(shim, inst.x, want_hessian=False)
    fm = inst.device(True)
    fm.update_x(inst.x.copy())
    fm.update_t(1e3)
    got = {"slacks": BR.ratio(fm.slacks, ref["slacks"], ref["b_slacks"]),
           "nobj": BR.ratio(fm.newton_objective(), ref["nobj"], ref["b_nobj"]),
           "grad": BR.ratio(fm.gradient(), ref["grad"], ref["b_grad"])}
    f_ld = (ref["nobj"] + np.log(ref["slacks"] + BR.LD(BR.O.EPS_LOG)).sum()) / BR.LD(1e3)
    got["obj"] = BR.ratio(fm.objective(), f_ld, ref["b_nobj"] / 1e3)
    print(f"[{group}] err / bound {got}")
    assert BR.all_within(got, 1.0), got


SAME_H = [(33, 31, 33, "both", "log", 1e3, 0.9), (130, 97, 31, "lb", "half0", 1e3, 0.9),
          (300, 40, 20, "none", "ones", 1.0, 0.999), (520, 127, 130, "both", "absent", 1e6, 0.9)]


@pytest.mark.parametrize("state", SAME_H, ids=Q.state_id)
def test_psd_condition_and_stale_slack_options(state):
    """use_psd_condition = 1: 1e-9 on D only (the reference with the same add); update_slacks_every > 0 changes
    the line search, not the Hessian of the step: the plain reference"""
    n, m, k, b, r, t, frac = state
    inst = Q.instance(n, m, k, b, r, frac)
    fm = inst.device(True)
    for kw, add in ((dict(use_psd_condition=True), 1e-9), (dict(update_slacks_every=2), 0.0)):
        ref = Q.reference_step(state, add)
        dx, _, _ = _step(fm, inst, t, **kw)
        e = float(np.linalg.norm(dx - ref["dx"]) / ref["bound"])
        print(f"[{Q.state_id(state)}] {kw}: |dx - dx_ref| / B {e:.3g}")
        assert e <= 1.0, (kw, e)
    plain, psd = Q.reference_step(state, 0.0)["dx"], Q.reference_step(state, 1e-9)["dx"]
    assert np.linalg.norm(plain - psd) > 0


@pytest.mark.parametrize("shape", [(17, 5, 3), (65, 64, 64), (520, 127, 130)], ids=lambda s: "n%d-m%d-k%d" % s)
def test_repeat_step_is_bitwise_equal(shape):
    n, m, k = shape
    inst = Q.instance(n, m, k, "both", "log", 0.9)
    fm = inst.device(True)
    a = _step(fm, inst, 1e3)
    b = _step(fm, inst, 1e3)
    c = _step(inst.device(True), inst, 1e3)
    # a step at another t in between refills the stacked weights' tail: the first t again gives the first bits
    _step(fm, inst, 1.0)
    d = _step(fm, inst, 1e3)
    for u, v in ((a, b), (a, c), (a, d)):
        assert u[0].tobytes() == v[0].tobytes() and u[1] == v[1] and u[2].tobytes() == v[2].tobytes()


@pytest.mark.parametrize("where", ["F", "rho"])
def test_nan_input_never_gives_a_finite_step(where):
    import ipm355
    inst = Q.instance(65, 64, 64, "both", "log", 0.0)
    F, rho = inst.F.copy(), inst.rho.copy()
    if where == "F":
        F[7, 11] = np.nan
    else:
        rho[11] = np.nan
    fm = ipm355.FunctionManagerQP(P_factor=F, P_diag=rho, q=inst.q, C=inst.C, d=inst.d, x0=inst.x.copy(),
                                  lower_bound=inst.lb, upper_bound=inst.ub, t=1)
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
    fm = Q.instance(17, 5, 3, "both", "ones", 0.0).device(True)
    with pytest.raises(IPMBackendError, match=NOT_SUPPORTED + ".*IPM_SOLVE_CHOLESKY_DUAL_QP"):
        fm.hessian()
    assert np.all(np.isfinite(fm.gradient()))


def test_unsupported_problems_are_rejected_at_create():
    from ipm355 import IPMBackendError
    from ipm355 import _lib as L
    from ipm355.device import DeviceProblem
    inst = Q.instance(17, 5, 3, "both", "ones", 0.0)
    n = inst.n
    base = dict(solve_method=L.SOLVE_CHOLESKY_DUAL_QP, q=inst.q, C=inst.C, d=inst.d, lb=inst.lb, ub=inst.ub,
                P_factor=inst.F, P_diag=inst.rho)
    DeviceProblem("QP", n, **base)                                                        # the supported form
    DeviceProblem("QP", n, **dict(base, ub=None, P_diag=None))                            # one bound, no rho
    DeviceProblem("QP", n, **dict(base, lb=None, ub=None))                                # rho in place of a bound
    DeviceProblem("QP", n, **dict(base, C=None, d=None))                                  # m = 0
    DeviceProblem("QP", n, **dict(base, P_factor=None))                                   # kf = 0
    A, bb = np.ones((2, n)), np.zeros(2)
    bad = {
        "QP only": lambda: DeviceProblem("LP", n, c=inst.q, **dict(base, q=None)),
        "no phase 1": lambda: DeviceProblem("QP", n, phase1=True, **base),
        "no equality rows": lambda: DeviceProblem("QP", n, A=A, b=bb, **base),
        "P must be NULL": lambda: DeviceProblem("QP", n, P=np.eye(n), **base),
        r"m \+ kf > 0": lambda: DeviceProblem("QP", n, **dict(base, C=None, d=None, P_factor=None)),
        "bound, or Pdiag": lambda: DeviceProblem("QP", n, **dict(base, lb=None, ub=None, P_diag=None)),
    }
    for why, make in bad.items():
        with pytest.raises(IPMBackendError, match=NOT_SUPPORTED + ": IPM_SOLVE_CHOLESKY_DUAL_QP: .*" + why):
            make()
