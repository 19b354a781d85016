"""-m gpu: one Newton step of IPM_SOLVE_CHOLESKY_DUAL_QP_EQ (a QP with the factored P = diag(rho) + F^T F and
equality rows A x = b) through ipm_newton_solve (max_iters = 1).

The device directions (ipm_fm_last_direction / ipm_fm_last_dual_direction: what the linear solve left, before the
step size) are compared as [dx; v + dv] with the long-double solve of the KKT system
[[H, A^T], [A, 0]] [dx; nu] = [-g; -(A x - b)], H formed in long double from F, rho and C, within

    B = 64 eps cond2(KKT) ||[dx; nu]||_2

over the grid of tests/dual_qp_eq_ref.py (10 shapes: each block empty, inside, at and across a 64-row tile of the
stacked operand, a tile straddling both seams, the K split of the assembly; three bound sets; four kinds of rho;
t in {1, 1e3, 1e6}; points 0, 0.9 and 0.999 of the way to the boundary; x off A x = b).
tests/test_dual_qp_eq_ref.py (no GPU) holds the fp64 restatement of the step to B / 4 on the same states.
"""
import numpy as np
import pytest

import dual_qp_eq_ref as R

pytestmark = pytest.mark.gpu
ALPHA, BETA = 0.2, 0.6
NOT_SUPPORTED = "ipm355 error 4"


def _solver(fm, inst, **kw):
    import ipm355
    from ipm355 import _lib as L
    dual = fm.prob.desc.solve_method == L.SOLVE_CHOLESKY_DUAL_QP_EQ
    cls = ipm355.newton.NewtonSolverCholeskyDualQPInfeasibleStart if dual else ipm355.NewtonSolverCholeskyInfeasibleStart
    return cls(inst.A, inst.b, inst.C, inst.d, fm, max_iters=1, epsilon=1e-5, alpha=ALPHA, beta=BETA, **kw)


def _step(fm, inst, t, **kw):
    """one Newton step from the instance's point and dual -> (dx, dv, step size, x after, v after)"""
    fm.update_t(t)
    ns = _solver(fm, inst, **kw)
    x, v = inst.x.copy(), inst.v.copy()
    _, _, iters, _, _ = ns.solve(x, t, v0=v)
    assert iters == 1
    return (fm.prob.last_direction().cpu().numpy(), fm.prob.last_dual_direction().cpu().numpy(), ns.trace[0][0], x, v)


GROUPS = [(n, m, k, p, b) for (n, m, k, p) in R.SHAPES for b in R.BOUNDS]


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "n%d-m%d-k%d-p%d-%s" % g)
def test_direction_within_bound_and_step_size(group):
    """every (rho, t, point) of one (shape, bounds): the device problems are created once per (rho, point).  The
    accepted step size must equal the dense Cholesky problem's on the same state -- and the oracle's -- wherever
    each of the oracle's line-search decisions is at least 1e-9 from flipping."""
    n, m, k, p, b = group
    worst, compared, total = 0.0, 0, 0
    for rho in R.Q.rhos_for(b):
        for frac in R.FRACS:
            inst = R.instance(n, m, k, p, b, rho, frac)
            fm_dual, fm_chol = inst.device(True), None
            for t in R.TS:
                state = (n, m, k, p, b, rho, t, frac)
                ref = R.reference_step(state)
                dx, dv, step, x, v = _step(fm_dual, inst, t)
                total += 1
                assert fm_dual.prob.use_backup is False
                assert np.all(np.isfinite(dx)) and np.all(np.isfinite(dv)) and np.all(np.isfinite(x))
                r = R.joint_error(dx, dv, ref)
                worst = max(worst, r)
                assert r <= 1.0, (R.state_id(state), r)
                np.testing.assert_array_equal(x, inst.x + step * dx)
                np.testing.assert_array_equal(v, inst.v + step * dv)
                ls = R.oracle_line_search(state, ALPHA, BETA)
                if ls["decisive"]:
                    fm_chol = fm_chol or inst.device(False)
                    _, _, step_c, _, _ = _step(fm_chol, inst, t)
                    compared += 1
                    assert step == step_c == ls["step"], (R.state_id(state), step, step_c, ls)
    print(f"[n{n} m{m} k{k} p{p} {b}] worst |[dx; nu] - ref| / B {worst:.3g}; step size compared on {compared} of "
          f"{total} states")


SAME_H = [(17, 3, 5, 2, "both", "ones", 1e3, 0.9), (130, 63, 2, 30, "lb", "half0", 1e3, 0.9),
          (257, 129, 65, 33, "none", "log", 1e6, 0.999)]


@pytest.mark.parametrize("state", SAME_H, ids=R.state_id)
def test_psd_condition_and_stale_slack_options(state):
    """use_psd_condition = 1: 1e-9 on D only (the reference with the same add on H's diagonal: the same system);
    update_slacks_every > 0 changes the line search, not the system of the step: the plain reference"""
    n, m, k, p, b, rho, t, frac = state
    inst = R.instance(n, m, k, p, b, rho, frac)
    fm = inst.device(True)
    for kw, add in ((dict(use_psd_condition=True), 1e-9), (dict(update_slacks_every=2), 0.0)):
        ref = R.reference_step(state, add)
        dx, dv, _, _, _ = _step(fm, inst, t, **kw)
        r = R.joint_error(dx, dv, ref)
        print(f"[{R.state_id(state)}] {kw}: |[dx; nu] - ref| / B {r:.3g}")
        assert r <= 1.0, (kw, r)
    plain, psd = R.reference_step(state, 0.0)["sol"], R.reference_step(state, 1e-9)["sol"]
    assert np.linalg.norm(plain - psd) > 0


@pytest.mark.parametrize("shape", [(17, 3, 5, 2), (130, 63, 2, 30), (520, 127, 130, 65)],
                         ids=lambda s: "n%d-m%d-k%d-p%d" % s)
def test_repeat_step_is_bitwise_equal(shape):
    inst = R.instance(*shape, "both", "log", 0.9)
    fm = inst.device(True)
    a = _step(fm, inst, 1e3)
    b = _step(fm, inst, 1e3)
    c = _step(inst.device(True), inst, 1e3)
    for u, w in ((a, b), (a, c)):
        assert u[2] == w[2]
        for i in (0, 1, 3, 4):
            assert u[i].tobytes() == w[i].tobytes()


@pytest.mark.parametrize("where", ["F", "rho", "A", "b", "d"])
def test_nan_input_never_gives_a_finite_step(where):
    """a NaN in F, rho, A, b or d: K or its right-hand side is not finite -- the Cholesky fails (linalg_error ->
    LinAlgError from the Newton class, no fallback) or the step is non-finite; never a finite step"""
    import ipm355
    inst = R.instance(65, 64, 1, 1, "both", "ones", 0.0)
    data = {"F": inst.F.copy(), "rho": inst.rho.copy(), "A": inst.A.copy(), "b": inst.b.copy(), "d": inst.d.copy()}
    data[where].flat[0 if where == "b" else 7] = np.nan
    fm = ipm355.FunctionManagerQP(P_factor=data["F"], P_diag=data["rho"], q=inst.q, A=data["A"], b=data["b"], C=inst.C,
                                  d=data["d"], x0=inst.x.copy(), lower_bound=inst.lb, upper_bound=inst.ub, t=1)
    assert fm.prob.desc.solve_method == ipm355._lib.SOLVE_CHOLESKY_DUAL_QP_EQ
    fm.update_t(1.0)
    ns = ipm355.newton.NewtonSolverCholeskyDualQPInfeasibleStart(data["A"], data["b"], inst.C, data["d"], fm,
                                                                 max_iters=1, epsilon=1e-5, alpha=ALPHA, beta=BETA)
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
    fm = R.instance(17, 3, 5, 2, "both", "ones", 0.0).device(True)
    with pytest.raises(IPMBackendError, match=NOT_SUPPORTED + ".*IPM_SOLVE_CHOLESKY_DUAL_QP_EQ"):
        fm.hessian()
    assert np.all(np.isfinite(fm.gradient()))      # the rest of the protocol is untouched


def test_unsupported_problems_are_rejected_at_create():
    from ipm355 import IPMBackendError
    from ipm355 import _lib as L
    from ipm355.device import DeviceProblem
    inst = R.instance(17, 3, 5, 2, "both", "ones", 0.0)
    n = inst.n
    base = dict(solve_method=L.SOLVE_CHOLESKY_DUAL_QP_EQ, q=inst.q, C=inst.C, d=inst.d, lb=inst.lb, ub=inst.ub,
                P_factor=inst.F, P_diag=inst.rho, A=inst.A, b=inst.b)
    DeviceProblem("QP", n, **base)                                                        # the supported form
    DeviceProblem("QP", n, **dict(base, ub=None, P_diag=None))                            # one bound, no rho
    DeviceProblem("QP", n, **dict(base, lb=None, ub=None))                                # rho in place of a bound
    DeviceProblem("QP", n, **dict(base, C=None, d=None))                                  # m = 0
    DeviceProblem("QP", n, **dict(base, P_factor=None))                                   # kf = 0
    bad = {
        "QP only": lambda: DeviceProblem("LP", n, c=inst.q, **dict(base, q=None)),
        "no phase 1": lambda: DeviceProblem("QP", n, phase1=True, **base),
        "needs equality rows": lambda: DeviceProblem("QP", n, **dict(base, A=None, b=None)),
        "P must be NULL": lambda: DeviceProblem("QP", n, P=np.eye(n), **base),
        r"m \+ kf > 0": lambda: DeviceProblem("QP", n, **dict(base, C=None, d=None, P_factor=None)),
        "bound, or Pdiag": lambda: DeviceProblem("QP", n, **dict(base, lb=None, ub=None, P_diag=None)),
    }
    for why, make in bad.items():
        with pytest.raises(IPMBackendError, match=NOT_SUPPORTED + ": IPM_SOLVE_CHOLESKY_DUAL_QP_EQ: .*" + why):
            make()
    # method 9 keeps refusing equality rows in its own words
    with pytest.raises(IPMBackendError, match=NOT_SUPPORTED + ": IPM_SOLVE_CHOLESKY_DUAL_QP: .*no equality rows"):
        DeviceProblem("QP", n, **dict(base, solve_method=L.SOLVE_CHOLESKY_DUAL_QP))


def test_other_methods_give_the_same_bits_before_and_after():
    """a dense 'cholesky' QP step, a method-8 LP step and a method-9 QP step, each taken before and after a
    method-10 step in one process: the same bits"""
    import dual_eq_ref as E8
    import test_gpu_dual_eq_step as T8
    import test_gpu_dual_qp_step as T9
    from ipm355 import _lib as L
    inst = R.instance(130, 63, 2, 30, "both", "log", 0.9)
    i8 = E8.instance(130, 30, 97, "both", 0.9)
    i9 = R.Q.instance(130, 97, 31, "both", "log", 0.9)

    def others():
        out = list(_step(inst.device(False), inst, 1e3))
        out += list(T8._step(i8.device(L.SOLVE_CHOLESKY_DUAL_EQ), i8, 1e3))
        out += [np.asarray(a) for a in T9._step(i9.device(True), i9, 1e3)]
        return out
    before = others()
    _step(inst.device(True), inst, 1e3)
    after = others()
    assert len(before) == len(after)
    for u, w in zip(before, after):
        assert np.asarray(u).tobytes() == np.asarray(w).tobytes()
