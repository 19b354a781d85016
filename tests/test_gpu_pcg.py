"""-m gpu: cg_preconditioner='jacobi' -- ipm_pcg against the restatement tests/pcg_ref.py and against
ipm_cg, one preconditioned Newton step through the product, full solves against reference-run
fixtures (tests/golden/pcg_*.npz, make_golden_pcg.py), the facade's keyword.

Conventions and helpers of test_gpu_cg.py: H on the device with a NaN strict upper triangle and NaN
ld padding, x in front of a sentinel, each test prints its worst err / bound.  Without the feature
the level-0 and step tests fail on a missing symbol or keyword; test_plain_cg_misses_scaled_lp's
plain run is what the product computed before (the wrong optimum).
"""
import ctypes

import numpy as np
import pytest

import cg_ref
import pcg_ref
import test_gpu_cg as TC
from gpu_util import dev, handle, host

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
IPM_OK, IPM_INVALID_ARG = 0, 2
SENTINEL = TC.SENTINEL


def _pcg(n, Hd, ldh, minvd, bd, xd, maxiter, rtol=1e-5):
    from ipm355 import _lib as L
    h = handle()
    it, info = ctypes.c_int32(-7), ctypes.c_int32(-7)
    rc = h.lib.ipm_pcg(h.ptr, n, L.dptr(Hd), ldh, None if minvd is None else L.dptr(minvd), L.dptr(bd), L.dptr(xd),
                       maxiter, rtol, ctypes.byref(it), ctypes.byref(info))
    return rc, it.value, info.value


def _minv_dev(minv):
    """n entries in front of a NaN: nothing past n may be read"""
    return dev(np.append(minv, np.nan))[:len(minv)]


def _run(fn, n, x0, *args):
    """-> (x, iters, info); the sentinel behind x checked"""
    buf, xd = TC._xbuf(x0)
    rc, it, info = fn(n, *args[:-1], xd, args[-1])
    got = host(buf)
    assert rc == IPM_OK and got[n] == SENTINEL
    return got[:n], it, info


def _spd(n, seed):
    """A A^T / n + I in units spread over two decades, and a right-hand side"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    s = 10.0 ** rng.uniform(-1, 1, n)
    H = s[:, None] * (A @ A.T / n + np.eye(n)) * s[None, :]
    return (H + H.T) / 2, rng.standard_normal(n)


def _clustered_scaled(n):
    """the matrices of test_pcg_ref.py (d)"""
    K, _ = cg_ref.clustered(n, seed=n)
    b0 = np.random.default_rng(n + 1).standard_normal(n)
    return pcg_ref.scaled_system(K, b0, n + 3)[:2]


# ------------------------------------------------------------------ level 0: ipm_pcg
@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 257, 300])
def test_pcg_default_minv_is_the_diagonal(n):
    """k_cg_minv at the SYMV's tile edges, ldh = n, n + 3 and the next multiple of 16: minv = NULL
    (1 / diag(H) read from the lower triangle with its own ldh) and an explicit 1 / diag(H) give
    the same bits, twice; all finite although everything but the lower triangle is NaN."""
    H, b = _spd(n, seed=n)
    minv = 1.0 / np.diag(H)
    bd = dev(b)
    for ldh in (n, n + 3, (n // 16 + 1) * 16):
        Hd = TC._lower_dev(H, ldh)
        outs = [_run(_pcg, n, np.zeros(n), Hd, ldh, md, bd, 30) for md in (None, None, _minv_dev(minv), _minv_dev(minv))]
        x, it, info = outs[0]
        assert np.all(np.isfinite(x)), ("non-finite: upper triangle or padding read", ldh)
        assert 0 < it <= 30 and info in (0, 30)
        for o in outs[1:]:
            assert np.array_equal(o[0], x) and o[1:] == (it, info), ldh
        xr, infor, itr = pcg_ref.pcg(H, b, minv, maxiter=30)
        print(f"[pcg minv n={n} ldh={ldh}] iters {it} info {info} (restatement {itr} {infor}) "
              f"||x - x_ref|| / ||x_ref|| {np.linalg.norm(x - xr) / np.linalg.norm(xr):.3g}")


@pytest.mark.parametrize("n", [1, 129, 300, 1025])
def test_pcg_identity_equals_cg(n):
    """minv = ones: z = r, so the PRE kernels must give ipm_cg's bits, iteration count and info --
    a truncated run (maxiter 4) and one to convergence or the cap of 60.  n = 1025: the second trip
    of the single-workgroup kernels' 1024-stride loops."""
    H, b = _spd(n, seed=n + 11)
    ldh = n + 3
    Hd, bd, ones = TC._lower_dev(H, ldh), dev(b), _minv_dev(np.ones(n))
    x0 = np.random.default_rng(n + 12).standard_normal(n) * 1e-2
    for maxiter in (4, 60):
        for start in (np.zeros(n), x0):
            xp, itp, ip = _run(_pcg, n, start, Hd, ldh, ones, bd, maxiter)
            xc, itc, ic = _run(TC._cg, n, start, Hd, ldh, bd, maxiter)
            assert (itp, ip) == (itc, ic) and itc > 0
            assert np.array_equal(xp, xc), (maxiter, float(np.max(np.abs(xp - xc))))
        print(f"[pcg ones n={n} maxiter={maxiter}] iters {itc} info {ic}: bitwise ipm_cg")


@pytest.mark.parametrize("n", [257, 300])
def test_pcg_converged(n):
    """H = S K S with K the six-cluster matrix and S = diag(10 ** U(-3, 3)) (cond ~ 1e13): the solve
    converges in exactly the restatement's number of iterations -- test_pcg_ref.py asserts that
    the last two ||r|| / ||b|| sit >= 5 % away from rtol.  Both x have a residual under rtol ||b||,
    hence the distance bound 2e-5 ||b|| / lam_min(H) (test_cg_converged's).  Then a non-zero x0
    (there the restatement passes rtol by 3 %: no exact count is asked) and b = 0."""
    H, b = _clustered_scaled(n)
    lam_min = float(np.linalg.eigvalsh(H)[0])
    ldh = (n // 16 + 1) * 16
    Hd = TC._lower_dev(H, ldh)
    minv = pcg_ref.jacobi(H)
    bn = np.linalg.norm(b)

    def check(x0, tag):
        xref, inforef, itref = pcg_ref.pcg(H, b, minv, x0=x0, maxiter=200)
        assert inforef == 0
        xg, it, info = _run(_pcg, n, x0, Hd, ldh, None, dev(b), 200)
        res = np.linalg.norm(H @ xg - b)
        dist = np.linalg.norm(xg - xref)
        print(f"[pcg converged n={n} {tag}] iters {it} (restatement {itref}) info {info} ||Hx-b||/||b|| "
              f"{res / bn:.3g} ||x-xref|| / bound {dist / (2e-5 * bn / lam_min):.3g}")
        assert info == 0
        assert res < 1e-5 * bn * (1 + 64 * n * EPS)
        assert dist <= 2e-5 * bn / lam_min
        return it, itref

    it, itref = check(np.zeros(n), "x0=0")
    assert it == itref
    xc = np.random.default_rng(n + 2).standard_normal(n)
    it, _ = check((xc @ b) * xc / (xc @ (H @ xc)), "x0=scaled")
    assert 0 < it <= 200
    xg, it, info = _run(_pcg, n, xc, Hd, ldh, None, dev(np.zeros(n)), 200)
    assert (it, info) == (0, 0) and not xg.any()


def test_pcg_truncated():
    """S K S with K = Q diag(logspace(0, 6, 257)) Q^T, maxiter 8: the cap ends the solve.  The
    deviation is measured against the restatement as test_cg_truncated does: x_ld in longdouble,
    x_f64 scipy's bits; another summation order gets 64 x their distance (floor eps ||x_ld||).
    maxiter = 0 hands x0 back untouched with info 0."""
    n = 257
    K, _ = cg_ref.ill_conditioned(n, seed=5)
    H, b, _ = pcg_ref.scaled_system(K, np.random.default_rng(6).standard_normal(n), n + 3)
    minv = pcg_ref.jacobi(H)
    Hd, bd = TC._lower_dev(H, n + 3), dev(b)
    xg, it, info = _run(_pcg, n, np.zeros(n), Hd, n + 3, None, bd, 8)
    assert (it, info) == (8, 8)
    x_ld, info_ld, _ = pcg_ref.pcg(H, b, minv, maxiter=8, dtype=np.longdouble)
    x_f64, info_f, _ = pcg_ref.pcg(H, b, minv, maxiter=8)
    assert info_ld == info_f == 8
    d_ref = float(np.linalg.norm(x_f64 - x_ld))
    floor = float(EPS * np.linalg.norm(x_ld))
    d_dev = float(np.linalg.norm(xg - x_ld))
    print(f"[pcg truncated] ||x_dev - x_ld|| {d_dev:.3g}  ||x_f64 - x_ld|| {d_ref:.3g}  eps ||x_ld|| {floor:.3g}  "
          f"ratio to bound {d_dev / (64 * max(d_ref, floor)):.3g}")
    assert d_dev <= 64 * max(d_ref, floor)
    x0 = np.random.default_rng(7).standard_normal(n)
    xg, it, info = _run(_pcg, n, x0, Hd, n + 3, None, bd, 0)
    assert (it, info) == (0, 0) and np.array_equal(xg, x0)


def test_pcg_sign_symmetry():
    """ipm_pcg(-H, -b) == ipm_pcg(H, b) bit for bit (M = 1 / diag(-H) is negative too): the engine's
    H dx = -g is the reference's -H dx = g"""
    n = 300
    H, b = _clustered_scaled(n)
    ldh = n + 3
    Hp, Hm = TC._lower_dev(H, ldh), TC._lower_dev(-H, ldh)
    for maxiter in (8, 200):
        xp, itp, ip = _run(_pcg, n, np.zeros(n), Hp, ldh, None, dev(b), maxiter)
        xm, itm, im = _run(_pcg, n, np.zeros(n), Hm, ldh, None, dev(-b), maxiter)
        assert (itp, ip) == (itm, im) and np.array_equal(xp, xm)
    assert ip == 0


def test_pcg_bad_arguments():
    from ipm355 import _lib as L
    from ipm355 import problems
    from ipm355.device import DeviceProblem, expand_bound
    from gpu_util import devnan
    d = devnan((4,))
    assert _pcg(3, d, 2, None, d, d, 5)[0] == IPM_INVALID_ARG          # ldh < n
    assert _pcg(2, d, 2, None, d, d, -1)[0] == IPM_INVALID_ARG
    assert _pcg(2, d, 2, d, d, d, 5, rtol=-1.0)[0] == IPM_INVALID_ARG
    assert _pcg(0, d, 0, None, d, d, 5) == (IPM_OK, 0, 0)
    q = problems.qp_ineq_box(n=16, m=4, seed=0)
    prob = DeviceProblem("QP", 16, solve_method=L.SOLVE_CG, P=q["P"], q=q["q"], C=q["C"], d=q["d"],
                         lb=expand_bound(-3, 16), ub=expand_bound(3, 16))
    lib = prob.handle.lib
    assert prob.cg_precond == 0
    assert lib.ipm_set_cg_precond(prob.ptr, 2) == IPM_INVALID_ARG
    assert lib.ipm_set_cg_precond(prob.ptr, -1) == IPM_INVALID_ARG
    assert prob.cg_precond == 0
    assert lib.ipm_set_cg_precond(prob.ptr, L.CG_PRECOND_JACOBI) == IPM_OK and prob.cg_precond == 1
    prob.set_cg_precond(None)
    assert prob.cg_precond == 0
    prob.set_cg_precond("jacobi")
    assert prob.cg_precond == 1


# ------------------------------------------------------------------ one Newton step through the product
def _check_step(tag, H, g, x, xn, step, stats):
    """x_new = x + step dx_ref within 2e-5 ||g|| / lam_min(H) of the preconditioned restatement
    (both runs end under rtol ||g||)"""
    lam_min = float(np.linalg.eigvalsh(H)[0])
    dx_ref, info, iters, scaled = pcg_ref.newton_step(H, x, g, maxiter=1000)
    assert info == 0
    err = np.linalg.norm(xn - (x + step * dx_ref))
    bound = 2e-5 * np.linalg.norm(g) / lam_min
    print(f"[pcg newton step {tag}] N {len(x)} x.g {x @ g:.4g} scaled start {scaled} step {step:.3g} device CG iters "
          f"{stats['last_iters']} info {stats['last_info']} (restatement {iters}) err / bound {err / bound:.3g}")
    assert stats["last_info"] == 0 and 0 < stats["last_iters"] <= 1000
    assert step > 0 and err <= bound
    return scaled


def _check_one_iteration(tag, H, g, x, xn, step, stats):
    """with a cap of ONE iteration the step is x0 + a z: compared with the preconditioned
    restatement and with the unpreconditioned one (x0 + a' r) under test_gpu_cg._check_branch's
    bound -- the step must match the first and miss the second by more than 1e3 bounds (z, not r,
    was the direction)"""
    N = len(x)
    x0r, scaled = cg_ref.warm_start(H, x, g)
    dx_r, info, _ = pcg_ref.pcg(-H, g, -pcg_ref.jacobi(H), x0=x0r, maxiter=1)
    dx_w, _, _ = cg_ref.cg(-H, g, x0=x0r, maxiter=1)
    assert info == 1 and stats["last_info"] == 1 and stats["last_iters"] == 1
    r = -g - H @ x0r
    amp = max(1.0, (np.linalg.norm(g) + np.linalg.norm(np.abs(H) @ np.abs(x0r))) / np.linalg.norm(r))
    if scaled:
        amp += float(np.abs(x) @ np.abs(g) / abs(x @ g))
    bound = step * 64 * N * EPS * 8 * amp * (np.linalg.norm(x0r) + np.linalg.norm(dx_r)) + 4 * EPS * np.linalg.norm(x)
    e_right = np.linalg.norm(xn - (x + step * dx_r))
    e_wrong = np.linalg.norm(xn - (x + step * dx_w))
    print(f"[pcg one iteration {tag}] scaled start {scaled} step {step:.3g} err(preconditioned) / bound "
          f"{e_right / bound:.3g} err(unpreconditioned) / bound {e_wrong / bound:.3g}")
    assert step > 0 and e_right <= bound and e_wrong > 1e3 * bound


def _both_steps(tag, s, x, N):
    prob = s.fm.prob
    assert s.ns.method == "cg" and prob.cg_precond == 1
    H, g, xn, step, st = TC._one_step(s.fm, s.ns, prob, x, s.t0, 1000)
    assert H.shape == (N, N) and np.array_equal(H, H.T)
    scaled = _check_step(tag, H, g, x, xn, step, st)
    H1, g1, xn1, step1, st1 = TC._one_step(s.fm, s.ns, prob, x, s.t0, 1)
    assert np.array_equal(H1, H) and np.array_equal(g1, g)
    _check_one_iteration(tag, H, g, x, xn1, step1, st1)
    assert set(st1) == {"solves", "iters", "last_iters", "last_info"}
    return scaled


def test_newton_step_qp():
    """QPSolver(qp_ineq_box(n=130, m=64, seed=3), 'cg', max_cg_iters=1000, cg_preconditioner='jacobi')
    at both entry points of test_gpu_cg (one per warm-start branch): the converged step and the
    one-iteration step; cg_precond reads back 1 and cg_stats counts the solves (_one_step)."""
    import ipm355
    inst, xf = TC._qp130()
    s = ipm355.QPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method="cg", max_cg_iters=1000,
                        cg_preconditioner="jacobi", **inst)
    assert s.cg_preconditioner == "jacobi" and s.ns.cg_preconditioner == "jacobi"
    assert s.fm.prob.cg_stats() == {"solves": 0, "iters": 0, "last_iters": 0, "last_info": 0}
    for tag, x, scaled in TC._entry_points(inst, xf):
        assert _both_steps("qp130 " + tag, s, x, 130) == scaled


def test_newton_step_scaled_lp():
    """the scaled lp_ineq_box(n=40, m=20, seed=3) (sigma = 10 ** U(-2, 2)) from x_f / sigma"""
    import ipm355
    from ipm355 import problems
    sigma = 10.0 ** np.random.default_rng(7).uniform(-2, 2, 40)
    inst = problems.scale_variables(problems.lp_ineq_box(n=40, m=20, seed=3, with_xf=True), sigma)
    y = inst.pop("xf")
    assert (inst["C"] @ y < inst["d"]).all() and (y > inst["lower_bound"]).all() and (y < inst["upper_bound"]).all()
    s = ipm355.LPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method="cg", max_cg_iters=1000,
                        cg_preconditioner="jacobi", **inst)
    _both_steps("scaled lp40", s, y, 40)


def test_newton_step_phase1_problem():
    """the n = 130 instance's phase-1 barrier with IPM_SOLVE_CG and the Jacobi preconditioner:
    N = 131, the diagonal of the bordered H includes the border entry"""
    from ipm355 import _lib as L
    from ipm355 import newton as NS
    from ipm355.device import DeviceProblem, expand_bound
    from ipm355.function_manager import FunctionManagerPhase1
    inst, _ = TC._qp130()
    n = 130
    prob = DeviceProblem("LP", n, phase1=True, solve_method=L.SOLVE_CG, C=inst["C"], d=inst["d"],
                         lb=expand_bound(-3, n), ub=expand_bound(3, n))
    fm = FunctionManagerPhase1(C=inst["C"], d=inst["d"], x0=np.zeros(n), lower_bound=-3, upper_bound=3, t=0.01,
                               _prob=prob)
    ns = NS.NewtonSolverCG(function_manager=fm, max_iters=1, max_cg_iters=1000, phase1_flag=True, phase1_tol=0,
                           cg_preconditioner="jacobi")
    assert prob.cg_precond == 1
    x = np.append(np.zeros(n), fm.s)
    H, g, xn, step, st = TC._one_step(fm, ns, prob, x, 0.01, 1000)
    assert H.shape == (131, 131)
    _check_step("phase 1", H, g, x, xn, step, st)


def test_newton_step_socp():
    """an SOCPSolver step on socp_cones(n=24, K=4, mi=3, seed=3, eq=0) from its strictly feasible x0"""
    import ipm355
    from ipm355 import problems
    inst = problems.socp_cones(n=24, K=4, mi=3, seed=3, eq=0)
    s = ipm355.SOCPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method="cg", max_cg_iters=1000,
                          cg_preconditioner="jacobi", **inst)
    prob = s.fm.prob
    assert s.ns.method == "cg" and prob.cg_precond == 1
    x = np.array(inst["x0"], copy=True)
    H, g, xn, step, st = TC._one_step(s.fm, s.ns, prob, x, s.t0, 1000)
    assert H.shape == (24, 24)
    _check_step("socp24", H, g, x, xn, step, st)


# ------------------------------------------------------------------ full solves
def _solve(name, cap, **extra):
    z, kw = TC._fixture(name)
    s = TC._solver_class(str(z["kind"]))(check_cvxpy=False, suppress_print=True, linear_solve_method="cg",
                                         max_cg_iters=cap, **extra, **kw)
    return z, kw, s, s.solve()


@pytest.mark.parametrize("name", ["pcg_lp_n40_scaled", "pcg_lp_n200_scaled", "pcg_qp_n130"])
def test_full_solve_matches_preconditioned_reference_run(name):
    """the reference's run with M = 1 / diag(A) passed to scipy's cg (make_golden_pcg.py): the same
    number of outer iterations, x* feasible, the value within the fixture's value_tol"""
    z, _ = TC._fixture(name)
    z, kw, s, val = _solve(name, int(z["max_cg_iters"]), cg_preconditioner="jacobi")
    st = s.fm.prob.cg_stats()
    tol = float(z["value_tol"])
    print(f"[{name}] value {val!r} reference {float(z['value'])!r} |diff| / value_tol "
          f"{abs(val - float(z['value'])) / tol:.3g} outer {s.outer_iters} (reference {int(z['outer_iters'])}) "
          f"inner {s.inner_iters} cg {st}")
    assert s.fm.prob.cg_precond == 1
    assert s.outer_iters == int(z["outer_iters"])
    TC._assert_feasible(str(z["kind"]), kw, s.xstar)
    assert abs(val - float(z["value"])) <= tol
    assert st["solves"] == sum(s.inner_iters) and st["iters"] > 0


@pytest.mark.parametrize("name", ["pcg_lp_n40_scaled", "pcg_lp_n200_scaled"])
def test_plain_cg_misses_scaled_lp(name):
    """the same instance and cap without the preconditioner: the device's own plain 'cg' lands more
    than 100 value_tol from the optimum (the reference's plain run: plain_value), the Jacobi run
    inside value_tol -- the preconditioner decides whether 'cg' returns the optimum at all"""
    z, _ = TC._fixture(name)
    cap, tol, ref = int(z["max_cg_iters"]), float(z["value_tol"]), float(z["value"])
    _, _, sp, vp = _solve(name, cap)
    _, _, sj, vj = _solve(name, cap, cg_preconditioner="jacobi")
    print(f"[{name}] plain cg value {vp!r} (reference's plain run {float(z['plain_value'])!r}) off by "
          f"{abs(vp - ref) / tol:.3g} value_tol; jacobi {vj!r} off by {abs(vj - ref) / tol:.3g} value_tol")
    assert sp.fm.prob.cg_precond == 0 and sj.fm.prob.cg_precond == 1
    assert abs(vp - ref) > 100 * tol
    assert abs(vj - ref) <= tol


def test_default_is_bitwise_unpreconditioned():
    """cg_lp_n40 without the keyword and with cg_preconditioner=None: the same x* bit for bit, the
    same CG counters -- the default path is the unpreconditioned instantiation"""
    z, _ = TC._fixture("cg_lp_n40")
    cap = int(z["max_cg_iters"])
    _, _, s0, v0 = _solve("cg_lp_n40", cap)
    _, _, s1, v1 = _solve("cg_lp_n40", cap, cg_preconditioner=None)
    assert s0.fm.prob.cg_precond == 0 and s1.fm.prob.cg_precond == 0 and s1.cg_preconditioner is None
    assert v0 == v1 and np.array_equal(s0.xstar, s1.xstar)
    assert s0.fm.prob.cg_stats() == s1.fm.prob.cg_stats()
    assert abs(v0 - float(z["value"])) <= float(z["value_tol"])


# ------------------------------------------------------------------ facade
def test_facade_keyword():
    """an unknown preconditioner raises at construction; 'jacobi' with 'cholesky' changes nothing
    (x* bit for bit); equality rows with 'cg' keep the reference's NotImplementedError"""
    import ipm355
    from ipm355 import problems
    inst = problems.lp_ineq_box(n=40, m=20, seed=3)
    for cls, kw in ((ipm355.LPSolver, inst), (ipm355.QPSolver, problems.qp_ineq_box(n=16, m=4, seed=0)),
                    (ipm355.SOCPSolver, problems.socp_cones(n=24, K=4, mi=3, seed=3, eq=0))):
        with pytest.raises(ValueError, match="Please enter a valid CG preconditioner!"):
            cls(check_cvxpy=False, suppress_print=True, linear_solve_method="cg", cg_preconditioner="ssor", **kw)
    a = ipm355.LPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method="cholesky", **inst)
    b = ipm355.LPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method="cholesky",
                        cg_preconditioner="jacobi", **inst)
    va, vb = a.solve(), b.solve()
    assert b.cg_preconditioner == "jacobi" and b.ns.method == "cholesky"
    assert va == vb and np.array_equal(a.xstar, b.xstar) and a.inner_iters == b.inner_iters
    eq = problems.lp_eq_box(20, 5, seed=0)
    with pytest.raises(NotImplementedError, match="CONJUGATE GRADIENT GIVING UNSTABLE RESULTS"):
        ipm355.LPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method="cg", try_diag=False,
                        cg_preconditioner="jacobi", **eq)
