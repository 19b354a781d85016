"""-m gpu: linear_solve_method='cg' -- ipm_symv and ipm_cg against NumPy and the restatement
tests/cg_ref.py, one Newton step through the product, full solves against reference-run fixtures
(tests/golden/cg_*.npz, make_golden_cg.py).

Conventions of test_gpu_level0.py: operands padded with NaN (for ipm_symv the strict UPPER triangle
too: only the lower one may be read), a sentinel behind every output, each test prints its worst
err / bound.  Without the feature every test here fails on a missing symbol or NotImplementedError.
"""
import ctypes
import os

import numpy as np
import pytest

import cg_ref
import golden_io
from conftest import GOLDEN
from gpu_util import dev, devnan, handle, host

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
IPM_OK, IPM_INVALID_ARG = 0, 2
SENTINEL = 12345.0
T = 128      # SYMV_T, the tile edge of k_symv_tiles


def _lower_dev(H, ldh):
    """column-major lower triangle of H with leading dimension ldh on the device; the strict upper
    triangle and the ld padding are NaN"""
    n = H.shape[0]
    M = np.full((n, ldh), np.nan)
    M[:, :n] = np.where(np.triu(np.ones((n, n), dtype=bool)), H.T, np.nan)   # M[j, i] = H[i, j], i >= j
    return dev(M)


def _symv(n, alpha, Hd, ldh, xd, beta, yd):
    from ipm355 import _lib as L
    h = handle()
    return h.lib.ipm_symv(h.ptr, n, alpha, L.dptr(Hd), ldh, L.dptr(xd), beta, L.dptr(yd))


def _cg(n, Hd, ldh, bd, xd, maxiter, rtol=1e-5):
    from ipm355 import _lib as L
    h = handle()
    it, info = ctypes.c_int32(-7), ctypes.c_int32(-7)
    rc = h.lib.ipm_cg(h.ptr, n, L.dptr(Hd), ldh, L.dptr(bd), L.dptr(xd), maxiter, rtol, ctypes.byref(it),
                      ctypes.byref(info))
    return rc, it.value, info.value


def _xbuf(x):
    """x in front of a sentinel: the solve must not write past n"""
    buf = dev(np.append(x, SENTINEL))
    return buf, buf[:len(x)]


SYMV_N = [1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 255, 256, 257, 300, 513]


@pytest.mark.parametrize("n", SYMV_N)
def test_symv_matches_numpy(n):
    """k_symv_tiles / k_symv_reduce with 128 x 128 tiles (T - 1, T, T + 1, 2T + 1 = 127, 128, 129, 257):
      n <= 128      one diagonal tile (1, 2, 3: most lanes without a row; 63 / 64 / 65: the scalar
                    layout's second row l + 64 absent / absent / present on lane 0; 127: ragged)
      129           2 x 2 blocks, the off-diagonal tile one row high: its transposed product feeds
                    block 0 from a single row, block 1's diagonal tile holds one entry
      191, 255, 256 ragged and full second block; 257, 300: 3 blocks, 513: 5 blocks (10 off-diagonal
                    tiles, every output block summed from 5 slots)
    ldh = n (even n: the 16-byte loads; odd n: scalar loads), n + 3 (the other parity) and the next
    multiple of 16 above n (vector loads; odd n: the last row of a tile falls back to scalar).
    The strict upper triangle and the ld padding are NaN; with beta = 0 so is y.  Two calls on the
    same inputs must agree bit for bit (fixed summation order, no atomics)."""
    rng = np.random.default_rng(n)
    A = rng.uniform(-2, 2, (n, n))
    H = (A + A.T) / 2
    x = rng.uniform(-2, 2, n)
    y0 = rng.uniform(-2, 2, n)
    full, fbound = H @ x, np.abs(H) @ np.abs(x)
    worst = 0.0
    for ldh in (n, n + 3, (n // 16 + 1) * 16):
        Hd = _lower_dev(H, ldh)
        xd = dev(x)
        for alpha, beta in [(1.0, 0.0), (-0.75, 0.5)]:
            outs = []
            for _ in range(2):
                ybuf = devnan((n + 2,)) if beta == 0.0 else dev(np.append(y0, [0.0, 0.0]))
                ybuf[n:] = SENTINEL
                assert _symv(n, alpha, Hd, ldh, xd, beta, ybuf[:n]) == IPM_OK
                outs.append(host(ybuf))
            got = outs[0]
            assert np.array_equal(outs[0], outs[1]), ("not repeatable", ldh, alpha, beta)
            assert np.all(got[n:] == SENTINEL)
            assert np.all(np.isfinite(got[:n])), ("non-finite: upper triangle or padding read", ldh, alpha, beta)
            ref = alpha * full + beta * y0
            bound = 64 * EPS * (abs(alpha) * fbound + abs(beta * y0))
            r = float(np.max(np.abs(got[:n] - ref) / bound))
            assert r <= 1.0, (ldh, alpha, beta, r)
            worst = max(worst, r)
    print(f"[symv n={n}] worst err / bound {worst:.3g}")


def test_symv_bad_arguments():
    d = devnan((4,))
    assert _symv(-1, 1.0, d, 4, d, 0.0, d) == IPM_INVALID_ARG
    assert _symv(3, 1.0, d, 2, d, 0.0, d) == IPM_INVALID_ARG      # ldh < n
    assert _symv(0, 1.0, d, 0, d, 0.0, d) == IPM_OK


@pytest.mark.parametrize("n", [257, 300])
def test_cg_converged(n):
    """Q diag(lam) Q^T with six distinct eigenvalues (3 blocks of the SYMV, the last ragged): CG
    ends after exactly six iterations -- test_cg_ref.py asserts the margin (||r|| / ||b|| >= 0.1
    before, <= 1e-9 after).  Both residuals are under rtol ||b||, hence the distance bound
    2e-5 ||b|| / lam_min.  Then a non-zero x0 (the warm start's scaled vector: r = b - H x0 takes
    the extra SYMV) and b = 0 (x = 0 whatever x0, no iteration)."""
    H, lam = cg_ref.clustered(n, seed=n)
    b = np.random.default_rng(n + 1).standard_normal(n)
    ldh = (n // 16 + 1) * 16
    Hd = _lower_dev(H, ldh)
    xref, inforef, itref = cg_ref.cg(H, b, maxiter=50)
    assert inforef == 0 and itref == 6
    bn = np.linalg.norm(b)

    def check(x0, tag):
        buf, xd = _xbuf(x0)
        rc, it, info = _cg(n, Hd, ldh, dev(b), xd, 50)
        got = host(buf)
        assert rc == IPM_OK and got[n] == SENTINEL
        xg = got[:n]
        res = np.linalg.norm(H @ xg - b)
        dist = np.linalg.norm(xg - xref)
        print(f"[cg converged n={n} {tag}] iters {it} info {info} ||Hx-b||/||b|| {res / bn:.3g} "
              f"||x-xref|| / bound {dist / (2e-5 * bn / lam.min()):.3g}")
        assert info == 0
        assert res < 1e-5 * bn * (1 + 64 * n * EPS)
        assert dist <= 2e-5 * bn / lam.min()
        return it

    assert check(np.zeros(n), "x0=0") == 6
    xc = np.random.default_rng(n + 2).standard_normal(n)
    x0w = (xc @ b) * xc / (xc @ (H @ xc))
    _, inforw, itw = cg_ref.cg(H, b, x0=x0w, maxiter=50)
    assert inforw == 0
    assert check(x0w, "x0=scaled") <= 50
    buf, xd = _xbuf(x0w)
    rc, it, info = _cg(n, Hd, ldh, dev(np.zeros(n)), xd, 50)
    got = host(buf)
    assert (rc, it, info) == (IPM_OK, 0, 0) and not got[:n].any() and got[n] == SENTINEL


def test_cg_truncated():
    """lam = logspace(0, 6, 257), maxiter 8: the cap ends the solve (info == 8 == iters).  The
    deviation is measured against the restatement, not the code under test: x_ld is cg_ref in
    longdouble, x_f64 the float64 restatement (scipy's bits); another summation order gets 64 x
    their distance (floor eps ||x_ld||).  maxiter = 0 hands x0 back untouched with info 0."""
    n = 257
    H, lam = cg_ref.ill_conditioned(n, seed=5)
    b = np.random.default_rng(6).standard_normal(n)
    Hd = _lower_dev(H, n + 3)
    buf, xd = _xbuf(np.zeros(n))
    rc, it, info = _cg(n, Hd, n + 3, dev(b), xd, 8)
    got = host(buf)
    assert rc == IPM_OK and got[n] == SENTINEL
    assert (it, info) == (8, 8)
    x_ld, info_ld, _ = cg_ref.cg(H, b, maxiter=8, dtype=np.longdouble)
    x_f64, info_f, _ = cg_ref.cg(H, b, maxiter=8)
    assert info_ld == info_f == 8
    d_ref = float(np.linalg.norm(x_f64 - x_ld))
    floor = float(EPS * np.linalg.norm(x_ld))
    d_dev = float(np.linalg.norm(got[:n] - x_ld))
    print(f"[cg truncated] ||x_dev - x_ld|| {d_dev:.3g}  ||x_f64 - x_ld|| {d_ref:.3g}  eps ||x_ld|| {floor:.3g}  "
          f"ratio to bound {d_dev / (64 * max(d_ref, floor)):.3g}")
    assert d_dev <= 64 * max(d_ref, floor)
    x0 = np.random.default_rng(7).standard_normal(n)
    buf, xd = _xbuf(x0)
    rc, it, info = _cg(n, Hd, n + 3, dev(b), xd, 0)
    assert (rc, it, info) == (IPM_OK, 0, 0)
    assert np.array_equal(host(buf), np.append(x0, SENTINEL))


def test_cg_bad_arguments():
    d = devnan((4,))
    assert _cg(3, d, 2, d, d, 5)[0] == IPM_INVALID_ARG          # ldh < n
    assert _cg(2, d, 2, d, d, -1)[0] == IPM_INVALID_ARG
    assert _cg(2, d, 2, d, d, 5, rtol=-1.0)[0] == IPM_INVALID_ARG


# ------------------------------------------------------------------ one Newton step through the product
def _qp130():
    from ipm355 import problems
    inst = problems.qp_ineq_box(n=130, m=64, seed=3, with_xf=True)
    xf = inst.pop("xf")
    return inst, xf


def _entry_points(inst, xf):
    """two strictly feasible points of the n = 130 instance: x_f itself (slack 1 on every row:
    x.g > 0 at t = 0.1, the zero start) and x_f moved to slack 0.01 on the row with the most
    negative d (that row's barrier term (C x)_i / slack_i ~ -4000 makes x.g < 0: the scaled start)"""
    C, d = inst["C"], inst["d"]
    i = int(np.argmin(d))
    xb = xf + 0.99 * C[i] / (C[i] @ C[i])
    assert (C @ xb < d).all() and (np.abs(xb) < 3).all()
    return [("x_f", xf, False), ("near row %d" % i, xb, True)]


def _one_step(fm, ns, prob, x, t, cap):
    """H, g at (x, t) through ipm_fm_hessian / ipm_fm_gradient, then one Newton iteration"""
    xt = dev(x)
    fm.update_x(xt)
    fm.update_t(t)
    H, g = fm.hessian(), fm.gradient()
    prob.set_cg(cap)
    ns.max_iters = 1
    s0 = prob.cg_stats()
    xn = xt.clone()
    ns.solve(xn, t)
    s1 = prob.cg_stats()
    assert s1["solves"] == s0["solves"] + 1 and s1["iters"] == s0["iters"] + s1["last_iters"]
    return H, g, host(xn), float(ns.last_result.last_step), s1


def _check_step(tag, H, g, x, xn, step, stats, scaled_expected, cap_small=1):
    N = len(x)
    lam_min = float(np.linalg.eigvalsh(H)[0])
    dx_ref, info, iters, scaled = cg_ref.newton_step(H, x, g, maxiter=1000)
    assert info == 0 and scaled == scaled_expected, (tag, info, scaled, float(x @ g))
    err = np.linalg.norm(xn - (x + step * dx_ref))
    bound = 2e-5 * np.linalg.norm(g) / lam_min
    print(f"[newton step {tag}] N {N} x.g {x @ g:.4g} scaled start {scaled} step {step:.3g} device CG iters "
          f"{stats['last_iters']} info {stats['last_info']} (restatement {iters}) err / bound {err / bound:.3g}")
    assert stats["last_info"] == 0 and 0 < stats["last_iters"] <= 1000
    assert step > 0 and err <= bound


def _check_branch(tag, H, g, x, xn, step, stats, scaled_expected):
    """with a cap of ONE iteration the step shows which x0 the device started from: x0 + a r is
    compared with the restatement from the right and from the other start.  One iteration is a
    SYMV and three dot products at N <= 131: 64 N eps relative each, times the cancellation
    (||g|| + || |H| |x0| ||) / ||r|| of r = -g - H x0 (and |x|.|g| / |x.g| of the scaled start),
    times 8 for the chained operations; plus the rounding of x + step dx itself."""
    N = len(x)
    x0r, scaled = cg_ref.warm_start(H, x, g)
    assert scaled == scaled_expected
    x0w = np.zeros(N) if scaled else -(x @ g) * x / (x @ (H @ x))
    dx_r, info, _ = cg_ref.cg(-H, g, x0=x0r, maxiter=1)
    dx_w, _, _ = cg_ref.cg(-H, g, x0=x0w, maxiter=1)
    assert info == 1 and stats["last_info"] == 1 and stats["last_iters"] == 1
    r = -g - H @ x0r
    amp = max(1.0, (np.linalg.norm(g) + np.linalg.norm(np.abs(H) @ np.abs(x0r))) / np.linalg.norm(r))
    if scaled:     # x0 carries the cancellation of x.g (terms of both signs) as well
        amp += float(np.abs(x) @ np.abs(g) / abs(x @ g))
    bound = step * 64 * N * EPS * 8 * amp * (np.linalg.norm(x0r) + np.linalg.norm(dx_r)) + 4 * EPS * np.linalg.norm(x)
    e_right = np.linalg.norm(xn - (x + step * dx_r))
    e_wrong = np.linalg.norm(xn - (x + step * dx_w))
    print(f"[warm start {tag}] scaled {scaled} step {step:.3g} err(right start) / bound {e_right / bound:.3g} "
          f"err(other start) / bound {e_wrong / bound:.3g}")
    assert step > 0 and e_right <= bound and e_wrong > 1e3 * bound


def test_newton_step_matches_restatement():
    """QPSolver(qp_ineq_box(n=130, m=64, seed=3), 'cg', max_cg_iters=1000): one centering call with
    max_iters = 1 at the solver's first barrier t from two entry points, one per warm-start branch
    (N = 130: two SYMV blocks, the second with 2 rows).  x_new = x + last_step dx_ref within
    2e-5 ||g|| / lam_min(H) (both CG runs end under rtol ||g||); cg_stats counts the solve."""
    import ipm355
    inst, xf = _qp130()
    s = ipm355.QPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method="cg", max_cg_iters=1000, **inst)
    prob = s.fm.prob
    assert s.ns.method == "cg" and prob.cg_stats() == {"solves": 0, "iters": 0, "last_iters": 0, "last_info": 0}
    for tag, x, scaled in _entry_points(inst, xf):
        H, g, xn, step, st = _one_step(s.fm, s.ns, prob, x, s.t0, 1000)
        assert H.shape == (130, 130) and np.array_equal(H, H.T)
        _check_step(tag, H, g, x, xn, step, st, scaled)
        H1, g1, xn1, step1, st1 = _one_step(s.fm, s.ns, prob, x, s.t0, 1)
        assert np.array_equal(H1, H) and np.array_equal(g1, g)
        _check_branch(tag, H, g, x, xn1, step1, st1, scaled)


def test_newton_step_phase1_problem():
    """the same instance's phase-1 barrier with IPM_SOLVE_CG: N = n + 1 = 131, H the bordered
    (n + 1) x (n + 1) matrix (the facades keep phase 1 on Cholesky as the reference does; the engine
    branch is reached through the device problem)."""
    from ipm355 import _lib as L
    from ipm355 import newton as NS
    from ipm355.device import DeviceProblem, expand_bound
    from ipm355.function_manager import FunctionManagerPhase1
    inst, _ = _qp130()
    n = 130
    prob = DeviceProblem("LP", n, phase1=True, solve_method=L.SOLVE_CG, C=inst["C"], d=inst["d"],
                         lb=expand_bound(-3, n), ub=expand_bound(3, n))
    fm = FunctionManagerPhase1(C=inst["C"], d=inst["d"], x0=np.zeros(n), lower_bound=-3, upper_bound=3, t=0.01,
                               _prob=prob)
    ns = NS.NewtonSolverCG(function_manager=fm, max_iters=1, max_cg_iters=1000, phase1_flag=True, phase1_tol=0)
    x = np.append(np.zeros(n), fm.s)
    H, g, xn, step, st = _one_step(fm, ns, prob, x, 0.01, 1000)
    assert H.shape == (131, 131)
    _, scaled = cg_ref.warm_start(H, x, g)
    _check_step("phase 1", H, g, x, xn, step, st, scaled)


# ------------------------------------------------------------------ full solves
def _fixture(name):
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    kw = golden_io.solver_kwargs(z)
    kw = {k: (v.item() if isinstance(v, np.ndarray) and v.ndim == 0 else v) for k, v in kw.items()}
    return z, kw


def _solver_class(kind):
    import ipm355
    return {"LP": ipm355.LPSolver, "QP": ipm355.QPSolver, "SOCP": ipm355.SOCPSolver}[kind]


def _assert_feasible(kind, kw, x):
    """bounds compared as they are; the rows recomputed here on the host get the rounding of that
    recomputation, 64 eps sum|terms| (at the last barrier t ~ 1e12 the active slacks are ~1e-14:
    the reference's own x* of cg_qp_n130 gives a recomputed slack of exactly 0)"""
    lb, ub = kw.get("lower_bound"), kw.get("upper_bound")
    if lb is not None:
        assert (x >= lb).all()
    if ub is not None:
        assert (x <= ub).all()
    if kind == "SOCP":
        for A, b, c, d in zip(kw["A"], kw["b"], kw["c"], kw["d"]):
            terms = np.linalg.norm(np.abs(A) @ np.abs(x) + np.abs(b)) + np.abs(c) @ np.abs(x) + abs(d)
            assert np.linalg.norm(A @ x + b) <= c @ x + d + 64 * EPS * terms
    else:
        C, d = kw["C"], kw["d"]
        assert (C @ x <= d + 64 * EPS * (np.abs(C) @ np.abs(x) + np.abs(d))).all()


@pytest.mark.parametrize("name", ["cg_qp_n40", "cg_qp_n130", "cg_lp_n40", "cg_socp_n24"])
def test_full_solve_matches_reference_run(name):
    """the reference's own 'cg' run (make_golden_cg.py): the same number of outer iterations, x*
    feasible, the value within the fixture's value_tol = 10 x the reference's spread over
    {cholesky, cg at the cap, cg at twice the cap} (floor 1e-9 relative)"""
    z, kw = _fixture(name)
    kind, cap = str(z["kind"]), int(z["max_cg_iters"])
    s = _solver_class(kind)(check_cvxpy=False, suppress_print=True, linear_solve_method="cg", max_cg_iters=cap, **kw)
    val = s.solve()
    st = s.fm.prob.cg_stats()
    tol = float(z["value_tol"])
    print(f"[{name}] value {val!r} reference {float(z['value'])!r} |diff| / value_tol "
          f"{abs(val - float(z['value'])) / tol:.3g} outer {s.outer_iters} (reference {int(z['outer_iters'])}) "
          f"inner {s.inner_iters} cg {st}")
    assert s.outer_iters == int(z["outer_iters"])
    _assert_feasible(kind, kw, s.xstar)
    assert abs(val - float(z["value"])) <= tol
    assert st["solves"] == sum(s.inner_iters) and st["iters"] > 0


def test_truncation_is_reported():
    """cg_qp_n130 with max_cg_iters = 50: the solve completes with a finite value (no comparison:
    the reference itself lands 6e-5 away with this cap) and the counters show truncated solves
    (info == 50), sampled after every centering call"""
    z, kw = _fixture("cg_qp_n130")
    s = _solver_class("QP")(check_cvxpy=False, suppress_print=True, linear_solve_method="cg", max_cg_iters=50, **kw)
    prob, seen = s.fm.prob, []
    inner = s.ns.solve

    def sampled(*a, **k):
        out = inner(*a, **k)
        seen.append(prob.cg_stats()["last_info"])
        return out
    s.ns.solve = sampled
    val = s.solve()
    st = prob.cg_stats()
    print(f"[truncation] value {val!r} last info per centering call {seen} cg {st}")
    assert np.isfinite(val) and np.all(np.isfinite(s.xstar))
    assert 50 in seen
    assert st["iters"] <= 50 * st["solves"]


def test_unchanged_refusals():
    """equality constraints with 'cg' keep the reference's NotImplementedError; the C ABI refuses a
    CG problem with equality rows and a negative cap"""
    import ipm355
    from ipm355 import _lib as L
    from ipm355 import problems
    from ipm355.device import DeviceProblem, expand_bound
    inst = problems.lp_eq_box(20, 5, seed=0)
    with pytest.raises(NotImplementedError, match="CONJUGATE GRADIENT GIVING UNSTABLE RESULTS"):
        ipm355.LPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method="cg", try_diag=False, **inst)
    with pytest.raises(NotImplementedError, match="CONJUGATE GRADIENT GIVING UNSTABLE RESULTS"):
        ipm355.LPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method="cg", **inst)
    with pytest.raises(L.IPMBackendError, match="error 4"):
        DeviceProblem("LP", 20, solve_method=L.SOLVE_CG, c=inst["c"], A=inst["A"], b=inst["b"],
                      lb=expand_bound(0, 20), ub=expand_bound(3, 20))
    q = problems.qp_ineq_box(n=16, m=4, seed=0)
    prob = DeviceProblem("QP", 16, solve_method=L.SOLVE_CG, P=q["P"], q=q["q"], C=q["C"], d=q["d"],
                         lb=expand_bound(-3, 16), ub=expand_bound(3, 16))
    lib = prob.handle.lib
    assert lib.ipm_set_cg(prob.ptr, -1, 1e-5) == IPM_INVALID_ARG
    assert lib.ipm_set_cg(prob.ptr, 50, -1.0) == IPM_INVALID_ARG
    assert lib.ipm_set_cg(prob.ptr, 50, 1e-5) == IPM_OK
