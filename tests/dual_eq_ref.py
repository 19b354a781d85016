"""The dual-form LP Newton step with equality rows (linear_solve_method='cholesky_dual_eq'): NumPy
restatement, long-double reference, instances and the error bound shared by test_dual_eq_ref.py (CPU) and
the GPU tests test_gpu_dual_eq_step.py / test_gpu_dual_eq_solve.py.

Infeasible-start Newton on min c'x, A x = b, C x <= d, lb <= x <= ub (the system the reference's block
elimination solves, NewtonSolverInfeasibleStart.py:386-511):

    H dx + A^T nu = -g,   A dx = -(A x - b),   dv = nu - v,    H = diag(D) + C^T diag(w) C

(D, w as in tests/dual_ref.py).  With z = w o (C dx), E = 1/D and M = [C; A] the device eliminates
dx = E o (-g - C^T z - A^T nu) and solves one symmetric system of order m + p,

    K = diag([1/w; 0]) + M diag(E) M^T,    K [z; nu] = [C (E o -g); A (E o -g) + (A x - b)],

followed by three rounds of iterative refinement on the residual of the full KKT system (H applied
through C, never formed):

    rho_x = -g - (D o dx + C^T (w o (C dx))) - A^T nu,   rho_p = -(A x - b) - A dx
    [z'; nu'] = K^-1 [C (E o rho_x); A (E o rho_x) - rho_p],   dx += E o (rho_x - M^T [z'; nu']),  nu += nu'

  * ``eq_direction`` restates exactly that in fp64.
  * ``reference_step`` solves the KKT matrix [[H, A^T], [A, 0]] with H formed in long double (an fp64 LU of
    its rounding, refined against the long-double matrix: dual_ref.reference_solve).
  * the bound is B = 64 eps cond2(KKT) ||[dx; nu]||_2, the project's Newton-step allowance on the system
    the step solves.  It is not a theorem for the dual form: test_dual_eq_ref.py holds the fp64
    restatement to B / 4 at every state, the device is then held to B.

States: dual_ref.Instance(n, m, bounds, frac) plus a seeded normal A (p x n), b = A x_f (x_f the
instance's strictly feasible point, so A x = b is consistent with the inequalities) and a seeded normal
v, at SHAPES x the three bound sets x t in {1, 1e3, 1e6} x frac in {0, 0.9, 0.999}: 270 states.  The
KKT matrix does not depend on t: each (shape, bounds, frac) forms and factors it once.
"""
import numpy as np
import scipy.linalg

import dual_ref as D
from dual_ref import EPS, LD, O, problems

# (n, p, m): m + p < n (K needs A of full row rank and is cheapest there), both sides of the 16-row MFMA
# block and of the 64-row tile for m, for p and for m + p, a 64-row block straddling m (m not a multiple of
# 64) and not (m = 64), the K split of the assembly (n > 512)
SHAPES = [(2, 1, 1), (17, 3, 15), (33, 1, 31), (64, 16, 47), (65, 17, 64), (130, 30, 97), (129, 64, 64),
          (257, 65, 129), (300, 64, 40), (520, 130, 127)]
BOUNDS, TS, FRACS = D.BOUNDS, D.TS, D.FRACS
REFINE = 3          # the engine's DUAL_REFINE
MARGIN = D.MARGIN
_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def states():
    return [(n, p, m, b, t, f) for (n, p, m) in SHAPES for b in BOUNDS for t in TS for f in FRACS]


def state_id(s):
    n, p, m, b, t, f = s
    return f"n{n}-p{p}-m{m}-{b}-t{t:g}-f{f:g}"


class EqInstance:
    """dual_ref.Instance(n, m, bounds, frac) with p seeded equality rows through its feasible point"""

    def __init__(self, n, p, m, bounds, frac):
        self.base = D.instance(n, m, bounds, frac)
        self.n, self.p, self.m, self.bounds, self.frac = n, p, m, bounds, frac
        seed = 1000 + 7 * n + m
        xf = problems.lp_ineq_box(n, m, seed=seed, with_xf=True)["xf"]
        rng = np.random.default_rng(seed + 2)
        self.A = rng.normal(size=(p, n))
        self.b = self.A @ xf
        self.v = rng.normal(size=p)
        for k in ("c", "C", "d", "lb", "ub", "x"):
            setattr(self, k, getattr(self.base, k))

    def oracle(self, t):
        return self.base.oracle(t)

    def device(self, solve_method):
        import ipm355
        return ipm355.FunctionManagerLP(c=self.c, A=self.A, b=self.b, C=self.C, d=self.d, x0=self.x.copy(),
                                        lower_bound=self.lb, upper_bound=self.ub, t=1, try_diag=False,
                                        solve_method=solve_method)


def instance(n, p, m, bounds, frac):
    return _memo(("inst", n, p, m, bounds, frac), lambda: EqInstance(n, p, m, bounds, frac))


# ------------------------------------------------------------------ the step, three ways
def eq_direction(fm, A, b, x, v, g, add=0.0, refine=REFINE):
    """the fp64 restatement of the device's step at the manager's slack state -> (dx, dv)"""
    w, Dv = D.hessian_vectors(fm, add)
    C = fm.C
    m = len(w)
    E = 1 / Dv
    M = np.vstack([C, A])
    K = (M * E) @ M.T
    K[np.arange(m), np.arange(m)] += 1 / w
    axb = A @ x - b
    eg = E * (-g)
    r = np.concatenate([C @ eg, A @ eg - (-axb)])
    L = scipy.linalg.cho_factor(K, lower=True, check_finite=False)
    y = scipy.linalg.cho_solve(L, r, check_finite=False)
    nu = y[m:].copy()
    dx = E * (-g - C.T @ y[:m] - A.T @ nu)
    for _ in range(refine):
        rho_x = -g - (Dv * dx + C.T @ (w * (C @ dx))) - A.T @ nu
        rho_p = -axb - A @ dx
        er = E * rho_x
        y = scipy.linalg.cho_solve(L, np.concatenate([C @ er, A @ er - rho_p]), check_finite=False)
        dx = dx + E * (rho_x - C.T @ y[:m] - A.T @ y[m:])
        nu = nu + y[m:]
    return dx, nu - v


def oracle_direction(fm, A, b, x, v, g, add=0.0):
    """the Cholesky block elimination of oracle.InfeasibleNewton.direction (psd add on H's diagonal)"""
    ns = O.InfeasibleNewton(A, b, fm, "cholesky", use_psd_condition=add != 0.0)
    return ns.direction(x, v, g)


def kkt_ref(inst, add=0.0):
    """(long-double KKT matrix, the fp64 LU of its rounding, cond2) at the instance's point: shared by every t"""
    def run():
        fm = inst.oracle(1.0)
        H = D._ld_hessian(fm, add)
        n, p = inst.n, inst.p
        Kk = np.zeros((n + p, n + p), LD)
        Kk[:n, :n] = H
        Kk[:n, n:] = inst.A.T.astype(LD)
        Kk[n:, :n] = inst.A.astype(LD)
        K64 = Kk.astype(np.float64)
        return Kk, scipy.linalg.lu_factor(K64, check_finite=False), float(np.linalg.cond(K64))
    return _memo(("kkt", inst.n, inst.p, inst.m, inst.bounds, inst.frac, add), run)


def reference_step(state, add=0.0):
    """dict(sol = [dx; nu] (fp64 rounding of the refined long-double solve), g, bound, cond2, inst)"""
    n, p, m, bounds, t, frac = state

    def run():
        inst = instance(n, p, m, bounds, frac)
        fm = inst.oracle(t)
        g = fm.gradient().copy()
        Kk, lu, cond2 = kkt_ref(inst, add)
        rhs = np.concatenate([-g, -(inst.A @ inst.x - inst.b)])
        sol = D.reference_solve(Kk, lu, rhs, cond2).astype(np.float64)
        return {"sol": sol, "g": g, "cond2": cond2, "bound": 64 * EPS * cond2 * float(np.linalg.norm(sol)),
                "inst": inst}
    return _memo(("step", state, add), run)


def joint_error(dx, dv, ref):
    """||[dx; v + dv] - reference|| / B"""
    inst = ref["inst"]
    got = np.concatenate([dx, inst.v + dv])
    return float(np.linalg.norm(got - ref["sol"]) / ref["bound"])


# ------------------------------------------------------------------ the oracle's residual line search
def replay_line_search(fm, A, b, x0, v, dx, dv, g, alpha, beta, K=0):
    """InfeasibleNewton.backtrack (NewtonSolverInfeasibleStart.py:170-273) decision by decision ->
    dict(step, feas_margin: min over the feasibility candidates of min|s| / max|s0|, res_margin: min over the
    residual tests of |rn - (1 - alpha step) r| / max(1, r), decisive: both >= MARGIN and the step floor not
    reached).  Leaves fm at x0."""
    s0 = np.array(fm.slacks, copy=True)
    smax = float(np.abs(s0).max())
    step = 1
    fm.update_x(x0 + step * dx)
    feas = [float(np.abs(fm.slacks).min()) / smax]
    floor = False
    while (fm.slacks < 0).any():
        step *= beta
        if step < O.STEP_FLOOR:
            floor = True
            break
        fm.update_x(x0 + step * dx)
        feas.append(float(np.abs(fm.slacks).min()) / smax)
    res = []
    if not floor:
        ATv, ATdv, Axb, Adx = A.T @ v, A.T @ dv, A @ x0 - b, A @ dx
        r = np.linalg.norm(np.append(g + ATv, Axb))
        rn = np.linalg.norm(np.append(fm.gradient() + ATv + step * ATdv, Axb + step * Adx))
        attempt = 0
        while True:
            rhs = (1 - alpha * step) * r
            res.append(abs(float(rn - rhs)) / max(1.0, float(r)))
            if not rn > rhs:
                break
            attempt += 1
            step *= beta
            if step < O.STEP_FLOOR:
                floor = True
                break
            fm.update_x(x0 + step * dx, update_slacks=(K > 0 and attempt % K == K - 1))
            rn = np.linalg.norm(np.append(fm.gradient() + ATv + step * ATdv, Axb + step * Adx))
    fm.update_x(x0.copy())
    fmn, rm = min(feas), (min(res) if res else 0.0)
    return {"step": step, "feas_margin": fmn, "res_margin": rm,
            "decisive": (not floor) and fmn >= MARGIN and rm >= MARGIN}


def oracle_line_search(state, alpha=0.2, beta=0.6):
    """one InfeasibleNewton step of the Cholesky oracle from the state's point (v the instance's), replayed"""
    n, p, m, bounds, t, frac = state

    def run():
        inst = instance(n, p, m, bounds, frac)
        fm = inst.oracle(t)
        x0 = inst.x.copy()
        g = fm.gradient(x0).copy()
        dx, dv = oracle_direction(fm, inst.A, inst.b, x0, inst.v, g)
        return replay_line_search(fm, inst.A, inst.b, x0, inst.v, dx, dv, g, alpha, beta)
    return _memo(("ls", state, alpha, beta), run)


def restated_line_search(state, alpha=0.2, beta=0.6):
    n, p, m, bounds, t, frac = state
    inst = instance(n, p, m, bounds, frac)
    fm = inst.oracle(t)
    x0 = inst.x.copy()
    g = fm.gradient(x0).copy()
    dx, dv = eq_direction(fm, inst.A, inst.b, x0, inst.v, g)
    return replay_line_search(fm, inst.A, inst.b, x0, inst.v, dx, dv, g, alpha, beta)


# ------------------------------------------------------------------ full oracle solves
SOLVE_SHAPES = [(17, 3, 15), (65, 1, 64), (130, 30, 97), (200, 50, 100), (257, 65, 129), (300, 64, 40)]
SHORT_OUTER = 4     # beyond it the reference's own infeasible-start trajectory is not reproducible


def generated(n, p, m):
    """C / d / c of lp_ineq_box(seed = 5), A normal from default_rng(5), b = A x_f, bounds +-3, LP_KWARGS"""
    inst = problems.lp_ineq_box(n, m, seed=5, with_xf=True)
    xf = inst.pop("xf")
    A = np.random.default_rng(5).normal(size=(p, n))
    return dict(inst, A=A, b=A @ xf, **problems.LP_KWARGS)


def copy_kw(kw):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


def perturbed(kw, seed):
    """every array input times (1 + 1e-15 N(0, 1)): the oracle's own numerical envelope (make_golden.py)"""
    rng = np.random.default_rng(seed)
    out = copy_kw(kw)
    for k in ("c", "A", "b", "C", "d"):
        out[k] = out[k] * (1 + 1e-15 * rng.standard_normal(out[k].shape))
    return out


def oracle_lp(kw, dual, **solve_kw):
    """the oracle's LPSolver on kw; dual: its infeasible-start direction replaced by the restatement
    (phase 1 stays on Cholesky)"""
    s = O.LPSolver(**kw)
    if dual:
        ns = s.ns
        ns.direction = lambda x, v, g: eq_direction(ns.fm, ns.A, ns.b, x, v, g)
    s.solve(**solve_kw)
    return s


def short_reference(shape):
    """the oracle's Cholesky solve of a generated case cut at SHORT_OUTER barrier iterations, with its spread:
    dict(solver, xbar = max(1e-9, 4 x the largest relative move of x* over two perturbed re-runs), stable)"""
    def run():
        kw = generated(*shape)
        a = oracle_lp(copy_kw(kw), False, max_outer_iters=SHORT_OUTER)
        spread, stable = 0.0, True
        for seed in (11, 12):
            q = oracle_lp(perturbed(kw, seed), False, max_outer_iters=SHORT_OUTER)
            spread = max(spread, float(np.linalg.norm(q.xstar - a.xstar) / np.linalg.norm(a.xstar)))
            stable = stable and list(q.inner_iters) == list(a.inner_iters)
        return {"solver": a, "kw": kw, "spread": spread, "xbar": max(1e-9, 4 * spread), "stable": stable}
    return _memo(("short", shape), run)
