"""The dual-form QP Newton step on a factored P = diag(rho) + F^T F WITH equality rows (QPSolver(P_factor=F,
P_diag=rho, A=A, b=b, linear_solve_method='cholesky_dual_eq'), IPM_SOLVE_CHOLESKY_DUAL_QP_EQ): NumPy restatement,
long-double reference, instances and the error bound shared by test_dual_qp_eq_ref.py (CPU) and the GPU tests
test_gpu_dual_qp_eq_step.py / test_gpu_dual_qp_eq_solve.py.  Built on dual_qp_ref (the factored H) and dual_eq_ref
(the equality rows, the residual line search).

Infeasible-start Newton (NewtonSolverInfeasibleStart.py:386-511) with w, D, E and W of dual_qp_ref:

    H dx + A^T nu = -g,   A dx = -(A x - b),   dv = nu - v,    H = diag(D) + Mc^T diag(W) Mc,   Mc = [C; F]
    M = [C; F; A],   y = [z; nu],   z = W o (Mc dx)
    K = diag([1/W; 0_p]) + M diag(E) M^T                       (order m + k + p)
    K y = [Mc (E o -g); A (E o -g) + (A x - b)],     dx = E o (-g - M^T y)
    refinement, three rounds, on the residual of the full KKT system (W+ = [w; t 1_k; 1_p]):
      rho_x = -g - (D o dx + M^T (W+ o [Mc dx; nu])),    rho_p = -(A x - b) - A dx
      y' = K^-1 [Mc (E o rho_x); A (E o rho_x) - rho_p],   dx += E o (rho_x - M^T y'),   nu += nu'

  * ``qe_direction`` restates exactly that in fp64.
  * ``reference_step`` solves [[H, A^T], [A, 0]] with H formed in long double from F, rho and C
    (dual_qp_ref.ld_hessian), refined against the long-double matrix (dual_ref.reference_solve).
  * the bound is dual_eq_ref's: B = 64 eps cond2(KKT) ||[dx; nu]||_2.  test_dual_qp_eq_ref.py holds the fp64
    restatement to B / 4 on every state, the device is then held to B.

States: dual_qp_ref.Instance(n, m, k, bounds, rho, frac) plus a seeded normal A (p x n), a seeded normal v and
b = A (x_f + 0.01 u) (u seeded normal: the states' points are OFF A x = b, at frac = 0 too), at SHAPES x the bound
sets {both, lb only, none} x rho in {ones, 10^U(-3, 3), every other entry 0, absent} (the last two only with a
bound) x t in {1, 1e3, 1e6} x the points 0, 0.9, 0.999 of the way to the boundary: 900 states.
"""
import numpy as np
import scipy.linalg

import dual_eq_ref as E
import dual_qp_ref as Q
import dual_ref as D
from dual_ref import EPS, LD, O, problems

# (n, m, k, p): the smallest case; all three blocks inside one 64-row tile; no C and one budget row; k = 0 (rho
# only); the first seam on a tile edge; the second seam on a tile edge; a tile straddling both seams; every block a
# whole tile; none a whole tile over several tiles; the K split of the assembly (n > 512)
SHAPES = [(2, 1, 1, 1), (17, 3, 5, 2), (33, 0, 7, 1), (33, 31, 0, 3), (65, 64, 1, 1), (64, 40, 24, 17),
          (130, 63, 2, 30), (129, 64, 64, 64), (257, 129, 65, 33), (520, 127, 130, 65)]
BOUNDS, RHOS, TS, FRACS = Q.BOUNDS, Q.RHOS, Q.TS, Q.FRACS
REFINE = 3          # the engine's DUAL_REFINE
MARGIN = D.MARGIN
UNDECIDED_CAP = 0.02   # the share of states the oracle's line search may leave undecided
_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def groups():
    return [(n, m, k, p, b, r) for (n, m, k, p) in SHAPES for b in BOUNDS for r in Q.rhos_for(b)]


def states():
    return [g + (t, f) for g in groups() for t in TS for f in FRACS]


def state_id(s):
    n, m, k, p, b, r, t, f = s
    return f"n{n}-m{m}-k{k}-p{p}-{b}-{r}-t{t:g}-f{f:g}"


class QEInstance:
    """dual_qp_ref.Instance with p seeded equality rows; its point x is off A x = b"""

    def __init__(self, n, m, k, p, bounds, rho, frac):
        self.base = Q.instance(n, m, k, bounds, rho, frac)
        self.n, self.m, self.k, self.p, self.bounds, self.frac = n, m, k, p, bounds, frac
        seed = 2000 + 7 * n + 3 * m + k                    # (dual_qp_ref.Instance's: the same x_f)
        xf = problems.lp_ineq_box(n, m, seed=seed, with_xf=True)["xf"]
        rng = np.random.default_rng(seed + 5 + p)
        self.A = rng.normal(size=(p, n))
        self.b = self.A @ (xf + 0.01 * rng.normal(size=n))
        self.v = rng.normal(size=p)
        for key in ("F", "rho", "q", "C", "d", "lb", "ub", "x"):
            setattr(self, key, getattr(self.base, key))

    def dense_P(self):
        return self.base.dense_P()

    def oracle(self, t):
        return self.base.oracle(t)

    def device(self, factored=True, solve_method=None):
        import ipm355
        kw = dict(q=self.q, A=self.A, b=self.b, C=self.C, d=self.d, x0=self.x.copy(), lower_bound=self.lb,
                  upper_bound=self.ub, t=1)
        if factored:   # (an absent rho / F stays NULL in the descriptor: the method is named explicitly)
            return ipm355.FunctionManagerQP(P_factor=self.F, P_diag=self.rho,
                                            solve_method=ipm355._lib.SOLVE_CHOLESKY_DUAL_QP_EQ, **kw)
        return ipm355.FunctionManagerQP(P=self.dense_P(), **kw)


def instance(n, m, k, p, bounds, rho, frac):
    return _memo(("inst", n, m, k, p, bounds, rho, frac), lambda: QEInstance(n, m, k, p, bounds, rho, frac))


# ------------------------------------------------------------------ the step, three ways
def qe_direction(fm, F, rho, A, b, x, v, t, g, add=0.0, refine=REFINE):
    """the fp64 restatement of the device's step at the manager's slack state -> (dx, dv)"""
    n, p = len(fm.x), len(b)
    w, Dv = Q.hessian_vectors(fm, rho, t, add)
    Mc = Q.stacked(fm.C, F, n)
    mc = len(Mc)
    W = np.concatenate([w, np.full(mc - len(w), float(t))])
    Wp = np.concatenate([W, np.ones(p)])
    M = np.vstack([Mc, A])
    Ev = 1 / Dv
    K = (M * Ev) @ M.T
    K[np.arange(mc), np.arange(mc)] += 1 / W
    axb = A @ x - b
    r = M @ (Ev * (-g))
    r[mc:] = r[mc:] - (-axb)
    L = scipy.linalg.cho_factor(K, lower=True, check_finite=False)
    y = scipy.linalg.cho_solve(L, r, check_finite=False)
    nu = y[mc:].copy()
    dx = Ev * (-g - M.T @ y)
    for _ in range(refine):
        s = M @ dx
        adx = s[mc:].copy()
        s[mc:] = nu
        rho_x = -g - (Dv * dx + M.T @ (Wp * s))            # H and A^T nu in one transposed product
        r = M @ (Ev * rho_x)
        r[mc:] = r[mc:] - (-axb - adx)
        y = scipy.linalg.cho_solve(L, r, check_finite=False)
        dx = dx + Ev * (rho_x - M.T @ y)
        nu = nu + y[mc:]
    return dx, nu - v


def oracle_direction(fm, A, b, x, v, g, add=0.0):
    """the Cholesky block elimination of oracle.InfeasibleNewton.direction on the host-formed dense P"""
    return E.oracle_direction(fm, A, b, x, v, g, add)


def reference_step(state, add=0.0):
    """dict(sol = [dx; nu] (fp64 rounding of the refined long-double solve), g, bound, cond2, inst)"""
    n, m, k, p, bounds, rho, t, frac = state

    def run():
        inst = instance(n, m, k, p, bounds, rho, frac)
        fm = inst.oracle(t)
        g = fm.gradient().copy()
        Kk = np.zeros((n + p, n + p), LD)
        Kk[:n, :n] = Q.ld_hessian(inst.base, t, add)
        Kk[:n, n:] = inst.A.T.astype(LD)
        Kk[n:, :n] = inst.A.astype(LD)
        K64 = Kk.astype(np.float64)
        lu, cond2 = scipy.linalg.lu_factor(K64, check_finite=False), float(np.linalg.cond(K64))
        rhs = np.concatenate([-g, -(inst.A @ inst.x - inst.b)])
        sol = D.reference_solve(Kk, lu, rhs, cond2).astype(np.float64)
        return {"sol": sol, "g": g, "cond2": cond2, "bound": 64 * EPS * cond2 * float(np.linalg.norm(sol)),
                "inst": inst}
    return _memo(("step", state, add), run)


joint_error = E.joint_error      # ||[dx; v + dv] - reference|| / B


# ------------------------------------------------------------------ the oracle's residual line search
def replay_line_search(fm, A, b, x0, v, dx, dv, g, alpha, beta, K=0):
    """dual_eq_ref.replay_line_search; a problem without any slack (no C, no bound) has no feasibility loop:
    the residual tests alone, every candidate feasible"""
    if fm.constrained:
        return E.replay_line_search(fm, A, b, x0, v, dx, dv, g, alpha, beta, K)
    ATv, ATdv, Axb, Adx = A.T @ v, A.T @ dv, A @ x0 - b, A @ dx
    r = np.linalg.norm(np.append(g + ATv, Axb))
    step, res, floor = 1, [], False
    while True:
        fm.update_x(x0 + step * dx)
        rn = np.linalg.norm(np.append(fm.gradient() + ATv + step * ATdv, Axb + step * Adx))
        rhs = (1 - alpha * step) * r
        res.append(abs(float(rn - rhs)) / max(1.0, float(r)))
        if not rn > rhs:
            break
        step *= beta
        if step < O.STEP_FLOOR:
            floor = True
            break
    fm.update_x(x0.copy())
    return {"step": step, "feas_margin": 1.0, "res_margin": min(res), "decisive": (not floor) and min(res) >= MARGIN}


def oracle_line_search(state, alpha=0.2, beta=0.6):
    """one InfeasibleNewton step of the dense Cholesky oracle from the state's point (v the instance's), replayed"""
    n, m, k, p, bounds, rho, t, frac = state

    def run():
        inst = instance(n, m, k, p, bounds, rho, frac)
        fm = inst.oracle(t)
        x0 = inst.x.copy()
        g = fm.gradient(x0).copy()
        dx, dv = oracle_direction(fm, inst.A, inst.b, x0, inst.v, g)
        return replay_line_search(fm, inst.A, inst.b, x0, inst.v, dx, dv, g, alpha, beta)
    return _memo(("ls", state, alpha, beta), run)


def restated_line_search(state, alpha=0.2, beta=0.6):
    n, m, k, p, bounds, rho, t, frac = state
    inst = instance(n, m, k, p, bounds, rho, frac)
    fm = inst.oracle(t)
    x0 = inst.x.copy()
    g = fm.gradient(x0).copy()
    dx, dv = qe_direction(fm, inst.F, inst.rho, inst.A, inst.b, x0, inst.v, t, g)
    return replay_line_search(fm, inst.A, inst.b, x0, inst.v, dx, dv, g, alpha, beta)


# ------------------------------------------------------------------ full oracle solves
# (n, m, k, p, rho of problems.qp_factor_eq_box): a budget-like single row, no C, k = 0, and two general ones
SOLVES = [(64, 16, 8, 4, "ones"), (120, 0, 10, 1, "ones"), (96, 24, 12, 8, "pow2"), (200, 50, 0, 20, "pow2"),
          (257, 40, 33, 30, "ones")]


def solve_id(c):
    return "n%d-m%d-k%d-p%d-%s" % c


def generated(case):
    """(factored kwargs for ipm355.QPSolver, dense kwargs for the oracle / the dense device solver)"""
    n, m, k, p, rho = case
    fac = dict(problems.qp_factor_eq_box(n, m, k, p, seed=5, grid=True, rho=rho), **problems.QP_KWARGS)
    F, r = fac["P_factor"], fac["P_diag"]
    P = (F.T @ F if F is not None else np.zeros((n, n)))
    P[np.diag_indices(n)] += r
    dense = {key: v for key, v in fac.items() if key not in ("P_factor", "P_diag")}
    dense["P"] = P
    return fac, dense


def oracle_qp(dense, factors=None, **solve_kw):
    """the oracle's QPSolver on the host-formed dense P; factors = (F, rho): its infeasible-start direction
    replaced by the restatement (phase 1 stays on the oracle's Cholesky: it involves neither P nor A)"""
    s = O.QPSolver(**Q.copy_kw(dense))
    if factors is not None:
        F, rho = factors
        ns = s.ns
        ns.direction = lambda x, v, g: qe_direction(ns.fm, F, rho, ns.A, ns.b, x, v, ns.fm.t, g)
    s.solve(**solve_kw)
    return s


def common_prefix(*lists):
    n = 0
    while all(len(l) > n for l in lists) and len({l[n] for l in lists}) == 1:
        n += 1
    return n


def solve_reference(case):
    """the oracle's dense Cholesky solve of a SOLVES case with its envelope under a 1e-15 relative perturbation of
    q and b: dict(solver, fac, dense, spread, xbar = max(1e-6, 4 x spread), cut: the number of leading barrier
    iterations whose inner counts the perturbation leaves unchanged)"""
    def run():
        fac, dense = generated(case)
        a = oracle_qp(dense)
        spread, lists = 0.0, [list(a.inner_iters)]
        for seed in (11, 12):
            pk = Q.copy_kw(dense)
            rng = np.random.default_rng(seed)
            for key in ("q", "b"):
                pk[key] = pk[key] * (1 + 1e-15 * rng.standard_normal(pk[key].shape))
            bsol = oracle_qp(pk)
            spread = max(spread, float(np.linalg.norm(bsol.xstar - a.xstar) / np.linalg.norm(a.xstar)))
            lists.append(list(bsol.inner_iters))
        return {"solver": a, "fac": fac, "dense": dense, "spread": spread, "xbar": max(1e-6, 4 * spread),
                "cut": common_prefix(*lists)}
    return _memo(("solve", solve_id(case)), run)


# the cuts solve_reference found on the CPU (recorded as dual_eq_ref's SHORT_OUTER is): the tests compare
# iteration lists up to the smaller of this and the cut the oracle's envelope gives on the host they run on
CUTS = {"n64-m16-k8-p4-ones": 10, "n120-m0-k10-p1-ones": 9, "n96-m24-k12-p8-pow2": 6, "n200-m50-k0-p20-pow2": 9,
        "n257-m40-k33-p30-ones": 9}
