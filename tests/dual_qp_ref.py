"""The dual-form QP Newton step on a factored P = diag(rho) + F^T F (QPSolver(P_factor=F, P_diag=rho,
linear_solve_method='cholesky_dual'), IPM_SOLVE_CHOLESKY_DUAL_QP): NumPy restatement, long-double reference,
instances and the error bound shared by test_dual_qp_ref.py (CPU) and the GPU tests test_gpu_dual_qp_step.py /
test_gpu_dual_qp_solve.py.

For the QP barrier with rows C x <= d and box bounds, at barrier parameter t,

    H = diag(D) + M^T diag(W) M,    M = [C; F],   W = [w; t 1_k],
    w = 1/(s_C + 1e-15)^2,   D = t rho + 1/s_lb^2 + 1/s_ub^2 (+ psd add, on D only),

and the device takes the step H dx = -g in its dual form of order m + k:

    E = 1/D,   K = diag(1/W) + M diag(E) M^T,   z = K^-1 M (E o -g),   dx = E o (-g - M^T z),

followed by three rounds of iterative refinement: rho_x = -g - (D o dx + M^T (W o (M dx))) (H applied, never
formed), z' = K^-1 M (E o rho_x), dx += E o (rho_x - M^T z').  P is never formed on the device.

  * ``dual_qp_direction`` restates exactly that in fp64.
  * ``reference_step`` solves H dx = -g with H formed in long double from F, rho, C (dual_ref.reference_solve).
  * ``bound`` is dual_ref's B with M and W:  B = 64 eps ( cond2(H) ||dx||_2 + || E o (|g| + |M|^T |z|) ||_2 ),
    z = W o (M dx).  It is not a theorem for the dual form: test_dual_qp_ref.py holds the fp64 restatement to
    B / 4 on every state, the device is then held to B.

States: C / d / x_f of ipm355.problems.lp_ineq_box (seeded), F and q ~ U(-2, 2), at the shapes (n, m, k) of SHAPES
(m = 0 and k = 0; m inside, at and across a 64-row tile of the stacked operand; the 32-column stage; the K-split
plan of the assembly), the bound sets {both, lb only, none}, rho in {ones, 10^U(-3, 3), the same with every other
entry 0, absent} (the last two only with a bound: D must be positive), t in {1, 1e3, 1e6} and the points 0, 0.9
and 0.999 of the way from x_f to the boundary along a seeded direction.
"""
import numpy as np
import scipy.linalg

import dual_ref as D
from dual_ref import EPS, LD, O, problems

SHAPES = [(1, 0, 1), (2, 1, 1), (17, 5, 3), (33, 0, 7), (33, 31, 33), (64, 63, 1), (65, 64, 64), (40, 12, 0),
          (130, 97, 31), (257, 64, 65), (300, 40, 20), (520, 127, 130)]
BOUNDS = {"both": (-3.0, 3.0), "lb": (-3.0, None), "none": (None, None)}
RHOS = ["ones", "log", "half0", "absent"]
TS, FRACS = D.TS, D.FRACS
REFINE = 3          # the engine's DUAL_REFINE
MARGIN = D.MARGIN
_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def rhos_for(bounds):
    """rho with zeros (or absent) needs a bound: without one D = t rho must be positive by itself"""
    return RHOS if bounds != "none" else RHOS[:2]


def groups():
    return [(n, m, k, b, r) for (n, m, k) in SHAPES for b in BOUNDS for r in rhos_for(b)]


def states():
    return [(n, m, k, b, r, t, f) for (n, m, k, b, r) in groups() for t in TS for f in FRACS]


def state_id(s):
    n, m, k, b, r, t, f = s
    return f"n{n}-m{m}-k{k}-{b}-{r}-t{t:g}-f{f:g}"


class Instance:
    """F (k x n), rho, q, C (m x n), d, one bound set and a point frac of the way to the boundary; C / F are
    None when m / k is 0, rho is None when absent"""

    def __init__(self, n, m, k, bounds, rho, frac):
        seed = 2000 + 7 * n + 3 * m + k
        base = problems.lp_ineq_box(n, m, seed=seed, with_xf=True)
        self.n, self.m, self.k, self.bounds, self.rho_kind, self.frac = n, m, k, bounds, rho, frac
        self.C = base["C"] if m > 0 else None
        self.d = base["d"] if m > 0 else None
        xf = base["xf"]
        rng = np.random.default_rng(seed + 3)
        F = rng.uniform(-2, 2, size=(k, n))
        self.F = F if k > 0 else None
        self.q = rng.uniform(-2, 2, size=n)
        r = 10.0 ** rng.uniform(-3, 3, size=n)
        if rho == "ones":
            self.rho = np.ones(n)
        elif rho == "log":
            self.rho = r
        elif rho == "half0":
            self.rho = r.copy()
            self.rho[1::2] = 0.0
        else:
            self.rho = None
        lo, hi = BOUNDS[bounds]
        self.lb = None if lo is None else np.full(n, lo)
        self.ub = None if hi is None else np.full(n, hi)
        u = np.random.default_rng(seed + 1).normal(size=n)
        s0, ds = [np.zeros(0)], [np.zeros(0)]
        if m > 0:
            s0.append(self.d - self.C @ xf)
            ds.append(-(self.C @ u))
        if self.ub is not None:
            s0.append(self.ub - xf)
            ds.append(-u)
        if self.lb is not None:
            s0.append(xf - self.lb)
            ds.append(u)
        s0, ds = np.concatenate(s0), np.concatenate(ds)
        if len(ds) and not (ds < 0).any():
            u, ds = -u, -ds
        with np.errstate(divide="ignore"):
            reach = np.where(ds < 0, s0 / -ds, np.inf)
        # (no constraint at all: any point is interior; the grid's three points are x_f + frac u)
        self.amax = float(reach.min()) if len(reach) and np.isfinite(reach.min()) else 1.0
        self.x = xf + frac * self.amax * u

    def dense_P(self):
        """diag(rho) + F^T F formed on the host in fp64: what the dense solvers are given"""
        P = self.F.T @ self.F if self.F is not None else np.zeros((self.n, self.n))
        if self.rho is not None:
            P[np.diag_indices(self.n)] += self.rho
        return P

    def oracle(self, t):
        fm = O.QPBarrier(P=self.dense_P(), q=self.q, C=self.C, d=self.d, x0=self.x.copy(), lb=self.lb, ub=self.ub,
                         t=1, n=self.n)
        fm.update_x(self.x.copy())
        fm.update_t(t)
        return fm

    def device(self, factored=True):
        import ipm355
        kw = dict(q=self.q, C=self.C, d=self.d, x0=self.x.copy(), lower_bound=self.lb, upper_bound=self.ub, t=1)
        if factored:   # (an absent rho / F stays NULL in the descriptor: the method is named explicitly)
            return ipm355.FunctionManagerQP(P_factor=self.F, P_diag=self.rho,
                                            solve_method=ipm355._lib.SOLVE_CHOLESKY_DUAL_QP, **kw)
        return ipm355.FunctionManagerQP(P=self.dense_P(), **kw)


def instance(n, m, k, bounds, rho, frac):
    return _memo(("inst", n, m, k, bounds, rho, frac), lambda: Instance(n, m, k, bounds, rho, frac))


# ------------------------------------------------------------------ the step, three ways
def stacked(C, F, n):
    return np.vstack([C if C is not None else np.zeros((0, n)), F if F is not None else np.zeros((0, n))])


def hessian_vectors(fm, rho, t, add=0.0):
    """(w, D) of H = diag(D) + [C; F]^T diag([w; t]) [C; F] at the manager's slack state (+ the psd add on D)"""
    n = len(fm.x)
    w = fm._inv()[fm.seg_C] ** 2 if fm.C is not None else np.zeros(0)
    Dv = np.zeros(n)
    if fm.lb is not None:
        Dv = Dv + 1 / (fm.slacks[fm.seg_lb]) ** 2
    if fm.ub is not None:
        Dv = Dv + 1 / (fm.slacks[fm.seg_ub]) ** 2
    Dv = Dv + add
    if rho is not None:
        Dv = Dv + t * rho
    return w, Dv


def dual_qp_direction(fm, F, rho, t, g, add=0.0, refine=REFINE):
    """the fp64 restatement of the device's dual-form QP step at the manager's slack state"""
    n = len(fm.x)
    w, Dv = hessian_vectors(fm, rho, t, add)
    M = stacked(fm.C, F, n)
    W = np.concatenate([w, np.full(len(M) - len(w), float(t))])
    E = 1 / Dv
    K = (M * E) @ M.T
    K[np.diag_indices(len(W))] += 1 / W
    L = scipy.linalg.cho_factor(K, lower=True, check_finite=False)
    z = scipy.linalg.cho_solve(L, M @ ((-E) * g), check_finite=False)
    dx = E * (-g - M.T @ z)
    for _ in range(refine):
        rx = -g - (Dv * dx + M.T @ (W * (M @ dx)))            # H applied, never formed
        z = scipy.linalg.cho_solve(L, M @ (E * rx), check_finite=False)
        dx = dx + E * (rx - M.T @ z)
    return dx


def _ld_gram(inst):
    """F^T F in long double: one per shape (F does not depend on the bound set, rho or the point)"""
    def run():
        if inst.F is None:
            return np.zeros((inst.n, inst.n), LD)
        F = inst.F.astype(LD)
        return F.T @ F
    return _memo(("gram", inst.n, inst.m, inst.k), run)


def _ld_cwc(inst):
    """C^T diag(w) C in long double at the instance's point: shared by every t and rho"""
    def run():
        if inst.C is None:
            return np.zeros((inst.n, inst.n), LD)
        fm = inst.oracle(1.0)
        w = fm._inv()[fm.seg_C] ** 2
        C = inst.C.astype(LD)
        return (C.T * w.astype(LD)) @ C
    return _memo(("cwc", inst.n, inst.m, inst.k, inst.bounds, inst.frac), run)


def ld_hessian(inst, t, add=0.0):
    fm = inst.oracle(t)
    _, Dv = hessian_vectors(fm, None, t, add)
    H = LD(t) * _ld_gram(inst) + _ld_cwc(inst)
    dg = Dv.astype(LD)
    if inst.rho is not None:
        dg = dg + LD(t) * inst.rho.astype(LD)
    H[np.diag_indices(inst.n)] += dg
    return H


def bound(M, E, g, z, dx, cond2):
    """B = 64 eps ( cond2(H) ||dx|| + || E o (|g| + |M|^T |z|) || ): dual_ref.bound with M and W"""
    return D.bound(M, E, g, z, dx, cond2)


def reference_step(state, add=0.0):
    """dict(dx (fp64 rounding of the refined long-double solve), g, bound, cond2, inst) for one state"""
    n, m, k, bounds, rho, t, frac = state

    def run():
        inst = instance(n, m, k, bounds, rho, frac)
        fm = inst.oracle(t)
        g = fm.gradient().copy()
        H = ld_hessian(inst, t, add)
        H64 = H.astype(np.float64)
        lu = scipy.linalg.lu_factor(H64, check_finite=False)
        cond2 = float(np.linalg.cond(H64))
        dx = D.reference_solve(H, lu, -g, cond2)
        w, Dv = hessian_vectors(fm, inst.rho, t, add)
        M = stacked(inst.C, inst.F, n)
        W = np.concatenate([w, np.full(len(M) - len(w), float(t))])
        z = (W.astype(LD) * (M.astype(LD) @ dx)).astype(np.float64)
        dx = dx.astype(np.float64)
        return {"dx": dx, "g": g, "cond2": cond2, "bound": bound(M, 1 / Dv, g, z, dx, cond2), "inst": inst}
    return _memo(("step", state, add), run)


# ------------------------------------------------------------------ the oracle's line search
def replay_line_search(fm, x0, dx, g, alpha, beta, K=0):
    """FeasibleNewton.backtrack (NewtonSolver.py:157-206) decision by decision, as dual_ref.oracle_line_search
    (an unconstrained problem has no slacks: every point is feasible) -> dict(step, feas_margin, armijo_margin,
    decisive).  Leaves fm at x0."""
    con = fm.constrained
    smax = float(np.abs(fm.slacks).max()) if con else 1.0
    fx = fm.newton_objective()
    gc = g.dot(x0)
    st = 1
    fm.update_x(x0 + st * dx)
    feas = [float(np.abs(fm.slacks).min()) / smax] if con else [1.0]
    floor = False
    while con and (fm.slacks < 0).any():
        st *= beta
        if st < O.STEP_FLOOR:
            floor = True
            break
        fm.update_x(x0 + st * dx)
        feas.append(float(np.abs(fm.slacks).min()) / smax)
    arm = []
    attempt = 0
    while not floor:
        f = fm.newton_objective()
        rhs = fx + alpha * st * gc
        arm.append(abs(float(f - rhs)) / max(1.0, abs(float(fx))))
        if not f > rhs:
            break
        attempt += 1
        nxt = x0 + st * dx
        if st < O.STEP_FLOOR:
            floor = True
            break
        st *= beta
        fm.update_x(nxt, update_slacks=(K > 0 and attempt % K == K - 1))
    fm.update_x(x0.copy())
    fmn, am = min(feas), (min(arm) if arm else 0.0)
    return {"step": st, "feas_margin": fmn, "armijo_margin": am,
            "decisive": (not floor) and fmn >= MARGIN and am >= MARGIN}


def oracle_line_search(state, alpha=0.2, beta=0.6):
    """one FeasibleNewton step of the dense Cholesky oracle (host-formed P) from the state's point, replayed"""
    n, m, k, bounds, rho, t, frac = state

    def run():
        inst = instance(n, m, k, bounds, rho, frac)
        fm = inst.oracle(t)
        x0 = inst.x.copy()
        g = fm.gradient(x0).copy()
        H = np.array(fm.hessian(), dtype=np.float64, copy=True)
        dx = scipy.linalg.cho_solve(scipy.linalg.cho_factor(H, check_finite=False), -g, check_finite=False)
        return replay_line_search(fm, x0, dx, g, alpha, beta)
    return _memo(("ls", state, alpha, beta), run)


def restated_line_search(state, alpha=0.2, beta=0.6):
    n, m, k, bounds, rho, t, frac = state
    inst = instance(n, m, k, bounds, rho, frac)
    fm = inst.oracle(t)
    x0 = inst.x.copy()
    g = fm.gradient(x0).copy()
    dx = dual_qp_direction(fm, inst.F, inst.rho, t, g)
    return replay_line_search(fm, x0, dx, g, alpha, beta)


# ------------------------------------------------------------------ full oracle solves
TIGHT = dict(t0=1, mu=15, epsilon=1e-6)
# (n, m, k, rho of problems.qp_factor_box, bound override, solver kwargs): iteration lists of the oracle with the
# restatement equal the dense Cholesky oracle's on every one of these (test_dual_qp_ref.py checks it)
SOLVES = [(64, 16, 8, "ones", {}, {}), (200, 50, 0, "pow2", {}, {}), (300, 40, 20, "ones", {"upper_bound": None}, {}),
          (257, 0, 33, "ones", {}, {}), (96, 24, 100, "ones", {}, {}),
          (64, 16, 8, "ones", {}, TIGHT), (200, 50, 0, "pow2", {}, TIGHT),
          (300, 40, 20, "ones", {"upper_bound": None}, TIGHT), (257, 0, 33, "ones", {}, TIGHT),
          (96, 24, 100, "ones", {}, TIGHT), (130, 40, 12, "pow2", {}, TIGHT)]


# Outside the exact-list set: at the oracle's default kwargs (epsilon 1e-10) this instance spends eight barrier
# iterations at the inner cap of 50 and the restatement's last inner count is 5 against the dense oracle's 4 (its
# x* stays inside the oracle's own spread, 2.0e-6 against 3.5e-6): held to the x* and value bars only.  (130, 40,
# 12) at the default epsilon is chaotic in the same way and is not a case at all.
NOT_EXACT = {"n96-m24-k100-ones"}


def solve_id(c):
    n, m, k, rho, bnd, kw = c
    return f"n{n}-m{m}-k{k}-{rho}{'-lb' if bnd else ''}{'-tight' if kw else ''}"


def generated(case):
    """(factored kwargs for ipm355.QPSolver, dense kwargs for the oracle / the dense device solver)"""
    n, m, k, rho, bnd, kw = case
    inst = dict(problems.qp_factor_box(n, m, k, seed=5, rho=rho), **bnd)
    fac = dict(inst, **kw)
    F, r = inst["P_factor"], inst["P_diag"]
    P = (F.T @ F if F is not None else np.zeros((n, n)))
    P[np.diag_indices(n)] += r
    dense = {key: v for key, v in fac.items() if key not in ("P_factor", "P_diag")}
    dense["P"] = P
    return fac, dense


def copy_kw(kw):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


def oracle_qp(dense, factors=None, **solve_kw):
    """the oracle's QPSolver on the host-formed dense P; factors = (F, rho): its Newton direction replaced by the
    restatement and its objective and objective gradient by the factored forms rho o x + F^T (F x) (phase 1
    stays on the oracle's Cholesky: it does not involve P)"""
    s = O.QPSolver(**copy_kw(dense))
    if factors is not None:
        F, rho = factors
        fm, ns = s.fm, s.ns

        def Px(x):
            v = rho * x if rho is not None else np.zeros(len(x))
            return v + F.T @ (F @ x) if F is not None else v

        def objective(x=None):
            if x is not None:
                fm.update_x(x)
            elif not fm.dirty_obj:
                return fm.obj
            val = 1 / 2 * fm.x.dot(Px(fm.x))
            if fm.q is not None:
                val += fm.q.dot(fm.x)
            fm.obj = val
            fm.dirty_obj = False
            return val

        def objective_gradient():
            g = Px(fm.x)
            if fm.q is not None:
                g += fm.q
            g *= fm.t
            return g
        fm.objective = objective
        fm._objective_gradient = objective_gradient
        ns.direction = lambda g: dual_qp_direction(fm, F, rho, fm.t, g)
    s.solve(**solve_kw)
    return s


def solve_reference(case):
    """the oracle's dense Cholesky solve of a SOLVES case with its spread under a 1e-15 relative perturbation of
    q: dict(solver, fac, dense, spread, xbar = max(1e-6, 4 x spread), stable)"""
    def run():
        fac, dense = generated(case)
        a = oracle_qp(dense)
        spread, stable = 0.0, True
        for seed in (11, 12):
            pk = copy_kw(dense)
            pk["q"] = pk["q"] * (1 + 1e-15 * np.random.default_rng(seed).standard_normal(pk["q"].shape))
            b = oracle_qp(pk)
            spread = max(spread, float(np.linalg.norm(b.xstar - a.xstar) / np.linalg.norm(a.xstar)))
            stable = stable and list(b.inner_iters) == list(a.inner_iters) and \
                list(b.phase1_iters) == list(a.phase1_iters)
        return {"solver": a, "fac": fac, "dense": dense, "spread": spread, "xbar": max(1e-6, 4 * spread),
                "stable": stable}
    return _memo(("solve", solve_id(case)), run)
