"""The dual-form LP Newton step (linear_solve_method='cholesky_dual'): NumPy restatement, long-double
reference, instances and the error bound shared by test_dual_ref.py (CPU) and test_gpu_dual_step.py.

For an LP barrier with rows C x <= d and box bounds the Hessian is

    H = diag(D) + C^T diag(w) C,     D = 1/s_lb^2 + 1/s_ub^2 (+ psd add),   w = 1/(s_C + 1e-15)^2

and the device takes the Newton step H dx = -g in its m x m dual form (Sherman-Morrison-Woodbury):

    E = 1/D,   S = diag(1/w) + C diag(E) C^T,   z = S^-1 C (E o -g),   dx = E o (-g - C^T z),

followed by three rounds of iterative refinement: rho = -g - H dx with H applied as diag(D) + C^T diag(w) C
(never formed), dx += E o (rho - C^T S^-1 C (E o rho)).

  * ``dual_direction`` restates exactly that in fp64 (the same H as oracle.LPBarrier.hessian()).
  * ``reference_direction`` solves H dx = -g with H formed in long double: an fp64 LU of the rounded H
    plus iterative refinement whose residual uses the long-double H, run until the corrections stop
    shrinking; the last one must be below 2^-6 eps cond2(H) ||dx|| (1/4096 of B's first term).
  * ``bound`` is

        B = 64 eps ( cond2(H) ||dx||_2 + || E o (|g| + |C|^T |z|) ||_2 )

    the project's Newton-step allowance (tests/barrier_ref.py x_bound) plus the rounding of the last
    combination E o (-g - C^T z), whose terms cancel.  It is not a theorem for the dual form, so
    test_dual_ref.py checks it: the fp64 restatement must stay within a QUARTER of B at every state
    the GPU test uses; the device is then held to B itself.

States: LP instances of ipm355.problems.lp_ineq_box (seeded, x_f strictly feasible) at the shapes
SHAPES, with the bounds (-3, 3), (-3, None), (None, 3), t in {1, 1e3, 1e6}, and the point
x_f + frac * amax * u, frac in {0, 0.9, 0.999}: u a seeded direction and amax the distance to the
boundary along it.  H does not depend on t, so each (shape, bounds, frac) forms its long-double H once.
"""
import os
import sys

import numpy as np
import scipy.linalg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "interiorpoint-gpu_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from ipm355 import problems  # noqa: E402
from oracle import ipm_oracle as O  # noqa: E402

EPS = np.finfo(np.float64).eps
LD = np.longdouble
SHAPES = [(1, 1), (2, 1), (17, 15), (33, 31), (64, 63), (65, 64), (130, 127), (129, 128), (257, 129), (300, 40),
          (520, 257)]
BOUNDS = {"both": (-3.0, 3.0), "lb": (-3.0, None), "ub": (None, 3.0)}
TS = [1.0, 1e3, 1e6]
FRACS = [0.0, 0.9, 0.999]
_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def states():
    return [(n, m, b, t, f) for (n, m) in SHAPES for b in BOUNDS for t in TS for f in FRACS]


def state_id(s):
    n, m, b, t, f = s
    return f"n{n}-m{m}-{b}-t{t:g}-f{f:g}"


class Instance:
    """lp_ineq_box(n, m) with one of the three bound sets and a point frac of the way to the boundary"""

    def __init__(self, n, m, bounds, frac):
        seed = 1000 + 7 * n + m
        inst = problems.lp_ineq_box(n, m, seed=seed, with_xf=True)
        self.n, self.m, self.bounds, self.frac = n, m, bounds, frac
        self.c, self.C, self.d, xf = inst["c"], inst["C"], inst["d"], inst["xf"]
        lo, hi = BOUNDS[bounds]
        self.lb = None if lo is None else np.full(n, lo)
        self.ub = None if hi is None else np.full(n, hi)
        u = np.random.default_rng(seed + 1).normal(size=n)
        # distance to the boundary along u: the first slack of [d - C x | ub - x | x - lb] to reach 0
        s0 = [self.d - self.C @ xf]
        ds = [-(self.C @ u)]
        if self.ub is not None:
            s0.append(self.ub - xf)
            ds.append(-u)
        if self.lb is not None:
            s0.append(xf - self.lb)
            ds.append(u)
        s0, ds = np.concatenate(s0), np.concatenate(ds)
        if not (ds < 0).any():          # (n = 1 with one bound: no slack shrinks along u, but one does along -u)
            u, ds = -u, -ds
        with np.errstate(divide="ignore"):
            reach = np.where(ds < 0, s0 / -ds, np.inf)
        self.amax = float(reach.min())
        self.x = xf + frac * self.amax * u

    def oracle(self, t):
        fm = O.LPBarrier(c=self.c, C=self.C, d=self.d, x0=self.x.copy(), lb=self.lb, ub=self.ub, t=1, try_diag=False)
        fm.update_x(self.x.copy())
        fm.update_t(t)
        return fm

    def device(self, solve_method):
        import ipm355
        return ipm355.FunctionManagerLP(c=self.c, C=self.C, d=self.d, x0=self.x.copy(), lower_bound=self.lb,
                                        upper_bound=self.ub, t=1, try_diag=False, solve_method=solve_method)


def instance(n, m, bounds, frac):
    return _memo(("inst", n, m, bounds, frac), lambda: Instance(n, m, bounds, frac))


# ------------------------------------------------------------------ the step, three ways
def hessian_vectors(fm, add=0.0):
    """(w, D) of H = diag(D) + C^T diag(w) C exactly as LPBarrier.hessian forms them (+ the psd add)"""
    inv = fm._inv()
    w = inv[fm.seg_C] ** 2
    D = np.zeros(len(fm.x))
    if fm.lb is not None:
        D = D + 1 / (fm.slacks[fm.seg_lb]) ** 2
    if fm.ub is not None:
        D = D + 1 / (fm.slacks[fm.seg_ub]) ** 2
    return w, D + add


REFINE = 3     # the engine's DUAL_REFINE


def dual_direction(fm, g, add=0.0, refine=REFINE):
    """the fp64 restatement of the device's dual-form step at the manager's slack state: the
    Woodbury solve, then `refine` rounds of iterative refinement on the primal residual -g - H dx"""
    w, D = hessian_vectors(fm, add)
    C = fm.C
    E = 1 / D
    S = (C * E) @ C.T
    S[np.diag_indices(len(w))] += 1 / w
    r = C @ ((-E) * g)
    L = scipy.linalg.cho_factor(S, lower=True, check_finite=False)
    z = scipy.linalg.cho_solve(L, r, check_finite=False)
    dx = E * (-g - C.T @ z)
    for _ in range(refine):
        rho = -g - (D * dx + C.T @ (w * (C @ dx)))            # H applied, never formed
        z = scipy.linalg.cho_solve(L, C @ (E * rho), check_finite=False)
        dx = dx + E * (rho - C.T @ z)
    return dx


def _ld_hessian(fm, add=0.0):
    w, D = hessian_vectors(fm, add)
    C = fm.C.astype(LD)
    H = (C.T * w.astype(LD)) @ C
    H[np.diag_indices(len(D))] += D.astype(LD)
    return H


def reference_solve(H_ld, lu, b, cond2):
    """H x = b: fp64 LU of the rounded H, refined against the long-double H until the corrections
    stop shrinking (their floor is ~ cond2 eps_longdouble ||x||); the last correction must be below
    2^-6 eps cond2 ||x||, 1/4096 of the bound's first term"""
    b = b.astype(LD)
    x = scipy.linalg.lu_solve(lu, b.astype(np.float64), check_finite=False).astype(LD)
    last = np.inf
    for _ in range(60):
        r = b - H_ld @ x
        dx = scipy.linalg.lu_solve(lu, r.astype(np.float64), check_finite=False).astype(LD)
        x = x + dx
        cur = float(np.linalg.norm(dx.astype(np.float64)))
        if cur == 0.0 or cur >= 0.5 * last:
            break
        last = cur
    if not cur <= 2.0 ** -6 * EPS * cond2 * float(np.linalg.norm(x.astype(np.float64))):
        raise ValueError("the refinement of the long-double reference did not converge")
    return x


def hessian_ref(inst, add=0.0):
    """(long-double H, the fp64 LU of its rounding, cond2) at the instance's point: shared by every t"""
    def run():
        fm = inst.oracle(1.0)
        H = _ld_hessian(fm, add)
        H64 = H.astype(np.float64)
        return H, scipy.linalg.lu_factor(H64, check_finite=False), float(np.linalg.cond(H64))
    return _memo(("H", inst.n, inst.m, inst.bounds, inst.frac, add), run)


def reference_step(state, add=0.0):
    """dict(dx (fp64 rounding of the refined long-double solve), g, bound, cond2, fm) for one state"""
    n, m, bounds, t, frac = state

    def run():
        inst = instance(n, m, bounds, frac)
        fm = inst.oracle(t)
        g = fm.gradient().copy()
        H, lu, cond2 = hessian_ref(inst, add)
        dx = reference_solve(H, lu, -g, cond2)
        w, D = hessian_vectors(fm, add)
        z = (w.astype(LD) * (fm.C.astype(LD) @ dx)).astype(np.float64)     # z = w o (C dx)
        dx = dx.astype(np.float64)
        return {"dx": dx, "g": g, "cond2": cond2, "bound": bound(fm.C, 1 / D, g, z, dx, cond2), "inst": inst}
    return _memo(("step", state, add), run)


def bound(C, E, g, z, dx, cond2):
    """B = 64 eps ( cond2(H) ||dx|| + || E o (|g| + |C|^T |z|) || )"""
    return 64 * EPS * (cond2 * np.linalg.norm(dx) + np.linalg.norm(E * (np.abs(g) + np.abs(C).T @ np.abs(z))))


# ------------------------------------------------------------------ the oracle's line search
MARGIN = 1e-9      # decisiveness of the oracle's own decisions (the convention of barrier_ref.py)


def oracle_line_search(state, alpha=0.2, beta=0.6):
    """One FeasibleNewton step of the Cholesky oracle from the state's point, with its backtracking
    replayed decision by decision (as barrier_ref.reference_newton_step does) -> dict(step,
    feas_margin: min over the feasibility candidates of min|s| / max|s0|, armijo_margin: min over the
    Armijo candidates of |f - (f0 + alpha step g.x)| / max(1, |f0|), decisive: both >= MARGIN and the
    step floor not reached)"""
    n, m, bounds, t, frac = state

    def run():
        inst = instance(n, m, bounds, frac)
        fm = inst.oracle(t)
        x0 = inst.x.copy()
        g = fm.gradient(x0).copy()
        H = np.array(fm.hessian(), dtype=np.float64, copy=True)
        dx = scipy.linalg.cho_solve(scipy.linalg.cho_factor(H, check_finite=False), -g, check_finite=False)
        s0 = np.array(fm.slacks, copy=True)
        smax = float(np.abs(s0).max())
        fx = fm.newton_objective()
        gc = g.dot(x0)
        st = 1
        fm.update_x(x0 + st * dx)
        feas = [float(np.abs(fm.slacks).min()) / smax]
        floor = False
        while (fm.slacks < 0).any():
            st *= beta
            if st < O.STEP_FLOOR:
                floor = True
                break
            fm.update_x(x0 + st * dx)
            feas.append(float(np.abs(fm.slacks).min()) / smax)
        arm = []
        while not floor:
            f = fm.newton_objective()
            rhs = fx + alpha * st * gc
            arm.append(abs(float(f - rhs)) / max(1.0, abs(float(fx))))
            if not f > rhs:
                break
            nxt = x0 + st * dx
            if st < O.STEP_FLOOR:
                floor = True
                break
            st *= beta
            fm.update_x(nxt, update_slacks=False)
        fm_, am = min(feas), (min(arm) if arm else 0.0)
        return {"step": st, "feas_margin": fm_, "armijo_margin": am,
                "decisive": (not floor) and fm_ >= MARGIN and am >= MARGIN}
    return _memo(("ls", state, alpha, beta), run)


# ------------------------------------------------------------------ full oracle solves
def oracle_lp(kw, dual, refine=REFINE):
    """the oracle's LPSolver on kw; dual: its Newton direction replaced by the restatement (phase 1
    stays on Cholesky, as in the facades)"""
    s = O.LPSolver(**kw)
    if dual:
        ns = s.ns
        ns.direction = lambda g: dual_direction(ns.fm, g, refine=refine)
    s.solve()
    return s
