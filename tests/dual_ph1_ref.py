"""The dual-form PHASE-1 Newton step (PhaseOneSolver(linear_solve_method='cholesky_dual'), engine method
IPM_SOLVE_CHOLESKY_DUAL_PHASE1): NumPy restatement, long-double reference, states and the error bound
shared by test_dual_ph1_ref.py (CPU) and test_gpu_dual_ph1_step.py.

The phase-1 barrier in x~ = (x, s) over sigma = [s + d - C x | s + ub - x | s + x - lb] has the Hessian

    H~ = [[ Hxx , h  ],     Hxx = diag(D) + C^T diag(w) C,    D = inv_lb^2 + inv_ub^2 (+ add),  w = inv_C^2
          [ h^T , hss]]     h   = -C^T w + inv_lb^2 - inv_ub^2,   hss = sum inv^2 (+ add),  inv = 1/(sigma + 1e-15)

Hxx is the positive-diagonal-plus-rank-m matrix of the phase-2 dual step (tests/dual_ref.py); s is one
bordering column.  With E = 1/D and ONE Cholesky of S = diag(1/w) + C diag(E) C^T the device forms

    [z_u | z_y] = S^-1 C (E o [-g_x | h]),   u = E o (-g_x - C^T z_u),   y = E o (h - C^T z_y)
    sigma = hss - h.y  formed as  sum w (1 + C y)^2 + sum inv_lb^2 (1 - y)^2 + sum inv_ub^2 (1 + y)^2 + add (y.y + 1)
    ds = (-g_s - h.u) / sigma,   dx = u - y ds

(the sum-of-squares form of sigma has no cancellation: y minimizes the quadratic form of H~ over (v, 1), so
its error enters squared.  hss - h.y loses sigma / hss digits -- down to 4.7e-9 on the states below -- and
then the refinement rounds, which divide by the same sigma, diverge: 43 of 360 states up to 2.6e4 x B1)

then `refine` rounds on the residual of the full bordered system (H~ applied through C, y not refined):

    rho_x = -g_x - (D o dx + C^T (w o (C dx))) - h ds,      rho_s = -g_s - h.dx - hss ds
    du = E o (rho_x - C^T S^-1 C (E o rho_x)),   dds = (rho_s - h.du) / sigma,   dx += du - y dds,  ds += dds

  * ``dual_phase1_direction`` restates exactly that in fp64 (the same H~ as oracle.Phase1Barrier.hessian()).
  * ``reference_step`` solves H~ d = -g with H~ formed in long double (dual_ref.reference_solve).
  * the bound is the project's Newton-step allowance B1 = 64 eps cond2(H~) ||d||_2 (tests/barrier_ref.py),
    with no extra term.  test_dual_ph1_ref.py holds the restatement to B1 / 4, the device is held to B1.

States: dual_ref.SHAPES x dual_ref.BOUNDS x t in {0.01, 1, 1e3} x the point x_f + frac * amax * u with
frac in {0, 1.5} (1.5 is past the boundary: phase 1 has work to do) x s = -min(slacks at s = 0) + delta
with delta in {1, 1e-3} (1e-3: close to the boundary of the phase-1 domain).  H~ does not depend on t.
"""
import numpy as np
import scipy.linalg

import dual_ref as D
from dual_ref import EPS, LD, O, problems  # noqa: F401

SHAPES, BOUNDS = D.SHAPES, D.BOUNDS
TS = [0.01, 1.0, 1e3]
FRACS = [0.0, 1.5]
DELTAS = [1.0, 1e-3]
REFINE = D.REFINE       # the engine's DUAL_REFINE, shared by both phases
MARGIN = D.MARGIN
_memo = D._memo


def states():
    return [(n, m, b, t, f, dl) for (n, m) in SHAPES for b in BOUNDS for t in TS for f in FRACS for dl in DELTAS]


def state_id(s):
    n, m, b, t, f, dl = s
    return f"n{n}-m{m}-{b}-t{t:g}-f{f:g}-d{dl:g}"


class Point:
    """the phase-1 start of dual_ref.Instance(n, m, bounds, frac): x~ = (x, -min(slacks at s = 0) + delta)"""

    def __init__(self, n, m, bounds, frac, delta):
        self.inst = inst = D.instance(n, m, bounds, frac)
        self.n, self.m = n, m
        self.C, self.d, self.lb, self.ub = inst.C, inst.d, inst.lb, inst.ub
        fm = O.Phase1Barrier(C=self.C, d=self.d, x0=inst.x.copy(), lb=self.lb, ub=self.ub, t=1)
        self.s = float(fm.s - 1 + delta)            # fm.s = -min(slacks at s = 0) + 1
        self.x = np.append(inst.x, self.s)

    def oracle(self, t):
        fm = O.Phase1Barrier(C=self.C, d=self.d, x0=self.inst.x.copy(), lb=self.lb, ub=self.ub, t=1)
        fm.update_x(self.x.copy())
        fm.update_t(t)
        return fm

    def device(self, solve_method):
        """FunctionManagerPhase1 on the given engine method, moved to this point"""
        import ipm355
        fm = ipm355.FunctionManagerPhase1(C=self.C, d=self.d, x0=self.inst.x.copy(), lower_bound=self.lb,
                                          upper_bound=self.ub, t=1, solve_method=solve_method)
        fm.update_x(self.x.copy())
        return fm


def point(n, m, bounds, frac, delta):
    return _memo(("ph1pt", n, m, bounds, frac, delta), lambda: Point(n, m, bounds, frac, delta))


# ------------------------------------------------------------------ the step
def hessian_pieces(fm, add=0.0):
    """(w, D, h, hss) of H~ exactly as Phase1Barrier.hessian forms them (+ the psd add on all n + 1
    diagonal entries: on D and on hss)"""
    inv2 = fm._inv() ** 2
    w = inv2[fm.seg_C]
    h = -(fm.C.T @ w)
    Dv = np.zeros(len(fm.x))
    if fm.lb is not None:
        Dv = Dv + inv2[fm.seg_lb]
        h = h + inv2[fm.seg_lb]
    if fm.ub is not None:
        Dv = Dv + inv2[fm.seg_ub]
        h = h - inv2[fm.seg_ub]
    return w, Dv + add, h, inv2.sum() + add


def dual_phase1_direction(fm, g, add=0.0, refine=REFINE):
    """the fp64 restatement of the device's dual-form phase-1 step at the manager's slack state"""
    w, Dv, h, hss = hessian_pieces(fm, add)
    C = fm.C
    gx, gs = g[:-1], g[-1]
    E = 1 / Dv
    S = (C * E) @ C.T
    S[np.diag_indices(len(w))] += 1 / w
    L = scipy.linalg.cho_factor(S, lower=True, check_finite=False)
    Z = scipy.linalg.cho_solve(L, C @ np.column_stack([E * -gx, E * h]), check_finite=False)
    u = E * (-gx - C.T @ Z[:, 0])
    y = E * (h - C.T @ Z[:, 1])
    # sigma = hss - h.y, the Schur complement of Hxx in H~, as the device forms it: H~ is a sum of squares
    # over the slack rows and (-y, 1) minimizes its quadratic form over (v, 1), so no cancellation
    inv2 = fm._inv() ** 2
    sigma = (w * (1 + C @ y) ** 2).sum() + add * (y @ y + 1)
    if fm.lb is not None:
        sigma = sigma + (inv2[fm.seg_lb] * (1 - y) ** 2).sum()
    if fm.ub is not None:
        sigma = sigma + (inv2[fm.seg_ub] * (1 + y) ** 2).sum()
    if not (np.isfinite(sigma) and sigma > 0):
        raise np.linalg.LinAlgError("dual phase 1: sigma is not finite and positive")
    ds = (-gs - h @ u) / sigma
    dx = u - y * ds
    for _ in range(refine):
        rx = -gx - (Dv * dx + C.T @ (w * (C @ dx))) - h * ds          # H~ applied, never formed
        rs = -gs - h @ dx - hss * ds
        z = scipy.linalg.cho_solve(L, C @ (E * rx), check_finite=False)
        du = E * (rx - C.T @ z)
        dds = (rs - h @ du) / sigma
        dx = dx + (du - y * dds)
        ds = ds + dds
    return np.append(dx, ds)


def _ld_hessian(fm, add=0.0):
    """H~ in long double from the fp64 vectors inv^2 (what both the oracle and the device start from)"""
    inv2 = (fm._inv() ** 2).astype(LD)
    n = len(fm.x)
    C = fm.C.astype(LD)
    w = inv2[fm.seg_C]
    H = np.zeros((n + 1, n + 1), dtype=LD)
    H[:n, :n] = (C.T * w) @ C
    h = -(C.T @ w)
    dg = np.zeros(n, dtype=LD)
    if fm.lb is not None:
        dg += inv2[fm.seg_lb]
        h = h + inv2[fm.seg_lb]
    if fm.ub is not None:
        dg += inv2[fm.seg_ub]
        h = h - inv2[fm.seg_ub]
    H[np.arange(n), np.arange(n)] += dg + LD(add)
    H[:n, n] = H[n, :n] = h
    H[n, n] = inv2.sum() + LD(add)
    return H


def hessian_ref(pt, add=0.0):
    """(long-double H~, the fp64 LU of its rounding, cond2) at the point: shared by every t"""
    def run():
        H = _ld_hessian(pt.oracle(1.0), add)
        H64 = H.astype(np.float64)
        return H, scipy.linalg.lu_factor(H64, check_finite=False), float(np.linalg.cond(H64))
    return _memo(("ph1H", pt.n, pt.m, pt.inst.bounds, pt.inst.frac, pt.s, add), run)


def reference_step(state, add=0.0):
    """dict(d = (dx, ds) (fp64 rounding of the refined long-double solve), g, cond2, bound = B1, pt)"""
    n, m, bounds, t, frac, delta = state

    def run():
        pt = point(n, m, bounds, frac, delta)
        fm = pt.oracle(t)
        g = fm.gradient().copy()
        H, lu, cond2 = hessian_ref(pt, add)
        d = D.reference_solve(H, lu, -g, cond2).astype(np.float64)
        return {"d": d, "g": g, "cond2": cond2, "bound": 64 * EPS * cond2 * float(np.linalg.norm(d)), "pt": pt}
    return _memo(("ph1step", state, add), run)


# ------------------------------------------------------------------ the oracle's line search
def oracle_line_search(state, alpha=0.2, beta=0.6):
    """dual_ref.oracle_line_search for the phase-1 barrier: one FeasibleNewton step of the Cholesky
    oracle from the state's point with its backtracking replayed decision by decision -> dict(step,
    feas_margin, armijo_margin, decisive: both margins >= MARGIN and the step floor not reached)"""
    n, m, bounds, t, frac, delta = state

    def run():
        pt = point(n, m, bounds, frac, delta)
        fm = pt.oracle(t)
        x0 = pt.x.copy()
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
        return {"step": st, "feas_margin": fm_, "armijo_margin": am, "dx": dx,
                "decisive": (not floor) and fm_ >= MARGIN and am >= MARGIN}
    return _memo(("ph1ls", state, alpha, beta), run)


# ------------------------------------------------------------------ oracle solves
def _copy(kw):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


def _restate(ns, refine):
    ns.direction = lambda g: dual_phase1_direction(ns.fm, g, 1e-9 if ns.use_psd_condition else 0.0, refine)


def oracle_phase_one(kw, dual, refine=REFINE):
    """the oracle's PhaseOne as LPSolver(**kw) builds it; dual: its direction replaced by the restatement.
    Returns the LPSolver (its .phase1 solved: inner_iters, x)"""
    s = O.LPSolver(**_copy(kw))
    if dual:
        _restate(s.phase1.ns, refine)
    s.phase1.solve()
    return s


def oracle_lp(kw, dual, refine=REFINE):
    """the oracle's LPSolver on kw; dual: BOTH phases' directions replaced by the restatements"""
    s = O.LPSolver(**_copy(kw))
    if dual:
        _restate(s.phase1.ns, refine)
        ns = s.ns
        ns.direction = lambda g: D.dual_direction(ns.fm, g, refine=refine)
    s.solve()
    return s
