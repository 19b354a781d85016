"""Seeded barrier instances at kernel-edge shapes, long-double references of the LP / QP and the SOCP
barrier with derived entry-wise error bounds, and the decisiveness margins of one reference Newton step.

Shared by tests/test_gpu_barrier_shapes.py (-m gpu: the device managers and one device Newton step
against these) and tests/test_barrier_ref.py (no GPU: the fp64 oracle alone sits far inside the same
bounds and every Newton-step instance is decisive).  A plain module: it reads nothing but its
arguments and the oracle.

Instances (strictly feasible by construction): C normal, x0 ~ U[-0.5, 0.5], d = C x0 + U[0.05, 2],
lb = x0 - U[0.05, 2], ub = x0 + U[0.05, 2], QP P = M M^T / n + 0.1 I, t = 7.  ``tiny`` sets every
7th lower-bound gap to 1e-6 and every 11th upper-bound gap to 1e-7 (bound slacks only): there the
reference's two epsilon conventions (the dense Hessian's bound diagonal 1/s^2 has no epsilon, the
gradient and the diagonal-Hessian vector use 1/(s + 1e-15)) differ by ~1e-9 relative, far above
64 eps, in single entries that a norm would hide.

Error bounds (the convention of tests/test_gpu_kernels.py: fp64 sums of products in another order
differ by at most 64 eps sum|terms|), with inv_i = 1/(s_i + 1e-15):
  slack i (C row)   B_s = 64 eps (|d_i| + sum_j |C_ij x_j|);   bound slacks 4 eps (|x| + |bound|)
  rho_i = B_s / s_i (the relative slack error, which every reciprocal inherits)
  gradient j        64 eps (|t c_j|  or  |t| (|P||x| + |q|)_j,  + 1/s_lb + 1/s_ub + sum_i |C_ij| inv_i)
                    + sum_i |C_ij| inv_i rho_i
  Hessian (j, k)    sum_i |C_ij C_ik| inv_i^2 (64 eps + 2 rho_i) + [j == k] 64 eps (1/s_lb^2 + 1/s_ub^2)
                    + 64 eps |t P_jk|
  barrier objective 64 eps (|t| sum|objective terms| + sum|log(s + 1e-15)|) + sum_i rho_i

SOCP (socp_reference).  Cone i: lhs_i = A_i x + b_i, rhs_i = c_i.x + d_i, s_i = rhs_i^2 - ||lhs_i||^2,
coef_i = 2 / (s_i + 1e-12), g_i = coef_i (A_i^T lhs_i - c_i rhs_i); the bound Hessian diagonal is
1 / (s + 1e-12)^2 and the gradient's bound terms 1 / (s + 1e-15).  Phase 1 shifts the barrier slacks
(cones, bounds) by s, uses inv = 1 / (sigma + 1e-15) throughout (coef_i = 2 inv_i), and appends
hxs = -sum_i g_i inv_i + inv_lb^2 - inv_ub^2, hss = sum inv^2 and the gradient entry t - sum inv.
s_i is a difference of two sums of squares, so near the boundary (s_i = mu rhs_i^2) its absolute
error stays that of rhs_i^2 while s_i shrinks by mu: the relative error rho_i grows as 1 / mu, and
coef_i, g_i and the Hessian block inherit it.  The bounds carry rho_i instead of hiding it:
  lhs row r         B_lhs = 64 eps (|A_i||x| + |b_i|)_r         rhs_i   B_rhs = 64 eps (|c_i|.|x| + |d_i|)
  s_i               B_s = 64 eps (rhs_i^2 + ||lhs_i||^2)         (the sum rhs^2 - sum_r lhs_r^2 in any order)
                          + 2 |rhs_i| B_rhs + 2 sum_r |lhs_r| B_lhs_r    (d(rhs^2) = 2 rhs d rhs, likewise lhs_r^2)
                    phase 1: + 4 eps (|s_i| + |s|) for the rounded shift;   bound slacks as above (+ the same)
  rho_i = B_s / s_i;  d coef_i / coef_i = d s_i / (s_i + 1e-12) <= rho_i
  g_i entry j       e_ij = coef_i [ (64 eps + rho_i) (|A_i|^T |lhs_i| + |c_i| |rhs_i|)_j    (the sum's order, and coef_i's error)
                                    + (|A_i|^T B_lhs + |c_i| B_rhs)_j ]                      (the operands' errors)
  gradient j        64 eps |t| (|P||x| + |q|)_j + sum_b inv_b (64 eps + rho_b) + sum_i e_ij
  Hessian (j, k)    64 eps |t P_jk| + sum_i coef_i (64 eps + rho_i) (|A_i|^T |A_i| + |c_i| |c_i|^T)_jk
                    + sum_i (|g_ij| e_ik + e_ij |g_ik| + e_ij e_ik)           (d(g g^T) with |dg| <= e)
                    + [j == k] sum_b (1 / (s_b + 1e-12)^2) (64 eps + 2 rho_b)
  phase 1 border    hxs_j: sum_i inv_i (e_ij + |g_ij| (64 eps + rho_i)) + sum_b inv_b^2 (64 eps + 2 rho_b)
                    hss: sum inv^2 (64 eps + 2 rho);   last gradient entry: 64 eps (|t| + sum inv) + sum inv rho
  barrier objective as above, rho summed over the cones and the bounds
A diagonal cone has A_i = diag(a_i): |A_i|^T |A_i| = diag(a_i^2).  Under a stale update (Q2) lhs,
rhs and the slacks stay at the first point; only t (P x + q), or phase 1's t s, moves.
Measured (tests/test_barrier_ref.py): the fp64 oracle is within 0.13 of every bound on every SOCP
instance, both phases (slacks 0.13, everything else below 0.03), and on the entries that a
mu = 1e-6 cone dominates the gradient bound is below 1e-2 of the entry.
"""
from __future__ import annotations

import numpy as np

from oracle import ipm_oracle as O

EPS = np.finfo(np.float64).eps
LD = np.longdouble
T_BARRIER = 7.0
LD_HESS_FLOPS = 1e8     # above n*n*m of this the long-double Hessian product takes seconds: fp64 oracle
MARGIN = 1e-9           # decisiveness of the reference's own line-search decisions


class Instance:
    """One LP / QP / LP-phase-1 barrier instance (kind in 'lp', 'qp', 'ph1', 'lpdiag')."""

    def __init__(self, kind, n, m, bounds, seed, tiny=False, near_bound=False):
        rng = np.random.default_rng(seed)
        self.kind, self.n, self.m, self.bounds, self.seed, self.tiny = kind, n, m, bounds, seed, tiny
        self.name = f"{kind}-n{n}-m{m}-{bounds}" + ("-tiny" if tiny else "") + ("-near" if near_bound else "")
        self.t = T_BARRIER
        self.x0 = rng.uniform(-0.5, 0.5, n)
        self.C = rng.normal(size=(m, n)) if m > 0 else None
        self.d = self.C @ self.x0 + rng.uniform(0.05, 2, m) if m > 0 else None
        glb, gub = rng.uniform(0.05, 2, n), rng.uniform(0.05, 2, n)
        if tiny:
            glb[::7] = 1e-6
            gub[::11] = 1e-7
        if near_bound:          # (the beta = 0.97 Newton step: many feasibility backtracks)
            glb[:] = rng.uniform(0.02, 0.05, n)
        self.lb = self.x0 - glb if bounds in ("both", "lb") else None
        self.ub = self.x0 + gub if bounds in ("both", "ub") else None
        self.c = rng.normal(size=n)
        if near_bound:          # a cost that pushes every variable at its near lower bound
            self.c = 30.0 * np.abs(self.c)
        self.P = self.q = None
        if kind == "qp":
            M = rng.normal(size=(n, n))
            self.P = M @ M.T / n + 0.1 * np.eye(n)
            self.q = rng.normal(size=n)
        self.x2 = self.x0 + 0.01 * rng.uniform(-1, 1, n)   # the stale-slack evaluation point (Q2)
        self.S = m + n * (self.lb is not None) + n * (self.ub is not None)

    # ---- the fp64 oracle and the device manager of this instance
    def oracle(self):
        x0 = self.x0.copy()
        if self.kind == "lp":
            return O.LPBarrier(c=self.c, C=self.C, d=self.d, x0=x0, lb=self.lb, ub=self.ub, t=1, try_diag=False)
        if self.kind == "lpdiag":
            return O.LPBarrier(c=self.c, x0=x0, lb=self.lb, ub=self.ub, t=1, try_diag=True)
        if self.kind == "qp":
            return O.QPBarrier(P=self.P, q=self.q, C=self.C, d=self.d, x0=x0, lb=self.lb, ub=self.ub, t=1)
        return O.Phase1Barrier(C=self.C, d=self.d, x0=x0, lb=self.lb, ub=self.ub, t=1)

    def device(self):
        import ipm355
        x0 = self.x0.copy()
        if self.kind == "lp":
            return ipm355.FunctionManagerLP(c=self.c, C=self.C, d=self.d, x0=x0, lower_bound=self.lb,
                                            upper_bound=self.ub, t=1, try_diag=False)
        if self.kind == "lpdiag":
            return ipm355.FunctionManagerLP(c=self.c, x0=x0, lower_bound=self.lb, upper_bound=self.ub, t=1,
                                            try_diag=True)
        if self.kind == "qp":
            return ipm355.FunctionManagerQP(P=self.P, q=self.q, C=self.C, d=self.d, x0=x0, lower_bound=self.lb,
                                            upper_bound=self.ub, t=1)
        return ipm355.FunctionManagerPhase1(C=self.C, d=self.d, x0=x0, lower_bound=self.lb, upper_bound=self.ub, t=1)

    def points(self, fm):
        """(x, stale x) as test_oracle_protocol_values drives them: phase 1 appends the manager's s."""
        if self.kind == "ph1":
            xt = np.append(self.x0, float(fm.s))
            return xt, xt + 0.01
        return self.x0.copy(), self.x2.copy()


class SocpInstance:
    """SOCP with box bounds.  ``rows``: rows of each dense cone, 0 = a diagonal cone (A_i a vector).
    The start point is pulled toward a point where every lhs_i is small, until every cone slack is
    at least 0.1 rhs_i^2, so no slack is small and no entry dominates a norm.

    The keyword options (their defaults leave the instance as it was without them, bit for bit):
    ``mu``: per cone a boundary margin or None; cone i with a margin gets d_i (c_i, moved along x0,
    when there is no d) reset so that s_i = mu_i rhs_i^2 at the start point, rhs_i > 0.
    ``scale``: multiplies every A_i and b_i.  ``q_c0``: q = q_c0 sqrt(n) c_0.  ``P_eye``:
    P = P_eye I.  ``box``: lb = x0 - box, ub = x0 + box.  ``tag``: the name's suffix."""

    def __init__(self, n, rows, seed, has_b=True, has_c=True, has_d=True, mu=None, scale=None, q_c0=None,
                 P_eye=None, box=None, tag=""):
        assert has_c or has_d
        assert has_b or has_d          # without b the centre is x = 0, where c.x = 0
        rng = np.random.default_rng(seed)
        self.kind, self.n, self.K, self.seed = "socp", n, len(rows), seed
        self.name = f"socp-n{n}-K{len(rows)}" + ("" if has_b else "-nob") + ("" if has_c else "-noc") + \
            ("" if has_d else "-nod") + (f"-{tag}" if tag else "")
        self.t = T_BARRIER
        self.mu = tuple(mu) if mu is not None else (None,) * len(rows)
        assert len(self.mu) == len(rows)
        xc = rng.uniform(-0.5, 0.5, n) if has_b else np.zeros(n)
        self.A = [rng.normal(size=(r, n)) / np.sqrt(n) if r > 0 else rng.normal(size=n) for r in rows]
        self.b = self.c = self.d = None
        if has_b:
            self.b = [-(A @ xc if A.ndim > 1 else A * xc) + 0.02 * rng.normal(size=A.shape[0]) for A in self.A]
        if scale is not None:
            self.A = [scale * A for A in self.A]
            if has_b:
                self.b = [scale * b for b in self.b]
        target = [1.0 + 0.4 * rng.uniform() for _ in rows]           # rhs_i at the centre
        if has_c:
            self.c = [rng.normal(size=n) / np.sqrt(n) for _ in rows]
            if has_d:
                self.d = [tg - ci.dot(xc) for tg, ci in zip(target, self.c)]
            else:
                self.c = [ci + (tg - ci.dot(xc)) / xc.dot(xc) * xc for tg, ci in zip(target, self.c)]
        else:
            self.d = list(target)
        M = rng.normal(size=(n, n))
        self.P = M @ M.T / n + 0.1 * np.eye(n)
        self.q = rng.normal(size=n)
        if P_eye is not None:
            self.P = P_eye * np.eye(n)
        if q_c0 is not None:
            self.q = q_c0 * np.sqrt(n) * self.c[0]
        delta = rng.uniform(-0.5, 0.5, n)
        lam = 1.0
        while True:
            x0 = xc + lam * delta
            lhs = [(A @ x0 if A.ndim > 1 else A * x0) + (self.b[i] if has_b else 0.0) for i, A in enumerate(self.A)]
            rhs = [(self.c[i].dot(x0) if has_c else 0.0) + (self.d[i] if has_d else 0.0) for i in range(len(rows))]
            if all(r > 0 and r * r - (l * l).sum() >= 0.1 * r * r for r, l in zip(rhs, lhs)):
                break
            lam *= 0.5
            assert lam > 1e-6
        for i, mi in enumerate(self.mu):        # the near-boundary cones: s_i = mu_i rhs_i^2
            if mi is None:
                continue
            new = float(np.sqrt((lhs[i] * lhs[i]).sum() / (1.0 - mi)))
            if has_d:
                self.d[i] = self.d[i] + (new - rhs[i])
            else:
                self.c[i] = self.c[i] + (new - rhs[i]) / x0.dot(x0) * x0
        self.x0 = x0
        if box is not None:
            self.lb, self.ub = x0 - box, x0 + box
        else:
            self.lb = x0 - rng.uniform(0.05, 2, n)
            self.ub = x0 + rng.uniform(0.05, 2, n)
        self.x2 = x0 + 0.01
        self.S = len(rows) + 2 * n + len(rows)

    def _kw(self, phase1):
        kw = dict(A=[a.copy() for a in self.A], b=self.b, c=self.c, d=self.d, x0=self.x0.copy(), t=1)
        if not phase1:
            kw.update(P=self.P, q=self.q)
        return kw

    def oracle(self, phase1=False):
        cls = O.SOCPPhase1Barrier if phase1 else O.SOCPBarrier
        return cls(lb=self.lb, ub=self.ub, **self._kw(phase1))

    def device(self, phase1=False):
        import ipm355
        cls = ipm355.FunctionManagerSOCPPhase1 if phase1 else ipm355.FunctionManagerSOCP
        return cls(lower_bound=self.lb, upper_bound=self.ub, **self._kw(phase1))

    def points(self, fm, phase1=False):
        if phase1:
            xt = np.append(self.x0, float(fm.s))
            return xt, xt + 0.01
        return self.x0.copy(), self.x2.copy()


# ------------------------------------------------------------------------------------------------
# the instance lists (kind, n, m, bounds, seed, tiny).  n in {1, 2, 63, 64, 65, 130, 513, 1026,
# 1027, 1400}: even and odd n (the vector / scalar GEMV and GEMM operand loads: ld = n) and every
# unrolled loop of gemv_row<true> (lane l enters the 8-deep loop when l + 448 < n/2 and the 4-deep
# loop when j + 192 < n/2: 514 -> 4-deep on every lane, 900 -> 8-deep on lanes 0 and 1 and 4-deep on
# the others, 1026 -> 8-deep on every lane, 1400 -> 8-deep and tail trips; 513, 1027 -> scalar);
# m in {1, 5, 255, 257, 300} and (n, m) = (200, 2049): 1 .. 19 row chunks of gemv_t_plan and 129
# chunks (8-unrolled sum with a tail of 1), column blocks of 256 with and without a tail.
# ------------------------------------------------------------------------------------------------
_LPQP = [
    ("lp", 1, 1, "none", 11, False), ("lp", 2, 5, "lb", 12, False), ("lp", 63, 1, "both", 13, True),
    ("lp", 64, 255, "ub", 14, False), ("lp", 65, 257, "lb", 15, True), ("lp", 130, 300, "both", 16, False),
    ("lp", 513, 5, "both", 17, True), ("lp", 1026, 257, "ub", 18, False), ("lp", 1027, 300, "lb", 19, False),
    ("lp", 1400, 255, "none", 20, False), ("lp", 200, 2049, "both", 21, False),
    ("lp", 514, 300, "both", 23, False), ("lpdiag", 1027, 0, "both", 22, True),
    ("qp", 1, 0, "lb", 31, False), ("qp", 2, 1, "both", 32, False), ("qp", 63, 5, "both", 33, True),
    ("qp", 64, 0, "both", 34, False), ("qp", 65, 255, "none", 35, False), ("qp", 130, 257, "ub", 36, True),
    ("qp", 513, 300, "lb", 37, False), ("qp", 1026, 5, "both", 38, True), ("qp", 1027, 1, "ub", 39, False),
    ("qp", 1400, 300, "both", 40, False), ("qp", 200, 2049, "none", 41, False),
    ("qp", 900, 5, "ub", 42, False),
]
_PH1 = [
    ("ph1", 1, 1, "none", 51, False), ("ph1", 2, 5, "both", 52, False), ("ph1", 63, 255, "lb", 53, False),
    ("ph1", 64, 257, "ub", 54, False), ("ph1", 65, 300, "both", 55, False), ("ph1", 130, 1, "both", 56, False),
    ("ph1", 513, 257, "none", 57, False), ("ph1", 1026, 300, "lb", 58, False), ("ph1", 1027, 5, "ub", 59, False),
    ("ph1", 1400, 255, "both", 60, False), ("ph1", 200, 2049, "both", 61, False),
]
# (n, rows per cone (0: diagonal), seed, b, c, d): cones of 1, 255, 256, 257 and 600 rows (k_cone_slacks
# and k_ls_cone stride 256 threads over a cone's rows: below, at and past one and two strides)
_SOCP = [
    (130, (1, 255, 256, 257, 600, 0), 71, True, True, True),
    (257, (1, 255, 256, 257, 600, 0), 72, False, True, True),
    (130, (600,), 73, True, False, True),
    (257, (257,), 74, True, True, False),
]
# The edge specs carry a seventh field, the keyword options of SocpInstance as sorted pairs.
#   near: the six cones above with every other one at mu = 1e-4 / 1e-6 (s_i = mu rhs_i^2): coefficients
#     2 / s_i of 1e4 .. 1e6 beside order-one ones, so single entries carry the slack's relative error;
#   diag3: three diagonal cones (dslot 0, 1, 2: the dc * n offsets of Ad, bd and the diagonal lhs
#     block) between dense ones, n = 300 (the diagonal stride loop past 256), the middle one near;
#   alldiag: R = 0, X holds the c rows and the G rows only;
#   K257 / K513: cones of 1 .. 3 rows past one and two 256-blocks of k_cone_coef (cone 256 near) and
#     R + 2K = 1028 / 2052 rows of k_cone_rowweights;
#   n = 2 and n = 513 (one column block of k_cone_grows with a single thread pair, three blocks with a
#     tail of one) under cones of 257 and of 1 and 600 rows.
_ALT_A = (1e-4, None, 1e-6, None, 1e-4, None)
_ALT_B = (None, 1e-6, None, 1e-4, None, 1e-6)
_ROWS6 = (1, 255, 256, 257, 600, 0)
_ROWS257 = tuple(1 + i % 3 for i in range(257))
_ROWS513 = tuple(1 + (i * 7) % 3 for i in range(513))
_SOCP_EDGE = [
    (130, _ROWS6, 81, True, True, True, (("mu", _ALT_A), ("tag", "near"))),
    (257, _ROWS6, 82, True, True, True, (("mu", _ALT_B), ("tag", "near"))),
    (130, _ROWS6, 83, True, False, True, (("mu", _ALT_B), ("tag", "near"))),
    (257, _ROWS6, 84, True, True, False, (("mu", _ALT_A), ("tag", "near"))),
    (300, (0, 5, 0, 300, 0), 85, True, True, True, (("mu", (None, None, 1e-6, None, None)), ("tag", "diag3"))),
    (65, (0, 0), 86, True, True, True, (("tag", "alldiag"),)),
    (64, _ROWS257, 87, True, True, True, (("mu", (None,) * 256 + (1e-6,)), ("tag", "K257"))),
    (63, _ROWS513, 88, True, True, True, (("tag", "K513"),)),
    (2, (257,), 89, True, True, True, (("tag", "cols"),)),
    (2, (1, 600), 90, True, True, True, (("tag", "cols"),)),
    (513, (257,), 91, True, True, True, (("tag", "cols"),)),
    (513, (1, 600), 92, True, True, True, (("tag", "cols"),)),
]
# The other-nappe Newton steps: A, b scaled by 0.1, q = 40 sqrt(n) c_0, P = 1e-3 I and a box of
# +-50 send the full step through the apex, so the first candidates have a positive cone slack
# (rhs^2 > ||lhs||^2) with rhs < 0: only the appended rhs block rejects them.
_NAPPE_OPTS = (("P_eye", 1e-3), ("box", 50.0), ("q_c0", 40.0), ("scale", 0.1), ("tag", "nappe"))
_SOCP_NAPPE = [
    (130, (257,), 93, True, True, True, _NAPPE_OPTS),
    (130, (257, 0), 94, True, True, True, _NAPPE_OPTS),
]

_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def lpqp_specs():
    """the LP / QP sweep, and the LP / QP instances of the Newton-step test (a subset of it)"""
    return list(_LPQP) + [e[1] for e in _NEWTON if e[1][0] in ("lp", "qp")]


def ph1_specs():
    return list(_PH1) + [e[1] for e in _NEWTON if e[1][0] == "ph1"]


def socp_specs():
    return list(_SOCP)


def socp_edge_specs():
    """the near-boundary, diagonal-cone, K-edge, column-block and other-nappe instances"""
    return list(_SOCP_EDGE) + list(_SOCP_NAPPE)


def socp_all_specs():
    return list(_SOCP) + socp_edge_specs()


def socp_near_specs():
    """the edge specs with at least one near-boundary cone"""
    return [s for s in _SOCP_EDGE if any(m is not None for m in dict(s[6]).get("mu", ()))]


def spec_id(spec):
    if isinstance(spec[1], tuple):
        tag = "-" + dict(spec[6])["tag"] if len(spec) > 6 else ""
        return f"socp-n{spec[0]}-K{len(spec[1])}-s{spec[2]}{tag}"
    return "-".join(str(v) for v in spec[:5]) + ("-tiny" if spec[5] else "") + ("-near" if len(spec) > 6 else "")


def instance(spec):
    """spec = (kind, n, m, bounds, seed, tiny[, near_bound])"""
    return _memo(("inst",) + tuple(spec), lambda: Instance(*spec))


def socp_instance(spec):
    return _memo(("socp",) + tuple(spec), lambda: SocpInstance(*spec[:6], **dict(spec[6] if len(spec) > 6 else ())))


# ------------------------------------------------------------------------------------------------
# long-double reference of the LP / QP barrier and its bounds
# ------------------------------------------------------------------------------------------------
def lpqp_reference(inst, x, slack_x=None, want_hessian=True):
    """Values at the evaluation point x with the slacks of slack_x (default x; the stale-slack rule
    Q2 evaluates the objective at a new x with the old slacks), in long double, and the entry-wise
    bounds of the module docstring.  Returns a dict: slacks, nobj, grad, hess (None when the long-
    double product is too slow: the caller uses the fp64 oracle's), and b_slacks, b_nobj, b_grad,
    b_hess; for 'lpdiag' hess is the diagonal vector (with epsilon) and ihess its reciprocal."""
    n, m, t = inst.n, inst.m, LD(inst.t)
    xs = np.asarray(x if slack_x is None else slack_x, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    xl, xsl = x.astype(LD), xs.astype(LD)
    aC = np.abs(inst.C) if m else None
    parts, bparts = [], []
    if m:
        parts.append(inst.d.astype(LD) - inst.C.astype(LD) @ xsl)
        bparts.append(64 * EPS * (np.abs(inst.d) + aC @ np.abs(xs)))
    if inst.ub is not None:
        parts.append(inst.ub.astype(LD) - xsl)
        bparts.append(4 * EPS * (np.abs(xs) + np.abs(inst.ub)))
    if inst.lb is not None:
        parts.append(xsl - inst.lb.astype(LD))
        bparts.append(4 * EPS * (np.abs(xs) + np.abs(inst.lb)))
    s = np.concatenate(parts)
    b_s = np.concatenate(bparts)
    s64 = s.astype(np.float64)
    rho = b_s / s64
    inv = 1 / (s + LD(O.EPS_LOG))
    inv64 = inv.astype(np.float64)
    sC = slice(0, m)
    off = m
    s_ub = s_lb = None
    if inst.ub is not None:
        s_ub = slice(off, off + n)
        off += n
    if inst.lb is not None:
        s_lb = slice(off, off + n)
    # objective and its gradient
    if inst.kind == "qp":
        Pl = inst.P.astype(LD)
        Px = Pl @ xl
        f = LD(0.5) * xl.dot(Px) + inst.q.astype(LD).dot(xl)
        fterms = 0.5 * np.abs(x) @ (np.abs(inst.P) @ np.abs(x)) + np.abs(inst.q) @ np.abs(x)
        go = t * (Px + inst.q.astype(LD))
        b_go = abs(inst.t) * (np.abs(inst.P) @ np.abs(x) + np.abs(inst.q))
    else:
        f = inst.c.astype(LD).dot(xl)
        fterms = np.abs(inst.c) @ np.abs(x)
        go = t * inst.c.astype(LD)
        b_go = np.abs(inst.t * inst.c)
    out = {"slacks": s, "b_slacks": b_s}
    out["nobj"] = t * f - np.log(s + LD(O.EPS_LOG)).sum()
    out["b_nobj"] = 64 * EPS * (abs(inst.t) * fterms + np.abs(np.log(s64 + O.EPS_LOG)).sum()) + rho.sum()
    g = go.copy()
    b_g = b_go.copy()
    if s_lb is not None:
        g -= inv[s_lb]
        b_g += inv64[s_lb]
    if s_ub is not None:
        g += inv[s_ub]
        b_g += inv64[s_ub]
    b_rho = np.zeros(n)
    if m:
        g += inst.C.T.astype(LD) @ inv[sC]
        b_g += aC.T @ inv64[sC]
        b_rho = aC.T @ (inv64[sC] * rho[sC])
    out["grad"] = g
    out["b_grad"] = 64 * EPS * b_g + b_rho
    if not want_hessian:
        return out
    if inst.kind == "lpdiag":
        h = np.zeros(n, dtype=LD)
        if s_lb is not None:
            h += inv[s_lb] ** 2
        if s_ub is not None:
            h += inv[s_ub] ** 2
        out["hess"], out["b_hess"] = h, 64 * EPS * h.astype(np.float64)
        out["ihess"], out["b_ihess"] = 1 / h, 64 * EPS * (1 / h).astype(np.float64)
        return out
    b_H = np.zeros((n, n))
    H = None
    use_ld = n * n * max(m, 1) <= LD_HESS_FLOPS
    if use_ld:
        H = np.zeros((n, n), dtype=LD)
    if m:
        w64 = inv64[sC] ** 2
        b_H += aC.T @ ((w64 * (64 * EPS + 2 * rho[sC]))[:, None] * aC)
        if use_ld:
            Cl = inst.C.astype(LD)
            H += Cl.T @ ((inv[sC] ** 2)[:, None] * Cl)
    dg = np.zeros(n, dtype=LD)
    for seg in (s_lb, s_ub):
        if seg is not None:
            dg += 1 / s[seg] ** 2              # the dense Hessian's bound diagonal: NO epsilon
    b_H[np.diag_indices(n)] += 64 * EPS * dg.astype(np.float64)
    if inst.kind == "qp":
        b_H += 64 * EPS * np.abs(inst.t * inst.P)
    if use_ld:
        H[np.diag_indices(n)] += dg
        if inst.kind == "qp":
            H += t * inst.P.astype(LD)
    out["hess"], out["b_hess"] = H, b_H
    return out


# ------------------------------------------------------------------------------------------------
# long-double reference of the SOCP barrier (and its phase 1) and its bounds
# ------------------------------------------------------------------------------------------------
def socp_reference(inst, x, slack_x=None, phase1=False, want_hessian=True):
    """The SOCP barrier at the evaluation point x with lhs, rhs and the slacks of slack_x (default
    x; Q2: only the objective and its gradient follow a stale update), in long double, with the
    entry-wise bounds of the module docstring.  Phase 1: x and slack_x carry the shift s as their
    last entry, there is no P, q, and the objective is s.  Returns a dict: lhs (the cones' blocks
    joined in cone order), rhs, slacks ([cones | ub - x | x - lb | rhs]), nobj, grad, hess (None
    without want_hessian) and b_lhs, b_rhs, b_slacks, b_nobj, b_grad, b_hess, rho (the relative
    error bound of each barrier slack)."""
    n, K, t = inst.n, inst.K, LD(inst.t)
    x = np.asarray(x, dtype=np.float64)
    xs = x if slack_x is None else np.asarray(slack_x, dtype=np.float64)
    shift = shift_s = None
    if phase1:
        x, shift = x[:n], float(x[n])
        xs, shift_s = xs[:n], float(xs[n])
    xl, xsl, axs = x.astype(LD), xs.astype(LD), np.abs(xs)
    e64 = 64 * EPS
    # ---- lhs, rhs and the cone slacks
    lhs, b_lhs = [], []
    rhs, b_rhs = np.zeros(K, dtype=LD), np.zeros(K)
    s_c, b_c = np.zeros(K, dtype=LD), np.zeros(K)
    for i, A in enumerate(inst.A):
        if A.ndim > 1:
            l, bl = A.astype(LD) @ xsl, np.abs(A) @ axs
        else:
            l, bl = A.astype(LD) * xsl, np.abs(A) * axs
        if inst.b is not None:
            l, bl = l + inst.b[i].astype(LD), bl + np.abs(inst.b[i])
        bl = e64 * bl
        r, br = LD(0), 0.0
        if inst.c is not None:
            r, br = inst.c[i].astype(LD).dot(xsl), float(np.abs(inst.c[i]) @ axs)
        if inst.d is not None:
            r, br = r + LD(inst.d[i]), br + abs(float(inst.d[i]))
        br = e64 * br
        l64, r64 = l.astype(np.float64), float(r)
        lhs.append(l)
        b_lhs.append(bl)
        rhs[i], b_rhs[i] = r, br
        s_c[i] = r * r - l.dot(l)
        b_c[i] = e64 * (r64 * r64 + l64.dot(l64)) + 2 * abs(r64) * br + 2 * np.abs(l64).dot(bl)
    parts, bparts = [s_c], [b_c]
    if inst.ub is not None:
        parts.append(inst.ub.astype(LD) - xsl)
        bparts.append(4 * EPS * (axs + np.abs(inst.ub)))
    if inst.lb is not None:
        parts.append(xsl - inst.lb.astype(LD))
        bparts.append(4 * EPS * (axs + np.abs(inst.lb)))
    sig, b_sig = np.concatenate(parts), np.concatenate(bparts)
    if phase1:                         # the shift is one more rounded addition
        b_sig = b_sig + 4 * EPS * (np.abs(sig.astype(np.float64)) + abs(shift_s))
        sig = sig + LD(shift_s)
    nbar = len(sig)
    sig64 = sig.astype(np.float64)
    rho = b_sig / sig64
    out = {"lhs": np.concatenate(lhs), "b_lhs": np.concatenate(b_lhs), "rhs": rhs, "b_rhs": b_rhs,
           "slacks": np.concatenate([sig, rhs]), "b_slacks": np.concatenate([b_sig, b_rhs]), "rho": rho}
    seg_ub = seg_lb = None
    off = K
    if inst.ub is not None:
        seg_ub = slice(off, off + n)
        off += n
    if inst.lb is not None:
        seg_lb = slice(off, off + n)
    # ---- the barrier objective
    if phase1:
        f, fterms = LD(shift), abs(shift)
        go, b_go = np.zeros(n, dtype=LD), np.zeros(n)
    else:
        Pl, ql = inst.P.astype(LD), inst.q.astype(LD)
        Px = Pl @ xl
        f = LD(0.5) * xl.dot(Px) + ql.dot(xl)
        fterms = 0.5 * np.abs(x) @ (np.abs(inst.P) @ np.abs(x)) + np.abs(inst.q) @ np.abs(x)
        go = t * (Px + ql)
        b_go = abs(inst.t) * (np.abs(inst.P) @ np.abs(x) + np.abs(inst.q))
    out["nobj"] = t * f - np.log(sig + LD(O.EPS_LOG)).sum()
    out["b_nobj"] = e64 * (abs(inst.t) * fterms + np.abs(np.log(sig64 + O.EPS_LOG)).sum()) + rho.sum()
    # ---- the cones' gradient pieces g_i = coef_i (A_i^T lhs_i - c_i rhs_i) and their bounds e_i
    inv = 1 / (sig + LD(O.EPS_LOG))
    inv64 = inv.astype(np.float64)
    coef = 2 * inv[:K] if phase1 else 2 / (sig[:K] + LD(O.EPS_CONE))
    coef64 = coef.astype(np.float64)
    G, E = np.zeros((K, n), dtype=LD), np.zeros((K, n))
    for i, A in enumerate(inst.A):
        l64 = np.abs(lhs[i].astype(np.float64))
        if A.ndim > 1:
            v, mag, prop = A.T.astype(LD) @ lhs[i], np.abs(A).T @ l64, np.abs(A).T @ b_lhs[i]
        else:
            v, mag, prop = A.astype(LD) * lhs[i], np.abs(A) * l64, np.abs(A) * b_lhs[i]
        if inst.c is not None:
            ac = np.abs(inst.c[i])
            v = v - inst.c[i].astype(LD) * rhs[i]
            mag, prop = mag + ac * abs(float(rhs[i])), prop + ac * b_rhs[i]
        G[i] = coef[i] * v
        E[i] = coef64[i] * ((e64 + rho[i]) * mag + prop)
    g = go + G.sum(axis=0)
    b_g = e64 * b_go + E.sum(axis=0)
    for seg, sgn in ((seg_lb, -1), (seg_ub, 1)):
        if seg is not None:
            g = g + sgn * inv[seg]
            b_g = b_g + inv64[seg] * (e64 + rho[seg])
    if phase1:
        g = np.append(g, t - inv.sum())
        b_g = np.append(b_g, e64 * (abs(inst.t) + inv64.sum()) + (inv64 * rho).sum())
    out["grad"], out["b_grad"], out["cone_grad"] = g, b_g, G
    out["hess"] = out["b_hess"] = None
    if not want_hessian:
        return out
    # ---- the Hessian: one weighted Gram product over the rows A_i, c_i (weight coef_i) and g_i (1)
    rows, wts, bw = [], [], []
    dgl, b_dg = np.zeros(n, dtype=LD), np.zeros(n)
    for i, A in enumerate(inst.A):
        wb = coef64[i] * (e64 + rho[i])
        if A.ndim > 1:
            rows.append(A)
            wts.append(np.full(A.shape[0], coef[i], dtype=LD))
            bw.append(np.full(A.shape[0], wb))
        else:
            dgl += coef[i] * A.astype(LD) ** 2
            b_dg += wb * A * A
        if inst.c is not None:
            rows.append(inst.c[i][None, :])
            wts.append(np.full(1, coef[i], dtype=LD))
            bw.append(np.full(1, wb))
    H, b_H = G.T @ G, np.zeros((n, n))
    if rows:
        X, w, bw = np.concatenate(rows, axis=0), np.concatenate(wts), np.concatenate(bw)
        Xl = X.astype(LD)
        H = H + Xl.T @ (w[:, None] * Xl)
        aX = np.abs(X)
        b_H += aX.T @ (bw[:, None] * aX)
    G64 = np.abs(G.astype(np.float64))
    GE = G64.T @ E
    b_H += GE + GE.T + E.T @ E
    ib = inv if phase1 else 1 / (sig + LD(O.EPS_CONE))          # the bound diagonal's own epsilon
    ib2 = ib ** 2
    ib264 = ib2.astype(np.float64)
    for seg in (seg_lb, seg_ub):
        if seg is not None:
            dgl += ib2[seg]
            b_dg += ib264[seg] * (e64 + 2 * rho[seg])
    if not phase1:
        H = H + t * inst.P.astype(LD)
        b_H += e64 * np.abs(inst.t * inst.P)
    H[np.diag_indices(n)] += dgl
    b_H[np.diag_indices(n)] += b_dg
    if phase1:                         # the border: hxs = -sum_i g_i inv_i + inv_lb^2 - inv_ub^2, hss = sum inv^2
        hxs = -(inv[:K, None] * G).sum(axis=0)
        b_hxs = (inv64[:K, None] * (E + G64 * (e64 + rho[:K, None]))).sum(axis=0)
        for seg, sgn in ((seg_lb, 1), (seg_ub, -1)):
            if seg is not None:
                hxs = hxs + sgn * ib2[seg]
                b_hxs = b_hxs + ib264[seg] * (e64 + 2 * rho[seg])
        hss = ib2[:nbar].sum()
        b_hss = (ib264[:nbar] * (e64 + 2 * rho)).sum()
        H = np.block([[H, hxs[:, None]], [hxs[None, :], np.array([[hss]], dtype=LD)]])
        b_H = np.block([[b_H, b_hxs[:, None]], [b_hxs[None, :], np.array([[b_hss]])]])
    out["hess"], out["b_hess"] = H, b_H
    return out


def _socp_refs(inst, phase1):
    fm_s = oracle_values(inst, phase1)["s"]
    if phase1:
        xt = np.append(inst.x0, fm_s)
        xv, xs = xt, xt + 0.01
    else:
        xv, xs = inst.x0, inst.x2
    return socp_reference(inst, xv, phase1=phase1), socp_reference(inst, xs, slack_x=xv, phase1=phase1,
                                                                   want_hessian=False)


def socp_refs(inst, phase1=False):
    """(reference at the start point, reference of the stale-slack pair), computed once"""
    return _memo(("sref", inst.name, inst.seed, phase1), lambda: _socp_refs(inst, phase1))


def near_dominated(inst, ref, mu_max=1e-6):
    """the gradient entries that the cones with a margin of at most mu_max dominate: their pieces
    sum to at least half of the entry, and the entry is at least 1e-2 of the largest one (a smaller
    one is itself the result of a cancellation inside A_i^T lhs_i - c_i rhs_i, whose factor comes
    on top of the slack's)"""
    near = np.array([m is not None and m <= mu_max for m in inst.mu])
    g = np.abs(ref["grad"][:inst.n].astype(np.float64))
    part = np.abs(ref["cone_grad"][near].sum(axis=0).astype(np.float64))
    return (part >= 0.5 * g) & (g >= 1e-2 * g.max())


def socp_ratios(inst, vals, phase1=False):
    """worst err / bound per quantity of protocol_values() output (and of lhs, rhs where vals has
    them) against socp_reference at the instance's two points; phase 1 starts at the oracle's s"""
    r0, r1 = socp_refs(inst, phase1)
    out = {k: ratio(vals[k], r0[k], r0["b_" + k]) for k in ("lhs", "rhs") if k in vals}
    out.update({k: ratio(vals[k], r0[k], r0["b_" + k]) for k in ("slacks", "nobj", "grad", "hess")})
    out["stale_nobj"] = ratio(vals["stale_nobj"], r1["nobj"], r1["b_nobj"])
    out["stale_grad"] = ratio(vals["stale_grad"], r1["grad"], r1["b_grad"])
    return out


def ratio(got, ref, bound):
    """worst |got - ref| / bound over the entries (0 / 0 counts as 0); inf when any entry of got,
    of the error or of the quotient is not finite, so that a NaN can never pass a comparison"""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != np.shape(ref) or not np.all(np.isfinite(got)):
        return float("inf")
    err = np.abs(got.astype(LD) - np.asarray(ref, dtype=LD)).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    if not np.all(np.isfinite(err)):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    if not np.all(np.isfinite(r)):
        return float("inf")
    return float(np.max(r)) if r.size else 0.0


def rel(a, b):
    """relative norm of a - b; inf when a holds a non-finite entry or the shapes differ"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    if a.shape != b.shape or not np.all(np.isfinite(a)):
        return float("inf")
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def all_within(values, limit):
    """every value of the dict at most limit (a NaN fails: max() would drop it)"""
    return all(v <= limit for v in values.values())


def protocol_values(fm, xv, xs, t, diag=False):
    """The call sequence of test_oracle_protocol_values on any manager (oracle or device)."""
    fm.update_x(xv.copy())
    fm.update_t(t)
    out = {"slacks": np.array(fm.slacks, dtype=np.float64), "nobj": float(fm.newton_objective()),
           "grad": np.array(fm.gradient(), dtype=np.float64), "hess": np.array(fm.hessian(), dtype=np.float64)}
    if diag:
        out["ihess"] = np.array(fm.inv_hessian(), dtype=np.float64)
    fm.update_x(xs.copy(), update_slacks=False)          # Q2: stale slacks
    out["stale_nobj"] = float(fm.newton_objective())
    out["stale_grad"] = np.array(fm.gradient(), dtype=np.float64)
    return out


def lpqp_ratios(inst, vals):
    """worst err / bound per quantity of protocol_values() output against the long-double reference
    (the Hessian against the fp64 oracle's where the long-double product is too slow)"""
    ref = _memo(("ref", inst.name, inst.seed), lambda: _lpqp_refs(inst))
    r0, r1, Href = ref
    out = {"slacks": ratio(vals["slacks"], r0["slacks"], r0["b_slacks"]),
           "nobj": ratio(vals["nobj"], r0["nobj"], r0["b_nobj"]),
           "grad": ratio(vals["grad"], r0["grad"], r0["b_grad"]),
           "hess": ratio(vals["hess"], Href, r0["b_hess"]),
           "stale_nobj": ratio(vals["stale_nobj"], r1["nobj"], r1["b_nobj"]),
           "stale_grad": ratio(vals["stale_grad"], r1["grad"], r1["b_grad"])}
    if inst.kind == "lpdiag":
        out["ihess"] = ratio(vals["ihess"], r0["ihess"], r0["b_ihess"])
    return out


def _lpqp_refs(inst):
    r0 = lpqp_reference(inst, inst.x0)
    r1 = lpqp_reference(inst, inst.x2, slack_x=inst.x0, want_hessian=False)
    Href = r0["hess"]
    if Href is None:
        Href = oracle_values(inst)["hess"]
    return r0, r1, Href


def oracle_values(inst, phase1=False):
    """protocol_values() of the fp64 oracle, computed once per instance"""
    def run():
        fm = inst.oracle(phase1) if inst.kind == "socp" else inst.oracle()
        s_start = float(getattr(fm, "s", 0.0))       # (phase 1: before the stale update moves it)
        xv, xs = inst.points(fm, phase1) if inst.kind == "socp" else inst.points(fm)
        v = protocol_values(fm, xv, xs, inst.t, diag=inst.kind == "lpdiag")
        v["s"] = s_start
        if inst.kind == "socp":      # (a stale update leaves the manager's lhs and rhs at the first point)
            v["lhs"] = np.concatenate([np.atleast_1d(l) for l in fm.lhs]).astype(np.float64)
            v["rhs"] = np.array(fm.rhs, dtype=np.float64)
        return v
    return _memo(("orc", inst.name, inst.seed, phase1), run)


# ------------------------------------------------------------------------------------------------
# one Newton step: the reference's own line search, with the margins of each of its decisions
# ------------------------------------------------------------------------------------------------
# (tag, spec or SOCP spec, phase1, beta).  S = m + n [ub] + n [lb] hits 1, 63, 64, 65, 960, 1025,
# 1088 and 8257: 1, 1, 1, 2, 15, 17, 17 and 130 blocks of 64 slacks in k_ls_lin, whose partial sums
# k_ls_fold reduces in 16 groups (groups empty; a tail only; 8-unrolled plus a tail).
_NEWTON = [
    ("S1", ("lp", 1, 1, "none", 201, False), False, 0.6),
    ("S63", ("qp", 63, 0, "lb", 102, False), False, 0.6),
    ("S64", ("lp", 2, 60, "both", 103, False), False, 0.6),
    ("S65", ("lp", 1, 63, "both", 104, False), False, 0.6),
    ("S960", ("lp", 130, 700, "both", 105, False), False, 0.6),
    ("S1025", ("ph1", 384, 257, "both", 106, False), False, 0.6),
    ("S1088", ("qp", 416, 256, "both", 107, False), False, 0.6),
    ("S8257", ("lp", 130, 7997, "both", 108, False), False, 0.6),
    ("socpK6", _SOCP[0], False, 0.6),
    ("socpK1", _SOCP[2], False, 0.6),
    # beta = 0.97 from a point near its lower bounds with a cost pushing at them: the reference
    # accepts k in 65..120, past the first 64-candidate table, so the second pass runs
    ("near97", ("lp", 130, 300, "both", 200, False, True), False, 0.97),
    # SOCP phase 1 (the shp / dshp arm of k_ls_cone), with one and with three diagonal cones
    ("socpK6ph1", _SOCP[0], True, 0.6),
    ("socpDiag3ph1", _SOCP_EDGE[4], True, 0.6),
    # from points with cones at s = 1e-4 rhs^2 and 1e-6 rhs^2: the full step accepted, and (without d)
    # 25 Armijo backtracks
    ("socpNear", _SOCP_EDGE[1], False, 0.6),
    ("socpNearArmijo", _SOCP_EDGE[3], False, 0.6),
    # candidates in the cone's other nappe: rejected by the sign of rhs alone
    ("nappe1", _SOCP_NAPPE[0], False, 0.6),
    ("nappe2", _SOCP_NAPPE[1], False, 0.6),
]


def newton_specs():
    return list(_NEWTON)


def newton_instance(entry):
    tag, spec, phase1, beta = entry
    if isinstance(spec[1], tuple):
        return socp_instance(spec)
    return instance(spec)


def _oracle_fm(inst, phase1):
    return inst.oracle(phase1) if inst.kind == "socp" else inst.oracle()


def newton_start(inst, fm, phase1=False):
    """the start point of the Newton step: x0 (phase 1: with the manager's s appended)"""
    if inst.kind == "ph1" or phase1:
        return np.append(inst.x0, float(fm.s))
    return inst.x0.copy()


def reference_newton_step(entry, alpha=0.2):
    """One FeasibleNewton step of the oracle from the instance's start point, and a replay of its
    backtracking (NewtonSolver.py:157-206 as oracle.FeasibleNewton.backtrack restates it) that
    records, for each candidate it examined, how far the decision was from flipping.  Returns a dict:
    x, step, k (backtracks: step = beta^k by repeated multiplication), nd, dx, x_start, cond2,
    feas_margin (min over the feasibility candidates of min_i |s_i| / max|s0|), armijo_margin (min
    over the Armijo candidates of |f - (f0 + a step g.x)| / max(1, |f0|)), first_block (index of the
    slack that reaches zero first along dx, -1 when the full step is feasible), S, nappe (the rejected
    SOCP candidates k whose barrier slacks are all >= MARGIN max|s0| while an appended rhs is
    <= -MARGIN max|s0|: the cone's other nappe)."""
    tag, spec, phase1, beta = entry

    def run():
        inst = newton_instance(entry)
        # the solve itself
        fm = _oracle_fm(inst, phase1)
        x_start = newton_start(inst, fm, phase1)
        fm.update_t(inst.t)
        ns = O.FeasibleNewton(fm, max_iters=1, eps=1e-5, alpha=alpha, beta=beta)
        x, _, iters, nd, ok = ns.solve(x_start.copy(), inst.t)
        step = ns.trace[0]["step"]
        # the same step on a second manager, decision by decision
        fm = _oracle_fm(inst, phase1)
        fm.update_t(inst.t)
        x0 = x_start.copy()
        g = fm.gradient(x0).copy()
        H = np.array(fm.hessian(), dtype=np.float64, copy=True)
        cond2 = float(np.linalg.cond(H))
        dx = ns2_direction(fm, g)
        s0 = np.array(fm.slacks, dtype=np.float64, copy=True)
        smax = float(np.abs(s0).max())
        fx = fm.newton_objective()
        gc = g.dot(x0)
        st, k = 1, 0
        fm.update_x(x0 + st * dx)
        s1 = np.array(fm.slacks, dtype=np.float64, copy=True)
        ds = s1 - s0
        with np.errstate(divide="ignore", invalid="ignore"):
            reach = np.where(ds < 0, s0 / -ds, np.inf)
        first_block = int(np.argmin(reach)) if reach.min() < 1 else -1
        feas = [float(np.abs(fm.slacks).min()) / smax]
        nappe = []

        def note_nappe():
            # a rejected SOCP candidate in the cone's other nappe: every barrier slack (cones, bounds)
            # non-negative by the margin, some appended rhs negative by it -- the rhs sign alone rejects
            if inst.kind == "socp" and (fm.slacks < 0).any():
                nb = fm.seg_barrier.stop
                if fm.slacks[:nb].min() >= MARGIN * smax and fm.slacks[nb:].min() <= -MARGIN * smax:
                    nappe.append(k)
        note_nappe()
        while (fm.slacks < 0).any():
            st *= beta
            k += 1
            if st < O.STEP_FLOOR:
                raise ValueError(f"{tag}: the reference's line search ran into its step floor")
            fm.update_x(x0 + st * dx)
            feas.append(float(np.abs(fm.slacks).min()) / smax)
            note_nappe()
        kf = k
        arm = []
        nxt = x0 + st * dx
        while True:
            f = fm.newton_objective()
            rhs = fx + alpha * st * gc
            arm.append(abs(float(f - rhs)) / max(1.0, abs(float(fx))))
            if not f > rhs:
                break
            nxt = x0 + st * dx
            if st < O.STEP_FLOOR:
                raise ValueError(f"{tag}: the reference's line search ran into its step floor")
            st *= beta
            k += 1
            fm.update_x(nxt, update_slacks=False)
        assert st == step, (st, step)
        return {"x": x, "step": step, "k": k, "k_feas": kf, "nd": nd, "dx": dx, "x_start": x_start, "cond2": cond2,
                "feas_margin": min(feas), "armijo_margin": min(arm), "first_block": first_block,
                "S": len(s0), "ok": ok, "iters": iters, "nappe": nappe}
    return _memo(("newton", tag), run)


def ns2_direction(fm, g):
    """the Cholesky direction on a copy of H (cho_factor in FeasibleNewton overwrites the manager's)"""
    import scipy.linalg
    H = np.array(fm.hessian(), dtype=np.float64, copy=True)
    L = scipy.linalg.cho_factor(H, overwrite_a=True, check_finite=False)
    return scipy.linalg.cho_solve(L, -g, check_finite=False)


def x_bound(ref):
    """||x_dev - x_orc|| <= 64 eps cond2(H) ||step dx|| + 4 eps ||x||: the Cholesky backward-error form"""
    return 64 * EPS * ref["cond2"] * np.linalg.norm(ref["step"] * ref["dx"]) + 4 * EPS * np.linalg.norm(ref["x"])
