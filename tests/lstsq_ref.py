"""Reference for the symmetric minimum-norm least squares (ipm_lstsq_sym): symmetric matrices with a
prescribed spectrum, the minimum-norm solution evaluated from the prescribed eigenpairs in long
double, the quantities tests/test_gpu_lstsq.py bounds, and its seeded instances.

H = Q diag(lambda) Q^T with Q from the QR of a seeded normal matrix; the product is formed in
np.longdouble, symmetrised and rounded to fp64, so the eigenpairs of the stored H are the prescribed
ones to about eps ||H||.  The kept set follows gelsd's rcond = None rule on the PRESCRIBED spectrum:
|lambda_i| > eps n max|lambda|; every instance keeps a factor of 4 between any |lambda_i| and that
cut (a factor of 8 in the two cut-edge instances), so the rule decides the same on the computed
eigenvalues.
    x_ref = sum_{kept} q_i (q_i . b) / lambda_i        (long double)
"""
import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble

# 8 x the worst value np.linalg.eigh itself reaches over the instance set (tests/test_lstsq_ref.py
# measures and asserts them; the table is in tests/test_gpu_lstsq.py):
#   ||V^T V - I||_max <= C1 n eps;  ||H V - V diag(lambda)||_F, max|lambda - prescribed| <= C2 n eps ||H||_F
C1 = 10.5
C2 = 7.5


class Instance:
    def __init__(self, name, n, lam, Q, H, kept):
        self.name, self.n, self.lam, self.Q, self.H, self.kept = name, n, lam, Q, H, kept

    @property
    def cond(self):
        a = np.abs(self.lam[self.kept])
        return float(a.max() / a.min()) if a.size else 1.0

    def x_ref(self, B):
        Q, lam, k = self.Q.astype(LD), self.lam.astype(LD), self.kept
        B = np.asarray(B, dtype=LD).reshape(self.n, -1)
        if not k.any():
            return np.zeros(B.shape)
        return ((Q[:, k] * (1 / lam[k])) @ (Q[:, k].T @ B)).astype(np.float64)

    @property
    def null(self):
        return self.Q[:, ~self.kept]


def _orth(n, seed):
    Q, _ = np.linalg.qr(np.random.default_rng([n, seed, 17]).normal(size=(n, n)))
    return Q


def _form(lam, Q):
    H = matmul_ld(Q * lam, Q.T)       # (Q * lam in fp64: the spectrum is prescribed to eps ||H|| anyway)
    return (0.5 * (H + H.T)).astype(np.float64)


def cut(lam):
    return EPS * len(lam) * np.abs(lam).max() if len(lam) else 0.0


def spectrum(kind, n):
    if kind == "full":           # well conditioned, positive
        return np.logspace(0, -3, n)
    if kind == "indef":          # full rank, mixed signs
        return np.logspace(0, -3, n) * np.where(np.arange(n) % 3 == 1, -1.0, 1.0)
    if kind == "psd_def":        # rank n // 2, PSD
        lam = np.zeros(n)
        lam[:n // 2] = np.logspace(0, -2, n // 2)
        return lam
    if kind == "indef_def":      # rank n // 2, indefinite
        lam = np.zeros(n)
        lam[:n // 2] = np.logspace(0, -2, n // 2) * np.where(np.arange(n // 2) % 2 == 1, -1.0, 1.0)
        return lam
    if kind == "repeated":       # half exactly 2, half exactly -1
        return np.where(np.arange(n) < (n + 1) // 2, 2.0, -1.0)
    if kind == "clustered":
        return 1.0 + np.arange(n) * 1e-12
    raise ValueError(kind)


KINDS = ["full", "indef", "psd_def", "indef_def", "repeated", "clustered"]
SHAPES = [1, 2, 3, 31, 32, 33, 255, 256, 257, 320, 321, 511, 512]


def instance(kind, n, seed=0):
    lam = spectrum(kind, n)
    Q = _orth(n, seed)
    return Instance(f"{kind}-{n}", n, lam, Q, _form(lam, Q), np.abs(lam) > cut(lam))


def diagonal_instance(n):
    """already diagonal (Q = I), mixed signs, magnitudes 1 .. 2^-11 (powers of two: the weights
    1 / lambda are exact, so X = b / lambda exactly): no rotation at all"""
    lam = 2.0 ** -(np.arange(n) % 12) * np.where(np.arange(n) % 2 == 1, -1.0, 1.0)
    return Instance(f"diagonal-{n}", n, lam, np.eye(n), np.diag(lam), np.ones(n, dtype=bool))


def zero_instance(n):
    return Instance(f"zero-{n}", n, np.zeros(n), np.eye(n), np.zeros((n, n)), np.zeros(n, dtype=bool))


def cut_edge_instance(n):
    """one eigenvalue at 8 eps n max (kept) and one at eps n max / 8 (dropped), the rest logspace
    1 .. 1e-2, on a diagonal-plus-one-rotation matrix: the rotation (an exact 3-4-5 one) mixes the
    largest eigenvalue with a mid-sized one only, so forming H perturbs the two edge eigenvalues
    not at all (they stay exact diagonal entries)."""
    lam = np.logspace(0, -2, n)
    lam[n - 2] = 8 * EPS * n          # max|lambda| = 1
    lam[n - 1] = EPS * n / 8
    Q = np.eye(n)
    i, j = 0, n // 2
    Q[i, i], Q[i, j], Q[j, i], Q[j, j] = 0.6, -0.8, 0.8, 0.6
    kept = np.ones(n, dtype=bool)
    kept[n - 1] = False
    return Instance(f"cutedge-{n}", n, lam, Q, _form(lam, Q), kept)


# rank n // 2 needs n >= 4: rank 0 is the zero matrix (below), and with ONE kept vector a right-hand
# side's component along it can be arbitrarily small against the dropped part, an ||b|| / ||H x||
# factor the solution bound does not carry
SPECTRA = [(kind, n) for n in SHAPES for kind in KINDS if not (n < 4 and kind in ("psd_def", "indef_def"))]


def all_instances():
    for kind, n in SPECTRA:
        yield instance(kind, n)
    yield Instance("neg-1x1", 1, np.array([-3.0]), np.eye(1), np.array([[-3.0]]), np.ones(1, dtype=bool))
    for n in (5, 33, 300):
        yield diagonal_instance(n)
    for n in (3, 33, 300):
        yield zero_instance(n)
    for n in (64, 320):
        yield cut_edge_instance(n)


def rhs(n, nrhs):
    return np.random.default_rng([n, nrhs, 31]).normal(size=(n, nrhs))


# ------------------------------------------------------------------------------------------------
# the bounded quantities
# ------------------------------------------------------------------------------------------------
def _slices(M):
    """M / scale (scale: the power of two >= max|M|) as three fixed-point slices on the grids
    2^-20, 2^-40, 2^-60; what is left is below 2^-61"""
    m = float(np.abs(M).max()) if M.size else 0.0
    scale = 2.0 ** np.ceil(np.log2(m)) if m > 0 else 1.0
    R, out = M / scale, []
    for s in (1, 2, 3):
        g = 2.0 ** (-20 * s)
        hi = np.round(R / g) * g          # (every step exact: powers of two, |R / g| < 2^21)
        R = R - hi
        out.append(hi)
    return out, scale


def matmul_ld(A, B):
    """A @ B as a long double array, accurate to n 2^-60 max|A| max|B| per entry: the nine products of
    the 20-bit slices are exact in fp64 whatever the order of summation (terms below 2^40 units,
    n <= 8192 of them), and they are added in long double, smallest first.  This is a long double
    product at BLAS speed; a plain np.longdouble matmul takes seconds at n = 512."""
    assert A.shape[1] <= 8192
    sa, ca = _slices(np.asarray(A, dtype=np.float64))
    sb, cb = _slices(np.asarray(B, dtype=np.float64))
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for tot in (4, 3, 2, 1, 0):
        for i in range(3):
            j = tot - i
            if 0 <= j < 3:
                acc += (sa[i] @ sb[j]).astype(LD)
    return acc * LD(ca) * LD(cb)


def eig_quantities(H, V, lam_prescribed):
    """for an eigenvector matrix V (columns) of H, with lambda = diag(V^T H V) in long double:
      q1 = ||V^T V - I||_max / (n eps)
      q2 = ||H V - V diag(lambda)||_F / (n eps ||H||_F)
      q3 = max |sort(lambda) - sort(prescribed)| / (n eps ||H||_F)
    (||H||_F = 0, the zero matrix: q2, q3 are 0 when their numerators are, else inf.)  Non-finite V
    gives inf."""
    n = H.shape[0]
    if not np.all(np.isfinite(V)):
        return float("inf"), float("inf"), float("inf")
    Vl, Hl = V.astype(LD), H.astype(LD)
    q1 = float(np.abs(matmul_ld(V.T, V) - np.eye(n)).max() / (n * EPS))
    HV = matmul_ld(H, V)
    lam = np.sum(Vl * HV, axis=0)
    scale = n * EPS * np.sqrt(np.sum(Hl * Hl))
    r2 = np.sqrt(np.sum((HV - Vl * lam) ** 2))
    r3 = np.abs(np.sort(lam) - np.sort(lam_prescribed.astype(LD))).max()
    if scale == 0:
        return q1, (0.0 if r2 == 0 else float("inf")), (0.0 if r3 == 0 else float("inf"))
    return q1, float(r2 / scale), float(r3 / scale)


def solution_ratio(inst, X, B):
    """worst over the right-hand sides of ||x - x_ref|| / (64 n eps cond_kept ||x_ref||); x_ref = 0
    (nothing kept, or b = 0) requires x = 0 exactly"""
    X = np.reshape(X, (inst.n, -1))
    if not np.all(np.isfinite(X)):
        return float("inf")
    ref = inst.x_ref(B)
    worst = 0.0
    for c in range(ref.shape[1]):
        nr, err = np.linalg.norm(ref[:, c]), np.linalg.norm(X[:, c] - ref[:, c])
        if err == 0:
            continue
        if nr == 0:
            return float("inf")
        worst = max(worst, err / (64 * inst.n * EPS * inst.cond * nr))
    return float(worst)


def null_ratio(inst, X):
    """worst over the right-hand sides of ||N^T x|| / (64 n eps cond_kept ||x||)"""
    N = inst.null
    X = np.reshape(X, (inst.n, -1))
    if N.shape[1] == 0:
        return 0.0
    if not np.all(np.isfinite(X)):
        return float("inf")
    worst = 0.0
    for c in range(X.shape[1]):
        nx, comp = np.linalg.norm(X[:, c]), np.linalg.norm(N.T.astype(LD) @ X[:, c].astype(LD))
        if comp == 0:
            continue
        if nx == 0:
            return float("inf")
        worst = max(worst, float(comp) / (64 * inst.n * EPS * inst.cond * nx))
    return float(worst)


NONFINITE_NAMES = [f"{k}-{n}" for n in (5, 300) for k in ("nan-pair", "inf-diag", "all-nan")]


def nonfinite_inputs():
    """(name, H): symmetric inputs with a NaN pair, a +Inf diagonal entry, all NaN; n = 5 (one
    workgroup) and n = 300 (blocked)"""
    for n in (5, 300):
        H = instance("full", n).H
        A = H.copy(); A[1, 3] = A[3, 1] = np.nan
        yield f"nan-pair-{n}", A
        A = H.copy(); A[2, 2] = np.inf
        yield f"inf-diag-{n}", A
        yield f"all-nan-{n}", np.full((n, n), np.nan)
