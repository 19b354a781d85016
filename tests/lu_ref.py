"""Plain NumPy fp64 restatement of the device LU (ipm_getrf / ipm_getrs), the componentwise error
bounds the GPU tests hold it to, and the seeded instances of tests/test_gpu_lu.py.

Algorithm (csrc/ipm_blas.hip, "LU with partial pivoting"): right-looking Gaussian elimination, the
pivot of step k at the FIRST index of the largest |a_ik|, i >= k (LAPACK's idamax).  A pivot column
that is exactly zero is skipped: piv[k] = -1 - k, its L column zeroed, no swap and no update; the
solve skips that column in the forward sweep and sets component k of the solution to 0.  A NaN
candidate is not a zero: here it wins the search (the first NaN, as in LAPACK; the device keeps its
finite winner and sets the pivot to NaN, pivots are not compared on such input), so the factors are
NaN from there on and a NaN matrix cannot come back as a finite solution.

Layout here: A is an ordinary (row, column) NumPy array.  The device stores it column-major with a
leading dimension; tests/test_gpu_lu.py does that translation.

Bounds (N. J. Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., chapter 9; eps = 2^-52
= 2 u): for the COMPUTED factors L, U and pivots P of any variant of Gaussian elimination,
    |P A - L U|_ij <= gamma_min(i,j) (|L| |U|)_ij         (theorem 9.3 with lemma 8.4, entry by entry)
in any order of summation, so the blocked device form (fma triangular solve, MFMA trailing product)
is covered.  The tests use (min(i, j) + 2) eps with 0-based i, j, which is > 2 gamma_{min(i,j)+1}.
For the solve, theorem 9.4: (A + dA) x = b with |dA| <= gamma_3n P^T |L| |U|, hence
    |P b - P A x|_i <= 3 (n + 1) eps (|L| |U| |x|)_i
(3 (n + 1) eps > 2 gamma_3n).  Both products are formed in np.longdouble.  With skipped columns
P A = L U still holds (step k leaves the rows and columns past k unchanged), and the solve's
equations hold in every row of P A x = P b except the skipped rows k, where x_k = 0 is imposed.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble


# ------------------------------------------------------------------------------------------------
# the algorithm
# ------------------------------------------------------------------------------------------------
def getrf(A):
    """-> (LU, piv, ratio, ties).  LU holds the unit-lower L below and U on and above the diagonal
    of the row-permuted matrix; piv[k] is the row swapped with k at step k (0-based, in order), or
    -1 - k for a skipped column.  ratio[k] = second-largest / largest |candidate| of step k (0 for
    a single candidate or a skipped column; NaN once a NaN took part).  ties[k] lists the rows that
    attain the largest |candidate| when more than one does."""
    LU = np.array(A, dtype=np.float64, copy=True)
    n = LU.shape[0]
    assert LU.shape == (n, n)
    piv = np.zeros(n, dtype=np.int64)
    ratio = np.zeros(n)
    ties = {}
    for k in range(n):
        c = np.abs(LU[k:, k])
        nan = np.isnan(c)
        if nan.any():
            p = k + int(np.argmax(nan))       # the first NaN wins: the column is scaled by NaN
            ratio[k] = np.nan
        else:
            p = k + int(np.argmax(c))         # first index of the maximum
            best = c[p - k]
            if best == 0.0:
                piv[k] = -1 - k
                LU[k + 1:, k] = 0.0
                continue
            if c.size > 1:
                ratio[k] = np.partition(c, -2)[-2] / best if np.isfinite(best) else np.nan
                if ratio[k] == 1.0:
                    ties[k] = k + np.flatnonzero(c == best)
        piv[k] = p
        if p != k:
            LU[[k, p], :] = LU[[p, k], :]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            LU[k + 1:, k] /= LU[k, k]
            l = LU[k + 1:, k:k + 1]
            for j in range(k + 1, n, 128):      # (column chunks: the temporary stays in cache)
                LU[k + 1:, j:j + 128] -= l * LU[k:k + 1, j:j + 128]
    return LU, piv, ratio, ties


def getrs(LU, piv, B):
    """solve with getrf's factors: B (n x nrhs) -> X, the skip rule as on the device"""
    n = LU.shape[0]
    X = np.array(B, dtype=np.float64, copy=True).reshape(n, -1)
    for k in range(n):
        p = int(piv[k])
        if p >= 0 and p != k:
            X[[k, p], :] = X[[p, k], :]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(n):
            if piv[k] < 0:
                continue
            X[k + 1:, :] -= np.outer(LU[k + 1:, k], X[k, :])
        for k in range(n - 1, -1, -1):
            if piv[k] < 0:
                X[k, :] = 0.0
                continue
            X[k, :] /= LU[k, k]
            X[:k, :] -= np.outer(LU[:k, k], X[k, :])
    return X.reshape(np.shape(B))


def permute_rows(M, piv):
    """P M: the swaps of piv applied in order to the rows of M (a copy)"""
    M = np.array(M, copy=True)
    for k, p in enumerate(piv):
        p = int(p)
        if p >= 0 and p != k:
            M[[k, p]] = M[[p, k]]
    return M


def split(LU):
    n = LU.shape[0]
    return np.tril(LU, -1) + np.eye(n), np.triu(LU)


# ------------------------------------------------------------------------------------------------
# the bounds
# ------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    """worst err / bound; 0 / 0 counts as 0, anything non-finite as inf"""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    if err.size == 0:
        return 0.0
    if not (np.all(np.isfinite(err)) and np.all(np.isfinite(bound))):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


def factor_ratio(A, LU, piv):
    """worst |P A - L U|_ij / ((min(i, j) + 2) eps (|L| |U|)_ij), products in long double"""
    n = LU.shape[0]
    if not (np.all(np.isfinite(LU)) and np.all(np.isfinite(A))):
        return float("inf")
    L, U = split(LU)
    R = permute_rows(A, piv).astype(LD)
    Ll, Ul = L.astype(LD), U.astype(LD)
    for k in range(0, n, 128):        # (L U)_ij has min(i, j) + 1 terms: skip the zero blocks
        R[k:, k:] -= Ll[k:, k:k + 128] @ Ul[k:k + 128, k:]
    i = np.arange(n)
    cnt = (np.minimum.outer(i, i) + 2).astype(LD)
    # |L| |U| in fp64 (a sum of non-negative terms: relative error below n eps), rounded down
    absprod = (np.abs(L) @ np.abs(U)) * (1.0 - 4 * n * EPS)
    return _ratio(np.abs(R), cnt * LD(EPS) * absprod.astype(LD))


def solve_ratio(A, LU, piv, X, B):
    """worst |P b - P A x|_i / (3 (n + 1) eps (|L| |U| |x|)_i) over the right-hand sides and the
    rows that are not skipped columns"""
    n = LU.shape[0]
    X, B = np.reshape(X, (n, -1)), np.reshape(B, (n, -1))
    if not (np.all(np.isfinite(X)) and np.all(np.isfinite(LU))):
        return float("inf")
    L, U = split(LU)
    PA, PB = permute_rows(A, piv).astype(LD), permute_rows(B, piv).astype(LD)
    err = np.abs(PB - PA @ X.astype(LD))
    bound = LD(3 * (n + 1)) * LD(EPS) * (np.abs(L).astype(LD) @ (np.abs(U).astype(LD) @ np.abs(X).astype(LD)))
    keep = np.asarray(piv) >= 0
    return _ratio(err[keep], bound[keep])


# ------------------------------------------------------------------------------------------------
# instances
# ------------------------------------------------------------------------------------------------
SWEEP_N = [1, 2, 63, 64, 65, 127, 128, 129, 257, 1100]
CLASSES = ["general", "kkt", "schur"]
ILLCOND = [1e8, 1e12, 1e15]          # scripts/lu_accuracy.py's symmetric family, n = 80
DECISIVE = 1.0 - 1e-9


def _spd_spread(rng, n):
    """H SPD, diagonal spread 1e-6 .. 1e6: an interior-point Hessian near the boundary"""
    G = rng.normal(size=(n, n)) / np.sqrt(max(n, 1))
    d = np.logspace(-6, 6, n) if n > 1 else np.ones(1)
    s = np.sqrt(rng.permutation(d))
    H = (G @ G.T + np.eye(n)) * np.outer(s, s)
    return 0.5 * (H + H.T)


def matrix(cls, n, seed=0):
    rng = np.random.default_rng([seed, n, CLASSES.index(cls) if cls in CLASSES else 7])
    if cls == "general":
        return rng.normal(size=(n, n))
    if cls == "kkt":          # [[H, A^T], [A, 0]], the zero block of size p = n // 4
        p = n // 4
        m = n - p
        K = np.zeros((n, n))
        K[:m, :m] = _spd_spread(rng, m)
        Ae = rng.normal(size=(p, m))
        K[m:, :m] = Ae
        K[:m, m:] = Ae.T
        return K
    if cls == "schur":        # S = A H^-1 A^T, built on the host
        m = 2 * n
        H = _spd_spread(rng, m)
        Ae = rng.normal(size=(n, m))
        S = Ae @ np.linalg.solve(H, Ae.T)
        return 0.5 * (S + S.T)
    raise ValueError(cls)


def illcond(n, cond):
    rng = np.random.default_rng(n)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    A = (Q * np.logspace(0, -np.log10(cond), n)) @ Q.T
    return 0.5 * (A + A.T)


def rhs(n, nrhs, seed=0):
    return np.random.default_rng([seed, n, nrhs, 99]).normal(size=(n, nrhs))


def sweep_instances():
    """(name, A) of every non-singular finite instance whose pivots the GPU test compares"""
    for n in SWEEP_N:
        for cls in CLASSES:
            if cls == "kkt" and n < 4:      # (no zero block below n = 4: the class is H alone)
                continue
            yield f"{cls}-{n}", matrix(cls, n)
    for cond in ILLCOND:
        yield f"illcond-{cond:.0e}", illcond(80, cond)


def zero_column(k, n=130):
    """a normal matrix with column k exactly zero"""
    A = np.random.default_rng([n, k, 5]).normal(size=(n, n))
    A[:, k] = 0.0
    return A


ZERO_COLS = [0, 63, 64, 65, 129]


def exact_matrix(n, seed, pos=None, ties=(), dup=None, fixed=0):
    """An integer matrix whose elimination with partial pivoting is exact in fp64: A = Pi (L U)
    with L unit lower, entries in {-1/2, 0, 1/2}, U upper with diagonal in {+-2, +-4} and even
    off-diagonal entries in -4 .. 4: every multiplier is a quotient by a power of two, every
    intermediate entry an integer below 4 n, and the row of L U that holds step k's diagonal is the
    strict largest of its column (|l| <= 1/2) -- wherever Pi puts it.

    pos:   {original row: position} fixes part of Pi; the first `fixed` rows stay in place, the
           rest is a seeded permutation.
    ties:  (k, i, sign) sets L[i, k] = sign * 1: row i of L U then ties with the diagonal row of
           step k in magnitude, with that sign.
    dup:   (j, c), j < c: column c of U is column j's (so columns j and c of A are equal, and
           column c is exactly zero when elimination reaches it); L's column c is zero, as the skip
           rule leaves it."""
    rng = np.random.default_rng([n, seed, 11])
    L = np.tril(rng.integers(-1, 2, size=(n, n)).astype(np.float64) * 0.5, -1) + np.eye(n)
    U = np.triu(2.0 * rng.integers(-2, 3, size=(n, n)), 1)
    U += np.diag(rng.choice([-4.0, -2.0, 2.0, 4.0], size=n))
    for k, i, sign in ties:
        assert i > k
        L[i, k] = float(sign)
    if dup is not None:
        j, c = dup
        U[:, c] = U[:, j]
        U[j + 1:, c] = 0.0
        L[c + 1:, c] = 0.0
    B = L @ U
    pos = dict(pos or {})
    for r in range(fixed):
        pos.setdefault(r, r)
    free_rows = [r for r in range(n) if r not in pos]
    taken = set(pos.values())
    free_pos = [q for q in range(n) if q not in taken]
    for r, q in zip(free_rows, rng.permutation(free_pos)):
        pos[r] = int(q)
    A = np.empty_like(B)
    for r, q in pos.items():
        A[q] = B[r]
    return A


TIE_N = 1600


def tie_instances():
    """(name, A, k, rows, winner): at step k the rows `rows` hold the equal largest candidates and
    the pivot must be `winner`, the first of them.  k_lu_pivot's thread of row i at step k is
    (i - k) % 1024."""
    n = TIE_N
    # rows 100 and 1124: one search thread, first and second stride trip (strict > keeps 100)
    yield "trip", exact_matrix(n, 1, pos={0: 100, 5: 1124}, ties=[(0, 5, -1)]), 0, [100, 1124], 100
    # rows 700 and 1500: threads 700 and 476 -- the lower thread holds the higher row
    yield "reduce", exact_matrix(n, 2, pos={0: 700, 5: 1500}, ties=[(0, 5, 1)]), 0, [700, 1500], 700
    # rows 3 and 515: partners of the s = 512 reduction step
    yield "s512", exact_matrix(n, 3, pos={0: 3, 5: 515}, ties=[(0, 5, -1)]), 0, [3, 515], 3
    # the diagonal itself ties (with rows in its own thread's second trip and its s = 512 partner):
    # no swap
    yield ("diag0", exact_matrix(n, 4, pos={0: 0, 5: 512, 6: 1024}, ties=[(0, 5, -1), (0, 6, 1)]),
           0, [0, 512, 1024], 0)


def dup_instances():
    """(name, A, c): an exact integer matrix, n = 130, whose column c equals an earlier column and
    is exactly zero when elimination reaches it.  Rows 0 .. c stay in place, so that the row the
    skipped step leaves at position c is the one whose U row the construction wrote there; the
    steps after c pivot freely."""
    yield "dup64", exact_matrix(130, 6, dup=(10, 64), fixed=65), 64
    yield "dup70", exact_matrix(130, 7, dup=(3, 70), fixed=71), 70


def is_dyadic(M, bits=20):
    """every entry an integer multiple of 2^-bits (integers included), exactly"""
    S = np.asarray(M) * 2.0 ** bits
    return bool(np.all(np.isfinite(S)) and np.all(S == np.round(S)) and np.all(np.abs(S) < 2.0 ** 52))


def nonfinite_instances():
    """(name, A): matrices on which np.linalg.solve returns a non-finite vector"""
    nan = np.nan

    def base(n, seed):
        return np.random.default_rng([n, seed, 13]).normal(size=(n, n))
    A = base(70, 0); A[40, 0] = nan
    yield "nan-below-diag-col0", A
    A = base(70, 1); A[3, 50] = nan
    yield "nan-above-diag", A
    for c in (0, 64, 69):
        A = base(70, 2 + c); A[:, c] = nan
        yield f"nan-column-{c}", A
    for n in (5, 70):
        yield f"nan-matrix-{n}", np.full((n, n), nan)
