"""-m gpu: the level-0 entry points the solvers reach only at their own shapes -- ipm_gemv (both
trans values), ipm_gemm_tn, ipm_transpose, ipm_copy -- against NumPy at every loop-entry and tile
edge, with the coefficient and leading-dimension combinations the solvers never pass.

Bound (the convention of test_gpu_kernels.py): fp64 sums of products in another order satisfy
|got - ref| <= 64 eps sum|terms|, entry by entry.  Operands are padded with NaN wherever a leading
dimension leaves room, so a load outside the operand shows in the result; output padding holds a
sentinel that must come back untouched.  Each test prints its worst err / bound.
"""
import numpy as np
import pytest

from gpu_util import copy, dev, devnan, gemm_tn, gemv, host, transpose

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
IPM_OK, IPM_INVALID_ARG = 0, 2
COEFS = [(1.0, 0.0), (-0.75, 0.5)]
SENTINEL = 12345.0


def _worst(got, ref, bound):
    err = np.abs(got - ref)
    assert np.all(np.isfinite(got)), "non-finite output"
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def _padded(a, ld):
    """device copy of the rows of a with leading dimension ld, the padding NaN"""
    t = devnan((a.shape[0], ld))
    if a.size:
        t[:, :a.shape[1]] = dev(a)
    return t


GEMV_N_ROWS = [1, 3, 4, 5, 130]
GEMV_N_COLS = [1, 2, 3, 63, 64, 127, 128, 129, 130, 386, 450, 514, 898, 960, 1026, 1027, 2050, 2500]


@pytest.mark.parametrize("cols", GEMV_N_COLS)
def test_gemv_n_matches_numpy(cols):
    """k_gemv_n<VEC>, one wave per row (4 rows per workgroup: rows 1, 3, 4, 5 and 130 leave waves
    idle, fill one workgroup and start another).  With c2 = cols / 2 pairs, lane l enters the 8-deep
    loop when l + 448 < c2 and the 4-deep loop when j + 192 < c2:
      cols <= 130   neither loop (the 64-stride tail only; 1, 2, 3: lanes without any element)
      386 / 450     c2 = 193 / 225: the 4-deep loop on lane 0 only / on lanes 0..32
      514           c2 = 257: the 4-deep loop on every lane, one tail trip on lane 0
      898 / 960     c2 = 449 / 480: the 8-deep loop on lane 0 / lanes 0..31, the others 4-deep
      1026 / 1027   c2 = 513: 8-deep on every lane, then one tail trip on lane 0 (1027: + odd tail)
      2050 / 2500   c2 = 1025 / 1250: 8-deep twice on every lane, then a tail trip on lane 0 /
                    8-deep twice, 4-deep on lanes < 34, three or four tail trips on the others
    Layouts: ldm = cols when even (vector path); odd cols with ldm = cols + 1 (vector path, the odd
    last element by lane 0); ldm odd (scalar path); even ldm with x one double into its buffer
    (8- but not 16-byte aligned: the scalar path chosen by alignment).  beta = 0 on a NaN y must
    not read y."""
    rng = np.random.default_rng(cols)
    R = max(GEMV_N_ROWS)
    M = rng.uniform(-2, 2, (R, cols))
    x = rng.uniform(-2, 2, cols)
    y0 = rng.uniform(-2, 2, R)
    even = cols + (cols & 1)
    layouts = [("vector", even, 0), ("scalar-odd-ld", even + 1, 0), ("scalar-misaligned-x", even, 1)]
    full, fbound = M @ x, np.abs(M) @ np.abs(x)
    worst = 0.0
    for name, ldm, xoff in layouts:
        Md = _padded(M, ldm)
        xbuf = devnan((cols + 2,))
        xd = xbuf[xoff:xoff + cols]
        xd.copy_(dev(x))
        assert (xd.data_ptr() % 16 == 0) == (xoff == 0) and Md.data_ptr() % 16 == 0
        for rows in GEMV_N_ROWS:
            for alpha, beta in COEFS:
                yd = devnan((R,)) if beta == 0.0 else dev(y0)
                assert gemv(0, rows, cols, alpha, Md, ldm, xd, beta, yd) == IPM_OK
                got = host(yd)
                ref = alpha * full[:rows] + beta * y0[:rows]
                bound = 64 * EPS * (abs(alpha) * fbound[:rows] + abs(beta * y0[:rows]))
                r = _worst(got[:rows], ref, bound)
                assert r <= 1.0, (name, rows, alpha, beta, r)
                worst = max(worst, r)
                rest = got[rows:]          # rows past `rows` are not this call's
                assert np.all(np.isnan(rest)) if beta == 0.0 else np.array_equal(rest, y0[rows:])
    print(f"[gemv n cols={cols}] worst err / bound {worst:.3g}")


@pytest.mark.parametrize("alpha,beta", COEFS)
def test_gemv_n_empty(alpha, beta):
    """rows = 0 touches nothing; cols = 0 leaves y = beta y (zero, not NaN, for beta = 0)"""
    y0 = np.array([1.5, -2.0, 3.0])
    yd = dev(y0)
    assert gemv(0, 0, 7, alpha, devnan((1, 7)), 7, devnan((7,)), beta, yd) == IPM_OK
    np.testing.assert_array_equal(host(yd), y0)
    yd = devnan((3,)) if beta == 0.0 else dev(y0)
    assert gemv(0, 3, 0, alpha, devnan((3, 2)), 2, devnan((2,)), beta, yd) == IPM_OK
    np.testing.assert_array_equal(host(yd), beta * y0 if beta != 0.0 else np.zeros(3))


GEMV_T_ROWS = [0, 1, 5, 16, 17, 112, 128, 129, 257, 3000]


@pytest.mark.parametrize("cols", [1, 255, 256, 257, 700])
def test_gemv_t_matches_numpy(cols):
    """k_gemv_t_part / k_gemv_t_fin as gemv_t_plan lays them out: row chunks of 16, so rows 1, 5, 16
    -> 1 chunk, 17 -> 2, 112 -> 7 (the tail loop only), 128 -> 8 (one 8-unrolled trip, no tail), 129
    -> 9, 257 -> 17 (8-unrolled twice + tail), 3000 -> 188; rows = 0 -> no partial launch, the second
    stage alone gives y = beta y.  cols 1, 255, 256, 257, 700: a partial column block, a full one,
    one thread into the second, three blocks.  ldm = cols and cols + 3 (NaN padding)."""
    rng = np.random.default_rng(1000 + cols)
    R = max(GEMV_T_ROWS)
    M = rng.uniform(-2, 2, (R, cols))
    x = rng.uniform(-2, 2, R)
    y0 = rng.uniform(-2, 2, cols)
    xd = dev(x)
    worst = 0.0
    for ldm in (cols, cols + 3):
        Md = _padded(M, ldm)
        for rows in GEMV_T_ROWS:
            full, fbound = M[:rows].T @ x[:rows], np.abs(M[:rows]).T @ np.abs(x[:rows])
            for alpha, beta in COEFS:
                yd = devnan((cols,)) if beta == 0.0 else dev(y0)
                assert gemv(1, rows, cols, alpha, Md, ldm, xd, beta, yd) == IPM_OK
                ref = alpha * full + beta * y0
                bound = 64 * EPS * (abs(alpha) * fbound + abs(beta * y0))
                r = _worst(host(yd), ref, bound)
                assert r <= 1.0, (ldm, rows, alpha, beta, r)
                worst = max(worst, r)
    print(f"[gemv t cols={cols}] worst err / bound {worst:.3g}")


GEMM_CASES = [
    (1, 1, 1, False), (5, 3, 0, False), (64, 64, 4, False), (65, 63, 37, False), (130, 257, 100, False),
    (300, 30, 1200, False), (1025, 50, 1025, False), (129, 131, 67, True), (3000, 4000, 37, False),
]


@pytest.mark.parametrize("M,N,K,odd", GEMM_CASES)
def test_gemm_tn_matches_numpy(M, N, K, odd):
    """mfma_gemm_launch with tri = 0 (ni = N, nj = M, row-major C): (1, 1, 1) the smallest; (5, 3, 0)
    K = 0, C = beta C only; (64, 64, 4) one full 64-tile, a quarter K slab; (65, 63, 37) ragged tile
    edges in both dimensions and a ragged K slab; (130, 257, 100) several 64-tiles; (300, 30, 1200)
    the Lasso's thin N; (1025, 50, 1025) thin N, 17 tiles in M; (129, 131, 67) with odd lda and ldb:
    the non-vector operand load; (3000, 4000, 37) 24 x 32 = 768 tiles of 128: the BM = 128 grid,
    ragged edge tiles.  Every other case pads lda / ldb to even (NaN padding), the vector load.
    ldc = N and N + 5 (sentinel padding must come back); A and B independent, so A^T B != B^T A."""
    import torch
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    A = rng.uniform(-2, 2, (K, M))
    B = rng.uniform(-2, 2, (K, N))
    C0 = rng.uniform(-2, 2, (M, N))
    lda, ldb = (M, N) if odd else (M + (M & 1), N + (N & 1))
    assert not odd or (lda & 1 and ldb & 1)
    Ad, Bd = _padded(A, lda), _padded(B, ldb)
    prod, pbound = A.T @ B, np.abs(A).T @ np.abs(B)
    worst = 0.0
    for ldc in (N, N + 5):
        for alpha, beta in COEFS[:1] + [(-0.5, 2.0)]:
            Cd = torch.full((M, ldc), SENTINEL, dtype=torch.float64, device="cuda")
            Cd[:, :N] = float("nan") if beta == 0.0 else dev(C0)
            assert gemm_tn(M, N, K, alpha, Ad, lda, Bd, ldb, beta, Cd, ldc) == IPM_OK
            got = host(Cd)
            assert np.all(got[:, N:] == SENTINEL), "padding columns written"
            ref = alpha * prod + beta * C0
            bound = 64 * EPS * (abs(alpha) * pbound + abs(beta) * np.abs(C0))
            r = _worst(got[:, :N], ref, bound)
            assert r <= 1.0, (ldc, alpha, beta, r)
            worst = max(worst, r)
    print(f"[gemm_tn {M}x{N}x{K}] worst err / bound {worst:.3g}")


@pytest.mark.parametrize("rows,cols", [(1, 1), (31, 33), (32, 32), (33, 31), (100, 257), (257, 100)])
def test_transpose_exact(rows, cols):
    """32 x 32 tiles: below, at and past a tile in each dimension; padded ldi (NaN) and ldo (sentinel)"""
    import torch
    rng = np.random.default_rng(rows * 1000 + cols)
    a = rng.normal(size=(rows, cols))
    ldi, ldo = cols + 3, rows + 2
    out = torch.full((cols, ldo), SENTINEL, dtype=torch.float64, device="cuda")
    assert transpose(rows, cols, _padded(a, ldi), ldi, out, ldo) == IPM_OK
    got = host(out)
    np.testing.assert_array_equal(got[:, :rows], a.T)
    assert np.all(got[:, rows:] == SENTINEL)


@pytest.mark.parametrize("n", [0, 1, 1000003])
def test_copy_exact(n):
    """n = 0: no copy is enqueued; 1: one double; 1000003: an odd count past 2^20 doubles (8 MB).
    The destination past n keeps its sentinel."""
    import torch
    src = torch.arange(n + 2, dtype=torch.float64, device="cuda") * 0.5 - 7.0
    dst = torch.full((n + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    assert copy(dst, src, n) == IPM_OK
    got = host(dst)
    np.testing.assert_array_equal(got[:n], host(src)[:n])
    assert np.all(got[n:] == SENTINEL)


def test_invalid_arguments_are_rejected():
    """ldm < cols, ldc < N, a short lda / ldb / ldi / ldo and negative sizes: IPM_INVALID_ARG before
    any launch -- the NaN / sentinel outputs stay as they were"""
    import torch
    M, x = devnan((4, 8)), devnan((8,))
    y = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    for trans in (0, 1):
        assert gemv(trans, 4, 8, 1.0, M, 7, x, 0.0, y) == IPM_INVALID_ARG
        assert gemv(trans, -1, 8, 1.0, M, 8, x, 0.0, y) == IPM_INVALID_ARG
        assert gemv(trans, 4, -1, 1.0, M, 8, x, 0.0, y) == IPM_INVALID_ARG
    A, B = devnan((4, 8)), devnan((4, 8))
    C = torch.full((8, 8), SENTINEL, dtype=torch.float64, device="cuda")
    assert gemm_tn(8, 8, 4, 1.0, A, 8, B, 8, 0.0, C, 7) == IPM_INVALID_ARG
    assert gemm_tn(8, 8, 4, 1.0, A, 7, B, 8, 0.0, C, 8) == IPM_INVALID_ARG
    assert gemm_tn(8, 8, 4, 1.0, A, 8, B, 7, 0.0, C, 8) == IPM_INVALID_ARG
    for bad in ((-1, 8, 4), (8, -1, 4), (8, 8, -1)):
        assert gemm_tn(*bad, 1.0, A, 8, B, 8, 0.0, C, 8) == IPM_INVALID_ARG
    assert transpose(4, 8, A, 7, C, 8) == IPM_INVALID_ARG
    assert transpose(4, 8, A, 8, C, 3) == IPM_INVALID_ARG
    assert transpose(-1, 8, A, 8, C, 8) == IPM_INVALID_ARG
    assert transpose(4, -1, A, 8, C, 8) == IPM_INVALID_ARG
    assert copy(C, A, -1) == IPM_INVALID_ARG
    assert np.all(host(y) == SENTINEL) and np.all(host(C) == SENTINEL)
