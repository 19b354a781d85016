"""-m gpu: ipm_gemv_t2, the two-operand form of the deterministic two-stage transposed GEMV:
y = alpha [M0; M1]^T (w o x) + beta y with M0 (m0 rows, ld0) stacked over M1 (m1 rows, ld1), neither copied.
The factored-QP dual step (IPM_SOLVE_CHOLESKY_DUAL_QP) uses it for [C; F]^T (W o z).

(m0, m1) in {(0, 5), (5, 0), (1, 1), (15, 17), (16, 16), (17, 15), (63, 66), (300, 40)}: an absent operand either
side, the 16-row minimum chunk of the plan with m0 inside, at and past a chunk edge, more chunks than one, and
chunks that straddle m0.  cols in {1, 255, 256, 257, 1030}: both sides of the 256-column block and several blocks.
ld = cols, cols + 1, cols + 7 for each operand separately, NaN in the padding; weights present and absent; beta = 0
onto a NaN-filled y, and beta = 1.

Per call: the result equals ipm_gemv(trans) on a physically stacked copy (w o x formed on the host: one rounded
product per row, as the kernel forms it) BIT FOR BIT; every entry is within 64 eps sum|terms| of a long-double
product; a repeat gives the same bits.
"""
import numpy as np
import pytest

import gpu_util as G

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
ROWS = [(0, 5), (5, 0), (1, 1), (15, 17), (16, 16), (17, 15), (63, 66), (300, 40)]
COLS = [1, 255, 256, 257, 1030]
INVALID = 2


def gemv_t2(m0, m1, cols, alpha, M0, ld0, M1, ld1, x, w, beta, y):
    from ipm355 import _lib as L
    h = G.handle()
    return h.lib.ipm_gemv_t2(h.ptr, m0, m1, cols, alpha, L.dptr(M0), ld0, L.dptr(M1), ld1, L.dptr(x), L.dptr(w),
                             beta, L.dptr(y))


def _padded(rng, rows, cols, ld):
    M = np.full((max(rows, 1), ld), np.nan)
    M[:rows, :cols] = rng.uniform(-2, 2, size=(rows, cols))
    return M


def _case(rng, m0, m1, cols, ld0, ld1, weights, beta):
    import torch
    m = m0 + m1
    A0, A1 = _padded(rng, m0, cols, ld0), _padded(rng, m1, cols, ld1)
    x = rng.uniform(-2, 2, size=m)
    w = rng.uniform(0.1, 3, size=m) if weights else None
    alpha = 1.0 if beta == 0.0 else -0.75
    y0 = rng.uniform(-2, 2, size=cols)
    yd = G.devnan((cols,)) if beta == 0.0 else G.dev(y0)
    D0, D1, xd, wd = G.dev(A0), G.dev(A1), G.dev(x), (G.dev(w) if weights else None)
    assert gemv_t2(m0, m1, cols, alpha, D0, ld0, D1, ld1, xd, wd, beta, yd) == 0
    got = G.host(yd).copy()
    # the stacked copy through the one-matrix entry (no weights argument there: w o x rounded once per row)
    S = np.vstack([A0[:m0, :cols], A1[:m1, :cols]])
    xs = w * x if weights else x
    ys = G.devnan((cols,)) if beta == 0.0 else G.dev(y0)
    assert G.gemv(1, m, cols, alpha, G.dev(S), cols, G.dev(xs), beta, ys) == 0
    assert got.tobytes() == G.host(ys).tobytes(), (m0, m1, cols, ld0, ld1, weights, beta)
    # repeat: the same bits
    y2 = G.devnan((cols,)) if beta == 0.0 else G.dev(y0)
    assert gemv_t2(m0, m1, cols, alpha, D0, ld0, D1, ld1, xd, wd, beta, y2) == 0
    assert G.host(y2).tobytes() == got.tobytes()
    # entry-wise against a long-double product
    LDT = np.longdouble
    terms = S.T.astype(LDT) * xs.astype(LDT)[None, :]
    ref = alpha * terms.sum(axis=1) + (beta * y0.astype(LDT) if beta != 0.0 else 0)
    mag = abs(alpha) * np.abs(terms).sum(axis=1) + (abs(beta) * np.abs(y0) if beta != 0.0 else 0)
    err = np.abs(got.astype(LDT) - ref)
    assert np.all(err <= 64 * EPS * mag), (m0, m1, cols, ld0, ld1, weights, beta)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(mag > 0, err / (64 * EPS * mag), 0.0)))


@pytest.mark.parametrize("rows", ROWS, ids=lambda r: f"m{r[0]}+{r[1]}")
def test_equals_gemv_on_the_stacked_copy_bitwise(rows):
    m0, m1 = rows
    rng = np.random.default_rng(1000 * m0 + m1)
    worst = 0.0
    for cols in COLS:
        for ld0, ld1 in ((cols, cols), (cols + 1, cols), (cols, cols + 1), (cols + 7, cols), (cols, cols + 7),
                         (cols + 1, cols + 7)):
            for weights in (False, True):
                for beta in (0.0, 1.0):
                    worst = max(worst, _case(rng, m0, m1, cols, ld0, ld1, weights, beta))
    print(f"[m0 {m0} m1 {m1}] worst |y - y_ld| / (64 eps sum|terms|) {worst:.3g}")


def test_null_and_size_arguments_are_rejected():
    import torch
    M0 = torch.ones(4 * 6, dtype=torch.float64, device="cuda")
    M1 = torch.ones(3 * 6, dtype=torch.float64, device="cuda")
    x = torch.ones(7, dtype=torch.float64, device="cuda")
    y = torch.full((6,), -1234.5, dtype=torch.float64, device="cuda")
    assert gemv_t2(4, 3, 6, 1.0, M0, 6, M1, 6, x, None, 0.0, y) == 0
    assert np.all(G.host(y) == 7.0)
    bad = [(-1, 3, 6, 1.0, M0, 6, M1, 6, x, None, 0.0, y), (4, -1, 6, 1.0, M0, 6, M1, 6, x, None, 0.0, y),
           (4, 3, -1, 1.0, M0, 6, M1, 6, x, None, 0.0, y), (4, 3, 6, 1.0, M0, 5, M1, 6, x, None, 0.0, y),
           (4, 3, 6, 1.0, M0, 6, M1, 5, x, None, 0.0, y), (4, 3, 6, 1.0, None, 6, M1, 6, x, None, 0.0, y),
           (4, 3, 6, 1.0, M0, 6, None, 6, x, None, 0.0, y), (4, 3, 6, 1.0, M0, 6, M1, 6, None, None, 0.0, y),
           (4, 3, 6, 1.0, M0, 6, M1, 6, x, None, 0.0, None)]
    for args in bad:
        y.fill_(-1234.5)
        assert gemv_t2(*args) == INVALID, args
        assert bool((y == -1234.5).all())
    # an absent operand needs neither a pointer nor a leading dimension
    y.fill_(-1234.5)
    assert gemv_t2(0, 3, 6, 1.0, None, 0, M1, 6, x, None, 0.0, y) == 0
    assert np.all(G.host(y) == 3.0)
    assert gemv_t2(4, 0, 6, 1.0, M0, 6, None, 0, x, None, 0.0, y) == 0
    assert np.all(G.host(y) == 4.0)
