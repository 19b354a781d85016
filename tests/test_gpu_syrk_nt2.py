"""-m gpu: ipm_syrk_nt2, the weighted SYRK over TWO row-stacked row-major operands (the K assembly of
IPM_SOLVE_CHOLESKY_DUAL_EQ: X0 = C, X1 = A, neither copied).

  * the lower triangle equals ipm_syrk_nt on the physically stacked copy BIT FOR BIT (same plan, K split and
    fold order; the load width never changes the arithmetic, so this holds whichever of the 8- and 16-byte
    load paths either call takes);
  * entry by entry it is within test_gpu_syrk_nt.py's bound of a long-double product,
        |err| <= 64 eps sum_kk |X_ik w_kk X_jk|  (+ 2 eps |dvec_i| on the diagonal);
  * the strict upper triangle and the ldh padding of H keep a sentinel, the padding columns of both operands are
    NaN (a read of them would show), a NaN in a real entry propagates, a repeat call returns the same bits.

A 64-row block straddles m0 whenever m0 is not a multiple of 64: on diagonal tiles and in both operand blocks
of an off-diagonal tile (m0 = 65, 129 with m1 = 64, 65 put the seam in the second and third tile).
"""
import numpy as np
import pytest

import gpu_util as G
from test_gpu_syrk_nt import EPS, INVALID, LD, OK, SENT, check, plan, reference, weights

pytestmark = pytest.mark.gpu
M0S = [1, 15, 63, 64, 65, 129]
M1S = [1, 17, 64, 65]
KS = [1, 31, 33, 257, 1030]


def call2(m0, m1, k, X0, ldx0, X1, ldx1, w, dvec, H, ldh):
    from ipm355 import _lib as L
    h = G.handle()
    return h.lib.ipm_syrk_nt2(h.ptr, m0, m1, k, L.dptr(X0), ldx0, L.dptr(X1), ldx1, L.dptr(w), L.dptr(dvec),
                              L.dptr(H), ldh)


def call1(m, k, X, ldx, w, dvec, H, ldh):
    from ipm355 import _lib as L
    h = G.handle()
    return h.lib.ipm_syrk_nt(h.ptr, m, k, L.dptr(X), ldx, L.dptr(w), L.dptr(dvec), L.dptr(H), ldh)


def padded(X, ldx, offset=0):
    """X (rows x k host) in a NaN-filled device buffer with leading dimension ldx, `offset` doubles in"""
    rows, k = X.shape
    buf = G.devnan((max(rows, 1) * ldx + offset,))
    Xd = buf[offset:].view(max(rows, 1), ldx)
    if rows and k:
        Xd[:rows, :k] = G.dev(X)
    return Xd


def sentinel(m, ldh):
    import torch
    return torch.full((max(m, 1), ldh), SENT, dtype=torch.float64, device="cuda")


def run2(X0, X1, w, dvec, ldx0, ldx1, ldh, off0=0, off1=0):
    """(the (m, ldh) host image of H from ipm_syrk_nt2, the image from ipm_syrk_nt on the stacked copy)"""
    m0, m1, k = X0.shape[0], X1.shape[0], X0.shape[1]
    m = m0 + m1
    A0, A1 = padded(X0, ldx0, off0), padded(X1, ldx1, off1)
    wd = G.dev(w) if w is not None else None
    dd = G.dev(dvec) if dvec is not None else None
    H = sentinel(m, ldh)
    assert call2(m0, m1, k, A0, ldx0, A1, ldx1, wd, dd, H, ldh) == OK
    first = G.host(H).copy()
    assert call2(m0, m1, k, A0, ldx0, A1, ldx1, wd, dd, H, ldh) == OK
    assert first.tobytes() == G.host(H).tobytes(), "a repeat call changed bits"
    Hs = sentinel(m, ldh)
    S = padded(np.vstack([X0, X1]), max(k, 1))
    assert call1(m, k, S, max(k, 1), wd, dd, Hs, ldh) == OK
    return first, G.host(Hs)


def same_bits(a, b):
    """bitwise, NaN payloads included"""
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("m0", M0S)
def test_grid_bitwise_and_entry_by_entry(m0):
    rng = np.random.default_rng(300 + m0)
    worst = 0.0
    for m1 in M1S:
        m = m0 + m1
        for k in KS:
            X0, X1 = rng.normal(size=(m0, k)), rng.normal(size=(m1, k))
            w, dvec = weights(rng, k), rng.uniform(0.1, 1e3, m)
            Href, B = reference(np.vstack([X0, X1]), w, dvec)
            for ldx0, ldx1 in ((k, k), (k + 1, k), (k, k + 7)):
                for ldh in (m, m + 3):
                    tag = f"m0 {m0} m1 {m1} k {k} ldx {ldx0},{ldx1} ldh {ldh}"
                    img, stacked = run2(X0, X1, w, dvec, ldx0, ldx1, ldh)
                    assert same_bits(img, stacked), f"{tag}: differs from ipm_syrk_nt on the stacked copy"
                    r = check(img, m, ldh, Href, B, tag)
                    worst = max(worst, r)
                    assert r <= 1.0, (tag, r)
    print(f"[m0 = {m0}] worst err / bound over m1, k, ldx, ldh: {worst:.3g}")


@pytest.mark.parametrize("off0,off1", [(1, 0), (0, 1), (1, 1)])
def test_operand_at_an_8_byte_offset(off0, off1):
    """one (or each) operand one double into its allocation with even leading dimensions: its rows are 8-byte
    aligned only, so the launch takes the 8-byte loads for both; the stacked call takes the 16-byte ones"""
    rng = np.random.default_rng(17)
    for m0, m1, k in ((65, 17, 130), (15, 64, 1030)):
        m = m0 + m1
        X0, X1 = rng.normal(size=(m0, k)), rng.normal(size=(m1, k))
        w, dvec = weights(rng, k), rng.uniform(0.1, 10, m)
        Href, B = reference(np.vstack([X0, X1]), w, dvec)
        img, stacked = run2(X0, X1, w, dvec, k + 2, k + 4, m + 3, off0, off1)
        assert same_bits(img, stacked)
        assert check(img, m, m + 3, Href, B, f"offset {off0},{off1}") <= 1.0


@pytest.mark.parametrize("has_w,has_d", [(False, False), (False, True), (True, False), (True, True)])
def test_null_weights_and_diagonal(has_w, has_d):
    rng = np.random.default_rng(7)
    for m0, m1, k in ((15, 17, 5), (65, 64, 130), (40, 30, 1030)):
        m = m0 + m1
        X0, X1 = rng.normal(size=(m0, k)), rng.normal(size=(m1, k))
        w = weights(rng, k) if has_w else None
        dvec = rng.uniform(0.1, 10, m) if has_d else None
        Href, B = reference(np.vstack([X0, X1]), w, dvec)
        img, stacked = run2(X0, X1, w, dvec, k + 1, k, m + 3)
        assert same_bits(img, stacked)
        assert check(img, m, m + 3, Href, B, f"null m0 {m0} m1 {m1} k {k}") <= 1.0


PATHS = [
    # name, m0, m1, k, (tiles, ks, chunk) expected from the plan of m0 + m1 rows
    ("direct: k <= 512, one workgroup per tile", 100, 30, 512, (6, 1, 512)),
    ("K split, ragged rows: 70 rows in two 64-row blocks, 2048 = 8 x 256", 40, 30, 2048, (3, 8, 256)),
    ("K split capped by the 512-workgroup target: 21 tiles x 23 chunks of 288 (ragged: 164)", 200, 121, 6500,
     (21, 23, 288)),
]


@pytest.mark.parametrize("path", PATHS, ids=lambda p: p[0].split(":")[0].replace(" ", "-").replace(",", ""))
def test_launch_paths(path):
    """one shape per launch path: bitwise against the stacked call on the whole array, the long-double bound on
    sampled rows of the large one (all of their columns)"""
    name, m0, m1, k, want = path
    m = m0 + m1
    assert plan(m, k) == want, plan(m, k)
    rng = np.random.default_rng(m + k)
    X0, X1 = rng.normal(size=(m0, k)), rng.normal(size=(m1, k))
    X = np.vstack([X0, X1])
    w, dvec = weights(rng, k), rng.uniform(0.1, 1e3, m)
    img, stacked = run2(X0, X1, w, dvec, k + 1, k + 2, m + 3)
    assert same_bits(img, stacked)
    rows = np.unique(np.concatenate([[0, 63, 64, m0 - 1, m0, m - 1], rng.choice(m, min(m, 40), replace=False)]))
    rows = rows[rows < m]
    Xl, wl = X.astype(LD), w.astype(LD)
    Href = np.zeros((m, m), LD)
    Href[rows] = (Xl[rows] * wl) @ Xl.T
    B = np.zeros((m, m))
    B[rows] = 64 * EPS * ((np.abs(X[rows]) * w) @ np.abs(X).T)
    Href[rows, rows] += dvec[rows].astype(LD)
    B[rows, rows] += 2 * EPS * dvec[rows]
    r = check(img, m, m + 3, Href, B, name, rows=rows)
    print(f"[{name}] tiles, ks, chunk = {want}: err / bound {r:.3g} over {len(rows)} rows")
    assert r <= 1.0


def test_nan_reaches_every_entry_it_feeds():
    """a NaN in a real entry of either operand feeds its row and column of H (also under a zero weight), and
    nothing else"""
    rng = np.random.default_rng(11)
    for m0, m1, k in ((40, 30, 37), (40, 30, 1030)):
        m = m0 + m1
        X0, X1 = rng.normal(size=(m0, k)), rng.normal(size=(m1, k))
        w, dvec = weights(rng, k), rng.uniform(0.1, 10, m)
        low = np.tril(np.ones((m, m), bool))
        for which, i0 in ((0, 33), (1, 7)):
            for wk in (1.5, 0.0):
                Y0, Y1, wn = X0.copy(), X1.copy(), w.copy()
                (Y0 if which == 0 else Y1)[i0, k - 2] = np.nan
                wn[k - 2] = wk
                img, stacked = run2(Y0, Y1, wn, dvec, k + 1, k + 1, m)
                assert same_bits(img, stacked)
                got = img[:m, :m].T
                row = i0 + (m0 if which else 0)
                hit = np.zeros((m, m), bool)
                hit[row, :] = hit[:, row] = True
                assert np.isnan(got[low & hit]).all() and np.isfinite(got[low & ~hit]).all()


def test_m1_zero_is_syrk_nt_and_m0_zero_reads_only_x1():
    rng = np.random.default_rng(5)
    m, k = 70, 130
    X, w, dvec = rng.normal(size=(m, k)), weights(rng, k), rng.uniform(0.1, 10, m)
    Xd, wd, dd = padded(X, k + 1), G.dev(w), G.dev(dvec)
    H1, H2, H3 = sentinel(m, m + 3), sentinel(m, m + 3), sentinel(m, m + 3)
    assert call1(m, k, Xd, k + 1, wd, dd, H1, m + 3) == OK
    assert call2(m, 0, k, Xd, k + 1, None, 0, wd, dd, H2, m + 3) == OK
    assert call2(0, m, k, None, 0, Xd, k + 1, wd, dd, H3, m + 3) == OK
    assert same_bits(G.host(H1), G.host(H2)) and same_bits(G.host(H1), G.host(H3))


def test_empty_shapes():
    """k = 0: dvec (or zeros) on the diagonal, zeros below, nothing else touched; m0 = m1 = 0: IPM_OK, no store"""
    for m0, m1 in ((1, 1), (15, 2), (40, 30)):
        m = m0 + m1
        dvec = np.arange(1.0, m + 1)
        for dv in (dvec, None):
            img, stacked = run2(np.zeros((m0, 0)), np.zeros((m1, 0)), None, dv, 4, 6, m + 3)
            assert same_bits(img, stacked)
            got = img[:m, :m].T
            want = np.diag(dvec) if dv is not None else np.zeros((m, m))
            assert (np.tril(got) == want).all()
            keep = np.ones(img.shape, bool)
            keep[:m, :m] = ~np.tril(np.ones((m, m), bool)).T
            assert (img[keep] == SENT).all()
    H = sentinel(4, 4)
    X = G.devnan((8,))
    assert call2(0, 0, 5, X, 5, X, 5, None, None, H, 4) == OK
    assert call2(0, 0, 0, None, 0, None, 0, None, None, H, 0) == OK
    assert (G.host(H) == SENT).all()


def test_invalid_arguments():
    import torch
    H = torch.zeros((8, 8), dtype=torch.float64, device="cuda")
    X = torch.zeros((8, 8), dtype=torch.float64, device="cuda")
    assert call2(-1, 2, 4, X, 8, X, 8, None, None, H, 8) == INVALID
    assert call2(2, -1, 4, X, 8, X, 8, None, None, H, 8) == INVALID
    assert call2(2, 2, -1, X, 8, X, 8, None, None, H, 8) == INVALID
    assert call2(2, 2, 4, X, 3, X, 8, None, None, H, 8) == INVALID      # ldx0 < k
    assert call2(2, 2, 4, X, 8, X, 3, None, None, H, 8) == INVALID      # ldx1 < k
    assert call2(2, 2, 4, X, 8, X, 8, None, None, H, 3) == INVALID      # ldh < m0 + m1
    assert call2(2, 2, 4, None, 8, X, 8, None, None, H, 8) == INVALID   # null X0
    assert call2(2, 2, 4, X, 8, None, 8, None, None, H, 8) == INVALID   # null X1
    assert call2(2, 2, 4, X, 8, X, 8, None, None, None, 8) == INVALID   # null H
    assert call2(2, 0, 4, X, 3, None, 0, None, None, H, 8) == INVALID   # m1 = 0: ipm_syrk_nt's checks
