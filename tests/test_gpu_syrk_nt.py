"""-m gpu: ipm_syrk_nt, the weighted SYRK over the contiguous index of a row-major operand
(H = X diag(w) X^T + diag(dvec), lower triangle, column-major), entry by entry against long double:

    |err| <= 64 eps sum_kk |X_ik w_kk X_jk|     (+ 2 eps |dvec_i| on the diagonal)

The strict upper triangle and the padding of H are pre-filled with a sentinel and must come back bit
for bit; the padding of X is NaN; a second call must return the same bits.

Launch paths of syrk_nt_lower (csrc/ipm_syrk_nt.h, mirrored by ``plan`` below): 64 x 64 tiles of the
lower triangle; with fewer than 256 tiles and k > 512 the k range is cut into ks chunks (multiples of
32 columns, about 512 workgroups in all, no chunk under 256 columns) whose partial tiles a second
launch adds in order.  A chunk is never empty by construction (ks = ceil(k / chunk)); the last one is
ragged whenever chunk does not divide k.  16-byte loads when X and ldx are 16-byte aligned, 8-byte
loads otherwise.
"""
import numpy as np
import pytest

import gpu_util as G

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble
SENT = -7.25e33
MS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257]
KS = [1, 3, 4, 5, 15, 17, 64, 65, 130, 1030]
OK, INVALID = 0, 2


def plan(m, k):
    """(tiles, ks, chunk) as syrk_nt_plan computes them"""
    T = (m + 63) // 64
    nt = T * (T + 1) // 2
    ks, chunk = 1, (max(k, 1) + 31) // 32 * 32
    if nt < 256 and k > 512:
        want = min((512 + nt - 1) // nt, (k + 255) // 256)
        chunk = ((k + want - 1) // want + 31) // 32 * 32
        ks = (k + chunk - 1) // chunk
    return nt, ks, chunk


def weights(rng, k):
    """spread over 1e-12 .. 1e6, with exact zeros among them"""
    w = 10.0 ** rng.uniform(-12, 6, k)
    if k >= 3:
        w[rng.choice(k, max(1, k // 5), replace=False)] = 0.0
    return w


def call(m, k, X, ldx, w, dvec, H, ldh):
    from ipm355 import _lib as L
    h = G.handle()
    return h.lib.ipm_syrk_nt(h.ptr, m, k, L.dptr(X), ldx, L.dptr(w), L.dptr(dvec), L.dptr(H), ldh)


def run(X, w, dvec, ldx, ldh, offset=0):
    """X (m x k host) in a NaN-padded device buffer (leading dimension ldx, `offset` doubles into the
    allocation), H pre-filled with the sentinel -> the (m, ldh) host image of H, column j in row j"""
    import torch
    m, k = X.shape
    buf = G.devnan((m * ldx + offset,))
    Xd = buf[offset:].view(m, ldx) if m else buf[offset:]
    if m and k:
        Xd[:, :k] = G.dev(X)
    wd = G.dev(w) if w is not None else None
    dd = G.dev(dvec) if dvec is not None else None
    H = torch.full((max(m, 1), ldh), SENT, dtype=torch.float64, device="cuda")
    assert call(m, k, Xd, ldx, wd, dd, H, ldh) == OK
    first = G.host(H).copy()
    assert call(m, k, Xd, ldx, wd, dd, H, ldh) == OK
    second = G.host(H)
    assert first.tobytes() == second.tobytes(), "a repeat call changed bits"
    return first


def reference(X, w, dvec):
    """(long-double H, entrywise bound) of the full symmetric product"""
    m, k = X.shape
    wl = np.ones(k, LD) if w is None else w.astype(LD)
    Xl = X.astype(LD)
    H = (Xl * wl) @ Xl.T
    B = 64 * EPS * ((np.abs(X) * np.abs(np.ones(k) if w is None else w)) @ np.abs(X).T)
    if dvec is not None:
        H[np.diag_indices(m)] += dvec.astype(LD)
        B[np.diag_indices(m)] += 2 * EPS * np.abs(dvec)
    return H, B


def check(img, m, ldh, Href, B, tag, rows=None):
    """the lower triangle within the bound; everything else still the sentinel"""
    got = img[:m, :m].T                                 # got[i, j] = H(i, j)
    low = np.tril(np.ones((m, m), bool))
    keep = np.ones(img.shape, bool)
    keep[:m, :m] = ~low.T
    assert (img[keep] == SENT).all(), f"{tag}: wrote outside the lower triangle"
    sel = low if rows is None else low & np.isin(np.arange(m), rows)[:, None]
    err = np.abs((got.astype(LD) - Href).astype(np.float64))
    assert np.isfinite(got[sel]).all(), f"{tag}: non-finite entry"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(sel, np.where(B > 0, err / B, np.where(err == 0, 0.0, np.inf)), 0.0)
    return float(ratio.max()) if m else 0.0


@pytest.mark.parametrize("m", MS)
def test_shapes_entry_by_entry(m):
    """m = 1 .. 257 (1, 3, 6 and 15 tiles; rows short of, at and past the 16-row MFMA block and the
    64-row tile) by k = 1 .. 1030 (short of, at and past the 4-column MFMA step and the 32-column
    stage; 1030: the K split with a ragged last chunk), ldx = k, k + 1, k + 7 (both load widths) and
    ldh = m, m + 3"""
    rng = np.random.default_rng(100 + m)
    worst = 0.0
    for k in KS:
        X = rng.normal(size=(m, k))
        w, dvec = weights(rng, k), rng.uniform(0.1, 1e3, m)
        Href, B = reference(X, w, dvec)
        for ldx in (k, k + 1, k + 7):
            for ldh in (m, m + 3):
                img = run(X, w, dvec, ldx, ldh)
                r = check(img, m, ldh, Href, B, f"m{m} k{k} ldx{ldx} ldh{ldh}")
                worst = max(worst, r)
                assert r <= 1.0, (m, k, ldx, ldh, r)
    print(f"[m = {m}] worst err / bound over k, ldx, ldh: {worst:.3g}")


@pytest.mark.parametrize("has_w,has_d", [(False, False), (False, True), (True, False)])
def test_null_weights_and_diagonal(has_w, has_d):
    rng = np.random.default_rng(7)
    for m, k in ((17, 5), (65, 130), (70, 1030)):
        X = rng.normal(size=(m, k))
        w = weights(rng, k) if has_w else None
        dvec = rng.uniform(0.1, 10, m) if has_d else None
        Href, B = reference(X, w, dvec)
        r = check(run(X, w, dvec, k + 1, m + 3), m, m + 3, Href, B, f"null m{m} k{k}")
        assert r <= 1.0, (m, k, r)


def test_unaligned_base_pointer():
    """X one double into its allocation with an even ldx: rows 8-byte aligned only -> the 8-byte loads"""
    rng = np.random.default_rng(8)
    m, k = 65, 130
    X, w, dvec = rng.normal(size=(m, k)), weights(rng, k), rng.uniform(0.1, 10, m)
    Href, B = reference(X, w, dvec)
    assert check(run(X, w, dvec, k + 2, m, offset=1), m, m, Href, B, "offset") <= 1.0


def test_empty_shapes():
    """k = 0: dvec (or zeros) on the diagonal, zeros below, nothing else touched; m = 0: IPM_OK and
    no store at all"""
    import torch
    for m in (1, 17, 65):
        dvec = np.arange(1.0, m + 1)
        for dv in (dvec, None):
            img = run(np.zeros((m, 0)), None, dv, 4, m + 3)
            got = img[:m, :m].T
            want = np.diag(dvec) if dv is not None else np.zeros((m, m))
            assert (np.tril(got) == want).all()
            keep = np.ones(img.shape, bool)
            keep[:m, :m] = ~np.tril(np.ones((m, m), bool)).T
            assert (img[keep] == SENT).all()
    H = torch.full((4, 4), SENT, dtype=torch.float64, device="cuda")
    X = G.devnan((8,))
    assert call(0, 5, X, 5, None, None, H, 4) == OK
    assert call(0, 0, None, 0, None, None, H, 0) == OK
    assert (G.host(H) == SENT).all()


def test_invalid_arguments():
    import torch
    H = torch.zeros((8, 8), dtype=torch.float64, device="cuda")
    X = torch.zeros((8, 8), dtype=torch.float64, device="cuda")
    assert call(-1, 4, X, 8, None, None, H, 8) == INVALID
    assert call(4, -1, X, 8, None, None, H, 8) == INVALID
    assert call(4, 4, X, 3, None, None, H, 8) == INVALID      # ldx < k
    assert call(4, 4, X, 8, None, None, H, 3) == INVALID      # ldh < m
    assert call(4, 4, None, 8, None, None, H, 8) == INVALID   # null X
    assert call(4, 4, X, 8, None, None, None, 8) == INVALID   # null H


PATHS = [
    # name, m, k, (tiles, ks, chunk) expected from the plan
    ("direct: k <= 512, one workgroup per tile", 130, 512, (6, 1, 512)),
    ("K split, ragged last chunk: 1030 = 4 x 224 + 134", 65, 1030, (3, 5, 224)),
    ("K split, chunks divide k: 2048 = 8 x 256", 130, 2048, (6, 8, 256)),
    ("K split capped by the 512-workgroup target: 21 tiles x 23 chunks of 288 (ragged: 164)", 321, 6500,
     (21, 23, 288)),
    ("direct: 276 tiles >= 256, k > 512 left whole", 1409, 520, (276, 1, 544)),
]


@pytest.mark.parametrize("path", PATHS, ids=lambda p: p[0].split(":")[0].replace(" ", "-").replace(",", ""))
def test_launch_paths(path):
    """one shape per launch path; the large ones are compared on 48 sampled rows of H (all of their
    columns), the sentinel and the repeat on the whole array"""
    name, m, k, want = path
    assert plan(m, k) == want, plan(m, k)
    rng = np.random.default_rng(m + k)
    X, w, dvec = rng.normal(size=(m, k)), weights(rng, k), rng.uniform(0.1, 1e3, m)
    img = run(X, w, dvec, k + 1, m + 3)
    rows = np.unique(np.concatenate([[0, 63, 64, m - 1], rng.choice(m, min(m, 44), replace=False)]))
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


@pytest.mark.parametrize("m,k", [(70, 37), (70, 1030), (17, 3)])
def test_exact_integers_pin_the_lane_maps(m, k):
    """small integers: every product and partial sum is exact, so H must equal the integer result
    bit for bit -- a wrong MFMA row / column map, a dropped or doubled k column, a swapped tile or a
    misplaced K-split partial cannot hide inside a tolerance"""
    rng = np.random.default_rng(m * k)
    X = rng.integers(-3, 4, (m, k)).astype(np.float64)
    w = rng.integers(0, 5, k).astype(np.float64)
    dvec = rng.integers(1, 9, m).astype(np.float64)
    Xi = X.astype(np.int64)
    want = (Xi * w.astype(np.int64)) @ Xi.T + np.diag(dvec.astype(np.int64))
    for ldx in (k, k + 1):
        img = run(X, w, dvec, ldx, m + 3)
        got = np.tril(img[:m, :m].T)
        assert (got == np.tril(want).astype(np.float64)).all()


def test_nan_reaches_every_entry_it_feeds():
    rng = np.random.default_rng(11)
    for m, k in ((70, 37), (70, 1030)):
        X, w, dvec = rng.normal(size=(m, k)), weights(rng, k), rng.uniform(0.1, 10, m)
        low = np.tril(np.ones((m, m), bool))
        # a NaN in X[i0, k0] feeds row i0 and column i0 of H, even under a zero weight
        i0, k0 = 33, k - 2
        for wk in (w[k0], 0.0):
            Xn, wn = X.copy(), w.copy()
            Xn[i0, k0], wn[k0] = np.nan, wk
            got = run(Xn, wn, dvec, k + 1, m)[:m, :m].T
            hit = np.zeros((m, m), bool)
            hit[i0, :] = hit[:, i0] = True
            assert np.isnan(got[low & hit]).all() and np.isfinite(got[low & ~hit]).all()
        # a NaN weight feeds every entry
        wn = w.copy()
        wn[k0] = np.nan
        got = run(X, wn, dvec, k + 1, m)[:m, :m].T
        assert np.isnan(got[low]).all()
        # a NaN in dvec stays on its diagonal entry
        dn = dvec.copy()
        dn[5] = np.nan
        got = run(X, w, dn, k, m)[:m, :m].T
        only = np.zeros((m, m), bool)
        only[5, 5] = True
        assert np.isnan(got[only]).all() and np.isfinite(got[low & ~only]).all()
