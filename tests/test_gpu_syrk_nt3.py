"""-m gpu: ipm_syrk_nt3, the weighted SYRK over THREE row-stacked row-major operands (the K assembly of
IPM_SOLVE_CHOLESKY_DUAL_QP_EQ: X0 = C, X1 = Pf, X2 = A, none copied).

  * the lower triangle equals ipm_syrk_nt on the physically stacked copy BIT FOR BIT (same plan, K split and fold
    order, whichever of the 8- and 16-byte load paths either call takes); with m2 = 0 also ipm_syrk_nt2's;
  * entry by entry it is within test_gpu_syrk_nt.py's bound of a long-double product,
        |err| <= 64 eps sum_kk |X_ik w_kk X_jk|  (+ 2 eps |dvec_i| on the diagonal);
  * the strict upper triangle, the ldh padding of H and the rows beyond m0 + m1 + m2 keep a sentinel, the padding
    columns of all operands are NaN (a read of them would show), three calls give the same bits.

Row blocks: an empty block in each position ((0,5,3), (5,0,3), (5,3,0), (0,0,5)), a seam one row before / after
a 64-row tile edge ((63,1,1), (1,63,1)), both seams on tile edges ((64,64,64)), the second seam on one
((40,24,17): 40 + 24 = 64), one tile straddling both seams ((63,1,1), (1,63,1) and rows 64..127 of (40,24,17) do
not; (30,10,30) does: rows 0..63 hold all three), and several tiles per block ((100,100,100)).  k: short of, at
and past the 32-column stage, 520 and 1030 (past 512 the plan cuts k into chunks; both leave a ragged last one).
Leading dimensions k, k + 1, k + 3 per operand: exactly one, two or no operand disqualifies the 16-byte loads.
"""
import numpy as np
import pytest

import gpu_util as G
from test_gpu_syrk_nt import EPS, INVALID, LD, OK, SENT, check, plan, reference, weights
from test_gpu_syrk_nt2 import call1, call2, padded, same_bits

pytestmark = pytest.mark.gpu
BLOCKS = [(0, 5, 3), (5, 0, 3), (5, 3, 0), (0, 0, 5), (63, 1, 1), (1, 63, 1), (64, 64, 64), (40, 24, 17),
          (30, 10, 30), (100, 100, 100)]
KS = [1, 31, 32, 33, 520, 1030]
GUARD = 3   # sentinel rows of H beyond m0 + m1 + m2


def call3(m0, m1, m2, k, X0, ldx0, X1, ldx1, X2, ldx2, w, dvec, H, ldh):
    from ipm355 import _lib as L
    h = G.handle()
    return h.lib.ipm_syrk_nt3(h.ptr, m0, m1, m2, k, L.dptr(X0), ldx0, L.dptr(X1), ldx1, L.dptr(X2), ldx2, L.dptr(w),
                              L.dptr(dvec), L.dptr(H), ldh)


def sentinel(m, ldh):
    """column j of H in row j; GUARD more rows (columns of H beyond m) that no call may touch"""
    import torch
    return torch.full((max(m, 1) + GUARD, ldh), SENT, dtype=torch.float64, device="cuda")


def run3(Xs, w, dvec, lds, ldh, offs=(0, 0, 0)):
    """(the (m, ldh) image of H from ipm_syrk_nt3, the image from ipm_syrk_nt on the stacked copy)"""
    ms, k = [X.shape[0] for X in Xs], Xs[0].shape[1]
    m = sum(ms)
    D = [padded(X, ld, off) for X, ld, off in zip(Xs, lds, offs)]
    wd = G.dev(w) if w is not None else None
    dd = G.dev(dvec) if dvec is not None else None
    imgs = []
    for _ in range(3):
        H = sentinel(m, ldh)
        assert call3(ms[0], ms[1], ms[2], k, D[0], lds[0], D[1], lds[1], D[2], lds[2], wd, dd, H, ldh) == OK
        full = G.host(H)
        assert (full[max(m, 1):] == SENT).all(), "wrote beyond row / column m0 + m1 + m2"
        imgs.append(full[:max(m, 1)].copy())
    assert same_bits(imgs[0], imgs[1]) and same_bits(imgs[0], imgs[2]), "a repeat call changed bits"
    Hs = sentinel(m, ldh)
    S = padded(np.vstack(Xs), max(k, 1))
    assert call1(m, k, S, max(k, 1), wd, dd, Hs, ldh) == OK
    return imgs[0], G.host(Hs)[:max(m, 1)]


@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: "m%d+%d+%d" % b)
def test_grid_bitwise_and_entry_by_entry(blocks):
    m = sum(blocks)
    rng = np.random.default_rng(1000 * blocks[0] + 10 * blocks[1] + blocks[2])
    worst = 0.0
    for k in KS:
        Xs = [rng.normal(size=(mi, k)) for mi in blocks]
        w, dvec = weights(rng, k), rng.uniform(0.1, 1e3, m)
        Href, B = reference(np.vstack(Xs), w, dvec)
        # all qualify (k even) / exactly one operand odd, each in turn / all odd or mixed
        for lds in ((k, k, k), (k + 1, k, k), (k, k + 1, k), (k, k, k + 1), (k + 1, k + 3, k), (k + 3, k + 1, k + 3)):
            ldh = m + (0 if lds[0] == k else 3)
            tag = f"blocks {blocks} k {k} ldx {lds} ldh {ldh}"
            img, stacked = run3(Xs, w, dvec, lds, ldh)
            assert same_bits(img, stacked), f"{tag}: differs from ipm_syrk_nt on the stacked copy"
            r = check(img, m, ldh, Href, B, tag)
            worst = max(worst, r)
            assert r <= 1.0, (tag, r)
    print(f"[blocks {blocks}] worst err / bound over k, ldx, ldh: {worst:.3g}")


def test_k_split_plans_are_the_stacked_matrix_s():
    """the shapes above reach both launch forms: no split up to k = 512, a split at 520 and 1030"""
    assert plan(192, 33)[1] == 1 and plan(300, 512)[1] == 1
    for m in (5, 8, 65, 81, 70, 192, 300):
        for k in (520, 1030):
            nt, ks, chunk = plan(m, k)
            assert ks > 1 and k % chunk != 0, (m, k, ks, chunk)


@pytest.mark.parametrize("offs", [(1, 0, 0), (0, 1, 0), (0, 0, 1)])
def test_one_operand_at_an_odd_element_offset(offs):
    """one operand one double into its allocation with even leading dimensions everywhere: its rows are 8-byte
    aligned only, so the call takes the 8-byte loads for all three; the stacked call takes the 16-byte ones"""
    rng = np.random.default_rng(17)
    for blocks, k in (((63, 1, 1), 130), ((40, 24, 17), 1030)):
        m = sum(blocks)
        Xs = [rng.normal(size=(mi, k)) for mi in blocks]
        w, dvec = weights(rng, k), rng.uniform(0.1, 10, m)
        Href, B = reference(np.vstack(Xs), w, dvec)
        img, stacked = run3(Xs, w, dvec, (k + 2, k + 4, k), m + 3, offs)
        assert same_bits(img, stacked)
        assert check(img, m, m + 3, Href, B, f"offset {offs}") <= 1.0


@pytest.mark.parametrize("has_w,has_d", [(False, False), (False, True), (True, False), (True, True)])
def test_null_weights_and_diagonal(has_w, has_d):
    rng = np.random.default_rng(7)
    for blocks, k in (((5, 3, 4), 5), ((40, 24, 17), 130), ((30, 10, 30), 1030)):
        m = sum(blocks)
        Xs = [rng.normal(size=(mi, k)) for mi in blocks]
        w = weights(rng, k) if has_w else None
        dvec = rng.uniform(0.1, 10, m) if has_d else None
        Href, B = reference(np.vstack(Xs), w, dvec)
        img, stacked = run3(Xs, w, dvec, (k + 1, k, k + 3), m + 3)
        assert same_bits(img, stacked)
        assert check(img, m, m + 3, Href, B, f"null blocks {blocks} k {k}") <= 1.0


def test_empty_blocks_fall_back_and_never_read_their_pointer():
    """m2 = 0 is ipm_syrk_nt2 bit for bit, m1 = m2 = 0 ipm_syrk_nt; an empty block takes a null pointer and a
    zero leading dimension"""
    import torch
    rng = np.random.default_rng(5)
    k = 130
    X0, X1 = rng.normal(size=(5, k)), rng.normal(size=(3, k))
    w, dvec = weights(rng, k), rng.uniform(0.1, 10, 8)
    D0, D1, wd, dd = padded(X0, k + 1), padded(X1, k + 3), G.dev(w), G.dev(dvec)
    H3, H2 = sentinel(8, 11), sentinel(8, 11)
    assert call3(5, 3, 0, k, D0, k + 1, D1, k + 3, None, 0, wd, dd, H3, 11) == OK
    assert call2(5, 3, k, D0, k + 1, D1, k + 3, wd, dd, H2, 11) == OK
    assert same_bits(G.host(H3), G.host(H2))
    for blocks, ops in (((5, 0, 3), (D0, None, D1)), ((0, 5, 3), (None, D0, D1))):
        H = sentinel(8, 11)
        lds = [0 if o is None else (k + 1 if o is D0 else k + 3) for o in ops]
        assert call3(*blocks, k, ops[0], lds[0], ops[1], lds[1], ops[2], lds[2], wd, dd, H, 11) == OK
        assert same_bits(G.host(H), G.host(H2)), blocks
    H1, Hn = sentinel(5, 8), sentinel(5, 8)
    assert call1(5, k, D0, k + 1, wd, dd, H1, 8) == OK
    for blocks, ops in (((5, 0, 0), (D0, None, None)), ((0, 5, 0), (None, D0, None)), ((0, 0, 5), (None, None, D0))):
        Hn.fill_(SENT)
        lds = [0 if o is None else k + 1 for o in ops]
        assert call3(*blocks, k, ops[0], lds[0], ops[1], lds[1], ops[2], lds[2], wd, dd, Hn, 8) == OK
        assert same_bits(G.host(Hn), G.host(H1)), blocks
    # no rows at all: IPM_OK and no store (with the one-operand entry's argument rules: ldx >= k)
    Hn.fill_(SENT)
    assert call3(0, 0, 0, k, D0, k + 1, D0, k + 1, D0, k + 1, None, None, Hn, 8) == OK
    assert call3(0, 0, 0, 0, None, 0, None, 0, None, 0, None, None, Hn, 0) == OK
    assert bool((Hn == SENT).all())


def test_nan_reaches_every_entry_it_feeds():
    """a NaN in a real entry of any operand feeds its row and column of H, and nothing else"""
    rng = np.random.default_rng(11)
    blocks, k = (30, 10, 30), 37
    m = sum(blocks)
    Xs = [rng.normal(size=(mi, k)) for mi in blocks]
    w, dvec = weights(rng, k), rng.uniform(0.1, 10, m)
    low = np.tril(np.ones((m, m), bool))
    for which, i0 in ((0, 29), (1, 0), (2, 7)):
        Ys = [X.copy() for X in Xs]
        Ys[which][i0, k - 2] = np.nan
        img, stacked = run3(Ys, w, dvec, (k + 1, k + 1, k + 1), m)
        assert same_bits(img, stacked)
        got = img[:m, :m].T
        row = i0 + sum(blocks[:which])
        hit = np.zeros((m, m), bool)
        hit[row, :] = hit[:, row] = True
        assert np.isnan(got[low & hit]).all() and np.isfinite(got[low & ~hit]).all()


def test_invalid_arguments():
    import torch
    H = torch.zeros((8, 8), dtype=torch.float64, device="cuda")
    X = torch.zeros((8, 8), dtype=torch.float64, device="cuda")
    good = [2, 2, 2, 4, X, 8, X, 8, X, 8, None, None, H, 8]
    assert call3(*good) == OK
    for pos, val in ((0, -1), (1, -1), (2, -1), (3, -1),           # a negative size
                     (5, 3), (7, 3), (9, 3),                       # a leading dimension below k
                     (13, 5),                                      # ldh < m0 + m1 + m2
                     (4, None), (6, None), (8, None), (12, None)):  # a null operand with rows, a null H
        args = list(good)
        args[pos] = val
        assert call3(*args) == INVALID, (pos, val)
    assert call3(2, 2, 0, 4, X, 3, X, 8, None, 0, None, None, H, 8) == INVALID   # m2 = 0: ipm_syrk_nt2's checks
