"""-m gpu: ipm_gemv_t3 and ipm_gemv_n3, the three-operand forms of the two GEMVs (M = [C; Pf; A] of
IPM_SOLVE_CHOLESKY_DUAL_QP_EQ: three row-major matrices with their own leading dimensions, none copied).

  ipm_gemv_t3: y = alpha [M0; M1; M2]^T (w o x) + beta y -- BIT FOR BIT ipm_gemv(trans) on a physically stacked
               copy (w o x formed on the host: one rounded product per row, as the kernel forms it), so the
               same row chunks, partial sums and fold order; no atomics, a repeat gives the same bits.
  ipm_gemv_n3: y = [M0 x; M1 x; M2 x] in one launch -- every entry BIT FOR BIT ipm_gemv(no trans) of its row.

Both: every entry within 64 eps sum|terms| of a long-double product; NaN in the padding of every operand;
beta = 0 onto a NaN-filled y; weights present and absent; leading dimensions cols, cols + 1, cols + 3 mixed per
operand and one operand at an odd element offset (mixed 16-byte alignment: ipm_gemv_n3 then takes separate
launches).

Row blocks: test_gpu_syrk_nt3.py's and (5,3,20).  ``t_plan`` mirrors gemv_t_plan (16-row chunks at these
sizes) and ``straddles`` reads from it which seams fall strictly inside a row chunk: the first alone, the second
alone, each in a chunk of its own ((30,10,30)) and BOTH in one chunk ((5,3,20): rows 0..15 hold all three
blocks); a test asserts that each kind occurs in the list.
"""
import numpy as np
import pytest

import gpu_util as G

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LDT = np.longdouble
BLOCKS = [(0, 5, 3), (5, 0, 3), (5, 3, 0), (0, 0, 5), (63, 1, 1), (1, 63, 1), (64, 64, 64), (40, 24, 17),
          (30, 10, 30), (5, 3, 20), (100, 100, 100)]
COLS = [1, 255, 257, 1030]
INVALID = 2


def t_plan(rows, cols):
    """(rchunk, nchunk) as gemv_t_plan computes them"""
    cb = (cols + 255) // 256
    want = max(1, 2048 // max(cb, 1))
    rc = max(16, (rows + want - 1) // want)
    return rc, max(1, (rows + rc - 1) // rc)


def straddles(blocks, cols):
    """which seams lie strictly inside a row chunk of the plan: (first, second, both in ONE chunk)"""
    m0, m1, m2 = blocks
    rc, _ = t_plan(sum(blocks), cols)
    s0, s1 = m0, m0 + m1
    in0 = m0 > 0 and m1 + m2 > 0 and s0 % rc != 0
    in1 = m2 > 0 and m0 + m1 > 0 and s1 % rc != 0
    both = in0 and in1 and m1 > 0 and s0 // rc == s1 // rc
    return in0, in1, both


def test_the_block_list_straddles_each_seam_and_both():
    kinds = np.array([straddles(b, c) for b in BLOCKS for c in COLS])
    assert kinds[:, 0].any() and kinds[:, 1].any() and kinds[:, 2].any()
    assert straddles((5, 3, 20), 257) == (True, True, True)
    assert straddles((64, 64, 64), 257) == (False, False, False)
    assert t_plan(300, 1030) == (16, 19)


def gemv_t3(ms, cols, alpha, Ms, lds, x, w, beta, y):
    from ipm355 import _lib as L
    h = G.handle()
    return h.lib.ipm_gemv_t3(h.ptr, ms[0], ms[1], ms[2], cols, alpha, L.dptr(Ms[0]), lds[0], L.dptr(Ms[1]), lds[1],
                             L.dptr(Ms[2]), lds[2], L.dptr(x), L.dptr(w), beta, L.dptr(y))


def gemv_n3(ms, cols, Ms, lds, x, y):
    from ipm355 import _lib as L
    h = G.handle()
    return h.lib.ipm_gemv_n3(h.ptr, ms[0], ms[1], ms[2], cols, L.dptr(Ms[0]), lds[0], L.dptr(Ms[1]), lds[1],
                             L.dptr(Ms[2]), lds[2], L.dptr(x), L.dptr(y))


def _operands(rng, blocks, cols, lds, offs):
    """host blocks, and their NaN-padded device images (leading dimension ld, `off` doubles into the allocation)"""
    Hs, Ds = [], []
    for rows, ld, off in zip(blocks, lds, offs):
        M = rng.uniform(-2, 2, size=(rows, cols))
        buf = G.devnan((max(rows, 1) * ld + off,))
        D = buf[off:].view(max(rows, 1), ld)
        if rows:
            D[:rows, :cols] = G.dev(M)
        Hs.append(M)
        Ds.append(D)
    return Hs, Ds


def _ratio(got, ref, mag):
    err = np.abs(got.astype(LDT) - ref)
    assert np.all(err <= 64 * EPS * mag)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(mag > 0, err / (64 * EPS * mag), 0.0))) if len(got) else 0.0


def _case_t(rng, blocks, cols, lds, offs, weights, beta):
    m = sum(blocks)
    Hs, Ds = _operands(rng, blocks, cols, lds, offs)
    x = rng.uniform(-2, 2, size=m)
    w = rng.uniform(0.1, 3, size=m) if weights else None
    alpha = 1.0 if beta == 0.0 else -0.75
    y0 = rng.uniform(-2, 2, size=cols)
    fresh = (lambda: G.devnan((cols,))) if beta == 0.0 else (lambda: G.dev(y0))
    xd, wd = G.dev(x), (G.dev(w) if weights else None)
    yd = fresh()
    assert gemv_t3(blocks, cols, alpha, Ds, lds, xd, wd, beta, yd) == 0
    got = G.host(yd).copy()
    S = np.vstack(Hs)
    xs = w * x if weights else x
    ys = fresh()
    assert G.gemv(1, m, cols, alpha, G.dev(S), cols, G.dev(xs), beta, ys) == 0
    assert got.tobytes() == G.host(ys).tobytes(), (blocks, cols, lds, offs, weights, beta)
    y2 = fresh()
    assert gemv_t3(blocks, cols, alpha, Ds, lds, xd, wd, beta, y2) == 0
    assert G.host(y2).tobytes() == got.tobytes(), "a repeat call changed bits"
    terms = S.T.astype(LDT) * xs.astype(LDT)[None, :]
    ref = alpha * terms.sum(axis=1) + (beta * y0.astype(LDT) if beta != 0.0 else 0)
    mag = abs(alpha) * np.abs(terms).sum(axis=1) + (abs(beta) * np.abs(y0) if beta != 0.0 else 0)
    return _ratio(got, ref, mag)


def _case_n(rng, blocks, cols, lds, offs, xoff=0):
    m = sum(blocks)
    Hs, Ds = _operands(rng, blocks, cols, lds, offs)
    x = rng.uniform(-2, 2, size=cols)
    xd = G.devnan((cols + xoff,))[xoff:]
    xd.copy_(G.dev(x))
    yd = G.devnan((m + 2,))            # two guard entries past the end stay NaN
    assert gemv_n3(blocks, cols, Ds, lds, xd, yd) == 0
    got = G.host(yd).copy()
    assert np.isnan(got[m:]).all(), "wrote past y"
    got = got[:m]
    # row by row what the one-matrix entry gives on each operand where it lies
    want = []
    for rows, D, ld in zip(blocks, Ds, lds):
        yo = G.devnan((max(rows, 1),))
        assert G.gemv(0, rows, cols, 1.0, D, ld, xd, 0.0, yo) == 0
        want.append(G.host(yo)[:rows])
    assert got.tobytes() == np.concatenate(want).tobytes(), (blocks, cols, lds, offs)
    # ... and on a physically stacked copy.  ipm_gemv sums a row in one of two orders, by the 16-byte alignment of
    # its rows and of x; the copy gets the leading dimension that gives it the operands' order.  Operands of mixed
    # alignment have no single order (ipm_gemv_n3 then takes separate launches): the row-by-row check above is
    # the whole statement there.
    S = np.vstack(Hs)
    vec = {ld % 2 == 0 and off % 2 == 0 and xoff % 2 == 0 for ld, off, r in zip(lds, offs, blocks) if r}
    if len(vec) == 1:
        ld_s = cols + (cols % 2 if vec.pop() else 1 - cols % 2)
        Sd = G.devnan((m, ld_s))
        Sd[:, :cols] = G.dev(S)
        ys = G.devnan((m,))
        assert G.gemv(0, m, cols, 1.0, Sd, ld_s, xd, 0.0, ys) == 0
        assert got.tobytes() == G.host(ys).tobytes(), (blocks, cols, lds, offs)
    y2 = G.devnan((m + 2,))
    assert gemv_n3(blocks, cols, Ds, lds, xd, y2) == 0
    assert G.host(y2)[:m].tobytes() == got.tobytes(), "a repeat call changed bits"
    terms = S.astype(LDT) * x.astype(LDT)[None, :]
    return _ratio(got, terms.sum(axis=1), np.abs(terms).sum(axis=1))


def _lds(cols):
    return ((cols, cols, cols), (cols + 1, cols, cols), (cols, cols + 1, cols), (cols, cols, cols + 1),
            (cols + 1, cols + 3, cols), (cols + 3, cols + 1, cols + 3))


@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: "m%d+%d+%d" % b)
def test_gemv_t3_equals_gemv_on_the_stacked_copy_bitwise(blocks):
    rng = np.random.default_rng(1000 * blocks[0] + 10 * blocks[1] + blocks[2])
    worst = 0.0
    for cols in COLS:
        for lds in _lds(cols):
            for weights, beta in ((False, 0.0), (True, 0.0), (True, 1.0)):
                worst = max(worst, _case_t(rng, blocks, cols, lds, (0, 0, 0), weights, beta))
        worst = max(worst, _case_t(rng, blocks, cols, (cols + 2, cols + 4, cols + 2), (0, 1, 0), True, 0.0))
    print(f"[t3 blocks {blocks}] worst |y - y_ld| / (64 eps sum|terms|) {worst:.3g}")


@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: "m%d+%d+%d" % b)
def test_gemv_n3_rows_are_gemv_s_bitwise(blocks):
    rng = np.random.default_rng(2000 * blocks[0] + 20 * blocks[1] + blocks[2])
    worst = 0.0
    for cols in COLS + [256, 2050]:
        for lds in _lds(cols):
            worst = max(worst, _case_n(rng, blocks, cols, lds, (0, 0, 0)))
        for offs in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            worst = max(worst, _case_n(rng, blocks, cols, (cols + 2, cols + 4, cols + 2), offs))
        worst = max(worst, _case_n(rng, blocks, cols, (cols + 2, cols + 4, cols + 2), (0, 0, 0), xoff=1))
    print(f"[n3 blocks {blocks}] worst |y - y_ld| / (64 eps sum|terms|) {worst:.3g}")


def test_null_and_size_arguments_are_rejected():
    import torch
    M = [torch.ones(r * 6, dtype=torch.float64, device="cuda") for r in (4, 3, 2)]
    x9 = torch.ones(9, dtype=torch.float64, device="cuda")
    x6 = torch.ones(6, dtype=torch.float64, device="cuda")
    y = torch.full((9,), -1234.5, dtype=torch.float64, device="cuda")
    ms, lds = (4, 3, 2), (6, 6, 6)
    assert gemv_t3(ms, 6, 1.0, M, lds, x9, None, 0.0, y) == 0
    assert np.all(G.host(y)[:6] == 9.0)
    assert gemv_n3(ms, 6, M, lds, x6, y) == 0
    assert np.all(G.host(y) == 6.0)
    y.fill_(-1234.5)
    for i in range(3):
        neg = tuple(-1 if j == i else v for j, v in enumerate(ms))
        short = tuple(5 if j == i else 6 for j in range(3))
        nul = [None if j == i else v for j, v in enumerate(M)]
        for bad_t, bad_n in (((neg, 6, 1.0, M, lds, x9, None, 0.0, y), (neg, 6, M, lds, x6, y)),
                             ((ms, 6, 1.0, M, short, x9, None, 0.0, y), (ms, 6, M, short, x6, y)),
                             ((ms, 6, 1.0, nul, lds, x9, None, 0.0, y), (ms, 6, nul, lds, x6, y))):
            assert gemv_t3(*bad_t) == INVALID and gemv_n3(*bad_n) == INVALID, (i, bad_t[0], bad_t[4])
    assert gemv_t3(ms, -1, 1.0, M, lds, x9, None, 0.0, y) == INVALID and gemv_n3(ms, -1, M, lds, x6, y) == INVALID
    assert gemv_t3(ms, 6, 1.0, M, lds, None, None, 0.0, y) == INVALID and gemv_n3(ms, 6, M, lds, None, y) == INVALID
    assert gemv_t3(ms, 6, 1.0, M, lds, x9, None, 0.0, None) == INVALID and gemv_n3(ms, 6, M, lds, x6, None) == INVALID
    assert bool((y == -1234.5).all())
    # an absent operand needs neither a pointer nor a leading dimension
    for i in range(3):
        ms_i = tuple(0 if j == i else v for j, v in enumerate(ms))
        M_i = [None if j == i else v for j, v in enumerate(M)]
        ld_i = tuple(0 if j == i else 6 for j in range(3))
        y.fill_(-1234.5)
        assert gemv_t3(ms_i, 6, 1.0, M_i, ld_i, x9, None, 0.0, y) == 0
        assert np.all(G.host(y)[:6] == float(sum(ms_i)))
        assert gemv_n3(ms_i, 6, M_i, ld_i, x6, y) == 0
        assert np.all(G.host(y)[:sum(ms_i)] == 6.0)
