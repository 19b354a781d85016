"""-m gpu: ipm_gemv_2v, two vectors over one matrix (Y[:, 0:2] = op(M) [x0 | x1], M read once), both
transposes.  The dual-form phase-1 Newton step uses it for C (E o [-g_x | h]) and C^T [z_u | z_y].

Shapes: rows in {1, 3, 4, 5, 63, 64, 65, 257} x cols in {1, 2, 63, 64, 65, 255, 256, 257, 1030} and, for
the loops of the vector kernel those do not reach, 640 and 1542, with ldm in {cols, cols + 1, cols + 7},
16-byte-aligned and 8-byte-offset M and X, ldx = the vector length + 3 and + 4, and ldy != the output
length.  Which kernel a call runs is decided by alignment alone (M, ldm and BOTH vectors 16-byte
aligned: k_gemv_n_2v<true>; both vectors equally misaligned, or M / ldm odd: <false>; vectors that differ:
two single-vector launches), and x1 = X + ldx, so the two ldx together give every cols a call on each
path; test_every_path_runs_at_every_width asserts that from the pointers the calls were given.  Inside
k_gemv_n_2v<true> one lane walks 16-byte pairs j = lane, lane + 64, ...: the eight-load loop runs while
j + 448 < cols / 2 (1030, 1542), the four-load loop while j + 192 < cols / 2 (640, and after the eight-load
loop at 1542), the single-load tail everywhere else (and after both at 1030 and 1542), the odd last
column at 63, 65, 255, 257.  The transposed pair covers the 256-column blocks and the row chunks of its
plan; four rows per workgroup for the plain one.

Per call: each output column equals ipm_gemv on that vector BIT FOR BIT; every entry is within
2 K eps sum|M||x| of a long-double product (K = the summed length); the sentinels around Y are intact;
a repeat gives the same bits; a NaN in one vector reaches that column only.
"""
import numpy as np
import pytest

import gpu_util as G

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
ROWS = [1, 3, 4, 5, 63, 64, 65, 257]
COLS = [1, 2, 63, 64, 65, 255, 256, 257, 1030, 640, 1542]
PADS = [3, 4]        # ldx = the vector length + pad: odd and even, whatever the length
PATHS = {}           # (trans, cols) -> the kernel paths the calls of this session took
SENT = -1234.5


def gemv_2v(trans, rows, cols, M, ldm, X, ldx, Y, ldy):
    from ipm355 import _lib as L
    h = G.handle()
    return h.lib.ipm_gemv_2v(h.ptr, int(trans), rows, cols, L.dptr(M), ldm, L.dptr(X), ldx, L.dptr(Y), ldy)


def _offset(a, off):
    """a device copy of the flat array whose first element sits `off` doubles past a 16-byte boundary"""
    import torch
    buf = torch.zeros(a.size + off + 2, dtype=torch.float64, device="cuda")
    v = buf[off:off + a.size]
    v.copy_(G.dev(a.ravel()))
    assert (v.data_ptr() % 16) == 8 * (off % 2)
    return v


def _path(M, ldm, X, ldx):
    """the launch gemv_n_2v chooses for these pointers (its rule, restated: see the module docstring)"""
    vec = [ldm % 2 == 0 and M.data_ptr() % 16 == 0 and (X.data_ptr() + 8 * j * ldx) % 16 == 0 for j in range(2)]
    return "two launches" if vec[0] != vec[1] else ("vector" if vec[0] else "scalar")


def _case(trans, rows, cols, ldm, off, rng, nan_col=None, pad=3):
    import torch
    kin, kout = (rows, cols) if trans else (cols, rows)      # vector lengths in / out
    Mh = np.zeros((rows, ldm))
    Mh[:, :cols] = rng.uniform(-2, 2, size=(rows, cols))
    Mh[:, cols:] = np.nan                                     # the padding of M is never read
    ldx, ldy = kin + pad, kout + 5
    Xh = np.full(2 * ldx, np.nan)
    xs = [rng.uniform(-2, 2, size=kin) for _ in range(2)]
    if nan_col is not None:
        xs[nan_col][kin // 2] = np.nan
    for j in range(2):
        Xh[j * ldx:j * ldx + kin] = xs[j]
    Md, Xd = _offset(Mh, off), _offset(Xh, off)
    PATHS.setdefault((trans, cols), set()).add(_path(Md, ldm, Xd, ldx))
    guard = 4
    Y = torch.full((2 * ldy + 2 * guard,), SENT, dtype=torch.float64, device="cuda")
    Yv = Y[guard:]
    assert gemv_2v(trans, rows, cols, Md, ldm, Xd, ldx, Yv, ldy) == 0
    got = G.host(Y)
    cols_out = [got[guard + j * ldy: guard + j * ldy + kout].copy() for j in range(2)]
    # sentinels: before, between and after the two columns
    mask = np.ones(got.size, bool)
    for j in range(2):
        mask[guard + j * ldy: guard + j * ldy + kout] = False
    assert np.all(got[mask] == SENT), "ipm_gemv_2v wrote outside its two output columns"
    # each column bit for bit what the single-vector call gives for that vector alone
    for j in range(2):
        y1 = torch.full((kout + 2,), SENT, dtype=torch.float64, device="cuda")
        assert G.gemv(trans, rows, cols, 1.0, Md, ldm, Xd[j * ldx:], 0.0, y1) == 0
        ref = G.host(y1)[:kout]
        assert cols_out[j].tobytes() == ref.tobytes(), (trans, rows, cols, ldm, off, pad, j)
    # a repeat call gives the same bits
    Y2 = torch.full_like(Y, SENT)
    assert gemv_2v(trans, rows, cols, Md, ldm, Xd, ldx, Y2[guard:], ldy) == 0
    assert G.host(Y2).tobytes() == got.tobytes()
    return Mh[:, :cols], xs, cols_out


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("trans", [0, 1], ids=["n", "t"])
def test_columns_equal_the_single_vector_call(trans, rows):
    rng = np.random.default_rng(100 * rows + trans)
    worst = 0.0
    for cols in COLS:
        for ldm in (cols, cols + 1, cols + 7):
            for off, pad in ((0, 3), (0, 4), (1, 3), (1, 4)):
                M, xs, out = _case(trans, rows, cols, ldm, off, rng, pad=pad)
                A = (M.T if trans else M).astype(np.longdouble)
                K = A.shape[1]
                for j in range(2):
                    ref = A @ xs[j].astype(np.longdouble)
                    bound = 2 * K * EPS * (np.abs(A) @ np.abs(xs[j]).astype(np.longdouble))
                    err = np.abs(out[j].astype(np.longdouble) - ref)
                    assert np.all(err <= bound), (trans, rows, cols, ldm, off, pad, j)
                    worst = max(worst, float((err / bound).max()))
    print(f"[{'t' if trans else 'n'} rows {rows}] worst |y - y_ld| / (2 K eps sum|M||x|) {worst:.3g}")


def test_every_path_runs_at_every_width():
    """the bit-for-bit comparison above is not vacuous: for M x (the kernel with an alignment rule) every
    cols had calls on the vector kernel, on the scalar kernel and on the two-launch fallback"""
    rng = np.random.default_rng(5)
    for cols in COLS:
        for ldm in (cols, cols + 1):
            for off, pad in ((0, 3), (0, 4), (1, 3), (1, 4)):
                _case(0, 5, cols, ldm, off, rng, pad=pad)
        assert PATHS[(0, cols)] == {"vector", "scalar", "two launches"}, (cols, PATHS[(0, cols)])


@pytest.mark.parametrize("trans", [0, 1], ids=["n", "t"])
def test_nan_in_one_vector_reaches_that_column_only(trans):
    for rows, cols in ((5, 65), (65, 257), (257, 1030)):
        for nan_col in (0, 1):
            rng = np.random.default_rng(7)
            pad = 3 if (rows if trans else cols) % 2 else 4          # both vectors aligned: the vector kernel
            _, _, clean = _case(trans, rows, cols, cols + 1, 0, rng, pad=pad)
            rng = np.random.default_rng(7)
            _, _, out = _case(trans, rows, cols, cols + 1, 0, rng, nan_col=nan_col, pad=pad)
            assert np.all(np.isnan(out[nan_col]))
            assert out[1 - nan_col].tobytes() == clean[1 - nan_col].tobytes()


@pytest.mark.parametrize("trans", [0, 1], ids=["n", "t"])
def test_empty_shapes_return_cleanly(trans):
    """rows = 0 or cols = 0: IPM_OK, the outputs are what ipm_gemv leaves (zeros of an empty sum, or
    nothing at all), nothing else is touched"""
    import torch
    for rows, cols in ((0, 5), (5, 0), (0, 0)):
        kin, kout = (rows, cols) if trans else (cols, rows)
        ldm, ldx, ldy = max(cols, 1), kin + 3, kout + 5
        M = torch.ones(max(rows * ldm, 1), dtype=torch.float64, device="cuda")
        X = torch.ones(2 * ldx, dtype=torch.float64, device="cuda")
        Y = torch.full((2 * ldy + 8,), SENT, dtype=torch.float64, device="cuda")
        assert gemv_2v(trans, rows, cols, M, ldm, X, ldx, Y[4:], ldy) == 0
        got = G.host(Y)
        y1 = torch.full((kout + 2,), SENT, dtype=torch.float64, device="cuda")
        assert G.gemv(trans, rows, cols, 1.0, M, ldm, X, 0.0, y1) == 0
        ref = G.host(y1)
        want = np.full(got.size, SENT)
        for j in range(2):
            want[4 + j * ldy: 4 + j * ldy + kout] = ref[:kout]
        assert got.tobytes() == want.tobytes(), (trans, rows, cols)
    # IPM_INVALID_ARG: negative size, ldm < cols, ldx / ldy below the vector length, a null operand
    kin, kout = (4, 6) if trans else (6, 4)
    M = torch.ones(24, dtype=torch.float64, device="cuda")
    X = torch.ones(16, dtype=torch.float64, device="cuda")
    Y = torch.full((16,), SENT, dtype=torch.float64, device="cuda")
    assert gemv_2v(trans, 4, 6, M, 6, X, kin, Y, kout) == 0
    for bad in ((-1, 6, M, 6, X, kin, Y, kout), (4, 6, M, 5, X, kin, Y, kout), (4, 6, M, 6, X, kin - 1, Y, kout),
                (4, 6, M, 6, X, kin, Y, kout - 1), (4, 6, None, 6, X, kin, Y, kout), (4, 6, M, 6, None, kin, Y, kout),
                (4, 6, M, 6, X, kin, None, kout)):
        Y.fill_(SENT)
        assert gemv_2v(trans, *bad) == 2, bad
        assert bool((Y == SENT).all())
