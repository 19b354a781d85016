"""No GPU: tests/lasso_ref.py's long-double references against the fp64 oracle and plain fp64
NumPy, at every shape of the device tests (tests/test_gpu_lasso_kernels.py).  The fp64 results
must sit inside a QUARTER of the bounds the device is held to, so a bound that a correct fp64
evaluation only just meets would show here first; and the NumPy facts the colnorm tests rely on.
"""
import numpy as np
import pytest

import lasso_ref as R
from oracle import lasso_oracle as O

ALL_SHAPES = [s for s, _ in R.SMALL + R.LARGE + R.STRIDED]


def _oracle_prox(positive, add_bias):
    o = object.__new__(O.LassoSolver)
    o.positive, o.add_bias = bool(positive), bool(add_bias)
    return o.prox


def _fp64_step(st, positive, add_bias, dual_form):
    x = st["bA"] + st["Qs"].T @ st["W"]
    alpha = _oracle_prox(positive, add_bias)(x + st["u"], st["eta"])
    u = st["u"] + (x - alpha) if dual_form else st["u"] + x - alpha
    r2 = st["rho"] * (alpha - st["alpha"])
    sums = np.array([((x - alpha) ** 2).sum(), (r2 ** 2).sum(), (alpha ** 2).sum(), (u ** 2).sum()])
    return dict(x=x, alpha=alpha, u=u, W=u - alpha, sums=sums)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_longdouble_step_vs_fp64_numpy(shape):
    """a plain fp64 NumPy step (the oracle's prox) from the random state, every flag at the small
    shapes and one combination at the large ones, within a quarter of the bounds"""
    n, S = shape
    small = n <= 65
    combos = [(p, ab, df, bc) for p in (0, 1) for ab in (0, 1) for df in (0, 1) for bc in (0, 1)] if small \
        else [(n % 2, 1, S % 2, (n + S) % 2)]
    worst = 0.0
    for positive, add_bias, dual_form, bc in combos:
        st = R.state(n, S, seed=1000 * n + S, positive=positive, ba_bcast=bc, eta_bcast=bc)
        ref = R.admm_step(**st, positive=positive, add_bias=add_bias, dual_form=dual_form, ba_bcast=bc, eta_bcast=bc)
        got = _fp64_step(st, positive, add_bias, dual_form)
        for k in ("x", "alpha", "u", "W"):
            worst = max(worst, R.ratio(got[k], ref[k], ref["b" + k]))
        worst = max(worst, R.ratio(got["sums"], ref["sums"], ref["bsums"]))
        if n * S >= 3:
            full = [t for t in R.branches(st, ref) if sum(t) >= 3]
            assert all(min(t) >= 1 for t in full), (shape, full)   # every prox branch in every tile
        if add_bias:
            assert np.array_equal(ref["alpha"][0], ref["x"][0] + st["u"][0].astype(R.LD))
    print(f"[{n}x{S}] fp64 NumPy step: worst err / bound {worst:.3g}")
    assert worst <= 0.25


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_longdouble_step_vs_oracle_iteration(shape):
    """the second iteration of the oracle's LassoSolver (a real A and b; its first iteration starts
    from zero, where x' = bA exactly) against the long-double step from the oracle's state after one
    iteration, with Qs = the oracle's scaled Qinv transposed to k-major, within a quarter of the
    bounds"""
    n, S = shape
    rng = np.random.default_rng(7 * n + S)
    m = n + 5
    A = rng.normal(size=(m, n - 1))
    b = rng.normal(size=(m, S))
    reg = rng.uniform(0.05, 0.5, S)
    positive = n % 2
    kw = dict(reg=reg, rho=0.4, check_stop=1, add_bias=True, positive=bool(positive), eps_abs=0.0, eps_rel=0.0)
    o1 = O.LassoSolver(A, b, max_iters=1, **kw)
    o2 = O.LassoSolver(A, b, max_iters=2, **kw)
    assert o1.n == n
    Qs, bA, eta = np.ascontiguousarray(o1.Qinv_cache.T), o1.bA_cache.copy(), o1.eta.copy()
    assert o1.solve()[3] == 1 and o2.solve()[3] == 2
    ref = R.admm_step(Qs, o1.u - o1.alpha, bA, eta, o1.x, o1.alpha, o1.u, 0.4, positive=positive, add_bias=1)
    worst = max(R.ratio(getattr(o2, k), ref[k], ref["b" + k]) for k in ("x", "alpha", "u"))
    print(f"[{n}x{S}] oracle iteration: worst err / bound {worst:.3g}")
    assert worst <= 0.25


def test_three_steps_bounds_grow():
    """admm_steps: the propagated bounds grow and the fp64 loop stays within a quarter of them"""
    st = R.state(65, 17, seed=3)
    refs = R.admm_steps(3, **st, dual_form=1)
    cur = dict(st)
    for it, ref in enumerate(refs):
        got = _fp64_step(cur, 0, 0, 1)
        cur = dict(cur, x=got["x"], alpha=got["alpha"], u=got["u"], W=got["W"])
        worst = max(R.ratio(got[k], ref[k], ref["b" + k]) for k in ("x", "alpha", "u", "W"))
        assert worst <= 0.25, (it, worst)
    assert np.all(refs[2]["bx"] > refs[1]["bx"]) and np.all(refs[1]["bx"] > refs[0]["bx"])


def test_prox_propagates_nan_and_edges():
    v = np.array([[np.nan, 0.5, -0.5, 0.0, -0.0, np.inf, -np.inf, 2.0]]).T
    out = R.prox(v, np.array([0.5]), 0, 0)
    assert np.isnan(out[0, 0])
    assert np.array_equal(out[1:, 0], [0.0, 0.0, 0.0, 0.0, np.inf, -np.inf, 1.5])
    assert np.array_equal(R.prox(v, np.array([0.5]), 1, 0)[1:, 0], [0.0, 0.0, 0.0, 0.0, np.inf, 0.0, 1.5])
    for positive in (0, 1):
        for add_bias in (0, 1):
            w = np.random.default_rng(1).normal(size=(5, 4))
            w[2, 1] = np.nan
            assert np.array_equal(R.prox(w, np.full(4, 0.3), positive, add_bias),
                                  _oracle_prox(positive, add_bias)(w, np.full(4, 0.3)), equal_nan=True)


def test_ratio_rules():
    assert R.ratio([1.0, np.nan], np.array([1.0, np.nan]), [0.0, 0.0]) == 0.0
    assert R.ratio([0.0], np.array([np.nan]), [1.0]) == np.inf         # a swallowed NaN
    assert R.ratio([np.nan], np.array([1.0]), [1.0]) == np.inf
    assert R.ratio([np.inf], np.array([1.0]), [1.0]) == np.inf
    assert R.ratio([1.0 + 1e-9], np.array([1.0]), [0.0]) == np.inf
    assert R.ratio([np.inf, -np.inf], np.array([np.inf, -np.inf]), [0.0, 0.0]) == 0.0
    assert R.ratio([np.inf], np.array([-np.inf]), [1.0]) == np.inf
    assert abs(R.ratio([1.5], np.array([1.0]), [1.0]) - 0.5) < 1e-15


@pytest.mark.parametrize("absm", [0, 1])
@pytest.mark.parametrize("add_bias", [0, 1])
def test_loss_vs_oracle(absm, add_bias):
    rng = np.random.default_rng(5)
    m, n, S = 257, 33, 7
    A, alpha, b = rng.normal(size=(m, n)), rng.uniform(-2, 2, (n, S)), rng.normal(size=(m, S))
    reg = rng.uniform(0.1, 1, S)
    o = object.__new__(O.LassoSolver)
    o.A, o.m, o.positive, o.add_bias = A, m, not absm, bool(add_bias)
    val, bound = R.loss(A, alpha, b, reg, absm, add_bias)
    assert R.ratio(o._loss(alpha, b, reg), val, bound) <= 0.25
    cols = rng.permutation(S)
    prior = np.full(S + 2, -3.0)
    v2, b2 = R.loss(A, alpha, b[:, :1], reg[:1], absm, add_bias, b_bcast=1, reg_bcast=1, cols=cols, out=prior)
    assert np.array_equal(v2[S:], [-3.0, -3.0]) and np.array_equal(b2[S:], [0.0, 0.0])
    assert R.ratio(o._loss(alpha, b[:, :1], reg[:1]), v2[cols], b2[cols]) <= 0.25


@pytest.mark.parametrize("n", [1, 31, 32, 33, 70])
def test_block_qs_layout(n):
    Qs = np.random.default_rng(n).normal(size=(n, n))
    Qb = R.block_qs(Qs)
    assert Qb.size == -(-n // 32) * 32 * n
    for i in range(-(-n // 32) * 32):
        for k in (0, n // 2, n - 1):
            assert Qb[((i // 32) * n + k) * 32 + i % 32] == (Qs[k, i] if i < n else 0.0)


def test_ks_formula():
    for n, S, ks in [(400, 30, 3), (33, 31, 1), (1281, 3, 10), (2049, 1, 16)]:
        tiles = -(-S // 32) * -(-n // 32)
        total = 4 * tiles + 8 + (tiles * (1024 * ks + 1) if ks > 1 else 0)
        assert R.ks_from_partial_doubles(n, S, total) == ks
    assert R.kchunk(1281, 10) == (144, -15)       # an empty last chunk
    assert R.kchunk(1153, 9) == (144, 1)
    assert R.kchunk(1030, 8) == (144, 22)
    assert R.kchunk(257, 2) == (144, 113)
    assert R.kchunk(2049, 16) == (144, -111)


@pytest.mark.parametrize("shape", [(500, 150), (9, 2), (1000, 2), (300, 257), (1, 5)])
def test_colstd_inorder_is_numpy_for_two_or_more_columns(shape):
    A = np.random.default_rng(sum(shape)).normal(size=shape)
    An, sd = R.colstd_inorder(A)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(sd, A.std(axis=0))
        assert np.array_equal(An, A / A.std(axis=0), equal_nan=True)


def test_colstd_single_column_is_a_reordered_sum():
    """n = 1: NumPy sums the contiguous column pairwise, the kernel in order -- equal only to the
    bound of a reordered sum of m non-negative terms, 2 m eps relative (and not always bit-equal)"""
    m = 1000
    differs = 0
    for seed in range(8):
        A = np.random.default_rng(seed).normal(size=(m, 1))
        _, sd = R.colstd_inorder(A)
        rel = abs(sd[0] - A.std(axis=0)[0]) / A.std(axis=0)[0]
        print(f"in-order vs np.std at m = {m}, n = 1, seed {seed}: {rel:.3g} relative")
        assert rel <= 2 * m * R.EPS
        differs += rel > 0
    assert differs > 0
