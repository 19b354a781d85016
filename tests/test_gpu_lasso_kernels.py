"""-m gpu: every ipm_lasso_* entry point (ipm_lasso.hip) on its own, at tile and chunk edges,
entry by entry against the long-double references and derived bounds of tests/lasso_ref.py.

tests/test_lasso.py runs the solver end to end on six fixtures ((n, S) = (151, 30), (401, 50),
(401, 30), (1025, 30); lds == S, ldq == n, the blocked Qs; K splits 1, 3 and 8) and accepts X at
1e-6 after hundreds of contracting iterations.  Here one fused step is compared from a random
non-zero state, where a wrong element of a ragged tile, a dropped K row at a chunk boundary or a
misplaced partial sum shows in the entry it hits.  Common rules: operands with a leading dimension
above their width carry NaN in the padding, outputs a sentinel that must come back untouched, a
non-finite output where the reference is finite is an infinite error (lasso_ref.ratio), and every
test prints its worst err / bound.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_util as G
import lasso_ref as R

pytestmark = pytest.mark.gpu
SENT = R.DeviceStep.SENT


def _lib():
    from ipm355 import _lib as L
    return L, G.handle()


def _padded(a, ld, fill):
    import torch
    a = np.asarray(a, dtype=np.float64)
    buf = torch.full((a.shape[0], ld), fill, dtype=torch.float64, device="cuda")
    if a.shape[1]:
        buf[:, :a.shape[1]] = G.dev(a)
    return buf


def _one_step(st, ref, flags, qs_blocked, lds_pad, tag, repeats=2):
    """one ipm_lasso_admm step against `ref`; then `repeats` more on fresh copies of the state with
    the same partial buffer, which must be bitwise equal.  Returns the worst err / bound."""
    import torch
    n, S = st["u"].shape
    kw = dict(flags, lds=S + lds_pad, qs_blocked=qs_blocked, ldq=n if qs_blocked else n + 3)
    dv = R.DeviceStep(st, **kw)
    rc, it = dv.run()
    assert (rc, it) == (0, 0), (tag, rc, it)
    ratios = R.step_ratios(dv, ref)
    worst = max(ratios.values())
    assert worst <= 1.0, (tag, ratios)
    for k in ("x", "alpha", "u", "W1"):
        assert np.all(dv.out(k)[1] == SENT), (tag, k, "padding written")
    if flags.get("add_bias"):       # row 0 is unpenalised: alpha' = x' + u, exactly
        assert np.array_equal(dv.out("alpha")[0][0], dv.out("x")[0][0] + st["u"][0], equal_nan=True), tag
    for r in range(repeats):
        d2 = R.DeviceStep(st, partial=dv.t["partial"], **kw)
        before = dv.norms().copy()
        assert d2.run() == (0, 0)
        for k in ("x", "alpha", "u", "W1"):
            assert torch.equal(d2.t[k].view(torch.int64), dv.t[k].view(torch.int64)), (tag, k, "run", r + 2)
        assert np.array_equal(d2.norms().view(np.int64), before.view(np.int64)), (tag, "norms", r + 2)
    return worst


def _flag_sets():
    return [dict(positive=p, add_bias=ab, dual_form=df, ba_bcast=bc, eta_bcast=bc)
            for p in (0, 1) for ab in (0, 1) for df in (0, 1) for bc in (0, 1)]


# ------------------------------------------------------------------ a. one fused step
@pytest.mark.parametrize("qs_blocked", [0, 1], ids=["plain-ldq+3", "blocked"])
@pytest.mark.parametrize("shape,ks", R.SMALL, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"ks{v}")
def test_step_small_shapes(shape, ks, qs_blocked):
    """(1, 1): one entry; (15, 17), (31, 33), (33, 31): ragged tiles in both directions, one and two
    tiles; (32, 32): exactly one tile; (65, 64): a third row tile of one row, two exact column tiles.
    n < 32 and S on either side of 16 / 32 / 64; ks = 1.  Crossed with lds in {S, S + 5}, positive,
    add_bias, dual_form and broadcast against per-problem bA / eta."""
    n, S = shape
    assert R.admm_ks(n, S) == ks
    worst = 0.0
    for flags in _flag_sets():
        bc = flags["ba_bcast"]
        st = R.state(n, S, seed=1000 * n + S, ba_bcast=bc, eta_bcast=bc)
        ref = R.admm_step(**st, **flags)
        if n * S >= 3:
            assert all(min(t) >= 1 for t in R.branches(st, ref) if sum(t) >= 3)
        for lds_pad in (0, 5):
            worst = max(worst, _one_step(st, ref, flags, qs_blocked, lds_pad, (shape, flags, lds_pad)))
    print(f"[step {n}x{S} ks {ks} qs_blocked {qs_blocked}] worst err / bound {worst:.3g}")


@functools.lru_cache(maxsize=None)
def _k_split_case(shape):
    """(flags, state, long-double step) of one K-split shape, shared by its two Qs layouts"""
    n, S = shape
    flags = dict(positive=n % 2, add_bias=1 - n % 2, dual_form=S % 2, ba_bcast=(n + S) % 2, eta_bcast=(n + S) % 2)
    st = R.state(n, S, seed=1000 * n + S, ba_bcast=flags["ba_bcast"], eta_bcast=flags["eta_bcast"])
    ref = R.admm_step(**st, **flags)
    assert all(min(t) >= 1 for t in R.branches(st, ref) if sum(t) >= 3)
    return flags, st, ref


@pytest.mark.parametrize("qs_blocked", [0, 1], ids=["plain-ldq+3", "blocked"])
@pytest.mark.parametrize("shape,ks", R.LARGE + R.STRIDED,
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"ks{v}")
def test_step_k_split_shapes(shape, ks, qs_blocked):
    """The K split (chunks of 144 rows): (257, 33) ks 2, last chunk 113 rows and a 1 x 1 corner tile;
    (400, 30) ks 3; (1030, 17) ks 8, last chunk 22 rows; (1153, 5) ks 9, last chunk ONE row;
    (1281, 3) ks 10, 9 x 144 > n: the last workgroup of every tile has an empty K range and must
    still hand over a zero tile; (288, 900), 261 tiles, ks 2 and (224, 1200), 266 tiles, ks 1: the
    strided loop of k_admm_norms, with and without the K split.
    One flag combination per shape (it differs between shapes), lds = S + 5."""
    n, S = shape
    assert R.admm_ks(n, S) == ks
    kc, last = R.kchunk(n, ks)
    flags, st, ref = _k_split_case(shape)
    worst = _one_step(st, ref, flags, qs_blocked, 5, (shape, flags))
    print(f"[step {n}x{S} ks {ks} chunk {kc} last {last} qs_blocked {qs_blocked}] worst err / bound {worst:.3g}")


# ------------------------------------------------------------------ b. knobs read once per process
_KNOB_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import lasso_ref as R
worst = 0.0
for spec in sys.argv[3:]:
    n, S, ks = (int(v) for v in spec.split(","))
    assert R.admm_ks(n, S) == ks, (n, S, R.admm_ks(n, S))
    flags = dict(positive=0, add_bias=1, dual_form=n % 2, ba_bcast=0, eta_bcast=0)
    st = R.state(n, S, seed=1000 * n + S)
    ref = R.admm_step(**st, **flags)
    for qb in (0, 1):
        dv = R.DeviceStep(st, lds=S + 5, qs_blocked=qb, ldq=n if qb else n + 3, **flags)
        assert dv.run() == (0, 0)
        worst = max(worst, max(R.step_ratios(dv, ref).values()))
        assert all((dv.out(k)[1] == R.DeviceStep.SENT).all() for k in ("x", "alpha", "u", "W1"))
print("worst", worst)
"""


@pytest.mark.parametrize("env,specs", [({"IPM_ADMM_U": "8"}, ["1030,17,8", "33,31,1"]),
                                       ({"IPM_ADMM_U": "16"}, ["1030,17,8", "33,31,1"]),
                                       ({"IPM_ADMM_WG": "4096"}, ["2049,1,16"])],
                         ids=["U8", "U16", "WG4096"])
def test_step_knobs(env, specs):
    """IPM_ADMM_U = 8 / 16 (8 or 16 four-row slabs per wave and pass: a 144-row chunk and the
    33-row K range end inside a pass) and IPM_ADMM_WG = 4096 at (2049, 1): ks = 16, chunk 144, the
    15th chunk has 33 rows and the 16th is empty.  One child process per setting."""
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.join(here, "..", "interiorpoint-gpu_amd")
    out = subprocess.run([sys.executable, "-c", _KNOB_CHILD, here, pkg] + specs, env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    worst = float(out.stdout.split("worst")[-1])
    print(f"[knob {env}] worst err / bound {worst:.3g}")
    assert worst <= 1.0, worst


# ------------------------------------------------------------------ c. the loop's control flow
def _zero_state(n, S):
    z = np.zeros((n, S))
    return dict(Qs=np.zeros((n, n)), W=z, bA=z.copy(), eta=np.full(S, 0.5), x=z.copy(), alpha=z.copy(), u=z.copy(),
                rho=0.4)


@pytest.mark.parametrize("max_iters,check_stop", [(10, 3), (10, 1), (4, 4)])
def test_loop_stops_at_first_check(max_iters, check_stop):
    """Qs = 0, bA = 0 from the zero state: all four norms are exactly 0 < stop_multiplier"""
    dv = R.DeviceStep(_zero_state(33, 31), max_iters=max_iters, check_stop=check_stop, stop_multiplier=1e-3)
    assert dv.run() == (0, check_stop - 1)
    assert np.array_equal(dv.norms(), np.zeros(4))


@pytest.mark.parametrize("max_iters,check_stop", [(7, 3), (6, 2), (2, 5), (1, 1)])
def test_loop_never_stops_with_zero_tolerances(max_iters, check_stop):
    """stop_multiplier = 0, eps_rel = 0: 0 < 0 is false even with all norms zero -> the last index;
    max_iters no multiple of check_stop, and check_stop > max_iters (no check at all)"""
    dv = R.DeviceStep(_zero_state(33, 31), max_iters=max_iters, check_stop=check_stop)
    assert dv.run() == (0, max_iters - 1)
    st = R.state(33, 31, seed=9)
    dv = R.DeviceStep(st, max_iters=max_iters, check_stop=check_stop)
    assert dv.run() == (0, max_iters - 1)


def _loss_fields(dv, A, b, reg, b_bcast, reg_bcast, ldat_pad=1, ldb_pad=3):
    """AT, b, reg and R of a DeviceStep's args (the loss evaluation)"""
    import torch
    L, _ = _lib()
    m, n = A.shape
    a, t = dv.args, dv.t
    t["AT"] = _padded(A.T, m + ldat_pad, float("nan"))
    t["b"] = _padded(b, 1 if b_bcast else b.shape[1] + ldb_pad, float("nan"))
    t["reg"] = G.dev(reg)
    t["R"] = G.devnan((max(1, m * dv.S),))
    a.m, a.AT, a.ldat, a.b, a.ldb, a.b_bcast = m, L.dptr(t["AT"]), m + ldat_pad, L.dptr(t["b"]), t["b"].shape[1], \
        int(b_bcast)
    a.reg, a.reg_bcast, a.R = L.dptr(t["reg"]), int(reg_bcast), L.dptr(t["R"])
    return torch


def test_loop_compute_loss_rows_and_columns():
    """compute_loss with a permuted gap_cols and ldg > S: row `it` of gaps holds the loss of
    iteration it's alpha in the permuted columns (alpha of iteration it: the same deterministic
    loop stopped after it + 1 iterations), every other entry untouched"""
    import torch
    L, _ = _lib()
    n, S, m, iters = 33, 31, 40, 3
    st = R.state(n, S, seed=11)
    rng = np.random.default_rng(12)
    A, b, reg = rng.normal(size=(m, n)), rng.normal(size=(m, S)), rng.uniform(0.1, 1, S)
    ldg = S + 4
    cols = rng.permutation(ldg)[:S]
    alphas = []
    for k in range(1, iters + 1):
        d = R.DeviceStep(st, lds=S + 5, max_iters=k, check_stop=2, add_bias=1)
        assert d.run() == (0, k - 1)
        alphas.append(d.out("alpha")[0].copy())
    dv = R.DeviceStep(st, lds=S + 5, max_iters=iters, check_stop=2, add_bias=1)
    _loss_fields(dv, A, b, reg, 0, 0)
    gaps = torch.full((iters + 1, ldg), SENT, dtype=torch.float64, device="cuda")
    cd = torch.as_tensor(cols.astype(np.int64), device="cuda")
    dv.args.compute_loss, dv.args.gaps, dv.args.ldg, dv.args.gap_cols = 1, L.dptr(gaps), ldg, L.dptr(cd)
    assert dv.run() == (0, iters - 1)
    assert np.array_equal(dv.out("alpha")[0], alphas[-1])
    got = G.host(gaps)
    worst = 0.0
    for it in range(iters):
        val, bound = R.loss(A, alphas[it], b, reg, absm=1, add_bias=1, cols=cols, out=np.full(ldg, SENT))
        worst = max(worst, R.ratio(got[it], val, bound))
    assert np.all(got[iters] == SENT)
    print(f"[loop compute_loss] worst err / bound {worst:.3g}")
    assert worst <= 1.0


def test_three_iterations_propagated_bounds():
    """three iterations at (400, 30) (ks 3) against three long-double steps, each iteration within
    its one-step bound plus the propagated bound of its inputs (lasso_ref.admm_steps)"""
    n, S = 400, 30
    assert R.admm_ks(n, S) == 3
    st = R.state(n, S, seed=21)
    flags = dict(positive=0, add_bias=1, dual_form=1, ba_bcast=0, eta_bcast=0)
    refs = R.admm_steps(3, **st, **flags)
    worst = []
    for k in range(1, 4):
        dv = R.DeviceStep(st, lds=S + 5, max_iters=k, check_stop=1, **flags)
        assert dv.run() == (0, k - 1)
        ratios = R.step_ratios(dv, refs[k - 1], wkey="W1" if k % 2 else "W0")
        worst.append(max(ratios.values()))
        assert worst[-1] <= 1.0, (k, ratios)
    print("[three iterations 400x30] worst err / bound per iteration " + ", ".join(f"{w:.3g}" for w in worst))


# ------------------------------------------------------------------ d. ipm_lasso_loss
def _run_loss(A, alpha, b, reg, absm, add_bias, b_bcast, reg_bcast, cols, nout):
    import torch
    from ipm355.lasso import LassoArgs
    L, h = _lib()
    m, n = A.shape
    S = alpha.shape[1]
    a = LassoArgs()
    t = dict(alpha=_padded(alpha, S + 2, float("nan")), AT=_padded(A.T, m + 1, float("nan")),
             b=_padded(b, 1 if b_bcast else S + 3, float("nan")), reg=G.dev(reg), R=G.devnan((max(1, m * S),)),
             out=torch.full((nout,), SENT, dtype=torch.float64, device="cuda"),
             cols=None if cols is None else torch.as_tensor(np.asarray(cols, dtype=np.int64), device="cuda"))
    a.n, a.S, a.m, a.lds, a.alpha = n, S, m, S + 2, L.dptr(t["alpha"])
    a.AT, a.ldat, a.b, a.ldb, a.b_bcast = L.dptr(t["AT"]), m + 1, L.dptr(t["b"]), t["b"].shape[1], int(b_bcast)
    a.reg, a.reg_bcast, a.R, a.add_bias = L.dptr(t["reg"]), int(reg_bcast), L.dptr(t["R"]), int(add_bias)
    rc = h.lib.ipm_lasso_loss(h.ptr, ctypes.byref(a), int(absm), L.dptr(t["out"]), L.dptr(t["cols"]))
    return rc, G.host(t["out"])


@pytest.mark.parametrize("m", [1, 255, 256, 257, 600])
def test_loss_entry_point(m):
    """k_lasso_loss strides 256 threads over the m rows and the n entries of alpha: m and n on both
    sides of 256, one row, one or two variables (add_bias with n = 1: an empty l1 term), S = 1 and
    33 (two column tiles of the GEMM), |alpha| or alpha, b and reg broadcast, cols null or a
    permutation into a longer output whose other entries stay"""
    worst = 0.0
    for n in (1, 2, 257):
        for S in (1, 33):
            rng = np.random.default_rng(m * 1000 + n * 10 + S)
            A, alpha = rng.normal(size=(m, n)), rng.uniform(-2, 2, (n, S))
            bfull, regfull = rng.normal(size=(m, S)), rng.uniform(0.1, 1, S)
            assert (alpha < 0).any() or n * S < 3
            for absm in (0, 1):
                for add_bias in (0, 1):
                    for bc, perm in ((0, 0), (1, 1)) if n == 257 else ((0, 0), (0, 1), (1, 0), (1, 1)):
                        if True:
                            b, reg = (bfull[:, :1], regfull[:1]) if bc else (bfull, regfull)
                            nout = S + 2 if perm else S
                            cols = rng.permutation(nout)[:S] if perm else None
                            rc, got = _run_loss(A, alpha, b, reg, absm, add_bias, bc, bc, cols, nout)
                            assert rc == 0
                            val, bound = R.loss(A, alpha, b, reg, absm, add_bias, bc, bc, cols, np.full(nout, SENT))
                            r = R.ratio(got, val, bound)
                            assert r <= 1.0, (m, n, S, absm, add_bias, bc, perm, r)
                            worst = max(worst, r)
                            if add_bias and n == 1:     # quadratic term alone
                                v0, b0 = R.loss(A, alpha, b, 0 * reg, absm, 0, bc, bc, cols, np.full(nout, SENT))
                                assert R.ratio(got, v0, b0) <= 1.0
    print(f"[loss m {m}] worst err / bound {worst:.3g}")


def test_loss_empty_batch():
    """S = 0: no problems, IPM_OK and nothing written (as ipm_gemm_tn treats M == 0 or N == 0)"""
    rc, got = _run_loss(np.ones((5, 3)), np.zeros((3, 0)), np.zeros((5, 1)), np.ones(1), 1, 0, 1, 1, None, 2)
    assert rc == 0 and np.all(got == SENT)


# ------------------------------------------------------------------ e. ipm_lasso_prox
def _run_prox(v, eta, eta_bcast, positive, add_bias, ldv_pad=3, ldo_pad=2):
    import torch
    L, h = _lib()
    n, S = v.shape
    vd = _padded(v, S + ldv_pad, float("nan"))
    out = torch.full((n, S + ldo_pad), SENT, dtype=torch.float64, device="cuda")
    rc = h.lib.ipm_lasso_prox(h.ptr, n, S, L.dptr(vd), S + ldv_pad, L.dptr(G.dev(eta)), int(eta_bcast), int(positive),
                              int(add_bias), L.dptr(out), S + ldo_pad)
    o = G.host(out)
    return rc, o[:, :S], o[:, S:]


@pytest.mark.parametrize("shape", [(1, 1), (15, 17), (16, 16), (257, 1), (33, 31)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_prox_bit_equal_and_nan(shape):
    """n S = 1, 255, 256, 257 (the 256-thread blocks' edge) and (33, 31); ldv, ldo > S.  Values
    exactly at +-eta, +-0.0, +-inf, and NaN -- which must come back NaN, as np.maximum has it (C's
    fmax(NaN, 0) is 0: the solver then returned a finite alpha of zeros for a NaN in b)"""
    n, S = shape
    rng = np.random.default_rng(n * 100 + S)
    for eta_bcast in (0, 1):
        eta = rng.uniform(0.2, 1.0, 1 if eta_bcast else S)
        et = np.broadcast_to(eta[None, :], (n, S))
        v = rng.uniform(-2, 2, (n, S))
        special = [lambda e: e, lambda e: -e, lambda e: 0.0, lambda e: -0.0, lambda e: np.inf, lambda e: -np.inf,
                   lambda e: np.nan, lambda e: np.nextafter(e, 2), lambda e: np.nextafter(-e, -2)]
        flat = v.reshape(-1)
        for j in range(flat.size):
            if n * S == 1 or j % 3 == 0:
                flat[j] = special[(j // 3) % len(special)](et.reshape(-1)[j])
        variants = [v] if n * S > 1 else [np.full((1, 1), f(eta[0])) for f in special]
        for vv in variants:
            for positive in (0, 1):
                for add_bias in (0, 1):
                    rc, got, pad = _run_prox(vv, eta, eta_bcast, positive, add_bias)
                    assert rc == 0 and np.all(pad == SENT)
                    with np.errstate(invalid="ignore"):
                        ref = np.maximum(vv - et, 0)
                        if not positive:
                            ref = ref - np.maximum(-vv - et, 0)
                    if add_bias:
                        ref[0] = vv[0]
                    assert np.array_equal(got, ref, equal_nan=True), (shape, eta_bcast, positive, add_bias)
                    assert np.array_equal(np.isnan(got), np.isnan(vv))


def test_step_propagates_nan():
    """test a at (33, 31) with one NaN in bA: x', alpha', u' and W' are NaN exactly where the
    reference's are (alpha' was 0 there with fmax), the rest within bounds, and the stopping test --
    NaN < tol is false -- does not stop even with a huge tolerance"""
    n, S = 33, 31
    st = R.state(n, S, seed=5)
    st["bA"][5, 7] = np.nan
    for flags in (dict(positive=0, add_bias=0), dict(positive=1, add_bias=1, dual_form=1)):
        for qb in (0, 1):
            ref = R.admm_step(**st, **flags)
            assert np.isnan(np.asarray(ref["alpha"], dtype=np.float64)).sum() == 1
            worst = _one_step(st, ref, flags, qb, 5, ("nan", flags, qb), repeats=0)
            dv = R.DeviceStep(st, max_iters=1, qs_blocked=qb, ldq=n if qb else n + 3, **flags)
            assert dv.run() == (0, 0)
            assert np.array_equal(np.isnan(dv.out("alpha")[0]), np.isnan(np.asarray(ref["alpha"], dtype=np.float64)))
    dv = R.DeviceStep(st, max_iters=5, check_stop=1, stop_multiplier=1e300)
    assert dv.run() == (0, 4)
    assert np.isnan(dv.out("alpha")[0]).any()
    print(f"[step NaN 33x31] worst err / bound {worst:.3g}")


# ------------------------------------------------------------------ f. colnorm, bias, scale, block_qs
def _run_colnorm(A, with_std, pad=3):
    import torch
    L, h = _lib()
    m, n = A.shape
    Ad = _padded(A, n + pad, SENT)
    sd = torch.full((n + 1,), SENT, dtype=torch.float64, device="cuda") if with_std else None
    rc = h.lib.ipm_lasso_colnorm(h.ptr, m, n, L.dptr(Ad), n + pad, L.dptr(sd))
    a = G.host(Ad)
    return rc, a[:, :n], a[:, n:], (G.host(sd) if with_std else None)


@pytest.mark.parametrize("n", [2, 255, 256, 257])
@pytest.mark.parametrize("m", [1, 2, 500])
def test_colnorm_bit_equal_to_numpy(m, n):
    """two or more columns: A / A.std(0) and the std itself, bit for bit (NumPy reduces axis 0 of a
    C-contiguous array row by row, as the kernel's one thread per column does); one constant column
    (and every column when m = 1): sd = 0 and NumPy's inf / NaN pattern.  lda > n, stdv given or null."""
    A = np.random.default_rng(m * 1000 + n).normal(size=(m, n))
    A[:, 1] = 2.0
    A[0, 0] = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        sd_ref = A.std(axis=0)
        ref = A / sd_ref
    assert sd_ref[1] == 0.0
    for with_std in (1, 0):
        rc, got, pad, sd = _run_colnorm(A, with_std)
        assert rc == 0 and np.all(pad == SENT)
        assert np.array_equal(got, ref, equal_nan=True)
        if with_std:
            assert np.array_equal(sd[:n], sd_ref) and sd[n] == SENT


def test_colnorm_single_column():
    """n = 1 at m = 1000: bit for bit the in-order emulation; against np.std, which sums a single
    contiguous column pairwise, within 2 m eps relative (a reordered sum of m non-negative terms)"""
    m = 1000
    A = np.random.default_rng(0).normal(size=(m, 1))
    rc, got, pad, sd = _run_colnorm(A, 1)
    An, sde = R.colstd_inorder(A)
    assert rc == 0 and np.all(pad == SENT) and sd[1] == SENT
    assert sd[0] == sde[0] and np.array_equal(got, An)
    rel = abs(sd[0] - A.std(axis=0)[0]) / A.std(axis=0)[0]
    print(f"[colnorm n = 1, m = {m}] device vs np.std {rel:.3g} relative (bound {2 * m * R.EPS:.3g})")
    assert rel <= 2 * m * R.EPS


@pytest.mark.parametrize("m,n", [(15, 16), (16, 15), (1, 256), (257, 0), (3, 1)])
def test_bias_exact(m, n):
    """[1 | A] with m (n + 1) = 255, 256, 257 (the 256-thread blocks' edge), n = 0, ldo > n + 1"""
    import torch
    L, h = _lib()
    A = np.random.default_rng(m + n).normal(size=(m, n))
    Ad = _padded(A, n + 3, float("nan"))
    out = torch.full((m, n + 3), SENT, dtype=torch.float64, device="cuda")
    assert h.lib.ipm_lasso_bias(h.ptr, m, n, L.dptr(Ad), n + 3, L.dptr(out), n + 3) == 0
    o = G.host(out)
    assert np.array_equal(o[:, :n + 1], np.hstack((np.ones((m, 1)), A))) and np.all(o[:, n + 1:] == SENT)


@pytest.mark.parametrize("rows,cols", [(1, 1), (15, 17), (16, 16), (257, 1), (33, 31)])
def test_scale_bit_equal(rows, cols):
    L, h = _lib()
    M = np.random.default_rng(rows + cols).normal(size=(rows, cols))
    f1, f2 = -151 * 0.4, 0.4
    for two, ref in ((0, M * f1), (1, (M * f1) * f2)):
        Md = _padded(M, cols + 2, SENT)
        assert h.lib.ipm_lasso_scale(h.ptr, rows, cols, L.dptr(Md), cols + 2, f1, f2, two) == 0
        o = G.host(Md)
        assert np.array_equal(o[:, :cols], ref) and np.all(o[:, cols:] == SENT)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 257])
def test_block_qs_exact(n):
    """the permutation include/ipm355.h states, rows past n zero, from a Qs with ldq > n"""
    import torch
    L, h = _lib()
    Qs = np.random.default_rng(n).normal(size=(n, n))
    tot = int(h.lib.ipm_lasso_qb_doubles(n))
    assert tot == -(-n // 32) * 32 * n
    Qb = torch.full((tot + 4,), SENT, dtype=torch.float64, device="cuda")
    assert h.lib.ipm_lasso_block_qs(h.ptr, n, L.dptr(_padded(Qs, n + 3, float("nan"))), n + 3, L.dptr(Qb)) == 0
    o = G.host(Qb)
    assert np.array_equal(o[:tot], R.block_qs(Qs)) and np.all(o[tot:] == SENT)
    assert h.lib.ipm_lasso_qb_doubles(0) == 0


# ------------------------------------------------------------------ g. ipm_lasso_qinv
QINV_MARGIN = 8.0


def _run_qinv(A, n, rho, ldq):
    import torch
    L, h = _lib()
    m = A.shape[0]
    Ad = _padded(A, n + 2, float("nan")) if m else G.devnan((1, n + 2))
    Q = torch.full((n, ldq), SENT, dtype=torch.float64, device="cuda")
    QT = torch.full((n, ldq), SENT, dtype=torch.float64, device="cuda")
    info = ctypes.c_int(-7)
    rc = h.lib.ipm_lasso_qinv(h.ptr, m, n, L.dptr(Ad), n + 2, rho, L.dptr(Q), L.dptr(QT), ldq, ctypes.byref(info))
    return rc, info.value, G.host(Q), G.host(QT)


@pytest.mark.parametrize("pad", [0, 3], ids=["ldq=n", "ldq=n+3"])
@pytest.mark.parametrize("m,n", [(5, 1), (40, 127), (300, 128), (300, 129), (600, 257)])
def test_qinv_residual(m, n, pad):
    """Q = (m rho I + A^T A)^-1 through the MFMA GEMM, the blocked Cholesky and the multi-RHS solves
    at n around the 128 block: QT is Q^T bit for bit, info 0, and the residual ||M Q - I||_F (M formed
    and multiplied in long double) at most 8 x that of scipy's cho_solve(cho_factor(M), I) -- the
    same algorithm in another blocking order"""
    import scipy.linalg
    rho = 0.4
    A = np.random.default_rng(m + n).normal(size=(m, n))
    rc, info, Q, QT = _run_qinv(A, n, rho, n + pad)
    assert (rc, info) == (0, 0)
    assert np.array_equal(QT[:, :n], Q[:, :n].T)
    assert np.all(Q[:, n:] == SENT) and np.all(QT[:, n:] == SENT)
    assert np.all(np.isfinite(Q[:, :n]))
    Ml = A.astype(R.LD).T @ A.astype(R.LD) + R.LD(m) * R.LD(rho) * np.eye(n, dtype=R.LD)
    M64 = np.diag(np.ones(n) * m * rho) + A.T @ A
    Qref = scipy.linalg.cho_solve(scipy.linalg.cho_factor(M64), np.eye(n))

    def res(X):
        return float(np.linalg.norm((Ml @ X.astype(R.LD) - np.eye(n, dtype=R.LD)).astype(np.float64)))
    r_dev, r_ref = res(Q[:, :n]), res(Qref)
    print(f"[qinv m {m} n {n} ldq {n + pad}] residual device {r_dev:.3g}, scipy {r_ref:.3g}, ratio {r_dev / r_ref:.3g}")
    assert r_dev <= QINV_MARGIN * r_ref


def test_qinv_not_positive_definite():
    """m = 0: M = 0, the first pivot fails -> IPM_NOT_POSITIVE_DEFINITE, info 1"""
    L, _ = _lib()
    rc, info, _, _ = _run_qinv(np.zeros((0, 5)), 5, 0.4, 5)
    assert (rc, info) == (L.IPM_NOT_POSITIVE_DEFINITE, 1)


# ------------------------------------------------------------------ h. argument checks
def test_admm_rejects_bad_arguments():
    """every rejected combination returns IPM_INVALID_ARG and leaves the state as it was"""
    L, _ = _lib()
    st = R.state(33, 31, seed=2)

    def rejected(change, **kw):
        dv = R.DeviceStep(st, lds=36, qs_blocked=0, ldq=36, **kw)
        before = {k: G.host(dv.t[k]).copy() for k in ("x", "alpha", "u", "W0", "W1", "partial")}
        change(dv.args)
        rc, it = dv.run()
        assert rc == L.IPM_INVALID_ARG and it == -99, (rc, it)
        for k, v in before.items():
            assert np.array_equal(G.host(dv.t[k]), v, equal_nan=True), k

    rejected(lambda a: setattr(a, "lds", 30))
    rejected(lambda a: setattr(a, "ldq", 32))
    rejected(lambda a: setattr(a, "check_stop", 0))
    rejected(lambda a: setattr(a, "max_iters", -1))
    rejected(lambda a: setattr(a, "n", 0))
    rejected(lambda a: setattr(a, "S", 0))
    for k in ("Qs", "bA", "eta", "x", "alpha", "u", "W0", "W1", "partial"):
        rejected(lambda a, k=k: setattr(a, k, None))
    # compute_loss without gaps / AT / R
    import torch
    rng = np.random.default_rng(1)
    A, b, reg = rng.normal(size=(7, 33)), rng.normal(size=(7, 31)), np.full(31, 0.3)
    for missing in ("gaps", "AT", "R"):
        dv = R.DeviceStep(st)
        _loss_fields(dv, A, b, reg, 0, 0)
        gaps = torch.full((2, 31), SENT, dtype=torch.float64, device="cuda")
        dv.args.compute_loss, dv.args.gaps, dv.args.ldg = 1, L.dptr(gaps), 31
        setattr(dv.args, missing, None)
        before = G.host(dv.t["alpha"]).copy()
        rc, it = dv.run()
        assert rc == L.IPM_INVALID_ARG and it == -99
        assert np.array_equal(G.host(dv.t["alpha"]), before) and np.all(G.host(gaps) == SENT)


def test_helpers_reject_bad_arguments():
    import torch
    L, h = _lib()
    lib, bad = h.lib, L.IPM_INVALID_ARG
    buf = torch.full((64,), SENT, dtype=torch.float64, device="cuda")
    p = L.dptr(buf)
    assert lib.ipm_lasso_prox(h.ptr, 4, 4, p, 3, p, 0, 0, 0, p, 4) == bad        # ldv < S
    assert lib.ipm_lasso_prox(h.ptr, 4, 4, p, 4, p, 0, 0, 0, p, 3) == bad        # ldo < S
    assert lib.ipm_lasso_colnorm(h.ptr, 0, 4, p, 4, None) == bad                 # no rows
    assert lib.ipm_lasso_colnorm(h.ptr, 4, 4, p, 3, None) == bad                 # lda < n
    assert lib.ipm_lasso_bias(h.ptr, 4, 4, p, 4, p, 4) == bad                    # ldo < n + 1
    assert lib.ipm_lasso_scale(h.ptr, 4, 4, p, 3, 2.0, 2.0, 0) == bad            # ld < cols
    assert lib.ipm_lasso_block_qs(h.ptr, 4, p, 3, p) == bad                      # ldq < n
    assert lib.ipm_lasso_block_qs(h.ptr, 4, None, 4, p) == bad
    info = ctypes.c_int(-7)
    assert lib.ipm_lasso_qinv(h.ptr, 4, 4, p, 4, 0.4, p, p, 3, ctypes.byref(info)) == bad   # ldq < n
    assert lib.ipm_lasso_qinv(h.ptr, 4, 4, p, 4, 0.4, None, p, 4, ctypes.byref(info)) == bad
    assert info.value == -7
    assert lib.ipm_lasso_loss(h.ptr, None, 1, p, None) == bad
    assert np.all(G.host(buf) == SENT)
