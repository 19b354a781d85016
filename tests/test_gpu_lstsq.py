"""-m gpu: the symmetric minimum-norm least squares (ipm_lstsq_sym: the one-workgroup Jacobi
k_jacobi_wg, the blocked MFMA Jacobi k_bj_eig / k_bj_tile / k_bj_rows / k_bj_cols, the rcond cut
k_jacobi_weights and both apply paths) on matrices with a prescribed spectrum (tests/lstsq_ref.py).

Layout: A full symmetric, column-major with leading dimension lda.  On return A holds W = V^T:
A(i, j) = V(j, i), i.e. memory element [j * lda + i] is component j of eigenvector i -- a device
tensor of shape (n, lda) therefore has V(c, r) at [c, r]: its first n columns ARE V, eigenvectors in
columns.  B row-major n x nrhs (ldb), replaced by X.  The padding of A (lda > n) and of B
(ldb > nrhs) holds a sentinel that must come back untouched.

What is held, with eps = 2^-52 and lambda = diag(V^T H V) evaluated on the host in long double:
  q1  ||V^T V - I||_max                        <= C1 n eps
  q2  ||H V - V diag(lambda)||_F               <= C2 n eps ||H||_F
  q3  max |sort(lambda) - sort(prescribed)|    <= C2 n eps ||H||_F
  x   ||x - x_ref|| / ||x_ref||                <= 64 n eps max|lambda| / min_kept|lambda|   per column
  N   ||N^T x|| / ||x||                        <= the same, N the prescribed null vectors
  info == 0 and IPM_OK.
C1, C2 are 8 x the worst value np.linalg.eigh itself reaches over the whole instance set, measured on
the CPU by tests/test_lstsq_ref.py (never the device's):
    class        eigh q1   q2      q3
    full         0.867    0.458   0.908
    indef        0.377    0.600   0.936
    repeated     0.309    0.319   0.787
    clustered    1.313    0.792   0.911        (q1: n = 2, where n eps is two units)
    psd_def      0.405    0.306   0.200
    indef_def    0.347    0.258   0.159
    cut-edge     0.003    0.005   0.002        (diagonal, zero, 1 x 1: 0)
    worst        1.313            0.936   ->   C1 = 10.5, C2 = 7.5
The solution bound is the conditioning of the kept part times the eigensolver's backward error;
np.linalg.lstsq stays within it on every instance and right-hand side used here (same CPU test).
Each test prints its worst ratios (value / bound).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lstsq_ref as R
from gpu_util import dev, host, lstsq_sym

pytestmark = pytest.mark.gpu
IPM_OK, IPM_INVALID_ARG = 0, 2
SENTINEL = 12345.0


def _device(H, lda, B, ldb):
    """-> (rc, info, V, X)"""
    import torch
    n, nrhs = H.shape[0], B.shape[1]
    Ad = torch.full((n, lda), SENTINEL, dtype=torch.float64, device="cuda")
    Ad[:, :n] = dev(H.T)
    Bd = torch.full((n, ldb), SENTINEL, dtype=torch.float64, device="cuda")
    Bd[:, :nrhs] = dev(B)
    rc, info = lstsq_sym(Ad, n, lda, Bd, nrhs, ldb)
    A, Bm = host(Ad), host(Bd)
    assert np.all(A[:, n:] == SENTINEL), "padding of A written"
    assert np.all(Bm[:, nrhs:] == SENTINEL), "padding of B written"
    return rc, info, A[:, :n].copy(), Bm[:, :nrhs].copy()


def _eig_ratios(inst, V):
    q1, q2, q3 = R.eig_quantities(inst.H, V, inst.lam)
    return {"q1": q1 / R.C1, "q2": q2 / R.C2, "q3": q3 / R.C2}


def run_checked(inst, layouts, seen=None):
    """every (lda, nrhs, ldb) of layouts on the device -> (worst ratios, the last X).  The
    eigenvector checks run once per distinct V (V does not depend on B)."""
    worst = {"q1": 0.0, "q2": 0.0, "q3": 0.0, "x": 0.0, "N": 0.0}
    Vs, X = None, None
    for lda, nrhs, ldb in layouts:
        B = R.rhs(inst.n, nrhs)
        rc, info, V, X = _device(inst.H, lda, B, ldb)
        assert rc == IPM_OK and info == 0, (inst.name, lda, nrhs, ldb, rc, info)
        r = {"x": R.solution_ratio(inst, X, B), "N": R.null_ratio(inst, X)}
        if Vs is None or not np.array_equal(Vs, V):
            r.update(_eig_ratios(inst, V))
            Vs = V
        for k, v in r.items():
            worst[k] = max(worst[k], v)
    return worst, X, Vs


def _report(tag, worst):
    print(f"[lstsq {tag}] " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("kind,n", R.SPECTRA)
def test_lstsq_spectra(kind, n):
    """n = 1, 2, 3, 31, 32, 33, 255, 256: k_jacobi_wg (odd n: the JSINGLE dummy pair; 256 the largest
    one-workgroup size); 257 (9 -> 10 blocks of 32), 320 (10), 321 (11 -> 12), 511, 512 (16; the
    apply switch): the blocked Jacobi.  Spectra: full rank logspace 1 .. 1e-3; the same with mixed
    signs; rank n // 2 PSD and indefinite (n >= 4); half exactly 2 and half exactly -1 (V held
    through residual and orthogonality only, as every V here); clustered 1 + k 1e-12.
    lda = n with one right-hand side, lda = n + 5 with nine (ldb = 12)."""
    inst = R.instance(kind, n)
    worst, _, _ = run_checked(inst, [(n, 1, 1), (n + 5, 9, 12)])
    _report(f"{kind}-{n}", worst)


def _apply_layouts(n):
    full = [(nr, ld) for nr in (1, 7, 8, 9, 33) for ld in (nr, nr + 3)]
    some = [(1, 1), (7, 10), (8, 8), (9, 12), (33, 36)]
    return [(lda, nr, ld) for lda in (n, n + 5) for nr, ld in (full if n >= 511 else some)]


@pytest.mark.parametrize("n", [33, 256, 257, 320, 511, 512])
def test_lstsq_apply_layouts(n):
    """The apply switch (nrhs < 8 or n < 512: k_vtb + k_vt; else two MFMA GEMMs) on a rank-deficient
    indefinite matrix: nrhs = 1, 7, 8, 9, 33, ldb = nrhs and nrhs + 3, lda = n and n + 5 -- at
    n = 511 and 512 every combination (all four of nrhs < 8 / >= 8 x n < 512 / >= 512), below a
    subset with both lda on both sides of the 256 / 257 eigensolver switch."""
    inst = R.instance("indef_def", n)
    worst, _, _ = run_checked(inst, _apply_layouts(n))
    _report(f"layouts-{n}", worst)


@pytest.mark.parametrize("n", [5, 33, 300])
def test_lstsq_already_diagonal(n):
    """Q = I: no entry passes the rotation test, so V is exactly the identity and X exactly
    b / lambda (lambda = +-2^-k, the weights exact)."""
    inst = R.diagonal_instance(n)
    for lda, nrhs, ldb in [(n, 1, 1), (n + 5, 9, 12)]:
        B = R.rhs(n, nrhs)
        rc, info, V, X = _device(inst.H, lda, B, ldb)
        assert rc == IPM_OK and info == 0
        np.testing.assert_array_equal(V, np.eye(n))
        np.testing.assert_array_equal(X, B / inst.lam[:, None])


@pytest.mark.parametrize("n", [3, 33, 300])
def test_lstsq_zero_matrix(n):
    """frob2 = 0, every weight 0: X exactly 0 (as NumPy's), V the identity"""
    inst = R.zero_instance(n)
    for lda, nrhs, ldb in [(n, 1, 1), (n + 5, 9, 12)]:
        rc, info, V, X = _device(inst.H, lda, R.rhs(n, nrhs), ldb)
        assert rc == IPM_OK and info == 0
        np.testing.assert_array_equal(V, np.eye(n))
        np.testing.assert_array_equal(X, np.zeros((n, nrhs)))


def test_lstsq_1x1_negative():
    inst = R.Instance("neg-1x1", 1, np.array([-3.0]), np.eye(1), np.array([[-3.0]]), np.ones(1, dtype=bool))
    B = R.rhs(1, 3)
    rc, info, V, X = _device(inst.H, 6, B, 6)
    assert rc == IPM_OK and info == 0
    np.testing.assert_array_equal(V, [[1.0]])
    np.testing.assert_allclose(X, B / -3.0, rtol=2 * R.EPS, atol=0)


@pytest.mark.parametrize("n", [64, 320])
def test_lstsq_cut_edge(n):
    """One eigenvalue at 8 eps n max|lambda| (kept: it sets the conditioning, 1 / (8 n eps)) and one
    at eps n max|lambda| / 8 (dropped: the solution has no component along its vector)."""
    inst = R.cut_edge_instance(n)
    worst, X, _ = run_checked(inst, [(n, 1, 1), (n + 5, 9, 12)])
    _report(f"cutedge-{n}", worst)
    B = R.rhs(n, 9)
    kept_comp = inst.Q[:, n - 2] @ X          # = (q . b) / lambda for the kept edge eigenvalue
    want = (inst.Q[:, n - 2] @ B) / inst.lam[n - 2]
    np.testing.assert_allclose(kept_comp, want, rtol=1e-6)
    assert np.all(np.abs(inst.Q[:, n - 1] @ X) <= 1e-6 * np.abs(kept_comp))


# ---- IPM_BJ_FUSED / IPM_BJ_INNER: read once per process, so each setting runs in a child
KNOB_CASES = [("full", 257), ("psd_def", 257), ("full", 321), ("psd_def", 321)]
KNOB_LAYOUTS = lambda n: [(n + 5, 9, 12)]   # noqa: E731
_KNOB_CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import lstsq_ref as R
from test_gpu_lstsq import KNOB_CASES, KNOB_LAYOUTS, run_checked
out, xs = {}, {}
for kind, n in KNOB_CASES:
    worst, X, _ = run_checked(R.instance(kind, n), KNOB_LAYOUTS(n))
    out[f"{kind}-{n}"] = worst
    xs[f"{kind}-{n}"] = X
np.savez(sys.argv[3], **xs)
print("RATIOS", json.dumps(out))
"""


@pytest.mark.parametrize("knob,value", [("IPM_BJ_FUSED", "0"), ("IPM_BJ_INNER", "3")])
def test_lstsq_blocked_jacobi_knobs(knob, value, tmp_path):
    """IPM_BJ_FUSED=0 (k_bj_rows + the two-plane k_bj_cols instead of k_bj_tile) and IPM_BJ_INNER=3
    (three inner sweeps per subproblem, fused update) at n = 257 and 321, full rank and rank
    deficient, each in one fresh child process: the same checks as the default.  FUSED=0 differs
    from the default only in the order of two 64 x 64 products, so its X must also agree with the
    default's within the solution bound (observed: bitwise equal).

    The inner sweeps after the first apply their rotations in the small-angle form (rot_fine in
    ipm_lstsq.hip).  With the plain form in every sweep, k inner sweeps applied about k times the
    elementary rotations without saving an outer sweep and the rounding grew in proportion:
    IPM_BJ_INNER=3 missed these bounds (psd_def-321: q1 1.09, q2 1.17 of them; orthogonality 2.9,
    5.7, 8.2 n eps for k = 1, 2, 3 on full-257).  Now k = 3 gives q1 <= 0.37, q2 <= 0.45."""
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.join(here, "..", "interiorpoint-gpu_amd")
    npz = str(tmp_path / "x.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("IPM_BJ_FUSED", "IPM_BJ_INNER")}
    env[knob] = value
    out = subprocess.run([sys.executable, "-c", _KNOB_CHILD, here, pkg, npz], env=env, capture_output=True,
                         text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    ratios = json.loads(out.stdout.split("RATIOS")[-1])
    xs = np.load(npz)
    for tag, worst in ratios.items():      # (every figure before the first assertion)
        print(f"[lstsq {knob}={value} {tag}] " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for kind, n in KNOB_CASES:
        tag = f"{kind}-{n}"
        _report(f"{knob}={value} {tag}", ratios[tag])
        if knob == "IPM_BJ_FUSED":
            inst = R.instance(kind, n)
            _, Xd, _ = run_checked(inst, KNOB_LAYOUTS(n))
            ref = inst.x_ref(R.rhs(n, 9))
            rel = np.linalg.norm(xs[tag] - Xd, axis=0) / np.linalg.norm(ref, axis=0)
            r = float(rel.max() / (64 * n * R.EPS * inst.cond))
            print(f"[lstsq {knob}={value} {tag}] X against the default's: {r:.3g} of the bound")
            assert r <= 1.0


@pytest.mark.parametrize("name", R.NONFINITE_NAMES)
def test_lstsq_nonfinite_input_reports_failure(name):
    """A NaN pair, a +Inf diagonal entry, an all-NaN matrix at n = 5 (one workgroup) and n = 300
    (blocked): np.linalg.lstsq raises LinAlgError on each (tests/test_lstsq_ref.py); the device must
    report info == 1 -- never info == 0 together with a finite X."""
    H = dict(R.nonfinite_inputs())[name]
    n = H.shape[0]
    for lda, nrhs, ldb in [(n, 1, 1), (n + 5, 9, 12)]:
        rc, info, V, X = _device(H, lda, R.rhs(n, nrhs), ldb)
        print(f"[lstsq {name} lda={lda}] rc {rc} info {info} X finite: {bool(np.all(np.isfinite(X)))}")
        assert rc == IPM_OK
        assert not (info == 0 and np.all(np.isfinite(X))), "info 0 with a finite X from a non-finite matrix"
        assert info == 1


def test_lstsq_invalid_arguments_and_empty_sizes():
    """lda < n, ldb < nrhs, negative n / nrhs: IPM_INVALID_ARG, A and B untouched; n = 0 and
    nrhs = 0: IPM_OK (info 0), nothing touched."""
    import torch
    n = 4
    A = torch.full((n, n), SENTINEL, dtype=torch.float64, device="cuda")
    B = torch.full((n, 3), SENTINEL, dtype=torch.float64, device="cuda")
    assert lstsq_sym(A, n, n - 1, B, 3, 3)[0] == IPM_INVALID_ARG
    assert lstsq_sym(A, n, n, B, 3, 2)[0] == IPM_INVALID_ARG
    assert lstsq_sym(A, -1, n, B, 3, 3)[0] == IPM_INVALID_ARG
    assert lstsq_sym(A, n, n, B, -1, 3)[0] == IPM_INVALID_ARG
    assert lstsq_sym(A, 0, n, B, 3, 3) == (IPM_OK, 0)
    assert lstsq_sym(A, n, n, B, 0, 3) == (IPM_OK, 0)
    assert np.all(host(A) == SENTINEL) and np.all(host(B) == SENTINEL)
