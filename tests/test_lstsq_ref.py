"""CPU: the least-squares reference (lstsq_ref) against LAPACK, and the properties of its instances
that tests/test_gpu_lstsq.py relies on:
  * x_ref agrees with np.linalg.lstsq(H, B, rcond=None) within the bound the GPU test applies, and
    NumPy's rank is the prescribed kept count (it keeps and drops the same eigenvalues);
  * every kept / dropped decision is decisive: no |lambda_i| within a factor of 4 of
    eps n max|lambda| (the cut-edge instances sit at exactly 8 x and 1 / 8);
  * np.linalg.eigh stays within C1 / 8 and C2 / 8 on every instance (the constants are 8 x its worst);
  * np.linalg.lstsq raises LinAlgError on the non-finite inputs.
"""
import numpy as np
import pytest

import lstsq_ref as R

INSTANCES = list(R.all_instances())
NRHS = [1, 7, 8, 9, 33]


def test_instance_set_covers_the_shapes():
    names = {i.name for i in INSTANCES}
    assert len(names) == len(INSTANCES)
    for n in R.SHAPES:
        assert f"full-{n}" in names and f"repeated-{n}" in names
    assert {"neg-1x1", "cutedge-64", "cutedge-320", "zero-300", "diagonal-300"} <= names


@pytest.mark.parametrize("inst", INSTANCES, ids=[i.name for i in INSTANCES])
def test_instance_is_decisive_and_numpy_agrees(inst):
    n, lam = inst.n, inst.lam
    assert np.array_equal(inst.H, inst.H.T)
    c = R.cut(lam)
    a = np.abs(lam)
    assert np.all((a >= 4 * c) | (a <= c / 4)), "an eigenvalue within a factor of 4 of the cut"
    np.testing.assert_array_equal(inst.kept, a > c)
    if inst.name.startswith("cutedge"):
        assert a.max() == 1.0 and a[n - 2] == 8 * c and a[n - 1] == c / 8
        assert inst.kept[n - 2] and not inst.kept[n - 1] and inst.kept.sum() == n - 1
    worst = 0.0
    for nrhs in NRHS:
        B = R.rhs(n, nrhs)
        x, _, rank, _ = np.linalg.lstsq(inst.H, B, rcond=None)
        assert rank == inst.kept.sum()
        worst = max(worst, R.solution_ratio(inst, x, B), R.null_ratio(inst, x))
    if inst.name.startswith(("zero", "diagonal")):
        x = np.linalg.lstsq(inst.H, R.rhs(n, 3), rcond=None)[0]
        with np.errstate(divide="ignore"):
            exact = np.where(inst.kept[:, None], R.rhs(n, 3) / lam[:, None], 0.0)
        np.testing.assert_allclose(x, exact, rtol=8 * R.EPS, atol=0)
    print(f"[{inst.name}] numpy lstsq worst err / bound {worst:.3g}")
    assert worst <= 1.0


def test_eigh_calibrates_the_constants():
    """C1, C2 = 8 x the worst of q1 and of max(q2, q3) that np.linalg.eigh reaches (never the device)"""
    w1 = w2 = 0.0
    table = {}
    for inst in INSTANCES:
        _, V = np.linalg.eigh(inst.H)
        q = R.eig_quantities(inst.H, V, inst.lam)
        t = table.setdefault(inst.name.rsplit("-", 1)[0], [0.0, 0.0, 0.0])
        for i in range(3):
            t[i] = max(t[i], q[i])
        w1, w2 = max(w1, q[0]), max(w2, q[1], q[2])
    for k, t in table.items():
        print(f"eigh {k:10s} q1 {t[0]:.3f} q2 {t[1]:.3f} q3 {t[2]:.3f}")
    print(f"worst q1 {w1:.3f} -> C1 {R.C1}; worst q2, q3 {w2:.3f} -> C2 {R.C2}")
    assert w1 <= R.C1 and w2 <= R.C2


def test_matmul_ld_is_a_long_double_product():
    rng = np.random.default_rng(5)
    A, B = rng.normal(size=(70, 90)) * 1e3, rng.normal(size=(90, 40)) * 1e-5
    ref = A.astype(R.LD) @ B.astype(R.LD)
    assert np.abs(R.matmul_ld(A, B) - ref).max() <= 90 * 2.0 ** -58 * np.abs(A).max() * np.abs(B).max()


NONFINITE = list(R.nonfinite_inputs())


@pytest.mark.parametrize("name,H", NONFINITE, ids=[s[0] for s in NONFINITE])
def test_numpy_lstsq_raises_on_nonfinite_input(name, H):
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.lstsq(H, R.rhs(H.shape[0], 1), rcond=None)
