"""No GPU: the inputs of tests/test_gpu_barrier_shapes.py checked against the reference alone.

The GPU module holds the device to entry-wise bounds derived in tests/barrier_ref.py and to the
oracle's own line-search decisions.  Here the fp64 oracle itself is held to a quarter of the same
bounds (against the long-double evaluation), and every Newton-step instance is shown to be decisive
and to cover what it is there to cover -- so a later change of a seed or a shape cannot quietly turn
a GPU assertion into a coin flip.
"""
import numpy as np
import pytest

import barrier_ref as R


@pytest.mark.parametrize("spec", R.lpqp_specs(), ids=R.spec_id)
def test_oracle_within_quarter_of_bounds(spec):
    """slacks, barrier objective, gradient, Hessian (and the stale-slack pair) of the fp64 oracle
    against the long-double formulas: at most 0.25 of each entry-wise bound.  Where n * n * m
    exceeds barrier_ref.LD_HESS_FLOPS (n = 1026, 1027, 1400 with m >= 255, and (130, 7997)) the
    Hessian reference IS the fp64 oracle (the long-double product would take seconds), so its
    ratio of 0 there is no measurement: only the bound's own finiteness is checked by it."""
    inst = R.instance(spec)
    ratios = R.lpqp_ratios(inst, R.oracle_values(inst))
    print(f"[{inst.name}] oracle err / bound: " + ", ".join(f"{k} {v:.2g}" for k, v in ratios.items()))
    assert R.all_within(ratios, 0.25), ratios


def test_shape_coverage():
    """the shapes the issue names are all there"""
    lpqp = [R.instance(s) for s in R.lpqp_specs()]
    ph1 = [R.instance(s) for s in R.ph1_specs()]
    for group in ([i for i in lpqp if i.kind == "lp"], [i for i in lpqp if i.kind == "qp"], ph1):
        assert {1, 2, 63, 64, 65, 130, 513, 1026, 1027, 1400} <= {i.n for i in group}
        assert (200, 2049) in {(i.n, i.m) for i in group}
        assert {"both", "lb", "ub", "none"} <= {i.bounds for i in group}
        assert len(group) >= 10
    assert {1, 5, 255, 257, 300} <= {i.m for i in lpqp} and {1, 5, 255, 257, 300} <= {i.m for i in ph1}
    assert any(i.kind == "qp" and i.m == 0 and i.bounds != "none" for i in lpqp)
    assert sum(i.kind == "lp" and i.tiny for i in lpqp) >= 3 and sum(i.kind == "qp" and i.tiny for i in lpqp) >= 3
    assert any(i.kind == "lpdiag" and i.n == 1027 for i in lpqp)
    socp = [R.socp_instance(s) for s in R.socp_specs()]
    assert {130, 257} == {i.n for i in socp} and {1, 6} == {i.K for i in socp}
    rows = {(a.shape[0] if a.ndim > 1 else 0) for i in socp for a in i.A}
    assert {0, 1, 255, 256, 257, 600} <= rows
    assert any(i.b is None for i in socp) and any(i.c is None for i in socp) and any(i.d is None for i in socp)
    assert any(i.b is not None and i.c is not None and i.d is not None for i in socp)


@pytest.mark.parametrize("spec", R.socp_specs(), ids=R.spec_id)
def test_socp_start_is_interior(spec):
    """every cone slack at least 0.1 rhs^2 and every slack in [0.05, 2] (phase 1: shifted by its
    s, so the smallest is 1): no entry dominates the relative norms of the GPU test"""
    inst = R.socp_instance(spec)
    v = R.oracle_values(inst)
    s, K = v["slacks"], inst.K
    rhs = s[-K:]
    assert np.all(s[:K] >= 0.1 * rhs ** 2 * (1 - 1e-12))
    assert s.min() >= 0.05 and s[:-K].max() <= 2.0 + 1e-12 and rhs.max() <= 2.0
    vp = R.oracle_values(inst, True)
    assert abs(vp["slacks"][:-K].min() - 1.0) <= 1e-12 and vp["slacks"].max() <= 3.0


@pytest.mark.parametrize("spec", R.ph1_specs(), ids=R.spec_id)
def test_phase1_slacks_are_order_one(spec):
    """phase 1 starts at s = 1 - min(slack), so on every instance of the sweep (each n, m and bound
    combination; 'ph1-384-257' is the Newton-step instance) the smallest slack is 1 and the largest
    below 3: the relative norms of test_phase1_protocol are not dominated by single entries"""
    v = R.oracle_values(R.instance(spec))
    assert abs(v["slacks"].min() - 1.0) <= 1e-12 and v["slacks"].max() <= 3.0


@pytest.mark.parametrize("entry", R.newton_specs(), ids=lambda e: e[0])
def test_newton_step_reference_is_decisive(entry):
    """every line-search decision of the reference on this instance is at least 1e-9 from flipping
    (feasibility: min_i |s_i| >= 1e-9 max|s0| at each candidate; Armijo: |f - (f0 + a step g.x)|
    >= 1e-9 max(1, |f0|) at each candidate), and the x bound of the GPU test is below 1e-8 ||x||"""
    r = R.reference_newton_step(entry)
    print(f"[{entry[0]}] S {r['S']} k {r['k']} (feasibility {r['k_feas']}) step {r['step']:.6g} cond2 {r['cond2']:.3g} "
          f"feas margin {r['feas_margin']:.2g} armijo margin {r['armijo_margin']:.2g} "
          f"first blocking slack {r['first_block']}")
    assert r["iters"] == 1
    assert r["feas_margin"] >= R.MARGIN
    assert r["armijo_margin"] >= R.MARGIN
    assert R.x_bound(r) < 1e-8 * np.linalg.norm(r["x"])
    beta, st = entry[3], 1
    for _ in range(r["k"]):
        st *= beta
    assert st == r["step"]


def test_ratio_and_rel_reject_non_finite():
    """a NaN or Inf in a checked value must fail the comparison, wherever it stands in the dict"""
    ref, bound = np.ones(4), np.full(4, 1e-3)
    for bad in (np.nan, np.inf, -np.inf):
        got = ref.copy()
        got[2] = bad
        assert R.ratio(got, ref, bound) == np.inf and R.rel(got, ref) == np.inf
        assert R.ratio(bad, 1.0, 1e-3) == np.inf
        assert not R.all_within({"a": 0.1, "b": R.ratio(got, ref, bound), "c": 0.2}, 1.0)
    assert not R.all_within({"a": 0.1, "b": float("nan")}, 1.0)
    assert R.ratio(ref, ref, np.zeros(4)) == 0.0 and R.ratio(ref + 1e-6, ref, np.zeros(4)) == np.inf
    assert R.ratio(ref[:3], ref, bound) == np.inf and R.rel(ref[:3], ref) == np.inf
    assert R.all_within({"a": 0.1, "b": 1.0}, 1.0)


def test_newton_step_coverage():
    """S hits every k_ls_fold case; 0 and >= 3 backtracks; a first blocking slack in the last,
    partial, 64-slack block of several and one at index 0; the beta = 0.97 instance accepts
    k in 65..120 (the second 64-candidate pass); LP, QP, LP phase 1 and two SOCPs take part"""
    refs = {e[0]: R.reference_newton_step(e) for e in R.newton_specs()}
    assert {1, 63, 64, 65, 960, 1025, 1088, 8257} <= {r["S"] for r in refs.values()}
    assert any(r["k"] == 0 for r in refs.values())
    assert any(r["k"] >= 3 for r in refs.values())
    assert any(r["first_block"] == 0 for r in refs.values())
    assert any(r["S"] > 64 and r["S"] % 64 and r["first_block"] >= r["S"] // 64 * 64 for r in refs.values())
    far = [(e, refs[e[0]]) for e in R.newton_specs() if e[3] == 0.97]
    assert len(far) == 1 and 65 <= far[0][1]["k"] <= 120
    kinds = [R.newton_instance(e).kind for e in R.newton_specs()]
    assert {"lp", "qp", "ph1"} <= set(kinds) and kinds.count("socp") >= 2
