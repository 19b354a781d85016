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


@pytest.mark.parametrize("phase1", [False, True], ids=["socp", "socp-phase1"])
@pytest.mark.parametrize("spec", R.socp_all_specs(), ids=R.spec_id)
def test_socp_oracle_within_quarter_of_bounds(spec, phase1):
    """lhs, rhs, slacks, barrier objective, gradient, Hessian (phase 1: with its border) and the
    stale-slack pair of the fp64 oracle against socp_reference: at most 0.25 of each entry-wise
    bound, on the four interior instances and on every edge instance (cones at 1e-4 and 1e-6 of
    the boundary included).  Measured: at most 0.13 (the slacks; every other quantity below 0.03)."""
    inst = R.socp_instance(spec)
    ratios = R.socp_ratios(inst, R.oracle_values(inst, phase1), phase1)
    print(f"[{inst.name}{' phase 1' if phase1 else ''}] oracle err / bound: "
          + ", ".join(f"{k} {v:.2g}" for k, v in ratios.items()))
    assert set(ratios) == {"lhs", "rhs", "slacks", "nobj", "grad", "hess", "stale_nobj", "stale_grad"}
    assert R.all_within(ratios, 0.25), ratios


@pytest.mark.parametrize("spec", R.socp_near_specs(), ids=R.spec_id)
def test_socp_near_boundary_margin_and_bound(spec):
    """each near-boundary instance reaches its smallest requested margin (min_i s_i / rhs_i^2 within
    a factor 2 of it, every cone within a factor 2 of its own, the others at 0.1 or more), and the
    bounds stay decisive there: on the gradient entries that the mu <= 1e-6 cones dominate the bound
    is at most 1e-2 of the entry, so an error of a few per cent of one cone's piece cannot pass"""
    inst = R.socp_instance(spec)
    r0 = R.socp_refs(inst)[0]
    K = inst.K
    marg = (r0["slacks"][:K] / r0["rhs"] ** 2).astype(np.float64)
    want = min(m for m in inst.mu if m is not None)
    print(f"[{inst.name}] min s / rhs^2 {marg.min():.6g} (requested {want:g})")
    assert np.all(r0["rhs"] > 0)
    assert want / 2 <= marg.min() <= 2 * want
    for m, got in zip(inst.mu, marg):
        assert (m / 2 <= got <= 2 * m) if m is not None else got >= 0.1 * (1 - 1e-12)
    if want <= 1e-6:
        dom = R.near_dominated(inst, r0)
        rel = r0["b_grad"][dom] / np.abs(r0["grad"][dom].astype(np.float64))
        print(f"[{inst.name}] {dom.sum()} of {inst.n} gradient entries dominated, bound / |entry| at most {rel.max():.2g}")
        assert dom.sum() >= inst.n // 4
        assert rel.max() <= 1e-2


def test_socp_edge_coverage():
    """the edge instances the cone kernels have: cones of 1 .. 600 rows with near-boundary ones at
    n = 130 and 257, one without c and one without d; dslot 0, 1, 2 between dense cones with a near
    diagonal one at n > 256; R = 0; K = 257 (cone 256 near) and 513; n = 2 and 513"""
    insts = [R.socp_instance(s) for s in R.socp_edge_specs()]
    rows = lambda i: tuple(a.shape[0] if a.ndim > 1 else 0 for a in i.A)
    near = [i for i in insts if rows(i) == (1, 255, 256, 257, 600, 0) and any(m is not None for m in i.mu)]
    assert {130, 257} <= {i.n for i in near}
    assert any(i.c is None for i in near) and any(i.d is None for i in near)
    for i in near:
        assert {1e-4, 1e-6} <= set(i.mu) and None in i.mu
    d3 = [i for i in insts if rows(i) == (0, 5, 0, 300, 0)]
    assert d3 and d3[0].n == 300 and any(m is not None and rows(d3[0])[k] == 0 for k, m in enumerate(d3[0].mu))
    assert any(set(rows(i)) == {0} and i.n == 65 for i in insts)
    k257 = [i for i in insts if i.K == 257]
    assert k257 and k257[0].n == 64 and k257[0].mu[256] == 1e-6 and set(rows(k257[0])) == {1, 2, 3}
    assert any(i.K == 513 and i.n == 63 and set(rows(i)) == {1, 2, 3} for i in insts)
    for n in (2, 513):
        assert {(257,), (1, 600)} <= {rows(i) for i in insts if i.n == n}
    for i in insts:                  # the long-double Hessian stays affordable (the 1 + 600 rows at n = 513: 1.6e8)
        assert i.n <= 513 and i.n * i.n * (sum(rows(i)) + 2 * i.K) <= 2 * R.LD_HESS_FLOPS


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


def test_socp_newton_step_coverage():
    """the SOCP Newton entries: two phase-1 steps (one with three diagonal cones), near-boundary
    steps with and without Armijo backtracks, and two steps on which the reference rejects
    candidates in the cone's other nappe -- every barrier-segment slack (cones, bounds) at least
    MARGIN max|s0| while an appended rhs is at most -MARGIN max|s0| -- so that only the sign test of
    rhs in k_ls_cone rejects them; one of the two has a diagonal cone"""
    entries = {e[0]: e for e in R.newton_specs() if R.newton_instance(e).kind == "socp"}
    refs = {tag: R.reference_newton_step(e) for tag, e in entries.items()}
    ph1 = [tag for tag, e in entries.items() if e[2]]
    assert len(ph1) >= 2 and any(sum(a.ndim == 1 for a in R.newton_instance(entries[t]).A) >= 3 for t in ph1)
    near = [tag for tag, e in entries.items() if not e[2] and any(m is not None for m in R.newton_instance(e).mu)]
    assert near and any(refs[t]["k"] > refs[t]["k_feas"] for t in near)
    nappe = {tag: r["nappe"] for tag, r in refs.items() if r["nappe"]}
    print("other-nappe candidates (rejected by the sign of rhs alone): "
          + ", ".join(f"{tag} k = {ks} of {refs[tag]['k_feas']} rejected" for tag, ks in nappe.items()))
    assert {"nappe1", "nappe2"} <= set(nappe)
    assert any(any(a.ndim == 1 for a in R.newton_instance(entries[t]).A) for t in nappe)
    for tag, ks in nappe.items():
        assert max(ks) < refs[tag]["k_feas"] == refs[tag]["k"]


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
