"""-m gpu: the level-1 oracle protocol and one Newton step at kernel-edge shapes.

test_gpu_parity.py checks the five device managers against the reference at one tiny fixture
(n = 12, m = 5).  Here the same call sequence runs on seeded instances (tests/barrier_ref.py) whose
shapes place every branch of the slack / gradient GEMVs, the elementwise pieces, the reductions,
the cone kernels and the line-search kernels:
  - LP and QP: entry by entry against a long-double evaluation of the reference's formulas, within
    bounds derived from the 64 eps sum|terms| convention (barrier_ref.py's docstring) -- including
    bound slacks of 1e-6 / 1e-7, where the dense Hessian's epsilon-free bound diagonal and the
    1e-15 of the gradient / diagonal Hessian differ by ~1e-9 relative in single entries;
  - LP phase 1, SOCP and SOCP phase 1: against the fp64 oracle at FN_RTOL = 1e-10 (relative
    norm; every slack is of order one, so no entry dominates);
  - SOCP and SOCP phase 1 again, entry by entry against the long-double socp_reference, on those
    interior instances and on edge ones: cones at 1e-4 and 1e-6 of their boundary (where the fp64
    oracle itself is 1e-8 away in norm, so only bounds that carry the slack's relative error can
    hold a kernel), several diagonal cones, diagonal cones only, K = 257 and 513, n = 2 and 513;
  - one Newton step (IPM_LINESEARCH=compare): the accepted step must equal the oracle's exactly on
    instances where each of the oracle's decisions is at least 1e-9 from flipping.
tests/test_barrier_ref.py (no GPU) holds the oracle itself to a quarter of the same bounds and
checks the decisiveness and the coverage of the Newton-step instances.
"""
import numpy as np
import pytest

import barrier_ref as R

pytestmark = pytest.mark.gpu
FN_RTOL = 1e-10


@pytest.mark.parametrize("spec", R.lpqp_specs(), ids=R.spec_id)
def test_lp_qp_protocol_entrywise(spec):
    """update_x, update_t, slacks, newton_objective, gradient, hessian, then the stale-slack pair
    (Q2), each entry within its derived bound of the long-double reference.  n = 1, 2, 63, 64, 65,
    130: the GEMVs' 64-stride tail only (odd n: the scalar path, even n: the vector path, ld = n);
    513 and 1027: the scalar path past 512 and 1024 columns; 514: the 4-deep loop of gemv_row<true>
    on every lane + lane 0's tail; 900: the 8-deep loop on lanes 0 and 1, the 4-deep on the others;
    1026: 8-deep on every lane + lane 0's tail; 1400: 8-deep once, then tail trips.  m = 1, 5, 255,
    257, 300 and 2049 rows: 1, 1, 16, 17, 19 and 129 row chunks in the gradient's GEMV^T (the
    8-unrolled chunk sum without a tail, with a tail of 1, 3 and 1; one chunk: the tail alone);
    m = 0 (QP): no C kernels at all.  Bounds
    both / lb / ub / none move the slack segments' offsets.  'tiny': 1e-6 / 1e-7 bound slacks.
    'lpdiag': C = None with try_diag, the diagonal Hessian vector and inv_hessian.  The LP / QP
    instances of test_newton_step_matches_reference (S = 1 .. 8257, 'near') are part of the sweep.
    A non-finite device value gives a ratio of inf."""
    inst = R.instance(spec)
    fm = inst.device()
    xv, xs = inst.points(fm)
    vals = R.protocol_values(fm, xv, xs, inst.t, diag=inst.kind == "lpdiag")
    assert vals["slacks"].shape == (inst.S,)
    ratios = R.lpqp_ratios(inst, vals)
    print(f"[{inst.name}] device err / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert R.all_within(ratios, 1.0), ratios


def _norm_check(inst, fm, phase1):
    orc = R.oracle_values(inst, phase1) if inst.kind == "socp" else R.oracle_values(inst)
    if phase1 or inst.kind == "ph1":
        assert abs(fm.s - orc["s"]) <= 1e-12 * abs(orc["s"])
    xv, xs = inst.points(fm, phase1) if inst.kind == "socp" else inst.points(fm)
    vals = R.protocol_values(fm, xv, xs, inst.t)
    rels = {k: R.rel(vals[k], orc[k]) for k in ("slacks", "nobj", "grad", "hess", "stale_nobj", "stale_grad")}
    print(f"[{inst.name}{' phase 1' if phase1 else ''}] device vs oracle, relative norms: "
          + ", ".join(f"{k} {v:.2g}" for k, v in rels.items()))
    assert R.all_within(rels, FN_RTOL), rels


@pytest.mark.parametrize("spec", R.ph1_specs(), ids=R.spec_id)
def test_phase1_protocol(spec):
    """FunctionManagerPhase1 over the same n and m as the LP / QP sweep (the shifted slacks, the
    extra s row and column of the Hessian, sum inv and sum inv^2 reductions over m + 2n elements)"""
    inst = R.instance(spec)
    _norm_check(inst, inst.device(), False)


@pytest.mark.parametrize("phase1", [False, True], ids=["socp", "socp-phase1"])
@pytest.mark.parametrize("spec", R.socp_specs(), ids=R.spec_id)
def test_socp_protocol(spec, phase1):
    """k_cone_slacks strides 256 threads over a cone's rows: dense cones of 1, 255, 256, 257 and 600
    rows (K = 6, with one diagonal cone) and K = 1; n = 130 (vector GEMV) and 257 (scalar); without
    b (lhs = A x), without c (rhs = d) and without d (rhs = c.x); box bounds present"""
    inst = R.socp_instance(spec)
    _norm_check(inst, inst.device(phase1), phase1)


@pytest.mark.parametrize("phase1", [False, True], ids=["socp", "socp-phase1"])
@pytest.mark.parametrize("spec", R.socp_all_specs(), ids=R.spec_id)
def test_socp_protocol_entrywise(spec, phase1):
    """The same call sequence on the SOCP managers, each entry within its derived bound of the
    long-double socp_reference (barrier_ref.py's docstring: every cone coefficient carries its
    slack's relative error rho_i, so the bounds hold, and stay decisive, next to the boundary).
    Besides the four interior instances: cones of 1 .. 600 rows with every other one at
    s = 1e-4 rhs^2 / 1e-6 rhs^2 (n = 130, 257; without c; without d); three diagonal cones between
    dense ones at n = 300 (dslot 0, 1, 2: the dc * n offsets of Ad, bd and the diagonal lhs block,
    the j-loops past 256), one of them near; diagonal cones only (R = 0); K = 257 and 513 cones of
    1 .. 3 rows (the second and third block of k_cone_coef, cone 256 near; 1028 and 2052 rows in
    k_cone_rowweights; the widest k_cone_grows grid); n = 2 and n = 513 under cones of 257 and of 1
    and 600 rows (the column blocks of k_cone_grows, the GEMV paths); the two other-nappe
    instances.  Phase 1 starts both managers at the oracle's s, which the device's must match to
    1e-12.  A non-finite device value gives a ratio of inf."""
    inst = R.socp_instance(spec)
    fm = inst.device(phase1)
    s_orc = R.oracle_values(inst, phase1)["s"]
    if phase1:
        assert abs(fm.s - s_orc) <= 1e-12 * abs(s_orc)
        xv = np.append(inst.x0, s_orc)
        xs = xv + 0.01
    else:
        xv, xs = inst.points(fm)
    vals = R.protocol_values(fm, xv, xs, inst.t)
    assert vals["slacks"].shape == (inst.S,)
    ratios = R.socp_ratios(inst, vals, phase1)
    print(f"[{inst.name}{' phase 1' if phase1 else ''}] device err / bound: "
          + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert R.all_within(ratios, 1.0), ratios


@pytest.mark.parametrize("entry", R.newton_specs(), ids=lambda e: e[0])
def test_newton_step_matches_reference(entry, monkeypatch):
    """One device Newton step (fused gradient path, Cholesky, the 64-candidate table line search
    checked against the exact one: IPM_LINESEARCH=compare) against the oracle's FeasibleNewton from
    the same point.  k_ls_lin takes 64 slacks per workgroup and k_ls_fold sums the workgroups'
    partials in 16 groups of ceil(blocks / 16): S = 1, 63, 64 -> 1 block (a partial one, a full one;
    15 groups empty), 65 -> 2 (the second with one slack), 960 -> 15 full blocks (one per group, the
    last group empty), 1025 / 1088 -> 17 (groups of 2, 2, .., 1, then empty ones: the tail loop
    only), 8257 -> 130 (groups of 9: one 8-unrolled trip plus a tail of 1, a last group of 4); the
    SOCPs run k_ls_cone over cones of 1 .. 600 rows and a diagonal one, in phase 1 too (its shp /
    dshp arm; 'socpDiag3ph1' with three diagonal cones), from cones at 1e-4 / 1e-6 of the boundary
    ('socpNear': the full step; 'socpNearArmijo': 25 Armijo backtracks), and through the cone's
    other nappe ('nappe1' k = 4 .. 10 of 13 rejected, 'nappe2' with a diagonal cone k = 10 .. 12 of
    14: sigma >= 0 with rhs < 0, which only k_ls_cone's sign test of rhs rejects);
    'near97' (beta = 0.97) accepts k = 83: the second 64-candidate pass.  The accepted step must be
    the oracle's bit for bit (both form beta^k by repeated multiplication), the table and the exact
    search must agree, nd to 1e-9, and x to the Cholesky backward-error bound
    64 eps cond2(H) ||step dx|| + 4 eps ||x||.  The library has no exact search for cones
    (IPM_NOT_SUPPORTED), so the SOCPs run the default table search alone: there the table's own
    step is the one held to the oracle's."""
    import ipm355
    tag, spec, phase1, beta = entry
    ref = R.reference_newton_step(entry)
    inst = R.newton_instance(entry)
    compare = inst.kind != "socp"
    monkeypatch.setenv("IPM_LINESEARCH", "compare" if compare else "table")
    fm = inst.device(phase1) if inst.kind == "socp" else inst.device()
    fm.update_t(inst.t)
    ns = ipm355.NewtonSolverCholesky(function_manager=fm, max_iters=1, epsilon=1e-5, alpha=0.2, beta=beta)
    x = ref["x_start"].copy()
    _, _, iters, nd, ok = ns.solve(x, inst.t)
    step = ns.trace[0][0]
    err = float(np.linalg.norm(x - ref["x"]))
    bound = R.x_bound(ref)
    print(f"[{tag}] S {ref['S']} step {step!r} (oracle {ref['step']!r}, k = {ref['k']}), nd {nd!r} vs {ref['nd']!r}, "
          f"|x - x_orc| / bound {err / bound:.3g}, compared {fm.prob.ls_compared} flips {fm.prob.ls_flips}")
    assert iters == 1 and ok == ref["ok"]
    assert step == ref["step"]
    assert (fm.prob.ls_compared, fm.prob.ls_flips) == ((1, 0) if compare else (0, 0))
    assert np.all(np.isfinite(x)) and np.isfinite(nd)
    assert abs(nd - ref["nd"]) <= 1e-9 * abs(ref["nd"])
    assert err <= bound
