"""The dual-form phase-1 Newton step on the CPU (no GPU needed):
  * the fp64 restatement of the device's step stays within a quarter of B1 = 64 eps cond2(H~) ||d|| of a
    long-double solve at every state of the GPU test;
  * it solves the system of the oracle's Phase1Barrier.hessian(), with and without the psd add;
  * the oracle's PhaseOne with the restated direction keeps the Cholesky oracle's iteration lists, on the
    reference-run fixtures and on generated instances; full solves with both phases restated keep every list;
  * the oracle's own line search is decisive at nearly every state (the GPU test compares step sizes);
  * ipm_workspace_bytes of IPM_SOLVE_CHOLESKY_DUAL_PHASE1 has no n^2 term, every other count is unchanged;
  * the facades' argument checks.
"""
import ctypes
import os

import numpy as np
import pytest

import dual_ph1_ref as P
import golden_io


def test_states_cover_the_grid():
    st = P.states()
    assert len(st) == 11 * 3 * 3 * 2 * 2 == len(set(st))
    for n, m, b, t, f, dl in st:
        pt = P.point(n, m, b, f, dl)
        fm = pt.oracle(t)
        # inside the phase-1 domain, exactly delta from its boundary (up to the rounding of s)
        assert fm.slacks.min() > 0 and abs(fm.slacks.min() - dl) <= 1e-9 * max(1.0, abs(pt.s))
        s0 = fm.slacks - pt.s
        assert (s0.min() < 0) == (f == 1.5)      # frac = 1.5 is infeasible: phase 1 has work to do


def test_restatement_within_a_quarter_of_the_bound():
    worst, where = 0.0, None
    for s in P.states():
        ref = P.reference_step(s)
        fm = ref["pt"].oracle(s[3])
        d = P.dual_phase1_direction(fm, fm.gradient().copy())
        assert np.all(np.isfinite(d)) and np.isfinite(ref["bound"]) and ref["bound"] > 0
        r = float(np.linalg.norm(d - ref["d"]) / ref["bound"])
        if r > worst:
            worst, where = r, P.state_id(s)
    print(f"fp64 restatement: worst err / B1 {worst:.3g} at {where} over {len(P.states())} states")
    assert worst <= 0.25, (worst, where)


@pytest.mark.parametrize("add", [0.0, 1e-9])
@pytest.mark.parametrize("bounds", list(P.BOUNDS))
def test_restatement_solves_the_same_system(add, bounds):
    """dual_phase1_direction and a dense solve of the oracle's own Phase1Barrier.hessian() (psd add on
    its whole diagonal, as NewtonSolver.py:269-275 adds it) agree: the elimination is restated correctly"""
    pt = P.point(33, 31, bounds, 1.5, 1.0)
    fm = pt.oracle(1.0)
    g = fm.gradient().copy()
    H = np.array(fm.hessian(), copy=True)
    H[np.diag_indices(len(g))] += add
    d = np.linalg.solve(H, -g)
    got = P.dual_phase1_direction(fm, g, add)
    assert np.linalg.norm(got - d) <= 1e-9 * np.linalg.norm(d)
    w, Dv, h, hss = P.hessian_pieces(fm, add)
    np.testing.assert_allclose(H[:-1, -1], h, rtol=1e-13, atol=1e-13 * np.abs(h).max())
    np.testing.assert_allclose(H[-1, -1], hss, rtol=1e-14)
    np.testing.assert_allclose(np.diag(H)[:-1], Dv + np.einsum("ij,i,ij->j", fm.C, w, fm.C), rtol=1e-12)


def test_line_search_replay_and_decisiveness():
    """the replay of the oracle's backtracking returns the step its own solve takes, and at least 90 % of
    the states are decisive (margins >= 1e-9): the GPU test's step-size assertion is not vacuous"""
    from oracle import ipm_oracle as O
    st = P.states()
    for s in st[::41]:
        pt = P.point(s[0], s[1], s[2], s[4], s[5])
        ns = O.FeasibleNewton(pt.oracle(s[3]), max_iters=1, eps=1e-5, alpha=0.2, beta=0.6, phase1=True, phase1_tol=0.1)
        ns.solve(pt.x.copy(), s[3])
        assert ns.trace[0]["step"] == P.oracle_line_search(s)["step"]
    decisive = sum(P.oracle_line_search(s)["decisive"] for s in st)
    print(f"decisive line searches: {decisive} of {len(st)}")
    assert decisive >= 0.9 * len(st)


# ------------------------------------------------------------------ trajectories
def _fixture_kw(name):
    z = golden_io.load(name)
    kw = golden_io.solver_kwargs(z)
    kw = {k: (v.item() if isinstance(v, np.ndarray) and v.ndim == 0 else v) for k, v in kw.items()}
    kw.pop("linear_solve_method", None)
    if "x_init" in z:
        kw["x0"] = z["x_init"].copy()
    return z, kw


FIXTURE_LISTS = {"lp_ineq_box": [30, 21, 21, 19, 2], "lp_ineq_box_duals": [30, 21, 21, 19, 2],
                 "lp_ineq_box_testkw": [29, 2, 22, 2, 1]}


@pytest.mark.parametrize("name", list(FIXTURE_LISTS) + ["cg_lp_n40"])
def test_phase_one_keeps_the_fixture_lists(name):
    z, kw = _fixture_kw(name)
    a = P.oracle_phase_one(kw, False)
    b = P.oracle_phase_one(kw, True)
    xr = float(np.linalg.norm(a.phase1.x - b.phase1.x) / np.linalg.norm(a.phase1.x))
    print(f"[{name}] phase 1 inner {b.phase1.inner_iters} (cholesky {a.phase1.inner_iters}) exit x~ rel {xr:.2e}")
    assert list(b.phase1.inner_iters) == list(a.phase1.inner_iters)
    if name in FIXTURE_LISTS:
        assert list(b.phase1.inner_iters) == FIXTURE_LISTS[name] == list(z["phase1_inner_iters"])
    else:
        assert list(b.phase1.inner_iters) == [27, 19, 19, 2]
    assert xr <= 1e-8


GEN_SHAPES = [(1, 1), (2, 1), (17, 15), (64, 63), (65, 64), (130, 127), (129, 128), (257, 129), (300, 40),
              (200, 150), (1024, 256)]
GEN_BOUNDS = {"both": (-3, 3), "lb": (-3, None), "ub": (None, 3)}
GEN = [(n, m, b) for (n, m) in GEN_SHAPES for b in GEN_BOUNDS if not (n == 1024 and b == "ub")]


def generated_kw(n, m, bounds):
    from ipm355 import problems
    lo, hi = GEN_BOUNDS[bounds]
    return dict(problems.lp_ineq_box(n, m, seed=11), **problems.LP_KWARGS, lower_bound=lo, upper_bound=hi)


@pytest.mark.parametrize("case", GEN, ids=lambda c: f"n{c[0]}-m{c[1]}-{c[2]}")
def test_phase_one_keeps_the_list_on_generated_instances(case):
    """problems.lp_ineq_box(n, m, seed=11) with LP_KWARGS and one of three bound sets: the phase-1
    iteration list equals the Cholesky oracle's, the exit point agrees (single-bound cases, where s runs
    to about -1e5, were at 2.6e-9 when the scheme was proposed; 1e-11 with both bounds)"""
    kw = generated_kw(*case)
    a = P.oracle_phase_one(kw, False)
    b = P.oracle_phase_one(kw, True)
    xr = float(np.linalg.norm(a.phase1.x - b.phase1.x) / np.linalg.norm(a.phase1.x))
    print(f"[{case}] phase 1 inner {b.phase1.inner_iters} exit x~ rel {xr:.2e}")
    assert list(b.phase1.inner_iters) == list(a.phase1.inner_iters)
    assert xr <= (1e-10 if case[2] == "both" else 2.6e-8)


@pytest.mark.parametrize("shape", [(130, 127), (200, 150), (1024, 256)], ids=lambda s: f"n{s[0]}-m{s[1]}")
def test_full_solves_with_both_phases_restated(shape):
    kw = generated_kw(*shape, "both")
    a = P.oracle_lp(kw, False)
    b = P.oracle_lp(kw, True)
    xr = float(np.linalg.norm(a.xstar - b.xstar) / np.linalg.norm(a.xstar))
    print(f"[{shape}] phase 1 {b.phase1_iters} inner {b.inner_iters} x* rel {xr:.2e}")
    assert list(b.phase1_iters) == list(a.phase1_iters) and len(a.phase1_iters) > 0
    assert list(b.inner_iters) == list(a.inner_iters) and b.outer_iters == a.outer_iters
    assert xr <= 6e-11


# ------------------------------------------------------------------ workspace
def _desc(L, method, n=16384, m=256, phase1=0, **kw):
    d = L.ProblemDesc()
    d.kind = L.KIND_LP
    d.solve_method = method
    d.phase1 = phase1
    d.n, d.m, d.ldc = n, m, n
    d.c = d.C = d.d = d.lb = d.ub = 1      # non-null markers; only sizes are read
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_workspace_has_no_n_squared_term():
    from ipm355 import _lib as L
    lib = L.load_library()
    n = 16384
    dual = lib.ipm_workspace_bytes(ctypes.byref(_desc(L, L.SOLVE_CHOLESKY_DUAL_PHASE1, phase1=1)))
    chol = lib.ipm_workspace_bytes(ctypes.byref(_desc(L, L.SOLVE_CHOLESKY, phase1=1)))
    print(f"phase-1 workspace bytes at n = {n}, m = 256: dual {dual}, cholesky {chol}")
    assert 0 < dual < 8 * n * n // 16
    assert chol >= 8 * n * n
    dual2 = lib.ipm_workspace_bytes(ctypes.byref(_desc(L, L.SOLVE_CHOLESKY_DUAL_PHASE1, n=2 * n, ldc=2 * n, phase1=1)))
    assert dual2 <= 2 * dual


# the byte counts of the parent commit's library at LP n = 300, m = 40, both bounds: cholesky, LU, lstsq,
# cg, cholesky_dual -- and of the phase-1 Cholesky problem at the same sizes
PARENT_BYTES = {0: 5191176, 2: 4137992, 3: 5191176, 5: 832776, 6: 545032}
PARENT_PHASE1_CHOLESKY_BYTES = 5198344


def test_every_other_method_keeps_its_byte_count():
    from ipm355 import _lib as L
    lib = L.load_library()
    got = {meth: lib.ipm_workspace_bytes(ctypes.byref(_desc(L, meth, n=300, m=40, ldc=300)))
           for meth in (L.SOLVE_CHOLESKY, L.SOLVE_LU, L.SOLVE_LSTSQ, L.SOLVE_CG, L.SOLVE_CHOLESKY_DUAL)}
    assert got == PARENT_BYTES, got
    ph1 = lib.ipm_workspace_bytes(ctypes.byref(_desc(L, L.SOLVE_CHOLESKY, n=300, m=40, ldc=300, phase1=1)))
    assert ph1 == PARENT_PHASE1_CHOLESKY_BYTES, ph1


# ------------------------------------------------------------------ interface
def test_facade_argument_checks():
    """every check fires before anything touches the device"""
    from ipm355 import LPSolver, PhaseOneSolver, QPSolver, SOCPSolver
    rng = np.random.default_rng(0)
    n, m = 6, 3
    C, d, c = rng.normal(size=(m, n)), np.ones(m), rng.normal(size=n)
    kw = dict(check_cvxpy=False, suppress_print=True)
    with pytest.raises(ValueError, match="phase1_linear_solve_method.*inequality"):
        LPSolver(c=c, lower_bound=-3, upper_bound=3, phase1_linear_solve_method="cholesky_dual", **kw)
    with pytest.raises(ValueError, match="phase1_linear_solve_method.*bound"):
        LPSolver(c=c, C=C, d=d, lower_bound=None, upper_bound=None, phase1_linear_solve_method="cholesky_dual", **kw)
    for bad in ("cholesky", "np_solve", "dual", 7):
        with pytest.raises(ValueError, match="Please enter a valid linear solve method!"):
            LPSolver(c=c, C=C, d=d, lower_bound=-3, upper_bound=3, phase1_linear_solve_method=bad, **kw)
    for cls, args in ((QPSolver, dict(P=np.eye(n), q=c)), (SOCPSolver, dict(q=c))):
        with pytest.raises(TypeError, match="phase1_linear_solve_method"):
            cls(phase1_linear_solve_method="cholesky_dual", **args, **kw)
    with pytest.raises(ValueError, match="cholesky_dual.*socp"):
        PhaseOneSolver(socp=True, socp_params=(None, None, None, None), x0=np.zeros(n),
                       linear_solve_method="cholesky_dual")


def test_method_constant_and_plumbing():
    import inspect

    import FunctionManager as flat_fm
    import PhaseOneSolver as flat_p1
    from ipm355 import _lib as L
    from ipm355 import function_manager, newton, phase_one, solvers
    assert L.SOLVE_CHOLESKY_DUAL_PHASE1 == 7 and L.SOLVE_CHOLESKY_DUAL == 6
    assert "ipm_gemv_2v" in L.EXPORTS
    # the barrier phase's class keeps method 6; the phase-1 manager picks 7 itself
    assert solvers._solve_method_for(newton.NewtonSolverCholeskyDual) == L.SOLVE_CHOLESKY_DUAL
    sig = inspect.signature(function_manager.FunctionManagerPhase1.__init__)
    assert sig.parameters["solve_method"].default == L.SOLVE_CHOLESKY
    sig = inspect.signature(solvers.LPSolver.__init__)
    assert sig.parameters["phase1_linear_solve_method"].default is None
    assert sig.parameters["phase1_linear_solve_method"].kind is inspect.Parameter.KEYWORD_ONLY
    assert flat_p1.PhaseOneSolver is phase_one.PhaseOneSolver
    assert flat_fm.FunctionManagerPhase1 is function_manager.FunctionManagerPhase1
    src = open(os.path.join(os.path.dirname(golden_io.GOLDEN), "..", "include", "ipm355.h")).read()
    assert "#define IPM_SOLVE_CHOLESKY_DUAL_PHASE1 7" in src and "#define IPM_SOLVE_CHOLESKY_DUAL 6" in src
    assert "int ipm_gemv_2v(" in src
    lib = L.load_library()
    # ipm_workspace_bytes only sizes: method 7 has a byte count with phase1 = 1 and, like any descriptor,
    # without it (that form is rejected by ipm_problem_create, which needs a device)
    for ph1 in (1, 0):
        assert lib.ipm_workspace_bytes(ctypes.byref(_desc(L, 7, n=300, m=40, ldc=300, phase1=ph1))) > 0
