"""No GPU: the references of the dual-form Newton step with equality rows (tests/dual_eq_ref.py) and the
host-side rules of linear_solve_method='cholesky_dual_eq'.

  * the fp64 restatement of the step stays within a QUARTER of B = 64 eps cond2(KKT) ||[dx; nu]|| of a
    long-double KKT solve at every state test_gpu_dual_eq_step.py runs on the device (measured over the 270
    states: worst joint error 0.0018 B, at n2-p1-m1-both-t1000-f0; without the refinement rounds 0.065 B;
    the oracle's own Cholesky block elimination 0.0094 B);
  * the oracle's residual line search is decisive on at least 90 % of the states (268 of 270 measured),
    and on those the restated step is accepted at the oracle's step size;
  * short oracle solves with the restatement plugged in keep the Cholesky oracle's iteration lists;
  * the fixtures lp_eq_ineq and lp_npy_miplib are reproduced at the bars of test_gpu_parity.py;
  * ipm_workspace_bytes of IPM_SOLVE_CHOLESKY_DUAL_EQ has no n^2 and no n p term, every other count is
    the parent commit's;
  * the facades' argument checks.
"""
import ctypes
import os

import numpy as np
import pytest

import dual_eq_ref as Q
import golden_io
from oracle import ipm_oracle as O

ALPHA, BETA = 0.2, 0.6


def test_states_cover_the_grid():
    st = Q.states()
    assert len(st) == 10 * 3 * 3 * 3 == 270 == len(set(st))
    for n, p, m, b, t, f in st[::9]:
        inst = Q.instance(n, p, m, b, f)
        assert inst.oracle(t).slacks.min() > 0
        assert inst.A.shape == (p, n) and np.linalg.matrix_rank(inst.A) == p
        # x is not on A x = b unless frac = 0: the step has an equality residual to remove
        assert (np.linalg.norm(inst.A @ inst.x - inst.b) > 0) == (f != 0.0) or p == 0


def test_restatement_within_a_quarter_of_the_bound():
    worst, where, worst0, worst_o = 0.0, None, 0.0, 0.0
    for s in Q.states():
        ref = Q.reference_step(s)
        inst = ref["inst"]
        fm = inst.oracle(s[4])
        g = fm.gradient().copy()
        dx, dv = Q.eq_direction(fm, inst.A, inst.b, inst.x, inst.v, g)
        assert np.all(np.isfinite(dx)) and np.all(np.isfinite(dv)) and np.isfinite(ref["bound"]) and ref["bound"] > 0
        r = Q.joint_error(dx, dv, ref)
        if r > worst:
            worst, where = r, Q.state_id(s)
        worst0 = max(worst0, Q.joint_error(*Q.eq_direction(fm, inst.A, inst.b, inst.x, inst.v, g, refine=0), ref))
        worst_o = max(worst_o, Q.joint_error(*Q.oracle_direction(fm, inst.A, inst.b, inst.x, inst.v, g), ref))
    print(f"fp64 restatement: worst joint err / B {worst:.3g} at {where} over {len(Q.states())} states; "
          f"0 rounds {worst0:.3g}; the oracle's Cholesky block elimination {worst_o:.3g}")
    assert worst <= 0.25, (worst, where)


@pytest.mark.parametrize("add", [0.0, 1e-9])
def test_restatement_solves_the_same_system(add):
    """eq_direction and a dense solve of [[H, A^T], [A, 0]] with the oracle's own hessian() (psd add on its
    diagonal) agree: the elimination is restated correctly"""
    inst = Q.instance(33, 1, 31, "both", 0.9)
    for inst in (inst, Q.instance(130, 30, 97, "lb", 0.9)):
        fm = inst.oracle(1e3)
        g = fm.gradient().copy()
        H = np.array(fm.hessian(), copy=True)
        H[np.diag_indices(inst.n)] += add
        p = inst.p
        KKT = np.block([[H, inst.A.T], [inst.A, np.zeros((p, p))]])
        sol = np.linalg.solve(KKT, -np.concatenate([g, inst.A @ inst.x - inst.b]))
        dx, dv = Q.eq_direction(fm, inst.A, inst.b, inst.x, inst.v, g, add)
        got = np.concatenate([dx, inst.v + dv])
        assert np.linalg.norm(got - sol) <= 1e-9 * np.linalg.norm(sol)


def test_line_search_replay_and_decisiveness():
    """the replay returns the step the oracle's own solve takes; at least 90 % of the states are decisive
    for the oracle alone (the cap of the GPU test's step-size comparison), and on those the restated step is
    accepted at the oracle's step size"""
    st = Q.states()
    for s in st[::37]:
        inst = Q.instance(s[0], s[1], s[2], s[3], s[5])
        ns = O.InfeasibleNewton(inst.A, inst.b, inst.oracle(s[4]), "cholesky", max_iters=1, eps=1e-5, alpha=ALPHA,
                                beta=BETA)
        ns.solve(inst.x.copy(), s[4], v0=inst.v.copy())
        assert ns.trace[0]["step"] == Q.oracle_line_search(s, ALPHA, BETA)["step"]
    decisive = [s for s in st if Q.oracle_line_search(s, ALPHA, BETA)["decisive"]]
    print(f"decisive residual line searches: {len(decisive)} of {len(st)}")
    assert len(decisive) >= 0.9 * len(st)
    for s in decisive:
        assert Q.restated_line_search(s, ALPHA, BETA)["step"] == Q.oracle_line_search(s, ALPHA, BETA)["step"], \
            Q.state_id(s)


@pytest.mark.parametrize("shape", Q.SOLVE_SHAPES, ids=lambda s: "n%d-p%d-m%d" % s)
def test_short_oracle_solves_keep_the_trajectory(shape):
    """four barrier iterations (max_outer_iters limits only the barrier loop): iteration lists equal, x* within
    4 x the oracle's own spread under 1e-15 relative input perturbations (or 1e-9)"""
    ref = Q.short_reference(shape)
    a = ref["solver"]
    b = Q.oracle_lp(Q.copy_kw(ref["kw"]), True, max_outer_iters=Q.SHORT_OUTER)
    xr = float(np.linalg.norm(a.xstar - b.xstar) / np.linalg.norm(a.xstar))
    print(f"[{shape}] inner {list(b.inner_iters)} (cholesky {list(a.inner_iters)}) x* rel {xr:.2e}, oracle spread "
          f"{ref['spread']:.2e}, oracle lists stable under the perturbation: {ref['stable']}")
    assert list(a.phase1_iters) == list(b.phase1_iters)
    assert list(a.inner_iters) == list(b.inner_iters)
    assert xr <= ref["xbar"]


@pytest.mark.parametrize("name", ["lp_eq_ineq", "lp_npy_miplib"])
def test_fixtures_at_the_parity_bars(name):
    z = golden_io.load(name)
    kw = golden_io.solver_kwargs(z)
    kw["x0"] = z["x_init"].copy()
    s = Q.oracle_lp(kw, True)
    xr = float(np.linalg.norm(s.xstar - z["xstar"]) / np.linalg.norm(z["xstar"]))
    vr = abs(s.value - float(z["value"])) / max(1.0, abs(float(z["value"])))
    print(f"[{name}] x* rel {xr:.2e} value rel {vr:.2e} inner {list(s.inner_iters)} (fixture {list(z['inner_iters'])})")
    assert xr <= max(1e-6, 4 * float(z["sens_xstar_rel"]))
    assert vr <= max(1e-8, 4 * float(z["sens_value_rel"]))


# ------------------------------------------------------------------ workspace
def _desc(L, method, n=16384, m=256, p=0, phase1=0, **kw):
    d = L.ProblemDesc()
    d.kind = L.KIND_LP
    d.solve_method = method
    d.phase1 = phase1
    d.n, d.m, d.ldc = n, m, n
    d.c = d.C = d.d = d.lb = d.ub = 1      # non-null markers; only sizes are read
    if p:
        d.p, d.lda = p, n
        d.A = d.AT = d.b = 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_workspace_has_no_n_squared_and_no_n_p_term():
    from ipm355 import _lib as L
    lib = L.load_library()
    n, m, p = 16384, 256, 128
    dual = lib.ipm_workspace_bytes(ctypes.byref(_desc(L, L.SOLVE_CHOLESKY_DUAL_EQ, n, m, p)))
    chol = lib.ipm_workspace_bytes(ctypes.byref(_desc(L, L.SOLVE_CHOLESKY, n, m, p)))
    print(f"workspace bytes at n = {n}, m = {m}, p = {p}: cholesky_dual_eq {dual}, cholesky {chol}")
    assert 0 < dual < 8 * n * n // 16
    assert chol >= 8 * n * n + 8 * n * p
    dual2 = lib.ipm_workspace_bytes(ctypes.byref(_desc(L, L.SOLVE_CHOLESKY_DUAL_EQ, 2 * n, m, p, ldc=2 * n)))
    assert dual2 <= 2 * dual


# LP n = 300, m = 40, p = 64, both bounds, IPM_SOLVE_CHOLESKY: the parent commit's library, recorded before the
# carve learned about method 8
PARENT_EQ_CHOLESKY_BYTES = 4486920


def test_every_other_method_keeps_its_byte_count():
    import test_dual_ph1_ref as T
    from ipm355 import _lib as L
    lib = L.load_library()
    got = {meth: lib.ipm_workspace_bytes(ctypes.byref(_desc(L, meth, n=300, m=40)))
           for meth in (L.SOLVE_CHOLESKY, L.SOLVE_LU, L.SOLVE_LSTSQ, L.SOLVE_CG, L.SOLVE_CHOLESKY_DUAL)}
    assert got == T.PARENT_BYTES, got
    ph1 = lib.ipm_workspace_bytes(ctypes.byref(_desc(L, L.SOLVE_CHOLESKY, n=300, m=40, phase1=1)))
    assert ph1 == T.PARENT_PHASE1_CHOLESKY_BYTES, ph1
    eq = lib.ipm_workspace_bytes(ctypes.byref(_desc(L, L.SOLVE_CHOLESKY, n=300, m=40, p=64)))
    assert eq == PARENT_EQ_CHOLESKY_BYTES, eq


# ------------------------------------------------------------------ interface
def test_facade_argument_checks():
    """every check fires before anything touches the device"""
    from ipm355 import LPSolver, QPSolver
    rng = np.random.default_rng(0)
    n, m = 6, 3
    C, d, c = rng.normal(size=(m, n)), np.ones(m), rng.normal(size=n)
    A, b = rng.normal(size=(2, n)), np.zeros(2)
    kw = dict(check_cvxpy=False, suppress_print=True, linear_solve_method="cholesky_dual_eq")
    with pytest.raises(ValueError, match="cholesky_dual_eq.*'cholesky_dual'"):
        LPSolver(c=c, C=C, d=d, lower_bound=-3, upper_bound=3, **kw)
    with pytest.raises(ValueError, match="cholesky_dual_eq.*inequality"):
        LPSolver(c=c, A=A, b=b, lower_bound=-3, upper_bound=3, **kw)
    with pytest.raises(ValueError, match="cholesky_dual_eq.*bound"):
        LPSolver(c=c, A=A, b=b, C=C, d=d, lower_bound=None, upper_bound=None, **kw)
    # 'cholesky_dual' keeps refusing equality rows, in its own words
    with pytest.raises(ValueError, match="cholesky_dual' is a feasible-start method.*A must be None"):
        LPSolver(c=c, A=A, b=b, C=C, d=d, lower_bound=-3, upper_bound=3,
                 **dict(kw, linear_solve_method="cholesky_dual"))
    # QPSolver does not know the method, with or without equality rows (no C: nothing touches the device
    # before the dispatch; SOCPSolver builds its cones on the device first: test_gpu_dual_eq_solve.py)
    with pytest.raises(ValueError, match="Please enter a valid linear solve method!"):
        QPSolver(P=np.eye(n), q=c, **kw)
    with pytest.raises(ValueError, match="Please enter a valid linear solve method!"):
        QPSolver(P=np.eye(n), q=c, A=A, b=b, **kw)


def test_newton_class_constants_and_header():
    import NewtonSolverInfeasibleStart as flat
    from ipm355 import _lib as L
    from ipm355 import newton, solvers
    assert L.SOLVE_CHOLESKY_DUAL_EQ == 8
    assert "ipm_syrk_nt2" in L.EXPORTS and "ipm_fm_last_dual_direction" in L.EXPORTS
    cls = newton.NewtonSolverCholeskyDualInfeasibleStart
    assert flat.NewtonSolverCholeskyDualInfeasibleStart is cls
    assert issubclass(cls, newton.NewtonSolverInfeasibleStart) and cls.method == "chol_dual_eq" and cls.infeasible
    assert solvers._solve_method_for(cls) == L.SOLVE_CHOLESKY_DUAL_EQ
    assert solvers._solve_method_for(newton.NewtonSolverCholeskyDual) == L.SOLVE_CHOLESKY_DUAL
    assert solvers._solve_method_for(newton.NewtonSolverCholeskyInfeasibleStart) == L.SOLVE_CHOLESKY
    src = open(os.path.join(os.path.dirname(golden_io.GOLDEN), "..", "include", "ipm355.h")).read()
    for text in ("#define IPM_SOLVE_CHOLESKY_DUAL_EQ 8", "int ipm_syrk_nt2(", "int ipm_fm_last_dual_direction("):
        assert text in src, text
    lib = L.load_library()
    assert hasattr(lib, "ipm_syrk_nt2") and hasattr(lib, "ipm_fm_last_dual_direction")
