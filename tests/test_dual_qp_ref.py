"""No GPU: the references of the dual-form QP Newton step on a factored P (tests/dual_qp_ref.py) and the host-side
rules of QPSolver(P_factor=..., P_diag=..., linear_solve_method='cholesky_dual').

  * the fp64 restatement of the step stays within a QUARTER of B at every state test_gpu_dual_qp_step.py runs on
    the device (measured over the 1080 states: worst 0.0065 B, at n1-m0-k1-lb-absent-t1-f0.999; without the
    refinement rounds 0.31 B; an fp64 primal Cholesky of the dense H 0.013 B), and the long-double reference
    converges on every state;
  * the oracle's line search is decisive on at least 90 % of the states, and on those the restated step is
    accepted at the oracle's step size;
  * full oracle solves with the restatement and the factored gradient plugged in keep the dense Cholesky oracle's
    iteration lists and its x* within max(1e-6, 4 x the oracle's own spread);
  * the reference-run fixtures dual_qp_factored / dual_qp_diagonal are reproduced at the bars of
    test_gpu_parity.py;
  * ipm_workspace_bytes of IPM_SOLVE_CHOLESKY_DUAL_QP has no n^2 term, every other count is the parent commit's;
  * the facade's argument checks, the class constant, EXPORTS and the header text of constant 9.
"""
import ctypes
import os

import numpy as np
import pytest
import scipy.linalg

import dual_qp_ref as Q
import golden_io
from oracle import ipm_oracle as O

ALPHA, BETA = 0.2, 0.6


def test_states_cover_the_grid():
    st = Q.states()
    assert len(Q.SHAPES) == 12 and len(Q.groups()) == 12 * (4 + 4 + 2)
    assert len(st) == 120 * 9 == len(set(st))
    for n, m, k, b, r, t, f in st[::11]:
        inst = Q.instance(n, m, k, b, r, f)
        fm = inst.oracle(t)
        if fm.constrained:
            assert fm.slacks.min() > 0
        _, Dv = Q.hessian_vectors(fm, inst.rho, t)
        assert Dv.min() > 0
        assert (inst.C is None) == (m == 0) and (inst.F is None) == (k == 0)


def test_restatement_within_a_quarter_of_the_bound():
    worst, where, worst0, worst_c = 0.0, None, 0.0, 0.0
    for s in Q.states():
        ref = Q.reference_step(s)          # (raises if the long-double refinement does not converge)
        inst, t = ref["inst"], s[5]
        fm = inst.oracle(t)
        g = fm.gradient().copy()
        dx = Q.dual_qp_direction(fm, inst.F, inst.rho, t, g)
        assert np.all(np.isfinite(dx)) and np.isfinite(ref["bound"]) and ref["bound"] > 0
        e = float(np.linalg.norm(dx - ref["dx"]) / ref["bound"])
        if e > worst:
            worst, where = e, Q.state_id(s)
        d0 = Q.dual_qp_direction(fm, inst.F, inst.rho, t, g, refine=0)
        worst0 = max(worst0, float(np.linalg.norm(d0 - ref["dx"]) / ref["bound"]))
        H = np.array(fm.hessian(), copy=True)
        dc = scipy.linalg.cho_solve(scipy.linalg.cho_factor(H, check_finite=False), -g, check_finite=False)
        worst_c = max(worst_c, float(np.linalg.norm(dc - ref["dx"]) / ref["bound"]))
    print(f"fp64 restatement: worst err / B {worst:.3g} at {where} over {len(Q.states())} states; 0 rounds "
          f"{worst0:.3g}; fp64 primal Cholesky {worst_c:.3g}")
    assert worst <= 0.25, (worst, where)


@pytest.mark.parametrize("add", [0.0, 1e-9])
def test_restatement_solves_the_same_system(add):
    """dual_qp_direction and a dense solve with the oracle's own hessian() of the host-formed P (psd add on its
    diagonal) agree: D, M and W are restated correctly"""
    for key in ((33, 31, 33, "both", "log", 0.9), (130, 97, 31, "lb", "half0", 0.9), (40, 12, 0, "none", "ones", 0.9),
                (33, 0, 7, "both", "absent", 0.9)):
        inst = Q.instance(*key)
        for t in (1.0, 1e3):
            fm = inst.oracle(t)
            g = fm.gradient().copy()
            H = np.array(fm.hessian(), copy=True)
            H[np.diag_indices(inst.n)] += add
            sol = np.linalg.solve(H, -g)
            dx = Q.dual_qp_direction(fm, inst.F, inst.rho, t, g, add)
            assert np.linalg.norm(dx - sol) <= 1e-9 * np.linalg.norm(sol), (key, t)


def test_line_search_replay_and_decisiveness():
    st = Q.states()
    for s in st[::53]:
        n, m, k, b, r, t, f = s
        inst = Q.instance(n, m, k, b, r, f)
        fm = inst.oracle(t)
        if not fm.constrained:
            continue                   # (the oracle's own backtrack needs slacks)
        ns = O.FeasibleNewton(fm, "cholesky", max_iters=1, eps=1e-5, alpha=ALPHA, beta=BETA)
        ns.solve(inst.x.copy(), t)
        assert ns.trace[0]["step"] == Q.oracle_line_search(s, ALPHA, BETA)["step"]
    decisive = [s for s in st if Q.oracle_line_search(s, ALPHA, BETA)["decisive"]]
    print(f"decisive line searches: {len(decisive)} of {len(st)}")
    assert len(decisive) >= 0.9 * len(st)
    for s in decisive:
        assert Q.restated_line_search(s, ALPHA, BETA)["step"] == Q.oracle_line_search(s, ALPHA, BETA)["step"], \
            Q.state_id(s)


@pytest.mark.parametrize("case", Q.SOLVES, ids=Q.solve_id)
def test_full_oracle_solves_keep_the_trajectory(case):
    ref = Q.solve_reference(case)
    a = ref["solver"]
    b = Q.oracle_qp(ref["dense"], (ref["fac"]["P_factor"], ref["fac"]["P_diag"]))
    xr = float(np.linalg.norm(a.xstar - b.xstar) / np.linalg.norm(a.xstar))
    print(f"[{Q.solve_id(case)}] inner {list(b.inner_iters)} (dense {list(a.inner_iters)}) phase 1 "
          f"{list(a.phase1_iters)} x* rel {xr:.2e}, oracle spread {ref['spread']:.2e}, stable {ref['stable']}")
    assert list(a.phase1_iters) == list(b.phase1_iters)
    # (which cases keep the lists is decided HERE, by the restatement: the GPU test holds the device to the same set)
    assert (list(a.inner_iters) == list(b.inner_iters)) == (Q.solve_id(case) not in Q.NOT_EXACT)
    assert xr <= ref["xbar"]
    assert abs(a.value - b.value) <= 1e-8 * max(1.0, abs(a.value))


@pytest.mark.parametrize("name", ["dual_qp_factored", "dual_qp_diagonal"])
def test_fixtures_at_the_parity_bars(name):
    """the oracle with the restatement on the fixture's factored inputs reaches the reference's own run"""
    z = golden_io.load(name)
    kw = golden_io.solver_kwargs(z)
    F, rho = kw.pop("P_factor", None), kw.pop("P_diag")
    n = len(rho)
    P = F.T @ F if F is not None else np.zeros((n, n))
    P[np.diag_indices(n)] += rho
    s = Q.oracle_qp(dict(kw, P=P), (F, rho))
    xr = float(np.linalg.norm(s.xstar - z["xstar"]) / np.linalg.norm(z["xstar"]))
    vr = abs(s.value - float(z["value"])) / max(1.0, abs(float(z["value"])))
    print(f"[{name}] x* rel {xr:.2e} value rel {vr:.2e} inner {list(s.inner_iters)} (fixture {list(z['inner_iters'])})")
    assert xr <= max(1e-6, 4 * float(z["sens_xstar_rel"]))
    assert vr <= max(1e-8, 4 * float(z["sens_value_rel"]))
    if bool(z["sens_iters_stable"]):
        assert list(s.inner_iters) == list(z["inner_iters"])


# ------------------------------------------------------------------ workspace
def _qp_desc(L, method, n, m, kf=0):
    d = L.ProblemDesc()
    d.kind = L.KIND_QP
    d.solve_method = method
    d.n, d.m, d.ldc, d.ldp = n, m, n, n
    d.q = d.C = d.d = d.lb = d.ub = 1      # non-null markers; only sizes are read
    if method == L.SOLVE_CHOLESKY_DUAL_QP:
        d.Pf, d.ldpf, d.kf, d.Pdiag = 1, n, kf, 1
    else:
        d.P = 1
    return d


def test_workspace_has_no_n_squared_term():
    from ipm355 import _lib as L
    lib = L.load_library()
    n, m, kf = 16384, 256, 128
    dual = lib.ipm_workspace_bytes(ctypes.byref(_qp_desc(L, L.SOLVE_CHOLESKY_DUAL_QP, n, m, kf)))
    chol = lib.ipm_workspace_bytes(ctypes.byref(_qp_desc(L, L.SOLVE_CHOLESKY, n, m)))
    print(f"workspace bytes at n = {n}, m = {m}, kf = {kf}: factored cholesky_dual {dual}, cholesky {chol}")
    assert 0 < dual < 8 * n * n // 16
    assert chol >= 8 * n * n
    dual2 = lib.ipm_workspace_bytes(ctypes.byref(_qp_desc(L, L.SOLVE_CHOLESKY_DUAL_QP, 2 * n, m, kf)))
    assert dual2 <= 2 * dual


# the parent commit's library, recorded before the carve learned about method 9: the dense QP
# (IPM_SOLVE_CHOLESKY, n = 300, m = 40, both bounds), and the LP methods 7 (phase 1) and 8 (p = 64) at that shape
PARENT_QP_CHOLESKY_BYTES = 5191176
PARENT_DUAL_PHASE1_BYTES = 560904
PARENT_DUAL_EQ_BYTES = 635144


def test_every_other_method_keeps_its_byte_count():
    import test_dual_eq_ref as TE
    import test_dual_ph1_ref as T
    from ipm355 import _lib as L
    lib = L.load_library()
    got = {meth: lib.ipm_workspace_bytes(ctypes.byref(TE._desc(L, meth, n=300, m=40)))
           for meth in (L.SOLVE_CHOLESKY, L.SOLVE_LU, L.SOLVE_LSTSQ, L.SOLVE_CG, L.SOLVE_CHOLESKY_DUAL)}
    assert got == T.PARENT_BYTES, got
    eq = lib.ipm_workspace_bytes(ctypes.byref(TE._desc(L, L.SOLVE_CHOLESKY, n=300, m=40, p=64)))
    assert eq == TE.PARENT_EQ_CHOLESKY_BYTES, eq
    ph7 = lib.ipm_workspace_bytes(ctypes.byref(TE._desc(L, L.SOLVE_CHOLESKY_DUAL_PHASE1, n=300, m=40, phase1=1)))
    assert ph7 == PARENT_DUAL_PHASE1_BYTES, ph7
    eq8 = lib.ipm_workspace_bytes(ctypes.byref(TE._desc(L, L.SOLVE_CHOLESKY_DUAL_EQ, n=300, m=40, p=64)))
    assert eq8 == PARENT_DUAL_EQ_BYTES, eq8
    qp = lib.ipm_workspace_bytes(ctypes.byref(_qp_desc(L, L.SOLVE_CHOLESKY, 300, 40)))
    assert qp == PARENT_QP_CHOLESKY_BYTES, qp


# ------------------------------------------------------------------ interface
def test_facade_argument_checks():
    """every rule fires before anything touches the device"""
    from ipm355 import QPSolver
    rng = np.random.default_rng(0)
    n, m, k = 6, 3, 2
    F, rho, q = rng.normal(size=(k, n)), np.ones(n), rng.normal(size=n)
    C, d = rng.normal(size=(m, n)), np.ones(m)
    A, b = rng.normal(size=(2, n)), np.zeros(2)
    kw = dict(q=q, check_cvxpy=False, suppress_print=True, linear_solve_method="cholesky_dual")
    with pytest.raises(ValueError, match="P_factor.*P_diag.*P must be None"):
        QPSolver(P=np.eye(n), P_factor=F, **kw)
    with pytest.raises(ValueError, match="P_factor.*P_diag.*P must be None"):
        QPSolver(P=np.eye(n), P_diag=rho, C=C, d=d, **kw)
    for meth in ("cholesky", "cg", "np_solve", "cholesky_dual_eq", None):
        with pytest.raises(ValueError, match="factored form of P exists for linear_solve_method='cholesky_dual' only"):
            QPSolver(P_factor=F, P_diag=rho, **dict(kw, linear_solve_method=meth))
    with pytest.raises(ValueError, match="P_factor must be 2-dimensional"):
        QPSolver(P_factor=F[0], **kw)
    with pytest.raises(ValueError, match="P_factor must have the same number of columns"):
        QPSolver(P_factor=F[:, :5], **kw)
    for bad in (-1.0, np.nan, np.inf, -rho, np.r_[rho[:-1], np.nan]):
        with pytest.raises(ValueError, match="P_diag must be finite and >= 0"):
            QPSolver(P_factor=F, P_diag=bad, **kw)
    with pytest.raises(ValueError, match="P_diag must be a scalar or an n-vector"):
        QPSolver(P_factor=F, P_diag=np.ones(n + 1), **kw)
    with pytest.raises(ValueError, match="P_diag must be a scalar or an n-vector"):
        QPSolver(P_factor=F, P_diag=np.ones((n, n)), **kw)
    for bad in (None, 0.0, np.r_[0.0, rho[1:]]):
        with pytest.raises(ValueError, match="without a lower or an upper bound need P_diag > 0 everywhere"):
            QPSolver(P_factor=F, P_diag=bad, lower_bound=None, upper_bound=None, **kw)
    with pytest.raises(ValueError, match="does not take equality constraints \\(A must be None\\)"):
        QPSolver(P_factor=F, P_diag=rho, A=A, b=b, **kw)
    with pytest.raises(ValueError, match="Hessian is diagonal and there is nothing to factor"):
        QPSolver(P_diag=rho, **kw)
    # unchanged, pinned by the existing tests too
    with pytest.raises(ValueError, match="Please enter a valid linear solve method!"):
        QPSolver(P=np.eye(n), **kw)
    with pytest.raises(TypeError):
        QPSolver(P=np.eye(n), phase1_linear_solve_method="cholesky_dual", **dict(kw, linear_solve_method="cholesky"))
    with pytest.raises(ValueError, match="just an LP"):
        QPSolver(P=None, **dict(kw, linear_solve_method="cholesky"))


def test_newton_class_constants_exports_and_header():
    import NewtonSolver as flat
    import QPSolver as flat_qp
    from ipm355 import _lib as L
    from ipm355 import newton, problems, solvers
    assert L.SOLVE_CHOLESKY_DUAL_QP == 9
    assert "ipm_gemv_t2" in L.EXPORTS
    names = [f[0] for f in L.ProblemDesc._fields_]
    assert names[-4:] == ["Pf", "ldpf", "kf", "Pdiag"] and names[-5] == "dcone_id_host"
    cls = newton.NewtonSolverCholeskyDualQP
    assert flat.NewtonSolverCholeskyDualQP is cls and flat_qp.QPSolver is solvers.QPSolver
    assert issubclass(cls, newton._NoFallback) and cls.method == "chol_dual_qp" and not cls.infeasible
    assert solvers._solve_method_for(cls) == L.SOLVE_CHOLESKY_DUAL_QP
    assert solvers._solve_method_for(newton.NewtonSolverCholeskyDual) == L.SOLVE_CHOLESKY_DUAL
    assert solvers._solve_method_for(newton.NewtonSolverCholesky) == L.SOLVE_CHOLESKY
    src = open(os.path.join(os.path.dirname(golden_io.GOLDEN), "..", "include", "ipm355.h")).read()
    for text in ("#define IPM_SOLVE_CHOLESKY_DUAL_QP 9", "int ipm_gemv_t2(", "const double* Pf;", "int64_t ldpf;",
                 "int64_t kf;", "const double* Pdiag;", "K = diag(1/W) + M diag(E) M^T"):
        assert text in src, text
    assert src.index("const double* Pf;") > src.index("dcone_id_host;")
    lib = L.load_library()
    assert hasattr(lib, "ipm_gemv_t2") and lib.ipm_version() == 1
    # the generator: the dense P a test forms from a grid instance is exact in fp64
    inst = problems.qp_factor_box(40, 8, 5, seed=2, grid=True, with_xf=True, rho="pow2")
    F, rho = inst["P_factor"], inst["P_diag"]
    P = F.T @ F
    P[np.diag_indices(40)] += rho
    Pl = F.T.astype(np.longdouble) @ F.astype(np.longdouble)
    Pl[np.diag_indices(40)] += rho.astype(np.longdouble)
    assert np.array_equal(P.astype(np.longdouble), Pl)
    assert set(inst) == {"P_factor", "P_diag", "q", "C", "d", "lower_bound", "upper_bound", "xf"}
