"""CPU: the factored QP with equality rows (linear_solve_method='cholesky_dual_eq' with P_factor / P_diag,
IPM_SOLVE_CHOLESKY_DUAL_QP_EQ) -- the fp64 restatement of the device's step (tests/dual_qp_eq_ref.py) against a
long-double solve of the KKT system, the oracle's residual line search on it, and the interface.

  * every state of the grid: the restatement's [dx; nu] within B / 4 of the long-double reference with three
    refinement rounds (B = 64 eps cond2(KKT) ||[dx; nu]||); the figure without refinement and the oracle's own
    Cholesky block elimination are reported beside it;
  * on the states the oracle's residual line search decides on (every decision at least 1e-9 from flipping, the
    step floor not reached) the restated step is accepted at the oracle's step size; at most 2 % of the states are
    undecided, asserted;
  * the facade's rules with their pinned messages, the constant, the exports, the header text, the Newton class
    and its flat re-export, the create-time rejections' reasons in the library's method table;
  * ipm_workspace_bytes of methods 0 .. 9 on a fixed set of descriptors equals the parent commit's library, and
    method 10 has no n^2 and no n p term;
  * the restatement plugged into the oracle's QP solve on five generated instances against the oracle's own
    Cholesky block elimination.
"""
import ctypes
import os

import numpy as np
import pytest

import dual_qp_eq_ref as R
import golden_io

GROUPS = R.groups()


# ------------------------------------------------------------------ the step
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "n%d-m%d-k%d-p%d-%s-%s" % g)
def test_restatement_is_within_a_quarter_of_the_bound(group):
    worst3 = worst0 = worst_o = 0.0
    for t in R.TS:
        for frac in R.FRACS:
            state = group + (t, frac)
            ref = R.reference_step(state)
            inst = ref["inst"]
            fm = inst.oracle(t)
            g = ref["g"]
            dx, dv = R.qe_direction(fm, inst.F, inst.rho, inst.A, inst.b, inst.x, inst.v, t, g)
            e3 = R.joint_error(dx, dv, ref)
            dx0, dv0 = R.qe_direction(fm, inst.F, inst.rho, inst.A, inst.b, inst.x, inst.v, t, g, refine=0)
            e0 = R.joint_error(dx0, dv0, ref)
            try:
                dxo, dvo = R.oracle_direction(fm, inst.A, inst.b, inst.x, inst.v, g)
                eo = R.joint_error(np.asarray(dxo), np.asarray(dvo), ref)
            except np.linalg.LinAlgError:
                eo = np.inf
            worst3, worst0, worst_o = max(worst3, e3), max(worst0, e0), max(worst_o, eo)
            assert e3 <= 0.25, (R.state_id(state), e3, ref["cond2"])
    print(f"[{group}] worst err / B: restatement {worst3:.3g} (0 rounds {worst0:.3g}), oracle block elimination "
          f"{worst_o:.3g}")


def test_restated_step_is_accepted_at_the_oracle_s_step_size():
    states = R.states()
    undecided, checked = [], 0
    for s in states:
        o = R.oracle_line_search(s)
        if not o["decisive"]:
            undecided.append(R.state_id(s))
            continue
        r = R.restated_line_search(s)
        checked += 1
        assert r["step"] == o["step"], (R.state_id(s), r["step"], o["step"], o["feas_margin"], o["res_margin"])
    share = len(undecided) / len(states)
    print(f"line search: {checked} of {len(states)} states decided, {len(undecided)} undecided ({share:.2%}): "
          f"{undecided}")
    assert share <= R.UNDECIDED_CAP, (len(undecided), len(states))


# ------------------------------------------------------------------ workspace
def _lp_desc(L, method, n=300, m=40, p=0, phase1=0):
    d = L.ProblemDesc()
    d.kind, d.solve_method, d.phase1 = L.KIND_LP, method, phase1
    d.n, d.m, d.ldc = n, m, n
    d.c = d.C = d.d = d.lb = d.ub = 1      # non-null markers; only sizes are read
    if p:
        d.p, d.lda = p, n
        d.A = d.AT = d.b = 1
    return d


def _qp_desc(L, method, n=300, m=40, kf=0, p=0):
    d = L.ProblemDesc()
    d.kind, d.solve_method = L.KIND_QP, method
    d.n, d.m, d.ldc, d.ldp = n, m, n, n
    d.q = d.C = d.d = d.lb = d.ub = 1
    if method in (L.SOLVE_CHOLESKY_DUAL_QP, L.SOLVE_CHOLESKY_DUAL_QP_EQ):
        d.Pf, d.ldpf, d.kf, d.Pdiag = 1, n, kf, 1
    else:
        d.P = 1
    if p:
        d.p, d.lda = p, n
        d.A = d.AT = d.b = 1
    return d


# the parent commit's library at n = 300, m = 40 (p = 64, kf = 24 where present), both bounds: recorded before the
# carve learned about method 10.  lp0, lp2, lp3, lp5, lp6, lp0_ph1, lp7_ph1, lp0_eq, lp8_eq and qp0 are the figures
# test_dual_ph1_ref.py, test_dual_eq_ref.py and test_dual_qp_ref.py record.
PARENT_BYTES = {
    "lp0": 5191176, "lp1": 2171656, "lp2": 4137992, "lp3": 5191176, "lp4": 2171656, "lp5": 832776, "lp6": 545032,
    "lp0_ph1": 5198344, "lp7_ph1": 560904,
    "lp0_eq": 4486920, "lp1_eq": 2520584, "lp2_eq": 4486920, "lp3_eq": 5758472, "lp4_eq": 2554888, "lp8_eq": 635144,
    "qp0": 5191176, "qp2": 4137992, "qp3": 5191176, "qp5": 832776,
    "qp0_eq": 4486920, "qp2_eq": 4486920, "qp3_eq": 5758472, "qp9": 576264, "qp9_k0": 547848}


def test_every_other_method_keeps_its_byte_count():
    import test_dual_eq_ref as TE
    import test_dual_ph1_ref as TP
    import test_dual_qp_ref as TQ
    from ipm355 import _lib as L
    lib = L.load_library()
    B = lambda d: lib.ipm_workspace_bytes(ctypes.byref(d))
    got = {f"lp{meth}": B(_lp_desc(L, meth)) for meth in (0, 1, 2, 3, 4, 5, 6)}
    got["lp0_ph1"] = B(_lp_desc(L, 0, phase1=1))
    got["lp7_ph1"] = B(_lp_desc(L, 7, phase1=1))
    got.update({f"lp{meth}_eq": B(_lp_desc(L, meth, p=64)) for meth in (0, 1, 2, 3, 4, 8)})
    got.update({f"qp{meth}": B(_qp_desc(L, meth)) for meth in (0, 2, 3, 5)})
    got.update({f"qp{meth}_eq": B(_qp_desc(L, meth, p=64)) for meth in (0, 2, 3)})
    got["qp9"] = B(_qp_desc(L, 9, kf=24))
    got["qp9_k0"] = B(_qp_desc(L, 9, kf=0))
    assert got == PARENT_BYTES, {k: (v, PARENT_BYTES[k]) for k, v in got.items() if v != PARENT_BYTES[k]}
    # the figures the sibling tests record are among them
    assert {m: got[f"lp{m}"] for m in TP.PARENT_BYTES} == TP.PARENT_BYTES
    assert got["lp0_ph1"] == TP.PARENT_PHASE1_CHOLESKY_BYTES and got["lp0_eq"] == TE.PARENT_EQ_CHOLESKY_BYTES
    assert got["lp7_ph1"] == TQ.PARENT_DUAL_PHASE1_BYTES and got["lp8_eq"] == TQ.PARENT_DUAL_EQ_BYTES
    assert got["qp0"] == TQ.PARENT_QP_CHOLESKY_BYTES


def test_workspace_has_no_n_squared_and_no_n_p_term():
    from ipm355 import _lib as L
    lib = L.load_library()
    n, m, kf, p = 16384, 256, 128, 128
    dual = lib.ipm_workspace_bytes(ctypes.byref(_qp_desc(L, L.SOLVE_CHOLESKY_DUAL_QP_EQ, n, m, kf, p)))
    chol = lib.ipm_workspace_bytes(ctypes.byref(_qp_desc(L, L.SOLVE_CHOLESKY, n, m, p=p)))
    print(f"workspace bytes at n = {n}, m = {m}, kf = {kf}, p = {p}: factored cholesky_dual_eq {dual}, cholesky {chol}")
    assert 0 < dual < 8 * n * n // 16
    assert chol >= 8 * n * n + 8 * n * p
    dual2 = lib.ipm_workspace_bytes(ctypes.byref(_qp_desc(L, L.SOLVE_CHOLESKY_DUAL_QP_EQ, 2 * n, m, kf, p)))
    dualp = lib.ipm_workspace_bytes(ctypes.byref(_qp_desc(L, L.SOLVE_CHOLESKY_DUAL_QP_EQ, n, m, kf, 2 * p)))
    assert dual2 <= 2 * dual and dualp - dual < 8 * n * p // 4


# ------------------------------------------------------------------ interface
def test_facade_argument_checks():
    """every rule fires before anything touches the device (no C: no phase-1 problem is built)"""
    from ipm355 import QPSolver
    rng = np.random.default_rng(0)
    n, k = 6, 2
    F, rho, q = rng.normal(size=(k, n)), np.ones(n), rng.normal(size=n)
    A, b = rng.normal(size=(2, n)), np.zeros(2)
    kw = dict(q=q, check_cvxpy=False, suppress_print=True, linear_solve_method="cholesky_dual_eq")
    # the two pinned texts
    with pytest.raises(ValueError, match="does not take equality constraints \\(A must be None\\)"):
        QPSolver(P_factor=F, P_diag=rho, A=A, b=b, **dict(kw, linear_solve_method="cholesky_dual"))
    for meth in ("cholesky_dual_eq", "cholesky", "cg", None):
        with pytest.raises(ValueError, match="factored form of P exists for linear_solve_method='cholesky_dual' only"):
            QPSolver(P_factor=F, P_diag=rho, **dict(kw, linear_solve_method=meth))
    # factors with A: 'cholesky_dual_eq' and nothing else
    for meth in ("cholesky", "cg", "np_solve", "kkt", None):
        with pytest.raises(ValueError, match="'cholesky_dual_eq'"):
            QPSolver(P_factor=F, P_diag=rho, A=A, b=b, **dict(kw, linear_solve_method=meth))
    with pytest.raises(ValueError, match="Both A and b must be defined"):
        QPSolver(P_factor=F, P_diag=rho, A=A, **kw)
    with pytest.raises(ValueError, match="A must be 2-dimensional"):
        QPSolver(P_factor=F, P_diag=rho, A=A[0], b=b[:1], **kw)
    with pytest.raises(ValueError, match="A must be 2-dimensional"):
        QPSolver(P_factor=F, P_diag=rho, A=np.zeros((0, n)), b=np.zeros(0), **kw)
    with pytest.raises(ValueError, match="A must have n columns"):
        QPSolver(P_factor=F, P_diag=rho, A=A[:, :5], b=b, **kw)
    with pytest.raises(ValueError, match="A and b must have agreeing dimensions"):
        QPSolver(P_factor=F, P_diag=rho, A=A, b=np.zeros(3), **kw)
    with pytest.raises(ValueError, match="Hessian is diagonal and there is nothing to factor"):
        QPSolver(P_diag=rho, A=A, b=b, **kw)
    for bad in (None, 0.0, np.r_[0.0, rho[1:]]):
        with pytest.raises(ValueError, match="without a lower or an upper bound need P_diag > 0 everywhere"):
            QPSolver(P_factor=F, P_diag=bad, A=A, b=b, lower_bound=None, upper_bound=None, **kw)
    with pytest.raises(ValueError, match="P_factor.*P_diag.*P must be None"):
        QPSolver(P=np.eye(n), P_factor=F, A=A, b=b, **kw)
    # a dense P with 'cholesky_dual_eq' stays rejected as before
    with pytest.raises(ValueError, match="Please enter a valid linear solve method!"):
        QPSolver(P=np.eye(n), A=A, b=b, **kw)


def test_newton_class_constants_exports_and_header():
    import NewtonSolver as flat
    import NewtonSolverInfeasibleStart as flat_inf
    from ipm355 import _lib as L
    from ipm355 import newton, problems, solvers
    assert L.SOLVE_CHOLESKY_DUAL_QP_EQ == 10
    for name in ("ipm_syrk_nt3", "ipm_gemv_t3", "ipm_gemv_n3"):
        assert name in L.EXPORTS
    names = [f[0] for f in L.ProblemDesc._fields_]
    assert names[-4:] == ["Pf", "ldpf", "kf", "Pdiag"]           # no field added
    cls = newton.NewtonSolverCholeskyDualQPInfeasibleStart
    assert flat.NewtonSolverCholeskyDualQPInfeasibleStart is cls
    assert flat_inf.NewtonSolverCholeskyDualQPInfeasibleStart is cls
    assert issubclass(cls, newton._NoFallback) and issubclass(cls, newton.NewtonSolverInfeasibleStart)
    assert cls.method == "chol_dual_qp_eq" and cls.infeasible
    assert solvers._solve_method_for(cls) == L.SOLVE_CHOLESKY_DUAL_QP_EQ
    assert solvers._solve_method_for(newton.NewtonSolverCholeskyDualQP) == L.SOLVE_CHOLESKY_DUAL_QP
    assert solvers._solve_method_for(newton.NewtonSolverCholeskyDualInfeasibleStart) == L.SOLVE_CHOLESKY_DUAL_EQ
    src = open(os.path.join(os.path.dirname(golden_io.GOLDEN), "..", "include", "ipm355.h")).read()
    for text in ("#define IPM_SOLVE_CHOLESKY_DUAL_QP_EQ 10", "int ipm_syrk_nt3(", "int ipm_gemv_t3(",
                 "int ipm_gemv_n3(", "K = diag([1/W; 0_p]) + M diag(E) M^T"):
        assert text in src, text
    lib = L.load_library()
    assert all(hasattr(lib, s) for s in ("ipm_syrk_nt3", "ipm_gemv_t3", "ipm_gemv_n3")) and lib.ipm_version() == 1
    # the create-time rejections' reasons, as the library words them
    so = open(L.LIB_PATH, "rb").read()
    for why in (b"IPM_SOLVE_CHOLESKY_DUAL_QP_EQ", b"needs equality rows (p > 0 with A and b",
                b"an LP takes IPM_SOLVE_CHOLESKY_DUAL_EQ", b"phase 1 involves neither P nor A"):
        assert why in so, why
    # the generator: its own function and key set, exact on the grid
    inst = problems.qp_factor_eq_box(40, 8, 5, 3, seed=2, grid=True, with_xf=True, rho="pow2")
    assert sorted(inst) == sorted(["P_factor", "P_diag", "q", "A", "b", "C", "d", "lower_bound", "upper_bound", "xf"])
    xf, LD = inst["xf"], np.longdouble
    assert np.array_equal((inst["A"].astype(LD) @ xf.astype(LD)).astype(np.float64), inst["b"])
    assert (inst["C"] @ xf < inst["d"]).all() and (np.abs(xf) < 3).all()
    for key in ("P_factor", "q", "A", "C", "xf"):
        assert np.array_equal(inst[key] * 1024, np.round(inst[key] * 1024)), key
    F, P = inst["P_factor"], inst["P_factor"].T @ inst["P_factor"]
    assert np.array_equal((F.T.astype(LD) @ F.astype(LD)).astype(np.float64), P)
    none = problems.qp_factor_eq_box(12, 0, 0, 2, seed=1)
    assert none["P_factor"] is None and none["C"] is None and none["d"] is None and none["A"].shape == (2, 12)


# ------------------------------------------------------------------ oracle solves
@pytest.mark.parametrize("case", R.SOLVES, ids=R.solve_id)
def test_oracle_solve_with_the_restatement(case):
    """the restatement as the oracle's infeasible-start direction reaches the oracle's own x* (inside
    max(1e-6, 4 x the oracle's spread under a 1e-15 perturbation of q and b)) and repeats its inner-iteration
    counts up to the barrier iteration until which that perturbation leaves the oracle's own counts unchanged"""
    ref = R.solve_reference(case)
    a = ref["solver"]
    fac = ref["fac"]
    s = R.oracle_qp(ref["dense"], (fac["P_factor"], fac["P_diag"]))
    xr = float(np.linalg.norm(s.xstar - a.xstar) / np.linalg.norm(a.xstar))
    cut = min(ref["cut"], R.CUTS[R.solve_id(case)])     # (the recorded cut, or a shorter one found on this host)
    print(f"[{R.solve_id(case)}] x* rel {xr:.2e} (bar {ref['xbar']:.2e}, spread {ref['spread']:.2e}) cut {cut} inner "
          f"{list(s.inner_iters)} (oracle {list(a.inner_iters)}) |Ax-b| "
          f"{np.linalg.norm(fac['A'] @ s.xstar - fac['b']):.2e}")
    assert xr <= ref["xbar"]
    assert list(s.inner_iters)[:cut] == list(a.inner_iters)[:cut]


# ------------------------------------------------------------------ fixtures (the reference's own runs)
def fixture_kwargs(name):
    """(the fixture, factored solver kwargs, dense kwargs with the host-formed P)"""
    z = golden_io.load(name)
    kw = golden_io.solver_kwargs(z)
    F, rho = kw["P_factor"], kw["P_diag"]
    n = len(rho)
    P = F.T @ F
    P[np.diag_indices(n)] += rho
    dense = {key: v for key, v in kw.items() if key not in ("P_factor", "P_diag")}
    return z, kw, dict(dense, P=P)


@pytest.mark.parametrize("name", ["dual_qp_eq_factored", "dual_qp_eq_budget"])
def test_fixture_is_data_only_and_the_oracle_reaches_it(name):
    """the oracle with the restatement on the fixture's factored inputs reaches the reference's own run"""
    z, kw, dense = fixture_kwargs(name)
    assert os.path.getsize(os.path.join(golden_io.GOLDEN, name + ".npz")) < 128 * 1024
    assert all(v.dtype.kind in "fiubU" for v in z.values())
    s = R.oracle_qp(dense, (kw["P_factor"], kw["P_diag"]))
    xr = float(np.linalg.norm(s.xstar - z["xstar"]) / np.linalg.norm(z["xstar"]))
    vr = abs(s.value - float(z["value"])) / max(1.0, abs(float(z["value"])))
    print(f"[{name}] x* rel {xr:.2e} value rel {vr:.2e} inner {list(s.inner_iters)} (fixture {list(z['inner_iters'])})")
    assert xr <= max(1e-6, 4 * float(z["sens_xstar_rel"]))
    assert vr <= max(1e-8, 4 * float(z["sens_value_rel"]))
    if bool(z["sens_iters_stable"]):
        assert list(s.inner_iters) == list(z["inner_iters"])
