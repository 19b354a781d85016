"""No GPU: the references of the dual-form Newton step (tests/dual_ref.py) and the host-side rules of
linear_solve_method='cholesky_dual'.

  * the fp64 restatement of the step stays within a QUARTER of the bound B at every state
    test_gpu_dual_step.py runs on the device (B is not a theorem for the dual form: this is where it
    is checked; worst err / B measured over the 297 states: 0.0045);
  * full oracle solves with the restatement plugged in keep the Cholesky oracle's iteration counts
    and land on its x* and value;
  * ipm_workspace_bytes of IPM_SOLVE_CHOLESKY_DUAL has no n^2 term;
  * the facades' argument checks.
"""
import ctypes

import numpy as np
import pytest

import dual_ref as D
import golden_io


def test_restatement_within_a_quarter_of_the_bound():
    worst, where = 0.0, None
    for s in D.states():
        ref = D.reference_step(s)
        fm = ref["inst"].oracle(s[3])
        dx = D.dual_direction(fm, fm.gradient().copy())
        assert np.all(np.isfinite(dx)) and np.isfinite(ref["bound"]) and ref["bound"] > 0
        r = float(np.linalg.norm(dx - ref["dx"]) / ref["bound"])
        if r > worst:
            worst, where = r, D.state_id(s)
    print(f"fp64 restatement: worst err / B {worst:.3g} at {where} over {len(D.states())} states")
    assert worst <= 0.25, (worst, where)


def test_states_cover_the_grid():
    st = D.states()
    assert len(st) == 11 * 3 * 3 * 3 == len(set(st))
    # m >= n is legal; every point is strictly inside, the 0.999 ones close to the boundary
    assert any(m >= n for n, m, *_ in st)
    for n, m, b, t, f in st:
        inst = D.instance(n, m, b, f)
        s = inst.oracle(t).slacks
        assert s.min() > 0 and np.isfinite(inst.amax)
    near = [D.instance(n, m, b, 0.999).oracle(1.0).slacks.min() for n, m, b, t, f in st if f == 0.999 and t == 1.0]
    assert max(near) < 0.05


def test_line_search_replay_and_decisiveness():
    """the replay of the oracle's backtracking returns the step its own solve takes, and nearly every
    state is decisive (295 of 297 when written): the GPU test's step-size assertion is not vacuous"""
    from oracle import ipm_oracle as O
    st = D.states()
    for s in st[::37]:
        inst = D.instance(s[0], s[1], s[2], s[4])
        ns = O.FeasibleNewton(inst.oracle(s[3]), max_iters=1, eps=1e-5, alpha=0.2, beta=0.6)
        ns.solve(inst.x.copy(), s[3])
        assert ns.trace[0]["step"] == D.oracle_line_search(s)["step"]
    decisive = sum(D.oracle_line_search(s)["decisive"] for s in st)
    print(f"decisive line searches: {decisive} of {len(st)}")
    assert decisive >= 0.9 * len(st)


@pytest.mark.parametrize("add", [0.0, 1e-9])
def test_restatement_solves_the_same_system(add):
    """dual_direction and a dense solve of H = diag(D) + C^T diag(w) C (the oracle's own hessian(),
    psd add on its diagonal) agree: the Woodbury identity is restated correctly"""
    inst = D.instance(33, 31, "both", 0.9)
    fm = inst.oracle(1e3)
    g = fm.gradient().copy()
    H = np.array(fm.hessian(), copy=True)
    H[np.diag_indices(len(g))] += add
    dx = np.linalg.solve(H, -g)
    got = D.dual_direction(fm, g, add)
    assert np.linalg.norm(got - dx) <= 1e-9 * np.linalg.norm(dx)


def _lp_cases():
    from ipm355 import problems
    z = golden_io.load("lp_ineq_box")
    kw = golden_io.solver_kwargs(z)
    kw["x0"] = z["x_init"].copy()
    # (x* bar, value bar): 10 x the figures measured when the method was proposed
    yield "lp_ineq_box", kw, 6.6e-9, 3.5e-9
    for (n, m), xb in (((200, 150), 5.8e-8), ((300, 40), 6.1e-9), ((64, 63), 3.2e-8)):
        yield f"generated-{n}x{m}", dict(problems.lp_ineq_box(n, m, seed=5)), xb, 3.5e-9


@pytest.mark.parametrize("case", list(_lp_cases()), ids=lambda c: c[0])
def test_full_oracle_solves_keep_the_trajectory(case):
    """default epsilon = 1e-10 (t up to 1.3e13): the restatement's worst single steps are far less
    accurate than the Cholesky's there, the solves still agree"""
    name, kw, xbar, vbar = case
    copy = lambda: {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}  # noqa: E731
    a = D.oracle_lp(copy(), False)
    b = D.oracle_lp(copy(), True)
    xr = float(np.linalg.norm(a.xstar - b.xstar) / np.linalg.norm(a.xstar))
    vr = abs(a.value - b.value) / abs(a.value)
    print(f"[{name}] inner {b.inner_iters} (cholesky {a.inner_iters}) x* rel {xr:.2e} value rel {vr:.2e}")
    assert list(a.inner_iters) == list(b.inner_iters)
    assert xr <= xbar and vr <= vbar


def _desc(L, method, n=16384, m=256, **kw):
    d = L.ProblemDesc()
    d.kind = L.KIND_LP
    d.solve_method = method
    d.n, d.m, d.ldc = n, m, n
    d.c = d.C = d.d = d.lb = d.ub = 1      # non-null markers; only sizes are read
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_workspace_has_no_n_squared_term():
    from ipm355 import _lib as L
    lib = L.load_library()
    n = 16384
    dual = lib.ipm_workspace_bytes(ctypes.byref(_desc(L, L.SOLVE_CHOLESKY_DUAL)))
    chol = lib.ipm_workspace_bytes(ctypes.byref(_desc(L, L.SOLVE_CHOLESKY)))
    print(f"workspace bytes at n = {n}, m = 256: cholesky_dual {dual}, cholesky {chol}")
    assert 0 < dual < 8 * n * n // 16
    assert chol >= 8 * n * n
    # doubling n doubles it at most (plus the parts that do not depend on n)
    dual2 = lib.ipm_workspace_bytes(ctypes.byref(_desc(L, L.SOLVE_CHOLESKY_DUAL, n=2 * n, ldc=2 * n)))
    assert dual2 <= 2 * dual


def test_every_other_method_keeps_its_byte_count():
    """the byte counts of the parent commit's library at this descriptor (LP n = 300, m = 40, both
    bounds), recorded before the carve learned about the dual form"""
    from ipm355 import _lib as L
    lib = L.load_library()
    got = {meth: lib.ipm_workspace_bytes(ctypes.byref(_desc(L, meth, n=300, m=40, ldc=300)))
           for meth in (L.SOLVE_CHOLESKY, L.SOLVE_LU, L.SOLVE_LSTSQ, L.SOLVE_CG)}
    assert got == PARENT_BYTES, got


PARENT_BYTES = {0: 5191176, 2: 4137992, 3: 5191176, 5: 832776}   # cholesky, LU, lstsq, cg


def test_facade_argument_checks():
    from ipm355 import LPSolver, QPSolver
    rng = np.random.default_rng(0)
    n, m = 6, 3
    C, d, c = rng.normal(size=(m, n)), np.ones(m), rng.normal(size=n)
    A, b = rng.normal(size=(2, n)), np.zeros(2)
    kw = dict(check_cvxpy=False, suppress_print=True, linear_solve_method="cholesky_dual")
    with pytest.raises(ValueError, match="cholesky_dual.*equality"):
        LPSolver(c=c, A=A, b=b, C=C, d=d, lower_bound=-3, upper_bound=3, **kw)
    with pytest.raises(ValueError, match="cholesky_dual.*inequality"):
        LPSolver(c=c, lower_bound=-3, upper_bound=3, **kw)
    with pytest.raises(ValueError, match="cholesky_dual.*bound"):
        LPSolver(c=c, C=C, d=d, lower_bound=None, upper_bound=None, **kw)
    # QPSolver does not know the method (no C: nothing touches the device before the dispatch)
    with pytest.raises(ValueError, match="Please enter a valid linear solve method!"):
        QPSolver(P=np.eye(n), q=c, **kw)


def test_newton_class_and_method_constant():
    import NewtonSolver as flat
    from ipm355 import _lib as L
    from ipm355 import newton, solvers
    assert L.SOLVE_CHOLESKY_DUAL == 6
    assert flat.NewtonSolverCholeskyDual is newton.NewtonSolverCholeskyDual
    assert newton.NewtonSolverCholeskyDual.method == "chol_dual"
    assert solvers._solve_method_for(newton.NewtonSolverCholeskyDual) == L.SOLVE_CHOLESKY_DUAL
    assert solvers._solve_method_for(newton.NewtonSolverCholesky) == L.SOLVE_CHOLESKY
    src = open(golden_io.os.path.join(golden_io.os.path.dirname(golden_io.GOLDEN), "..", "include", "ipm355.h")).read()
    assert "#define IPM_SOLVE_CHOLESKY_DUAL 6" in src
