"""Cost of the dual-form phase 1 (PhaseOneSolver(linear_solve_method='cholesky_dual')):

  * one phase-1 Newton step (ipm_newton_solve, max_iters = 1, from the same phase-1 start x = 0,
    s = -min(slacks) + 1) of the LP n = 8192, m = 2048 and n = 2048, m = 512 on the primal bordered
    Cholesky and on the dual form: both problems live in one process, the steps are interleaved, the
    median of --steps wall-clock times per method is reported with the engine's HIP-event slots (kkt: the
    assembly of H~ or S, potrf: the factorization);
  * HIP-event time of ipm_gemv_2v (two vectors over one matrix) against two ipm_gemv calls on the same C,
    both transposes, with the GB/s of the matrix bytes each moves (C once, resp. twice);
  * the two ways to the second solution column S^-1 r_y on a factored S (m = 2048 and 512): one
    single-column ipm_potrs (the substitution kernels the step uses; the first column's forward solve
    rides through the bordered Cholesky, so the step adds one backward substitution to this) against
    ipm_potrs with nrhs = 2 (both columns through the blocked multi-column kernels);
  * wall clock and workspace bytes (phase-1 problem + barrier problem, both alive during a solve) of a whole
    LPSolver.solve() on problems.lp_ineq_box(n, m) with LP_KWARGS in three configurations: all primal,
    linear_solve_method='cholesky_dual' with the primal phase 1, and both phases dual.

    python scripts/dual_phase1_time.py [--sizes 8192x2048,2048x512] [--steps 20] [--reps 20] [--solve 8192x2048]

Run it three times for the process-to-process spread.  Prints one JSON line per measurement and the
sha256 of the library that ran.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "interiorpoint-gpu_amd"))


def _events(fn, reps):
    import torch
    for _ in range(3):
        fn()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return float(np.median(ms)), min(ms)


def gemv_time(n, m, reps):
    """C [x0 | x1] and C^T [z0 | z1]: one ipm_gemv_2v call against two ipm_gemv calls"""
    import torch
    from ipm355 import _lib as L
    h = L.Handle.get(0)
    g = torch.Generator(device="cuda").manual_seed(n + m)
    C = torch.rand((m, n), dtype=torch.float64, device="cuda", generator=g) - 0.5
    out = []
    for trans, kin, kout in ((0, n, m), (1, m, n)):
        X = torch.rand((2, kin), dtype=torch.float64, device="cuda", generator=g) - 0.5
        Y = torch.zeros((2, kout), dtype=torch.float64, device="cuda")
        Y1 = torch.zeros((2, kout), dtype=torch.float64, device="cuda")

        def two_vec():
            h.check(h.lib.ipm_gemv_2v(h.ptr, trans, m, n, L.dptr(C), n, L.dptr(X), kin, L.dptr(Y), kout), h.ptr)

        def two_calls():
            for j in range(2):
                h.check(h.lib.ipm_gemv(h.ptr, trans, m, n, 1.0, L.dptr(C), n, L.dptr(X[j]), 0.0, L.dptr(Y1[j])), h.ptr)
        for name, fn, passes in (("ipm_gemv_2v", two_vec, 1), ("2 x ipm_gemv", two_calls, 2)):
            t, tmin = _events(fn, reps)
            out.append({"what": "gemv_two_vectors", "trans": trans, "kernel": name, "n": n, "m": m, "ms": round(t, 4),
                        "ms_min": round(tmin, 4), "matrix_GBps": round(passes * 8.0 * m * n / t / 1e6, 1)})
        out.append({"what": "gemv_two_vectors_agreement", "trans": trans, "n": n, "m": m,
                    "bitwise_equal": bool(torch.equal(Y, Y1))})
    return out


def second_column_time(n, m, reps):
    """S = diag(dv) + C diag(E) C^T factored once; then S^-1 B for one column and for two (wall clock per
    call with its synchronisation, median of reps: the single-column entry reads its error word back)"""
    import torch
    from ipm355 import _lib as L
    h = L.Handle.get(0)
    g = torch.Generator(device="cuda").manual_seed(n + m + 1)
    C = torch.rand((m, n), dtype=torch.float64, device="cuda", generator=g) - 0.5
    E = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) + 0.1
    dv = torch.rand(m, dtype=torch.float64, device="cuda", generator=g) + 0.1
    lds = (m + 1 + 15) // 16 * 16
    S = torch.zeros((m + 1, lds), dtype=torch.float64, device="cuda")
    h.check(h.lib.ipm_syrk_nt(h.ptr, m, n, L.dptr(C), n, L.dptr(E), L.dptr(dv), L.dptr(S), lds), h.ptr)
    info = ctypes.c_int(-1)
    h.check(h.lib.ipm_potrf(h.ptr, m, L.dptr(S), lds, ctypes.byref(info)), h.ptr)
    B0 = torch.rand((m, 2), dtype=torch.float64, device="cuda", generator=g) - 0.5
    out, sol = [], {}
    for nrhs in (1, 2):
        ts = []
        for r in range(reps + 3):
            B = B0[:, :nrhs].clone()          # (a fresh right-hand side per call: the solve is in place)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.check(h.lib.ipm_potrs(h.ptr, m, nrhs, L.dptr(S), lds, L.dptr(B), nrhs), h.ptr)
            torch.cuda.synchronize()
            if r >= 3:
                ts.append((time.perf_counter() - t0) * 1e3)
        sol[nrhs] = B
        out.append({"what": "factor_solve", "m": m, "nrhs": nrhs, "potrf_info": info.value,
                    "ms": round(float(np.median(ts)), 4), "ms_min": round(min(ts), 4)})
    d = (sol[1][:, 0] - sol[2][:, 0]).norm() / sol[2][:, 0].norm()
    out.append({"what": "factor_solve_agreement", "m": m, "rel_diff": float(d.item())})
    return out


def step_time(n, m, steps):
    import torch

    import ipm355
    from ipm355 import _lib as L
    from ipm355 import problems
    inst = problems.lp_ineq_box(n=n, m=m, seed=0, grid=True)
    kw = problems.LP_KWARGS
    t = 0.01                                   # LPSolver's phase1_t0
    lib = L.Handle.get(0)
    runs = {}
    x_start = None
    for method, sm, cls in (("cholesky", L.SOLVE_CHOLESKY, ipm355.NewtonSolverCholesky),
                            ("cholesky_dual", L.SOLVE_CHOLESKY_DUAL_PHASE1, ipm355.NewtonSolverCholeskyDual)):
        fm = ipm355.FunctionManagerPhase1(C=inst["C"], d=inst["d"], x0=np.zeros(n), lower_bound=-3, upper_bound=3,
                                          t=t, solve_method=sm)
        x_start = np.append(np.zeros(n), fm.s)
        ns = cls(function_manager=fm, max_iters=1, epsilon=1e-5, alpha=kw["alpha"], beta=kw["beta"], phase1_flag=True,
                 phase1_tol=0)
        runs[method] = (fm, ns, [], fm.prob.ws.numel())
    x0 = torch.as_tensor(x_start, device="cuda")
    slots = {}
    for r in range(steps + 1):
        for method, (fm, ns, ts, _) in runs.items():
            x = x0.clone()
            fm.update_x(x)
            if r == 1:
                lib.lib.ipm_set_timing(lib.ptr, 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ns.solve(x, t)
            torch.cuda.synchronize()
            if r:
                ts.append((time.perf_counter() - t0) * 1e3)
            if r == 1:
                a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
                lib.lib.ipm_last_timings(lib.ptr, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
                slots[method] = (a.value, b.value)
                lib.lib.ipm_set_timing(lib.ptr, 0)
    out = []
    for method, (fm, ns, ts, wsb) in runs.items():
        out.append({"what": "phase1_newton_step", "n": n, "m": m, "method": method,
                    "ms": round(float(np.median(ts)), 4), "ms_min": round(min(ts), 4),
                    "kkt_ms": round(slots[method][0], 4), "potrf_ms": round(slots[method][1], 4),
                    "step": ns.last_result.last_step, "workspace_MB": round(wsb / 2 ** 20, 1)})
    a, b = runs["cholesky"][0].prob.last_direction(), runs["cholesky_dual"][0].prob.last_direction()
    out.append({"what": "phase1_direction_agreement", "n": n, "m": m, "rel_diff": float(((a - b).norm() / a.norm()).item())})
    return out


def solve_time(n, m, solves):
    import torch

    import ipm355
    from ipm355 import problems
    inst = problems.lp_ineq_box(n=n, m=m, seed=0)
    out = []
    configs = (("all primal", "cholesky", None), ("cholesky_dual, primal phase 1", "cholesky_dual", None),
               ("both phases dual", "cholesky_dual", "cholesky_dual"))
    for name, method, p1 in configs:
        ts, rec = [], None
        for _ in range(solves):
            s = ipm355.LPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method=method,
                                phase1_linear_solve_method=p1, **dict(inst, **problems.LP_KWARGS))
            wsb = s.fm.prob.ws.numel() + s.phase1_solver.phase1_fm.prob.ws.numel()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            val = s.solve()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            rec = {"what": "lp_solve", "n": n, "m": m, "config": name, "value": val,
                   "phase1_iters": list(s.phase1_solver.inner_iters), "inner_iters": list(s.inner_iters),
                   "workspace_MB": round(wsb / 2 ** 20, 1)}
            del s
            torch.cuda.empty_cache()
        rec.update({"seconds": round(float(np.median(ts)), 4), "seconds_min": round(min(ts), 4),
                    "seconds_first": round(ts[0], 4)})
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192x2048,2048x512", help="n x m, comma separated")
    ap.add_argument("--steps", type=int, default=20, help="timed Newton steps per method (interleaved)")
    ap.add_argument("--reps", type=int, default=20, help="kernel calls per timed window (5 windows)")
    ap.add_argument("--solve", default="8192x2048", help="n x m of the whole LPSolver.solve() ('' to skip)")
    ap.add_argument("--solves", type=int, default=3, help="solves per configuration (the median is reported)")
    a = ap.parse_args()
    from ipm355 import _lib as L
    print(json.dumps({"library_sha256": hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()}), flush=True)
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",") if s]
    for n, m in sizes:
        for rec in gemv_time(n, m, a.reps):
            print(json.dumps(rec), flush=True)
    for n, m in sizes:
        for rec in second_column_time(n, m, a.reps):
            print(json.dumps(rec), flush=True)
    for n, m in sizes:
        for rec in step_time(n, m, a.steps):
            print(json.dumps(rec), flush=True)
    if a.solve:
        n, m = (int(v) for v in a.solve.split("x"))
        for rec in solve_time(n, m, a.solves):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
