"""Cost of linear_solve_method='cholesky_dual_eq' on the device:

  * one Newton step (ipm_newton_solve, max_iters = 1, from the same strictly feasible point and v = 0) of the
    LP n = 8192, m = 2048, p = 512 and n = 2048, m = 512, p = 128 with 'cholesky' (the primal infeasible-start
    block elimination) and with 'cholesky_dual_eq': both problems live in one process, the steps are
    interleaved, the median of --steps wall-clock times per method is reported with the engine's own
    HIP-event slots (kkt: the assembly of H or K, potrf: the first factorization) and the workspace bytes;
  * HIP-event time of ipm_syrk_nt2 on (C, A) against ipm_syrk_nt on a physically stacked copy of the two
    (the same plan and arithmetic: the difference is the per-row choice of the operand), with the agreement
    of the two results (bitwise).

    python scripts/dual_eq_step_time.py [--sizes 8192x2048x512,2048x512x128] [--steps 20] [--reps 20]

Run it three times for the process-to-process spread.  Prints one JSON line per measurement and the sha256
of the library that ran.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dual_step_time import PEAK_TFLOPS, _events  # noqa: E402


def syrk_time(n, m, p, reps):
    """K's product M diag(E) M^T, M = [C; A], by ipm_syrk_nt2 on (C, A) and by ipm_syrk_nt on a stacked copy"""
    import torch
    from ipm355 import _lib as L
    h = L.Handle.get(0)
    g = torch.Generator(device="cuda").manual_seed(n + m + p)
    M = torch.rand((m + p, n), dtype=torch.float64, device="cuda", generator=g) - 0.5
    C, A = M[:m].clone(), M[m:].clone()
    E = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) + 0.1
    dv = torch.rand(m + p, dtype=torch.float64, device="cuda", generator=g) + 0.1
    mk = m + p
    lds = (mk + 1 + 15) // 16 * 16
    K1 = torch.zeros((mk + 1, lds), dtype=torch.float64, device="cuda")
    K2 = torch.zeros((mk + 1, lds), dtype=torch.float64, device="cuda")

    def two():
        h.check(h.lib.ipm_syrk_nt2(h.ptr, m, p, n, L.dptr(C), n, L.dptr(A), n, L.dptr(E), L.dptr(dv), L.dptr(K1),
                                   lds), h.ptr)

    def stacked():
        h.check(h.lib.ipm_syrk_nt(h.ptr, mk, n, L.dptr(M), n, L.dptr(E), L.dptr(dv), L.dptr(K2), lds), h.ptr)
    out = []
    flops = float(mk) * mk * n
    # interleaved: each kernel timed twice, in the order two, stacked, two, stacked
    for name, fn in (("ipm_syrk_nt2 (C, A)", two), ("ipm_syrk_nt (stacked copy)", stacked)) * 2:
        t, tmin = _events(fn, reps)
        out.append({"what": "K_assembly", "kernel": name, "n": n, "m": m, "p": p, "ms": round(t, 4),
                    "ms_min": round(tmin, 4), "TFLOPs": round(flops / t / 1e9, 2),
                    "share_of_fp64_peak": round(flops / t / 1e9 / PEAK_TFLOPS, 3)})
    out.append({"what": "K_assembly_agreement", "n": n, "m": m, "p": p,
                "bitwise_equal": bool(torch.equal(torch.tril(K1[:mk, :mk].t()), torch.tril(K2[:mk, :mk].t())))})
    return out


def step_time(n, m, p, steps):
    import torch

    import ipm355
    from ipm355 import _lib as L
    from ipm355 import problems
    inst = problems.lp_ineq_box(n=n, m=m, seed=0, grid=True, with_xf=True)
    xf = inst.pop("xf")
    A = np.random.default_rng(1).normal(size=(p, n))
    x0h = xf + 0.001 * np.random.default_rng(2).uniform(-1, 1, n)      # strictly inside, off A x = b
    b = A @ xf
    kw = problems.LP_KWARGS
    lib = L.Handle.get(0)
    runs = {}
    for method, sm, cls in (("cholesky", L.SOLVE_CHOLESKY, ipm355.NewtonSolverCholeskyInfeasibleStart),
                            ("cholesky_dual_eq", L.SOLVE_CHOLESKY_DUAL_EQ,
                             ipm355.NewtonSolverCholeskyDualInfeasibleStart)):
        fm = ipm355.FunctionManagerLP(c=inst["c"], A=A, b=b, C=inst["C"], d=inst["d"], x0=x0h.copy(), lower_bound=-3,
                                      upper_bound=3, t=1, try_diag=False, solve_method=sm)
        fm.update_t(kw["t0"])
        ns = cls(A, b, inst["C"], inst["d"], fm, max_iters=1, epsilon=1e-5, alpha=kw["alpha"], beta=kw["beta"])
        runs[method] = (fm, ns, [], fm.prob.ws.numel())
    x0 = torch.as_tensor(x0h, device="cuda")
    slots = {}
    for r in range(steps + 1):
        for method, (fm, ns, ts, _) in runs.items():
            x = x0.clone()
            v = torch.zeros(p, dtype=torch.float64, device="cuda")
            if r == 1:
                lib.lib.ipm_set_timing(lib.ptr, 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ns.solve(x, kw["t0"], v0=v)
            torch.cuda.synchronize()
            if r:
                ts.append((time.perf_counter() - t0) * 1e3)
            if r == 1:
                a, bb, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
                lib.lib.ipm_last_timings(lib.ptr, ctypes.byref(a), ctypes.byref(bb), ctypes.byref(c))
                slots[method] = (a.value, bb.value)
                lib.lib.ipm_set_timing(lib.ptr, 0)
    out = []
    for method, (fm, ns, ts, wsb) in runs.items():
        out.append({"what": "newton_step", "n": n, "m": m, "p": p, "method": method,
                    "ms": round(float(np.median(ts)), 4), "ms_min": round(min(ts), 4),
                    "kkt_ms": round(slots[method][0], 4), "potrf_ms": round(slots[method][1], 4),
                    "step": ns.last_result.last_step, "workspace_MB": round(wsb / 2 ** 20, 1)})
    pa, pb = runs["cholesky"][0].prob, runs["cholesky_dual_eq"][0].prob
    d = (pa.last_direction() - pb.last_direction()).norm() / pa.last_direction().norm()
    dv = (pa.last_dual_direction() - pb.last_dual_direction()).norm() / pa.last_dual_direction().norm()
    out.append({"what": "direction_agreement", "n": n, "m": m, "p": p, "dx_rel_diff": float(d.item()),
                "dv_rel_diff": float(dv.item())})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192x2048x512,2048x512x128", help="n x m x p, comma separated")
    ap.add_argument("--steps", type=int, default=20, help="timed Newton steps per method (interleaved)")
    ap.add_argument("--reps", type=int, default=20, help="kernel calls per timed window (5 windows)")
    a = ap.parse_args()
    from ipm355 import _lib as L
    print(json.dumps({"library_sha256": hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()}), flush=True)
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",") if s]
    for n, m, p in sizes:
        for rec in syrk_time(n, m, p, a.reps):
            print(json.dumps(rec), flush=True)
    for n, m, p in sizes:
        for rec in step_time(n, m, p, a.steps):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
