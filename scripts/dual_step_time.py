"""Cost of linear_solve_method='cholesky_dual' on the device:

  * one Newton step (ipm_newton_solve, max_iters = 1, from the same strictly feasible point) of the LP
    n = 8192, m = 2048 (BASELINE config 3) and n = 2048, m = 512 with 'cholesky' and with
    'cholesky_dual': both problems live in one process, the steps are interleaved, the median of
    --steps wall-clock times per method is reported with the engine's own HIP-event slots (kkt: the
    assembly of H or S, potrf: the factorization);
  * HIP-event time of ipm_syrk_nt alone on the same C with weights E, against its m^2 n flops (TF/s
    and the share of the 78.6 TF/s fp64 peak);
  * the same product through ipm_syrk on a transposed copy of C (k-major operand): the comparison
    that says whether the new kernel earns its place against keeping C^T resident.

    python scripts/dual_step_time.py [--sizes 8192x2048,2048x512] [--steps 20] [--reps 20]

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
PEAK_TFLOPS = 78.6


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


def syrk_time(n, m, reps):
    """S = C diag(E) C^T (m x m, sum over n) by ipm_syrk_nt on C and by ipm_syrk on C^T"""
    import torch
    from ipm355 import _lib as L
    h = L.Handle.get(0)
    g = torch.Generator(device="cuda").manual_seed(n + m)
    C = torch.rand((m, n), dtype=torch.float64, device="cuda", generator=g) - 0.5
    E = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) + 0.1
    dv = torch.rand(m, dtype=torch.float64, device="cuda", generator=g) + 0.1
    lds = (m + 1 + 15) // 16 * 16
    S1 = torch.zeros((m + 1, lds), dtype=torch.float64, device="cuda")
    S2 = torch.zeros((m + 1, lds), dtype=torch.float64, device="cuda")
    CT = C.t().contiguous()

    def nt():
        h.check(h.lib.ipm_syrk_nt(h.ptr, m, n, L.dptr(C), n, L.dptr(E), L.dptr(dv), L.dptr(S1), lds), h.ptr)

    def kmajor():
        h.check(h.lib.ipm_syrk(h.ptr, m, n, L.dptr(CT), m, L.dptr(E), 1.0, 0.0, L.dptr(S2), lds), h.ptr)
    out = []
    flops = float(m) * m * n
    for name, fn in (("ipm_syrk_nt (C row-major)", nt), ("ipm_syrk (transposed copy of C)", kmajor)):
        t, tmin = _events(fn, reps)
        out.append({"what": "S_assembly", "kernel": name, "n": n, "m": m, "ms": round(t, 4), "ms_min": round(tmin, 4),
                    "TFLOPs": round(flops / t / 1e9, 2), "share_of_fp64_peak": round(flops / t / 1e9 / PEAK_TFLOPS, 3)})
    a = torch.tril(S1[:m, :m].t())
    b = torch.tril(S2[:m, :m].t()) + torch.diag(dv)
    out.append({"what": "S_assembly_agreement", "n": n, "m": m,
                "max_rel_diff": float(((a - b).abs().max() / b.abs().max()).item())})
    return out


def step_time(n, m, steps):
    import torch

    import ipm355
    from ipm355 import _lib as L
    from ipm355 import problems
    inst = problems.lp_ineq_box(n=n, m=m, seed=0, grid=True, with_xf=True)
    xf = inst.pop("xf")
    kw = problems.LP_KWARGS
    lib = L.Handle.get(0)
    runs = {}
    for method, sm, cls in (("cholesky", L.SOLVE_CHOLESKY, ipm355.NewtonSolverCholesky),
                            ("cholesky_dual", L.SOLVE_CHOLESKY_DUAL, ipm355.NewtonSolverCholeskyDual)):
        fm = ipm355.FunctionManagerLP(c=inst["c"], C=inst["C"], d=inst["d"], x0=xf.copy(), lower_bound=-3,
                                      upper_bound=3, t=1, try_diag=False, solve_method=sm)
        fm.update_t(kw["t0"])
        ns = cls(function_manager=fm, max_iters=1, epsilon=1e-5, alpha=kw["alpha"], beta=kw["beta"])
        runs[method] = (fm, ns, [], fm.prob.ws.numel())
    x0 = torch.as_tensor(xf, device="cuda")
    slots = {}
    for r in range(steps + 1):
        for method, (fm, ns, ts, _) in runs.items():
            x = x0.clone()
            if r == 1:
                lib.lib.ipm_set_timing(lib.ptr, 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ns.solve(x, kw["t0"])
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
        out.append({"what": "newton_step", "n": n, "m": m, "method": method, "ms": round(float(np.median(ts)), 4),
                    "ms_min": round(min(ts), 4), "kkt_ms": round(slots[method][0], 4),
                    "potrf_ms": round(slots[method][1], 4), "step": ns.last_result.last_step,
                    "workspace_MB": round(wsb / 2 ** 20, 1)})
    d = (runs["cholesky"][0].prob.last_direction() - runs["cholesky_dual"][0].prob.last_direction()).norm()
    out.append({"what": "direction_agreement", "n": n, "m": m,
                "rel_diff": float((d / runs["cholesky"][0].prob.last_direction().norm()).item())})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192x2048,2048x512", help="n x m, comma separated")
    ap.add_argument("--steps", type=int, default=20, help="timed Newton steps per method (interleaved)")
    ap.add_argument("--reps", type=int, default=20, help="kernel calls per timed window (5 windows)")
    a = ap.parse_args()
    from ipm355 import _lib as L
    print(json.dumps({"library_sha256": hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()}), flush=True)
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",") if s]
    for n, m in sizes:
        for rec in syrk_time(n, m, a.reps):
            print(json.dumps(rec), flush=True)
    for n, m in sizes:
        for rec in step_time(n, m, a.steps):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
