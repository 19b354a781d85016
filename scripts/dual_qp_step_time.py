"""Cost of the factored QP, QPSolver(P_factor=F, P_diag=rho, linear_solve_method='cholesky_dual'), on the device
(DESIGN.md §11.3):

  one Newton step (ipm_newton_solve, max_iters = 1, from the same strictly feasible point) of the QP n = 8192,
  m = 2048, k = 512 and n = 2048, m = 512, k = 128 with the dense 'cholesky' path (P = diag(rho) + F'F formed on the
  host and resident on the device) and with the factored 'cholesky_dual' path built from the same F, rho: both
  problems live in one process, the steps are interleaved, the median of --steps wall-clock times per method is
  reported with the engine's own HIP-event slots (kkt: the assembly of H or K, potrf: the factorization) and
  the workspace and problem-data bytes.

    python scripts/dual_qp_step_time.py [--sizes 8192x2048x512,2048x512x128] [--steps 20]

Run it three times for the process-to-process spread.  Prints one JSON line per measurement and the sha256 of the
library that ran.
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


def step_time(n, m, k, steps):
    import torch

    import ipm355
    from ipm355 import _lib as L
    from ipm355 import problems
    inst = problems.qp_factor_box(n=n, m=m, k=k, seed=0, grid=True, with_xf=True)
    xf = inst.pop("xf")
    F, rho = inst["P_factor"], inst["P_diag"]
    P = F.T @ F
    P[np.diag_indices(n)] += rho
    kw = problems.QP_KWARGS
    lib = L.Handle.get(0)
    common = dict(q=inst["q"], C=inst["C"], d=inst["d"], x0=xf.copy(), lower_bound=-3, upper_bound=3, t=1)
    runs = {}
    for method, cls, extra in (("cholesky", ipm355.NewtonSolverCholesky, dict(P=P)),
                               ("cholesky_dual (factored)", ipm355.NewtonSolverCholeskyDualQP,
                                dict(P_factor=F, P_diag=rho))):
        fm = ipm355.FunctionManagerQP(**common, **extra)
        fm.update_t(kw["t0"])
        ns = cls(function_manager=fm, max_iters=1, epsilon=1e-5, alpha=kw["alpha"], beta=kw["beta"])
        pr = fm.prob
        data = sum(t.numel() * 8 for t in (pr.P, pr.P_factor, pr.P_diag, pr.C) if t is not None)
        runs[method] = (fm, ns, [], pr.ws.numel(), data)
    del P
    x0 = torch.as_tensor(xf, device="cuda")
    slots = {}
    for r in range(steps + 1):
        for method, (fm, ns, ts, _, _) in runs.items():
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
    for method, (fm, ns, ts, wsb, data) in runs.items():
        out.append({"what": "newton_step", "n": n, "m": m, "k": k, "method": method,
                    "ms": round(float(np.median(ts)), 4), "ms_min": round(min(ts), 4),
                    "kkt_ms": round(slots[method][0], 4), "potrf_ms": round(slots[method][1], 4),
                    "step": ns.last_result.last_step, "workspace_MB": round(wsb / 2 ** 20, 1),
                    "P_and_C_data_MB": round(data / 2 ** 20, 1)})
    pa, pb = (runs[key][0].prob for key in runs)
    d = (pa.last_direction() - pb.last_direction()).norm() / pa.last_direction().norm()
    out.append({"what": "direction_agreement", "n": n, "m": m, "k": k, "dx_rel_diff": float(d.item())})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192x2048x512,2048x512x128", help="n x m x k, comma separated")
    ap.add_argument("--steps", type=int, default=20, help="timed Newton steps per method (interleaved)")
    a = ap.parse_args()
    from ipm355 import _lib as L
    print(json.dumps({"library_sha256": hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()}), flush=True)
    for s in a.sizes.split(","):
        if s:
            n, m, k = (int(v) for v in s.split("x"))
            for rec in step_time(n, m, k, a.steps):
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
