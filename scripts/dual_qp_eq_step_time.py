"""Cost of the factored QP with equality rows, linear_solve_method='cholesky_dual_eq' with P_factor / P_diag
(IPM_SOLVE_CHOLESKY_DUAL_QP_EQ):

  * one Newton step (ipm_newton_solve, max_iters = 1, from the same strictly feasible point off A x = b and
    v = 0) of the QP n = 8192, m = 2048, k = 512, p = 512 and n = 2048, m = 512, k = 128, p = 128 with the dense
    'cholesky' (P formed on the host from the same F, rho; the primal infeasible-start block elimination) and
    with the factored 'cholesky_dual_eq': both problems live in one process, the steps are interleaved, the
    median of --steps wall-clock times per method is reported with the engine's own HIP-event slots (kkt: the
    assembly of H or K, potrf: the first factorization), the workspace bytes, the bytes of the problem data on
    the device and the flop ratio  (m n^2 + n^3 / 3 + 2 n^2 p) / ((m + k + p)^2 n + (m + k + p)^3 / 3);
  * HIP-event time of ipm_syrk_nt3 on (C, F, A) and of ipm_syrk_nt2 on (C, [F; A] stacked) against ipm_syrk_nt
    on a physically stacked copy of all three (the same plan and arithmetic: the difference is the per-row
    choice of the operand), with the agreement of the results (bitwise).

    python scripts/dual_qp_eq_step_time.py [--sizes 8192x2048x512x512,2048x512x128x128] [--steps 20] [--reps 20]

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


def syrk_time(n, m, k, p, reps):
    """K's product M diag(E) M^T, M = [C; F; A]: three operands, two operands, and one stacked copy"""
    import torch
    from ipm355 import _lib as L
    h = L.Handle.get(0)
    g = torch.Generator(device="cuda").manual_seed(n + m + k + p)
    mk = m + k + p
    M = torch.rand((mk, n), dtype=torch.float64, device="cuda", generator=g) - 0.5
    C, F, A, FA = M[:m].clone(), M[m:m + k].clone(), M[m + k:].clone(), M[m:].clone()
    E = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) + 0.1
    dv = torch.rand(mk, dtype=torch.float64, device="cuda", generator=g) + 0.1
    lds = (mk + 1 + 15) // 16 * 16
    K1, K2, K3 = (torch.zeros((mk + 1, lds), dtype=torch.float64, device="cuda") for _ in range(3))

    def three():
        h.check(h.lib.ipm_syrk_nt3(h.ptr, m, k, p, n, L.dptr(C), n, L.dptr(F), n, L.dptr(A), n, L.dptr(E), L.dptr(dv),
                                   L.dptr(K3), lds), h.ptr)

    def two():
        h.check(h.lib.ipm_syrk_nt2(h.ptr, m, k + p, n, L.dptr(C), n, L.dptr(FA), n, L.dptr(E), L.dptr(dv), L.dptr(K2),
                                   lds), h.ptr)

    def stacked():
        h.check(h.lib.ipm_syrk_nt(h.ptr, mk, n, L.dptr(M), n, L.dptr(E), L.dptr(dv), L.dptr(K1), lds), h.ptr)
    out = []
    flops = float(mk) * mk * n
    # alternating within the process: each kernel timed twice
    for name, fn in (("ipm_syrk_nt3 (C, F, A)", three), ("ipm_syrk_nt2 (C, [F; A])", two),
                     ("ipm_syrk_nt (stacked copy)", stacked)) * 2:
        t, tmin = _events(fn, reps)
        out.append({"what": "K_assembly", "kernel": name, "n": n, "m": m, "k": k, "p": p, "ms": round(t, 4),
                    "ms_min": round(tmin, 4), "TFLOPs": round(flops / t / 1e9, 2),
                    "share_of_fp64_peak": round(flops / t / 1e9 / PEAK_TFLOPS, 3)})
    low = lambda K: torch.tril(K[:mk, :mk].t())
    out.append({"what": "K_assembly_agreement", "n": n, "m": m, "k": k, "p": p,
                "bitwise_equal": bool(torch.equal(low(K3), low(K1)) and torch.equal(low(K2), low(K1)))})
    return out


def step_time(n, m, k, p, steps):
    import torch

    import ipm355
    from ipm355 import _lib as L
    from ipm355 import problems
    inst = problems.qp_factor_eq_box(n, m, k, p, seed=0, grid=True, with_xf=True)
    xf = inst.pop("xf")
    F, rho, A, b = inst["P_factor"], inst["P_diag"], inst["A"], inst["b"]
    P = F.T @ F
    P[np.diag_indices(n)] += rho
    x0h = xf + 0.001 * np.random.default_rng(2).uniform(-1, 1, n)      # strictly inside, off A x = b
    kw = problems.QP_KWARGS
    lib = L.Handle.get(0)
    runs = {}
    common = dict(q=inst["q"], A=A, b=b, C=inst["C"], d=inst["d"], lower_bound=-3, upper_bound=3, t=1)
    for method, extra, cls in (("cholesky", dict(P=P), ipm355.NewtonSolverCholeskyInfeasibleStart),
                               ("cholesky_dual_eq", dict(P_factor=F, P_diag=rho),
                                ipm355.newton.NewtonSolverCholeskyDualQPInfeasibleStart)):
        fm = ipm355.FunctionManagerQP(x0=x0h.copy(), **common, **extra)
        fm.update_t(kw["t0"])
        ns = cls(A, b, inst["C"], inst["d"], fm, max_iters=1, epsilon=1e-5, alpha=kw["alpha"], beta=kw["beta"])
        pr = fm.prob
        data = sum(t.numel() * 8 for t in (pr.P, pr.P_factor, pr.P_diag, pr.q, pr.C, pr.d, pr.lb, pr.ub, pr.A,
                                           pr.AT, pr.b) if t is not None)
        runs[method] = (fm, ns, [], pr.ws.numel(), data)
    x0 = torch.as_tensor(x0h, device="cuda")
    slots = {}
    for r in range(steps + 1):
        for method, (fm, ns, ts, _, _) in runs.items():
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
    for method, (fm, ns, ts, wsb, data) in runs.items():
        out.append({"what": "newton_step", "n": n, "m": m, "k": k, "p": p, "method": method,
                    "ms": round(float(np.median(ts)), 4), "ms_min": round(min(ts), 4),
                    "kkt_ms": round(slots[method][0], 4), "potrf_ms": round(slots[method][1], 4),
                    "step": ns.last_result.last_step, "workspace_MB": round(wsb / 2 ** 20, 1),
                    "data_MB": round(data / 2 ** 20, 1)})
    dm = m + k + p
    dense_flops = float(m) * n * n + n ** 3 / 3.0 + 2.0 * n * n * p
    dual_flops = float(dm) * dm * n + dm ** 3 / 3.0
    td, tf = (float(np.median(runs[key][2])) for key in ("cholesky", "cholesky_dual_eq"))
    out.append({"what": "ratio", "n": n, "m": m, "k": k, "p": p, "flop_ratio": round(dense_flops / dual_flops, 2),
                "time_ratio": round(td / tf, 2)})
    pa, pb = runs["cholesky"][0].prob, runs["cholesky_dual_eq"][0].prob
    d = (pa.last_direction() - pb.last_direction()).norm() / pa.last_direction().norm()
    dv = (pa.last_dual_direction() - pb.last_dual_direction()).norm() / pa.last_dual_direction().norm()
    out.append({"what": "direction_agreement", "n": n, "m": m, "k": k, "p": p, "dx_rel_diff": float(d.item()),
                "dv_rel_diff": float(dv.item())})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192x2048x512x512,2048x512x128x128", help="n x m x k x p, comma separated")
    ap.add_argument("--steps", type=int, default=20, help="timed Newton steps per method (interleaved)")
    ap.add_argument("--reps", type=int, default=20, help="kernel calls per timed window (5 windows)")
    a = ap.parse_args()
    from ipm355 import _lib as L
    print(json.dumps({"library_sha256": hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()}), flush=True)
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",") if s]
    for n, m, k, p in sizes:
        for rec in syrk_time(n, m, k, p, a.reps):
            print(json.dumps(rec), flush=True)
    for n, m, k, p in sizes:
        for rec in step_time(n, m, k, p, a.steps):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
