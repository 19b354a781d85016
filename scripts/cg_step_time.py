"""Cost of linear_solve_method='cg' on the device (the CG section):

  * HIP-event time of ipm_symv at n = 2049, 4097, 8193 with the leading dimension the engine gives
    H (whole 128-byte lines above n + 1), as GB/s of the lower-triangle bytes n (n + 1) / 2 * 8;
  * HIP-event time of one ipm_cg and one ipm_pcg call (minv = NULL: 1 / diag(H) computed by the call)
    with the same maxiter on the same H at the same sizes -- rtol = 0, so every one of the maxiter
    iterations runs -- and of the preconditioner's own launch, as the difference of the two
    maxiter = 0 calls (the prologue with and without k_cg_minv);
  * one Newton step (ipm_newton_solve, max_iters = 1, from the same strictly feasible point) of the
    QP n = 2048 (m = 512) and n = 8192 (m = 2048), with 'cg' (cap 50) and with 'cholesky', in one
    process on one instance.

    python scripts/cg_step_time.py [--symv-sizes 2049,4097,8193] [--sizes 2048,8192] [--reps 1000] [--steps 20]
                                   [--cg-maxiter 50] [--cg-reps 20]

Prints one JSON line per measurement and the sha256 of the library that ran.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "interiorpoint-gpu_amd"))


def symv_time(n, reps):
    import torch
    from ipm355 import _lib as L
    h = L.Handle.get(0)
    ldh = (n + 1 + 15) // 16 * 16
    H = torch.rand((n, ldh), dtype=torch.float64, device="cuda")
    x = torch.rand(n, dtype=torch.float64, device="cuda")
    y = torch.empty(n, dtype=torch.float64, device="cuda")

    def run():
        h.check(h.lib.ipm_symv(h.ptr, n, 1.0, L.dptr(H), ldh, L.dptr(x), 0.0, L.dptr(y)), h.ptr)
    for _ in range(3):
        run()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    t = float(np.median(ms))
    nbytes = n * (n + 1) / 2 * 8
    return {"what": "ipm_symv", "n": n, "ldh": ldh, "ms": round(t, 5), "ms_min": round(min(ms), 5),
            "lower_triangle_GBps": round(nbytes / t / 1e6, 1)}


def cg_time(n, maxiter, reps):
    """median of 5 windows of `reps` calls, HIP events around each window -> ms per call of ipm_cg and
    (where the library has it) ipm_pcg; H = S (A + n I) S, S = diag(10 ** U(-1, 1)): positive
    definite, only its lower triangle is read"""
    import ctypes

    import torch
    from ipm355 import _lib as L
    h = L.Handle.get(0)
    ldh = (n + 1 + 15) // 16 * 16
    g = torch.Generator(device="cuda").manual_seed(n)
    H = torch.rand((n, ldh), dtype=torch.float64, device="cuda", generator=g)
    s = 10.0 ** (2 * torch.rand(n, dtype=torch.float64, device="cuda", generator=g) - 1)
    H[:, :n] += n * torch.eye(n, dtype=torch.float64, device="cuda")
    H[:, :n] *= s[:, None] * s[None, :]
    b = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    it, info = ctypes.c_int32(), ctypes.c_int32()

    def cg(mi):
        x.zero_()
        h.check(h.lib.ipm_cg(h.ptr, n, L.dptr(H), ldh, L.dptr(b), L.dptr(x), mi, 0.0, ctypes.byref(it),
                             ctypes.byref(info)), h.ptr)

    def pcg(mi):
        x.zero_()
        h.check(h.lib.ipm_pcg(h.ptr, n, L.dptr(H), ldh, None, L.dptr(b), L.dptr(x), mi, 0.0, ctypes.byref(it),
                              ctypes.byref(info)), h.ptr)

    def timed(fn, mi, reps):
        for _ in range(3):
            fn(mi)
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn(mi)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
        return float(np.median(ms)), min(ms)
    rec = {"what": "cg_call", "n": n, "ldh": ldh, "maxiter": maxiter}
    t, tmin = timed(cg, maxiter, reps)
    rec.update(cg_ms=round(t, 4), cg_ms_min=round(tmin, 4), cg_iters=it.value)
    if hasattr(h.lib, "ipm_pcg"):
        t, tmin = timed(pcg, maxiter, reps)
        rec.update(pcg_ms=round(t, 4), pcg_ms_min=round(tmin, 4), pcg_iters=it.value)
        t0, _ = timed(cg, 0, 50 * reps)
        t1, _ = timed(pcg, 0, 50 * reps)
        rec.update(prologue_cg_ms=round(t0, 5), prologue_pcg_ms=round(t1, 5), minv_ms=round(t1 - t0, 5))
    return rec


def step_time(n, m, reps):
    import torch

    import ipm355
    from ipm355 import problems

    def gram(Pp):
        d = torch.as_tensor(Pp, device="cuda")
        return (d.T @ d).cpu().numpy()
    inst = problems.qp_ineq_box(n=n, m=m, seed=0, grid=True, with_xf=True, gram=gram)
    xf = inst.pop("xf")
    out = []
    for method in ("cholesky", "cg"):
        s = ipm355.QPSolver(check_cvxpy=False, suppress_print=True, linear_solve_method=method, max_cg_iters=50,
                            **dict(inst, **problems.QP_KWARGS))
        x0 = torch.as_tensor(xf, device="cuda")
        s.fm.update_t(s.t0)
        s.ns.max_iters = 1
        ts = []
        for r in range(reps + 1):
            x = x0.clone()
            s.fm.update_x(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.ns.solve(x, s.t0)
            torch.cuda.synchronize()
            if r:
                ts.append((time.perf_counter() - t0) * 1e3)
        rec = {"what": "newton_step", "n": n, "m": m, "method": method, "ms": round(float(np.median(ts)), 4),
               "ms_min": round(min(ts), 4), "step": s.ns.last_result.last_step}
        if method == "cg":
            rec["cg"] = s.fm.prob.cg_stats()
        out.append(rec)
        del s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--symv-sizes", default="2049,4097,8193")
    ap.add_argument("--sizes", default="2048,8192")
    ap.add_argument("--reps", type=int, default=1000, help="ipm_symv calls per timed window (5 windows)")
    ap.add_argument("--steps", type=int, default=20, help="timed Newton steps per method")
    ap.add_argument("--cg-maxiter", type=int, default=50, help="iterations of the timed ipm_cg / ipm_pcg calls")
    ap.add_argument("--cg-reps", type=int, default=20, help="ipm_cg / ipm_pcg calls per timed window (5 windows)")
    a = ap.parse_args()
    from ipm355 import _lib as L
    print(json.dumps({"library_sha256": hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()}), flush=True)
    for n in [int(v) for v in a.symv_sizes.split(",") if v]:
        print(json.dumps(symv_time(n, a.reps)), flush=True)
    for n in [int(v) for v in a.symv_sizes.split(",") if v]:
        print(json.dumps(cg_time(n, a.cg_maxiter, a.cg_reps)), flush=True)
    for n in [int(v) for v in a.sizes.split(",") if v]:
        for rec in step_time(n, n // 4, a.steps):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
