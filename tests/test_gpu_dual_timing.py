"""-m gpu: the HIP-event timing mode (ipm_set_timing / ipm_last_timings) on the three dual-form Newton steps,
IPM_SOLVE_CHOLESKY_DUAL, IPM_SOLVE_CHOLESKY_DUAL_PHASE1 and IPM_SOLVE_CHOLESKY_DUAL_EQ.

The events bracket the assembly of S / K (kkt) and its bordered factorization (potrf); scripts/dual*_time.py
read them.  Recording them must not change a bit of the step: three one-step solves (max_iters = 1) with
timing on and the same three on a fresh problem with timing off give byte-equal directions, iterates and step
sizes, and the timed run reports count == 3 with finite positive kkt_ms and potrf_ms.

Shapes, from each method's grid: (n, m) = (17, 15) resp. (n, p, m) = (17, 3, 15), one tile and no K split, and the
smallest that takes the assembly's K split (n > 512), (520, 257) resp. (520, 130, 127); bounds "both".  Phase 2 (methods 6 and 8): t = 1e3, the point 0.9 of the way to the boundary.  Phase 1:
t = 1, the point x_f (frac 0) with s at 1 from the boundary of the phase-1 domain.
"""
import ctypes
import math

import pytest

import dual_eq_ref as Q
import dual_ph1_ref as P
import dual_ref as D

pytestmark = pytest.mark.gpu
ALPHA, BETA = 0.2, 0.6
STEPS = 3


def _dual(shape):
    import ipm355
    from ipm355 import _lib as L
    inst = D.instance(*shape, "both", 0.9)
    make = lambda fm: ipm355.NewtonSolverCholeskyDual(function_manager=fm, max_iters=1, epsilon=1e-5, alpha=ALPHA,
                                                      beta=BETA)
    return (lambda: inst.device(L.SOLVE_CHOLESKY_DUAL)), make, inst.x, None, 1e3


def _dual_ph1(shape):
    import ipm355
    from ipm355 import _lib as L
    pt = P.point(*shape, "both", 0.0, 1.0)
    make = lambda fm: ipm355.NewtonSolverCholeskyDual(function_manager=fm, max_iters=1, epsilon=1e-5, alpha=ALPHA,
                                                      beta=BETA, phase1_flag=False)
    return (lambda: pt.device(L.SOLVE_CHOLESKY_DUAL_PHASE1)), make, pt.x, None, 1.0


def _dual_eq(shape):
    import ipm355
    from ipm355 import _lib as L
    inst = Q.instance(*shape, "both", 0.9)
    make = lambda fm: ipm355.NewtonSolverCholeskyDualInfeasibleStart(inst.A, inst.b, inst.C, inst.d, fm, max_iters=1,
                                                                     epsilon=1e-5, alpha=ALPHA, beta=BETA)
    return (lambda: inst.device(L.SOLVE_CHOLESKY_DUAL_EQ)), make, inst.x, inst.v, 1e3


CASES = [("dual", _dual, (17, 15)), ("dual", _dual, (520, 257)),
         ("dual_ph1", _dual_ph1, (17, 15)), ("dual_ph1", _dual_ph1, (520, 257)),
         ("dual_eq", _dual_eq, (17, 3, 15)), ("dual_eq", _dual_eq, (520, 130, 127))]


def _three_steps(device, make, x0, v0, t):
    """STEPS one-step solves on a fresh problem, each from the point the one before left -> the bytes of
    (dx, dv, x, v) and the step size of every solve"""
    fm = device()
    fm.update_t(t)
    x = x0.copy()
    v = None if v0 is None else v0.copy()
    out = []
    for _ in range(STEPS):
        ns = make(fm)
        _, _, iters, _, _ = ns.solve(x, t, v0=v)
        assert iters == 1 and not ns.last_result.linalg_error
        rec = [fm.prob.last_direction().cpu().numpy().tobytes(), x.tobytes(), float(ns.trace[0][0])]
        if v is not None:
            rec += [fm.prob.last_dual_direction().cpu().numpy().tobytes(), v.tobytes()]
        out.append(rec)
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0] + "-" + "x".join(str(k) for k in c[2]))
def test_timing_mode_changes_no_bit_and_reports_every_step(case):
    from ipm355 import _lib as L
    _, setup, shape = case
    args = setup(shape)
    h = L.Handle.get(0)
    kkt, potrf, count = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    h.check(h.lib.ipm_set_timing(h.ptr, 1), h.ptr)
    try:
        timed = _three_steps(*args)
        h.check(h.lib.ipm_last_timings(h.ptr, ctypes.byref(kkt), ctypes.byref(potrf), ctypes.byref(count)), h.ptr)
    finally:
        h.check(h.lib.ipm_set_timing(h.ptr, 0), h.ptr)
    plain = _three_steps(*args)
    print(f"[{case[0]} {shape}] kkt_ms {kkt.value:.4g} potrf_ms {potrf.value:.4g} count {count.value:g}")
    assert timed == plain
    assert count.value == STEPS
    assert math.isfinite(kkt.value) and kkt.value > 0
    assert math.isfinite(potrf.value) and potrf.value > 0
