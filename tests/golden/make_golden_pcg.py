"""Golden vectors for linear_solve_method='cg' with cg_preconditioner='jacobi', written by running
the REFERENCE itself on the CPU (build container only).

    PYTHONDONTWRITEBYTECODE=1 OPENBLAS_NUM_THREADS=1 python tests/golden/make_golden_pcg.py

The reference is imported read-only exactly as make_golden_cg.py does (this module reuses its
set-up).  The one addition: in the namespace of the reference's NewtonSolver module the name
``scipy`` is bound to a stand-in whose ``scipy.sparse.linalg.cg`` passes
``M = LinearOperator(r -> r / diag(A))`` to the real function -- scipy's own preconditioner
argument, which the reference never uses.  The reference's files and scipy itself are not touched.

Each instance is solved four ways: 'cholesky', preconditioned 'cg' at the fixture's cap and at
twice the cap, and plain 'cg' (no M) at the cap.  The fixture keeps the preconditioned run at the
cap as the expected result, with make_golden_cg.py's rule

    value_tol = 10 x the largest pairwise spread of the first three values, floor 1e-9 |value|

and ``plain_value``, what the reference returns without the preconditioner.  The generator refuses
to write a fixture whose first three runs differ in outer iterations, or (unless the instance waives
it) whose plain-CG value is closer than 1e4 value_tol to the preconditioned one: the scaled
instances are there because plain CG gets them wrong.
"""
from __future__ import annotations

import os

import make_golden_cg as G        # the reference on sys.path, RefLP / RefQP, _cp, problems
import numpy as np
import scipy
import scipy.sparse.linalg as spla

import NewtonSolver as RefNS      # the reference's module (on sys.path through make_golden_cg)

from ipm355 import problems

HERE = os.path.dirname(os.path.abspath(__file__))
_REAL_SCIPY = RefNS.scipy


def _cg_jacobi(A, b, x0=None, **kw):
    dg = np.diag(np.asarray(A)).copy()
    M = spla.LinearOperator(A.shape, matvec=lambda r: r / dg, dtype=np.float64)
    return spla.cg(A, b, x0=x0, M=M, **kw)


class _Over:
    """a module seen through: the given names replaced, every other attribute the module's own
    (phase 1 and the Cholesky runs go on calling scipy.linalg)"""

    def __init__(self, mod, **over):
        self._mod = mod
        self.__dict__.update(over)

    def __getattr__(self, name):
        return getattr(self._mod, name)


_PCG_SCIPY = _Over(_REAL_SCIPY, sparse=_Over(_REAL_SCIPY.sparse, linalg=_Over(spla, cg=_cg_jacobi)))


def _run(cls, kwargs, method, cap, jacobi):
    RefNS.scipy = _PCG_SCIPY if jacobi else _REAL_SCIPY
    try:
        kw = {k: G._cp(v) for k, v in kwargs.items()}
        s = cls(check_cvxpy=False, suppress_print=True, linear_solve_method=method, max_cg_iters=cap, **kw)
        val = s.solve()
        return float(val), np.asarray(s.xstar, dtype=np.float64), int(s.outer_iters), list(s.inner_iters)
    finally:
        RefNS.scipy = _REAL_SCIPY


def run_case(name, cls, kind, kwargs, cap, sigma=None, waive_plain=False):
    runs = {"cholesky": _run(cls, kwargs, "cholesky", cap, False), "pcg": _run(cls, kwargs, "cg", cap, True),
            "pcg2": _run(cls, kwargs, "cg", 2 * cap, True)}
    plain = _run(cls, kwargs, "cg", cap, False)
    vals = np.array([runs[k][0] for k in ("cholesky", "pcg", "pcg2")])
    spread = float(np.max(np.abs(vals[:, None] - vals[None, :])))
    val = runs["pcg"][0]
    tol = max(10.0 * spread, 1e-9 * abs(val))
    outers = {runs[k][2] for k in runs}
    assert np.isfinite(tol) and np.all(np.abs(vals - val) <= tol), (name, vals, tol)
    assert len(outers) == 1, (name, outers)
    gap = abs(plain[0] - val)
    if waive_plain:
        print(f"{name}: well-scaled instance, the plain-CG condition is waived (plain CG off by {gap:.2e})")
    else:
        assert gap >= 1e4 * tol, (name, plain[0], val, tol)
    out = {"kind": np.array(kind), "max_cg_iters": np.array(cap), "cg_preconditioner": np.array("jacobi"),
           "plain_waived": np.array(bool(waive_plain))}
    if sigma is not None:
        out["sigma"] = np.asarray(sigma)
    for k, v in kwargs.items():
        if v is not None:
            out["in_" + k] = np.asarray(v)
    out.update(value=np.array(val), xstar=runs["pcg"][1], outer_iters=np.array(runs["pcg"][2]),
               value_tol=np.array(tol), ref_values=vals, ref_spread=np.array(spread),
               ref_inner_iters_cg=np.array(runs["pcg"][3]), plain_value=np.array(plain[0]),
               plain_outer_iters=np.array(plain[2]))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(f"{name}: cholesky {vals[0]!r} pcg@{cap} {vals[1]!r} pcg@{2 * cap} {vals[2]!r} spread {spread:.2e} "
          f"value_tol {tol:.2e} plain cg@{cap} {plain[0]!r} (off by {gap:.3g}) outer {runs['pcg'][2]} "
          f"inner {runs['pcg'][3]}")


def _scaled_lp(n, m):
    sigma = 10.0 ** np.random.default_rng(7).uniform(-2, 2, n)
    return problems.scale_variables(problems.lp_ineq_box(n=n, m=m, seed=3), sigma), sigma


def main():
    assert scipy is _REAL_SCIPY
    inst, sigma = _scaled_lp(40, 20)
    run_case("pcg_lp_n40_scaled", G.RefLP, "LP", inst, 100, sigma=sigma)
    inst, sigma = _scaled_lp(200, 50)
    run_case("pcg_lp_n200_scaled", G.RefLP, "LP", inst, 200, sigma=sigma)
    run_case("pcg_qp_n130", G.RefQP, "QP", problems.qp_ineq_box(n=130, m=64, seed=3), 1000, waive_plain=True)


if __name__ == "__main__":
    main()
