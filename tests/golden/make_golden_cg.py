"""Golden vectors for linear_solve_method='cg', written by running the REFERENCE itself on the CPU
(build container only).

    PYTHONDONTWRITEBYTECODE=1 OPENBLAS_NUM_THREADS=1 python tests/golden/make_golden_cg.py

The reference is imported read-only with an empty ``cvxpy`` stub, as make_golden.py does; only
inputs and recorded results are written (tests/golden/cg_*.npz).  Each instance is solved three
ways -- 'cholesky', 'cg' at the fixture's cap and 'cg' at twice the cap -- and the fixture keeps the
'cg'-at-the-cap run as the expected result together with

    value_tol = 10 x the largest pairwise spread of the three values, floor 1e-9 |value|

(a truncated-Newton iterate moves about as much with another summation order as with another cap,
so the reference's own spread over caps is the yardstick; the factor 10 is the margin).  The
generator refuses to write a fixture whose three values do not all sit inside value_tol of the
stored one, or whose three runs differ in outer iterations.
"""
from __future__ import annotations

import os
import sys
import types

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "interiorpoint-gpu_amd"))
sys.modules.setdefault("cvxpy", types.ModuleType("cvxpy"))
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

from LPSolver import LPSolver as RefLP  # noqa: E402
from QPSolver import QPSolver as RefQP  # noqa: E402
from SOCPSolver import SOCPSolver as RefSOCP  # noqa: E402

from ipm355 import problems  # noqa: E402


def _cp(v):
    if isinstance(v, list):
        return [np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in v]
    return np.array(v, copy=True) if isinstance(v, np.ndarray) else v


def _run(cls, kwargs, method, cap):
    kw = {k: _cp(v) for k, v in kwargs.items()}
    s = cls(check_cvxpy=False, suppress_print=True, linear_solve_method=method, max_cg_iters=cap, **kw)
    val = s.solve()
    return float(val), np.asarray(s.xstar, dtype=np.float64), int(s.outer_iters), list(s.inner_iters)


def run_case(name, cls, kind, kwargs, cap):
    runs = {"cholesky": _run(cls, kwargs, "cholesky", cap), "cg": _run(cls, kwargs, "cg", cap),
            "cg2": _run(cls, kwargs, "cg", 2 * cap)}
    vals = np.array([runs[k][0] for k in ("cholesky", "cg", "cg2")])
    spread = float(np.max(np.abs(vals[:, None] - vals[None, :])))
    val = runs["cg"][0]
    tol = max(10.0 * spread, 1e-9 * abs(val))
    outers = {runs[k][2] for k in runs}
    assert np.all(np.abs(vals - val) <= tol), (name, vals, tol)
    assert len(outers) == 1, (name, outers)
    assert np.isfinite(tol)
    out = {"kind": np.array(kind), "max_cg_iters": np.array(cap)}
    for k, v in kwargs.items():
        if v is None:
            continue
        if isinstance(v, list):
            out[f"in_{k}_count"] = np.array(len(v))
            for i, a in enumerate(v):
                out[f"in_{k}_{i}"] = np.asarray(a)
        else:
            out["in_" + k] = np.asarray(v)
    out.update(value=np.array(val), xstar=runs["cg"][1], outer_iters=np.array(runs["cg"][2]),
               value_tol=np.array(tol), ref_values=vals, ref_spread=np.array(spread),
               ref_inner_iters_cg=np.array(runs["cg"][3]))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(f"{name}: cholesky {vals[0]!r} cg@{cap} {vals[1]!r} cg@{2 * cap} {vals[2]!r} spread {spread:.2e} "
          f"(rel {spread / abs(val):.1e}) value_tol {tol:.2e} outer {runs['cg'][2]} inner {runs['cg'][3]}")


def main():
    run_case("cg_qp_n40", RefQP, "QP", problems.qp_ineq_box(n=40, m=20, seed=3), 50)
    run_case("cg_qp_n130", RefQP, "QP", problems.qp_ineq_box(n=130, m=64, seed=3), 1000)
    run_case("cg_lp_n40", RefLP, "LP", problems.lp_ineq_box(n=40, m=20, seed=3), 400)
    run_case("cg_socp_n24", RefSOCP, "SOCP", problems.socp_cones(n=24, K=4, mi=3, seed=3, eq=0), 200)


if __name__ == "__main__":
    main()
