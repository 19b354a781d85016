"""Golden vectors for the factored QP with equality rows (QPSolver(P_factor=F, P_diag=rho, A=A, b=b,
linear_solve_method='cholesky_dual_eq')), written by running the REFERENCE itself on the CPU (build container only).

    PYTHONDONTWRITEBYTECODE=1 OPENBLAS_NUM_THREADS=1 python tests/golden/make_golden_dual_qp_eq.py

The reference is imported read-only with an empty ``cvxpy`` stub, as make_golden_dual_qp.py does; only inputs and
recorded results are written (tests/golden/dual_qp_eq_*.npz).  The reference knows dense P only: its own QPSolver
('cholesky', infeasible start: block elimination) is run on P = diag(rho) + F'F formed here in fp64 with A and b, and
the fixture stores the FACTORED inputs (F, rho, q, A, b, C, d, bounds, x0 = a strictly feasible point: no phase 1),
the reference's value, x*, iteration lists, and its own sensitivity to a 1e-15 relative perturbation of q and of b
(sens_xstar_rel, sens_value_rel, sens_iters_stable: whether every re-run kept the lists).
Two instances: dual_qp_eq_factored (n = 96, m = 24, k = 12, p = 8, problems.qp_factor_eq_box) and dual_qp_eq_budget
(n = 120, no C, k = 10, one budget row 1'x = 1, x >= 0 only: a long-only factor-model portfolio, x0 = 1 / n).
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

from QPSolver import QPSolver as RefQP  # noqa: E402

from ipm355 import problems  # noqa: E402


def _cp(v):
    return np.array(v, copy=True) if isinstance(v, np.ndarray) else v


def _run(dense):
    s = RefQP(check_cvxpy=False, suppress_print=True, linear_solve_method="cholesky",
              **{k: _cp(v) for k, v in dense.items()})
    val = s.solve()
    return float(val), np.asarray(s.xstar, dtype=np.float64), int(s.outer_iters), list(s.inner_iters)


def run_case(name, inst, x0, extra):
    n = len(inst["q"])
    inst = {k: v for k, v in inst.items() if v is not None}
    F, r = inst.pop("P_factor"), inst.pop("P_diag")
    P = F.T @ F
    P[np.diag_indices(n)] += r
    dense = dict(inst, P=P, x0=x0.copy(), **extra)
    dense.setdefault("upper_bound", None)
    val, xs, outer, inner = _run(dense)
    rng = np.random.default_rng(n + 100)
    wx = wv = 0.0
    stable = True
    for key in ("q", "b"):
        for _ in range(4):
            kw = {kk: _cp(v) for kk, v in dense.items()}
            kw[key] = kw[key] * (1 + 1e-15 * rng.standard_normal(kw[key].shape))
            v2, x2, o2, i2 = _run(kw)
            wx = max(wx, float(np.linalg.norm(x2 - xs) / np.linalg.norm(xs)))
            wv = max(wv, abs(v2 - val) / max(abs(val), 1e-300))
            stable = stable and i2 == inner and o2 == outer
    out = {"kind": np.array("QP"), "in_P_factor": F, "in_P_diag": r, "in_x0": x0}
    for kk, v in list(inst.items()) + list(extra.items()):
        out["in_" + kk] = np.array(v)
    out.update(value=np.array(val), xstar=xs, outer_iters=np.array(outer), inner_iters=np.array(inner),
               sens_xstar_rel=np.array(wx), sens_value_rel=np.array(wv),
               sens_iters_stable=np.array(stable))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(f"{name}: value={val!r} outer={outer} inner={inner} sens x* {wx:.1e} value {wv:.1e} "
          f"iters stable {stable} |Ax-b| {np.linalg.norm(inst['A'] @ xs - inst['b']):.1e}")


def main():
    inst = problems.qp_factor_eq_box(96, 24, 12, 8, seed=3, rho="pow2", with_xf=True)
    xf = inst.pop("xf")
    run_case("dual_qp_eq_factored", inst, xf, dict(problems.QP_KWARGS))
    # long-only portfolio: factor loadings F (10 x 120), specific variances rho, expected returns -q, budget row
    n = 120
    inst = problems.qp_factor_eq_box(n, 0, 10, 1, seed=4, rho="pow2")
    inst.update(A=np.ones((1, n)), b=np.ones(1), lower_bound=0, upper_bound=None)
    run_case("dual_qp_eq_budget", inst, np.full(n, 1.0 / n), dict(problems.QP_KWARGS))


if __name__ == "__main__":
    main()
