"""Golden vectors for the factored QP (QPSolver(P_factor=F, P_diag=rho, linear_solve_method='cholesky_dual')),
written by running the REFERENCE itself on the CPU (build container only).

    PYTHONDONTWRITEBYTECODE=1 OPENBLAS_NUM_THREADS=1 python tests/golden/make_golden_dual_qp.py

The reference is imported read-only with an empty ``cvxpy`` stub, as make_golden_cg.py does; only inputs and
recorded results are written (tests/golden/dual_qp_*.npz).  The reference knows dense P only: its own QPSolver
('cholesky') is run on P = diag(rho) + F'F formed here in fp64, and the fixture stores the FACTORED inputs (F, rho,
q, C, d, bounds, x0 = the generator's strictly feasible point: no phase 1), the reference's value, x*, iteration lists, and its own sensitivity to a 1e-15 relative
perturbation of q and of d (sens_xstar_rel, sens_value_rel, sens_iters_stable: whether every re-run kept the lists).
Two instances: dual_qp_factored (n = 96, m = 24, k = 12) and dual_qp_diagonal (n = 120, m = 30, k = 0: P = diag(rho)).
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


def run_case(name, n, m, k, rho, seed, extra):
    inst = problems.qp_factor_box(n, m, k, seed=seed, rho=rho, with_xf=True)
    xf = inst.pop("xf")
    F, r = inst.pop("P_factor"), inst.pop("P_diag")
    P = F.T @ F if F is not None else np.zeros((n, n))
    P[np.diag_indices(n)] += r
    dense = dict(inst, P=P, x0=xf.copy(), **extra)
    val, xs, outer, inner = _run(dense)
    rng = np.random.default_rng(seed + 100)
    wx = wv = 0.0
    stable = True
    for key in ("q", "d"):
        for _ in range(4):
            kw = {kk: _cp(v) for kk, v in dense.items()}
            kw[key] = kw[key] * (1 + 1e-15 * rng.standard_normal(kw[key].shape))
            v2, x2, o2, i2 = _run(kw)
            wx = max(wx, float(np.linalg.norm(x2 - xs) / np.linalg.norm(xs)))
            wv = max(wv, abs(v2 - val) / max(abs(val), 1e-300))
            stable = stable and i2 == inner and o2 == outer
    out = {"kind": np.array("QP"), "in_q": inst["q"], "in_C": inst["C"], "in_d": inst["d"],
           "in_lower_bound": np.array(inst["lower_bound"]), "in_upper_bound": np.array(inst["upper_bound"]),
           "in_P_diag": r, "in_x0": xf}
    if F is not None:
        out["in_P_factor"] = F
    for kk, v in extra.items():
        out["in_" + kk] = np.array(v)
    out.update(value=np.array(val), xstar=xs, outer_iters=np.array(outer), inner_iters=np.array(inner),
               sens_xstar_rel=np.array(wx), sens_value_rel=np.array(wv),
               sens_iters_stable=np.array(stable))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(f"{name}: value={val!r} outer={outer} inner={inner} sens x* {wx:.1e} value {wv:.1e} "
          f"iters stable {stable}")


def main():
    run_case("dual_qp_factored", 96, 24, 12, "pow2", 3, dict(problems.QP_KWARGS))
    run_case("dual_qp_diagonal", 120, 30, 0, "pow2", 4, dict(problems.QP_KWARGS))


if __name__ == "__main__":
    main()
