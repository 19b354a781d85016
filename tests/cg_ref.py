"""NumPy restatement of the conjugate-gradient Newton step (linear_solve_method='cg').

``cg`` follows scipy.sparse.linalg.cg (1.15) operation by operation -- atol = max(0, rtol ||b||),
b == 0 -> x = b, r = b - A x0 only when x0 has a non-zero entry, the convergence test ``||r|| <
atol`` at the HEAD of each iteration, ``p *= beta; p += r``, ``x += alpha p; r -= alpha q`` and
info = maxiter when the loop runs out -- so that in float64 it returns scipy's bits
(tests/test_cg_ref.py).  Any dtype NumPy has can be passed (np.longdouble for a reference the
fp64 runs are measured against).  ``warm_start`` is NewtonSolver.py:379-383; ``newton_step`` the
whole ``newton_linear_solve`` of NewtonSolverCG: cg(-H, g, x0, maxiter).
"""
import numpy as np


def cg(A, b, x0=None, maxiter=50, rtol=1e-5, dtype=np.float64, trace=None):
    """-> (x, info, iters).  trace (a list): ||r|| / ||b|| at every convergence test."""
    A = np.asarray(A, dtype=dtype)
    b = np.asarray(b, dtype=dtype)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=dtype)
    bnrm2 = np.linalg.norm(b)
    atol = max(0.0, dtype(rtol) * bnrm2)
    if bnrm2 == 0:
        return b.copy(), 0, 0
    r = b - A.dot(x) if x.any() else b.copy()
    rho_prev, p = None, None
    for iteration in range(maxiter):
        rn = np.linalg.norm(r)
        if trace is not None:
            trace.append(float(rn / bnrm2))
        if rn < atol:
            return x, 0, iteration
        rho_cur = np.dot(r, r)
        if iteration > 0:
            beta = rho_cur / rho_prev
            p *= beta
            p += r
        else:
            p = np.empty_like(r)
            p[:] = r[:]
        q = A.dot(p)
        alpha = rho_cur / np.dot(p, q)
        x += alpha * p
        r -= alpha * q
        rho_prev = rho_cur
    return x, maxiter, maxiter


def warm_start(H, x, g):
    """NewtonSolver.py:379-383 -> (x0, took_scaled_branch)"""
    dc = np.dot(x, g)
    if dc < 0:
        return -dc * x / np.dot(x, np.dot(H, x)), True
    return np.zeros_like(x), False


def newton_step(H, x, g, maxiter=50, dtype=np.float64):
    """NewtonSolverCG.newton_linear_solve -> (xstep, info, iters, took_scaled_branch)"""
    x0, scaled = warm_start(H, x, g)
    xs, info, iters = cg(-np.asarray(H), g, x0=x0, maxiter=maxiter, dtype=dtype)
    return xs, info, iters, scaled


def clustered(n, seed=0):
    """Q diag(lam) Q^T, symmetrised, lam drawn from six values: CG ends in exactly six iterations
    -> (H, lam)"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = rng.choice(np.array([1.0, 2.5, 7.0, 19.0, 40.0, 100.0]), n)
    lam[:6] = [1.0, 2.5, 7.0, 19.0, 40.0, 100.0]     # every value present
    H = (Q * lam) @ Q.T
    return (H + H.T) / 2, lam


def ill_conditioned(n, seed=0):
    """Q diag(logspace(0, 6, n)) Q^T, symmetrised -> (H, lam)"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0, 6, n)
    H = (Q * lam) @ Q.T
    return (H + H.T) / 2, lam
