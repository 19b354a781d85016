"""NumPy restatement of the preconditioned conjugate-gradient Newton step
(linear_solve_method='cg', cg_preconditioner='jacobi').

``pcg`` follows scipy.sparse.linalg.cg (1.15) with its ``M`` argument operation by operation, for
a diagonal M given by its diagonal ``minv``: the convergence test ``||r|| < atol`` at the HEAD of
each iteration is on r (not on z), then ``z = minv * r``, ``rho = r.z``, ``p *= rho / rho_prev;
p += z`` (``p = z`` on the first iteration), ``q = A p``, ``alpha = rho / p.q``, ``x += alpha p``,
``r -= alpha q``; info = maxiter when the loop runs out.  In float64 it returns scipy's bits
(tests/test_pcg_ref.py).  ``newton_step`` is NewtonSolverCG.newton_linear_solve with
M = 1 / diag(A) for A = -H: pcg(-H, g, -1 / diag(H), x0 = the warm start).
"""
import numpy as np

import cg_ref


def pcg(A, b, minv, x0=None, maxiter=50, rtol=1e-5, dtype=np.float64, trace=None):
    """-> (x, info, iters).  trace (a list): ||r|| / ||b|| at every convergence test."""
    A = np.asarray(A, dtype=dtype)
    b = np.asarray(b, dtype=dtype)
    minv = np.asarray(minv, dtype=dtype)
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
        z = minv * r
        rho_cur = np.dot(r, z)
        if iteration > 0:
            beta = rho_cur / rho_prev
            p *= beta
            p += z
        else:
            p = np.empty_like(r)
            p[:] = z[:]
        q = A.dot(p)
        alpha = rho_cur / np.dot(p, q)
        x += alpha * p
        r -= alpha * q
        rho_prev = rho_cur
    return x, maxiter, maxiter


def jacobi(H):
    """the diagonal of M = 1 / diag(H)"""
    return 1.0 / np.diag(np.asarray(H)).copy()


def newton_step(H, x, g, maxiter=50, dtype=np.float64):
    """NewtonSolverCG.newton_linear_solve with M = 1 / diag(-H) -> (xstep, info, iters, took_scaled_branch)"""
    x0, scaled = cg_ref.warm_start(H, x, g)
    xs, info, iters = pcg(-np.asarray(H), g, -jacobi(H), x0=x0, maxiter=maxiter, dtype=dtype)
    return xs, info, iters, scaled


def scaled_system(K, b0, seed):
    """H = S K S, b = S b0 with S = diag(10 ** U(-3, 3)): K in badly chosen units -> (H, b, sigma)"""
    n = K.shape[0]
    sigma = 10.0 ** np.random.default_rng(seed).uniform(-3, 3, n)
    H = sigma[:, None] * K * sigma[None, :]
    return (H + H.T) / 2, sigma * b0, sigma
