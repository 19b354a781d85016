"""Helpers for the -m gpu tests (device tensors + C-ABI calls)."""
import ctypes

import numpy as np


def handle():
    from ipm355 import _lib
    return _lib.Handle.get(0)


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def colmajor_lower(Hmem, n):
    """device buffer laid out column-major with ld = Hmem.shape[1] -> dense lower-tri matrix"""
    M = host(Hmem).T[:n, :n]
    return np.tril(M)


def syrk(X, w, n, ldh=None, beta=0.0, H0=None, alpha=1.0):
    import torch
    from ipm355 import _lib as L
    h = handle()
    k = X.shape[0]
    ldh = ldh or n
    Xd = dev(X)
    wd = dev(w) if w is not None else None
    H = dev(H0) if H0 is not None else torch.zeros((n, ldh), dtype=torch.float64, device="cuda")
    h.check(h.lib.ipm_syrk(h.ptr, n, k, L.dptr(Xd), X.shape[1], L.dptr(wd), alpha, beta, L.dptr(H), ldh), h.ptr)
    return H


def potrf(Hmem, n, ldh, ncols=None):
    from ipm355 import _lib as L
    h = handle()
    info = ctypes.c_int(-7)
    if ncols is None:
        rc = h.lib.ipm_potrf(h.ptr, n, L.dptr(Hmem), ldh, ctypes.byref(info))
    else:
        rc = h.lib.ipm_potrf_partial(h.ptr, n, ncols, L.dptr(Hmem), ldh, ctypes.byref(info))
    return rc, info.value


def devnan(shape):
    """a NaN-filled device tensor: anything a kernel reads outside its operands shows in its output"""
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def gemv(trans, rows, cols, alpha, M, ldm, x, beta, y):
    """raw ipm_gemv on device tensors (any views): the return code, unchecked"""
    from ipm355 import _lib as L
    h = handle()
    return h.lib.ipm_gemv(h.ptr, int(trans), rows, cols, alpha, L.dptr(M), ldm, L.dptr(x), beta, L.dptr(y))


def gemm_tn(M, N, K, alpha, A, lda, B, ldb, beta, C, ldc):
    from ipm355 import _lib as L
    h = handle()
    return h.lib.ipm_gemm_tn(h.ptr, M, N, K, alpha, L.dptr(A), lda, L.dptr(B), ldb, beta, L.dptr(C), ldc)


def transpose(rows, cols, src, ldi, dst, ldo):
    from ipm355 import _lib as L
    h = handle()
    return h.lib.ipm_transpose(h.ptr, rows, cols, L.dptr(src), ldi, L.dptr(dst), ldo)


def copy(dst, src, n):
    from ipm355 import _lib as L
    h = handle()
    return h.lib.ipm_copy(h.ptr, L.dptr(dst), L.dptr(src), n)


def potrs(Lmem, n, ldl, B):
    from ipm355 import _lib as L
    h = handle()
    Bd = dev(B.reshape(n, -1))
    h.check(h.lib.ipm_potrs(h.ptr, n, Bd.shape[1], L.dptr(Lmem), ldl, L.dptr(Bd), Bd.shape[1]), h.ptr)
    return host(Bd)


def getrf(A, n, lda, piv):
    """raw ipm_getrf on device tensors: A column-major (lda), piv int64 (None: a null pointer)
    -> (rc, info)"""
    from ipm355 import _lib as L
    h = handle()
    info = ctypes.c_int(-7)
    rc = h.lib.ipm_getrf(h.ptr, n, L.dptr(A), lda, L.dptr(piv), ctypes.byref(info))
    return rc, info.value


def getrs(LU, n, lda, piv, B, nrhs, ldb):
    """raw ipm_getrs on device tensors: B row-major n x nrhs (ldb), in place -> rc (synchronised)"""
    import torch
    from ipm355 import _lib as L
    h = handle()
    rc = h.lib.ipm_getrs(h.ptr, n, nrhs, L.dptr(LU), lda, L.dptr(piv), L.dptr(B), ldb)
    torch.cuda.synchronize()
    return rc


def lstsq_sym(A, n, lda, B, nrhs, ldb):
    """raw ipm_lstsq_sym on device tensors: A symmetric (lda) <- V^T, B row-major (ldb) <- A^+ B
    -> (rc, info)"""
    from ipm355 import _lib as L
    h = handle()
    info = ctypes.c_int(-7)
    rc = h.lib.ipm_lstsq_sym(h.ptr, n, nrhs, L.dptr(A), lda, L.dptr(B), ldb, ctypes.byref(info))
    return rc, info.value
