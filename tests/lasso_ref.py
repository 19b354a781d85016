"""Long-double references of the batched ADMM Lasso's operations (ipm_lasso.hip), each with the
entry-by-entry error bound it implies, and the helpers the Lasso kernel tests share.

Shared by tests/test_gpu_lasso_kernels.py (-m gpu: every ipm_lasso_* entry point against these)
and tests/test_lasso_ref.py (no GPU: the fp64 oracle and a plain fp64 NumPy step sit inside a
quarter of the same bounds).  A plain module: it reads nothing but its arguments.

All references take the fp64 inputs as they are and evaluate in np.longdouble, with np.maximum
semantics in prox (a NaN stays a NaN).

Error bounds (the convention of tests/test_gpu_kernels.py: an fp64 sum of products in another order
differs by at most 64 eps sum|terms|).  One ADMM step, T(i, s) = sum_k |Qs[k, i]| |W[k, s]|:
  x'      bx = 64 eps (T + |bA|)
  alpha'  balpha = bx + 4 eps (|x'| + |u| + |eta|)       prox is 1-Lipschitz: the threshold is no edge
  u'      bu = bx + balpha + 4 eps (|u| + |x'| + |alpha'|)
  W'      bW = bu + balpha + eps |W'|
  a sum of squares sum r_i^2 whose entries carry bounds d_i:  sum (2 |r_i| d_i + d_i^2) + 64 eps sum r_i^2
  with d = bx + balpha + eps |r| for r = x' - alpha', |rho| (balpha + dalpha) + 2 eps |r| for
  r = rho (alpha' - alpha), balpha for alpha' and bu for u'.
Inputs that carry bounds of their own (dW, dalpha, du: the second and later iterations of a loop)
add, exactly propagated: dx = |Qs|^T dW to x', dx + du to alpha' (1-Lipschitz in x' + u), and
du + dx + (dx + du) to u'; W' takes the sum of the u' and alpha' terms.
The loss: each residual (A alpha - b)_r carries 64 eps sum_i |A_ri| |alpha_i| + 2 eps (|A alpha|_r + |b_r|),
the sum of squares as above, times 1 / (2 m); the l1 term 64 eps |reg| sum |alpha|; 4 eps on the
final operations.
"""
from __future__ import annotations

import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
LT = 32                     # the step's tile: 32 rows x 32 problems


# --------------------------------------------------------------------------- comparing
def ratio(got, ref, bound):
    """max |got - ref| / bound over the entries; a NaN of the reference must be a NaN of `got`, an
    infinity the same infinity, and a non-finite `got` where the reference is finite counts as
    an infinite error (as does any error where the bound is zero)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    fin = np.isfinite(ref.astype(np.float64))
    r = np.zeros(ref.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got.astype(LD) - ref.astype(LD)).astype(np.float64)
        q = np.where(err == 0.0, 0.0, err / bound)
    q = np.where(np.isfinite(got), q, np.inf)
    r[fin] = q[fin]
    nf = ~fin
    same = (np.isnan(ref.astype(np.float64)) & np.isnan(got)) | (ref.astype(np.float64) == got)
    r[nf] = np.where(same[nf], 0.0, np.inf)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def sumsq_bound(r, d):
    """bound of an fp64 sum (any order, fma or not) of r_i^2 whose entries carry the bounds d_i"""
    r = np.abs(np.asarray(r, dtype=LD))
    d = np.asarray(d, dtype=LD)
    return float((2 * r * d + d * d).sum() + 64 * EPS * (r * r).sum())


# --------------------------------------------------------------------------- one ADMM step
def prox(v, eta, positive, add_bias):
    """LassoSolver.prox with np.maximum (NaN propagates); eta broadcasts along rows"""
    out = np.maximum(v - eta, 0)
    if not positive:
        out = out - np.maximum(-v - eta, 0)
    if add_bias:
        out[0] = v[0]
    return out


def admm_step(Qs, W, bA, eta, x, alpha, u, rho, positive=0, add_bias=0, dual_form=0, ba_bcast=0, eta_bcast=0,
              dtype=LD, dW=None, dalpha=None, du=None):
    """One ADMM step from an arbitrary state.  Qs: (n, n) k-major (row k holds Qs(i, k)); W, x,
    alpha, u: (n, S); bA: (n, S) or (n, 1) with ba_bcast; eta: (S,) or (1,) with eta_bcast.  x is the
    state's x, which the step overwrites without reading.  dW / dalpha / du: entry bounds the inputs
    already carry (None: exact inputs).  Returns a dict: x, alpha, u, W, sums (4,) in `dtype`, and
    their bounds bx, balpha, bu, bW, bsums as float64."""
    n, S = W.shape
    assert Qs.shape == (n, n) and alpha.shape == (n, S) and u.shape == (n, S) and x.shape == (n, S)
    bA = np.asarray(bA).reshape(n, -1)
    eta = np.asarray(eta).reshape(-1)
    assert bA.shape[1] == (1 if ba_bcast else S) and eta.shape[0] == (1 if eta_bcast else S)
    t = lambda a: np.asarray(a, dtype=dtype)    # noqa: E731
    Qt, Wt, bAt, etat, at, ut = t(Qs).T, t(W), t(bA), t(eta), t(alpha), t(u)
    with np.errstate(invalid="ignore"):
        xn = bAt + Qt @ Wt
        v = xn + ut
        an = prox(v, etat[None, :], positive, add_bias)
        un = ut + (xn - an) if dual_form else (ut + xn) - an
        Wn = un - an
        r1, r2 = xn - an, t(rho) * (an - at)
        sums = np.array([(r1 * r1).sum(), (r2 * r2).sum(), (an * an).sum(), (un * un).sum()], dtype=dtype)
        # bounds (float64 is plenty for them)
        f = lambda a: np.abs(np.asarray(a, dtype=np.float64))   # noqa: E731
        T = f(Qs).T @ f(W)
        z = np.zeros((n, S))
        dW, dalpha, du = (z if d is None else np.asarray(d, dtype=np.float64) for d in (dW, dalpha, du))
        dx = f(Qs).T @ dW
        bx = 64 * EPS * (T + f(bA)) + dx
        balpha = bx + 4 * EPS * (f(xn) + f(u) + f(eta)[None, :]) + du
        bu = bx + balpha + 4 * EPS * (f(u) + f(xn) + f(an)) + du
        bW = bu + balpha + EPS * f(Wn)
        bsums = np.array([sumsq_bound(r1, bx + balpha + EPS * f(r1)),
                          sumsq_bound(r2, abs(float(rho)) * (balpha + dalpha) + 2 * EPS * f(r2)),
                          sumsq_bound(an, balpha), sumsq_bound(un, bu)])
    return dict(x=xn, alpha=an, u=un, W=Wn, sums=sums, bx=bx, balpha=balpha, bu=bu, bW=bW, bsums=bsums)


def admm_steps(k, Qs, W, bA, eta, x, alpha, u, rho, **flags):
    """k steps in long double, each iteration's bounds = its one-step bounds + the propagated
    bounds of its inputs.  Returns the list of the k step dicts."""
    out = []
    dW = dalpha = du = None
    for _ in range(k):
        st = admm_step(Qs, W, bA, eta, x, alpha, u, rho, dW=dW, dalpha=dalpha, du=du, **flags)
        out.append(st)
        # the next step's inputs: the long-double state itself (the device's fp64 state is within
        # the bounds of it, which is what dW / dalpha / du say)
        W, x, alpha, u = st["W"], st["x"], st["alpha"], st["u"]
        dW, dalpha, du = st["bW"], st["balpha"], st["bu"]
    return out


def state(n, S, seed, positive=0, ba_bcast=0, eta_bcast=0):
    """A seeded random non-zero state: Qs ~ U(-1, 1) / sqrt(n), bA ~ U(-1, 1), x, alpha, u ~ U(-2, 2),
    W = u - alpha (exact in fp64 or not: the step takes W as given), rho = 0.4.  eta is placed so
    that every tile of three or more entries has all three prox branches: with e the entry's
    row-major index inside its tile, e mod 5 = 0 / 1 / 2 get v = x' + u at eta + 1.5, -eta - 1.5 and
    eta / 4 (above, below, inside), by setting u there from the fp64 x'; the other two fifths stay
    random."""
    rng = np.random.default_rng(seed)
    Qs = rng.uniform(-1, 1, (n, n)) / np.sqrt(n)
    bA = rng.uniform(-1, 1, (n, 1 if ba_bcast else S))
    x, alpha, u = (rng.uniform(-2, 2, (n, S)) for _ in range(3))
    eta = rng.uniform(0.3, 0.9, 1 if eta_bcast else S)
    # moving u moves W and with it every x' of the column by about 0.45 of the move: twelve passes
    # of the fixed point leave x' + u within 1e-4 of the targets, whose margins are 0.2 and more
    sl = np.arange(S) % LT
    width = np.minimum(LT, S - (np.arange(S) - sl))          # columns of the entry's tile
    c = ((np.arange(n) % LT)[:, None] * width[None, :] + sl[None, :]) % 5
    et = np.broadcast_to(eta[None, :], (n, S))
    target = np.where(c == 0, et + 1.5, np.where(c == 1, -et - 1.5, 0.25 * et))
    for _ in range(12):
        xn = bA + Qs.T @ (u - alpha)
        u = np.where(c < 3, target - xn, u)
    return dict(Qs=Qs, W=u - alpha, bA=bA, eta=eta, x=x, alpha=alpha, u=u, rho=0.4)


def branches(st, step, add_bias=0):
    """per tile, how many entries took (above, below, inside) in the reference step"""
    n, S = st["u"].shape
    v = np.asarray(step["x"] + st["u"].astype(LD), dtype=np.float64)
    et = np.broadcast_to(np.asarray(st["eta"]).reshape(1, -1), (n, S))
    out = []
    for i0 in range(0, n, LT):
        for s0 in range(0, S, LT):
            vv, ee = v[i0:i0 + LT, s0:s0 + LT], et[i0:i0 + LT, s0:s0 + LT]
            out.append((int((vv > ee).sum()), int((vv < -ee).sum()), int((np.abs(vv) <= ee).sum())))
    return out


# --------------------------------------------------------------------------- loss
def loss(A, alpha, b, reg, absm, add_bias, b_bcast=0, reg_bcast=0, cols=None, out=None, dtype=LD):
    """per problem 1/(2m) sum_r (A alpha - b)_r^2 + reg sum_i g(alpha_i), g = |.| with absm, row 0
    skipped with add_bias; result s goes to out[cols[s]] (out: the prior contents, or zeros).
    Returns (values, bounds), both of out's shape; untouched entries keep out's value, bound 0."""
    m, n = A.shape
    S = alpha.shape[1]
    b = np.asarray(b).reshape(m, -1)
    reg = np.asarray(reg).reshape(-1)
    assert b.shape[1] == (1 if b_bcast else S) and reg.shape[0] == (1 if reg_bcast else S)
    t = lambda a: np.asarray(a, dtype=dtype)    # noqa: E731
    f = lambda a: np.abs(np.asarray(a, dtype=np.float64))   # noqa: E731
    R = t(A) @ t(alpha)
    d = R - t(b)
    q = (d * d).sum(axis=0)
    al = t(alpha)[1:] if add_bias else t(alpha)
    g = np.abs(al) if absm else al
    l1 = g.sum(axis=0)
    regS = np.broadcast_to(t(reg), (S,))
    val = q / (2 * t(m)) + regS * l1
    dd = 64 * EPS * (f(A) @ f(alpha)) + 2 * EPS * (f(R) + f(b))
    bq = np.array([sumsq_bound(d[:, s], dd[:, s]) for s in range(S)])
    bl1 = 64 * EPS * f(al).sum(axis=0)
    bound = bq / (2 * m) + f(regS) * bl1 + 4 * EPS * (f(q) / (2 * m) + f(regS) * f(g).sum(axis=0))
    cols = np.arange(S) if cols is None else np.asarray(cols)
    vals = np.zeros(S, dtype=dtype) if out is None else np.array(out, dtype=dtype)
    bnds = np.zeros(vals.shape)
    vals[cols] = val
    bnds[cols] = bound
    return vals, bnds


# --------------------------------------------------------------------------- layouts, helpers
def block_qs(Qs):
    """the tile-blocked copy of a k-major Qs (include/ipm355.h): element (i, k) = Qs[k, i] at
    ((i // 32) n + k) 32 + i % 32, rows i >= n zero"""
    n = Qs.shape[0]
    nt = (n + LT - 1) // LT
    Qb = np.zeros(nt * n * LT)
    i = np.arange(n)
    for k in range(n):
        Qb[((i // LT) * n + k) * LT + i % LT] = Qs[k, :n]
    return Qb


def colstd_inorder(A):
    """what k_colstd_scale computes: per column the fp64 sums taken row by row, separate multiply
    and add -> (A / sd, sd)"""
    A = np.asarray(A, dtype=np.float64)
    m = A.shape[0]
    s = np.zeros(A.shape[1])
    for i in range(m):
        s = s + A[i]
    mean = s / float(m)
    v = np.zeros(A.shape[1])
    for i in range(m):
        d = A[i] - mean
        v = v + d * d
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.sqrt(v / float(m))
        return A / sd, sd


def ks_from_partial_doubles(n, S, total):
    """the K-split count behind ipm_lasso_partial_doubles(n, S) = 4 tiles + 8 +
    (ks > 1 ? tiles (1024 ks + 1) : 0)"""
    tiles = ((S + LT - 1) // LT) * ((n + LT - 1) // LT)
    rest = total - 4 * tiles - 8
    if rest == 0:
        return 1
    assert rest > 0 and rest % tiles == 0 and (rest // tiles - 1) % (LT * LT) == 0, (n, S, total)
    ks = (rest // tiles - 1) // (LT * LT)
    assert ks > 1, (n, S, total)
    return ks


def admm_ks(n, S):
    """the library's K-split count at (n, S), recovered from ipm_lasso_partial_doubles"""
    import gpu_util as G
    return ks_from_partial_doubles(n, S, int(G.handle().lib.ipm_lasso_partial_doubles(n, S)))


def kchunk(n, ks):
    """rows of one K chunk of the step (multiples of 16) and the rows of the last chunk (<= 0: empty)"""
    kc = ((n + 16 * ks - 1) // (16 * ks)) * 16
    return kc, n - (ks - 1) * kc


# the one-step shapes (n, S) and the ks each must produce with the default workgroup target
SMALL = [((1, 1), 1), ((15, 17), 1), ((31, 33), 1), ((32, 32), 1), ((33, 31), 1), ((65, 64), 1)]
LARGE = [((257, 33), 2), ((400, 30), 3), ((1030, 17), 8), ((1153, 5), 9), ((1281, 3), 10)]
# more than 256 tiles: the strided loop of k_admm_norms.  (288, 900) has 261 tiles and, by the
# library's rule (at least 512 workgroups, chunks of at least 128 rows), ks = ceil(512 / 261) = 2;
# (224, 1200) has 266 tiles and n / 128 = 1, so ks = 1
STRIDED = [((288, 900), 2), ((224, 1200), 1)]


# --------------------------------------------------------------------------- device side
class DeviceStep:
    """Device buffers of one ipm_lasso_admm call built from a `state` dict: NaN in the padding of
    every input with a leading dimension above its width, the sentinel SENT in the padding of the
    in/out state.  `args` is the filled ipm355.lasso.LassoArgs; the tensors stay alive in `t`."""
    SENT = -7.25

    def __init__(self, st, lds=None, qs_blocked=1, ldq=None, partial=None, positive=0, add_bias=0, dual_form=0,
                 ba_bcast=0, eta_bcast=0, max_iters=1, check_stop=1, stop_multiplier=0.0, eps_rel=0.0):
        import torch
        import gpu_util as G
        from ipm355 import _lib as L
        from ipm355.lasso import LassoArgs
        n, S = st["u"].shape
        self.n, self.S = n, S
        lds = lds or S
        ldq = ldq or n
        self.lds, self.ldq = lds, ldq
        lib = L.load_library()
        t = {}

        def padded(a, ld, fill):
            buf = torch.full((a.shape[0], ld), fill, dtype=torch.float64, device="cuda")
            buf[:, :a.shape[1]] = G.dev(a)
            return buf
        Qs = padded(st["Qs"], ldq, float("nan"))
        if qs_blocked:
            Qb = G.devnan((int(lib.ipm_lasso_qb_doubles(n)),))
            h = G.handle()
            h.check(lib.ipm_lasso_block_qs(h.ptr, n, L.dptr(Qs), ldq, L.dptr(Qb)), h.ptr)
            t["Qs"] = Qb
        else:
            t["Qs"] = Qs
        ldba = 1 if ba_bcast else lds
        t["bA"] = padded(st["bA"], ldba, float("nan"))
        t["eta"] = G.dev(st["eta"])
        for k in ("x", "alpha", "u"):
            t[k] = padded(st[k], lds, self.SENT)
        t["W0"] = padded(st["W"], lds, float("nan"))
        t["W1"] = torch.full((n, lds), self.SENT, dtype=torch.float64, device="cuda")
        npart = int(lib.ipm_lasso_partial_doubles(n, S))
        t["partial"] = partial if partial is not None else torch.zeros(npart, dtype=torch.float64, device="cuda")
        assert t["partial"].numel() == npart
        a = LassoArgs()
        a.n, a.S, a.m, a.lds = n, S, 0, lds
        a.Qs, a.ldq, a.qs_blocked = L.dptr(t["Qs"]), ldq, int(qs_blocked)
        a.bA, a.ldba, a.ba_bcast = L.dptr(t["bA"]), ldba, int(ba_bcast)
        a.eta, a.eta_bcast = L.dptr(t["eta"]), int(eta_bcast)
        for k in ("x", "alpha", "u", "W0", "W1", "partial"):
            setattr(a, k, L.dptr(t[k]))
        a.rho, a.eps_abs, a.eps_rel, a.stop_multiplier = float(st["rho"]), 0.0, float(eps_rel), float(stop_multiplier)
        a.max_iters, a.check_stop = int(max_iters), int(check_stop)
        a.positive, a.add_bias, a.dual_form = int(positive), int(add_bias), int(dual_form)
        self.args, self.t = a, t
        self.nblk = ((S + LT - 1) // LT) * ((n + LT - 1) // LT)

    def run(self):
        """ipm_lasso_admm -> (rc, iters)"""
        import ctypes
        import gpu_util as G
        h = G.handle()
        it = ctypes.c_int32(-99)
        rc = h.lib.ipm_lasso_admm(h.ptr, ctypes.byref(self.args), ctypes.byref(it))
        return rc, int(it.value)

    def out(self, k):
        """(values (n, S), padding (n, lds - S)) of x / alpha / u / W0 / W1 on the host"""
        import gpu_util as G
        a = G.host(self.t[k])
        return a[:, :self.S], a[:, self.S:]

    def norms(self):
        import gpu_util as G
        return G.host(self.t["partial"][4 * self.nblk: 4 * self.nblk + 4])


def step_ratios(dv, ref, wkey="W1"):
    """err / bound of a finished one-step DeviceStep against an admm_step dict"""
    r = {k: ratio(dv.out(k)[0], ref[k], ref["b" + k]) for k in ("x", "alpha", "u")}
    r["W"] = ratio(dv.out(wkey)[0], ref["W"], ref["bW"])
    r["sums"] = ratio(dv.norms(), ref["sums"], ref["bsums"])
    return r
