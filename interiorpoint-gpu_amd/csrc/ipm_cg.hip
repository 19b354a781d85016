// linear_solve_method='cg' (NewtonSolver.py:365-400): the symmetric matrix-vector product on the
// lower triangle of H and scipy.sparse.linalg.cg's loop, as launches on one stream.
//
// SYMV.  H (column-major lower, ldh) is cut into 128 x 128 tiles; workgroup (bi, bj), bi >= bj,
// loads its tile ONCE and forms two 128-vectors: L_ij x_j for output block bi and L_ij^T x_i for
// output block bj (a diagonal tile folds both into one, its strict upper half never loaded).
// Each goes to its own slot of a partial array -- output block b has nb slots, slot k written by
// tile (b, k) for k <= b and by tile (k, b) for k > b -- and a second launch adds the nb slots of
// every output row in slot order.  No atomics, no workgroup waits on another, and every sum has
// a fixed order: two calls on the same inputs give the same bits.
//
// CG.  3 launches per iteration (tiles, slot sums with the p.q partials, one single-workgroup
// update that also does the next iteration's convergence test and direction), issued maxiter
// times whatever happens; every kernel first reads the device `done` word and returns when it
// is set, so after convergence x is not touched and the rest of the sequence costs launches only.
//
// Preconditioner.  With minv (the diagonal of M; k_cg_minv writes 1 / diag(H)) the start and update
// kernels run their PRE instantiations: scipy's loop with M, z = minv r recomputed where it is
// needed instead of stored.  One more launch in the prologue, the same 3 per iteration.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/ipm355.h"
#include "ipm_cg.h"
#include "ipm_common.h"
#include "ipm_handle.h"

namespace ipm {
namespace {

constexpr int T = SYMV_T;
constexpr int VT = 1024;   // the single-workgroup vector kernels
enum { CTL_DONE = 0, CTL_FLAG = 1 };
enum { CSC_ATOL = 0, CSC_RHO = 1, CSC_DC = 2 };

// mode 1: the launch also needs the flag word (x0 non-zero / warm start taken)
__device__ __forceinline__ bool cg_skip(const int* ctl, int mode) {
  if (!ctl) return false;
  if (ctl[CTL_DONE]) return true;
  return mode == 1 && ctl[CTL_FLAG] == 0;
}

// one step of the transpose-reduce: 2K values per lane -> K, summed with the lane S away
template <int K, int S>
__device__ __forceinline__ void fold_step(double* t, int lane) {
  const bool up = (lane & S) != 0;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const double keep = up ? t[i + K] : t[i];
    const double send = up ? t[i] : t[i + K];
    t[i] = keep + __shfl_xor(send, S, 64);
  }
}

// 256 threads: wave w owns columns [32 w, 32 w + 32) of the tile, each lane two rows (VEC: rows
// 2l, 2l + 1 in one 16-byte load; otherwise rows l and l + 64).  VEC needs ldh even and H 16-byte
// aligned; diagonal tiles and a ragged last row take the guarded scalar loads.
template <bool VEC>
__global__ __launch_bounds__(256) void k_symv_tiles(int64_t n, const double* __restrict__ H, int64_t ldh,
                                                    const double* __restrict__ x, double* __restrict__ part,
                                                    int nb, const int* ctl, int mode) {
  if (cg_skip(ctl, mode)) return;
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;
  __shared__ double sx[T];
  __shared__ double srow[4][T];
  __shared__ double scol[T];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t i0 = (int64_t)bi * T, j0 = (int64_t)bj * T;
  const bool diag = bi == bj;
  if (tid < T) sx[tid] = (j0 + tid < n) ? x[j0 + tid] : 0.0;
  const int r0 = VEC ? 2 * lane : lane, r1 = VEC ? 2 * lane + 1 : lane + 64;
  const bool in0 = i0 + r0 < n, in1 = i0 + r1 < n;
  const double xr0 = in0 ? x[i0 + r0] : 0.0, xr1 = in1 ? x[i0 + r1] : 0.0;
  __syncthreads();
  double acc0 = 0.0, acc1 = 0.0;
  const int c0 = wid * 32;
  // 8 columns at a time (their loads in flight together; occupancy hides the rest)
#pragma unroll 1
  for (int ch = 0; ch < 4; ++ch) {
    double t[8];
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) {
      const int c = c0 + ch * 8 + cc;
      const int64_t j = j0 + c;
      double h0 = 0.0, h1 = 0.0;
      if (j < n) {
        const double* col = H + j * ldh + i0;
        if (VEC && !diag && in1) {
          const double2 v = *reinterpret_cast<const double2*>(col + r0);
          h0 = v.x;
          h1 = v.y;
        } else {
          if (in0 && (!diag || r0 >= c)) h0 = col[r0];
          if (in1 && (!diag || r1 >= c)) h1 = col[r1];
        }
      }
      const double xj = sx[c];
      acc0 = fma(h0, xj, acc0);
      acc1 = fma(h1, xj, acc1);
      // the transposed product: a diagonal tile's diagonal entries belong to the row part only
      const double a0 = (diag && r0 == c) ? 0.0 : h0, a1 = (diag && r1 == c) ? 0.0 : h1;
      t[cc] = fma(a1, xr1, a0 * xr0);
    }
    // column sums over the wave's 64 lanes: the 8 values per lane are folded 4, 2, 1 at a time
    // with the lanes 32, 16, 8 away (7 shuffles), then the one left over the 8 lanes of its
    // group (3 more) -- 10 shuffles for 8 columns instead of 48; every lane of group k = lane / 8
    // ends with column k of the chunk, in an order that depends on nothing but the lane number
    fold_step<4, 32>(t, lane);
    fold_step<2, 16>(t, lane);
    fold_step<1, 8>(t, lane);
    double cs = t[0];
    cs += __shfl_xor(cs, 4, 64);
    cs += __shfl_xor(cs, 2, 64);
    cs += __shfl_xor(cs, 1, 64);
    if ((lane & 7) == 0) scol[c0 + ch * 8 + (lane >> 3)] = cs;
  }
  srow[wid][r0] = acc0;
  srow[wid][r1] = acc1;
  __syncthreads();
  if (tid < T) {
    double v = ((srow[0][tid] + srow[1][tid]) + srow[2][tid]) + srow[3][tid];
    if (diag) v += scol[tid];
    part[((int64_t)bi * nb + bj) * T + tid] = v;
  } else if (!diag) {
    part[((int64_t)bj * nb + bi) * T + (tid - T)] = scol[tid - T];
  }
}

// y = alpha * (sum of the nb slots, in slot order) + beta * y; dpart[b] = sum_i dotv[i] y[i] over
// the block's rows (the CG's p.q partials)
__global__ __launch_bounds__(T) void k_symv_reduce(int64_t n, int nb, const double* __restrict__ part, double alpha,
                                                   double beta, double* y, const double* dotv, double* dpart,
                                                   const int* ctl, int mode) {
  if (cg_skip(ctl, mode)) return;
  __shared__ double red[16];
  const int b = blockIdx.x, r = threadIdx.x;
  const int64_t i = (int64_t)b * T + r;
  const double* p = part + (int64_t)b * nb * T + r;
  double s = 0.0;
  for (int k = 0; k < nb; ++k) s += p[(int64_t)k * T];
  double d = 0.0;
  if (i < n) {
    double v = alpha * s;
    if (beta != 0.0) v += beta * y[i];
    y[i] = v;
    if (dotv) d = dotv[i] * v;
  }
  if (dpart) {
    d = block_sum(d, red);
    if (r == 0) dpart[b] = d;
  }
}

// ||b||, atol, "x0 has a non-zero entry"; b == 0: x = b, done (scipy's early return)
__global__ __launch_bounds__(VT) void k_cg_prep(int64_t n, const double* b, double bsign, double* x, double rtol,
                                                int maxiter, int* ctl, int* res, double* sc) {
  __shared__ double red[16];
  double bb = 0.0;
  int nz = 0;
  for (int64_t i = threadIdx.x; i < n; i += VT) {
    const double v = b[i];
    bb = fma(v, v, bb);
    nz |= (x[i] != 0.0) ? 1 : 0;
  }
  bb = block_sum(bb, red);
  nz = __syncthreads_or(nz);
  const double bn = sqrt(bb);
  const bool zero = bn == 0.0;
  if (zero)
    for (int64_t i = threadIdx.x; i < n; i += VT) x[i] = bsign * b[i];
  if (threadIdx.x == 0) {
    const double atol = rtol * bn;
    sc[CSC_ATOL] = atol > 0.0 ? atol : 0.0;   // max(0.0, rtol * ||b||) as Python evaluates it
    ctl[CTL_FLAG] = nz ? 1 : 0;
    ctl[CTL_DONE] = (zero || maxiter <= 0) ? 1 : 0;
    res[0] = 0;
    res[1] = 0;
  }
}

// minv = 1 / diag(H) (the Jacobi preconditioner), zero in the padding up to nb * 128.  Only the
// diagonal entries H[i + i ldh], i < n, are read.  Nothing is special-cased: a zero, negative or
// NaN diagonal entry gives 1 / h as the arithmetic does.  Part of the prologue: it runs before the
// control words are reset, so it does not look at `done`.
__global__ __launch_bounds__(T) void k_cg_minv(int64_t n, const double* __restrict__ H, int64_t ldh,
                                               double* __restrict__ minv) {
  const int64_t i = (int64_t)blockIdx.x * T + threadIdx.x;   // the grid is nb blocks: i < nb * T
  minv[i] = i < n ? 1.0 / H[i + i * ldh] : 0.0;
}

// r = b - A x0 (q = A x0; r = b when x0 is all zero), the first convergence test, p = r
// PRE: z = minv r (one rounded product, never stored), p = z, rho = r.z
template <bool PRE>
__global__ __launch_bounds__(VT) void k_cg_start(int64_t n, const double* b, double bsign, const double* q, double* r,
                                                 double* p, const double* minv, int* ctl, double* sc) {
  if (ctl[CTL_DONE]) return;
  __shared__ double red[16];
  const bool nz = ctl[CTL_FLAG] != 0;
  const double atol = sc[CSC_ATOL];
  double rr = 0.0, rz = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += VT) {
    double v = bsign * b[i];
    if (nz) v = v - q[i];
    r[i] = v;
    if (PRE) {
      const double z = minv[i] * v;
      p[i] = z;
      rz = fma(v, z, rz);
    } else {
      p[i] = v;
    }
    rr = fma(v, v, rr);
  }
  rr = block_sum(rr, red);
  if (PRE) rz = block_sum(rz, red);
  if (threadIdx.x == 0) {
    if (sqrt(rr) < atol) ctl[CTL_DONE] = 1;
    else sc[CSC_RHO] = PRE ? rz : rr;
  }
}

// the tail of iteration `it` (a = rho / p.q, x += a p, r -= a q) and the head of the next one
// (||r|| < atol -> done; rho = r.r, p = (rho / rho_prev) p + r)
// PRE: the test stays on r; rho = r.z with z = minv r, p = (rho / rho_prev) p + z, z recomputed
// from r and minv (the same product, the same bits)
template <bool PRE>
__global__ __launch_bounds__(VT) void k_cg_update(int64_t n, int it, int maxiter, double* x, double* r, double* p,
                                                  const double* q, const double* pq, int nb, const double* minv,
                                                  int* ctl, int* res, double* sc) {
  if (ctl[CTL_DONE]) return;
  __shared__ double red[16];
  const double rho = sc[CSC_RHO], atol = sc[CSC_ATOL];
  double d = 0.0;
  for (int k = threadIdx.x; k < nb; k += VT) d += pq[k];
  d = block_sum(d, red);
  const double a = rho / d;
  double rr = 0.0, rz = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += VT) {
    x[i] = x[i] + a * p[i];
    const double v = r[i] - a * q[i];
    r[i] = v;
    rr = fma(v, v, rr);
    if (PRE) rz = fma(v, minv[i] * v, rz);
  }
  rr = block_sum(rr, red);
  if (PRE) rz = block_sum(rz, red);
  const double rho_new = PRE ? rz : rr;
  const bool last = it + 1 >= maxiter;
  const bool conv = !last && sqrt(rr) < atol;
  if (!last && !conv) {
    const double be = rho_new / rho;
    for (int64_t i = threadIdx.x; i < n; i += VT) p[i] = be * p[i] + (PRE ? minv[i] * r[i] : r[i]);
  }
  if (threadIdx.x == 0) {
    res[0] = it + 1;
    if (last) {
      res[1] = maxiter;
      ctl[CTL_DONE] = 1;
    } else if (conv) {
      ctl[CTL_DONE] = 1;
    } else {
      sc[CSC_RHO] = rho_new;
    }
  }
}

// dc = xc.g; flag = dc < 0 (only then the warm start needs H xc)
__global__ __launch_bounds__(VT) void k_cg_dc(int64_t n, const double* xc, const double* g, int* ctl, double* sc) {
  __shared__ double red[16];
  double d = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += VT) d = fma(xc[i], g[i], d);
  d = block_sum(d, red);
  if (threadIdx.x == 0) {
    sc[CSC_DC] = d;
    ctl[CTL_DONE] = 0;
    ctl[CTL_FLAG] = d < 0.0 ? 1 : 0;
  }
}

// x0 = (-dc * xc) / (xc.q) with q = H xc, or 0 (NewtonSolver.py:380-383)
__global__ __launch_bounds__(VT) void k_cg_warm(int64_t n, const double* xc, const double* q, double* x0,
                                                const double* sc) {
  __shared__ double red[16];
  const double dc = sc[CSC_DC];
  if (dc < 0.0) {
    double d = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += VT) d = fma(xc[i], q[i], d);
    d = block_sum(d, red);
    for (int64_t i = threadIdx.x; i < n; i += VT) x0[i] = (-dc * xc[i]) / d;
  } else {
    for (int64_t i = threadIdx.x; i < n; i += VT) x0[i] = 0.0;
  }
}

struct CgWs {
  double* sc;
  int* ctl;
  double *r, *p, *q, *pq, *part, *minv;
};
CgWs cg_carve(int64_t n, double* ws) {
  const int64_t nb = symv_blocks(n), np = nb * T;
  CgWs w;
  w.sc = ws;
  w.ctl = reinterpret_cast<int*>(ws + 8);
  w.r = ws + 16;
  w.p = w.r + np;
  w.q = w.p + np;
  w.pq = w.q + np;
  w.part = w.pq + ((nb + 7) & ~int64_t(7));
  w.minv = ws + cg_ws_doubles(n) - np;   // the last region: no other offset moved
  return w;
}

void symv_tiles(hipStream_t st, int64_t n, const double* H, int64_t ldh, const double* x, double* part,
                const int* ctl, int mode) {
  const int nb = (int)symv_blocks(n);
  const bool vec = (ldh % 2) == 0 && (reinterpret_cast<uintptr_t>(H) & 15) == 0;
  dim3 g(nb, nb), b(256);
  if (vec) hipLaunchKernelGGL(k_symv_tiles<true>, g, b, 0, st, n, H, ldh, x, part, nb, ctl, mode);
  else hipLaunchKernelGGL(k_symv_tiles<false>, g, b, 0, st, n, H, ldh, x, part, nb, ctl, mode);
}

void symv_reduce(hipStream_t st, int64_t n, const double* part, double alpha, double beta, double* y,
                 const double* dotv, double* dpart, const int* ctl, int mode) {
  const int nb = (int)symv_blocks(n);
  hipLaunchKernelGGL(k_symv_reduce, dim3(nb), dim3(T), 0, st, n, nb, part, alpha, beta, y, dotv, dpart, ctl, mode);
}

}  // namespace

void symv_lower(hipStream_t st, int64_t n, double alpha, const double* H, int64_t ldh, const double* x, double beta,
                double* y, double* ws) {
  if (n <= 0) return;
  symv_tiles(st, n, H, ldh, x, ws, nullptr, 0);
  symv_reduce(st, n, ws, alpha, beta, y, nullptr, nullptr, nullptr, 0);
}

void cg_minv(hipStream_t st, int64_t n, const double* H, int64_t ldh, double* minv) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_cg_minv, dim3((int)symv_blocks(n)), dim3(T), 0, st, n, H, ldh, minv);
}

double* cg_ws_minv(int64_t n, double* ws) { return cg_carve(n, ws).minv; }

void cg_solve(hipStream_t st, int64_t n, const double* H, int64_t ldh, const double* b, double bsign, double* x,
              int32_t maxiter, double rtol, double* ws, int* res, const double* minv) {
  if (n <= 0) return;
  const CgWs w = cg_carve(n, ws);
  const int nb = (int)symv_blocks(n);
  hipLaunchKernelGGL(k_cg_prep, dim3(1), dim3(VT), 0, st, n, b, bsign, x, rtol, (int)maxiter, w.ctl, res, w.sc);
  if (maxiter <= 0) return;
  symv_tiles(st, n, H, ldh, x, w.part, w.ctl, 1);
  symv_reduce(st, n, w.part, 1.0, 0.0, w.q, nullptr, nullptr, w.ctl, 1);
  if (minv) hipLaunchKernelGGL(k_cg_start<true>, dim3(1), dim3(VT), 0, st, n, b, bsign, w.q, w.r, w.p, minv, w.ctl, w.sc);
  else hipLaunchKernelGGL(k_cg_start<false>, dim3(1), dim3(VT), 0, st, n, b, bsign, w.q, w.r, w.p, minv, w.ctl, w.sc);
  for (int it = 0; it < maxiter; ++it) {
    symv_tiles(st, n, H, ldh, w.p, w.part, w.ctl, 0);
    symv_reduce(st, n, w.part, 1.0, 0.0, w.q, w.p, w.pq, w.ctl, 0);
    if (minv)
      hipLaunchKernelGGL(k_cg_update<true>, dim3(1), dim3(VT), 0, st, n, it, (int)maxiter, x, w.r, w.p, w.q, w.pq, nb,
                         minv, w.ctl, res, w.sc);
    else
      hipLaunchKernelGGL(k_cg_update<false>, dim3(1), dim3(VT), 0, st, n, it, (int)maxiter, x, w.r, w.p, w.q, w.pq, nb,
                         minv, w.ctl, res, w.sc);
  }
}

void cg_warm_start(hipStream_t st, int64_t n, const double* H, int64_t ldh, const double* xc, const double* g,
                   double* x0, double* ws) {
  if (n <= 0) return;
  const CgWs w = cg_carve(n, ws);
  hipLaunchKernelGGL(k_cg_dc, dim3(1), dim3(VT), 0, st, n, xc, g, w.ctl, w.sc);
  symv_tiles(st, n, H, ldh, xc, w.part, w.ctl, 1);
  symv_reduce(st, n, w.part, 1.0, 0.0, w.q, nullptr, nullptr, w.ctl, 1);
  hipLaunchKernelGGL(k_cg_warm, dim3(1), dim3(VT), 0, st, n, xc, w.q, x0, w.sc);
}

}  // namespace ipm

using namespace ipm;

// ======================================================================= C ABI (level 0)
extern "C" int ipm_symv(ipm_handle* h, int64_t n, double alpha, const double* H, int64_t ldh, const double* x,
                        double beta, double* y) {
  if (!h || n < 0 || ldh < n) return IPM_INVALID_ARG;
  if (n == 0) return IPM_OK;
  double* ws = ipm_handle_scratch(h, (size_t)symv_ws_doubles(n) * sizeof(double));
  if (!ws) { h->err = "scratch alloc failed"; return IPM_HIP_ERROR; }
  symv_lower(h->stream, n, alpha, H, ldh, x, beta, y, ws);
  HIPCHK(h, hipGetLastError());
  return IPM_OK;
}

namespace {
// ipm_cg and ipm_pcg: pre == false is the unpreconditioned solve; pre with minv == nullptr takes
// 1 / diag(H), computed into the handle's scratch
int cg_level0(ipm_handle* h, int64_t n, const double* H, int64_t ldh, bool pre, const double* minv, const double* b,
              double* x, int32_t maxiter, double rtol, int32_t* iters, int32_t* info) {
  if (!h || n < 0 || ldh < n || maxiter < 0 || !(rtol >= 0.0)) return IPM_INVALID_ARG;
  if (iters) *iters = 0;
  if (info) *info = 0;
  if (n == 0) return IPM_OK;
  double* ws = ipm_handle_scratch(h, (size_t)cg_ws_doubles(n) * sizeof(double));
  if (!ws) { h->err = "scratch alloc failed"; return IPM_HIP_ERROR; }
  int* res = h->dinfo + 2;   // (word 0 is the level-0 Cholesky's)
  if (pre && !minv) {
    double* own = cg_ws_minv(n, ws);
    cg_minv(h->stream, n, H, ldh, own);
    minv = own;
  }
  cg_solve(h->stream, n, H, ldh, b, 1.0, x, maxiter, rtol, ws, res, pre ? minv : nullptr);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(h->hbuf, res, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int out[2];
  std::memcpy(out, h->hbuf, sizeof(out));
  if (iters) *iters = out[0];
  if (info) *info = out[1];
  return IPM_OK;
}
}  // namespace

extern "C" int ipm_cg(ipm_handle* h, int64_t n, const double* H, int64_t ldh, const double* b, double* x,
                      int32_t maxiter, double rtol, int32_t* iters, int32_t* info) {
  return cg_level0(h, n, H, ldh, false, nullptr, b, x, maxiter, rtol, iters, info);
}

extern "C" int ipm_pcg(ipm_handle* h, int64_t n, const double* H, int64_t ldh, const double* minv, const double* b,
                       double* x, int32_t maxiter, double rtol, int32_t* iters, int32_t* info) {
  return cg_level0(h, n, H, ldh, true, minv, b, x, maxiter, rtol, iters, info);
}
