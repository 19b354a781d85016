// H = X diag(w) X^T (+ diag(dvec)), lower triangle, for a ROW-MAJOR X (m x k): the sum runs over
// the contiguous index of X.  The product of the dual-form Newton step, S = diag(1/w) + C diag(E) C^T
// with C the LP's row-major inequality matrix -- every other MFMA GEMM of the library sums over the
// rows of its operands (k-major), which would need a resident transposed copy of C.
//
// One workgroup (4 waves) per 64 x 64 lower-triangle tile and K chunk.  Per stage of 32 k columns
// the two 64 x 32 operand blocks (rows of the tile's column range, scaled by w, and rows of its row
// range) are read with coalesced loads along k -- 16-byte loads when every row is 16-byte aligned,
// 8-byte loads otherwise (odd ldx) -- and parked in LDS (row stride 36 doubles: the fragment reads
// of 16 rows x 4 columns then spread over all banks); the next stage's global loads are issued
// before the MFMAs of the current one.  Each wave owns a 32 x 32 quarter: 2 x 2 accumulators of
// v_mfma_f64_16x16x4_f64.  Lane l holds A[row = l & 15][k = l >> 4], B[k = l >> 4][col = l & 15] and
// D[row = (l >> 4) + 4 reg][col = l & 15]; the MFMA's column index is H's ROW index, so that the 16
// lanes of a register store 128 contiguous bytes of a column of the column-major H.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ipm355.h"
#include "ipm_common.h"
#include "ipm_handle.h"
#include "ipm_syrk_nt.h"

namespace ipm {
namespace {

constexpr int NT_T = SYRK_NT_TILE, NT_BK = SYRK_NT_BK, NT_LD = NT_BK + 4;

typedef double dbl2 __attribute__((ext_vector_type(2)));

// tile t of the row-by-row enumeration of the lower triangle: (ti, tj), tj <= ti
__device__ __forceinline__ void tri_decode(int64_t t, int64_t& ti, int64_t& tj) {
  int64_t r = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (r * (r + 1) / 2 > t) --r;
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  ti = r;
  tj = t - r * (r + 1) / 2;
}

// part == null: the tile goes to H (the whole k range in this workgroup); otherwise the full 64 x 64
// partial tile of chunk blockIdx.y goes to part[(tile * gridDim.y + chunk) * 4096 + 64 jl + il]
// Second = NtSecond (syrk_nt_lower2): the operand is two row-stacked matrices, rows [0, m0) from X (ldx)
// and rows [m0, m) from X1 (ldx1); a 64-row block may straddle m0, so the source is chosen per loaded
// row.  Everything after the load is the one-operand kernel's: the same sums in the same order.  With
// the empty pack the signature and the code are the one-operand kernel's, unchanged.
struct NtSecond {
  int64_t m0;
  const double* X1;
  int64_t ldx1;
};
__device__ __forceinline__ NtSecond nt_second() { return NtSecond{0, nullptr, 0}; }
__device__ __forceinline__ NtSecond nt_second(NtSecond s) { return s; }

template <bool VEC, class... Second>
__global__ __launch_bounds__(256) void k_syrk_nt(int64_t m, int64_t k, const double* __restrict__ X, int64_t ldx,
                                                 const double* __restrict__ w, const double* __restrict__ dvec,
                                                 double* __restrict__ H, int64_t ldh, double* __restrict__ part,
                                                 int64_t chunk, Second... second) {
  constexpr bool TWO = sizeof...(Second) != 0;
  const NtSecond sec = nt_second(second...);
  __shared__ __attribute__((aligned(16))) double sJ[NT_T * NT_LD];
  __shared__ __attribute__((aligned(16))) double sI[NT_T * NT_LD];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fr = lane & 15, fk = lane >> 4;
  const int wi = wv & 1, wj = wv >> 1;
  int64_t ti, tj;
  tri_decode(blockIdx.x, ti, tj);
  const int64_t i0 = ti * NT_T, j0 = tj * NT_T;
  const bool diag = ti == tj;
  const int64_t kbeg = (int64_t)blockIdx.y * chunk, kend = min(k, kbeg + chunk);
  // loader: thread -> rows lr + 16 pass (pass 0..3) of both blocks, columns lc and lc + 1
  const int lr = tid >> 4, lc = (tid & 15) * 2;
  double rj[4][2], ri[4][2], rw[2];
  // two operands: the start of each of this thread's eight rows, in whichever matrix holds it, once per
  // workgroup (the per-row choice stays out of the stage loop)
  const double *bj[4] = {nullptr, nullptr, nullptr, nullptr}, *bi[4] = {nullptr, nullptr, nullptr, nullptr};
  if constexpr (TWO) {
    auto rowbase = [&](int64_t row) {
      if (row >= m) return X;   // (never read: row2 returns first)
      return row >= sec.m0 ? sec.X1 + (row - sec.m0) * sec.ldx1 : X + row * ldx;
    };
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      bj[ps] = rowbase(j0 + lr + 16 * ps);
      bi[ps] = rowbase(i0 + lr + 16 * ps);
    }
  }
  auto gload = [&](int64_t kk0) {
    const int64_t c = kk0 + lc;
    const bool c0 = c < kend, c1 = c + 1 < kend;
    rw[0] = c0 ? (w ? w[c] : 1.0) : 0.0;
    rw[1] = c1 ? (w ? w[c + 1] : 1.0) : 0.0;
    auto row2 = [&](int64_t row, const double* base, double* o) {
      o[0] = 0.0;
      o[1] = 0.0;
      if (row >= m || !c0) return;
      const double* p = TWO ? base + c : X + row * ldx + c;
      if (VEC && c1) {
        const dbl2 v = *reinterpret_cast<const dbl2*>(p);
        o[0] = v[0];
        o[1] = v[1];
      } else {
        o[0] = p[0];
        if (c1) o[1] = p[1];
      }
    };
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      row2(j0 + lr + 16 * ps, bj[ps], rj[ps]);
      if (!diag) row2(i0 + lr + 16 * ps, bi[ps], ri[ps]);
    }
  };
  dbl4 acc[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[p][q] = dbl4{0.0, 0.0, 0.0, 0.0};
  if (kbeg < kend) gload(kbeg);
  for (int64_t kk0 = kbeg; kk0 < kend; kk0 += NT_BK) {
    __syncthreads();   // the previous stage's fragment reads are done
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int o = (lr + 16 * ps) * NT_LD + lc;
      // an out-of-range column is 0 * 0, never w * (padding of X)
      *reinterpret_cast<dbl2*>(&sJ[o]) = dbl2{rj[ps][0] * rw[0], rj[ps][1] * rw[1]};
      *reinterpret_cast<dbl2*>(&sI[o]) = diag ? dbl2{rj[ps][0], rj[ps][1]} : dbl2{ri[ps][0], ri[ps][1]};
    }
    __syncthreads();
    if (kk0 + NT_BK < kend) gload(kk0 + NT_BK);
    const double* aj = sJ + (32 * wj + fr) * NT_LD + fk;
    const double* bi = sI + (32 * wi + fr) * NT_LD + fk;
#pragma unroll
    for (int u = 0; u < NT_BK / 4; ++u) {
      double a[2], b[2];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        a[p] = aj[16 * p * NT_LD + 4 * u];
        b[p] = bi[16 * p * NT_LD + 4 * u];
      }
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p], b[q], acc[p][q], 0, 0, 0);
    }
  }
  // accumulator (p, q), register r: column j = 32 wj + 16 p + fk + 4 r, row i = 32 wi + 16 q + fr
  double* pt = part ? part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * (NT_T * NT_T) : nullptr;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jl = 32 * wj + 16 * p + fk + 4 * r, il = 32 * wi + 16 * q + fr;
        if (pt) {
          pt[jl * NT_T + il] = acc[p][q][r];
        } else {
          const int64_t i = i0 + il, j = j0 + jl;
          if (i < m && j <= i) {
            double v = acc[p][q][r];
            if (i == j && dvec) v = v + dvec[i];
            H[j * ldh + i] = v;
          }
        }
      }
}

// H tile = part[tile][0] + part[tile][1] + ... in chunk order (+ dvec on the diagonal); ks == 0
// writes the empty sum (k = 0)
__global__ __launch_bounds__(256) void k_syrk_nt_fold(int64_t m, int64_t ks, const double* __restrict__ part,
                                                      const double* __restrict__ dvec, double* __restrict__ H,
                                                      int64_t ldh) {
  int64_t ti, tj;
  tri_decode(blockIdx.x, ti, tj);
  const double* pt = part + (int64_t)blockIdx.x * ks * (NT_T * NT_T);
  for (int e = threadIdx.x; e < NT_T * NT_T; e += 256) {
    const int64_t i = ti * NT_T + (e & (NT_T - 1)), j = tj * NT_T + (e >> 6);
    if (i >= m || j > i) continue;
    double v = 0.0;
    for (int64_t z = 0; z < ks; ++z) v = v + pt[z * (NT_T * NT_T) + e];
    if (i == j && dvec) v = v + dvec[i];
    H[j * ldh + i] = v;
  }
}

__global__ void k_dual_combine(int64_t n, const double* __restrict__ E, const double* __restrict__ g,
                               const double* __restrict__ ctz, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = E[i] * (-g[i] - ctz[i]);
}

__global__ void k_dual_residual(int64_t n, const double* __restrict__ g, const double* __restrict__ dvec,
                                const double* __restrict__ dx, const double* __restrict__ hc,
                                double* __restrict__ rho) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) rho[i] = -g[i] - (dvec[i] * dx[i] + hc[i]);
}

__global__ void k_dual_correct(int64_t n, const double* __restrict__ E, const double* __restrict__ rho,
                               const double* __restrict__ ctz, double* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dx[i] = dx[i] + E[i] * (rho[i] - ctz[i]);
}

// ---- the dual-form step with equality rows (IPM_SOLVE_CHOLESKY_DUAL_EQ): K [z; nu] = r over M = [C; A]
// r[i] = r[i] - (-axb[i] - adx[i]) = A (E o rho_x) - rho_p with rho_p = -(A x - b) - A dx (adx null: dx = 0)
__global__ void k_dual_eq_rhs(int64_t p, const double* __restrict__ axb, const double* __restrict__ adx,
                              double* __restrict__ r) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < p) r[i] = r[i] - (-axb[i] - (adx ? adx[i] : 0.0));
}

__global__ void k_dual_eq_combine(int64_t n, const double* __restrict__ E, const double* __restrict__ g,
                                  const double* __restrict__ ctz, const double* __restrict__ atv,
                                  double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = E[i] * (-g[i] - ctz[i] - atv[i]);
}

__global__ void k_dual_eq_residual(int64_t n, const double* __restrict__ g, const double* __restrict__ dvec,
                                   const double* __restrict__ dx, const double* __restrict__ hc,
                                   const double* __restrict__ atv, const double* __restrict__ E,
                                   double* __restrict__ rho, double* __restrict__ erho) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const double r = -g[i] - (dvec[i] * dx[i] + hc[i]) - atv[i];
    rho[i] = r;
    erho[i] = E[i] * r;
  }
}

// dx += E o (rho - ctz - atv) over n entries, nu += nup over p entries (one grid over max(n, p))
__global__ void k_dual_eq_correct(int64_t n, int64_t p, const double* __restrict__ E, const double* __restrict__ rho,
                                  const double* __restrict__ ctz, const double* __restrict__ atv,
                                  double* __restrict__ dx, const double* __restrict__ nup, double* __restrict__ nu) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dx[i] = dx[i] + E[i] * (rho[i] - ctz[i] - atv[i]);
  if (i < p) nu[i] = nu[i] + nup[i];
}

// ---- the dual-form PHASE-1 step (IPM_SOLVE_CHOLESKY_DUAL_PHASE1): the bordered system
// [[Hxx, h], [h^T, hss]] (dx, ds) = (-g_x, -g_s) with Hxx^-1 applied through S.  Scalars stay on the
// device in sc[]: every reduction is a fixed-order sum (per-thread strided partials, wave shuffles,
// then the waves in order), no atomics: two calls give the same bits.
constexpr int PH1_T = 1024;   // threads of the one-workgroup stages

// ru = E o (-g_x), ry = E o h: the two right-hand sides before C
__global__ void k_dual_ph1_rhs(int64_t n, const double* __restrict__ E, const double* __restrict__ g,
                               const double* __restrict__ h, double* __restrict__ ru, double* __restrict__ ry) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    ru[i] = E[i] * (-g[i]);
    ry[i] = E[i] * h[i];
  }
}

// u = E o (-g_x - C^T z_u) (into dx[0:n]), y = E o (h - C^T z_y): the two solutions of Hxx . = [-g_x | h]
__global__ void k_dual_ph1_uy(int64_t n, const double* __restrict__ E, const double* __restrict__ g,
                              const double* __restrict__ h, const double* __restrict__ ctzu,
                              const double* __restrict__ ctzy, double* __restrict__ u, double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    u[i] = E[i] * (-g[i] - ctzu[i]);
    y[i] = E[i] * (h[i] - ctzy[i]);
  }
}

// sigma = hss - h.y, the Schur complement of Hxx in H~, in its form WITHOUT cancellation: H~ is a sum of
// squares over the slack rows, and (-y, 1) minimizes its quadratic form over (v, 1), so
//   sigma = sum_C w (1 + C y)^2 + sum inv_lb^2 (1 - y)^2 + sum inv_ub^2 (1 + y)^2 + add (y.y + 1)
// (the error of y enters squared; hss - h.y loses sigma / hss digits: 4.7e-9 on the test grid).
// Then ds = (-g_s - h.u) / sigma and dx = u - y ds (u arrives in dx[0:n]).  One workgroup.
// sc[0] = sigma, sc[1] = hss (+ add); *bad = 1 unless sigma is finite and positive.
__global__ __launch_bounds__(PH1_T) void k_dual_ph1_combine(int64_t n, int64_t m, const double* __restrict__ h,
                                                            const double* __restrict__ y,
                                                            const double* __restrict__ w,
                                                            const double* __restrict__ cy,
                                                            const double* __restrict__ ilb,
                                                            const double* __restrict__ iub,
                                                            const double* __restrict__ hss, double add,
                                                            const double* __restrict__ g, double* __restrict__ dx,
                                                            double* __restrict__ sc, int* __restrict__ bad) {
  __shared__ double red[16];
  double sg = 0.0, hu = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += PH1_T) {
    const double a = 1.0 + cy[i];
    sg += w[i] * (a * a);
  }
  for (int64_t i = threadIdx.x; i < n; i += PH1_T) {
    const double yi = y[i];
    double v = add * (yi * yi);
    if (ilb) {
      const double a = 1.0 - yi, b = ilb[i];
      v += (b * b) * (a * a);
    }
    if (iub) {
      const double a = 1.0 + yi, b = iub[i];
      v += (b * b) * (a * a);
    }
    sg += v;
    hu = fma(h[i], dx[i], hu);
  }
  sg = block_sum(sg, red);
  hu = block_sum(hu, red);
  const double sigma = sg + add;
  const double ds = (-g[n] - hu) / sigma;
  for (int64_t i = threadIdx.x; i < n; i += PH1_T) dx[i] = dx[i] - y[i] * ds;
  if (threadIdx.x == 0) {
    dx[n] = ds;
    sc[0] = sigma;
    sc[1] = hss[0] + add;
    *bad = (isfinite(sigma) && sigma > 0.0) ? 0 : 1;
  }
}

// rho_x = -g_x - (D o dx + hc) - h ds with hc = C^T (w o (C dx)); erho = E o rho_x (the next solve's
// right-hand side before C); part[block] = the block's share of h.dx (for rho_s)
__global__ __launch_bounds__(256) void k_dual_ph1_residual(int64_t n, const double* __restrict__ g,
                                                           const double* __restrict__ dvec,
                                                           const double* __restrict__ dx,
                                                           const double* __restrict__ hc,
                                                           const double* __restrict__ h,
                                                           const double* __restrict__ E, double* __restrict__ rho,
                                                           double* __restrict__ erho, double* __restrict__ part) {
  __shared__ double red[16];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const double ds = dx[n];
  double hd = 0.0;
  if (i < n) {
    const double r = -g[i] - (dvec[i] * dx[i] + hc[i]) - h[i] * ds;
    rho[i] = r;
    erho[i] = E[i] * r;
    hd = h[i] * dx[i];
  }
  hd = block_sum(hd, red);
  if (threadIdx.x == 0) part[blockIdx.x] = hd;
}

// du = E o (rho_x - C^T z'), rho_s = -g_s - h.dx - hss ds, dds = (rho_s - h.du) / sigma;
// dx += du - y dds, ds += dds.  One workgroup; h.dx from the residual launch's partials in block order.
__global__ __launch_bounds__(PH1_T) void k_dual_ph1_correct(int64_t n, int64_t nblk, const double* __restrict__ E,
                                                            const double* __restrict__ rho,
                                                            const double* __restrict__ ctz,
                                                            const double* __restrict__ h,
                                                            const double* __restrict__ y,
                                                            const double* __restrict__ g,
                                                            const double* __restrict__ sc,
                                                            const double* __restrict__ part, double* __restrict__ dx) {
  __shared__ double red[16];
  double hdx = 0.0, hdu = 0.0;
  for (int64_t b = threadIdx.x; b < nblk; b += PH1_T) hdx += part[b];
  for (int64_t i = threadIdx.x; i < n; i += PH1_T) hdu = fma(h[i], E[i] * (rho[i] - ctz[i]), hdu);
  hdx = block_sum(hdx, red);
  hdu = block_sum(hdu, red);
  const double ds = dx[n];
  const double rs = -g[n] - hdx - sc[1] * ds;
  const double dds = (rs - hdu) / sc[0];
  for (int64_t i = threadIdx.x; i < n; i += PH1_T) dx[i] = dx[i] + (E[i] * (rho[i] - ctz[i]) - y[i] * dds);
  __syncthreads();   // every thread has read ds = dx[n]
  if (threadIdx.x == 0) dx[n] = ds + dds;
}

}  // namespace

void dual_ph1_rhs(hipStream_t st, int64_t n, const double* E, const double* g, const double* h, double* ru,
                  double* ry) {
  if (n > 0) hipLaunchKernelGGL(k_dual_ph1_rhs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, E, g, h, ru, ry);
}

void dual_ph1_uy(hipStream_t st, int64_t n, const double* E, const double* g, const double* h, const double* ctzu,
                 const double* ctzy, double* u, double* y) {
  if (n > 0)
    hipLaunchKernelGGL(k_dual_ph1_uy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, E, g, h, ctzu, ctzy, u, y);
}

void dual_ph1_combine(hipStream_t st, int64_t n, int64_t m, const double* h, const double* y, const double* w,
                      const double* cy, const double* ilb, const double* iub, const double* hss, double add,
                      const double* g, double* dx, double* sc, int* bad) {
  hipLaunchKernelGGL(k_dual_ph1_combine, dim3(1), dim3(PH1_T), 0, st, n, m, h, y, w, cy, ilb, iub, hss, add, g, dx, sc,
                     bad);
}

void dual_ph1_residual(hipStream_t st, int64_t n, const double* g, const double* dvec, const double* dx,
                       const double* hc, const double* h, const double* E, double* rho, double* erho, double* part) {
  if (n > 0)
    hipLaunchKernelGGL(k_dual_ph1_residual, dim3((unsigned)dual_ph1_blocks(n)), dim3(256), 0, st, n, g, dvec, dx, hc, h,
                       E, rho, erho, part);
}

void dual_ph1_correct(hipStream_t st, int64_t n, const double* E, const double* rho, const double* ctz, const double* h,
                      const double* y, const double* g, const double* sc, const double* part, double* dx) {
  hipLaunchKernelGGL(k_dual_ph1_correct, dim3(1), dim3(PH1_T), 0, st, n, dual_ph1_blocks(n), E, rho, ctz, h, y, g, sc,
                     part, dx);
}

void syrk_nt_lower(hipStream_t st, int64_t m, int64_t k, const double* X, int64_t ldx, const double* w,
                   const double* dvec, double* H, int64_t ldh, double* ws) {
  if (m <= 0) return;
  SyrkNtPlan p = syrk_nt_plan(m, k);
  if (k <= 0) {
    hipLaunchKernelGGL(k_syrk_nt_fold, dim3((unsigned)p.ntiles), dim3(256), 0, st, m, (int64_t)0, ws, dvec, H, ldh);
    return;
  }
  if (!ws && p.ks > 1) {
    p.ks = 1;
    p.chunk = (k + NT_BK - 1) / NT_BK * NT_BK;
  }
  double* part = p.ks > 1 ? ws : nullptr;
  // 16-byte loads need every row start 16-byte aligned (as symv_lower decides it)
  const bool vec = (reinterpret_cast<uintptr_t>(X) & 15) == 0 && (ldx & 1) == 0;
  const dim3 grid((unsigned)p.ntiles, (unsigned)p.ks);
  if (vec) hipLaunchKernelGGL(k_syrk_nt<true>, grid, dim3(256), 0, st, m, k, X, ldx, w, dvec, H, ldh, part, p.chunk);
  else hipLaunchKernelGGL(k_syrk_nt<false>, grid, dim3(256), 0, st, m, k, X, ldx, w, dvec, H, ldh, part, p.chunk);
  if (part)
    hipLaunchKernelGGL(k_syrk_nt_fold, dim3((unsigned)p.ntiles), dim3(256), 0, st, m, p.ks, part, dvec, H, ldh);
}

void syrk_nt_lower2(hipStream_t st, int64_t m0, int64_t m1, int64_t k, const double* X0, int64_t ldx0,
                    const double* X1, int64_t ldx1, const double* w, const double* dvec, double* H, int64_t ldh,
                    double* ws) {
  if (m1 <= 0) {
    syrk_nt_lower(st, m0, k, X0, ldx0, w, dvec, H, ldh, ws);
    return;
  }
  m0 = std::max<int64_t>(m0, 0);
  const int64_t m = m0 + m1;
  // the plan of the stacked matrix: tiles, K split, workspace layout and fold order are syrk_nt_lower's
  SyrkNtPlan p = syrk_nt_plan(m, k);
  if (k <= 0) {
    hipLaunchKernelGGL(k_syrk_nt_fold, dim3((unsigned)p.ntiles), dim3(256), 0, st, m, (int64_t)0, ws, dvec, H, ldh);
    return;
  }
  if (!ws && p.ks > 1) {
    p.ks = 1;
    p.chunk = (k + NT_BK - 1) / NT_BK * NT_BK;
  }
  double* part = p.ks > 1 ? ws : nullptr;
  // 16-byte loads only when every row start of BOTH operands is 16-byte aligned (an empty X0 is never read)
  const bool vec = (m0 == 0 || ((reinterpret_cast<uintptr_t>(X0) & 15) == 0 && (ldx0 & 1) == 0)) &&
                   (reinterpret_cast<uintptr_t>(X1) & 15) == 0 && (ldx1 & 1) == 0;
  const dim3 grid((unsigned)p.ntiles, (unsigned)p.ks);
  const NtSecond sec{m0, X1, ldx1};
  if (vec)
    hipLaunchKernelGGL((k_syrk_nt<true, NtSecond>), grid, dim3(256), 0, st, m, k, X0, ldx0, w, dvec, H, ldh, part,
                       p.chunk, sec);
  else
    hipLaunchKernelGGL((k_syrk_nt<false, NtSecond>), grid, dim3(256), 0, st, m, k, X0, ldx0, w, dvec, H, ldh, part,
                       p.chunk, sec);
  if (part)
    hipLaunchKernelGGL(k_syrk_nt_fold, dim3((unsigned)p.ntiles), dim3(256), 0, st, m, p.ks, part, dvec, H, ldh);
}

void dual_eq_rhs(hipStream_t st, int64_t p, const double* axb, const double* adx, double* r) {
  if (p > 0) hipLaunchKernelGGL(k_dual_eq_rhs, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, st, p, axb, adx, r);
}

void dual_eq_combine(hipStream_t st, int64_t n, const double* E, const double* g, const double* ctz, const double* atv,
                     double* out) {
  if (n > 0)
    hipLaunchKernelGGL(k_dual_eq_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, E, g, ctz, atv, out);
}

void dual_eq_residual(hipStream_t st, int64_t n, const double* g, const double* dvec, const double* dx,
                      const double* hc, const double* atv, const double* E, double* rho, double* erho) {
  if (n > 0)
    hipLaunchKernelGGL(k_dual_eq_residual, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, g, dvec, dx, hc, atv,
                       E, rho, erho);
}

void dual_eq_correct(hipStream_t st, int64_t n, int64_t p, const double* E, const double* rho, const double* ctz,
                     const double* atv, double* dx, const double* nup, double* nu) {
  const int64_t len = std::max(n, p);
  if (len > 0)
    hipLaunchKernelGGL(k_dual_eq_correct, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, n, p, E, rho, ctz, atv,
                       dx, nup, nu);
}

void dual_combine(hipStream_t st, int64_t n, const double* E, const double* g, const double* ctz, double* out) {
  if (n > 0) hipLaunchKernelGGL(k_dual_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, E, g, ctz, out);
}

void dual_residual(hipStream_t st, int64_t n, const double* g, const double* dvec, const double* dx, const double* hc,
                   double* rho) {
  if (n > 0)
    hipLaunchKernelGGL(k_dual_residual, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, g, dvec, dx, hc, rho);
}

void dual_correct(hipStream_t st, int64_t n, const double* E, const double* rho, const double* ctz, double* dx) {
  if (n > 0)
    hipLaunchKernelGGL(k_dual_correct, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, E, rho, ctz, dx);
}

}  // namespace ipm

using namespace ipm;

extern "C" int ipm_syrk_nt(ipm_handle* h, int64_t m, int64_t k, const double* X, int64_t ldx, const double* w,
                           const double* dvec, double* H, int64_t ldh) {
  if (!h || m < 0 || k < 0 || ldh < m || (k > 0 && ldx < k)) return IPM_INVALID_ARG;
  if (m == 0) return IPM_OK;
  if (!H || (k > 0 && !X)) return IPM_INVALID_ARG;
  double* ws = nullptr;
  const int64_t wd = syrk_nt_ws_doubles(m, k);
  if (wd > 0) {
    ws = ipm_handle_scratch(h, (size_t)wd * sizeof(double));
    if (!ws) { h->err = "scratch alloc failed"; return IPM_HIP_ERROR; }
  }
  syrk_nt_lower(h->stream, m, k, X, ldx, w, dvec, H, ldh, ws);
  HIPCHK(h, hipGetLastError());
  return IPM_OK;
}

extern "C" int ipm_syrk_nt2(ipm_handle* h, int64_t m0, int64_t m1, int64_t k, const double* X0, int64_t ldx0,
                            const double* X1, int64_t ldx1, const double* w, const double* dvec, double* H,
                            int64_t ldh) {
  if (!h || m0 < 0 || m1 < 0 || k < 0) return IPM_INVALID_ARG;
  if (m1 == 0) return ipm_syrk_nt(h, m0, k, X0, ldx0, w, dvec, H, ldh);
  const int64_t m = m0 + m1;
  if (ldh < m || (k > 0 && ((m0 > 0 && ldx0 < k) || ldx1 < k))) return IPM_INVALID_ARG;
  if (!H || (k > 0 && ((m0 > 0 && !X0) || !X1))) return IPM_INVALID_ARG;
  double* ws = nullptr;
  const int64_t wd = syrk_nt_ws_doubles(m, k);
  if (wd > 0) {
    ws = ipm_handle_scratch(h, (size_t)wd * sizeof(double));
    if (!ws) { h->err = "scratch alloc failed"; return IPM_HIP_ERROR; }
  }
  syrk_nt_lower2(h->stream, m0, m1, k, X0, ldx0, X1, ldx1, w, dvec, H, ldh, ws);
  HIPCHK(h, hipGetLastError());
  return IPM_OK;
}
