// H = X diag(w) X^T (+ diag(dvec)), lower triangle, for a ROW-MAJOR X (m x k): the sum runs over
// the contiguous index of X.  The product of the dual-form Newton step (ipm_dual.hip), S = diag(1/w) + C diag(E) C^T
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
// Second = NtThird (syrk_nt_lower3): three row-stacked matrices, rows [0, m0) from X (ldx), [m0, m01) from X1
// (ldx1) and [m01, m) from X2 (ldx2); a 64-row block may straddle either seam or both.  One more select per
// row start than NtSecond, before the stage loop; the loads and everything after them are the same.
struct NtThird {
  int64_t m0;
  const double* X1;
  int64_t ldx1;
  int64_t m01;
  const double* X2;
  int64_t ldx2;
};
__device__ __forceinline__ NtThird nt_second(NtThird s) { return s; }
__device__ __forceinline__ const double* nt_rowbase(const NtSecond& s, const double* X, int64_t ldx, int64_t row) {
  return row >= s.m0 ? s.X1 + (row - s.m0) * s.ldx1 : X + row * ldx;
}
__device__ __forceinline__ const double* nt_rowbase(const NtThird& s, const double* X, int64_t ldx, int64_t row) {
  if (row >= s.m01) return s.X2 + (row - s.m01) * s.ldx2;
  return row >= s.m0 ? s.X1 + (row - s.m0) * s.ldx1 : X + row * ldx;
}

template <bool VEC, class... Second>
__global__ __launch_bounds__(256) void k_syrk_nt(int64_t m, int64_t k, const double* __restrict__ X, int64_t ldx,
                                                 const double* __restrict__ w, const double* __restrict__ dvec,
                                                 double* __restrict__ H, int64_t ldh, double* __restrict__ part,
                                                 int64_t chunk, Second... second) {
  constexpr bool TWO = sizeof...(Second) != 0;
  const auto sec = nt_second(second...);
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
      return nt_rowbase(sec, X, ldx, row);
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

// 16-byte loads need every row start 16-byte aligned (as symv_lower decides it) -- with a second operand,
// of BOTH (an empty X0 is never read)
inline bool nt_aligned(const double* X, int64_t ldx) {
  return (reinterpret_cast<uintptr_t>(X) & 15) == 0 && (ldx & 1) == 0;
}
inline bool nt_vec(const double* X, int64_t ldx) { return nt_aligned(X, ldx); }
inline bool nt_vec(const double* X, int64_t ldx, NtSecond s) {
  return (s.m0 == 0 || nt_aligned(X, ldx)) && nt_aligned(s.X1, s.ldx1);
}
// (three operands: all three have rows, syrk_nt_lower3 sends every other case to the forms above)
inline bool nt_vec(const double* X, int64_t ldx, NtThird s) {
  return nt_aligned(X, ldx) && nt_aligned(s.X1, s.ldx1) && nt_aligned(s.X2, s.ldx2);
}

// the one launcher of all entry forms; second: empty (the m x k operand X), or the NtSecond / NtThird of the
// stacked operand, whose plan, K split, workspace layout and fold order are those of one m-row matrix
template <class... Second>
void syrk_nt_launch(hipStream_t st, int64_t m, int64_t k, const double* X, int64_t ldx, const double* w,
                    const double* dvec, double* H, int64_t ldh, double* ws, Second... second) {
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
  const dim3 grid((unsigned)p.ntiles, (unsigned)p.ks);
  if (nt_vec(X, ldx, second...))
    hipLaunchKernelGGL((k_syrk_nt<true, Second...>), grid, dim3(256), 0, st, m, k, X, ldx, w, dvec, H, ldh, part,
                       p.chunk, second...);
  else
    hipLaunchKernelGGL((k_syrk_nt<false, Second...>), grid, dim3(256), 0, st, m, k, X, ldx, w, dvec, H, ldh, part,
                       p.chunk, second...);
  if (part)
    hipLaunchKernelGGL(k_syrk_nt_fold, dim3((unsigned)p.ntiles), dim3(256), 0, st, m, p.ks, part, dvec, H, ldh);
}

}  // namespace

void syrk_nt_lower(hipStream_t st, int64_t m, int64_t k, const double* X, int64_t ldx, const double* w,
                   const double* dvec, double* H, int64_t ldh, double* ws) {
  if (m > 0) syrk_nt_launch(st, m, k, X, ldx, w, dvec, H, ldh, ws);
}

void syrk_nt_lower2(hipStream_t st, int64_t m0, int64_t m1, int64_t k, const double* X0, int64_t ldx0,
                    const double* X1, int64_t ldx1, const double* w, const double* dvec, double* H, int64_t ldh,
                    double* ws) {
  if (m1 <= 0) {
    syrk_nt_lower(st, m0, k, X0, ldx0, w, dvec, H, ldh, ws);
    return;
  }
  m0 = std::max<int64_t>(m0, 0);
  syrk_nt_launch(st, m0 + m1, k, X0, ldx0, w, dvec, H, ldh, ws, NtSecond{m0, X1, ldx1});
}

void syrk_nt_lower3(hipStream_t st, int64_t m0, int64_t m1, int64_t m2, int64_t k, const double* X0, int64_t ldx0,
                    const double* X1, int64_t ldx1, const double* X2, int64_t ldx2, const double* w,
                    const double* dvec, double* H, int64_t ldh, double* ws) {
  // an empty block leaves a two-operand (or one-operand) stack: the same rows in the same order, and the empty
  // block's pointer goes nowhere
  if (m2 <= 0) {
    syrk_nt_lower2(st, m0, m1, k, X0, ldx0, X1, ldx1, w, dvec, H, ldh, ws);
    return;
  }
  if (m1 <= 0) {
    syrk_nt_lower2(st, m0, m2, k, X0, ldx0, X2, ldx2, w, dvec, H, ldh, ws);
    return;
  }
  if (m0 <= 0) {
    syrk_nt_lower2(st, m1, m2, k, X1, ldx1, X2, ldx2, w, dvec, H, ldh, ws);
    return;
  }
  syrk_nt_launch(st, m0 + m1 + m2, k, X0, ldx0, w, dvec, H, ldh, ws, NtThird{m0, X1, ldx1, m0 + m1, X2, ldx2});
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

extern "C" int ipm_syrk_nt3(ipm_handle* h, int64_t m0, int64_t m1, int64_t m2, int64_t k, const double* X0,
                            int64_t ldx0, const double* X1, int64_t ldx1, const double* X2, int64_t ldx2,
                            const double* w, const double* dvec, double* H, int64_t ldh) {
  if (!h || m0 < 0 || m1 < 0 || m2 < 0 || k < 0) return IPM_INVALID_ARG;
  if (m2 == 0) return ipm_syrk_nt2(h, m0, m1, k, X0, ldx0, X1, ldx1, w, dvec, H, ldh);
  if (m1 == 0) return ipm_syrk_nt2(h, m0, m2, k, X0, ldx0, X2, ldx2, w, dvec, H, ldh);
  if (m0 == 0) return ipm_syrk_nt2(h, m1, m2, k, X1, ldx1, X2, ldx2, w, dvec, H, ldh);
  const int64_t m = m0 + m1 + m2;
  if (ldh < m || (k > 0 && (ldx0 < k || ldx1 < k || ldx2 < k))) return IPM_INVALID_ARG;
  if (!H || (k > 0 && (!X0 || !X1 || !X2))) return IPM_INVALID_ARG;
  double* ws = nullptr;
  const int64_t wd = syrk_nt_ws_doubles(m, k);
  if (wd > 0) {
    ws = ipm_handle_scratch(h, (size_t)wd * sizeof(double));
    if (!ws) { h->err = "scratch alloc failed"; return IPM_HIP_ERROR; }
  }
  syrk_nt_lower3(h->stream, m0, m1, m2, k, X0, ldx0, X1, ldx1, X2, ldx2, w, dvec, H, ldh, ws);
  HIPCHK(h, hipGetLastError());
  return IPM_OK;
}
