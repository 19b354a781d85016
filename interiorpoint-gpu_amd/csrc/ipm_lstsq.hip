// Minimum-norm least squares for the symmetric Newton systems: the reference's
//   np.linalg.lstsq(H, rhs, rcond=None)
// (NewtonSolver.py:212-227 np_lstsq, :334-341 the Cholesky-failure backup (Q9);
//  NewtonSolverInfeasibleStart.py:279-316 np_lstsq block elimination, :692-724 the diagonal class).
//
// NumPy's lstsq is LAPACK gelsd: singular values s_i <= rcond * s_max are treated as zero, with
// rcond = eps * max(M, N) when rcond is None.  Every matrix the reference hands to lstsq on this
// path is symmetric (H, and S = A H^+ A^T), so its singular values are |lambda_i| and its singular
// vectors are eigenvectors:
//   x = sum_{|lambda_i| > eps n max|lambda|} v_i (v_i^T b) / lambda_i
// which is the gelsd solution up to rounding (the same minimum-norm vector whenever H is
// singular, where an LU solve returns a huge or non-finite step instead).
//
// The eigendecomposition is a hand-written parallel cyclic Jacobi method (no vendor library):
// every round rotates n/2 disjoint index pairs (p, q) at once -- the round-robin "circle"
// ordering visits every pair once per sweep of n-1 rounds -- with the rotation that zeroes A_pq
// (Golub & Van Loan, sym.schur2), applied two-sided to A (each thread owns a 2 x 2 block of A, so
// the update is in place) and to the columns of V.  Sweeps repeat until no off-diagonal entry is
// rotated: |A_pq| <= eps sqrt|A_pp A_qq| (relative), or |A_pq| <= eps ||A||_F / n (absolute:
// the off-diagonal rest then moves an eigenvalue by at most eps ||A||_F, the backward error of
// gelsd itself).  The absolute bound is needed on rank-deficient H: in the null-space block
// A_pp, A_qq and A_pq are all rounding noise of the large rotations, the relative test keeps
// rotating that noise forever (a numpy restatement at n = 1025, rank 700 never stops), and those
// eigenvalues fall below gelsd's cut anyway.  Small systems (n <= JWG_MAX) run the whole iteration in
// ONE workgroup (no launches per round); larger ones one rotation + one update launch per round and
// a 4-byte readback per sweep.  Non-convergence within JMAX_SWEEPS sets *info_dev = 1 (the host
// raises LinAlgError like numpy's "SVD did not converge"), and so does a matrix with a NaN or Inf
// entry (numpy's lstsq raises on those too); the word is sticky -- a factorization
// never clears it, so of several eigensolves in one Newton step (the block elimination's H and S)
// a failed one cannot be overwritten by a later converged one.
// Right-hand sides use the engine's row-major convention: B is n x nrhs, element (i, j) at
// B[i * ldb + j].
#include <hip/hip_runtime.h>

#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ipm_common.h"

namespace ipm {

constexpr int JWG_MAX = 256;       // single-workgroup path up to this n
constexpr int JMAX_SWEEPS = 60;

// pair i of round r in the circle ordering of nn (even) players: player 0 fixed, the others rotate
__device__ __forceinline__ void circle_pair(int nn, int r, int i, int& a, int& b) {
  const int m = nn - 1;
  a = (i == 0) ? 0 : ((i - 1 + r) % m) + 1;
  b = ((nn - 2 - i + r) % m) + 1;
}

// rotation (c, s) zeroing A_pq (p < q): J = [[c, s], [-s, c]] on rows / columns (p, q)
__device__ __forceinline__ bool jacobi_rot(double app, double aqq, double apq, double tiny, double& c, double& s) {
  const double ap = fabs(apq);
  if (!(ap > DBL_EPSILON * sqrt(fabs(app) * fabs(aqq))) || !(ap > tiny)) {
    c = 1.0;
    s = 0.0;
    return false;
  }
  const double tau = (aqq - app) / (2.0 * apq);
  const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
  c = 1.0 / sqrt(1.0 + t * t);
  s = t * c;
  return true;
}

// (a, b) -> (c a - s b, s a + c b) written as a correction of (a, b), with t = s / (1 + c) = tan(phi / 2)
// (Rutishauser's form of the Jacobi update): the rounding error is proportional to |s| instead of
// to |a|, |b|, so a small-angle rotation adds next to nothing.  The blocked Jacobi uses it for the
// inner sweeps after the first (IPM_BJ_INNER > 1), whose rotations are mostly small: with the plain
// form k inner sweeps cost k times the rounding of one (orthogonality of V 2.9, 5.7, 8.2 n eps for
// k = 1, 2, 3 at n = 257) without saving an outer sweep.  The first inner sweep -- the only one by
// default -- keeps the plain form, so default results are bit for bit what they were.
__device__ __forceinline__ void rot_fine(double s, double t, double a, double b, double& ra, double& rb) {
  ra = a - s * (b + t * a);
  rb = b + s * (a - t * b);
}

// pair encoding: p | (q << 16), q = JSINGLE when the pair is an odd n's last index with the dummy
// player -- a single index p that no rotation touches, but whose entries in the rotated rows and
// columns of the OTHER pairs still turn with them
constexpr int JSINGLE = 0xFFFF;
__device__ __forceinline__ int jpack(int p, int q, int n) { return p | ((q < n ? q : JSINGLE) << 16); }

// the block (rows of pair P, columns of pair Q) of A <- J^T A J, in place: 2 x 2 for two real pairs,
// 2 x 1 / 1 x 2 when one side is a single index (identity rotation on that side), nothing for two
// singles
__device__ __forceinline__ void jacobi_block(double* A, int64_t lda, int pp, double c1, double s1, int pq, double c2,
                                             double s2, bool diag) {
  const int p1 = pp & 0xFFFF, q1 = (pp >> 16) & 0xFFFF, p2 = pq & 0xFFFF, q2 = (pq >> 16) & 0xFFFF;
  const bool r2 = q1 != JSINGLE, k2 = q2 != JSINGLE;
  if (r2 && k2) {
    double* a11 = A + (int64_t)p2 * lda + p1;   // (p1, p2)
    double* a12 = A + (int64_t)q2 * lda + p1;   // (p1, q2)
    double* a21 = A + (int64_t)p2 * lda + q1;   // (q1, p2)
    double* a22 = A + (int64_t)q2 * lda + q1;   // (q1, q2)
    const double x11 = *a11, x12 = *a12, x21 = *a21, x22 = *a22;
    // rows: r_p = c r_p - s r_q, r_q = s r_p + c r_q
    const double y11 = c1 * x11 - s1 * x21, y12 = c1 * x12 - s1 * x22;
    const double y21 = s1 * x11 + c1 * x21, y22 = s1 * x12 + c1 * x22;
    // columns: likewise with the column pair's rotation
    double z11 = c2 * y11 - s2 * y12, z12 = s2 * y11 + c2 * y12;
    double z21 = c2 * y21 - s2 * y22, z22 = s2 * y21 + c2 * y22;
    if (diag) {   // the rotated pair itself: symmetric, off-diagonal zero by construction
      z12 = z21 = 0.0;
    }
    *a11 = z11;
    *a12 = z12;
    *a21 = z21;
    *a22 = z22;
  } else if (r2) {   // column p2 alone: rows (p1, q1) turn
    double* a11 = A + (int64_t)p2 * lda + p1;
    double* a21 = A + (int64_t)p2 * lda + q1;
    const double x11 = *a11, x21 = *a21;
    *a11 = c1 * x11 - s1 * x21;
    *a21 = s1 * x11 + c1 * x21;
  } else if (k2) {   // row p1 alone: columns (p2, q2) turn
    double* a11 = A + (int64_t)p2 * lda + p1;
    double* a12 = A + (int64_t)q2 * lda + p1;
    const double x11 = *a11, x12 = *a12;
    *a11 = c2 * x11 - s2 * x12;
    *a12 = s2 * x11 + c2 * x12;
  }
}

__device__ __forceinline__ void jacobi_vcols(double* V, int64_t n, int p, int q, double c, double s, int64_t k) {
  double* vp = V + (int64_t)p * n;
  double* vq = V + (int64_t)q * n;
  const double a = vp[k], b = vq[k];
  vp[k] = c * a - s * b;
  vq[k] = s * a + c * b;
}

// ||A||_F^2 in two fixed-order stages (deterministic): workgroup b sums the squares of columns
// b, b + G, b + 2G, ... (G = gridDim.x) into part[b]; k_frob2_fin adds the G partial sums.
// A sum that is not finite (a NaN or Inf entry, or squares that overflow) sets the sticky info word:
// the rotation threshold derived from it would be NaN or Inf, no entry would ever pass
// jacobi_rot's tests, and the iteration would "converge" at once on a matrix it never looked at.
__global__ __launch_bounds__(256) void k_frob2(int64_t n, const double* __restrict__ A, int64_t lda, double* part) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int64_t j = blockIdx.x; j < n; j += gridDim.x)
    for (int64_t i = threadIdx.x; i < n; i += 256) {
      const double v = A[j * lda + i];
      acc = fma(v, v, acc);
    }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void k_frob2_fin(int np, const double* __restrict__ part, double* out,
                                                     int* info) {
  __shared__ double red[256];
  red[threadIdx.x] = (int)threadIdx.x < np ? part[threadIdx.x] : 0.0;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *out = red[0];
    if (!(red[0] <= DBL_MAX)) *info = 1;   // NaN or +Inf (a sum of squares is never negative)
  }
}

__global__ void k_eye(int64_t n, double* V) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n * n) V[e] = (e / n == e % n) ? 1.0 : 0.0;
}

// whole Jacobi iteration in one workgroup (n <= JWG_MAX): A, V in global memory (L2-resident)
__global__ __launch_bounds__(1024) void k_jacobi_wg(int n, double* A, int64_t lda, double* V, const double* frob2,
                                                    int* info) {
  __shared__ int spart[JWG_MAX + 1];
  __shared__ double sc[JWG_MAX + 1], ss[JWG_MAX + 1];
  __shared__ int srot;
  const int nn = n + (n & 1), half = nn / 2, tid = threadIdx.x;
  const double tiny = DBL_EPSILON * sqrt(*frob2) / (double)n;
  int sweep = 0;
  for (; sweep < JMAX_SWEEPS; ++sweep) {
    if (tid == 0) srot = 0;
    __syncthreads();
    for (int r = 0; r < nn - 1; ++r) {
      for (int i = tid; i < half; i += 1024) {
        int a, b;
        circle_pair(nn, r, i, a, b);
        const int p = min(a, b), q = max(a, b);
        double c = 1.0, s = 0.0;
        if (q < n && jacobi_rot(A[(int64_t)p * lda + p], A[(int64_t)q * lda + q], A[(int64_t)q * lda + p], tiny, c, s))
          atomicAdd(&srot, 1);
        spart[i] = jpack(p, q, n);
        sc[i] = c;
        ss[i] = s;
      }
      __syncthreads();
      // A blocks (pair P, pair Q) and V column pairs
      for (int e = tid; e < half * half; e += 1024) {
        const int P = e / half, Q = e % half;
        const int pp = spart[P], pq = spart[Q];
        if (sc[P] == 1.0 && ss[P] == 0.0 && sc[Q] == 1.0 && ss[Q] == 0.0) continue;
        jacobi_block(A, lda, pp, sc[P], ss[P], pq, sc[Q], ss[Q], P == Q);
      }
      for (int e = tid; e < half * n; e += 1024) {
        const int P = e / n, k = e % n;
        const int pp = spart[P];
        if (sc[P] == 1.0 && ss[P] == 0.0) continue;   // (singles always: identity)
        jacobi_vcols(V, n, pp & 0xFFFF, pp >> 16, sc[P], ss[P], k);
      }
      __syncthreads();
    }
    if (srot == 0) break;
    __syncthreads();
  }
  if (tid == 0 && sweep >= JMAX_SWEEPS) *info = 1;   // sticky: never cleared here
}

// ---------------------------------------------------------------------------------------------
// Large n: BLOCKED two-sided Jacobi.  The index range is cut into nb = ceil(n / 32) blocks of 32
// (an odd count gets one empty block); every round pairs the blocks by the same circle ordering
// and, for each pair (P, Q), rotates the 64 x 64 subproblem S = A[P u Q, P u Q] by one cyclic sweep
// (k_bj_eig: the cyclic Jacobi above, in LDS, one workgroup per pair) into S' = G^T S G.  The
// orthogonal G (64 x 64) is then applied to the whole matrix on MFMA tiles -- rows
// A[P u Q, :] <- G^T A[P u Q, :] (k_bj_rows), then columns A[:, P u Q] <- A[:, P u Q] G and
// V[:, P u Q] <- V[:, P u Q] G (k_bj_cols) -- and the pair's own 64 x 64 block is replaced by the
// rotated S' (whose rotated entries are exact zeros, like the 2 x 2 form's).  A sweep is
// nb - 1 rounds; the sweeps stop when no subproblem rotated anything (the same per-entry tests as
// the 2 x 2 method, so the stopping rule and the answer are the same; a sweep of the outer loop is
// the convergence unit, JMAX_SWEEPS of them without convergence sets the info word).  Work per sweep ~12 n^3
// flops on MFMA instead of n - 1 rounds of scattered 2 x 2 updates over all of A and V; a pair
// whose subproblem did not rotate (most of them in the last sweeps) skips its updates.
constexpr int BJ = 32;         // block size
constexpr int BS = 2 * BJ;     // subproblem size
constexpr int BLD = BS + 1;    // LDS leading dimension (odd: conflict-free row and column walks)

__device__ __forceinline__ int64_t bj_index(int P, int Q, int k) {
  return k < BJ ? (int64_t)P * BJ + k : (int64_t)Q * BJ + (k - BJ);
}

// per-pair scratch: G (BS x BS, column-major) | S' (BS x BS) ; rot flags (one int per pair)
// 1024 threads: one 2 x 2 block of S and two G pairs per thread per rotation round (the rounds
// are latency-bound; 32 pairs per round of the circle ordering)
constexpr int BJ_EIG_T = 1024;
__global__ __launch_bounds__(BJ_EIG_T) void k_bj_eig(int n, int nbp, int r, const double* __restrict__ A, int64_t lda,
                                                const double* frob2, double* __restrict__ gbuf,
                                                int* __restrict__ rflag, int* __restrict__ nrot, int inner) {
  __shared__ double S[BS * BLD], G[BS * BLD];
  __shared__ double sc[BS / 2], ss[BS / 2];
  __shared__ int sp[BS / 2], sq[BS / 2];
  __shared__ int srot;
  const int pair = blockIdx.x, tid = threadIdx.x;
  int a, b;
  circle_pair(nbp, r, pair, a, b);
  const int P = min(a, b), Q = max(a, b);
  // S from the lower triangle of A (symmetrised: the updates keep A symmetric only to rounding)
  for (int e = tid; e < BS * BS; e += BJ_EIG_T) {
    const int i = e % BS, j = e / BS;
    const int64_t gi = bj_index(P, Q, i), gj = bj_index(P, Q, j);
    double v = 0.0;
    if (gi < n && gj < n) v = gi >= gj ? A[gj * lda + gi] : A[gi * lda + gj];
    S[j * BLD + i] = v;
    G[j * BLD + i] = (i == j) ? 1.0 : 0.0;
  }
  const double tiny = DBL_EPSILON * sqrt(*frob2) / (double)n;
  int total = 0, sweep = 0;
  if (tid == 0) srot = 0;
  __syncthreads();
  // a subproblem none of whose 2016 pairs passes jacobi_rot's rotation test would come out of the
  // sweep unchanged (G = I, S' = S, no rotation: S never changes, so every round sees the same
  // entries) -- skip the 63 rounds then (most pairs of the last outer sweeps; bitwise the same)
  {
    int any = 0;
    for (int e = tid; e < BS * BS; e += BJ_EIG_T) {
      const int p = e % BS, q = e / BS;
      if (p < q) {
        const double ap = fabs(S[q * BLD + p]);
        any |= (ap > DBL_EPSILON * sqrt(fabs(S[p * BLD + p]) * fabs(S[q * BLD + q])) && ap > tiny) ? 1 : 0;
      }
    }
    if (any) srot = 1;   // (benign race: every writer stores 1)
    __syncthreads();
    if (srot == 0) inner = 0;
    __syncthreads();
  }
  for (; sweep < inner; ++sweep) {
    if (tid == 0) srot = 0;
    __syncthreads();
    for (int rr = 0; rr < BS - 1; ++rr) {
      if (tid < BS / 2) {
        int x, y;
        circle_pair(BS, rr, tid, x, y);
        const int p = min(x, y), q = max(x, y);
        double c = 1.0, s = 0.0;
        if (jacobi_rot(S[p * BLD + p], S[q * BLD + q], S[q * BLD + p], tiny, c, s)) atomicAdd(&srot, 1);
        sp[tid] = p;
        sq[tid] = q;
        sc[tid] = c;
        ss[tid] = s;
      }
      __syncthreads();
      // S <- J^T S J, 2 x 2 blocks (row pair I, column pair K)
      for (int e = tid; e < (BS / 2) * (BS / 2); e += BJ_EIG_T) {
        const int I = e % (BS / 2), K = e / (BS / 2);
        const double c1 = sc[I], s1 = ss[I], c2 = sc[K], s2 = ss[K];
        if (s1 == 0.0 && s2 == 0.0) continue;   // (s == 0 <=> identity: jacobi_rot's c is then 1)
        const int p1 = sp[I], q1 = sq[I], p2 = sp[K], q2 = sq[K];
        const double x11 = S[p2 * BLD + p1], x12 = S[q2 * BLD + p1], x21 = S[p2 * BLD + q1], x22 = S[q2 * BLD + q1];
        double z11, z12, z21, z22;
        if (sweep == 0) {
          const double y11 = c1 * x11 - s1 * x21, y12 = c1 * x12 - s1 * x22;
          const double y21 = s1 * x11 + c1 * x21, y22 = s1 * x12 + c1 * x22;
          z11 = c2 * y11 - s2 * y12;
          z12 = s2 * y11 + c2 * y12;
          z21 = c2 * y21 - s2 * y22;
          z22 = s2 * y21 + c2 * y22;
        } else {   // (further inner sweeps: the small-angle form, see rot_fine)
          const double t1 = s1 / (1.0 + c1), t2 = s2 / (1.0 + c2);
          double y11, y12, y21, y22;
          rot_fine(s1, t1, x11, x21, y11, y21);
          rot_fine(s1, t1, x12, x22, y12, y22);
          rot_fine(s2, t2, y11, y12, z11, z12);
          rot_fine(s2, t2, y21, y22, z21, z22);
        }
        if (I == K) z12 = z21 = 0.0;
        S[p2 * BLD + p1] = z11;
        S[q2 * BLD + p1] = z12;
        S[p2 * BLD + q1] = z21;
        S[q2 * BLD + q1] = z22;
      }
      // G <- G J (columns p, q of every row k)
      for (int e = tid; e < (BS / 2) * BS; e += BJ_EIG_T) {
        const int I = e / BS, k = e % BS;
        const double c = sc[I], s = ss[I];
        if (s == 0.0) continue;
        const int p = sp[I], q = sq[I];
        const double u = G[p * BLD + k], w = G[q * BLD + k];
        if (sweep == 0) {
          G[p * BLD + k] = c * u - s * w;
          G[q * BLD + k] = s * u + c * w;
        } else {
          double gu, gw;
          rot_fine(s, s / (1.0 + c), u, w, gu, gw);
          G[p * BLD + k] = gu;
          G[q * BLD + k] = gw;
        }
      }
      __syncthreads();
    }
    const int nr = srot;
    total += nr;
    __syncthreads();
    if (nr == 0) break;
  }
  double* go = gbuf + (int64_t)pair * 2 * BS * BS;
  for (int e = tid; e < BS * BS; e += BJ_EIG_T) {
    const int i = e % BS, j = e / BS;
    go[e] = G[j * BLD + i];
    go[BS * BS + e] = S[j * BLD + i];
  }
  if (tid == 0) {
    rflag[pair] = total > 0 ? 1 : 0;
    if (total > 0) atomicAdd(nrot, total);
  }
}

// One 64 x 64 output tile on fp64 MFMA (16x16x4; cdna_hip_programming.md §3 maps: A lane l:
// A[l&15][l>>4], B lane l: B[l>>4][l&15], D lane l, reg r: D[(l>>4)+4r][l&15]).  Wave w computes
// output rows [16 w, 16 w + 16) x all 64 columns; D(i, j) = sum_k opA(i, k) opB(k, j) with
// opA(i, k) = LA[ia(i, k)] and opB(k, j) = LB[ib(k, j)] read from LDS; D goes back to LDS tile Out
// (column-major, BLD) -- the caller stores it coalesced.
template <class FA, class FB>
__device__ __forceinline__ void bj_tile(FA fa, FB fb, double* Out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i0 = 16 * wv, li = lane & 15, lk = lane >> 4;
  dbl4 acc[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) acc[jt] = dbl4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int k0 = 0; k0 < BS; k0 += 4) {
    const double av = fa(i0 + li, k0 + lk);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, fb(k0 + lk, 16 * jt + li), acc[jt], 0, 0, 0);
  }
  __syncthreads();   // every operand read before Out (which may alias an operand) is written
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) Out[(16 * jt + li) * BLD + i0 + lk + 4 * rr] = acc[jt][rr];
  __syncthreads();
}

// rows: A[P u Q, c0 : c0 + 64] <- G^T A[P u Q, c0 : c0 + 64]
__global__ __launch_bounds__(256) void k_bj_rows(int n, int nbp, int r, double* __restrict__ A, int64_t lda,
                                                 const double* __restrict__ gbuf, const int* __restrict__ rflag) {
  const int pair = blockIdx.y;
  if (!rflag[pair]) return;
  __shared__ double Gl[BS * BLD], X[BS * BLD];
  int a, b;
  circle_pair(nbp, r, pair, a, b);
  const int P = min(a, b), Q = max(a, b), tid = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * BS;
  const double* g = gbuf + (int64_t)pair * 2 * BS * BS;
  for (int e = tid; e < BS * BS; e += 256) {
    const int k = e % BS, j = e / BS;
    Gl[j * BLD + k] = g[e];
    const int64_t gi = bj_index(P, Q, k), gj = c0 + j;
    X[j * BLD + k] = (gi < n && gj < n) ? A[gj * lda + gi] : 0.0;   // X(k, j)
  }
  __syncthreads();
  // D(i, j) = sum_k G(k, i) X(k, j)
  bj_tile([&](int i, int k) { return Gl[i * BLD + k]; }, [&](int k, int j) { return X[j * BLD + k]; }, X);
  for (int e = tid; e < BS * BS; e += 256) {
    const int i = e % BS, j = e / BS;
    const int64_t gi = bj_index(P, Q, i), gj = c0 + j;
    if (gi < n && gj < n) A[gj * lda + gi] = X[j * BLD + i];
  }
}

// A <- J^T A J in ONE pass: the tile of A on pair I's rows and pair J's columns (64 x 64, the same
// pairing on both sides) becomes G_I^T T G_J -- A is read and written once per round instead of
// twice (a row pass, then a column pass).  The pair's own tile (I == J) takes the rotated S'.  A
// pair that did not rotate has G = I exactly, so its product is exact (no skip needed for one side).
__global__ __launch_bounds__(256) void k_bj_tile(int n, int nbp, int r, double* __restrict__ A, int64_t lda,
                                                 const double* __restrict__ gbuf, const int* __restrict__ rflag) {
  const int I = blockIdx.x, J = blockIdx.y;
  if (!rflag[I] && !rflag[J]) return;
  __shared__ double Gl[BS * BLD], T[BS * BLD];
  int a, b;
  circle_pair(nbp, r, I, a, b);
  const int PI = min(a, b), QI = max(a, b);
  circle_pair(nbp, r, J, a, b);
  const int PJ = min(a, b), QJ = max(a, b);
  const int tid = threadIdx.x;
  const double* gI = gbuf + (int64_t)I * 2 * BS * BS;
  if (I == J) {
    const double* sfin = gI + BS * BS;
    for (int e = tid; e < BS * BS; e += 256) {
      const int i = e % BS, j = e / BS;
      const int64_t gi = bj_index(PI, QI, i), gj = bj_index(PJ, QJ, j);
      if (gi < n && gj < n) A[gj * lda + gi] = sfin[e];
    }
    return;
  }
  for (int e = tid; e < BS * BS; e += 256) {
    const int k = e % BS, j = e / BS;
    Gl[j * BLD + k] = gI[e];   // G_I(k, j)
    const int64_t gi = bj_index(PI, QI, k), gj = bj_index(PJ, QJ, j);
    T[j * BLD + k] = (gi < n && gj < n) ? A[gj * lda + gi] : 0.0;   // T(k, j)
  }
  __syncthreads();
  // T <- G_I^T T : D(i, j) = sum_k G_I(k, i) T(k, j)
  bj_tile([&](int i, int k) { return Gl[i * BLD + k]; }, [&](int k, int j) { return T[j * BLD + k]; }, T);
  const double* gJ = gbuf + (int64_t)J * 2 * BS * BS;
  for (int e = tid; e < BS * BS; e += 256) Gl[(e / BS) * BLD + e % BS] = gJ[e];   // G_J(k, j)
  __syncthreads();
  // T <- T G_J : D(i, j) = sum_k T(i, k) G_J(k, j)
  bj_tile([&](int i, int k) { return T[k * BLD + i]; }, [&](int k, int j) { return Gl[j * BLD + k]; }, T);
  for (int e = tid; e < BS * BS; e += 256) {
    const int i = e % BS, j = e / BS;
    const int64_t gi = bj_index(PI, QI, i), gj = bj_index(PJ, QJ, j);
    if (gi < n && gj < n) A[gj * lda + gi] = T[j * BLD + i];
  }
}

// columns: M[r0 : r0 + 64, P u Q] <- M[r0 : r0 + 64, P u Q] G for M = A (z = 0) and V (z = 1);
// in A the pair's own rows take the diagonalised S' instead
__global__ __launch_bounds__(256) void k_bj_cols(int n, int nbp, int r, double* __restrict__ A, int64_t lda,
                                                 double* __restrict__ V, int64_t ldv,
                                                 const double* __restrict__ gbuf, const int* __restrict__ rflag,
                                                 int vonly) {
  const int pair = blockIdx.y;
  if (!rflag[pair]) return;
  __shared__ double Gl[BS * BLD], Y[BS * BLD];
  int a, b;
  circle_pair(nbp, r, pair, a, b);
  const int P = min(a, b), Q = max(a, b), tid = threadIdx.x;
  const bool isA = !vonly && blockIdx.z == 0;
  double* M = isA ? A : V;
  const int64_t ld = isA ? lda : ldv;
  const int64_t r0 = (int64_t)blockIdx.x * BS;
  const double* g = gbuf + (int64_t)pair * 2 * BS * BS;
  for (int e = tid; e < BS * BS; e += 256) {
    const int i = e % BS, k = e / BS;
    Gl[k * BLD + i] = g[e];   // G(i, k)
    const int64_t gi = r0 + i, gk = bj_index(P, Q, k);
    Y[k * BLD + i] = (gi < n && gk < n) ? M[gk * ld + gi] : 0.0;   // Y(i, k)
  }
  __syncthreads();
  // D(i, j) = sum_k Y(i, k) G(k, j)
  bj_tile([&](int i, int k) { return Y[k * BLD + i]; }, [&](int k, int j) { return Gl[j * BLD + k]; }, Y);
  const double* sfin = g + BS * BS;
  for (int e = tid; e < BS * BS; e += 256) {
    const int i = e % BS, j = e / BS;
    const int64_t gi = r0 + i, gj = bj_index(P, Q, j);
    if (gi >= n || gj >= n) continue;
    double v = Y[j * BLD + i];
    if (isA) {
      const int64_t blk = gi / BJ;
      if (blk == P) v = sfin[j * BS + (int)(gi % BJ)];
      else if (blk == Q) v = sfin[j * BS + BJ + (int)(gi % BJ)];
    }
    M[gj * ld + gi] = v;
  }
}

// eigenvalues (diagonal of the rotated A) -> pseudo-inverse weights f_i = 1/lambda_i if
// |lambda_i| > eps * n * max|lambda| else 0 (gelsd's rcond=None rule)
__global__ __launch_bounds__(256) void k_jacobi_weights(int64_t n, const double* __restrict__ A, int64_t lda,
                                                        double* __restrict__ f) {
  __shared__ double red[256];
  double m = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) m = fmax(m, fabs(A[i * lda + i]));
  red[threadIdx.x] = m;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  const double cut = DBL_EPSILON * (double)n * red[0];
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double l = A[i * lda + i];
    f[i] = (fabs(l) > cut) ? 1.0 / l : 0.0;
  }
}

// T(i, r) = f_i sum_k V(k, i) B(k, r): one wave per (i, r), lanes split k (V column i contiguous)
__global__ __launch_bounds__(256) void k_vtb(int64_t n, int64_t nrhs, const double* __restrict__ V, int64_t ldv,
                                             const double* __restrict__ B, int64_t ldb, const double* __restrict__ f,
                                             double* __restrict__ T) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= n * nrhs) return;
  const int64_t i = w / nrhs, r = w % nrhs;
  const double* v = V + i * ldv;
  double acc = 0.0;
  for (int64_t k = lane; k < n; k += 64) acc = fma(v[k], B[k * ldb + r], acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) T[r * n + i] = f[i] * acc;
}

// B(i, r) = sum_k V(i, k) T(k, r): one thread per (i, r); V(i, k) for fixed k is contiguous in i
__global__ __launch_bounds__(256) void k_vt(int64_t n, int64_t nrhs, const double* __restrict__ V, int64_t ldv,
                                            const double* __restrict__ T, double* __restrict__ B, int64_t ldb) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * nrhs) return;
  const int64_t i = e % n, r = e / n;
  const double* t = T + r * n;
  double acc = 0.0;
  for (int64_t k = 0; k < n; ++k) acc = fma(V[k * ldv + i], t[k], acc);
  B[i * ldb + r] = acc;
}

// T (row-major n x nrhs) rows scaled by f
__global__ void k_scale_rows(int64_t n, int64_t nrhs, const double* __restrict__ f, double* __restrict__ T) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n * nrhs) T[e] *= f[e / nrhs];
}

// upper triangle <- lower triangle, in place (column-major, ld): the two element sets are
// disjoint, so no scratch copy is needed
__global__ void k_sym_expand(int64_t n, double* __restrict__ M, int64_t ld) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * n) return;
  const int64_t i = e % n, j = e / n;
  if (i < j) M[j * ld + i] = M[i * ld + j];
}
void sym_expand_inplace(hipStream_t st, int64_t n, double* M, int64_t ld) {
  if (n > 1) hipLaunchKernelGGL(k_sym_expand, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, st, n, M, ld);
}

void lstsq_release(void* rb) { (void)rb; }

static std::atomic<int> g_fail_call{-1};
void set_lstsq_fail_call(int k) { g_fail_call.store(k); }
__global__ void k_set_flag(int* p) { *p = 1; }

// inner cyclic sweeps per subproblem and round (IPM_BJ_INNER, default 1): the subproblem need not
// be diagonalised completely -- every index pair is still rotated in every outer sweep, and the
// outer stopping rule (a sweep without any rotation) is unchanged, so is the answer's accuracy
static int bj_inner_sweeps() {
  static const int v = [] { const char* e = getenv("IPM_BJ_INNER"); return e ? std::max(1, atoi(e)) : 1; }();
  return v;
}
// IPM_BJ_FUSED=0: the two-pass A update (rows, then columns) instead of the one-pass tile update
static bool bj_fused() {
  static const bool v = [] { const char* e = getenv("IPM_BJ_FUSED"); return !(e && e[0] == '0'); }();
  return v;
}
static inline int64_t bj_pairs(int64_t n) {
  const int64_t nb = (n + BJ - 1) / BJ;
  return (nb + (nb & 1)) / 2;
}
// ws: f (n) | frob2 + counters (64) | V (n^2, column-major, ld n) | per-pair G + S' | rot flags | T (n * nrhs)
static inline int64_t ws_off_pairs(int64_t n) { return n + 64 + n * n; }
static inline int64_t ws_off_t(int64_t n) {
  return ws_off_pairs(n) + (n > JWG_MAX ? bj_pairs(n) * (2 * BS * BS + 1) : 0);
}
int64_t lstsq_ws_doubles(int64_t n, int64_t nrhs) { return ws_off_t(n) + std::max<int64_t>(nrhs, 1) * n; }

// A (full symmetric, column-major, lda): ws <- V (eigenvectors, column-major) and the
// pseudo-inverse weights f; A <- W = V^T (column-major, lda), the operand layout of the MFMA apply.
// *info_dev: set to 1 when Jacobi did not converge within JMAX_SWEEPS sweeps, or when ||A||_F^2 is
// not finite (sticky).
// Returns 0, or -1 on a launch error.
int lstsq_sym_factor(void** rb, hipStream_t st, int64_t n, double* A, int64_t lda, double* ws, int* info_dev) {
  (void)rb;
  if (n <= 0) return 0;
  if (n >= (1 << 15)) return -1;   // pair packing (16-bit indices)
  double* f = ws;
  double* frob2 = ws + n;
  int* nrot = reinterpret_cast<int*>(ws + n + 8);
  double* V = ws + n + 64;
  {
    // partial sums in V's first G slots (G <= n <= n^2; k_eye overwrites them next)
    const int G = (int)std::min<int64_t>(n, 256);
    hipLaunchKernelGGL(k_frob2, dim3(G), dim3(256), 0, st, n, A, lda, V);
    hipLaunchKernelGGL(k_frob2_fin, dim3(1), dim3(256), 0, st, G, V, frob2, info_dev);
  }
  hipLaunchKernelGGL(k_eye, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, st, n, V);
  if (n <= JWG_MAX) {
    hipLaunchKernelGGL(k_jacobi_wg, dim3(1), dim3(1024), 0, st, (int)n, A, lda, V, frob2, info_dev);
  } else {
    const int64_t nb = (n + BJ - 1) / BJ, nbp = nb + (nb & 1), np = nbp / 2, tiles = (n + BS - 1) / BS;
    double* gbuf = ws + ws_off_pairs(n);
    int* rflag = reinterpret_cast<int*>(gbuf + np * 2 * BS * BS);
    int sweep = 0;
    for (; sweep < JMAX_SWEEPS; ++sweep) {
      hipMemsetAsync(nrot, 0, sizeof(int), st);
      for (int r = 0; r < (int)nbp - 1; ++r) {
        hipLaunchKernelGGL(k_bj_eig, dim3((unsigned)np), dim3(BJ_EIG_T), 0, st, (int)n, (int)nbp, r, A, lda, frob2, gbuf,
                           rflag, nrot, bj_inner_sweeps());
        if (bj_fused()) {
          // A in one tile pass, V's columns in the column kernel (z = 1 only)
          hipLaunchKernelGGL(k_bj_tile, dim3((unsigned)np, (unsigned)np), dim3(256), 0, st, (int)n, (int)nbp, r, A,
                             lda, gbuf, rflag);
          hipLaunchKernelGGL(k_bj_cols, dim3((unsigned)tiles, (unsigned)np, 1), dim3(256), 0, st, (int)n, (int)nbp, r,
                             A, lda, V, n, gbuf, rflag, 1);
        } else {
          hipLaunchKernelGGL(k_bj_rows, dim3((unsigned)tiles, (unsigned)np), dim3(256), 0, st, (int)n, (int)nbp, r, A,
                             lda, gbuf, rflag);
          hipLaunchKernelGGL(k_bj_cols, dim3((unsigned)tiles, (unsigned)np, 2), dim3(256), 0, st, (int)n, (int)nbp, r,
                             A, lda, V, n, gbuf, rflag, 0);
        }
      }
      int h = 0;
      if (hipMemcpyAsync(&h, nrot, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess)
        return -1;
      static const bool dbg = getenv("IPM_BJ_DEBUG") != nullptr;
      if (dbg) fprintf(stderr, "blocked Jacobi n=%ld sweep %d: %d rotations\n", (long)n, sweep, h);
      if (h == 0) break;
    }
    if (sweep >= JMAX_SWEEPS) hipLaunchKernelGGL(k_set_flag, dim3(1), dim3(1), 0, st, info_dev);   // sticky
  }
  // debug knob: this call reports non-convergence
  if (g_fail_call.load() >= 0 && g_fail_call.fetch_sub(1) == 0)
    hipLaunchKernelGGL(k_set_flag, dim3(1), dim3(1), 0, st, info_dev);
  hipLaunchKernelGGL(k_jacobi_weights, dim3(1), dim3(256), 0, st, n, A, lda, f);
  // W = V^T into A's storage (V column-major = row-major V^T)
  transpose(st, n, n, V, n, A, lda);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// B (row-major n x nrhs, ldb) <- V diag(f) V^T B, with V, f (ws) and W = V^T (A) from
// lstsq_sym_factor.  Few right-hand sides or a small system: one pass over V per product (wave dot
// products); many: two MFMA GEMMs (gemm_kk: C(i, j) = sum_k X[k][i] Y[k][j]).
int lstsq_sym_apply(void** rb, hipStream_t st, int64_t n, int64_t nrhs, const double* W, int64_t ldw, double* B,
                    int64_t ldb, double* ws) {
  (void)rb;
  if (n <= 0 || nrhs <= 0) return 0;
  const double* f = ws;
  const double* V = ws + n + 64;
  double* T = ws + ws_off_t(n);
  // (the GEMM only pays for large systems; below n = 512 the dot-product kernels keep the summation
  // order the reference-run fixtures were matched with: meth_lp_eq_ineq_np_lstsq, n = 80 with 20
  // right-hand sides, flips one step size at t ~ 1e7 under the GEMM's order)
  if (nrhs < 8 || n < 512) {
    const int64_t waves = n * nrhs;
    hipLaunchKernelGGL(k_vtb, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, n, nrhs, V, n, B, ldb, f, T);
    hipLaunchKernelGGL(k_vt, dim3((unsigned)((n * nrhs + 255) / 256)), dim3(256), 0, st, n, nrhs, V, n, T, B, ldb);
  } else {
    // T (row-major n x nrhs): T(i, r) = sum_k V(k, i) B(k, r) -> C(r, i) with X = B, Y = W (W[k][i] = V(k, i))
    gemm_kk(st, nrhs, n, n, B, ldb, W, ldw, T, nrhs);
    hipLaunchKernelGGL(k_scale_rows, dim3((unsigned)((n * nrhs + 255) / 256)), dim3(256), 0, st, n, nrhs, f, T);
    // B(i, r) = sum_k V(i, k) T(k, r) -> C(r, i) with X = T, Y = V (V[k][i] = V(i, k), column-major)
    gemm_kk(st, nrhs, n, n, T, nrhs, V, n, B, ldb);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace ipm
