/*
 * ipm355.h -- C ABI of the MI355X (gfx950) interior-point Newton hot path.
 *
 * Drop-in boundary for the reference's Newton inner loop
 * (fdeguire03/InteriorPoint-GPU).  The reference is pure Python with no FFI;
 * its seam between the problem facades (LPSolver/QPSolver/SOCPSolver) and the
 * numerics is the "oracle protocol" of FunctionManager.py:94-195 and the
 * Newton protocol of NewtonSolver.py:80 / NewtonSolverInfeasibleStart.py:72.
 * Each entry point below names the reference interface it replaces.
 * The Python binding (ctypes) lives in interiorpoint-gpu_amd/ipm355/_lib.py;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - fp64 everywhere.  Dense inputs are row-major (C order) with explicit
 *     leading dimensions, exactly as NumPy hands them over.
 *   - Every pointer argument marked [dev] is a device pointer (in practice a
 *     torch tensor's data_ptr()); the library never allocates device memory on
 *     the hot path: the caller provides a workspace of ipm_workspace_bytes().
 *   - All work is enqueued on the handle's stream.  Entry points that return
 *     host scalars synchronise that stream once.
 *   - Return value: IPM_OK or an error code; ipm_last_error() has the text.
 */
#ifndef IPM355_H
#define IPM355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPM_OK 0
#define IPM_NOT_POSITIVE_DEFINITE 1 /* LAPACK potrf info > 0 (drives Q9 fallback) */
#define IPM_INVALID_ARG 2
#define IPM_HIP_ERROR 3
#define IPM_NOT_SUPPORTED 4
#define IPM_LINALG_NOT_CONVERGED 5 /* the least-squares eigensolver did not converge (numpy: LinAlgError
                                      "SVD did not converge in Linear Least Squares") */

/* problem kinds (LPSolver.py / QPSolver.py / SOCPSolver.py) */
#define IPM_KIND_LP 0
#define IPM_KIND_QP 1
#define IPM_KIND_SOCP 2

/* linear-solve strategies (dispatch tables LPSolver.py:371-469, QPSolver.py:385-455) */
#define IPM_SOLVE_CHOLESKY 0 /* dense Cholesky; first failure -> permanent fallback (Q9) */
#define IPM_SOLVE_DIAGONAL 1 /* H diagonal (LP, C is None, try_diag) */
#define IPM_SOLVE_LU 2       /* np_solve / direct: LU with partial pivoting */
#define IPM_SOLVE_LSTSQ 3    /* np_lstsq: minimum-norm least squares (lstsq(H, -g, rcond=None)) */
#define IPM_SOLVE_DIAGONAL_LSTSQ 4 /* diagonal H, equality system S = A H^-1 A^T by lstsq
                                      (NewtonSolverNPLstSqDiagonalInfeasibleStart) */
#define IPM_SOLVE_CG 5       /* cg: NewtonSolverCG (NewtonSolver.py:365-400), scipy.sparse.linalg.cg's loop
                                on the device, warm start included; feasible start only (p > 0:
                                IPM_NOT_SUPPORTED); H is never factored, so Q9 does not apply */
#define IPM_SOLVE_CHOLESKY_DUAL 6 /* extension (the reference has no such method): the dual form of the LP
                                Newton step.  H = diag(D) + C^T diag(w) C is a positive diagonal plus
                                a rank-m term, so with E = 1/D the step solves the m x m system
                                  S = diag(1/w) + C diag(E) C^T,   z = S^-1 C (E o -g),
                                  dx = E o (-g - C^T z)
                                (Sherman-Morrison-Woodbury) by a bordered Cholesky of S, followed by
                                three rounds of iterative refinement on the residual -g - H dx (H
                                applied as diag(D) + C^T diag(w) C, solved through S again); no
                                n x n array is allocated.  ipm_problem_create returns IPM_NOT_SUPPORTED
                                unless the problem is an LP (not phase 1: that is method 7) with inequality rows
                                (m > 0), at least one box bound and no equality rows.
                                ipm_fm_hessian returns IPM_NOT_SUPPORTED (there is no H).  No Q9:
                                a failed or non-finite factorization of S ends the Newton solve with
                                linalg_error = 1, use_backup stays 0.  Numerics: DESIGN.md §11 */
#define IPM_SOLVE_CHOLESKY_DUAL_PHASE1 7 /* extension: the dual form of the LP PHASE-1 Newton step.  The
                                phase-1 Hessian is H~ = [[Hxx, h], [h^T, hss]] with Hxx = diag(D) +
                                C^T diag(w) C the matrix method 6 inverts and the variable s one bordering
                                column, so with ONE factorization of S = diag(1/w) + C diag(E) C^T
                                  y = Hxx^-1 h,  u = Hxx^-1 (-g_x),  sigma = hss - h.y (formed as a sum
                                  of squares over the slack rows: no cancellation),
                                  ds = (-g_s - h.u) / sigma,  dx = u - y ds,
                                then the refinement rounds of method 6 on the residual of the full
                                bordered system (H~ applied through C, never formed; y is not
                                refined).  No (n+1) x (n+1) array is allocated.  ipm_problem_create
                                returns IPM_NOT_SUPPORTED unless the problem is an LP with phase1 = 1,
                                inequality rows (m > 0), at least one box bound, no equality rows.
                                ipm_fm_hessian returns IPM_NOT_SUPPORTED.  No Q9: a failed
                                factorization of S, or a sigma that is not finite and positive, ends
                                the Newton solve with linalg_error = 1, use_backup stays 0.
                                use_psd_condition adds 1e-9 to D and to hss (all n + 1 diagonal
                                entries of H~).  Numerics: DESIGN.md §11.1 */
#define IPM_SOLVE_CHOLESKY_DUAL_EQ 8 /* extension: the dual form of the LP Newton step WITH equality rows
                                (infeasible start).  H dx + A^T nu = -g, A dx = -(A x - b), dv = nu - v with
                                H = diag(D) + C^T diag(w) C.  With E = 1/D, z = w o (C dx) and M = [C; A]
                                (rows stacked, never copied) the step solves ONE symmetric system of order
                                m + p,
                                  K = diag([1/w; 0]) + M diag(E) M^T,
                                  K [z; nu] = [C (E o -g); A (E o -g) + (A x - b)],
                                  dx = E o (-g - C^T z - A^T nu),
                                by a bordered Cholesky of K (positive definite when A has full row rank),
                                followed by the refinement rounds of method 6 on the residual of the full
                                KKT system (H applied through C, never formed).  No n x n and no n x p
                                array is allocated, and desc.AT is not read (it may be NULL).
                                ipm_problem_create returns IPM_NOT_SUPPORTED unless the problem is an LP
                                (not phase 1) with inequality rows (m > 0), equality rows (p > 0) and at
                                least one box bound.  ipm_fm_hessian returns IPM_NOT_SUPPORTED.  No Q9: a
                                failed factorization of K (non-finite data or a rank-deficient A) ends the
                                Newton solve with linalg_error = 1, use_backup stays 0.
                                use_psd_condition adds 1e-9 to D only.  Numerics: DESIGN.md §11.2 */
#define IPM_SOLVE_CHOLESKY_DUAL_QP 9 /* extension: the dual form of the QP Newton step for a FACTORED
                                P = diag(Pdiag) + Pf^T Pf (Pdiag >= 0, n entries, NULL = 0; Pf kf x n
                                row-major, NULL / kf = 0 = absent); desc.P must be NULL and P is never
                                formed.  With w = 1/(s_C + 1e-15)^2, D = t Pdiag + 1/s_lb^2 + 1/s_ub^2,
                                E = 1/D, M = [C; Pf] (rows stacked, never copied) and W = [w; t 1_kf]
                                  H = diag(D) + M^T diag(W) M,
                                  K = diag(1/W) + M diag(E) M^T     (order m + kf, positive definite),
                                  z = K^-1 M (E o -g),   dx = E o (-g - M^T z),
                                by a bordered Cholesky of K, followed by the refinement rounds of method 6
                                on the residual -g - H dx (H applied through M, never formed).  The
                                objective is 1/2 x.Px + q.x with Px = Pdiag o x + Pf^T (Pf x).  No n x n
                                array is allocated.  ipm_problem_create returns IPM_NOT_SUPPORTED unless
                                the problem is a QP (not phase 1) without equality rows, with P NULL,
                                m + kf > 0 and a positive diagonal: a box bound, or Pdiag given (the caller
                                then answers for Pdiag > 0 everywhere).  ipm_fm_hessian returns
                                IPM_NOT_SUPPORTED.  No Q9: a failed factorization of K (non-finite data)
                                ends the Newton solve with linalg_error = 1, use_backup stays 0.
                                use_psd_condition adds 1e-9 to D only.  Numerics: DESIGN.md §11.3 */
#define IPM_SOLVE_CHOLESKY_DUAL_QP_EQ 10 /* extension: method 9's factored P WITH equality rows (infeasible
                                start): H dx + A^T nu = -g, A dx = -(A x - b), dv = nu - v with
                                H = diag(D) + Mc^T diag(W) Mc, Mc = [C; Pf], W = [w; t 1_kf], D and E as for
                                method 9.  With M = [C; Pf; A] (rows stacked, never copied), y = [z; nu],
                                z = W o (Mc dx) the step solves ONE symmetric system of order m + kf + p,
                                  K = diag([1/W; 0_p]) + M diag(E) M^T,
                                  K y = [Mc (E o -g); A (E o -g) + (A x - b)],   dx = E o (-g - M^T y),
                                by a bordered Cholesky of K (positive definite when A has full row rank),
                                followed by method 8's refinement rounds on the residual of the full KKT
                                system (H applied through Mc, never formed; with the weight tail
                                [w; t 1_kf; 1_p] the product Mc^T (W o Mc dx) + A^T nu is one transposed
                                product over M).  No n x n and no n x p array is allocated, and desc.AT is
                                not read (it may be NULL).  ipm_problem_create returns IPM_NOT_SUPPORTED
                                unless the problem is a QP (not phase 1) with P NULL, equality rows (p > 0,
                                A and b), m + kf > 0 and a positive diagonal: a box bound, or Pdiag given.
                                ipm_fm_hessian returns IPM_NOT_SUPPORTED.  No Q9: a failed factorization of
                                K (non-finite data or a rank-deficient A) ends the Newton solve with
                                linalg_error = 1, use_backup stays 0.  use_psd_condition adds 1e-9 to D
                                only.  DESIGN.md §11.4 */

typedef struct ipm_handle ipm_handle;
typedef struct ipm_problem ipm_problem;

/*
 * Problem description.  Mirrors the data the reference's FunctionManager*
 * constructors receive (FunctionManager.py:13-90, 359-425, 619-680, 834-931,
 * 1165-1256).  Absent items are NULL.  Scalar bounds are expanded to n-vectors
 * by the caller.
 */
typedef struct ipm_problem_desc {
  int32_t kind;          /* IPM_KIND_*                                           */
  int32_t phase1;        /* 1: the phase-1 barrier (FunctionManagerPhase1 /      */
                         /*    FunctionManagerSOCPPhase1); variables (x, s)      */
  int32_t solve_method;  /* IPM_SOLVE_*                                          */
  int32_t reserved0;
  int64_t n;             /* number of x variables (without the phase-1 s)        */
  /* objective */
  const double* c;       /* [dev] n      LP cost (FunctionManager.py:76-90)       */
  const double* P;       /* [dev] n x n  QP/SOCP quadratic term, row-major        */
  int64_t ldp;
  const double* q;       /* [dev] n      QP/SOCP linear term                      */
  /* linear inequalities C x <= d (LP, QP, LP phase 1) */
  int64_t m;
  const double* C;       /* [dev] m x n  row-major                                */
  int64_t ldc;
  const double* d;       /* [dev] m                                               */
  /* box bounds */
  const double* lb;      /* [dev] n                                               */
  const double* ub;      /* [dev] n                                               */
  /* equality constraints A x = b -> infeasible-start Newton
     (NewtonSolverInfeasibleStart.py; SOCPSolver passes F, g here)               */
  int64_t p;
  const double* A;       /* [dev] p x n  row-major                                */
  int64_t lda;
  const double* AT;      /* [dev] n x p  row-major copy of A^T (static, once);    */
                         /*    IPM_SOLVE_CHOLESKY_DUAL_EQ never reads it: NULL ok */
                         /*    (nor does IPM_SOLVE_CHOLESKY_DUAL_QP_EQ)            */
  const double* b;       /* [dev] p                                               */
  /* second-order cones (FunctionManagerSOCP): ||A_i x + b_i|| <= c_i.x + d_i    */
  int64_t K;             /* number of cones                                       */
  int64_t R;             /* total rows of the dense cones                         */
  double* X;             /* [dev] (R + 2K) x n row-major, ldx: rows [0,R) stacked */
                         /*   dense A_i, rows [R,R+K) the c_i, rows [R+K,R+2K)    */
                         /*   scratch for the per-cone gradient rows g_i          */
  int64_t ldx;
  const int64_t* cone_row_off; /* [dev] K+1: rows of cone i are [off[i],off[i+1]); */
                               /*   a diagonal cone has off[i]==off[i+1]           */
  const int64_t* cone_row_off_host; /* host copy of the above                     */
  const double* cone_b;  /* [dev] R: b_i stacked for the dense rows (NULL: no b)   */
  const double* cone_d;  /* [dev] K: d_i (NULL: no d)                              */
  int32_t has_cone_c;    /* 0: no c_i (rhs_i = d_i)                                */
  int32_t reserved1;
  int64_t Kd;            /* number of diagonal cones (A_i = diag(a_i), SOCPSolver.py:285-292) */
  const double* Ad;      /* [dev] Kd x n  a_i                                       */
  const double* bd;      /* [dev] Kd x n  b_i (NULL: no b)                          */
  const int64_t* dcone_id; /* [dev] Kd: cone index of each diagonal cone            */
  const int64_t* dcone_id_host;
  /* factored quadratic term P = diag(Pdiag) + Pf^T Pf (IPM_SOLVE_CHOLESKY_DUAL_QP / _QP_EQ only; appended: a
     descriptor that leaves them zero / NULL means what it meant before they existed)          */
  const double* Pf;      /* [dev] kf x n row-major factor rows (NULL: none)               */
  int64_t ldpf;
  int64_t kf;            /* number of factor rows (0: none)                               */
  const double* Pdiag;   /* [dev] n      diagonal part, >= 0 (NULL: zero)                 */
} ipm_problem_desc;

/* Newton options: NewtonSolver.__init__ (NewtonSolver.py:16-78) */
typedef struct ipm_newton_opts {
  int32_t max_iters;
  int32_t update_slacks_every;   /* Q2 */
  int32_t phase1_flag;           /* early exit x[-1] < -phase1_tol (NewtonSolver.py:105-107) */
  int32_t use_psd_condition;     /* +1e-9 on diag before Cholesky (NewtonSolver.py:269-275) */
  double eps;                    /* inner epsilon */
  double alpha, beta;            /* backtracking parameters */
  double phase1_tol;
  double* trace;                 /* optional HOST buffer: per-iteration (step, stat) pairs  */
  int32_t trace_cap;             /* capacity in iterations (0: no trace)                   */
  int32_t linesearch_mode;       /* IPM_LS_* (feasible start)                                */
} ipm_newton_opts;

/* feasible-start backtracking (NewtonSolver.py:157-206) */
#define IPM_LS_TABLE 0   /* 64 candidate steps per pass: slacks s0 + a ds, f(x + a dx) by its
                            expansion; the reference's decision sequence replayed on the host   */
#define IPM_LS_EXACT 1   /* reference-exact: every trial point formed, fresh d - C next_x slacks
                            when the reference refreshes them, f(next_x) evaluated directly      */
#define IPM_LS_COMPARE 2 /* both; the exact step is taken, disagreements counted (ls_flips)     */

/* Result of one centering step: the tuple NewtonSolver.solve returns */
typedef struct ipm_newton_result {
  int32_t iters;        /* Newton iterations taken                               */
  int32_t success;      /* success flag                                          */
  int32_t stat_valid;   /* 0: the reference would return None                    */
  int32_t use_backup;   /* Cholesky fallback engaged (persists, Q9)              */
  double stat;          /* nd = -g.dx/2 (feasible) or trial residual (infeasible)*/
  double last_step;     /* last accepted step size                               */
  int64_t backtracks;   /* total trial points examined                           */
  int64_t ls_compared;  /* IPM_LS_COMPARE: steps compared / steps whose table and  */
  int64_t ls_flips;     /*   exact step sizes differ                             */
  int64_t linalg_error; /* the solve ended on a LinAlgError: a least-squares      */
                        /*   eigensolve did not converge (the reference's try /   */
                        /*   except in NewtonSolver.py:148-155 returns a failure)  */
                        /*   IPM_SOLVE_CHOLESKY_DUAL: the Cholesky of S failed    */
                        /*   IPM_SOLVE_CHOLESKY_DUAL_EQ: the Cholesky of K failed */
                        /*   IPM_SOLVE_CHOLESKY_DUAL_QP: the Cholesky of K failed */
                        /*   IPM_SOLVE_CHOLESKY_DUAL_QP_EQ: the same              */
} ipm_newton_result;

/* ---- handle --------------------------------------------------------------- */
/* one handle per (process, device, stream); stream = hipStream_t, NULL = legacy default stream */
int ipm_create(int device, void* stream, ipm_handle** out);
int ipm_destroy(ipm_handle* h);
const char* ipm_last_error(ipm_handle* h);
int ipm_version(void);

/* ---- level 2: the Newton inner loop (the hot path) ------------------------- */
/* bytes of device workspace the problem needs */
int64_t ipm_workspace_bytes(const ipm_problem_desc* desc);
int ipm_problem_create(ipm_handle* h, const ipm_problem_desc* desc, void* workspace /*[dev]*/,
                       int64_t workspace_bytes, ipm_problem** out);
int ipm_problem_destroy(ipm_problem* pr);
/* NewtonSolver.solve / NewtonSolverInfeasibleStart.solve: x [dev] (N = n(+1)) is
   updated in place (Q8); v [dev] (p) likewise; t is the barrier parameter. */
int ipm_newton_solve(ipm_problem* pr, double* x, double t, double* v, const ipm_newton_opts* opts,
                     ipm_newton_result* res);
/* persistent Cholesky-failure flag (Q9) */
int ipm_get_use_backup(ipm_problem* pr);
int ipm_set_use_backup(ipm_problem* pr, int flag);
/* IPM_SOLVE_CG: the iteration cap (max_cg_iters, default 50) and relative tolerance (scipy's rtol,
   default 1e-5) of every CG solve of this problem from now on; a negative value: IPM_INVALID_ARG.
   (A setter, not a field: the option and result structs keep their sizes.) */
int ipm_set_cg(ipm_problem* pr, int32_t max_cg_iters, double rtol);
/* out[0] CG solves since creation, out[1] their CG iterations in total, out[2] / out[3] the last
   solve's iterations and info (0: ||r|| < rtol ||b|| reached; max_cg_iters: the cap truncated it,
   as scipy reports).  The device words travel with the Newton step's one read-back. */
int ipm_get_cg_stats(ipm_problem* pr, int64_t out[4]);
/* IPM_SOLVE_CG: the preconditioner of every CG solve of this problem from now on.  JACOBI:
   M = 1 / diag(H), taken from the assembled Hessian at every Newton step (scipy's cg(..., M=M):
   the convergence test stays on r).  Any other kind: IPM_INVALID_ARG.  Accepted on any problem;
   only IPM_SOLVE_CG reads it.  Default NONE.  A zero, negative or NaN diagonal entry is not
   special-cased: 1 / h propagates, the solve reports info = max_cg_iters. */
#define IPM_CG_PRECOND_NONE 0
#define IPM_CG_PRECOND_JACOBI 1
int ipm_set_cg_precond(ipm_problem* pr, int32_t kind);
int ipm_get_cg_precond(ipm_problem* pr);

/* ---- level 1: the oracle protocol (FunctionManager.py:94-195) ---------------- */
/* update_x(x, update_slacks): the evaluation point becomes x [dev]; slacks are
   recomputed only if update_slacks (Q2) */
int ipm_fm_update_x(ipm_problem* pr, const double* x, int update_slacks);
/* slacks [dev out] (FunctionManager.slacks) */
int ipm_fm_slacks(ipm_problem* pr, double* out);
int64_t ipm_fm_num_slacks(ipm_problem* pr);
/* objective(): f(x) at the evaluation point (host scalar) */
int ipm_fm_objective(ipm_problem* pr, double* out);
/* newton_objective(): t f(x) - sum log(s + eps) with the CURRENT (maybe stale) slacks */
int ipm_fm_newton_objective(ipm_problem* pr, double t, double* out);
/* gradient() [dev out, N] */
int ipm_fm_gradient(ipm_problem* pr, double t, double* g);
/* hessian() [dev out]: dense N x N row-major full matrix (both triangles), or for
   IPM_SOLVE_DIAGONAL the diagonal vector (N) */
int ipm_fm_hessian(ipm_problem* pr, double t, double* H, int64_t ldh);

/* the Newton direction dx [dev out, N] of the last step ipm_newton_solve took on this problem, as the
   linear solve left it (before the step size is applied): tests compare it with a reference */
int ipm_fm_last_direction(ipm_problem* pr, double* out);
/* its sibling for a problem with equality rows: the dual direction dv [dev out, p] of the last step
   (v + dv is the multiplier nu of the Newton system).  No equality rows: IPM_INVALID_ARG */
int ipm_fm_last_dual_direction(ipm_problem* pr, double* out);

/* ---- level 0: dense fp64 kernels (exposed for tests and benches) -------------- */
/* y = alpha * op(M) x + beta * y ; M row-major rows x cols */
int ipm_gemv(ipm_handle* h, int trans, int64_t rows, int64_t cols, double alpha, const double* M,
             int64_t ldm, const double* x, double beta, double* y);
/* TWO vectors over ONE matrix: Y[:, j] = op(M) X[:, j] for j = 0, 1, with M (row-major rows x cols,
   ldm >= cols) read once.  X and Y are column-major: vector j starts at X + j * ldx (cols entries;
   trans: rows) and Y + j * ldy (rows entries; trans: cols).  Each output column is bit for bit what
   ipm_gemv(alpha 1, beta 0) gives for that vector alone (same loads, same summation order; vectors of
   different 16-byte alignment take two single-vector launches).  rows == 0 or cols == 0: as ipm_gemv.
   IPM_INVALID_ARG: ldm < cols, ldx (ldy) below the input (output) vector length, or a null M, X or Y
   that would be read or written.
   (The engine's gemv_n2 is the other thing: two matrices, one vector.) */
int ipm_gemv_2v(ipm_handle* h, int trans, int64_t rows, int64_t cols, const double* M, int64_t ldm,
                const double* X, int64_t ldx, double* Y, int64_t ldy);
/* TWO matrices stacked, transposed: y = alpha [M0; M1]^T (w o x) + beta y with M0 (m0 x cols, ld0) over M1
   (m1 x cols, ld1), both row-major, neither copied; x and w (NULL: all ones) have m0 + m1 entries, y has cols.
   Bit for bit ipm_gemv(trans) (with w folded into x) on a physically stacked copy: the same row chunks,
   partial sums and fold order; no atomics.  m0 == 0 or m1 == 0: the one-matrix product.  beta == 0: y is
   only written.  IPM_INVALID_ARG: a negative size, ld0 or ld1 < cols for an operand with rows, or a null
   M0, M1, x or y that would be read or written. */
int ipm_gemv_t2(ipm_handle* h, int64_t m0, int64_t m1, int64_t cols, double alpha, const double* M0, int64_t ld0,
                const double* M1, int64_t ld1, const double* x, const double* w, double beta, double* y);
/* THREE matrices stacked, transposed: y = alpha [M0; M1; M2]^T (w o x) + beta y; x and w (NULL: all ones) have
   m0 + m1 + m2 entries.  As ipm_gemv_t2: bit for bit ipm_gemv(trans) on a physically stacked copy (a row chunk
   may straddle either seam or both), no atomics.  An operand without rows is never read and needs neither a
   pointer nor a leading dimension: the call is then the two-matrix (or one-matrix) product of the others.
   IPM_INVALID_ARG as ipm_gemv_t2.  (M^T y of IPM_SOLVE_CHOLESKY_DUAL_QP_EQ: M0 = C, M1 = Pf, M2 = A.) */
int ipm_gemv_t3(ipm_handle* h, int64_t m0, int64_t m1, int64_t m2, int64_t cols, double alpha, const double* M0,
                int64_t ld0, const double* M1, int64_t ld1, const double* M2, int64_t ld2, const double* x,
                const double* w, double beta, double* y);
/* THREE matrices, one vector, one launch: y = [M0 x; M1 x; M2 x] (y has m0 + m1 + m2 entries, only written).
   Every entry is bit for bit what ipm_gemv(no trans, alpha 1, beta 0) gives for its row; operands of different
   16-byte alignment take separate launches.  An operand without rows is never read.  IPM_INVALID_ARG: a
   negative size, a leading dimension < cols for an operand with rows, or a null pointer that would be read or
   written. */
int ipm_gemv_n3(ipm_handle* h, int64_t m0, int64_t m1, int64_t m2, int64_t cols, const double* M0, int64_t ld0,
                const double* M1, int64_t ld1, const double* M2, int64_t ld2, const double* x, double* y);
/* H(lower, column-major ldh) = alpha * X^T diag(w) X + beta * H ; X row-major k x n.
   w may be NULL (all ones).  The SYRK of FunctionManager.py:301-306 / 801-805. */
int ipm_syrk(ipm_handle* h, int64_t n, int64_t k, const double* X, int64_t ldx, const double* w,
             double alpha, double beta, double* H, int64_t ldh);
/* lower triangle of H (column-major, ldh >= m) = X diag(w) X^T + diag(dvec); X row-major m x k
   (ldx >= k): the sum runs over the CONTIGUOUS index of X (ipm_syrk sums over its rows).  w [dev, k]
   and dvec [dev, m] may be NULL (all ones / no diagonal term).  H is overwritten, never read; its
   strict upper triangle and padding are not touched.  m == 0: IPM_OK without a launch; k == 0: dvec
   (or zeros) on the diagonal, zeros below.  K-split partial tiles (handle scratch) are added in a
   fixed order by a second launch (no atomics): bitwise repeatable.  The S assembly of
   IPM_SOLVE_CHOLESKY_DUAL. */
int ipm_syrk_nt(ipm_handle* h, int64_t m, int64_t k, const double* X, int64_t ldx, const double* w,
                const double* dvec, double* H, int64_t ldh);
/* the same product on the (m0 + m1) x k matrix whose first m0 rows are X0's (row-major, ldx0 >= k) and
   whose last m1 rows are X1's (ldx1 >= k); neither is copied.  Tiles, K split and summation order are
   those of ipm_syrk_nt on the physically stacked matrix: the result equals it bit for bit.  w [dev, k],
   dvec [dev, m0 + m1] may be NULL; ldh >= m0 + m1.  m1 == 0 behaves as ipm_syrk_nt(m0, X0); m0 == 0 never
   reads X0.  The K assembly of IPM_SOLVE_CHOLESKY_DUAL_EQ (X0 = C, X1 = A). */
int ipm_syrk_nt2(ipm_handle* h, int64_t m0, int64_t m1, int64_t k, const double* X0, int64_t ldx0,
                 const double* X1, int64_t ldx1, const double* w, const double* dvec, double* H, int64_t ldh);
/* ... and on the (m0 + m1 + m2) x k matrix of three row blocks X0, X1, X2 (each row-major with its own leading
   dimension >= k), none copied: bit for bit ipm_syrk_nt on the physically stacked matrix; a 64-row tile may
   straddle either seam or both.  dvec [dev, m0 + m1 + m2] may be NULL; ldh >= m0 + m1 + m2.  A block without
   rows is never read: m2 == 0 behaves as ipm_syrk_nt2(m0, m1), m1 == m2 == 0 as ipm_syrk_nt(m0).  The K assembly
   of IPM_SOLVE_CHOLESKY_DUAL_QP_EQ (X0 = C, X1 = Pf, X2 = A). */
int ipm_syrk_nt3(ipm_handle* h, int64_t m0, int64_t m1, int64_t m2, int64_t k, const double* X0, int64_t ldx0,
                 const double* X1, int64_t ldx1, const double* X2, int64_t ldx2, const double* w, const double* dvec,
                 double* H, int64_t ldh);
/* in-place Cholesky of the lower triangle of H (column-major, ldh); *info as LAPACK
   potrf (0 ok, j>0: leading minor j not positive definite).  work: [dev] >= 64 bytes */
int ipm_potrf(ipm_handle* h, int64_t n, double* H, int64_t ldh, int* info);
/* the first ncols columns only (0 <= ncols <= n): L11 = chol(H11) and L21 = H21 L11^-T, the
   rows below ncols untouched otherwise.  The Newton step factors [[H, -g], [-g^T, .]] this way
   with ncols = N, so row N becomes L^-1 (-g): the forward substitution of cho_solve
   (NewtonSolver.py:303-313) rides inside the factorisation */
int ipm_potrf_partial(ipm_handle* h, int64_t n, int64_t ncols, double* H, int64_t ldh, int* info);
/* solve L L^T X = B in place; L lower column-major (ldl); B row-major n x nrhs (ldb) */
int ipm_potrs(ipm_handle* h, int64_t n, int64_t nrhs, const double* L, int64_t ldl, double* B,
              int64_t ldb);
/* LU with partial pivoting, in place (column-major, lda): the np.linalg.solve / Cholesky-fallback
   factorisation (NewtonSolver.py:230-247, 334-341; NewtonSolverInfeasibleStart.py:513-538).  Blocked:
   64-column panels, MFMA trailing update.  piv [dev] n: row swapped with k, or -1-k for an exactly
   zero pivot column (skipped; ipm_getrs gives that component 0).  A NaN entry is never taken for a
   zero: a column with a NaN among its candidates gets a NaN pivot and the factors are NaN from
   there on, so ipm_getrs returns a non-finite vector for a NaN matrix, as np.linalg.solve does */
int ipm_getrf(ipm_handle* h, int64_t n, double* A, int64_t lda, int64_t* piv, int* info);
/* solve with the ipm_getrf factors; B row-major n x nrhs (ldb), in place */
int ipm_getrs(ipm_handle* h, int64_t n, int64_t nrhs, const double* LU, int64_t lda, const int64_t* piv,
              double* B, int64_t ldb);
/* minimum-norm least squares on a symmetric matrix: B <- A^+ B, the np.linalg.lstsq(A, B, rcond=None)
   of the np_lstsq method and of the Cholesky-failure backup (NewtonSolver.py:212-227, 334-341;
   NewtonSolverInfeasibleStart.py:279-316, 692-724).  A full symmetric (column-major, lda), replaced
   by W = V^T, the TRANSPOSED eigenvector matrix (column-major, lda: column j of A holds row j of V,
   i.e. A(i, j) = V(j, i), the operand layout of the MFMA apply); eigenvalues
   |lambda| <= eps * n * max|lambda| are dropped (gelsd's rcond rule).  B row-major n x nrhs (ldb), in place.  *info: the eigensolver's convergence info (0 = ok,
   1 = the hand-written Jacobi eigensolver did not converge, or A holds a NaN or Inf entry (its
   squared Frobenius norm is not finite) -- np.linalg.lstsq raises LinAlgError on both) */
int ipm_lstsq_sym(ipm_handle* h, int64_t n, int64_t nrhs, double* A, int64_t lda, double* B, int64_t ldb,
                  int* info);
/* y = alpha * H x + beta * y, H symmetric: only its lower triangle (column-major, any ldh >= n) is
   read, each 128 x 128 tile once for both of its output blocks.  Per-tile partials in the handle's
   scratch are added in a fixed order by a second launch (no atomics): bitwise repeatable.
   beta == 0 does not read y. */
int ipm_symv(ipm_handle* h, int64_t n, double alpha, const double* H, int64_t ldh, const double* x, double beta,
             double* y);
/* conjugate gradients on H x = b with scipy.sparse.linalg.cg's semantics (atol = 0, no
   preconditioner; ipm_pcg takes one): x [dev] holds x0 on entry and the iterate on return; b == 0 gives x = 0.
   *iters: iterations done; *info: 0 (||r|| < rtol ||b|| seen at the head of an iteration) or
   maxiter.  3 launches per iteration for maxiter iterations, each returning at once after the
   device `done` word is set; no host synchronisation before the single one that returns iters / info. */
int ipm_cg(ipm_handle* h, int64_t n, const double* H, int64_t ldh, const double* b, double* x /* in: x0, out */,
           int32_t maxiter, double rtol, int32_t* iters, int32_t* info);
/* ipm_cg with a diagonal preconditioner M = diag(minv) (scipy's cg(..., M=M)): minv [dev, n];
   minv == NULL means 1 / diag(H), computed into the handle's scratch.  The convergence test is on
   r, rho = r.(M r).  Same conventions, argument checks and launch sequence as ipm_cg (one more
   launch in the prologue when minv == NULL). */
int ipm_pcg(ipm_handle* h, int64_t n, const double* H, int64_t ldh, const double* minv, const double* b,
            double* x /* in: x0, out */, int32_t maxiter, double rtol, int32_t* iters, int32_t* info);
/* HIP-event timing of the KKT assembly and of the Cholesky factorisation inside
   ipm_newton_solve (enable/reset with ipm_set_timing; adds no synchronisation):
   averages (ms) over the Newton iterations since the reset, and their count */
int ipm_set_timing(ipm_handle* h, int on);
int ipm_last_timings(ipm_handle* h, double* kkt_ms, double* potrf_ms, double* count);
/* debug knob: the wall-clock bound (microseconds, s_memrealtime) after which the persistent
   backward solve's chain step stops waiting for its producer and raises its device error word; the
   Newton step's readback then returns IPM_HIP_ERROR instead of using the step.  0 restores the
   default 1 s.  Process-wide; tests use a tiny bound to trip the error path once. */
int ipm_debug_set_trsv_spin_limit(unsigned limit);
/* debug knob: the same wall-clock bound (microseconds; 0 = default 1 s) for every wait of the
   ticketed Cholesky (k_potrf_block: row chunks on their diagonal role, look-ahead / fold / split
   hand-offs).  A wait that runs out sets info to -1000
   (IPM_INFO_SPIN: never a LAPACK column), every later launch of the factorization returns at once,
   and ipm_potrf / the Newton step return IPM_HIP_ERROR.  Process-wide. */
int ipm_debug_set_potrf_spin_limit(unsigned microseconds);
/* debug knob: the k-th least-squares eigensolve from now (k = 0: the next one) reports
   non-convergence whatever happened (-1: off).  Tests that one failed eigensolve among several in
   a Newton step is not overwritten by a later converged one. */
int ipm_debug_lstsq_fail_call(int k);
/* debug knob: the backward-solve workgroup holding chain ticket `ticket` sleeps ~7 ms before
   publishing its progress word (-1: off), so later tickets overtake it -- exercises the monotonic
   progress publish.  ticket <= -2: ticket -2 - ticket sleeps before storing its x block instead,
   so the next ticket's bounded poll of that block runs out (exercises the loud failure).
   Process-wide. */
int ipm_debug_set_trsv_publish_delay(int ticket);
/* KKT-SYRK flops of one Newton step of this problem (m n (n+1) in total): all of them run in the
   SYRK kernel (*upfront); *deferred is always 0 (the round-2 deferred-slice experiment was
   removed; the argument is kept so existing bindings need no change) */
int ipm_kkt_flops(ipm_problem* pr, double* upfront, double* deferred);
/* measurement: HIP-event time (ms, averaged over `reps`, on the handle's stream) of the HBM-bound
   kernels of one Newton step on this problem's buffers -- ms[0] the slack GEMV C x, ms[1] the
   gradient GEMV C^T w, ms[2] one 64-candidate line-search pass over the S slacks.  Clobbers only
   scratch.  LP/QP problems with inequality rows (bench.py reports them as GB/s). */
int ipm_time_hbm_kernels(ipm_problem* pr, int reps, double* ms);
/* out[0..2] = m (inequality rows), n, S (slacks incl. box bounds) */
int ipm_problem_sizes(ipm_problem* pr, int64_t* out);

/* ---- batched ADMM Lasso (LassoSolver.py) ------------------------------ *
 * S problems  min_x 1/(2m) ||A x - b_s||^2 + reg_s ||x||_1  solved together.  Every n x S matrix
 * below is row-major with leading dimension lds (element (i, s) at i*lds + s).                  */
typedef struct ipm_lasso_args {
  int64_t n, S, m;         /* variables (incl. the bias column), problems, rows of A           */
  int64_t lds;             /* leading dimension of x, alpha, u, W0, W1                         */
  const double* Qs;        /* [dev] n x n, ldq: (-m rho Q)^T, Q = (diag(m rho) + A^T A)^-1      */
  int64_t ldq;
  const double* bA;        /* [dev] n x (S or 1), ldba: Q A^T b (LassoSolver.py:214-219)         */
  int64_t ldba;
  const double* eta;       /* [dev] S or 1: reg / rho                                         */
  double* x;               /* [dev] state (zeros on entry, LassoSolver.py:222-236)             */
  double* alpha;
  double* u;
  double* W0;              /* [dev] u - alpha on entry; W1 scratch (ping-pong)                 */
  double* W1;
  double* partial;         /* [dev] >= ipm_lasso_partial_doubles(n, S), zeroed once before use  */
  double rho, eps_abs, eps_rel, stop_multiplier;
  int32_t max_iters, check_stop;
  int32_t positive, add_bias;
  int32_t dual_form;       /* 0: u = u + x - alpha (:251); 1: u = u + (x - alpha) (chunks, :413) */
  int32_t compute_loss;    /* per-iteration loss into gaps (LassoSolver.py:254-268)            */
  int32_t ba_bcast, eta_bcast, b_bcast, reg_bcast;   /* 1: a single column / value for all S   */
  /* loss evaluation (compute_loss, ipm_lasso_loss) */
  const double* AT;        /* [dev] n x m, ldat: A^T row-major                                 */
  int64_t ldat;
  const double* b;         /* [dev] m x (S or 1), ldb                                          */
  int64_t ldb;
  const double* reg;       /* [dev] S or 1                                                    */
  double* R;               /* [dev] m x S scratch                                             */
  double* gaps;            /* [dev] max_iters rows of ldg: gaps[it*ldg + col(s)]               */
  int64_t ldg;
  const int64_t* gap_cols; /* [dev] S: column of problem s in gaps (chunks), NULL: s            */
  int32_t qs_blocked;      /* 1: Qs is the tile-blocked copy of ipm_lasso_block_qs (ldq unused)  */
} ipm_lasso_args;

/* row-major C (M x N, ldc) = alpha A^T B + beta C; A: K x M (lda), B: K x N (ldb); fp64 MFMA */
int ipm_gemm_tn(ipm_handle* h, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda,
                const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
/* out (cols x rows, ldo) = in^T (rows x cols, ldi), row-major; device copy of n doubles */
int ipm_transpose(ipm_handle* h, int64_t rows, int64_t cols, const double* in, int64_t ldi, double* out,
                  int64_t ldo);
int ipm_copy(ipm_handle* h, double* dst, const double* src, int64_t n);
/* normalize_A (LassoSolver.py:122-123): A /= A.std(axis=0) in place; stdv [dev] n (may be NULL) */
int ipm_lasso_colnorm(ipm_handle* h, int64_t m, int64_t n, double* A, int64_t lda, double* stdv);
/* add_bias (LassoSolver.py:124-131): out (m x (n+1), ldo) = [1 | A] */
int ipm_lasso_bias(ipm_handle* h, int64_t m, int64_t n, const double* A, int64_t lda, double* out, int64_t ldo);
/* LassoSolver.py:157-189: Q = (diag(m rho) + A^T A)^-1 via Cholesky (info as ipm_potrf), QT = Q^T */
int ipm_lasso_qinv(ipm_handle* h, int64_t m, int64_t n, const double* A, int64_t lda, double rho, double* Q,
                   double* QT, int64_t ldq, int* info);
/* M (rows x cols, ld) *= f1 (then *= f2 when two): Qinv *= -m*rho, or Qinv * -m * rho (chunks) */
int ipm_lasso_scale(ipm_handle* h, int64_t rows, int64_t cols, double* M, int64_t ld, double f1, double f2,
                    int two);
/* prox (LassoSolver.py:533-558): out = soft-threshold(v, eta), row 0 kept with add_bias */
int ipm_lasso_prox(ipm_handle* h, int64_t n, int64_t S, const double* v, int64_t ldv, const double* eta,
                   int eta_bcast, int positive, int add_bias, double* out, int64_t ldo);
/* loss per problem of the current alpha into out[cols ? cols[s] : s]; absm: |alpha| in the l1 term */
int ipm_lasso_loss(ipm_handle* h, const ipm_lasso_args* a, int absm, double* out, const int64_t* cols);
int64_t ipm_lasso_partial_doubles(int64_t n, int64_t S);
/* Qs (n x n, ldq, k-major) -> Qb in the ADMM step's tile-blocked layout: 32-row tiles of i, each
   tile's k rows contiguous (element (i, k) at ((i / 32) * n + k) * 32 + i % 32, rows >= n zero), so
   that each workgroup of the iteration GEMM streams one contiguous span instead of 256-byte pieces
   of every k row.  Qb holds ipm_lasso_qb_doubles(n) doubles. */
int64_t ipm_lasso_qb_doubles(int64_t n);
int ipm_lasso_block_qs(ipm_handle* h, int64_t n, const double* Qs, int64_t ldq, double* Qb);
/* the ADMM loop (LassoSolver.py:240-337, one chunk of :339-485): iterates until the stopping
   test (every check_stop iterations) or max_iters; *iters = the last iteration index */
int ipm_lasso_admm(ipm_handle* h, const ipm_lasso_args* a, int32_t* iters);

#ifdef __cplusplus
}
#endif
#endif /* IPM355_H */
