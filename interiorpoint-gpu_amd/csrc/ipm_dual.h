// The dual-form LP Newton steps (ipm_dual.hip): H = diag(D) + C^T diag(w) C is never
// formed, the step comes from the factorization of a matrix of the order of the constraint rows.  Each
// routine writes the direction the linear solve leaves (pr->dx, and pr->dv with equality rows) and the
// factorization's info word; `add` is the psd add on D (1e-9 with use_psd_condition, else 0).  A failed
// factorization has no fallback: ipm_newton_solve ends the solve with linalg_error.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct ipm_problem;

namespace ipm {

// IPM_SOLVE_CHOLESKY_DUAL: S = diag(1 / w) + C diag(E) C^T of order m, feasible start
void dual_direction(ipm_problem* pr, double add);
// IPM_SOLVE_CHOLESKY_DUAL_PHASE1: the same S, the phase-1 variable s as one bordering column (add on hss too);
// info word RB_INFO_DUAL1 is set unless the Schur complement sigma is finite and positive
void dual_direction_phase1(ipm_problem* pr, double add);
// IPM_SOLVE_CHOLESKY_DUAL_EQ: K = diag([1 / w; 0]) + [C; A] diag(E) [C; A]^T of order m + p, infeasible start
// from the dual v; expects pr->Axb = A x - b
void dual_direction_eq(ipm_problem* pr, const double* v, double add);
// IPM_SOLVE_CHOLESKY_DUAL_QP: K = diag([1 / w; 1 / t]) + [C; Pf] diag(E) [C; Pf]^T of order m + kf for the
// factored P = diag(Pdiag) + Pf^T Pf at barrier parameter t, feasible start
void dual_direction_qp(ipm_problem* pr, double add, double t);
// IPM_SOLVE_CHOLESKY_DUAL_QP_EQ: K = diag([1 / w; 1 / t; 0]) + [C; Pf; A] diag(E) [C; Pf; A]^T of order m + kf + p
// for the factored P with equality rows, infeasible start from the dual v; expects pr->Axb = A x - b
void dual_direction_qp_eq(ipm_problem* pr, const double* v, double add, double t);
// out = Pdiag o x + ftfx (either may be null: that term is absent): the last step of P x through its factors
void pfactor_combine(hipStream_t st, int64_t n, const double* pdiag, const double* x, const double* ftfx, double* out);

// partial sums of h.dx the phase-1 residual launch leaves (one per 256-entry block): the workspace's d1part
inline int64_t dual_ph1_blocks(int64_t n) { return (n + 255) / 256; }

}  // namespace ipm
