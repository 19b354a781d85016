// The Newton engine's problem object (include/ipm355.h: ipm_problem), shared by the translation units that
// take Newton steps on it (ipm_engine.hip: oracle protocol, workspace, Newton loop and the primal directions;
// ipm_dual.hip: the dual-form directions), with the layout of the per-iteration readback block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/ipm355.h"
#include "ipm_barrier.h"
#include "ipm_handle.h"

constexpr int NCAND = 64;
// IPM_SOLVE_CHOLESKY_DUAL: rounds of iterative refinement on the primal residual -g - H dx, each
// solved through the factored S again (without them the step's error along the
// nearly active rows leaves lam* = 1 / (t s) of lp_ineq_box at 4.4e-4 from the reference's; one
// round: 2.5e-6, two: 6.9e-7, three: 1.1e-9, four: 3.7e-10 -- the primal Cholesky's level)
constexpr int DUAL_REFINE = 3;
// readback block layout (bytes): info (8 ints), mask (4 words), sums (NCAND), scal (64)
constexpr int RB_MASK = 32, RB_SUMS = 64, RB_SCAL = RB_SUMS + NCAND * 8;
constexpr int RB_INFO_TRSV_ERR = 4;   // info word 4: sticky device error word of the backward solve
constexpr int RB_INFO_LSQ = 5;        // info word 5: non-convergence of the least-squares eigensolver
constexpr int RB_INFO_CG = 6;         // info words 6, 7: the CG solve's iteration count and info
constexpr int RB_INFO_DUAL1 = 2;      // info word 2: the dual phase-1 step's sigma was not finite and positive

enum Slot {
  SC_F0A = 0,  // c.x | x.Px | s
  SC_F0B,      // q.x
  SC_DFA,      // c.dx | x.Pdx | ds
  SC_DFB,      // q.dx
  SC_DDF,      // dx.Pdx
  SC_GX,       // g.x
  SC_GDX,      // g.dx
  SC_SUMLOG0,  // sum log(s0 + eps) over the barrier segment
  SC_SUMINV,   // phase 1: sum inv
  SC_SUMINV2,  // phase 1: sum inv^2
  SC_R0A,      // ||g + A^T v||^2
  SC_R0B,      // ||Ax - b||^2
  SC_XN,       // x[n]   (phase 1)
  SC_DXN,      // dx[n]  (phase 1)
  SC_COUNT
};

struct ipm_problem {
  ipm_handle* h = nullptr;
  ipm_problem_desc d{};
  // dims / flags
  int64_t n = 0, N = 0, S = 0, Sbar = 0, nub = 0, nlb = 0, m = 0, p = 0, K = 0, R = 0, XR = 0, Lh = 0;
  int64_t ldh = 0, nbb = 0;  // ld of H, bound-segment length (SOCP)
  bool lp = false, qp = false, socp = false, ph1 = false, eq = false, diag = false, lu = false, lsq = false,
       cg = false, dual = false, dual1 = false, dualeq = false, dualqp = false, dualqe = false;
  ipm::SocpView sv{};
  // workspace carve
  double *xe = nullptr, *s0 = nullptr, *ds = nullptr, *inv = nullptr, *w = nullptr, *dvec = nullptr;
  double *g = nullptr, *go = nullptr, *gb = nullptr, *ct = nullptr, *Px = nullptr, *Pdx = nullptr;
  double *Cx = nullptr, *Cdx = nullptr, *dx = nullptr, *H = nullptr, *W2 = nullptr, *hxs = nullptr;
  double *scal = nullptr, *lhs0 = nullptr, *rhs0 = nullptr, *dlhs = nullptr, *drhs = nullptr;
  double *coef = nullptr, *ones = nullptr, *psum = nullptr, *sums = nullptr, *xd = nullptr;
  double *Ybuf = nullptr, *Sbuf = nullptr, *Wp = nullptr, *ATv = nullptr, *ATdv = nullptr, *Axb = nullptr;
  double *Adx = nullptr, *wv = nullptr, *r2 = nullptr, *tmpn = nullptr, *part = nullptr, *hdiag = nullptr;
  double *sdv = nullptr, *lhsd = nullptr, *rhsd = nullptr, *dv = nullptr, *tmpp = nullptr;
  unsigned long long *pmask = nullptr, *mask = nullptr;
  int64_t *piv = nullptr, *pivp = nullptr;
  int* info = nullptr;
  unsigned* ctl = nullptr;  // persistent-solve control words
  double* pws = nullptr;    // Cholesky panel workspace (inverted diagonal blocks)
  double* xinv = nullptr;   // backward solve: inverted 128 x 128 diagonal blocks of L
  int64_t part_elems = 0, nls_blocks = 0;
  std::vector<int64_t> rowcone_h, dslot_h;
  int64_t *rowcone_d = nullptr, *dslot_d = nullptr;
  bool use_backup = false;
  bool pieces_valid = false;  // barrier pieces (inv/coef/G) match the current slack state
  // w = inv^2 and dvec (with hess_add) were formed with the gradient (gradient_at's fused LP-family
  // path): assemble_hessian skips them while the slack state is unchanged
  bool hess_pre = false;
  double hess_add = 0.0;
  double* sws = nullptr;   // KKT SYRK split tail (syrk_split_ws_doubles)
  double* lsw = nullptr;   // least-squares workspace (lstsq_ws_doubles; null when the method never uses it)
  // linear_solve_method='cg' (IPM_SOLVE_CG): workspace (cg_ws_doubles), cap and tolerance (ipm_set_cg),
  // and the counters of ipm_get_cg_stats
  double* cgw = nullptr;
  // IPM_SOLVE_CHOLESKY_DUAL: S ((m + 1) x dlds, column-major, the bordered row included), E = 1 / dvec
  // (n), 1 / w (m), the border row r = C (E o -g) (m), z (m), C^T z (n), the S assembly's K-split tiles
  double *dS = nullptr, *dE = nullptr, *diw = nullptr, *dr = nullptr, *dz = nullptr, *dctz = nullptr;
  double* dsw = nullptr;
  double *drho = nullptr, *dtw = nullptr;   // refinement: the primal residual (n), the forward solve's scratch (m)
  // IPM_SOLVE_CHOLESKY_DUAL_PHASE1 (dual1; dual is set too: the set above, C^T z_u in dctz): y = Hxx^-1 h (n),
  // the second right-hand side E o h (n) and its C product / solution z_y (m), C^T z_y (n), the residual
  // launch's partial sums of h.dx, the device scalars (sigma, hss)
  double *d1y = nullptr, *d1ry = nullptr, *d1zy = nullptr, *d1cty = nullptr, *d1part = nullptr, *d1sc = nullptr;
  // IPM_SOLVE_CHOLESKY_DUAL_EQ (dualeq; dual is set too): the set above over M = [C; A] -- dS is K
  // ((m + p + 1) x dlds), diw = [1 / w; 0], dr / dz the stacked right-hand side and solution [z; nu] (m + p)
  // IPM_SOLVE_CHOLESKY_DUAL_QP (dualqp; dual is set too): the set above over M = [C; Pf] -- dS is K
  // ((m + kf + 1) x dlds), dr / dz the stacked right-hand side and solution (m + kf); w carries the stacked
  // weights [w; t 1_kf] (its tail refilled when t changes: dq_t), diw = 1 / that; dD = dvec + t Pdiag (n),
  // Fx = Pf x / Pf dx (kf) on the way to P x = Pdiag o x + Pf^T (Pf x)
  // IPM_SOLVE_CHOLESKY_DUAL_QP_EQ (dualqe; dualqp and dual are set too, dualeq is not): the factored QP's set over
  // M = [C; Pf; A] -- dS is K ((m + kf + p + 1) x dlds), dr / dz the stacked right-hand side and solution
  // [z; nu] (m + kf + p), w = [w; t 1_kf; 1_p] (the tail refilled when t changes), diw = [1 / W; 0_p] (the zero
  // tail written at create), dtw = [C dx; Pf dx; nu] in the refinement rounds
  double *dD = nullptr, *Fx = nullptr;
  int64_t kf = 0;
  double dq_t = -1.0;
  // dm: the order of the dual system (m; m + p with equality rows; m + kf factored QP; m + kf + p with both)
  int64_t dlds = 0, dm = 0;
  int32_t drefine = DUAL_REFINE;
  int32_t cg_max = 50;
  double cg_rtol = 1e-5;
  int32_t cg_precond = IPM_CG_PRECOND_NONE;   // ipm_set_cg_precond
  int64_t cg_solves = 0, cg_total = 0, cg_last_iters = 0, cg_last_info = 0;
};

inline hipStream_t S(ipm_problem* pr) { return pr->h->stream; }

// the objective has a quadratic term: a dense P, or the factors of IPM_SOLVE_CHOLESKY_DUAL_QP
inline bool has_P(const ipm_problem* pr) { return pr->d.P != nullptr || pr->dualqp; }

inline unsigned* trsv_err(ipm_problem* pr) { return reinterpret_cast<unsigned*>(pr->info + RB_INFO_TRSV_ERR); }
// the Jacobi eigensolver's info (lstsq_sym_factor) goes to its own word: the Cholesky info words
// keep meaning "factorization failed" (Q9), and a non-converged eigensolve surfaces at the readback
inline int* lsq_info(ipm_problem* pr) { return pr->info + RB_INFO_LSQ; }

// the bound segments of inv (after barrier_pieces) and of a slack vector s; null without that bound
inline const double* inv_lb(ipm_problem* pr) {
  if (!pr->d.lb) return nullptr;
  return pr->socp ? pr->inv + pr->K + pr->nub : pr->inv + pr->m + pr->nub;
}
inline const double* inv_ub(ipm_problem* pr) {
  if (!pr->d.ub) return nullptr;
  return pr->socp ? pr->inv + pr->K : pr->inv + pr->m;
}
inline const double* s_lb(ipm_problem* pr, const double* s) {
  if (!pr->d.lb) return nullptr;
  return pr->socp ? s + pr->K + pr->nub : s + pr->m + pr->nub;
}
inline const double* s_ub(ipm_problem* pr, const double* s) {
  if (!pr->d.ub) return nullptr;
  return pr->socp ? s + pr->K : s + pr->m;
}

// the LP-family Hessian's vectors w and dvec at slack state s (ipm_engine.hip)
void hessian_vectors_lin(ipm_problem* pr, const double* s, double add);
