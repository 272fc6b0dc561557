// qp_backward_rows.h -- launch interface of the two kernels the backward pass adds for general
// rows on the inputs and for the gradients of D and the bounds (qp_backward_rows.hip; DESIGN.md
// 4.13).  Internal; the entry point is srbd_qp_solve_backward_rows_f64 (capi_backward.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace srbd {

// One struct for both kernels: each stage's active set is a function of these inputs alone, and
// the lift kernel forms it again instead of reading a stored factor.  Every array is in the
// caller's dims and layout (QP-major, column-major blocks; lg, ug and their masks have N + 1 rows
// per QP, of which row N is never active).
struct BackwardRowsArgs {
  int batch, N, nx, nu, ng;
  // the active set: pinned inputs (lbu NULL: no boxes), then active general rows (ng > 0)
  const double *u, *lbu, *ubu, *lbu_mask, *ubu_mask;
  const double *D, *lg, *ug, *lg_mask, *ug_mask;
  double act_tol, rank_tol;
  // projection: the QP's B, S, R and the cotangent that becomes r (NULL: zero) -> the stages the
  // adjoint QP is solved on, and [batch][3] counts (pinned, rows accepted, rows dropped; the
  // launcher clears them first; NULL: not counted)
  const double *B, *S, *R, *gu;
  double *Bm, *Sm, *Rm, *rm;
  int* count;
  // lift: the forward solution and r, the adjoint solution -> the gradients of D and the bounds
  // (any NULL: not formed; one that is passed is fully written, zeros included)
  const double *x, *pi, *r, *dx, *du, *dpi;
  double *gD, *glg, *gug, *glbu, *gubu;
  // lift, internal (srbd_qp_srbd_solve_backward_f64): the multipliers of the general rows and of
  // their adjoint as the kernel holds them, [batch][N][ng], 0 for an inactive or dropped row
  // (NULL: not written)
  double *nu_out, *dnu_out;
};
hipError_t launch_backward_project(const BackwardRowsArgs& a, hipStream_t stream);
hipError_t launch_backward_lift(const BackwardRowsArgs& a, hipStream_t stream);

}  // namespace srbd
