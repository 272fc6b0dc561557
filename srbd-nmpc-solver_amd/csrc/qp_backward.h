// qp_backward.h -- launch interface of the backward pass's own kernels (qp_backward.hip): the
// mask kernel that pins the active inputs of the adjoint QP, and the gradient kernel that turns
// the forward and the adjoint solution into the gradients of the QP data.
// Internal; the entry point is srbd_qp_solve_backward_f64 (capi_backward.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace srbd {

// The masked copy of the stages for a handle with input boxes.  Input (k, i) of a QP is pinned
// iff its bound is unmasked (a NULL mask: every bound) and u - lbu < act_tol or ubu - u < act_tol;
// then column i of B, row i of S, row and column i of R (1 on the diagonal) and entry i of r are
// cleared.  Every array is in the caller's dims and layout (QP-major, column-major blocks).
struct BackwardMaskArgs {
  int batch, N, nx, nu;
  const double *B, *S, *R;  // the QP's
  const double* gu;         // the cotangent that becomes r (NULL: zero)
  const double *u, *lbu, *ubu, *lbu_mask, *ubu_mask;
  double act_tol;
  double *Bm, *Sm, *Rm, *rm;  // out
  int* count;                 // out [batch]: pinned inputs per QP (NULL: not counted)
};
hipError_t launch_backward_mask(const BackwardMaskArgs& a, hipStream_t stream);

// The gradients.  x, u, pi: the forward solution; dx, du, dpi: the adjoint QP's.  An output
// whose pointer is NULL is skipped: its blocks are never formed.
struct BackwardGradArgs {
  int batch, N, nx, nu;
  const double *x, *u, *pi, *dx, *du, *dpi;
  double *A, *B, *b, *Q, *S, *R, *q, *r, *x0;
};
hipError_t launch_backward_grad(const BackwardGradArgs& a, hipStream_t stream);

}  // namespace srbd
