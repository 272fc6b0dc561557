// ipm_soft.hip -- the batched fp64 IPM with soft box constraints (srbd_qp_solve_soft_f64).
//
// HPIPM's soft constraints (Zl / Zu / zl / zu / idxs / lls / lus) on box bounds: a softened
// bound gets a slack s >= lls on each active side, penalised by 1/2 Z s^2 + z s.  The slacks
// belong to one bound each, so they are eliminated on the bound's lane and the Riccati
// recursion is the hard-constraint one with another diagonal (ipm_box_impl.h, "soft boxes").
// The SOFT instantiations of the phase kernels live in this translation unit alone, so the
// hard-constraint kernels of ipm_box.hip keep their code.
#include "kernels.h"

#include "riccati.h"

#define SRBD_IPM_SOFT_TU 1
#define SRBD_REAL double
#define SRBD_NS ipm_soft_f64
#include "ipm_box_impl.h"
#undef SRBD_REAL
#undef SRBD_NS

namespace srbd {

size_t ws_doubles_soft(int N) { return (size_t)(N + 1) * kSoftStage; }

hipError_t launch_ipm_soft(const ProblemArgsT<double>& a, const SoftArgsT<double>& s, hipStream_t stream) {
  return ipm_soft_f64::launch_soft(a, s, stream);
}

}  // namespace srbd
