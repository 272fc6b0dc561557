// srbd_rk4.h -- the plant's integrator, shared by the kernels that move the true robot: the
// closed loop's plant step (srbd_rollout.hip) and the open-loop plant rollout and its adjoint
// (srbd_plant.hip).  Internal: device code with internal linkage, as srbd_model.h.
#pragma once

#include "srbd_model.h"

namespace srbd {
namespace {

// `steps` classical RK4 steps of length h of xdot = f(x, u) + w from x (in place).  With has_w,
// w adds wr[0:3] to rows 3..5 and wr[3:6] / mass to rows 9..11 of every slope.  The slopes
// go through one call site of the model, as in the line search's stage_merit.
template <class St, class Rb>
__device__ __forceinline__ void rk4_steps(const Model& m, const St& sv, const Rb& rb, double (&x)[12],
                                          const double (&u)[12], const double (&wr)[6], bool has_w, double h,
                                          int steps) {
  double fw[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) fw[i] = wr[3 + i] / rb.mass(m.p);
#pragma unroll 1
  for (int st = 0; st < steps; ++st) {
    double acc[12], xt[12], kk[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      acc[i] = 0.0;
      xt[i] = x[i];
    }
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {
      m.f(sv, rb, xt, u, kk);
      if (has_w) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          kk[3 + i] += wr[i];
          kk[9 + i] += fw[i];
        }
      }
      const double wt = (s == 0 || s == 3) ? 1.0 : 2.0;
      const double hs = s < 2 ? 0.5 * h : h;
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        acc[i] += wt * kk[i];
        xt[i] = x[i] + hs * kk[i];
      }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) x[i] = x[i] + (h / 6.0) * acc[i];
  }
}

}  // namespace
}  // namespace srbd
