// srbd_terrain.h -- the height-map sampler of srbd_terrain_f64 (include/srbd_qp.h states the
// formula), shared by the kernels that read a map: the gait planner and the public sampler
// (srbd_gait.hip) and the plant's true ground (srbd_rollout.hip).  Internal linkage: each
// translation unit compiles its own copy.
#ifndef SRBD_TERRAIN_H_
#define SRBD_TERRAIN_H_
#include <hip/hip_runtime.h>

namespace srbd {
namespace {

// Clamped bilinear height of one map: H is [ny][nx].
__device__ __forceinline__ double terrain_bilinear(const double* H, int nx, int ny, double x0, double y0,
                                                   double cell, double x, double y) {
  const double s = fmin(fmax((x - x0) / cell, 0.0), (double)(nx - 1));
  const double t = fmin(fmax((y - y0) / cell, 0.0), (double)(ny - 1));
  const int i = min((int)floor(s), nx - 2), j = min((int)floor(t), ny - 2);
  const double a = s - (double)i, b = t - (double)j;
  const double* r0 = H + (size_t)j * nx + i;
  const double* r1 = r0 + nx;
  return (1.0 - b) * ((1.0 - a) * r0[0] + a * r0[1]) + b * ((1.0 - a) * r1[0] + a * r1[1]);
}

}  // namespace
}  // namespace srbd
#endif  // SRBD_TERRAIN_H_
