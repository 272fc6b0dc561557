// srbd_rollout.hip -- the kernels between two NMPC steps of the closed loop
// (srbd_qp_srbd_advance_f64 / srbd_qp_srbd_rollout_f64):
//   srbd_advance_kernel   per robot: the applied input u0 = us[0], the plant's RK4 steps from x
//                         with u0 (and an external wrench), the new last stage of the guess and
//                         the in-place shift of xs / us by one stage;
//   rollout_rows_kernel   strided row copies: the gather of one tick's plan window out of a
//                         plan longer than the horizon, x_log[:, 0], and the per-tick alpha.
// The model is srbd_model.h's, the one the linearisation and the line search evaluate.  The host
// restatement that pins both is srbd_model.py (plant_step, shift_guess).
#include "../../include/srbd_qp.h"
#include "kernels.h"
#include "srbd_model.h"

namespace srbd {
namespace {

constexpr int kWave = 64;
constexpr int kAdvWaves = 4;  // robots per block

struct AdvArgs {
  int batch, N, substeps;
  double *xs, *us;       // [batch][N+1][12], [batch][N][12], shifted in place
  double* x;             // [batch][12] plant state, in place (NULL: shift only)
  const double* wrench;  // wrench + qp * wrench_stride: 6 doubles (NULL: none)
  long long wrench_stride;
  double* u_out;  // u_out + qp * u_stride: the applied input (NULL: not written)
  long long u_stride;
  double* x_out;  // x_out + qp * x_stride: a copy of the new plant state (NULL: not written)
  long long x_stride;
  // the rollout's logs: it_log[qp * log_stride] = it_src[qp], the same for cv (NULL: none)
  const int *it_src, *cv_src;
  int *it_log, *cv_log;
  long long log_stride;
};
// With robots: what the two lanes that run the model read of the handle's roles, the mass
// and the inertia.  The launcher has resolved the plant's fallback to the MODEL role per field;
// a field that is still NULL is Model::p's.
struct AdvRobots {
  const double *model_mass, *model_Lbody;  // lane 1
  const double *plant_mass, *plant_Lbody;  // lane 0
};
struct NoAdvRobots {};
template <bool PLAN, bool ROBOT>
struct AdvArgsT : AdvArgs, PlanArgs<PLAN>, std::conditional_t<ROBOT, AdvRobots, NoAdvRobots> {};

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

// One wave per robot.
//   Lane 0 is the plant: u0 = us[0] (also written to u_out), x <- `substeps` RK4 steps of
//   dt / substeps with u0, the wrench and stage 0's feet.  Lane 1 is the new last stage:
//   xN = one RK4 step over dt from xs[N] with us[N-1] and stage N-1's feet, no wrench.  Both
//   run the same code on their own inputs.  With robots, lane 0 integrates the true robot
//   (the PLANT role's mass and inertia, else the MODEL role's, else Model::p's) and lane 1 the
//   robot the controller believes in (the MODEL role's).
//   Then the whole wave shifts the robot's rows by one stage (12 doubles = 6 double2), in place:
//   xs[k] <- xs[k+1] (k < N), us[k] <- us[k+1] (k < N-1), and lane 1 stores xN to xs[N].
//
// Why the in-place shift is race-free: a robot's rows are touched by this one wave only, and a
// wave's memory instructions take effect in program order.  The wave walks a row in ascending
// chunks of 64 double2; chunk c loads elements [64c + 6, 64c + 70) with ONE load instruction and
// then stores them to [64c, 64c + 64) with ONE store instruction.  Every element the store
// overwrites that is still needed ([64c + 6, 64c + 64)) was read by the load before it, and the
// elements later chunks read (>= 64c + 70) lie above everything stored so far.  The model's
// inputs us[0], xs[N], us[N-1] are loaded and consumed by lanes 0 / 1 before the first store of
// the shift (the stores may alias them, so the compiler keeps that order), and xN is stored
// after the last chunk has read the old xs[N].  The wave barriers (no instruction, convergent)
// keep the compiler from moving memory accesses across these points and from duplicating the
// shift into the divergent branches before it, where it would no longer run as whole-wave
// instructions.
// Rows are multiples of 96 bytes and the shift is 96 bytes, so the double2 accesses stay 16-byte
// aligned (the entry point checks the base pointers), adjacent lanes on adjacent 16 bytes.
template <bool PLAN, bool ROBOT>
__global__ void __launch_bounds__(kWave* kAdvWaves) srbd_advance_kernel(Model m, AdvArgsT<PLAN, ROBOT> a) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long qp = (long long)blockIdx.x * kAdvWaves + (threadIdx.x >> 6);
  if (qp >= a.batch) return;  // wave-uniform
  const int N = a.N;
  const srbd_model_params& p = m.p;
  double* xs = a.xs + (size_t)qp * (N + 1) * 12;
  double* us = a.us + (size_t)qp * N * 12;
  double xv[12];  // lane 0: the plant state; lane 1: xN
  if (lane < 2) {
    const bool plant = lane == 0;
    const int k = plant ? 0 : N - 1;  // the stage whose input and feet this lane uses
    double u[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) u[i] = us[(size_t)k * 12 + i];
    const bool run = !plant || a.x != nullptr;
    if (run) {
      const double* xin = plant ? a.x + (size_t)qp * 12 : xs + (size_t)N * 12;
#pragma unroll
      for (int i = 0; i < 12; ++i) xv[i] = xin[i];
      const StageVals<PLAN> sv = load_stage<PLAN>(p, a, (size_t)qp * N + k);
      RobotArgs<ROBOT> role{};
      if constexpr (ROBOT) {
        role.mass = plant ? a.plant_mass : a.model_mass;
        role.Lbody = plant ? a.plant_Lbody : a.model_Lbody;
      }
      const RobotVals<ROBOT> rb = load_robot<ROBOT>(p, role, (size_t)qp);
      double wr[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      const bool has_w = plant && a.wrench != nullptr;
      if (has_w) {
#pragma unroll
        for (int i = 0; i < 6; ++i) wr[i] = a.wrench[(size_t)qp * a.wrench_stride + i];
      }
      const int steps = plant ? a.substeps : 1;
      rk4_steps(m, sv, rb, xv, u, wr, has_w, p.dt / (double)steps, steps);
    }
    if (plant) {
      if (a.u_out) {
#pragma unroll
        for (int i = 0; i < 12; ++i) a.u_out[(size_t)qp * a.u_stride + i] = u[i];
      }
      if (run) {
#pragma unroll
        for (int i = 0; i < 12; ++i) a.x[(size_t)qp * 12 + i] = xv[i];
        if (a.x_out) {
#pragma unroll
          for (int i = 0; i < 12; ++i) a.x_out[(size_t)qp * a.x_stride + i] = xv[i];
        }
      }
    }
  } else if (lane == 2) {
    if (a.it_log) a.it_log[(size_t)qp * a.log_stride] = a.it_src[qp];
    if (a.cv_log) a.cv_log[(size_t)qp * a.log_stride] = a.cv_src[qp];
  }
  // ---- the shift (see above): one load, then one store per chunk ----
  __builtin_amdgcn_wave_barrier();
  double2* xs2 = reinterpret_cast<double2*>(xs);
  const int nx2 = 6 * N;  // double2 of xs[0 .. N-1]
  for (int c = 0; c < nx2; c += kWave) {
    const int i = c + lane;
    double2 v = make_double2(0.0, 0.0);
    if (i < nx2) v = xs2[i + 6];
    __builtin_amdgcn_wave_barrier();
    if (i < nx2) xs2[i] = v;
    __builtin_amdgcn_wave_barrier();
  }
  double2* us2 = reinterpret_cast<double2*>(us);
  const int nu2 = 6 * (N - 1);  // us[N-1] stays
  for (int c = 0; c < nu2; c += kWave) {
    const int i = c + lane;
    double2 v = make_double2(0.0, 0.0);
    if (i < nu2) v = us2[i + 6];
    __builtin_amdgcn_wave_barrier();
    if (i < nu2) us2[i] = v;
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 1) {
#pragma unroll
    for (int i = 0; i < 6; ++i) xs2[nx2 + i] = make_double2(xv[2 * i], xv[2 * i + 1]);
  }
}

// Up to four strided row copies in one launch, dst[r * dstride + e] = src[r * sstride + e] for
// e < width: the rollout's gather of tick t's plan window (row r = robot, src offset by t
// stages) and x_log[:, 0].  With `alpha`, alpha[r] = alpha_value as well.  Scalar accesses: the
// feet's rows start at multiples of 3 doubles.
struct RowCopy {
  const double* src;
  double* dst;
  int width;
  long long sstride, dstride;
};
struct RowsArgs {
  int batch, total;  // total = sum of the widths
  RowCopy c[4];
  double* alpha;
  double alpha_value;
};
__global__ void __launch_bounds__(256) rollout_rows_kernel(RowsArgs a) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (a.alpha && g < a.batch) a.alpha[g] = a.alpha_value;
  if (a.total == 0 || g >= (long long)a.batch * a.total) return;
  const long long r = g / a.total;
  int e = (int)(g - r * a.total);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const RowCopy& c = a.c[s];
    if (e >= 0 && e < c.width) c.dst[(size_t)r * c.dstride + e] = c.src[(size_t)r * c.sstride + e];
    e -= c.width;
  }
}

}  // namespace

hipError_t launch_srbd_advance(const srbd_model_params& p, int batch, int N, const AdvanceIo& io,
                               const srbd_plan_f64* plan, hipStream_t stream, const srbd_robots_f64* robots,
                               const srbd_robots_f64* plant) {
  if (batch <= 0) return hipSuccess;
  Model m{p};
  AdvArgs a{};
  a.batch = batch;
  a.N = N;
  a.substeps = io.substeps;
  a.xs = io.xs;
  a.us = io.us;
  a.x = io.x;
  a.wrench = io.wrench;
  a.wrench_stride = io.wrench_stride;
  a.u_out = io.u_out;
  a.u_stride = io.u_stride;
  a.x_out = io.x_out;
  a.x_stride = io.x_stride;
  a.it_src = io.it_src;
  a.cv_src = io.cv_src;
  a.it_log = io.it_log;
  a.cv_log = io.cv_log;
  a.log_stride = io.log_stride;
  const dim3 grid((unsigned)((batch + kAdvWaves - 1) / kAdvWaves)), block(kWave * kAdvWaves);
  // the kernel reads the feet only: a plan without them is the plan-less kernel; and of the
  // robots the mass and the inertia only
  AdvRobots r{};
  if (robots) {
    r.model_mass = r.plant_mass = robots->mass;
    r.model_Lbody = r.plant_Lbody = robots->Lbody;
  }
  if (plant && plant->mass) r.plant_mass = plant->mass;
  if (plant && plant->Lbody) r.plant_Lbody = plant->Lbody;
  const bool with_plan = plan && (plan->foot_r || plan->foot_l);
  const bool with_robots = r.model_mass || r.model_Lbody || r.plant_mass || r.plant_Lbody;
  auto launch = [&](auto PL, auto RB) {
    constexpr bool kP = decltype(PL)::value, kR = decltype(RB)::value;
    AdvArgsT<kP, kR> full;
    static_cast<AdvArgs&>(full) = a;
    if constexpr (kP) static_cast<srbd_plan_f64&>(full) = *plan;
    if constexpr (kR) static_cast<AdvRobots&>(full) = r;
    hipLaunchKernelGGL((srbd_advance_kernel<kP, kR>), grid, block, 0, stream, m, full);
  };
  if (with_plan && with_robots) launch(std::true_type{}, std::true_type{});
  else if (with_plan) launch(std::true_type{}, std::false_type{});
  else if (with_robots) launch(std::false_type{}, std::true_type{});
  else launch(std::false_type{}, std::false_type{});
  return hipGetLastError();
}

hipError_t launch_rollout_rows(int batch, const RolloutRow* rows, int nrows, double* alpha,
                               double alpha_value, hipStream_t stream) {
  if (batch <= 0) return hipSuccess;
  RowsArgs a{};
  a.batch = batch;
  for (int s = 0; s < nrows && s < 4; ++s) {
    a.c[s] = RowCopy{rows[s].src, rows[s].dst, rows[s].width, rows[s].sstride, rows[s].dstride};
    a.total += rows[s].width;
  }
  a.alpha = alpha;
  a.alpha_value = alpha_value;
  const long long n = (long long)batch * (a.total > 0 ? a.total : 1);
  if (a.total == 0 && !alpha) return hipSuccess;
  hipLaunchKernelGGL(rollout_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace srbd
