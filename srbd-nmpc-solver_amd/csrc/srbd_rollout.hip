// srbd_rollout.hip -- the kernels between two NMPC steps of the closed loop
// (srbd_qp_srbd_advance_f64 / srbd_qp_srbd_rollout_f64):
//   srbd_advance_kernel   per robot: the applied input u0 = us[0], the plant's RK4 steps from x
//                         with u0 (and an external wrench), the new last stage of the guess and
//                         the in-place shift of xs / us by one stage; with a contact model
//                         (srbd_contact_f64) u0 is first projected onto what the
//                         feet can transmit, and fallen robots are frozen;
//   rollout_rows_kernel   strided row copies: the gather of one tick's plan window out of a
//                         plan longer than the horizon, x_log[:, 0], and the per-tick alpha.
// The model is srbd_model.h's, the one the linearisation and the line search evaluate.  The host
// restatement that pins both is srbd_model.py (plant_step, shift_guess).
#include "../../include/srbd_qp.h"
#include "kernels.h"
#include "srbd_model.h"
#include "srbd_rk4.h"
#include "srbd_terrain.h"

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
// With a contact: the handle's srbd_contact_f64, read by lane 0 only.
struct AdvContact {
  srbd_contact_f64 c;
};
struct NoAdvContact {};
template <bool PLAN, bool ROBOT, bool CONTACT>
struct AdvArgsT : AdvArgs,
                  PlanArgs<PLAN>,
                  std::conditional_t<ROBOT, AdvRobots, NoAdvRobots>,
                  std::conditional_t<CONTACT, AdvContact, NoAdvContact> {};

// rk4_steps, the plant's integrator, is srbd_rk4.h's: the open-loop plant rollout shares it.

// The model step of lanes 0 and 1 with a contact (srbd_contact_f64; include/srbd_qp.h states the
// plant step operation for operation, srbd_model.py's plant_step(contact=...) restates it).
// Lane 1 takes no part in the contact: it runs rk4_steps on its own inputs as without one.  Lane
// 0 projects its input u in place onto what the feet can transmit (u then is the applied input),
// moves the feet in contact onto the true ground, integrates, and tests the new state for a
// fall; a robot that has fallen, or whose input is not finite, runs zero RK4 steps, so its x
// keeps its bits.  Each bound of the projection is one multiplication and nothing is added to
// it, so no operation is fused and the host statement agrees to the bit.  `xin` is the plant
// state in memory (not yet overwritten), `h` the RK4 step length.  Both lanes go through one
// call site of rk4_steps, with the feet as values (lane 0's may have moved).
template <bool PLAN, class Args, class Rb>
__device__ __forceinline__ void contact_step(const Model& m, const Args& a, const StageVals<PLAN>& sv, const Rb& rb,
                                             long long qp, bool plant, const double* xin, double (&xv)[12],
                                             double (&u)[12], const double (&wr)[6], bool has_w, double h,
                                             int steps) {
  const srbd_model_params& p = m.p;
  const srbd_contact_f64& c = a.c;
  StageVals<true> sc;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    sc.fr[i] = sv.foot_r(p, i);
    sc.fl[i] = sv.foot_l(p, i);
  }
#pragma unroll
  for (int f = 0; f < 2; ++f) sc.fz[f] = sv.fz_max(p, f);
  const srbd_terrain_f64& g = c.ground;
  const double* H = nullptr;  // lane 0: the robot's map of the true ground
  bool test = false;          // lane 0: the robot stood on entry and its input is finite
  if (plant) {
    const bool frozen = c.fallen && c.fallen[qp] != 0;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) finite = finite && __builtin_isfinite(u[i]);
    if (frozen || !finite) {
      if (!frozen && c.fallen) c.fallen[qp] = 1;
#pragma unroll
      for (int i = 0; i < 12; ++i) u[i] = 0.0;
      steps = 0;
    } else {
      const double mu = c.mu_r ? c.mu_r[qp] : c.mu;
      bool on[2] = {true, true};  // the contact flags
      if constexpr (PLAN) {
        if (a.fz_max) {
          on[0] = sc.fz[0] > c.fz_contact;
          on[1] = sc.fz[1] > c.fz_contact;
        }
      }
      const double Lt[3] = {c.Ltx, c.Lty, c.Ltz};
      unsigned sat = 0;
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const int o = 6 * f;
        const double fz = u[o + 2];
        const double fzp = on[f] ? fmin(fmax(fz, 0.0), c.fz_hi) : 0.0;
        const double b = mu * fzp;
        const double fxp = fmin(fmax(u[o], -b), b), fyp = fmin(fmax(u[o + 1], -b), b);
        if (fzp != fz) sat |= ((!on[f] || fzp > fz) ? 1u : 2u) << (4 * f);
        if (fxp != u[o] || fyp != u[o + 1]) sat |= 4u << (4 * f);
        bool torque = false;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const double bt = Lt[t] * fzp;
          const double tp = fmin(fmax(u[o + 3 + t], -bt), bt);
          torque = torque || tp != u[o + 3 + t];
          u[o + 3 + t] = tp;
        }
        if (torque) sat |= 8u << (4 * f);
        u[o] = fxp;
        u[o + 1] = fyp;
        u[o + 2] = fzp;
      }
      if (c.sat && sat) c.sat[qp] |= sat;
      if (g.height) {
        H = g.height + (size_t)(g.map_r ? g.map_r[qp] : 0) * g.ny * g.nx;
        if (on[0]) sc.fr[2] = c.ground_z + terrain_bilinear(H, g.nx, g.ny, g.x0, g.y0, g.cell, sc.fr[0], sc.fr[1]);
        if (on[1]) sc.fl[2] = c.ground_z + terrain_bilinear(H, g.nx, g.ny, g.x0, g.y0, g.cell, sc.fl[0], sc.fl[1]);
      }
      test = c.fallen != nullptr;
    }
  }
  rk4_steps(m, sc, rb, xv, u, wr, has_w, h, steps);
  if (test) {
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) finite = finite && __builtin_isfinite(xv[i]);
    bool fell = true;
    if (!finite) {  // the state of before the step
#pragma unroll
      for (int i = 0; i < 12; ++i) xv[i] = xin[i];
    } else {
      const double hg = H ? terrain_bilinear(H, g.nx, g.ny, g.x0, g.y0, g.cell, xv[6], xv[7]) : 0.0;
      fell = xv[8] - (c.ground_z + hg) < c.z_min || expm(seg(xv, 0)).a[2][2] < c.cos_tilt_min;
    }
    if (fell) c.fallen[qp] = 1;
    else if (c.alive) c.alive[qp] += 1;
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
//
// CONTACT (a contact model on the handle, and a plant state to step): lane 0's step is
// contact_step's -- a few min / max, up to three samples of the true ground and the fall test,
// all while lane 1 waits masked, as it already does through lane 0's substeps.  The lanes, the
// whole-wave shift and the barriers are as without; CONTACT = false is the code without.
template <bool PLAN, bool ROBOT, bool CONTACT>
__global__ void __launch_bounds__(kWave* kAdvWaves)
    srbd_advance_kernel(Model m, AdvArgsT<PLAN, ROBOT, CONTACT> a) {
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
      if constexpr (CONTACT)
        contact_step<PLAN>(m, a, sv, rb, qp, plant, xin, xv, u, wr, has_w, p.dt / (double)steps, steps);
      else
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
                               const srbd_robots_f64* plant, const srbd_contact_f64* contact) {
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
  // a contact is read by the plant step only: without a plant state it is the kernel without.
  // With it the contact flags come from the plan's fz_max, so a plan of fz_max alone is a plan
  const bool with_contact = contact && io.x;
  const bool with_plan = plan && (plan->foot_r || plan->foot_l || (with_contact && plan->fz_max));
  const bool with_robots = r.model_mass || r.model_Lbody || r.plant_mass || r.plant_Lbody;
  auto launch = [&](auto PL, auto RB, auto CT) {
    constexpr bool kP = decltype(PL)::value, kR = decltype(RB)::value, kC = decltype(CT)::value;
    AdvArgsT<kP, kR, kC> full;
    static_cast<AdvArgs&>(full) = a;
    if constexpr (kP) static_cast<srbd_plan_f64&>(full) = *plan;
    if constexpr (kR) static_cast<AdvRobots&>(full) = r;
    if constexpr (kC) full.c = *contact;
    hipLaunchKernelGGL((srbd_advance_kernel<kP, kR, kC>), grid, block, 0, stream, m, full);
  };
  auto pick = [&](auto CT) {
    if (with_plan && with_robots) launch(std::true_type{}, std::true_type{}, CT);
    else if (with_plan) launch(std::true_type{}, std::false_type{}, CT);
    else if (with_robots) launch(std::false_type{}, std::true_type{}, CT);
    else launch(std::false_type{}, std::false_type{}, CT);
  };
  if (with_contact) pick(std::true_type{});
  else pick(std::false_type{});
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
