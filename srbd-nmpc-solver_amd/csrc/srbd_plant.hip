// srbd_plant.hip -- the true robot without the controller around it:
//   srbd_plant_rollout_kernel      the open-loop plant rollout (srbd_qp_srbd_plant_rollout_f64):
//                                  T ticks of the plant step of srbd_advance_kernel from x0 with
//                                  the inputs, feet and wrench it is given, every state kept;
//   srbd_plant_rollout_bwd_kernel  its adjoint through time (srbd_qp_srbd_plant_rollout_backward_f64):
//                                  the gradients of a trajectory loss with respect to x0, the
//                                  inputs, the feet, the wrench, the mass and the inertia.
// One thread per robot in both: a robot's ticks are a chain, and a batch is thousands of robots.
// The integrator is srbd_rk4.h's (the closed loop's), the reverse of one slope is
// srbd_lin_backward.h's slope_reverse (the linearisation's).  The host restatements are
// srbd_model.py's plant_step and tests/plant_vjp_host.py.
#include "../../include/srbd_qp.h"
#include "kernels.h"
#include "srbd_lin_backward.h"
#include "srbd_model.h"
#include "srbd_rk4.h"

namespace srbd {
namespace {

constexpr int kPlantThreads = 64;

struct PlantArgs {
  int batch, T, substeps, foot_stages;
  const double* u;       // [batch][T][12]
  const double* wrench;  // [batch][T][6] or NULL
  const double* x0;      // forward: [batch][12]
  double* x_traj;        // forward: [batch][T+1][12], out
  const double* xt;      // backward: the forward's x_traj
  const double* gx;      // backward: [batch][T+1][12]
  srbd_plant_grad_f64 out;
};
// FEET: the feet of tick t are row qp * foot_stages + t of the plan part's foot_r / foot_l (its
// other fields are NULL).  ROBOT: the resolved mass / Lbody arrays in the robots part.
template <bool FEET, bool ROBOT>
struct PlantArgsT : PlantArgs, PlanArgs<FEET>, RobotArgs<ROBOT> {};

// rows of 12 doubles as six 16-byte accesses (the entry points check the base pointers)
__device__ __forceinline__ void load_row(const double* src, double (&v)[12]) {
  const double2* s2 = reinterpret_cast<const double2*>(src);
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double2 d = s2[i];
    v[2 * i] = d.x;
    v[2 * i + 1] = d.y;
  }
}
__device__ __forceinline__ void store_row(double* dst, const double (&v)[12]) {
  double2* d2 = reinterpret_cast<double2*>(dst);
#pragma unroll
  for (int i = 0; i < 6; ++i) d2[i] = make_double2(v[2 * i], v[2 * i + 1]);
}
__device__ __forceinline__ bool load_wrench(const PlantArgs& a, size_t row, double (&wr)[6]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) wr[i] = a.wrench ? a.wrench[row * 6 + i] : 0.0;
  return a.wrench != nullptr;
}

// x_traj[qp][0] = x0[qp]; x_traj[qp][t + 1] = x_traj[qp][t] after `substeps` RK4 steps with u[qp][t],
// the feet of tick t and wrench[qp][t]: srbd_advance_kernel's lane 0 without a contact, T times.
template <bool FEET, bool ROBOT>
__global__ void __launch_bounds__(kPlantThreads) srbd_plant_rollout_kernel(Model m, PlantArgsT<FEET, ROBOT> a) {
  const long long qp = (long long)blockIdx.x * kPlantThreads + threadIdx.x;
  if (qp >= a.batch) return;
  const srbd_model_params& p = m.p;
  const int T = a.T;
  double* xo = a.x_traj + (size_t)qp * (T + 1) * 12;
  double x[12];
  load_row(a.x0 + (size_t)qp * 12, x);
  store_row(xo, x);
  const RobotVals<ROBOT> rb = load_robot<ROBOT>(p, a, (size_t)qp);
  const double h = p.dt / (double)a.substeps;
#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    const size_t row = (size_t)qp * T + t;
    double u[12], wr[6];
    load_row(a.u + row * 12, u);
    const StageVals<FEET> sv = load_stage<FEET>(p, a, (size_t)qp * a.foot_stages + t);
    const bool has_w = load_wrench(a, row, wr);
    rk4_steps(m, sv, rb, x, u, wr, has_w, h, a.substeps);
    store_row(xo + (size_t)(t + 1) * 12, x);
  }
}

// The adjoint.  lam = d l / d x_traj[t + 1] (all later ticks included) walks back through the
// ticks; within a tick through the substeps, each recomputed from the tick's checkpoint
// x_traj[t]; within a substep through the four slopes, the last first:
//   kb_j = (h w_j / 6) lam + a_(j+1) pb_(j+1),  pb_j = J_x(p_j)' kb_j,  lam <- lam + sum_j pb_j
// with the points p_0 = x, p_j = x + a_j k_(j-1), a = (0, h/2, h/2, h), w = (1, 2, 2, 1).
// slope_reverse gives pb_j and the sums for 1 / Lbody, 1 / mass and the feet; the input's and
// the wrench's parts of a slope are formed here.  The three later points of a step live in LDS
// (point-major, thread-minor: no bank conflicts), so that the slope loop indexes them and keeps
// one copy of the reverse model.  No atomics, a fixed order: the same inputs give the same bits.
template <bool FEET, bool ROBOT>
__global__ void __launch_bounds__(kPlantThreads) srbd_plant_rollout_bwd_kernel(Model m, PlantArgsT<FEET, ROBOT> a) {
  __shared__ double pts_s[36 * kPlantThreads];
  const long long qp = (long long)blockIdx.x * kPlantThreads + threadIdx.x;
  if (qp >= a.batch) return;
  double* pts = pts_s + threadIdx.x;  // element e of this thread: pts[e * kPlantThreads]
  const srbd_model_params& p = m.p;
  const int T = a.T, S = a.substeps;
  const double* xc = a.xt + (size_t)qp * (T + 1) * 12;
  const double* gx = a.gx + (size_t)qp * (T + 1) * 12;
  const RobotVals<ROBOT> rb = load_robot<ROBOT>(p, a, (size_t)qp);
  const double h = p.dt / (double)S, im = 1.0 / rb.mass(p);
  const bool want_u = a.out.u != nullptr, want_w = a.out.wrench != nullptr;
  double lam[12];
  load_row(gx + (size_t)T * 12, lam);
  double giL[3] = {0.0, 0.0, 0.0}, gim = 0.0;  // the robot's sums over all ticks
#pragma unroll 1
  for (int t = T - 1; t >= 0; --t) {
    const size_t row = (size_t)qp * T + t;
    double u[12], wr[6];
    load_row(a.u + row * 12, u);
    const StageVals<FEET> sv = load_stage<FEET>(p, a, (size_t)qp * a.foot_stages + t);
    const bool has_w = load_wrench(a, row, wr);
    const V3 f0 = seg(u, 0), f1 = seg(u, 6);
    const V3 F{{f0.v[0] + f1.v[0], f0.v[1] + f1.v[1], f0.v[2] + f1.v[2]}};
    double ub[12], wb[6];
#pragma unroll
    for (int i = 0; i < 12; ++i) ub[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) wb[i] = 0.0;
    V3 kl{{0.0, 0.0, 0.0}};  // sum of kb[3:6] over the tick's slopes: the feet
#pragma unroll 1
    for (int s = S - 1; s >= 0; --s) {
      // the state at the start of substep s, from the checkpoint
      double x[12];
      load_row(xc + (size_t)t * 12, x);
      rk4_steps(m, sv, rb, x, u, wr, has_w, h, s);
      {  // the points of slopes 1..3
        double xq[12], kk[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) xq[i] = x[i];
#pragma unroll 1
        for (int j = 0; j < 3; ++j) {
          m.f(sv, rb, xq, u, kk);
          if (has_w) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
              kk[3 + i] += wr[i];
              kk[9 + i] += wr[3 + i] * im;
            }
          }
          const double hs = j < 2 ? 0.5 * h : h;
#pragma unroll
          for (int i = 0; i < 12; ++i) {
            xq[i] = x[i] + hs * kk[i];
            pts[(12 * j + i) * kPlantThreads] = xq[i];
          }
        }
      }
      double xb[12], sum[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) xb[i] = sum[i] = 0.0;
#pragma unroll 1
      for (int j = 3; j >= 0; --j) {
        const double wt = (j == 0 || j == 3) ? h / 6.0 : h / 3.0;
        const double hn = j == 2 ? h : (j == 3 ? 0.0 : 0.5 * h);  // a of the slope after it
        double xp[12], kb[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          xp[i] = j == 0 ? x[i] : pts[(12 * (j - 1) + i) * kPlantThreads];
          kb[i] = wt * lam[i] + hn * xb[i];
        }
        double bim = 0.0;
        slope_reverse(p, rb, xp, F, kb, true, giL, kl, bim, xb);
        const V3 kbl = seg(kb, 3), kbv = seg(kb, 9);
        gim += bim + (has_w ? dot3(seg(wr, 3), kbv) : 0.0);
#pragma unroll
        for (int i = 0; i < 12; ++i) sum[i] += xb[i];
        if (want_u) {
          const V3 p0{{sv.foot_r(p, 0) - xp[6], sv.foot_r(p, 1) - xp[7], sv.foot_r(p, 2) - xp[8]}};
          const V3 p1{{sv.foot_l(p, 0) - xp[6], sv.foot_l(p, 1) - xp[7], sv.foot_l(p, 2) - xp[8]}};
          const V3 c0 = cross(kbl, p0), c1 = cross(kbl, p1);
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            ub[i] += fma(kbv.v[i], im, c0.v[i]);
            ub[6 + i] += fma(kbv.v[i], im, c1.v[i]);
            ub[3 + i] += kbl.v[i];
            ub[9 + i] += kbl.v[i];
          }
        }
        if (want_w) {
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            wb[i] += kbl.v[i];
            wb[3 + i] = fma(kbv.v[i], im, wb[3 + i]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 12; ++i) lam[i] += sum[i];
    }
    if (want_u) {
#pragma unroll
      for (int i = 0; i < 12; ++i) a.out.u[row * 12 + i] = ub[i];
    }
    if (want_w) {
#pragma unroll
      for (int i = 0; i < 6; ++i) a.out.wrench[row * 6 + i] = wb[i];
    }
    // <kb[3:6], p x f> = p . (f x kb[3:6])
    if (a.out.foot_r) {
      const V3 c = cross(f0, kl);
#pragma unroll
      for (int i = 0; i < 3; ++i) a.out.foot_r[row * 3 + i] = c.v[i];
    }
    if (a.out.foot_l) {
      const V3 c = cross(f1, kl);
#pragma unroll
      for (int i = 0; i < 3; ++i) a.out.foot_l[row * 3 + i] = c.v[i];
    }
    double g[12];
    load_row(gx + (size_t)t * 12, g);
#pragma unroll
    for (int i = 0; i < 12; ++i) lam[i] += g[i];
  }
  if (a.out.x0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) a.out.x0[(size_t)qp * 12 + i] = lam[i];
  }
  // the chain rule from 1 / mass and 1 / Lbody, as srbd_lin_bwd_reduce_kernel's
  if (a.out.mass) a.out.mass[qp] = -gim * im * im;
  if (a.out.Lbody) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double iL = rb.inv_L(p, j);
      a.out.Lbody[(size_t)qp * 3 + j] = -giL[j] * iL * iL;
    }
  }
}

// FEET kernels only when a foot array is given, ROBOT kernels only when a role supplies a value
template <class Fn>
void plant_dispatch(const PlantArgs& a, const srbd_plant_rollout_f64& roll, const double* mass, const double* Lbody,
                    Fn&& fn) {
  const bool feet = roll.foot_r || roll.foot_l, robot = mass || Lbody;
  dispatch(feet, robot, [&](auto FT, auto RB) {
    constexpr bool kF = decltype(FT)::value, kR = decltype(RB)::value;
    PlantArgsT<kF, kR> full{};
    static_cast<PlantArgs&>(full) = a;
    if constexpr (kF) {
      full.foot_r = roll.foot_r;
      full.foot_l = roll.foot_l;
    }
    if constexpr (kR) {
      full.mass = mass;
      full.Lbody = Lbody;
    }
    fn(full);
  });
}

PlantArgs plant_args(int batch, const srbd_plant_rollout_f64& roll) {
  PlantArgs a{};
  a.batch = batch;
  a.T = roll.ticks;
  a.substeps = roll.substeps;
  a.foot_stages = roll.foot_stages > 0 ? roll.foot_stages : roll.ticks;
  a.u = roll.u;
  a.wrench = roll.wrench;
  return a;
}

}  // namespace

hipError_t launch_srbd_plant_rollout(const srbd_model_params& p, int batch, const srbd_plant_rollout_f64& roll,
                                     const double* mass, const double* Lbody, const double* x0, double* x_traj,
                                     hipStream_t stream) {
  if (batch <= 0) return hipSuccess;
  Model m{p};
  PlantArgs a = plant_args(batch, roll);
  a.x0 = x0;
  a.x_traj = x_traj;
  const dim3 grid((unsigned)((batch + kPlantThreads - 1) / kPlantThreads)), block(kPlantThreads);
  plant_dispatch(a, roll, mass, Lbody, [&](auto full) {
    using A = decltype(full);
    constexpr bool kF = std::is_base_of_v<srbd_plan_f64, A>, kR = std::is_base_of_v<srbd_robots_f64, A>;
    hipLaunchKernelGGL((srbd_plant_rollout_kernel<kF, kR>), grid, block, 0, stream, m, full);
  });
  return hipGetLastError();
}

hipError_t launch_srbd_plant_rollout_backward(const srbd_model_params& p, int batch,
                                              const srbd_plant_rollout_f64& roll, const double* mass,
                                              const double* Lbody, const double* x_traj, const double* gx,
                                              const srbd_plant_grad_f64& grad, hipStream_t stream) {
  if (batch <= 0) return hipSuccess;
  if (!grad.x0 && !grad.u && !grad.foot_r && !grad.foot_l && !grad.wrench && !grad.mass && !grad.Lbody)
    return hipSuccess;
  Model m{p};
  PlantArgs a = plant_args(batch, roll);
  a.xt = x_traj;
  a.gx = gx;
  a.out = grad;
  const dim3 grid((unsigned)((batch + kPlantThreads - 1) / kPlantThreads)), block(kPlantThreads);
  plant_dispatch(a, roll, mass, Lbody, [&](auto full) {
    using A = decltype(full);
    constexpr bool kF = std::is_base_of_v<srbd_plan_f64, A>, kR = std::is_base_of_v<srbd_robots_f64, A>;
    hipLaunchKernelGGL((srbd_plant_rollout_bwd_kernel<kF, kR>), grid, block, 0, stream, m, full);
  });
  return hipGetLastError();
}

}  // namespace srbd
