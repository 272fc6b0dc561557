// srbd_model.h -- the SRBD model on the device, shared by the kernels that evaluate it: the
// linearisation and the line search (srbd_linearize.hip) and the closed loop's plant step
// (srbd_rollout.hip).  dynamics/SRBD_model.cpp: GetContinuousDynamic (:75-176) incl. its
// Jacobians, GetConstrain (:237-260), Barrier (:262-295), with the SO(3) helpers of
// dynamics/orientation_tool.h:76-227, and the per-stage plan values (srbd_plan_f64).
// Everything here has internal linkage: each translation unit compiles its own copy.
#ifndef SRBD_MODEL_H_
#define SRBD_MODEL_H_
#include "../../include/srbd_qp.h"

#include <hip/hip_runtime.h>

#include <type_traits>

namespace srbd {
namespace {

struct M3 {
  double a[3][3];
};
struct V3 {
  double v[3];
};

__device__ __forceinline__ M3 zero3() {
  M3 m;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m.a[i][j] = 0.0;
  return m;
}
__device__ __forceinline__ M3 eye3(double s = 1.0) {
  M3 m = zero3();
  for (int i = 0; i < 3; ++i) m.a[i][i] = s;
  return m;
}
__device__ __forceinline__ M3 skew(const V3& v) {
  M3 m = zero3();
  m.a[0][1] = -v.v[2];
  m.a[0][2] = v.v[1];
  m.a[1][0] = v.v[2];
  m.a[1][2] = -v.v[0];
  m.a[2][0] = -v.v[1];
  m.a[2][1] = v.v[0];
  return m;
}
__device__ __forceinline__ M3 mul(const M3& x, const M3& y) {
  M3 m;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s = fma(x.a[i][k], y.a[k][j], s);
      m.a[i][j] = s;
    }
  return m;
}
__device__ __forceinline__ M3 tr(const M3& x) {
  M3 m;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m.a[i][j] = x.a[j][i];
  return m;
}
// sum_t c_t * M_t (t = up to 3 terms)
__device__ __forceinline__ M3 lin(double a, const M3& x, double b, const M3& y) {
  M3 m;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m.a[i][j] = a * x.a[i][j] + b * y.a[i][j];
  return m;
}
__device__ __forceinline__ M3 add(const M3& x, const M3& y) { return lin(1.0, x, 1.0, y); }
__device__ __forceinline__ V3 mv(const M3& x, const V3& y) {
  V3 r;
  for (int i = 0; i < 3; ++i)
    r.v[i] = fma(x.a[i][0], y.v[0], fma(x.a[i][1], y.v[1], x.a[i][2] * y.v[2]));
  return r;
}
__device__ __forceinline__ V3 seg(const double* x, int o) { return V3{{x[o], x[o + 1], x[o + 2]}}; }

// theta with the 1e-10 clamp (orientation_tool.h:82-86)
__device__ __forceinline__ double theta_of(const V3& v) {
  const double t = sqrt(v.v[0] * v.v[0] + v.v[1] * v.v[1] + v.v[2] * v.v[2]);
  return t > 1e-10 ? t : 1e-10;
}
// expm (orientation_tool.h:76-100)
__device__ M3 expm(const V3& v) {
  const double th = theta_of(v);
  const M3 V = skew(v);
  return add(eye3(), lin(sin(th) / th, V, (1.0 - cos(th)) / (th * th), mul(V, V)));
}
// left Jacobian jl (:102-130) and its inverse jlt (:132-160)
__device__ M3 jl(const V3& v) {
  const double th = theta_of(v);
  const M3 V = lin(1.0 / th, skew(v), 0.0, eye3());
  const double s = sin(th) / th;
  return add(add(eye3(s), lin(1.0 - s, add(mul(V, V), eye3()), 0.0, V)), lin((1.0 - cos(th)) / th, V, 0.0, V));
}
__device__ M3 jlt(const V3& v) {
  const double th = theta_of(v);
  const M3 V = lin(1.0 / th, skew(v), 0.0, eye3());
  const double ct = 0.5 * th / tan(0.5 * th);
  return add(add(eye3(ct), lin(1.0 - ct, add(mul(V, V), eye3()), 0.0, V)), lin(-0.5 * th, V, 0.0, V));
}
// d jl / d v_a (:162-200), a = 0..2
__device__ M3 djl(const V3& v, int a) {
  const double th = theta_of(v);
  const double s = sin(th), c = cos(th), th2 = th * th, th3 = th2 * th;
  const M3 sv = skew(v);
  const M3 V = lin(1.0 / th, sv, 0.0, sv);
  const M3 base = lin((th * s + 2.0 * (c - 1.0)) / th3, V, -(2.0 * th - 3.0 * s + th * c) / th3, mul(V, V));
  V3 e{{0.0, 0.0, 0.0}};
  e.v[a] = 1.0;
  const M3 se = skew(e);
  const M3 d = lin((th - s) / th3, add(mul(se, sv), mul(sv, se)), (1.0 - c) / th2, se);
  return lin(1.0, d, v.v[a], base);
}

// A plan (srbd_plan_f64) overrides four of the model's constants per robot and stage: the
// reference state, the two foot positions and the normal-force limit of each foot.  Kernels
// and helpers that read them take a `bool PLAN`: false is the code without plans (the values
// are Model::p's, StageVals is empty), true loads them from the plan's arrays, a NULL array
// falling back to Model::p on a wave-uniform branch.
struct NoPlan {};
template <bool PLAN>
using PlanArgs = std::conditional_t<PLAN, srbd_plan_f64, NoPlan>;

// The foot positions and force limits of one (robot, stage).  With a plan they are loaded once
// per stage and stay in registers: Model::f runs four times per stage.
template <bool PLAN>
struct StageVals {
  __device__ __forceinline__ double foot_r(const srbd_model_params& p, int i) const { return p.foot_r[i]; }
  __device__ __forceinline__ double foot_l(const srbd_model_params& p, int i) const { return p.foot_l[i]; }
  __device__ __forceinline__ double fz_max(const srbd_model_params& p, int) const { return p.fmax; }
};
template <>
struct StageVals<true> {
  double fr[3], fl[3], fz[2];
  __device__ __forceinline__ double foot_r(const srbd_model_params&, int i) const { return fr[i]; }
  __device__ __forceinline__ double foot_l(const srbd_model_params&, int i) const { return fl[i]; }
  __device__ __forceinline__ double fz_max(const srbd_model_params&, int leg) const { return fz[leg]; }
};
// t = qp * N + k: rows t of foot_r / foot_l ([batch][N][3]) and fz_max ([batch][N][2])
template <bool PLAN>
__device__ __forceinline__ StageVals<PLAN> load_stage(const srbd_model_params& p, const PlanArgs<PLAN>& pl,
                                                      size_t t) {
  StageVals<PLAN> s;
  if constexpr (PLAN) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      s.fr[i] = pl.foot_r ? pl.foot_r[t * 3 + i] : p.foot_r[i];
      s.fl[i] = pl.foot_l ? pl.foot_l[t * 3 + i] : p.foot_l[i];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) s.fz[i] = pl.fz_max ? pl.fz_max[t * 2 + i] : p.fmax;
  }
  return s;
}
// x_ref of element e = (qp * (N + 1) + k) * 12 + i of the [batch][N+1][12] arrays
template <bool PLAN>
__device__ __forceinline__ double x_ref_at(const srbd_model_params& p, const PlanArgs<PLAN>& pl, size_t e,
                                           int i) {
  if constexpr (PLAN) {
    if (pl.x_ref) return pl.x_ref[e];
  }
  return p.x_ref[i];
}

// Robots (srbd_robots_f64) override six more constants per robot, not per stage: the mass,
// the body inertia, the friction coefficient and the weights Q, Qf, R.  Kernels and helpers
// that read them take a `bool ROBOT` beside PLAN: false is the code without robots (the values
// are Model::p's, RobotVals is empty), true loads them from the robots' arrays, a NULL array
// falling back to Model::p on a wave-uniform branch.
struct NoRobots {};
template <bool ROBOT>
using RobotArgs = std::conditional_t<ROBOT, srbd_robots_f64, NoRobots>;

// The constants of one robot.  With robots, the mass, L^-1, mu and R are loaded once per
// thread and stay in registers; the 24 weights are read from the robot's rows (96 bytes each,
// cache-resident) where they are used: they would double a lane's live state.
template <bool ROBOT>
struct RobotVals {
  __device__ __forceinline__ double mass(const srbd_model_params& p) const { return p.mass; }
  __device__ __forceinline__ double inv_L(const srbd_model_params& p, int i) const { return 1.0 / p.Lbody[i]; }
  __device__ __forceinline__ double mu(const srbd_model_params& p) const { return p.mu; }
  __device__ __forceinline__ double R(const srbd_model_params& p) const { return p.R; }
  // weight i of the stage cost (k < N) or of the terminal cost
  __device__ __forceinline__ double w(const srbd_model_params& p, bool terminal, int i) const {
    return terminal ? p.Qf[i] : p.Q[i];
  }
};
template <>
struct RobotVals<true> {
  double m, iL[3], mu_, R_;
  const double *Q, *Qf;  // the robot's rows, or NULL
  __device__ __forceinline__ double mass(const srbd_model_params&) const { return m; }
  __device__ __forceinline__ double inv_L(const srbd_model_params&, int i) const { return iL[i]; }
  __device__ __forceinline__ double mu(const srbd_model_params&) const { return mu_; }
  __device__ __forceinline__ double R(const srbd_model_params&) const { return R_; }
  __device__ __forceinline__ double w(const srbd_model_params& p, bool terminal, int i) const {
    if (terminal) return Qf ? Qf[i] : p.Qf[i];
    return Q ? Q[i] : p.Q[i];
  }
};
// rows qp of mass, mu, R ([batch]), Lbody ([batch][3]) and Q, Qf ([batch][12])
template <bool ROBOT>
__device__ __forceinline__ RobotVals<ROBOT> load_robot(const srbd_model_params& p, const RobotArgs<ROBOT>& rb,
                                                       size_t qp) {
  RobotVals<ROBOT> r;
  if constexpr (ROBOT) {
    r.m = rb.mass ? rb.mass[qp] : p.mass;
#pragma unroll
    for (int i = 0; i < 3; ++i) r.iL[i] = 1.0 / (rb.Lbody ? rb.Lbody[qp * 3 + i] : p.Lbody[i]);
    r.mu_ = rb.mu ? rb.mu[qp] : p.mu;
    r.R_ = rb.R ? rb.R[qp] : p.R;
    r.Q = rb.Q ? rb.Q + qp * 12 : nullptr;
    r.Qf = rb.Qf ? rb.Qf + qp * 12 : nullptr;
  }
  return r;
}

struct Model {
  srbd_model_params p;
  // friction coefficient mu: p.mu, or the robot's
  __device__ double ac(int c, int j, double mu) const {
    // friction cone / torque rows of one leg (SRBD_model.cpp:237-260), R_f = I
    const int leg = c / 12, r = c % 12, jj = j - 6 * leg;
    if (jj < 0 || jj >= 6) return 0.0;
    switch (r) {
      case 0: return jj == 0 ? -1.0 : (jj == 2 ? mu : 0.0);
      case 1: return jj == 1 ? -1.0 : (jj == 2 ? mu : 0.0);
      case 2: return jj == 0 ? 1.0 : (jj == 2 ? mu : 0.0);
      case 3: return jj == 1 ? 1.0 : (jj == 2 ? mu : 0.0);
      case 4: return jj == 2 ? -1.0 : 0.0;
      case 5: return jj == 2 ? 1.0 : 0.0;
      case 6: return jj == 2 ? p.Lfx : (jj == 4 ? -1.0 : 0.0);
      case 7: return jj == 2 ? p.Lfx : (jj == 4 ? 1.0 : 0.0);
      case 8: return jj == 2 ? p.Lfz : (jj == 5 ? -1.0 : 0.0);
      case 9: return jj == 2 ? p.Lfz : (jj == 5 ? 1.0 : 0.0);
      case 10: return jj == 3 ? -1.0 : 0.0;
      default: return jj == 3 ? 1.0 : 0.0;
    }
  }
  __device__ double bc(int c) const {
    const int r = c % 12;
    return r == 4 ? p.fmax : (r == 5 ? -p.fmin : 0.0);
  }
  // continuous dynamics f(x, u) (GetContinuousDynamic)
  template <class St, class Rb>
  __device__ void f(const St& s, const Rb& rb, const double* x, const double* u, double* dx) const {
    const V3 r = seg(x, 0), l = seg(x, 3), pos = seg(x, 6);
    const M3 R = expm(r), Jlt = jlt(r);
    const M3 Lb = [&] {
      M3 m = zero3();
      for (int i = 0; i < 3; ++i) m.a[i][i] = rb.inv_L(p, i);  // SetInertia stores L^-1
      return m;
    }();
    const M3 RLR = mul(mul(R, Lb), tr(R));
    const V3 w = mv(RLR, l);
    const V3 dr = mv(Jlt, w);
    const V3 p0{{s.foot_r(p, 0) - pos.v[0], s.foot_r(p, 1) - pos.v[1], s.foot_r(p, 2) - pos.v[2]}};
    const V3 p1{{s.foot_l(p, 0) - pos.v[0], s.foot_l(p, 1) - pos.v[1], s.foot_l(p, 2) - pos.v[2]}};
    const V3 t0 = mv(skew(p0), seg(u, 0)), t1 = mv(skew(p1), seg(u, 6));
    for (int i = 0; i < 3; ++i) {
      dx[i] = dr.v[i];
      dx[3 + i] = u[3 + i] + u[9 + i] + t0.v[i] + t1.v[i];
      dx[6 + i] = x[9 + i];
      dx[9 + i] = (u[i] + u[6 + i]) / rb.mass(p) + (i == 2 ? -9.8 : 0.0);
    }
  }
  // Jacobian blocks of f (the nonzero 3x3 blocks of jfx / jfu, :104-176):
  // jfx[0:3,0:3] = J00, jfx[0:3,3:6] = J01, jfx[3:6,6:9] = [f0 + f1]x,
  // jfx[6:9,9:12] = I; jfu[3:6,0:3] = [p0]x, jfu[3:6,6:9] = [p1]x,
  // jfu[3:6,3:6] = jfu[3:6,9:12] = I, jfu[9:12,0:3] = jfu[9:12,6:9] = I / m
  template <class St, class Rb>
  __device__ void jac_blocks(const St& s, const Rb& rb, const double* x, const double* u, M3& J00, M3& J01,
                             M3& Sf, M3& S0, M3& S1) const {
    const V3 r = seg(x, 0), l = seg(x, 3), pos = seg(x, 6);
    const M3 R = expm(r), Jlt = jlt(r);
    M3 Lb = zero3();
    for (int i = 0; i < 3; ++i) Lb.a[i][i] = rb.inv_L(p, i);
    const M3 RLR = mul(mul(R, Lb), tr(R));
    const V3 w = mv(RLR, l);
    const M3 mid = mul(mul(Jlt, add(mul(RLR, skew(l)), lin(-1.0, skew(w), 0.0, Lb))), jl(r));
    for (int a = 0; a < 3; ++a) {
      const M3 dJ = lin(-1.0, mul(mul(Jlt, djl(r, a)), Jlt), 0.0, Jlt);
      const V3 col = mv(dJ, w);
      for (int i = 0; i < 3; ++i) J00.a[i][a] = col.v[i] + mid.a[i][a];
    }
    J01 = mul(Jlt, RLR);
    Sf = skew(V3{{u[0] + u[6], u[1] + u[7], u[2] + u[8]}});
    S0 = skew(V3{{s.foot_r(p, 0) - pos.v[0], s.foot_r(p, 1) - pos.v[1], s.foot_r(p, 2) - pos.v[2]}});
    S1 = skew(V3{{s.foot_l(p, 0) - pos.v[0], s.foot_l(p, 1) - pos.v[1], s.foot_l(p, 2) - pos.v[2]}});
  }
  // relaxed log barrier (Barrier, :262-295): db, ddb
  __device__ void barrier(double v, double& db, double& ddb) const {
    if (v > p.theta_b) {
      db = -p.mu_b / v;
      ddb = p.mu_b / (v * v);
    } else {
      db = p.mu_b * (v - 2.0 * p.theta_b) / (p.theta_b * p.theta_b);
      ddb = p.mu_b / (p.theta_b * p.theta_b);
    }
  }
};

}  // namespace
}  // namespace srbd
#endif  // SRBD_MODEL_H_
