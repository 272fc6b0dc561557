// srbd_lin_backward.h -- what the two backward passes of the SRBD linearisation share:
// srbd_linearize_backward.hip (from the cotangents of the QP arrays) and
// srbd_solve_backward.hip (from the vectors of the solve and its adjoint).  Both
// fill a per-stage cotangent descriptor in LDS, then one thread per stage runs the reverse model
// on it (stage_reverse) and the robot's sums are formed by srbd_lin_bwd_reduce_kernel.
// Internal: device code, included by those two files only.
#pragma once

#include "../../include/srbd_qp.h"
#include "kernels.h"
#include "srbd_model.h"

#include <type_traits>

namespace srbd {
namespace {

struct LinBwdArgs {
  int batch, N, mode;
  const double *xs, *us;
  const double *gA, *gB, *gb, *gQ, *gR, *gq, *gr, *gubu, *gD, *glg;  // cotangents, NULL = 0
  srbd_lin_grad_f64 out;                                            // NULL = not asked for
  double* part;  // [batch * N][kPart] per-stage parts of the robot sums, or NULL
  double qf_scale;
};
template <bool PLAN, bool ROBOT>
struct LinBwdArgsT : LinBwdArgs, PlanArgs<PLAN>, RobotArgs<ROBOT> {};

constexpr int kBwdThreads = 64;
// the scratch row of a stage: d l / d (1 / mass), d (1 / Lbody[0..2]), d mu, d R
constexpr int kPIm = 0, kPiL = 1, kPMu = 4, kPR = 5, kPart = 6;

// Per-stage cotangent descriptor: what the stage thread needs of cot A, cot B, cot R, cot D, each
// slot a short fixed sum of their elements (the transpose of a_at / b_at / r_at of the forward
// kernel, gathered):
//   J00, J01  <cot A, d A / d J00[i][j]> / dt: one element each
//   P0, P1    <cot B, d [p]x / d p_a>: two elements each (foot_r, foot_l)
//   Im        the trace of cot B's two I / m blocks: six elements
//   Rd        the diagonal of cot R;  Rp: per leg the pairs (0,2) (1,2) (2,4) (2,5), (i,j) + (j,i)
//   D0, D1    CONE: the entries of cot D where D holds mu, per leg: four elements each
constexpr int kGJ00 = 0, kGJ01 = 9, kGP0 = 18, kGP1 = 21, kGIm = 24, kGRd = 25, kGRp = 37, kGD = 45, kGDesc = 47;

__device__ __forceinline__ double dot3(const V3& a, const V3& b) {
  return fma(a.v[0], b.v[0], fma(a.v[1], b.v[1], a.v[2] * b.v[2]));
}
__device__ __forceinline__ V3 cross(const V3& a, const V3& b) {
  return V3{{a.v[1] * b.v[2] - a.v[2] * b.v[1], a.v[2] * b.v[0] - a.v[0] * b.v[2], a.v[0] * b.v[1] - a.v[1] * b.v[0]}};
}
__device__ __forceinline__ V3 colv(const M3& x, int j) { return V3{{x.a[0][j], x.a[1][j], x.a[2][j]}}; }
// x' y
__device__ __forceinline__ V3 tmv(const M3& x, const V3& y) { return mv(tr(x), y); }
// <G, d skew(v) / d v_a>, a = 0..2
__device__ __forceinline__ V3 unskew(const M3& G) {
  return V3{{G.a[2][1] - G.a[1][2], G.a[0][2] - G.a[2][0], G.a[1][0] - G.a[0][1]}};
}

// What one RK4 slope k = f(xp, u) gives back for its cotangent kb (12): the parameter parts
//   giL[j] += d <kb, f> / d (1 / Lbody_j),  kl += kb[3:6] (the feet: p x f is linear in p),
//   gim += d <kb, f> / d (1 / mass)
// and, with `chain`, xb = J_x(xp, u)' kb for the slope before it.  f[0:3] = Jlt R L^-1 R' l:
// with y = Jlt' kb[0:3] and c_j column j of R, d / d iL_j = (c_j . y)(c_j . l), and the transposed
// blocks of Model::jac_blocks are matrix-vector products:
//   J01' v = RLR y,   (J00' v)_a = -y . (djl_a Jlt w) + (Jl' (w x y - l x RLR y))_a.
template <class Rb>
__device__ void slope_reverse(const srbd_model_params& p, const Rb& rb, const double* xp, const V3& F,
                              const double* kb, bool chain, double* giL, V3& kl, double& gim, double* xb) {
  const V3 r = seg(xp, 0), l = seg(xp, 3);
  const M3 R = expm(r), Jlt = jlt(r);
  const V3 y = tmv(Jlt, seg(kb, 0));
  V3 w{{0.0, 0.0, 0.0}}, Ry{{0.0, 0.0, 0.0}};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const V3 c = colv(R, j);
    const double cl = dot3(c, l), cy = dot3(c, y), iL = rb.inv_L(p, j);
    giL[j] = fma(cy, cl, giL[j]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      w.v[i] = fma(iL * cl, c.v[i], w.v[i]);
      Ry.v[i] = fma(iL * cy, c.v[i], Ry.v[i]);
    }
  }
  const V3 kbl = seg(kb, 3), kbv = seg(kb, 9);
#pragma unroll
  for (int i = 0; i < 3; ++i) kl.v[i] += kbl.v[i];
  gim += dot3(F, kbv);
  if (!chain) return;
  const V3 dr = mv(Jlt, w);
  const V3 wy = cross(w, y), lR = cross(l, Ry);
  const V3 My{{wy.v[0] - lR.v[0], wy.v[1] - lR.v[1], wy.v[2] - lR.v[2]}};
  const V3 mid = tmv(jl(r), My);
  const V3 pos = cross(kbl, F);  // [F]x' kb[3:6]
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    xb[a] = mid.v[a] - dot3(y, mv(djl(r, a), dr));
    xb[3 + a] = Ry.v[a];
    xb[6 + a] = pos.v[a];
    xb[9 + a] = kb[6 + a];
  }
}

// The cotangents stage t reads besides its descriptor, each the stage's own row or NULL (zero):
//   gb (12) of b, gr (12) of r, gubu (12) of ubu (BOX_U), lg (24) of lg (CONE) times lg_sign.
// has_A: cot A is there (the descriptor's J00, J01 are read).
struct StageCot {
  const double *gb, *gr, *gubu, *lg;
  double lg_sign;
  bool has_A;
};

// The reverse model of stage t = qp N + k from its descriptor row (LDS, kGDesc doubles, which it
// overwrites) and `c`: foot_r, foot_l, fz_max of the stage are written, and its part of the
// robot's sums goes to the scratch row.
template <bool PLAN, bool ROBOT>
__device__ __forceinline__ void stage_reverse(const Model& m, const LinBwdArgsT<PLAN, ROBOT>& a, long long t,
                                              double* desc_row, const StageCot& c) {
  const srbd_model_params& p = m.p;
  const double dt = p.dt;
  const int N = a.N;
  const int qp = (int)(t / N), k = (int)(t % N);
  const double* g = desc_row;
  const double* x = a.xs + ((size_t)qp * (N + 1) + k) * 12;
  const double* u = a.us + (size_t)t * 12;
  const StageVals<PLAN> sv = load_stage<PLAN>(p, a, (size_t)t);
  const RobotVals<ROBOT> rb = load_robot<ROBOT>(p, a, (size_t)qp);
  const V3 f0 = seg(u, 0), f1 = seg(u, 6);
  const V3 F{{f0.v[0] + f1.v[0], f0.v[1] + f1.v[1], f0.v[2] + f1.v[2]}};
  double giL[3] = {0.0, 0.0, 0.0}, gim = 0.0;
  // ---- B = dt jfu: the [p0]x, [p1]x blocks (p = foot - pos) and the two I / m blocks ----
  V3 gfr{{dt * g[kGP0], dt * g[kGP0 + 1], dt * g[kGP0 + 2]}};
  V3 gfl{{dt * g[kGP1], dt * g[kGP1 + 1], dt * g[kGP1 + 2]}};
  gim = dt * g[kGIm];
  // ---- A = I + dt jfx: J00 and J01 are linear in L^-1 (through RLR, w and mid of jac_blocks).
  // In reverse, with Y = Jlt' G00, G_M = Y Jl', G_w = -Jlt' sum_a djl_a' Y[:, a] - unskew(G_M):
  // G_RLR = Jlt' G01 + G_M [l]x' + G_w l', and d / d iL_j = c_j' G_RLR c_j (c_j column j of R) ----
  if (c.has_A && a.part) {
    const V3 r = seg(x, 0), l = seg(x, 3);
    const M3 R = expm(r), Jlt = jlt(r), Jl = jl(r);
    M3 G00, G01;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        G00.a[i][j] = dt * g[kGJ00 + 3 * i + j];
        G01.a[i][j] = dt * g[kGJ01 + 3 * i + j];
      }
    const M3 JltT = tr(Jlt);
    const M3 Y = mul(JltT, G00);
    const M3 GM = mul(Y, tr(Jl));
    V3 tsum{{0.0, 0.0, 0.0}};
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      const V3 d = tmv(djl(r, cc), colv(Y, cc));
#pragma unroll
      for (int i = 0; i < 3; ++i) tsum.v[i] += d.v[i];
    }
    const V3 jt = mv(JltT, tsum), us_ = unskew(GM);
    const V3 Gw{{-jt.v[0] - us_.v[0], -jt.v[1] - us_.v[1], -jt.v[2] - us_.v[2]}};
    const M3 G1 = mul(JltT, G01);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const V3 cj = colv(R, j);
      // c' G_M [l]x' c = (G_M' c) . (c x l)
      giL[j] += dot3(cj, mv(G1, cj)) + dot3(tmv(GM, cj), cross(cj, l)) + dot3(cj, Gw) * dot3(l, cj);
    }
  }
  // ---- r = R_ u + Ac' db, R = R_ I + Ac' diag(ddb) Ac: the friction barrier.  Only rows 0..4 of
  // a leg's twelve depend on mu (0..3) or fz_max (4). ----
  const double* gr = c.gr;
  double gR = 0.0, gmu = 0.0, gfz[2];
#pragma unroll
  for (int i = 0; i < 12; ++i) gR += g[kGRd + i];
  if (gr) {
#pragma unroll
    for (int i = 0; i < 12; ++i) gR = fma(gr[i], u[i], gR);
  }
  const double mu = rb.mu(p);
#pragma unroll
  for (int leg = 0; leg < 2; ++leg) {
    const int o = 6 * leg;
    const double fx = u[o], fy = u[o + 1], fz = u[o + 2];
    const double r0 = gr ? gr[o] : 0.0, r1 = gr ? gr[o + 1] : 0.0, r2 = gr ? gr[o + 2] : 0.0;
    const double d0 = g[kGRd + o], d1 = g[kGRd + o + 1], d2 = g[kGRd + o + 2];
    const double p02 = g[kGRp + 4 * leg], p12 = g[kGRp + 4 * leg + 1];
    const double* lg = (a.mode == 2 && c.lg) ? c.lg + 12 * leg : nullptr;
    // row c = a_c . u + const with a_c = al e_i + ga e_fz
    const double v[5] = {-fx + mu * fz, -fy + mu * fz, fx + mu * fz, fy + mu * fz, -fz + sv.fz_max(p, leg)};
    const double al[5] = {-1.0, -1.0, 1.0, 1.0, 0.0}, ga[5] = {mu, mu, mu, mu, -1.0};
    const double ri[5] = {r0, r1, r0, r1, 0.0}, di[5] = {d0, d1, d0, d1, 0.0}, pi[5] = {p02, p12, p02, p12, 0.0};
#pragma unroll
    for (int cc = 0; cc < 5; ++cc) {
      double db, ddb;
      m.barrier(v[cc], db, ddb);
      const double d3b = v[cc] > p.theta_b ? -2.0 * p.mu_b / (v[cc] * v[cc] * v[cc]) : 0.0;
      const double s1 = al[cc] * ri[cc] + ga[cc] * r2;
      const double s2 = al[cc] * al[cc] * di[cc] + ga[cc] * ga[cc] * d2 + al[cc] * ga[cc] * pi[cc];
      const double vb = ddb * s1 + d3b * s2 - (lg ? c.lg_sign * lg[cc] : 0.0);
      if (cc < 4)
        gmu += vb * fz + db * r2 + ddb * (al[cc] * pi[cc] + 2.0 * mu * d2);
      else
        gfz[leg] = vb;
    }
    if (a.mode == 2) gmu += g[kGD + leg];
    if constexpr (PLAN) {  // the forward's ubu = min(u_hi[fz], fz_max) - u
      if (a.mode == 1 && c.gubu && sv.fz_max(p, leg) < p.u_hi[o + 2]) gfz[leg] += c.gubu[o + 2];
    }
  }
  // ---- b = x + dt / 6 (k1 + 2 k2 + 2 k3 + k4) - x_next: the RK4 in reverse, the last slope first.
  // The descriptor row has been read: it now holds the points of slopes 2..4 (36 doubles), so that
  // both loops keep one copy of the model and index the points in LDS, not in registers. ----
  if (c.gb) {
    double* pts = desc_row;
    const double* gb = c.gb;
    {
      double xt[12], kk[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) xt[i] = x[i];
#pragma unroll 1
      for (int s = 0; s < 3; ++s) {
        m.f(sv, rb, xt, u, kk);
        const double h = s < 2 ? 0.5 * dt : dt;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          xt[i] = x[i] + h * kk[i];
          pts[12 * s + i] = xt[i];
        }
      }
    }
    double xb[12];
    V3 kl{{0.0, 0.0, 0.0}};
    double bim = 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) xb[i] = 0.0;
#pragma unroll 1
    for (int s = 3; s >= 0; --s) {
      // slope s is f(x + h_s k_(s-1)), h = (0, dt / 2, dt / 2, dt); its weight in b is dt / 6 or dt / 3
      const double wt = (s == 0 || s == 3) ? dt / 6.0 : dt / 3.0;
      const double hn = s == 2 ? dt : (s == 3 ? 0.0 : 0.5 * dt);  // h of the slope after it
      double xp[12], kb[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        xp[i] = s == 0 ? x[i] : pts[12 * (s - 1) + i];
        kb[i] = wt * gb[i] + hn * xb[i];
      }
      slope_reverse(p, rb, xp, F, kb, s > 0, giL, kl, bim, xb);
    }
    gim += bim;
    // <kb[3:6], p x f> = p . (f x kb[3:6])
    const V3 cr = cross(f0, kl), cl = cross(f1, kl);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      gfr.v[i] += cr.v[i];
      gfl.v[i] += cl.v[i];
    }
  }
  if (a.out.foot_r) {
#pragma unroll
    for (int i = 0; i < 3; ++i) a.out.foot_r[(size_t)t * 3 + i] = gfr.v[i];
  }
  if (a.out.foot_l) {
#pragma unroll
    for (int i = 0; i < 3; ++i) a.out.foot_l[(size_t)t * 3 + i] = gfl.v[i];
  }
  if (a.out.fz_max) {
    a.out.fz_max[(size_t)t * 2] = gfz[0];
    a.out.fz_max[(size_t)t * 2 + 1] = gfz[1];
  }
  if (a.part) {
    double* pr = a.part + (size_t)t * kPart;
    pr[kPIm] = gim;
#pragma unroll
    for (int i = 0; i < 3; ++i) pr[kPiL + i] = giL[i];
    pr[kPMu] = gmu;
    pr[kPR] = gR;
  }
}

// One thread per (robot, entry of the scratch row): the sum over the robot's stages, in stage
// order, and the chain rule from 1 / mass and 1 / Lbody to mass and Lbody.
template <bool ROBOT>
__global__ void __launch_bounds__(256) srbd_lin_bwd_reduce_kernel(Model m, LinBwdArgsT<false, ROBOT> a) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)a.batch * kPart) return;
  const int qp = (int)(gid / kPart), c = (int)(gid % kPart);
  const double* pr = a.part + (size_t)qp * a.N * kPart + c;
  double s = 0.0;
  for (int k = 0; k < a.N; ++k) s += pr[(size_t)k * kPart];
  const srbd_model_params& p = m.p;
  if (c == kPIm) {
    if (!a.out.mass) return;
    double mass = p.mass;
    if constexpr (ROBOT) mass = a.mass ? a.mass[qp] : p.mass;
    a.out.mass[qp] = -s / (mass * mass);
  } else if (c < kPMu) {
    if (!a.out.Lbody) return;
    const int j = c - kPiL;
    double L = p.Lbody[j];
    if constexpr (ROBOT) L = a.Lbody ? a.Lbody[(size_t)qp * 3 + j] : p.Lbody[j];
    a.out.Lbody[(size_t)qp * 3 + j] = -s / (L * L);
  } else if (c == kPMu) {
    if (a.out.mu) a.out.mu[qp] = s;
  } else {
    if (a.out.R) a.out.R[qp] = s;
  }
}

// as srbd_linearize.hip: the PLAN kernels run only when the plan overrides something, the ROBOT
// kernels only when the MODEL role does
inline bool plan_given(const srbd_plan_f64* plan) {
  return plan && (plan->x_ref || plan->foot_r || plan->foot_l || plan->fz_max);
}
inline bool robots_given(const srbd_robots_f64* rb) {
  return rb && (rb->mass || rb->Lbody || rb->mu || rb->Q || rb->Qf || rb->R);
}
template <bool PLAN, bool ROBOT>
LinBwdArgsT<PLAN, ROBOT> full_args(const LinBwdArgs& a, const srbd_plan_f64* plan, const srbd_robots_f64* robots) {
  LinBwdArgsT<PLAN, ROBOT> full;
  static_cast<LinBwdArgs&>(full) = a;
  if constexpr (PLAN) static_cast<srbd_plan_f64&>(full) = *plan;
  if constexpr (ROBOT) static_cast<srbd_robots_f64&>(full) = *robots;
  return full;
}
template <class Fn>
void dispatch(bool plan, bool robot, Fn&& fn) {
  if (plan && robot) fn(std::true_type{}, std::true_type{});
  else if (plan) fn(std::true_type{}, std::false_type{});
  else if (robot) fn(std::false_type{}, std::true_type{});
  else fn(std::false_type{}, std::false_type{});
}

}  // namespace
}  // namespace srbd
