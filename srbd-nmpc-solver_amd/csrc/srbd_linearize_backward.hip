// srbd_linearize_backward.hip -- the backward pass of the batched SRBD linearisation
// (srbd_qp_srbd_linearize_backward_f64): from the cotangents of the QP arrays
// srbd_linearize.hip writes (what the QP's backward pass returns) to the gradients of what a
// caller sets per robot (srbd_robots_f64) and per robot and stage (srbd_plan_f64).  The
// linearisation point xs, us is held fixed.
//   srbd_lin_bwd_stage_kernel  one thread per (QP, stage k < N), the forward kernel's shape.  The
//       wave first folds the cotangents of A, B, R (and D) of its 64 stages, one contiguous run
//       of HBM read as whole lines, into a per-stage cotangent descriptor in LDS: the transpose
//       of a_at / b_at / r_at.  The stage thread then reverses model -> descriptor from
//       registers: foot_r, foot_l, fz_max of its stage are written, and its part of the robot's
//       sums (1 / mass, 1 / Lbody, mu, R) goes to a scratch row.
//   srbd_lin_bwd_reduce_kernel the robot's sums over its stages in stage order (no atomics: the
//       same bits from call to call, also where a robot's stages straddle workgroups), and
//       1 / mass -> mass, 1 / Lbody -> Lbody.
//   srbd_lin_bwd_cost_kernel   Q, Qf, x_ref from the diagonals of cot Q and from cot q.
// The host statement that pins it is tests/linearize_vjp_host.py.
#include "../../include/srbd_qp.h"
#include "kernels.h"
#include "srbd_model.h"

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
// stages of one array staged in LDS at a time (blocks of 144 doubles)
constexpr int kChunk = 8;

__device__ __forceinline__ double2 ld_nt(const double2* p) {
  typedef double dv2 __attribute__((ext_vector_type(2)));
  const dv2 v = __builtin_nontemporal_load(reinterpret_cast<const dv2*>(p));
  return make_double2(v.x, v.y);
}

// element (i, j) of a column-major 12 x 12 block
__device__ __forceinline__ double el(const double* blk, int i, int j) { return blk[j * 12 + i]; }

struct GatherA {
  static constexpr int kSlots = 18, kSlot0 = kGJ00, kBlocks = 1;
  __device__ static double at(const double* blk, int, int s) {
    const int top = s < 9 ? 0 : 3, e = s < 9 ? s : s - 9;
    return el(blk, e / 3, top + e % 3);
  }
};
struct GatherB {
  static constexpr int kSlots = 7, kSlot0 = kGP0, kBlocks = 1;
  __device__ static double at(const double* blk, int, int s) {
    if (s == 6) {
      double tr = 0.0;
      for (int i = 0; i < 3; ++i) tr += el(blk, 9 + i, i) + el(blk, 9 + i, 6 + i);
      return tr;
    }
    // skew(p)[r][c] = -p_a where c - r = 1 (mod 3), +p_a the other way round, a = 3 - r - c
    const int cb = s < 3 ? 0 : 6, a = s < 3 ? s : s - 3;
    const int r1 = (a + 1) % 3, c1 = (a + 2) % 3;
    return el(blk, 3 + c1, cb + r1) - el(blk, 3 + r1, cb + c1);
  }
};
struct GatherR {
  static constexpr int kSlots = 20, kSlot0 = kGRd, kBlocks = 1;
  __device__ static double at(const double* blk, int, int s) {
    if (s < 12) return el(blk, s, s);
    const int leg = (s - 12) / 4, pr = (s - 12) % 4, o = 6 * leg;
    const int lo = pr < 2 ? pr : 2, hi = pr < 2 ? 2 : pr + 2;
    return el(blk, o + lo, o + hi) + el(blk, o + hi, o + lo);
  }
};
// D is 24 x 12 column-major, two blocks of 144: leg 0's mu sit in column 2, rows 0..3 (block 0,
// elements 48..51), leg 1's in column 8, rows 12..15 (block 1, elements 60..63)
struct GatherD {
  static constexpr int kSlots = 1, kSlot0 = kGD, kBlocks = 2;
  __device__ static double at(const double* blk, int half, int) {
    const double* e = blk + (half == 0 ? 48 : 60);
    return (e[0] + e[1]) + (e[2] + e[3]);
  }
};

// The wave folds array X of the workgroup's nst stages into the descriptors: kChunk blocks of
// 1152 bytes at a time, 16 bytes per lane at consecutive addresses into LDS, then one descriptor
// slot per lane.  X == NULL: the slots are zero.
template <class G>
__device__ __forceinline__ void fold(const double* X, long long t0, int nst, double* desc, double2* stg) {
  const int nblk = nst * G::kBlocks;
  if (!X) {
    for (int it = threadIdx.x; it < nblk * G::kSlots; it += kBwdThreads) {
      const int blk = it / G::kSlots, s = it - blk * G::kSlots;
      desc[(blk / G::kBlocks) * kGDesc + G::kSlot0 + (blk % G::kBlocks) * G::kSlots + s] = 0.0;
    }
    return;
  }
  const double2* X2 = reinterpret_cast<const double2*>(X + t0 * (144 * G::kBlocks));
  constexpr int kPer = kChunk * 72 / kBwdThreads;  // double2 per lane and chunk
  for (int c0 = 0; c0 < nblk; c0 += kChunk) {
    const int nb = nblk - c0 < kChunk ? nblk - c0 : kChunk;
    double2 tmp[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int v = i * kBwdThreads + threadIdx.x;
      tmp[i] = v < nb * 72 ? ld_nt(&X2[(size_t)c0 * 72 + v]) : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i) stg[i * kBwdThreads + threadIdx.x] = tmp[i];
    __syncthreads();
    const double* sd = reinterpret_cast<const double*>(stg);
    for (int it = threadIdx.x; it < nb * G::kSlots; it += kBwdThreads) {
      const int b = it / G::kSlots, s = it - b * G::kSlots, blk = c0 + b;
      desc[(blk / G::kBlocks) * kGDesc + G::kSlot0 + (blk % G::kBlocks) * G::kSlots + s] =
          G::at(sd + b * 144, blk % G::kBlocks, s);
    }
    __syncthreads();
  }
}

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

template <bool PLAN, bool ROBOT>
__global__ void __launch_bounds__(kBwdThreads) srbd_lin_bwd_stage_kernel(Model m, LinBwdArgsT<PLAN, ROBOT> a) {
  __shared__ double desc[kBwdThreads * kGDesc];
  __shared__ double2 stg[kChunk * 72];
  const int N = a.N;
  const long long nst_all = (long long)a.batch * N;
  const long long t0 = (long long)blockIdx.x * kBwdThreads;
  const long long left = nst_all - t0;
  const int nst = left < kBwdThreads ? (int)left : kBwdThreads;
  fold<GatherA>(a.gA, t0, nst, desc, stg);
  fold<GatherB>(a.gB, t0, nst, desc, stg);
  fold<GatherR>(a.gR, t0, nst, desc, stg);
  if (a.mode == 2) fold<GatherD>(a.gD, t0, nst, desc, stg);
  __syncthreads();
  const long long t = t0 + threadIdx.x;
  if (t >= nst_all) return;
  const srbd_model_params& p = m.p;
  const double dt = p.dt;
  const int qp = (int)(t / N), k = (int)(t % N);
  const double* g = desc + threadIdx.x * kGDesc;
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
  if (a.gA && a.part) {
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
    for (int c = 0; c < 3; ++c) {
      const V3 d = tmv(djl(r, c), colv(Y, c));
#pragma unroll
      for (int i = 0; i < 3; ++i) tsum.v[i] += d.v[i];
    }
    const V3 jt = mv(JltT, tsum), us_ = unskew(GM);
    const V3 Gw{{-jt.v[0] - us_.v[0], -jt.v[1] - us_.v[1], -jt.v[2] - us_.v[2]}};
    const M3 G1 = mul(JltT, G01);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const V3 c = colv(R, j);
      // c' G_M [l]x' c = (G_M' c) . (c x l)
      giL[j] += dot3(c, mv(G1, c)) + dot3(tmv(GM, c), cross(c, l)) + dot3(c, Gw) * dot3(l, c);
    }
  }
  // ---- r = R_ u + Ac' db, R = R_ I + Ac' diag(ddb) Ac: the friction barrier.  Only rows 0..4 of
  // a leg's twelve depend on mu (0..3) or fz_max (4). ----
  const double* gr = a.gr ? a.gr + (size_t)t * 12 : nullptr;
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
    const double* lg = (a.mode == 2 && a.glg) ? a.glg + ((size_t)qp * (N + 1) + k) * 24 + 12 * leg : nullptr;
    // row c = a_c . u + const with a_c = al e_i + ga e_fz
    const double v[5] = {-fx + mu * fz, -fy + mu * fz, fx + mu * fz, fy + mu * fz, -fz + sv.fz_max(p, leg)};
    const double al[5] = {-1.0, -1.0, 1.0, 1.0, 0.0}, ga[5] = {mu, mu, mu, mu, -1.0};
    const double ri[5] = {r0, r1, r0, r1, 0.0}, di[5] = {d0, d1, d0, d1, 0.0}, pi[5] = {p02, p12, p02, p12, 0.0};
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      double db, ddb;
      m.barrier(v[c], db, ddb);
      const double d3b = v[c] > p.theta_b ? -2.0 * p.mu_b / (v[c] * v[c] * v[c]) : 0.0;
      const double s1 = al[c] * ri[c] + ga[c] * r2;
      const double s2 = al[c] * al[c] * di[c] + ga[c] * ga[c] * d2 + al[c] * ga[c] * pi[c];
      const double vb = ddb * s1 + d3b * s2 - (lg ? lg[c] : 0.0);
      if (c < 4)
        gmu += vb * fz + db * r2 + ddb * (al[c] * pi[c] + 2.0 * mu * d2);
      else
        gfz[leg] = vb;
    }
    if (a.mode == 2) gmu += g[kGD + leg];
    if constexpr (PLAN) {  // the forward's ubu = min(u_hi[fz], fz_max) - u
      if (a.mode == 1 && a.gubu && sv.fz_max(p, leg) < p.u_hi[o + 2]) gfz[leg] += a.gubu[(size_t)t * 12 + o + 2];
    }
  }
  // ---- b = x + dt / 6 (k1 + 2 k2 + 2 k3 + k4) - x_next: the RK4 in reverse, the last slope first.
  // The descriptor row has been read: it now holds the points of slopes 2..4 (36 doubles), so that
  // both loops keep one copy of the model and index the points in LDS, not in registers. ----
  if (a.gb) {
    double* pts = desc + threadIdx.x * kGDesc;
    const double* gb = a.gb + (size_t)t * 12;
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

// One thread per (robot, j < 12): Q = diag(w), q = diag(w) (x - x_ref) on every stage k <= N
// (srbd_lin_cost_kernel), so x_ref's gradient is element-wise in cot q and Q's, Qf's are sums of
// cot Q's diagonal and cot q (x - x_ref) over the stages, in stage order.
template <bool PLAN, bool ROBOT>
__global__ void __launch_bounds__(256) srbd_lin_bwd_cost_kernel(Model m, LinBwdArgsT<PLAN, ROBOT> a) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)a.batch * 12) return;
  const srbd_model_params& p = m.p;
  const int qp = (int)(gid / 12), j = (int)(gid % 12), N = a.N;
  double wQ = p.Q[j], wQf = p.Qf[j];
  if constexpr (ROBOT) {
    if (a.Q) wQ = a.Q[(size_t)qp * 12 + j];
    if (a.Qf) wQf = a.Qf[(size_t)qp * 12 + j];
  }
  double sQ = 0.0;
  for (int k = 0; k <= N; ++k) {
    const size_t blk = (size_t)qp * (N + 1) + k, e = blk * 12 + j;
    const double gq = a.gq ? a.gq[e] : 0.0;
    const double gQ = a.gQ ? a.gQ[blk * 144 + 13 * j] : 0.0;
    const double w = k < N ? wQ : a.qf_scale * wQf;
    if (a.out.x_ref) a.out.x_ref[e] = -w * gq;
    const double term = gQ + gq * (a.xs[e] - x_ref_at<PLAN>(p, a, e, j));
    if (k < N)
      sQ += term;
    else if (a.out.Qf)
      a.out.Qf[(size_t)qp * 12 + j] = a.qf_scale * term;
  }
  if (a.out.Q) a.out.Q[(size_t)qp * 12 + j] = sQ;
}

// as srbd_linearize.hip: the PLAN kernels run only when the plan overrides something, the ROBOT
// kernels only when the MODEL role does
bool plan_given(const srbd_plan_f64* plan) {
  return plan && (plan->x_ref || plan->foot_r || plan->foot_l || plan->fz_max);
}
bool robots_given(const srbd_robots_f64* rb) {
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

size_t lin_backward_part_elems(int batch, int N) { return (size_t)batch * (size_t)N * kPart; }

hipError_t launch_srbd_linearize_backward(const srbd_model_params& p, int batch, int N, int mode,
                                          const double* xs, const double* us, const srbd_qp_data_f64& cot,
                                          const srbd_lin_grad_f64& grad, double* part, hipStream_t stream,
                                          const srbd_plan_f64* plan, const srbd_robots_f64* robots) {
  if (batch <= 0) return hipSuccess;
  Model m{p};
  LinBwdArgs a{};
  a.batch = batch;
  a.N = N;
  a.mode = mode;
  a.xs = xs;
  a.us = us;
  a.gA = cot.A;
  a.gB = cot.B;
  a.gb = cot.b;
  a.gQ = cot.Q;
  a.gR = cot.R;
  a.gq = cot.q;
  a.gr = cot.r;
  a.gubu = mode == 1 ? cot.ubu : nullptr;
  a.gD = mode == 2 ? cot.D : nullptr;
  a.glg = mode == 2 ? cot.lg : nullptr;
  a.out = grad;
  const bool sums = grad.mass || grad.Lbody || grad.mu || grad.R;
  a.part = sums ? part : nullptr;
  a.qf_scale = p.qf_scale;
  const bool stage = sums || grad.foot_r || grad.foot_l || grad.fz_max;
  const bool cost = grad.Q || grad.Qf || grad.x_ref;
  const long long nst = (long long)batch * N;
  dispatch(plan_given(plan), robots_given(robots), [&](auto PL, auto RB) {
    constexpr bool kP = decltype(PL)::value, kR = decltype(RB)::value;
    const auto full = full_args<kP, kR>(a, plan, robots);
    if (stage)
      hipLaunchKernelGGL((srbd_lin_bwd_stage_kernel<kP, kR>), dim3((unsigned)((nst + kBwdThreads - 1) / kBwdThreads)),
                         dim3(kBwdThreads), 0, stream, m, full);
    if (sums)
      hipLaunchKernelGGL((srbd_lin_bwd_reduce_kernel<kR>), dim3((unsigned)(((long long)batch * kPart + 255) / 256)),
                         dim3(256), 0, stream, m, full_args<false, kR>(a, plan, robots));
    if (cost)
      hipLaunchKernelGGL((srbd_lin_bwd_cost_kernel<kP, kR>), dim3((unsigned)(((long long)batch * 12 + 255) / 256)),
                         dim3(256), 0, stream, m, full);
  });
  return hipGetLastError();
}

}  // namespace srbd
