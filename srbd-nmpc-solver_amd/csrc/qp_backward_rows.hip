// qp_backward_rows.hip -- the backward pass with general rows on the inputs:
// the projection kernel that writes the stages the adjoint QP is solved on, and the lift kernel
// that turns the adjoint solution into the gradients of D, lg, ug, lbu and ubu.
//
// E_k holds the active rows of stage k: a unit row for every pinned input (qp_backward.hip's
// rule), then row j of D_k for every active general row (unmasked and D_j u - lg_j < act_tol or
// ug_j - D_j u < act_tol; the nearer bound is the active one, the lower on a tie).  The rows are
// taken in that order by modified Gram-Schmidt, E' = Y T with Y orthonormal and T upper
// triangular; a general row is restricted to the unpinned coordinates first, and it is accepted
// iff what is left of it after the rows accepted so far exceeds rank_tol times its own norm and
// fewer than nu rows are accepted.  A row that is not accepted is dropped: nu = dnu = 0.
//
// The adjoint QP with E du = 0 is the unconstrained adjoint on the stages
//   B~ = B P    S~ = P S    R~ = P R P + (I - P)    r~ = P gu        P = I - Y Y' (= Z Z')
// which is  Qf diag(Z'(.)Z, I) Qf'  of the rotated form with Qf = [Z Y]: the Y part is cleared
// and gets the identity, so du = Z w comes out of the solve in the caller's coordinates.  A pin
// is the case Y = e_i, where P is diagonal and the products are the mask kernel's clearing; a
// stage without an accepted general row therefore takes the mask path (cleared entries, no
// products; a plain copy if nothing is pinned), bit for bit what backward_mask_kernel writes.
// The multipliers follow from stationarity, rho + E' nu = 0:
//   rho  = R u  + S x  + r  + B' pi+     nu  = -T^-1 Y' rho
//   rho~ = R du + S dx + gu + B' dpi+    dnu = -T^-1 Y' rho~
// and  grad D_j = dnu_j u' + nu_j du',  grad lg_j or ug_j = -dnu_j (the active side), the same
// for lbu_i / ubu_i of a pin; every entry of an inactive or dropped row is exactly 0.
//
// Shape: the project's 16-lane row owns a stage, one lane per coordinate, dot products by row
// reductions; a workgroup is 8 such rows, and what the rows find (Y, T or P, the flags) lives in
// LDS, so that the streaming part that follows is shaped over the arrays like the mask kernel's:
// 16-byte pieces, consecutive threads on consecutive pieces.  D is read where it is (ng = 64 is
// 6 KB per stage: eight stages of it would not leave room for anything else), row-parallel for
// D u (lane t takes rows t, t + 16, ...: consecutive lanes, consecutive addresses) and one row
// at a time for the few active ones.  The factor is a function of the inputs alone and the lift
// kernel forms it again, so no factor is stored between the two.
#include "qp_backward_rows.h"

#include <cstdint>
#include <initializer_list>

namespace srbd {
namespace {

constexpr int kThreads = 128;
constexpr int kLanes = 16;                   // a stage's row of lanes
constexpr int kStages = kThreads / kLanes;   // stages per workgroup
constexpr int kMaxG = 64;                    // ng <= 64 (srbd_qp_create)

// What a row of lanes finds about its stage.  pin / act: 0 inactive, 1 the lower bound, 2 the
// upper one.  In the projection kernel, which has no use for T, T becomes P and then Y becomes R P.
struct Stage {
  double Y[12][12];  // Y[m][c]: accepted row m, orthonormal
  double T[12][12];  // T[m][n], m <= n: E'_n = sum_m Y_m T[m][n]
  double u[12];
  unsigned char pin[12];
  unsigned char act[kMaxG];
  int nacc, npin, nrow, ndrop;
};
struct Factor {
  int nacc, npin, nrow, ndrop;
  int src;  // lane m < nacc: what slot m is -- row j of D, or -1 - c for the pin of input c
};

__device__ __forceinline__ double sum16(double v) {
  for (int off = kLanes / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kLanes);
  return v;
}
// 1 the lower bound is the active one, 2 the upper, 0 neither
__device__ __forceinline__ unsigned char active_side(double dl, double dh, bool lm, bool um, double tol) {
  const bool lo = lm && dl < tol, hi = um && dh < tol;
  if (!lo && !hi) return 0;
  return lo && (!hi || dl <= dh) ? 1 : 2;
}

// The active set and factorisation of stage `blk` = qp N + k by its row of lanes.  Every thread
// of the workgroup calls this (it synchronises); !valid: a stage past the end, found empty.
__device__ __forceinline__ Factor factor_stage(const BackwardRowsArgs& a, Stage& st, long long blk, bool valid,
                                               int lane) {
  const int nu = a.nu, ng = a.ng;
  for (int e = lane; e < 144; e += kLanes) (&st.Y[0][0])[e] = 0.0, (&st.T[0][0])[e] = 0.0;
  if (lane < 12) {
    double u = 0.0;
    unsigned char p = 0;
    if (valid && lane < nu) {
      const long long at = blk * nu + lane;
      u = a.u[at];
      if (a.lbu)
        p = active_side(u - a.lbu[at], a.ubu[at] - u, !a.lbu_mask || a.lbu_mask[at] != 0.0,
                        !a.ubu_mask || a.ubu_mask[at] != 0.0, a.act_tol);
    }
    st.u[lane] = u;
    st.pin[lane] = p;
  }
  __syncthreads();
  const double* D = a.D + (valid ? blk * ng * nu : 0);
  const long long row0 = valid ? (blk + blk / a.N) * ng : 0;  // lg, ug: N + 1 rows per QP
  for (int j = lane; j < kMaxG; j += kLanes) {
    unsigned char s = 0;
    if (valid && j < ng) {
      double g = 0.0;
      for (int c = 0; c < nu; ++c) g += D[j + ng * c] * st.u[c];
      s = active_side(g - a.lg[row0 + j], a.ug[row0 + j] - g, !a.lg_mask || a.lg_mask[row0 + j] != 0.0,
                      !a.ug_mask || a.ug_mask[row0 + j] != 0.0, a.act_tol);
    }
    st.act[j] = s;
  }
  __syncthreads();
  // From here on the rows of lanes of a wave go their own ways: lanes talk by sum16 alone, and a
  // lane reads back from LDS only what it wrote itself.
  Factor f{0, 0, 0, 0, 0};
  int slot = 0;  // a pinned lane's slot
  for (int c = 0; c < nu; ++c) {
    if (!st.pin[c]) continue;
    if (lane == c) st.Y[f.nacc][c] = 1.0, st.T[f.nacc][f.nacc] = 1.0, slot = f.nacc;
    if (lane == f.nacc) f.src = -1 - c;
    ++f.nacc;
  }
  f.npin = f.nacc;
  const bool free_lane = lane < nu && !st.pin[lane < 12 ? lane : 0];
  const bool pin_lane = lane < nu && !free_lane;
  for (int j = 0; j < ng; ++j) {
    if (!st.act[j]) continue;
    if (f.nacc >= nu) {  // no coordinate is left (and no slot: T has 12 columns)
      ++f.ndrop;
      continue;
    }
    const double d = lane < nu ? D[j + ng * lane] : 0.0;
    double v = free_lane ? d : 0.0;
    const double own = sqrt(sum16(v * v));
    for (int m = f.npin; m < f.nacc; ++m) {
      const double y = lane < 12 ? st.Y[m][lane] : 0.0;
      const double t = sum16(y * v);
      v -= t * y;
      if (lane == 12) st.T[m][f.nacc] = t;
    }
    const double left = sqrt(sum16(v * v));
    if (left > a.rank_tol * own) {
      if (lane < 12) st.Y[f.nacc][lane] = v / left;
      if (lane == 12) st.T[f.nacc][f.nacc] = left;
      if (pin_lane) st.T[slot][f.nacc] = d;  // the row's pinned coordinates
      if (lane == f.nacc) f.src = j;
      ++f.nacc, ++f.nrow;
    } else {
      ++f.ndrop;
    }
  }
  if (lane == 0) st.nacc = f.nacc, st.npin = f.npin, st.nrow = f.nrow, st.ndrop = f.ndrop;
  __syncthreads();
  return f;
}

// ---------------------------------------------------------------------------
// projection kernel
// ---------------------------------------------------------------------------
// kVec: nx = nu = 12 and every pointer 16-byte aligned; otherwise one element per thread with
// bounds from nx, nu on the caller's arrays.
template <bool kVec>
__global__ void __launch_bounds__(kThreads) backward_project_kernel(BackwardRowsArgs a) {
  __shared__ __attribute__((aligned(16))) Stage sst[kStages];
  const int tid = threadIdx.x, lane = tid & (kLanes - 1), ls = tid / kLanes;
  const int nx = a.nx, nu = a.nu;
  const long long nblk = (long long)a.batch * a.N;
  const long long blk0 = (long long)blockIdx.x * kStages;
  if (blk0 >= nblk) return;  // (the whole workgroup)
  const int nb = nblk - blk0 < kStages ? (int)(nblk - blk0) : kStages;
  const bool valid = ls < nb;
  Stage& st = sst[ls];
  const Factor f = factor_stage(a, st, blk0 + ls, valid, lane);
  if (valid && lane == 0 && a.count) {
    int* cnt = a.count + (blk0 + ls) / a.N * 3;
    if (f.npin) atomicAdd(cnt, f.npin);
    if (f.nrow) atomicAdd(cnt + 1, f.nrow);
    if (f.ndrop) atomicAdd(cnt + 2, f.ndrop);
  }
  // a stage with an accepted general row: P = I - Y Y' (into T), then W = R P (into Y)
  if (f.nrow > 0) {
    for (int e = lane; e < 144; e += kLanes) {
      const int i = e / 12, j = e - 12 * i;
      double p = i == j ? 1.0 : 0.0;
      for (int m = 0; m < f.nacc; ++m) p -= st.Y[m][i] * st.Y[m][j];
      st.T[i][j] = p;
    }
  }
  __syncthreads();
  if (f.nrow > 0) {
    const double* R = a.R + (blk0 + ls) * nu * nu;
    for (int e = lane; e < 144; e += kLanes) {
      const int c = e / 12, b = e - 12 * c;  // (R P)[b][c], consecutive lanes on consecutive rows b
      double w = 0.0;
      if (b < nu && c < nu)
        for (int k = 0; k < nu; ++k) w += R[b + nu * k] * st.T[k][c];
      st.Y[c][b] = w;  // (Y has done its work: W[c][b] = (R P)[b][c] takes its place)
    }
  }
  __syncthreads();
  if constexpr (kVec) {
    const double2* B = reinterpret_cast<const double2*>(a.B + blk0 * 144);
    const double2* S = reinterpret_cast<const double2*>(a.S + blk0 * 144);
    const double2* R = reinterpret_cast<const double2*>(a.R + blk0 * 144);
    double2* Bm = reinterpret_cast<double2*>(a.Bm + blk0 * 144);
    double2* Sm = reinterpret_cast<double2*>(a.Sm + blk0 * 144);
    double2* Rm = reinterpret_cast<double2*>(a.Rm + blk0 * 144);
    for (int l = tid; l < nb * 72; l += kThreads) {  // piece l: rows i, i + 1 of column j
      const int lb = l / 72, pc = l - lb * 72, e = 2 * pc, j = e / 12, i = e - 12 * j;
      const Stage& s = sst[lb];
      if (s.nrow == 0) {  // the mask kernel's piece
        const int pj = s.pin[j], p0 = s.pin[i], p1 = s.pin[i + 1];
        double2 bv = B[l];
        if (pj) bv.x = bv.y = 0.0;
        Bm[l] = bv;
        double2 sv = S[l];
        if (p0) sv.x = 0.0;
        if (p1) sv.y = 0.0;
        Sm[l] = sv;
        double2 rv = R[l];
        if (pj || p0) rv.x = i == j ? 1.0 : 0.0;
        if (pj || p1) rv.y = i + 1 == j ? 1.0 : 0.0;
        Rm[l] = rv;
        continue;
      }
      double b0 = 0.0, b1 = 0.0, s0 = 0.0, s1 = 0.0, r0 = 0.0, r1 = 0.0;
#pragma unroll 4
      for (int k = 0; k < 12; ++k) {
        const double2 bk = B[lb * 72 + (i + 12 * k) / 2];  // rows i, i + 1 of column k of B
        const double pkj = s.T[k][j], pik = s.T[i][k], pjk = s.T[i + 1][k];
        b0 += bk.x * pkj, b1 += bk.y * pkj;
        const double skj = a.S[(blk0 + lb) * 144 + k + 12 * j];  // (S)[k][j]
        s0 += pik * skj, s1 += pjk * skj;
        const double wkj = s.Y[j][k];
        r0 += pik * wkj, r1 += pjk * wkj;
      }
      r0 += (i == j ? 1.0 : 0.0) - s.T[i][j];
      r1 += (i + 1 == j ? 1.0 : 0.0) - s.T[i + 1][j];
      Bm[l] = make_double2(b0, b1), Sm[l] = make_double2(s0, s1), Rm[l] = make_double2(r0, r1);
    }
    const double2* gu = a.gu ? reinterpret_cast<const double2*>(a.gu + blk0 * 12) : nullptr;
    double2* rm = reinterpret_cast<double2*>(a.rm + blk0 * 12);
    for (int l = tid; l < nb * 6; l += kThreads) {
      const int lb = l / 6, i = 2 * (l - lb * 6);
      const Stage& s = sst[lb];
      double v0 = 0.0, v1 = 0.0;
      if (gu) {
        const double2 g2 = gu[l];
        v0 = g2.x, v1 = g2.y;
      }
      if (s.nrow == 0) {
        if (s.pin[i]) v0 = 0.0;
        if (s.pin[i + 1]) v1 = 0.0;
      } else if (gu) {
        v0 = v1 = 0.0;
        for (int k = 0; k < 12; ++k) {
          const double gk = a.gu[(blk0 + lb) * 12 + k];
          v0 += s.T[i][k] * gk, v1 += s.T[i + 1][k] * gk;
        }
      }
      rm[l] = make_double2(v0, v1);
    }
  } else {
    // element (i, j) of a rows x cols column-major block
    for (int which = 0; which < 3; ++which) {
      const int rows = which == 0 ? nx : nu, cols = which == 1 ? nx : nu, per = rows * cols;
      const double* src = which == 0 ? a.B : which == 1 ? a.S : a.R;
      double* dst = which == 0 ? a.Bm : which == 1 ? a.Sm : a.Rm;
      for (int l = tid; l < nb * per; l += kThreads) {
        const int lb = l / per, e = l - lb * per, j = e / rows, i = e - rows * j;
        const Stage& s = sst[lb];
        const double* blk = src + (blk0 + lb) * per;
        double v;
        if (s.nrow == 0) {
          if (which == 0) v = s.pin[j] ? 0.0 : blk[e];
          else if (which == 1) v = s.pin[i] ? 0.0 : blk[e];
          else v = s.pin[i] || s.pin[j] ? (i == j ? 1.0 : 0.0) : blk[e];
        } else {
          v = 0.0;
          if (which == 0)
            for (int k = 0; k < nu; ++k) v += blk[i + nx * k] * s.T[k][j];
          else if (which == 1)
            for (int k = 0; k < nu; ++k) v += s.T[i][k] * blk[k + nu * j];
          else {
            for (int k = 0; k < nu; ++k) v += s.T[i][k] * s.Y[j][k];
            v += (i == j ? 1.0 : 0.0) - s.T[i][j];
          }
        }
        dst[(blk0 + lb) * per + e] = v;
      }
    }
    for (int l = tid; l < nb * nu; l += kThreads) {
      const int lb = l / nu, i = l - lb * nu;
      const Stage& s = sst[lb];
      const double* gu = a.gu ? a.gu + (blk0 + lb) * nu : nullptr;
      double v = gu ? gu[i] : 0.0;
      if (s.nrow == 0) {
        if (s.pin[i]) v = 0.0;
      } else if (gu) {
        v = 0.0;
        for (int k = 0; k < nu; ++k) v += s.T[i][k] * gu[k];
      }
      a.rm[(blk0 + lb) * nu + i] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// lift kernel
// ---------------------------------------------------------------------------
// kVec: grad D as 16-byte pieces (ng even, the pointer aligned).  Everything else this kernel
// touches is bounds-checked on nx, nu, ng and goes element by element.
constexpr int kX = 0, kDx = 12, kU = 24, kDu = 36, kPip = 48, kDpip = 60;  // a stage's vectors
template <bool kVec>
__global__ void __launch_bounds__(kThreads) backward_lift_kernel(BackwardRowsArgs a) {
  __shared__ __attribute__((aligned(16))) Stage sst[kStages];
  __shared__ __attribute__((aligned(16))) double sv[kStages][72];
  __shared__ __attribute__((aligned(16))) double snu[kStages][kMaxG], sdnu[kStages][kMaxG];  // per row of D
  __shared__ double sdpin[kStages][12];                                                       // dnu of a pin
  const int tid = threadIdx.x, lane = tid & (kLanes - 1), ls = tid / kLanes;
  const int N = a.N, nx = a.nx, nu = a.nu, ng = a.ng;
  const long long nblk = (long long)a.batch * N;
  const long long blk0 = (long long)blockIdx.x * kStages;
  if (blk0 >= nblk) return;  // (the whole workgroup)
  const int nb = nblk - blk0 < kStages ? (int)(nblk - blk0) : kStages;
  const bool valid = ls < nb;
  const long long blk = blk0 + ls, qp = valid ? blk / N : 0;
  const long long xrow = blk + qp;  // x, dx: N + 1 rows per QP; pi+, dpi+: the next row
  for (int e = lane; e < 72; e += kLanes) {
    const int which = e / 12, c = e - which * 12;
    double v = 0.0;
    if (valid) {
      if (which < 2) {
        if (c < nx) v = (which == 0 ? a.x : a.dx)[xrow * nx + c];
      } else if (which < 4) {
        if (c < nu) v = (which == 2 ? a.u : a.du)[blk * nu + c];
      } else if (c < nx) {
        v = (which == 4 ? a.pi : a.dpi)[(xrow + 1) * nx + c];
      }
    }
    sv[ls][e] = v;
  }
  for (int j = lane; j < kMaxG; j += kLanes) snu[ls][j] = 0.0, sdnu[ls][j] = 0.0;
  if (lane < 12) sdpin[ls][lane] = 0.0;
  Stage& st = sst[ls];
  const Factor f = factor_stage(a, st, blk, valid, lane);  // (synchronises: sv is there after it)
  if (f.nacc > 0) {
    // rho (forward) and rho~ (adjoint) of input `lane`
    double rho = 0.0, rhot = 0.0;
    if (lane < nu) {
      const double* R = a.R + blk * nu * nu;
      const double* S = a.S + blk * nu * nx;
      const double* B = a.B + blk * nx * nu;
      const double* v = sv[ls];
      rho = a.r[blk * nu + lane];
      rhot = a.gu ? a.gu[blk * nu + lane] : 0.0;
      for (int k = 0; k < nu; ++k) {
        const double rk = R[lane + nu * k];
        rho += rk * v[kU + k], rhot += rk * v[kDu + k];
      }
      for (int k = 0; k < nx; ++k) {
        const double sk = S[lane + nu * k], bk = B[k + nx * lane];
        rho += sk * v[kX + k] + bk * v[kPip + k];
        rhot += sk * v[kDx + k] + bk * v[kDpip + k];
      }
    }
    // c = Y' rho, then T nu = -c from the last slot up; lane m holds slot m
    double c = 0.0, ct = 0.0;
    for (int m = 0; m < f.nacc; ++m) {
      const double y = lane < 12 ? st.Y[m][lane] : 0.0;
      const double t = sum16(y * rho), tt = sum16(y * rhot);
      if (lane == m) c = t, ct = tt;
    }
    double mu = 0.0, dmu = 0.0;
    for (int n = f.nacc - 1; n >= 0; --n) {
      const bool above = lane > n && lane < f.nacc;
      const double tnl = above ? st.T[n][lane] : 0.0;
      const double s = sum16(tnl * mu), stt = sum16(tnl * dmu);
      if (lane == n) {
        const double tnn = st.T[n][n];
        mu = (-c - s) / tnn, dmu = (-ct - stt) / tnn;
      }
    }
    if (lane < f.nacc) {
      if (f.src >= 0)
        snu[ls][f.src] = mu, sdnu[ls][f.src] = dmu;
      else
        sdpin[ls][-1 - f.src] = dmu;
    }
  }
  __syncthreads();
  if (a.gD) {
    const int per = ng * nu;
    if constexpr (kVec) {
      double2* out = reinterpret_cast<double2*>(a.gD + blk0 * per);
      for (int l = tid; l < nb * (per / 2); l += kThreads) {  // rows j, j + 1 of column c
        const int lb = l / (per / 2), e = 2 * (l - lb * (per / 2)), c = e / ng, j = e - ng * c;
        const double uc = sv[lb][kU + c], duc = sv[lb][kDu + c];
        out[l] = make_double2(sdnu[lb][j] * uc + snu[lb][j] * duc, sdnu[lb][j + 1] * uc + snu[lb][j + 1] * duc);
      }
    } else {
      for (int l = tid; l < nb * per; l += kThreads) {
        const int lb = l / per, e = l - lb * per, c = e / ng, j = e - ng * c;
        a.gD[blk0 * per + l] = sdnu[lb][j] * sv[lb][kU + c] + snu[lb][j] * sv[lb][kDu + c];
      }
    }
  }
  if (a.nu_out || a.dnu_out) {
    if constexpr (kVec) {
      double2* nuo = reinterpret_cast<double2*>(a.nu_out ? a.nu_out + blk0 * ng : nullptr);
      double2* dnuo = reinterpret_cast<double2*>(a.dnu_out ? a.dnu_out + blk0 * ng : nullptr);
      for (int l = tid; l < nb * (ng / 2); l += kThreads) {  // rows j, j + 1
        const int lb = l / (ng / 2), j = 2 * (l - lb * (ng / 2));
        if (nuo) nuo[l] = make_double2(snu[lb][j], snu[lb][j + 1]);
        if (dnuo) dnuo[l] = make_double2(sdnu[lb][j], sdnu[lb][j + 1]);
      }
    } else {
      for (int l = tid; l < nb * ng; l += kThreads) {
        const int lb = l / ng, j = l - lb * ng;
        if (a.nu_out) a.nu_out[blk0 * ng + l] = snu[lb][j];
        if (a.dnu_out) a.dnu_out[blk0 * ng + l] = sdnu[lb][j];
      }
    }
  }
  if (a.glg || a.gug) {
    for (int l = tid; l < nb * ng; l += kThreads) {
      const int lb = l / ng, j = l - lb * ng;
      const long long b = blk0 + lb, k = b % N, row = (b + b / N) * ng + j;
      const int side = sst[lb].act[j];
      const double g = 0.0 - sdnu[lb][j];
      if (a.glg) a.glg[row] = side == 1 ? g : 0.0;
      if (a.gug) a.gug[row] = side == 2 ? g : 0.0;
      if (k == N - 1) {  // the terminal row has no general rows (C = NULL)
        if (a.glg) a.glg[row + ng] = 0.0;
        if (a.gug) a.gug[row + ng] = 0.0;
      }
    }
  }
  if (a.glbu || a.gubu) {
    for (int l = tid; l < nb * nu; l += kThreads) {
      const int lb = l / nu, c = l - lb * nu;
      const int side = sst[lb].pin[c];
      const double g = 0.0 - sdpin[lb][c];
      if (a.glbu) a.glbu[blk0 * nu + l] = side == 1 ? g : 0.0;
      if (a.gubu) a.gubu[blk0 * nu + l] = side == 2 ? g : 0.0;
    }
  }
}

bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  return true;
}

}  // namespace

hipError_t launch_backward_project(const BackwardRowsArgs& a, hipStream_t stream) {
  if (a.batch <= 0) return hipSuccess;
  const long long nblk = (long long)a.batch * a.N;
  const dim3 grid((unsigned)((nblk + kStages - 1) / kStages));
  if (a.nx == 12 && a.nu == 12 && aligned16({a.B, a.S, a.R, a.gu, a.Bm, a.Sm, a.Rm, a.rm}))
    hipLaunchKernelGGL(backward_project_kernel<true>, grid, dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL(backward_project_kernel<false>, grid, dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_backward_lift(const BackwardRowsArgs& a, hipStream_t stream) {
  if (a.batch <= 0 || !(a.gD || a.glg || a.gug || a.glbu || a.gubu || a.nu_out || a.dnu_out)) return hipSuccess;
  const long long nblk = (long long)a.batch * a.N;
  const dim3 grid((unsigned)((nblk + kStages - 1) / kStages));
  if (a.ng % 2 == 0 && aligned16({a.gD, a.nu_out, a.dnu_out}))
    hipLaunchKernelGGL(backward_lift_kernel<true>, grid, dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL(backward_lift_kernel<false>, grid, dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace srbd
