// srbd_solve_backward.hip -- the fused backward pass robots / plan <- solve
// (srbd_qp_srbd_solve_backward_f64): what srbd_qp_solve_backward_rows_f64 followed
// by srbd_qp_srbd_linearize_backward_f64 returns, without the gradients of A, B, Q, S, R, D in
// between.  Every block of those is two outer products of the stage's vectors -- x, u, pi of the
// forward solve, dx, du, dpi of the adjoint, and with the cone the multipliers nu, dnu of the lift
// kernel -- so the 47 slots of the cotangent descriptor (srbd_lin_backward.h) are formed from the
// vectors, 72 doubles per stage read instead of 5 x 144 written and read again.
//   srbd_solve_bwd_stage_kernel  one thread per (QP, stage k < N), srbd_lin_bwd_stage_kernel's
//       shape.  The wave stages the six vectors of kStChunk stages at a time in LDS, 16-byte
//       pieces at consecutive addresses (u, du: one contiguous run; x, dx, pi, dpi have N + 1 rows
//       per QP, so a run skips a row at a QP boundary; pi+ is the next row), then one lane forms
//       one descriptor slot.  The stage thread runs the shared reverse model with
//       cot b := dpi+, cot r := du, cot lg := -dnu, cot ubu from the lift kernel's compact rows.
//   srbd_lin_bwd_reduce_kernel   unchanged (srbd_lin_backward.h): fixed order, no atomics.
//   srbd_solve_bwd_cost_kernel   Q, Qf, x_ref from cot Q[k]_jj = dx_kj x_kj and cot q[k] = dx_k
//       (dx_0 = 0 gives the zeros of stage 0), and grad_x0 = dpi_0.
// The host statement that pins it is tests/srbd_solve_vjp_host.py.
#include "srbd_lin_backward.h"

#include <cstdint>

namespace srbd {
namespace {

constexpr int kStChunk = 16;                                        // stages staged at a time
constexpr int kX = 0, kDx = 12, kU = 24, kDu = 36, kPip = 48, kDpip = 60;  // a stage's LDS row

// one descriptor slot of a stage from its staged row v (72 doubles); nu, dnu: the stage's 24
// multipliers (CONE) or NULL
__device__ __forceinline__ double slot_of(const double* v, int s, const double* nu, const double* dnu) {
  // G_A(i, j) = pi+_i dx_j + dpi+_i x_j,  G_B(i, j) = pi+_i du_j + dpi+_i u_j
  auto GA = [&](int i, int j) { return v[kPip + i] * v[kDx + j] + v[kDpip + i] * v[kX + j]; };
  auto GB = [&](int i, int j) { return v[kPip + i] * v[kDu + j] + v[kDpip + i] * v[kU + j]; };
  if (s < kGP0) {
    const int top = s < kGJ01 ? 0 : 3, e = s < kGJ01 ? s : s - kGJ01;
    return GA(e / 3, top + e % 3);
  }
  if (s < kGIm) {
    // skew(p)[r][c] = -p_a where c - r = 1 (mod 3), +p_a the other way round, a = 3 - r - c
    const int cb = s < kGP1 ? 0 : 6, a = s < kGP1 ? s - kGP0 : s - kGP1;
    const int r1 = (a + 1) % 3, c1 = (a + 2) % 3;
    return GB(3 + c1, cb + r1) - GB(3 + r1, cb + c1);
  }
  if (s == kGIm) {
    double tr = 0.0;
    for (int i = 0; i < 3; ++i) tr += GB(9 + i, i) + GB(9 + i, 6 + i);
    return tr;
  }
  if (s < kGRp) {
    const int i = s - kGRd;
    return v[kDu + i] * v[kU + i];
  }
  if (s < kGD) {
    const int leg = (s - kGRp) / 4, pr = (s - kGRp) % 4, o = 6 * leg;
    const int lo = o + (pr < 2 ? pr : 2), hi = o + (pr < 2 ? 2 : pr + 2);
    return v[kDu + lo] * v[kU + hi] + v[kU + lo] * v[kDu + hi];
  }
  if (!nu) return 0.0;
  // D holds mu in column fz of the leg's rows 0..3: grad D_j = dnu_j u' + nu_j du'
  const int leg = s - kGD, fz = 6 * leg + 2, r0 = 12 * leg;
  const double ufz = v[kU + fz], dufz = v[kDu + fz];
  double d[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = dnu[r0 + j] * ufz + nu[r0 + j] * dufz;
  return (d[0] + d[1]) + (d[2] + d[3]);
}

// kVec: the caller's x, u, pi are 16-byte aligned (the handle's dx, du, dpi always are); otherwise
// the staging loads go element by element.
template <bool PLAN, bool ROBOT, bool kVec>
__global__ void __launch_bounds__(kBwdThreads)
    srbd_solve_bwd_stage_kernel(Model m, LinBwdArgsT<PLAN, ROBOT> a, SolveBwdVecs sv) {
  __shared__ double desc[kBwdThreads * kGDesc];
  __shared__ double2 stg[kStChunk * 36];
  const int N = a.N;
  const long long nst_all = (long long)a.batch * N;
  const long long t0 = (long long)blockIdx.x * kBwdThreads;
  const long long left = nst_all - t0;
  const int nst = left < kBwdThreads ? (int)left : kBwdThreads;
  const long long qp0 = t0 / N;
  const int k0 = (int)(t0 - qp0 * N);  // stage t0 + b is stage (k0 + b) % N of QP qp0 + (k0 + b) / N
  const bool cone = a.mode == 2 && sv.nu && sv.dnu;
  constexpr int kPer = kStChunk * 36 / kBwdThreads;  // pieces per lane and chunk
  for (int c0 = 0; c0 < nst; c0 += kStChunk) {
    const int nb = nst - c0 < kStChunk ? nst - c0 : kStChunk;
    double2 tmp[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int pc = i * kBwdThreads + threadIdx.x;
      const int b = pc / 36, w = pc - b * 36, which = w / 6, e = 2 * (w - which * 6);
      tmp[i] = make_double2(0.0, 0.0);
      if (b < nb) {
        const long long t = t0 + c0 + b;
        const long long row = t + qp0 + (k0 + c0 + b) / N;  // x, dx; pi+, dpi+: the next row
        const double* base = which == 0 ? sv.x : which == 1 ? sv.dx : which == 2 ? sv.u : which == 3 ? sv.du
                             : which == 4 ? sv.pi : sv.dpi;
        const double* src = base + (which < 2 ? row : which < 4 ? t : row + 1) * 12 + e;
        // (the adjoint's rows are the handle's: aligned whatever the caller's are)
        if (kVec || (which & 1))
          tmp[i] = *reinterpret_cast<const double2*>(src);
        else
          tmp[i] = make_double2(src[0], src[1]);
      }
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i) stg[i * kBwdThreads + threadIdx.x] = tmp[i];
    __syncthreads();
    const double* sd = reinterpret_cast<const double*>(stg);
    for (int it = threadIdx.x; it < nb * kGDesc; it += kBwdThreads) {
      const int b = it / kGDesc, s = it - b * kGDesc;
      const size_t row24 = (size_t)(t0 + c0 + b) * 24;
      desc[(c0 + b) * kGDesc + s] = slot_of(sd + b * 72, s, cone ? sv.nu + row24 : nullptr, cone ? sv.dnu + row24 : nullptr);
    }
    __syncthreads();
  }
  const long long t = t0 + threadIdx.x;
  if (t >= nst_all) return;
  const long long row = t + t / N;
  StageCot c;
  c.gb = sv.dpi + (size_t)(row + 1) * 12;
  c.gr = sv.du + (size_t)t * 12;
  c.gubu = (a.mode == 1 && sv.gubu) ? sv.gubu + (size_t)t * 12 : nullptr;
  c.lg = cone ? sv.dnu + (size_t)t * 24 : nullptr;  // cot lg = -dnu: the cone's rows have no upper side
  c.lg_sign = -1.0;
  c.has_A = true;
  stage_reverse<PLAN, ROBOT>(m, a, t, desc + threadIdx.x * kGDesc, c);
}

// srbd_lin_bwd_cost_kernel with cot Q's diagonal and cot q formed from x and dx; one thread per
// (robot, j < 12).  grad_x0 = dpi_0 rides along.
template <bool PLAN, bool ROBOT>
__global__ void __launch_bounds__(256)
    srbd_solve_bwd_cost_kernel(Model m, LinBwdArgsT<PLAN, ROBOT> a, SolveBwdVecs sv) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)a.batch * 12) return;
  const srbd_model_params& p = m.p;
  const int qp = (int)(gid / 12), j = (int)(gid % 12), N = a.N;
  if (sv.gx0) sv.gx0[gid] = sv.dpi[(size_t)qp * (N + 1) * 12 + j];
  if (!a.out.Q && !a.out.Qf && !a.out.x_ref) return;
  double wQ = p.Q[j], wQf = p.Qf[j];
  if constexpr (ROBOT) {
    if (a.Q) wQ = a.Q[(size_t)qp * 12 + j];
    if (a.Qf) wQf = a.Qf[(size_t)qp * 12 + j];
  }
  double sQ = 0.0;
  for (int k = 0; k <= N; ++k) {
    const size_t e = ((size_t)qp * (N + 1) + k) * 12 + j;
    const double gq = sv.dx[e];
    const double gQ = gq * sv.x[e];
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

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

hipError_t launch_srbd_solve_backward(const srbd_model_params& p, int batch, int N, int mode, const double* xs,
                                      const double* us, const SolveBwdVecs& v, const srbd_lin_grad_f64& grad,
                                      double* part, hipStream_t stream, const srbd_plan_f64* plan,
                                      const srbd_robots_f64* robots) {
  if (batch <= 0) return hipSuccess;
  Model m{p};
  LinBwdArgs a{};
  a.batch = batch;
  a.N = N;
  a.mode = mode;
  a.xs = xs;
  a.us = us;
  a.out = grad;
  const bool sums = grad.mass || grad.Lbody || grad.mu || grad.R;
  a.part = sums ? part : nullptr;
  a.qf_scale = p.qf_scale;
  const bool stage = sums || grad.foot_r || grad.foot_l || grad.fz_max;
  const bool cost = grad.Q || grad.Qf || grad.x_ref || v.gx0;
  const bool vec = aligned16(v.x) && aligned16(v.u) && aligned16(v.pi);
  const long long nst = (long long)batch * N;
  dispatch(plan_given(plan), robots_given(robots), [&](auto PL, auto RB) {
    constexpr bool kP = decltype(PL)::value, kR = decltype(RB)::value;
    const auto full = full_args<kP, kR>(a, plan, robots);
    const dim3 grid((unsigned)((nst + kBwdThreads - 1) / kBwdThreads));
    if (stage && vec)
      hipLaunchKernelGGL((srbd_solve_bwd_stage_kernel<kP, kR, true>), grid, dim3(kBwdThreads), 0, stream, m, full, v);
    else if (stage)
      hipLaunchKernelGGL((srbd_solve_bwd_stage_kernel<kP, kR, false>), grid, dim3(kBwdThreads), 0, stream, m, full, v);
    if (sums)
      hipLaunchKernelGGL((srbd_lin_bwd_reduce_kernel<kR>), dim3((unsigned)(((long long)batch * kPart + 255) / 256)),
                         dim3(256), 0, stream, m, full_args<false, kR>(a, plan, robots));
    if (cost)
      hipLaunchKernelGGL((srbd_solve_bwd_cost_kernel<kP, kR>), dim3((unsigned)(((long long)batch * 12 + 255) / 256)),
                         dim3(256), 0, stream, m, full, v);
  });
  return hipGetLastError();
}

}  // namespace srbd
