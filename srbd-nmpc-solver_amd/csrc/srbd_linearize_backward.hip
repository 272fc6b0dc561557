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
// The descriptor's layout, the reverse model and the reduce kernel are in srbd_lin_backward.h,
// shared with the fused pass (srbd_solve_backward.hip).
// The host statement that pins it is tests/linearize_vjp_host.py.
#include "srbd_lin_backward.h"

namespace srbd {
namespace {

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
  const long long xrow = t + t / N;  // lg: N + 1 rows per QP
  StageCot c;
  c.gb = a.gb ? a.gb + (size_t)t * 12 : nullptr;
  c.gr = a.gr ? a.gr + (size_t)t * 12 : nullptr;
  c.gubu = a.gubu ? a.gubu + (size_t)t * 12 : nullptr;
  c.lg = a.glg ? a.glg + (size_t)xrow * 24 : nullptr;
  c.lg_sign = 1.0;
  c.has_A = a.gA != nullptr;
  stage_reverse<PLAN, ROBOT>(m, a, t, desc + threadIdx.x * kGDesc, c);
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
