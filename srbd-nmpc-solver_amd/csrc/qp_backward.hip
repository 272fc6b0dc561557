// qp_backward.hip -- the two kernels the backward pass adds to the solve.
//
// The backward pass of an OCP-QP is one more Riccati solve with the same matrices (the adjoint
// QP: q := dl/dx, r := dl/du, b := 0, x0 := 0; launch_riccati_unconstr as it is) and then outer
// products of the two solutions:
//   dQ = 1/2 (dx x' + x dx')   dR = 1/2 (du u' + u du')   dS = du x' + u dx'
//   dA = pi+ dx' + dpi+ x'     dB = pi+ du' + dpi+ u'
//   dq = dx   dr = du   db = dpi+   dx0 = dpi_0
// Every matrix gradient is  s (a c' + b d')  with two row vectors a, b and two column vectors
// c, d of its stage.  The kernel is write-bound: it reads 72 doubles per stage and writes up to
// five 144-double blocks.  In the QP-major layout each output array is one contiguous run of
// blocks, so the stores are shaped over the array, not over the block.  A workgroup takes
// kGroup consecutive stages: it stages their six vectors in LDS once (72 doubles per stage; the
// one division by N + 1 per stage happens here), then, for every requested matrix in turn, each
// thread forms 16-byte pieces (two rows of one column), consecutive threads consecutive pieces,
// so that a wave instruction stores 1 KiB of whole 128-byte lines (a run breaks only where a
// QP's terminal stage has no block).  An output that is not asked for costs no piece.  The
// vector gradients are copies and have a kernel of their own, so q, r, b, x0 alone never touch
// the matrix paths.
//
// The mask kernel (input boxes) writes the masked copy of B, S, R, r the adjoint QP is solved
// on, in the same shape: a workgroup evaluates the pin rule once for the 12 inputs of each of
// its kGroup stages, then streams the four arrays through.
//
// These are the kernels for nx = nu = 12 with every pointer 16-byte aligned.  Anything else
// takes the generic kernels: one thread per element, bounds from nx, nu on the caller's arrays.
#include "qp_backward.h"

#include <cstdint>
#include <initializer_list>

namespace srbd {
namespace {

constexpr int kThreads = 256;
constexpr int kGroup = 32;  // stages per workgroup: 2304 pieces per matrix, 9 per thread

enum GradKind { kGradA, kGradB, kGradQ, kGradS, kGradR, kGradq, kGradr, kGradb, kGradx0, kGradKinds };
struct GradList {
  int n;
  int kind[kGradKinds];
};

// The operands of a matrix gradient  s (a c' + b d'):  a, b indexed by the row, c, d by the
// column; rows x cols blocks.  The blocks count (qp, k) over `stages` stages per QP; a vector
// array holds stages + off rows per QP (off 0: u, du; off 1: x, dx, and pi+, dpi+ entered one
// row down), so block blk reads row blk + qp off.
struct Outer {
  double* out;
  const double *a, *b, *c, *d;
  int rows, cols, stages, row_off, col_off;
  double s;
};
__device__ __forceinline__ Outer outer_of(const BackwardGradArgs& g, int kind) {
  const int N = g.N, nx = g.nx, nu = g.nu;
  const double* pip = g.pi + nx;  // pi+ / dpi+ of stage k: row k + 1
  const double* dpip = g.dpi + nx;
  switch (kind) {
    case kGradA: return {g.A, pip, dpip, g.dx, g.x, nx, nx, N, 1, 1, 1.0};
    case kGradB: return {g.B, pip, dpip, g.du, g.u, nx, nu, N, 1, 0, 1.0};
    case kGradQ: return {g.Q, g.dx, g.x, g.x, g.dx, nx, nx, N + 1, 0, 0, 0.5};
    case kGradS: return {g.S, g.du, g.u, g.x, g.dx, nu, nx, N, 0, 1, 1.0};
    default: return {g.R, g.du, g.u, g.u, g.du, nu, nu, N, 0, 0, 0.5};
  }
}
// The vector gradients are copies of `n` values per QP out of rows of `stride`, from `skip` on
struct Rows {
  double* out;
  const double* src;
  long long n, stride, skip;
};
__device__ __forceinline__ Rows rows_of(const BackwardGradArgs& g, int kind) {
  const long long xs = (long long)(g.N + 1) * g.nx, us = (long long)g.N * g.nu;
  switch (kind) {
    case kGradq: return {g.q, g.dx, xs, xs, 0};
    case kGradr: return {g.r, g.du, us, us, 0};
    case kGradb: return {g.b, g.dpi, (long long)g.N * g.nx, xs, g.nx};  // dpi_{k+1}
    default: return {g.x0, g.dpi, g.nx, xs, 0};                          // dpi_0
  }
}

// ---------------------------------------------------------------------------
// gradient kernels
// ---------------------------------------------------------------------------
// The vector gradients: 16-byte pieces of a flat copy; blockIdx.y walks the requested ones.
__global__ void __launch_bounds__(kThreads) backward_rows_kernel(BackwardGradArgs g, GradList list) {
  const Rows r = rows_of(g, list.kind[blockIdx.y]);
  const long long e = 2 * ((long long)blockIdx.x * kThreads + threadIdx.x);
  if (e >= r.n * g.batch) return;
  const long long qp = e / r.n;
  *reinterpret_cast<double2*>(r.out + e) =
      *reinterpret_cast<const double2*>(r.src + qp * r.stride + r.skip + (e - qp * r.n));
}

// The matrix gradients of kGroup consecutive stages s = qp (N + 1) + k, every requested one from
// one staging of the stage's six vectors.  A, B, S, R have N blocks per QP: stage (qp, k < N)
// is their block s - qp, and the terminal stage has a Q block only.
constexpr int kX = 0, kDx = 12, kU = 24, kDu = 36, kPip = 48, kDpip = 60;  // a stage's LDS row
__global__ void __launch_bounds__(kThreads) backward_grad_kernel(BackwardGradArgs g, GradList list) {
  __shared__ __attribute__((aligned(16))) double sv[kGroup][72];
  __shared__ long long sblk[kGroup];  // s - qp, or -1 for the terminal stage
  const int tid = threadIdx.x, N = g.N;
  const long long nst = (long long)g.batch * (N + 1);
  const long long s0 = (long long)blockIdx.x * kGroup;
  if (s0 >= nst) return;  // (the whole workgroup)
  const int nb = nst - s0 < kGroup ? (int)(nst - s0) : kGroup;
  if (tid < nb) {
    const long long s = s0 + tid, qp = s / (N + 1);
    sblk[tid] = s - qp * (N + 1) < N ? s - qp : -1;
  }
  __syncthreads();
  for (int idx = tid; idx < nb * 72; idx += kThreads) {
    const int lb = idx / 72, w = idx - lb * 72, which = w / 12, e = w - which * 12;
    const long long s = s0 + lb, blk = sblk[lb];
    double v = 0.0;
    if (which < 2)
      v = (which == 0 ? g.x : g.dx)[s * 12 + e];
    else if (blk >= 0)  // u, du: N rows per QP; pi+, dpi+: the next stage's row
      v = which < 4 ? (which == 2 ? g.u : g.du)[blk * 12 + e] : (which == 4 ? g.pi : g.dpi)[(s + 1) * 12 + e];
    sv[lb][w] = v;
  }
  __syncthreads();
  for (int n = 0; n < list.n; ++n) {
    const int kind = list.kind[n];
    if (kind >= kGradq) break;  // (the vectors come after the matrices)
    // out = s (a c' + b d'): the operands' places in the stage's row
    int a, b, c, d;
    double* out;
    switch (kind) {
      case kGradA: out = g.A, a = kPip, b = kDpip, c = kDx, d = kX; break;
      case kGradB: out = g.B, a = kPip, b = kDpip, c = kDu, d = kU; break;
      case kGradQ: out = g.Q, a = kDx, b = kX, c = kX, d = kDx; break;
      case kGradS: out = g.S, a = kDu, b = kU, c = kX, d = kDx; break;
      default: out = g.R, a = kDu, b = kU, c = kU, d = kDu; break;
    }
    const double scale = kind == kGradQ || kind == kGradR ? 0.5 : 1.0;
    for (int l = tid; l < nb * 72; l += kThreads) {  // piece l: rows i, i + 1 of column j of stage lb
      const int lb = l / 72, e = 2 * (l - lb * 72), j = e / 12, i = e - 12 * j;
      const long long blk = kind == kGradQ ? s0 + lb : sblk[lb];
      if (blk < 0) continue;
      const double2 a2 = *reinterpret_cast<const double2*>(&sv[lb][a + i]);
      const double2 b2 = *reinterpret_cast<const double2*>(&sv[lb][b + i]);
      const double cj = sv[lb][c + j], dj = sv[lb][d + j];
      *reinterpret_cast<double2*>(out + blk * 144 + e) =
          make_double2(scale * (a2.x * cj + b2.x * dj), scale * (a2.y * cj + b2.y * dj));
    }
  }
}

__global__ void __launch_bounds__(kThreads) backward_grad_generic_kernel(BackwardGradArgs g, GradList list) {
  const int kind = list.kind[blockIdx.y];
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (kind >= kGradq) {
    const Rows r = rows_of(g, kind);
    if (t >= r.n * g.batch) return;
    const long long qp = t / r.n;
    r.out[t] = r.src[qp * r.stride + r.skip + (t - qp * r.n)];
    return;
  }
  const Outer o = outer_of(g, kind);
  const long long per = (long long)o.rows * o.cols;
  if (t >= per * g.batch * o.stages) return;
  const long long blk = t / per, qp = blk / o.stages;
  const int e = (int)(t - blk * per), j = e / o.rows, i = e - o.rows * j;
  const long long ra = (blk + qp * o.row_off) * o.rows + i, ca = (blk + qp * o.col_off) * o.cols + j;
  o.out[t] = o.s * (o.a[ra] * o.c[ca] + o.b[ra] * o.d[ca]);
}

// ---------------------------------------------------------------------------
// mask kernels
// ---------------------------------------------------------------------------
// input `at` = (qp N + k) nu + i
__device__ __forceinline__ bool pinned(const BackwardMaskArgs& a, long long at) {
  const double u = a.u[at];
  const bool lo = (!a.lbu_mask || a.lbu_mask[at] != 0.0) && u - a.lbu[at] < a.act_tol;
  const bool hi = (!a.ubu_mask || a.ubu_mask[at] != 0.0) && a.ubu[at] - u < a.act_tol;
  return lo || hi;
}
// the pinned inputs of QP t / 64, counted by one wave
__device__ __forceinline__ void count_pinned(const BackwardMaskArgs& a, long long t) {
  const long long qp = t / 64;
  const int lane = (int)(t & 63), per = a.N * a.nu;
  if (qp >= a.batch) return;  // (the whole wave)
  int n = 0;
  for (int s = lane; s < per; s += 64) n += pinned(a, qp * per + s) ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if (lane == 0) a.count[qp] = n;
}

// blockIdx.y 0: the four arrays of kGroup stages; 1: the counts
__global__ void __launch_bounds__(kThreads) backward_mask_kernel(BackwardMaskArgs a) {
  __shared__ int pin[kGroup * 12];
  const int tid = threadIdx.x;
  if (blockIdx.y == 1) {
    if (a.count) count_pinned(a, (long long)blockIdx.x * kThreads + tid);
    return;
  }
  const long long nblk = (long long)a.batch * a.N;
  const long long blk0 = (long long)blockIdx.x * kGroup;
  if (blk0 >= nblk) return;  // (the whole workgroup)
  const int nb = nblk - blk0 < kGroup ? (int)(nblk - blk0) : kGroup;
  for (int s = tid; s < nb * 12; s += kThreads) pin[s] = pinned(a, blk0 * 12 + s) ? 1 : 0;
  __syncthreads();
  const double2* B = reinterpret_cast<const double2*>(a.B + blk0 * 144);
  const double2* S = reinterpret_cast<const double2*>(a.S + blk0 * 144);
  const double2* R = reinterpret_cast<const double2*>(a.R + blk0 * 144);
  double2* Bm = reinterpret_cast<double2*>(a.Bm + blk0 * 144);
  double2* Sm = reinterpret_cast<double2*>(a.Sm + blk0 * 144);
  double2* Rm = reinterpret_cast<double2*>(a.Rm + blk0 * 144);
  const double2 zero = make_double2(0.0, 0.0);
  for (int l = tid; l < nb * 72; l += kThreads) {  // piece l: rows i, i + 1 of column j
    const int lb = l / 72, e = 2 * (l - lb * 72), j = e / 12, i = e - 12 * j;
    const int pj = pin[lb * 12 + j], p0 = pin[lb * 12 + i], p1 = pin[lb * 12 + i + 1];
    Bm[l] = pj ? zero : B[l];  // column of a pinned input
    double2 s = S[l];          // its row
    if (p0) s.x = 0.0;
    if (p1) s.y = 0.0;
    Sm[l] = s;
    double2 r = R[l];  // row and column, 1 on the diagonal
    if (pj || p0) r.x = i == j ? 1.0 : 0.0;
    if (pj || p1) r.y = i + 1 == j ? 1.0 : 0.0;
    Rm[l] = r;
  }
  const double2* gu = a.gu ? reinterpret_cast<const double2*>(a.gu + blk0 * 12) : nullptr;
  double2* rm = reinterpret_cast<double2*>(a.rm + blk0 * 12);
  for (int l = tid; l < nb * 6; l += kThreads) {  // the cotangent (NULL: zero), pinned entries cleared
    double2 v = gu ? gu[l] : zero;
    if (pin[2 * l]) v.x = 0.0;
    if (pin[2 * l + 1]) v.y = 0.0;
    rm[l] = v;
  }
}

enum MaskKind { kMaskB, kMaskS, kMaskR, kMaskr, kMaskCount, kMaskKinds };
__global__ void __launch_bounds__(kThreads) backward_mask_generic_kernel(BackwardMaskArgs a) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int nx = a.nx, nu = a.nu;
  const long long nblk = (long long)a.batch * a.N;
  if (blockIdx.y == kMaskCount) {
    if (a.count) count_pinned(a, t);
    return;
  }
  if (blockIdx.y == kMaskr) {
    if (t < nblk * nu) a.rm[t] = !a.gu || pinned(a, t) ? 0.0 : a.gu[t];
    return;
  }
  // element (i, j) of a rows x cols column-major block
  const int rows = blockIdx.y == kMaskB ? nx : nu, cols = blockIdx.y == kMaskS ? nx : nu;
  const long long per = (long long)rows * cols;
  if (t >= nblk * per) return;
  const long long blk = t / per;
  const int e = (int)(t - blk * per), j = e / rows, i = e - rows * j;
  if (blockIdx.y == kMaskB) {
    a.Bm[t] = pinned(a, blk * nu + j) ? 0.0 : a.B[t];
  } else if (blockIdx.y == kMaskS) {
    a.Sm[t] = pinned(a, blk * nu + i) ? 0.0 : a.S[t];
  } else {
    const bool z = pinned(a, blk * nu + i) || pinned(a, blk * nu + j);
    a.Rm[t] = z ? (i == j ? 1.0 : 0.0) : a.R[t];
  }
}

bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  return true;
}
unsigned blocks_for(long long threads, long long per_block = kThreads) {
  return (unsigned)((threads + per_block - 1) / per_block);
}

}  // namespace

hipError_t launch_backward_mask(const BackwardMaskArgs& a, hipStream_t stream) {
  if (a.batch <= 0) return hipSuccess;
  const long long nblk = (long long)a.batch * a.N;
  const unsigned count_blocks = blocks_for((long long)a.batch * 64);  // a wave per QP
  if (a.nx == 12 && a.nu == 12 && aligned16({a.B, a.S, a.R, a.gu, a.Bm, a.Sm, a.Rm, a.rm})) {
    const unsigned groups = blocks_for(nblk, kGroup);
    hipLaunchKernelGGL(backward_mask_kernel, dim3(groups > count_blocks ? groups : count_blocks, 2), dim3(kThreads), 0,
                       stream, a);
  } else {
    const unsigned elems = blocks_for(nblk * (a.nx > a.nu ? a.nx : a.nu) * a.nu);
    hipLaunchKernelGGL(backward_mask_generic_kernel, dim3(elems > count_blocks ? elems : count_blocks, kMaskKinds),
                       dim3(kThreads), 0, stream, a);
  }
  return hipGetLastError();
}

hipError_t launch_backward_grad(const BackwardGradArgs& a, hipStream_t stream) {
  if (a.batch <= 0) return hipSuccess;
  GradList list{};
  double* const out[kGradKinds] = {a.A, a.B, a.Q, a.S, a.R, a.q, a.r, a.b, a.x0};
  for (int k = 0; k < kGradKinds; ++k)
    if (out[k]) list.kind[list.n++] = k;
  if (list.n == 0) return hipSuccess;
  // the grid covers the largest requested output: Q's blocks among the matrices, q's values
  // among the vectors
  const bool matrices = a.A || a.B || a.Q || a.S || a.R;
  const long long stages = (long long)a.batch * (a.N + 1);
  if (a.nx == 12 && a.nu == 12 &&
      aligned16({a.x, a.u, a.pi, a.dx, a.du, a.dpi, a.A, a.B, a.b, a.Q, a.S, a.R, a.q, a.r, a.x0})) {
    if (matrices)
      hipLaunchKernelGGL(backward_grad_kernel, dim3(blocks_for(stages, kGroup)), dim3(kThreads), 0, stream, a, list);
    GradList rows{};
    for (int k = kGradq; k < kGradKinds; ++k)
      if (out[k]) rows.kind[rows.n++] = k;
    if (rows.n)
      hipLaunchKernelGGL(backward_rows_kernel, dim3(blocks_for(stages * 6), (unsigned)rows.n), dim3(kThreads), 0,
                         stream, a, rows);
  } else {
    const int m = a.nx > a.nu ? a.nx : a.nu;
    hipLaunchKernelGGL(backward_grad_generic_kernel, dim3(blocks_for(matrices ? stages * m * m : stages * m), (unsigned)list.n),
                       dim3(kThreads), 0, stream, a, list);
  }
  return hipGetLastError();
}

}  // namespace srbd
