// capi_backward.hip -- the backward pass of the device-pointer solve (include/srbd_qp.h:
// srbd_qp_solve_backward_f64, srbd_qp_backward_pinned_f64): the checks of a call, the adjoint
// QP's launch arguments, the Riccati solve that is the adjoint, and the gradient kernel
// (qp_backward.hip).
#include "capi_handle.h"
#include "qp_backward.h"

#include <cmath>
#include <cstring>
#include <string>

using namespace srbd::capi;

namespace {

// Element (double) offsets of the backward buffer, for `cap` QPs: the adjoint solution, a run
// of zeros (the adjoint's b and x0, and a NULL cotangent), and with input boxes the masked
// stages and the pinned count.
struct BackwardLayout {
  size_t dx, du, dpi, zero, zero_elems, Bm, Sm, Rm, rm, count, total;
  BackwardLayout(const srbd_qp_dims& m, size_t cap) {
    size_t o = 0;
    auto take = [&](size_t n) {
      const size_t at = o;
      o += (n + 31) / 32 * 32;  // 256-byte aligned
      return at;
    };
    const size_t N = (size_t)m.N, nx = (size_t)m.nx, nu = (size_t)m.nu;
    dx = take(cap * (N + 1) * nx);
    du = take(cap * N * nu);
    dpi = take(cap * (N + 1) * nx);
    zero_elems = cap * (N + 1) * (nx > nu ? nx : nu);
    zero = take(zero_elems);
    Bm = Sm = Rm = rm = count = 0;
    if (m.has_box_u) {
      Bm = take(cap * N * nx * nu);
      Sm = take(cap * N * nu * nx);
      Rm = take(cap * N * nu * nu);
      rm = take(cap * N * nu);
      count = take((cap + 1) / 2);  // ints
    }
    total = o;
  }
};

int backward_impl(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const srbd_qp_data_f64* d,
                  const srbd_qp_solution_f64* s, const double* gx, const double* gu, double act_tol,
                  const srbd_qp_grad_f64* g, void* stream) {
  // the checks that read the arguments alone come first; the handle is read after them
  if (!h) return fail(SRBD_QP_EINVAL, "handle is NULL");
  if (!d || !s || !g) return fail(SRBD_QP_EINVAL, "data/solution/grad is NULL");
  if (!st) return fail(SRBD_QP_EINVAL, "settings is NULL");
  if (!gx && !gu) return fail(SRBD_QP_EINVAL, "gx and gu are both NULL: no cotangent");
  if (!(act_tol >= 0.0) || !std::isfinite(act_tol))
    return fail(SRBD_QP_EINVAL, "act_tol must be finite and >= 0");
  if (!(st->reg_prim >= 0.0)) return fail(SRBD_QP_ESETTINGS, "OcpQpIpmSolverSettings.reg_prim must be non-negative");
  const srbd_qp_dims& dm = h->dims;
  if (dm.ng > 0)
    return fail(SRBD_QP_EDIM, "backward: general rows (ng > 0) are not supported, got ng = " + std::to_string(dm.ng));
  if (dm.has_box_x) return fail(SRBD_QP_EDIM, "backward: state boxes (has_box_x) are not supported");
  if (dm.layout != SRBD_QP_LAYOUT_QP_MAJOR) return fail(SRBD_QP_EDIM, "backward: the stage-major layout is not supported");
  if (batch < 0) return fail(SRBD_QP_EINVAL, "batch must be >= 0");
  if (batch > h->capacity)
    return fail(SRBD_QP_ECAPACITY, "batch " + std::to_string(batch) + " exceeds capacity " +
                                       std::to_string(h->capacity));
  if (!d->A || !d->B || !d->b || !d->Q || !d->S || !d->R || !d->q || !d->r || !d->x0)
    return fail(SRBD_QP_EINVAL, "A, B, b, Q, S, R, q, r and x0 are required");
  if (!s->x || !s->u || !s->pi) return fail(SRBD_QP_EINVAL, "the forward x, u and pi are required");
  if (dm.has_box_u && (!d->lbu || !d->ubu))
    return fail(SRBD_QP_EINVAL, "a handle with has_box_u needs lbu and ubu (the forward call's)");
  if (batch == 0) return SRBD_QP_OK;

  hipStream_t strm = stream_of(h, stream);
  srbd::DeviceGuard guard(h->device);
  const BackwardLayout L(dm, (size_t)h->capacity);
  const bool padded = dm.nx != 12 || dm.nu != 12;
  const void* before = h->bwd.p;
  hipError_t e = h->bwd.reserve(L.total * sizeof(double));
  if (e == hipSuccess && padded) e = h->pad.reserve(srbd::pad_elems(h->capacity, dm.N, 0) * sizeof(double));
  if (e != hipSuccess) return hip_fail(SRBD_QP_ENOMEM, "backward buffers: ", e);
  double* const buf = h->bwd.as<double>();
  // (nothing writes the zeros after this: once per allocation)
  if (h->bwd.p != before) e = hipMemsetAsync(buf + L.zero, 0, L.zero_elems * sizeof(double), strm);
  const double* const zero = buf + L.zero;

  // the adjoint QP: the forward matrices (masked where an input is pinned), q := gx, r := gu,
  // b := 0, x0 := 0; only reg_prim and ric_alg of the settings reach the kernel
  srbd::ProblemArgs a;
  std::memset(&a, 0, sizeof a);
  a.batch = batch;
  a.N = dm.N;
  a.nx = dm.nx;
  a.nu = dm.nu;
  a.A = d->A;
  a.B = d->B;
  a.Q = d->Q;
  a.S = d->S;
  a.R = d->R;
  a.q = gx ? gx : zero;
  a.r = gu ? gu : zero;
  a.b = zero;
  a.x0 = zero;
  a.x = buf + L.dx;
  a.u = buf + L.du;
  a.pi = buf + L.dpi;
  a.ws = h->ws;
  a.ws_qp = h->ws_qp;
  a.reg = st->reg_prim;
  a.ric_alg = st->ric_alg != 0;
  h->bwd_counted = 0;
  if (e == hipSuccess && dm.has_box_u) {
    srbd::BackwardMaskArgs m{};
    m.batch = batch;
    m.N = dm.N;
    m.nx = dm.nx;
    m.nu = dm.nu;
    m.B = d->B;
    m.S = d->S;
    m.R = d->R;
    m.gu = gu;
    m.u = s->u;
    m.lbu = d->lbu;
    m.ubu = d->ubu;
    m.lbu_mask = d->lbu_mask;
    m.ubu_mask = d->ubu_mask;
    m.act_tol = act_tol;
    m.Bm = buf + L.Bm;
    m.Sm = buf + L.Sm;
    m.Rm = buf + L.Rm;
    m.rm = buf + L.rm;
    m.count = reinterpret_cast<int*>(buf + L.count);
    e = srbd::launch_backward_mask(m, strm);
    a.B = m.Bm;
    a.S = m.Sm;
    a.R = m.Rm;
    a.r = m.rm;
    h->bwd_counted = batch;
  }
  // the adjoint is the unconstrained solve, on a handle with boxes too (nx or nu < 12: embedded
  // in 12 x 12 stages like the forward solve)
  srbd::ProblemArgs run = a;
  if (e == hipSuccess && padded) e = srbd::pad_problem<double>(a, h->pad.as<double>(), run, strm);
  if (e == hipSuccess) e = srbd::launch_riccati_unconstr(run, strm);
  if (e == hipSuccess && padded) e = srbd::unpad_solution<double>(a, run, strm);
  if (e == hipSuccess) {
    srbd::BackwardGradArgs ga{};
    ga.batch = batch;
    ga.N = dm.N;
    ga.nx = dm.nx;
    ga.nu = dm.nu;
    ga.x = s->x;
    ga.u = s->u;
    ga.pi = s->pi;
    ga.dx = a.x;
    ga.du = a.u;
    ga.dpi = a.pi;
    ga.A = g->A;
    ga.B = g->B;
    ga.b = g->b;
    ga.Q = g->Q;
    ga.S = g->S;
    ga.R = g->R;
    ga.q = g->q;
    ga.r = g->r;
    ga.x0 = g->x0;
    e = srbd::launch_backward_grad(ga, strm);
  }
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  return SRBD_QP_OK;
}

}  // namespace

extern "C" {

int srbd_qp_solve_backward_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                               const srbd_qp_data_f64* d, const srbd_qp_solution_f64* s, const double* gx,
                               const double* gu, double act_tol, const srbd_qp_grad_f64* g, void* stream) {
  return backward_impl(h, batch, st, d, s, gx, gu, act_tol, g, stream);
}

int srbd_qp_backward_pinned_f64(srbd_qp_handle h, int batch, int* count, void* stream) {
  if (!h) return fail(SRBD_QP_EINVAL, "handle is NULL");
  if (batch < 0) return fail(SRBD_QP_EINVAL, "batch must be >= 0");
  if (batch == 0) return SRBD_QP_OK;
  if (!count) return fail(SRBD_QP_EINVAL, "count is NULL");
  if (!h->dims.has_box_u || batch > h->bwd_counted)
    return fail(SRBD_QP_EINVAL, "no pinned counts: the handle's last backward pass (has_box_u) covered " +
                                    std::to_string(h->bwd_counted) + " QPs");
  srbd::DeviceGuard guard(h->device);
  const BackwardLayout L(h->dims, (size_t)h->capacity);
  const hipError_t e = hipMemcpyAsync(count, h->bwd.as<double>() + L.count, sizeof(int) * (size_t)batch,
                                      hipMemcpyDeviceToDevice, stream_of(h, stream));
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "pinned counts: ", e);
  return SRBD_QP_OK;
}

}  // extern "C"
