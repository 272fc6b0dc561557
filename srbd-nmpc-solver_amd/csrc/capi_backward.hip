// capi_backward.hip -- the backward pass of the device-pointer solve (include/srbd_qp.h:
// srbd_qp_solve_backward_f64, srbd_qp_backward_pinned_f64, and with general rows and the
// gradients of D and the bounds srbd_qp_solve_backward_rows_f64, srbd_qp_backward_active_f64):
// the checks of a call, the adjoint QP's launch arguments, the Riccati solve that is the adjoint,
// and the gradient kernels (qp_backward.hip, qp_backward_rows.hip).  The checks
// and the front half of a call (counts, projection or mask, the adjoint solve) are functions of
// their own, shared with srbd_qp_srbd_solve_backward_f64 (capi_srbd.hip).
#include "capi_handle.h"
#include "qp_backward.h"
#include "qp_backward_rows.h"

#include <cmath>
#include <cstring>
#include <string>

using namespace srbd::capi;

namespace {

// Element (double) offsets of the backward buffer, for `cap` QPs: the adjoint solution, a run
// of zeros (the adjoint's b and x0, and a NULL cotangent), and with input boxes the masked
// stages and the pinned count.  `rows` (srbd_qp_solve_backward_rows_f64): the same stages for
// general rows too, and the three counts per QP behind everything else, so that what the two
// entry points share sits at the same place.
struct BackwardLayout {
  size_t dx, du, dpi, zero, zero_elems, Bm, Sm, Rm, rm, count, active, total;
  BackwardLayout(const srbd_qp_dims& m, size_t cap, bool rows = false) {
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
    Bm = Sm = Rm = rm = count = active = 0;
    if (m.has_box_u || (rows && m.ng > 0)) {
      Bm = take(cap * N * nx * nu);
      Sm = take(cap * N * nu * nx);
      Rm = take(cap * N * nu * nu);
      rm = take(cap * N * nu);
      count = take((cap + 1) / 2);  // ints
    }
    if (rows) active = take((3 * cap + 1) / 2);  // ints
    total = o;
  }
};

}  // namespace

namespace srbd {
namespace capi {

// The checks of a backward call, in the header's order, up to (not including) batch == 0.
int backward_check(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const srbd_qp_data_f64* d,
                   const srbd_qp_solution_f64* s, const double* gx, const double* gu, double act_tol, bool rows,
                   double rank_tol, bool have_grad) {
  // the checks that read the arguments alone come first; the handle is read after them
  if (!h) return fail(SRBD_QP_EINVAL, "handle is NULL");
  if (!d || !s || !have_grad) return fail(SRBD_QP_EINVAL, "data/solution/grad is NULL");
  if (!st) return fail(SRBD_QP_EINVAL, "settings is NULL");
  if (!gx && !gu) return fail(SRBD_QP_EINVAL, "gx and gu are both NULL: no cotangent");
  if (!(act_tol >= 0.0) || !std::isfinite(act_tol))
    return fail(SRBD_QP_EINVAL, "act_tol must be finite and >= 0");
  if (rows && !(rank_tol >= 0.0 && rank_tol < 1.0)) return fail(SRBD_QP_EINVAL, "rank_tol must be in [0, 1)");
  if (!(st->reg_prim >= 0.0)) return fail(SRBD_QP_ESETTINGS, "OcpQpIpmSolverSettings.reg_prim must be non-negative");
  const srbd_qp_dims& dm = h->dims;
  if (rows && dm.ng > 0 && d->C)
    return fail(SRBD_QP_EDIM, "backward: general rows on the states (C != NULL) are not supported");
  if (!rows && dm.ng > 0)
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
  if (dm.ng > 0 && (!d->D || !d->lg || !d->ug))
    return fail(SRBD_QP_EINVAL, "a handle with ng > 0 needs D, lg and ug (the forward call's)");
  return SRBD_QP_OK;
}

// The front half of a backward call that has passed its checks, batch > 0, on the handle's device:
// the counts cleared, the stages projected or masked where an input or a row is active, and the
// adjoint QP solved by launch_riccati_unconstr.  out: where the adjoint solution is, and the lift
// kernel's arguments but for its outputs.
int backward_adjoint(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const srbd_qp_data_f64* d,
                     const srbd_qp_solution_f64* s, const double* gx, const double* gu, double act_tol, bool rows,
                     double rank_tol, hipStream_t strm, BackwardAdjoint* out) {
  const srbd_qp_dims& dm = h->dims;
  const BackwardLayout L(dm, (size_t)h->capacity, rows);
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
  h->bwd_active = 0;
  // what the projection and the lift kernel share: the inputs the active set is a function of
  srbd::BackwardRowsArgs& ra = out->rows;
  ra = srbd::BackwardRowsArgs{};
  if (rows) {
    ra.batch = batch;
    ra.N = dm.N;
    ra.nx = dm.nx;
    ra.nu = dm.nu;
    ra.ng = dm.ng;
    ra.u = s->u;
    if (dm.has_box_u) ra.lbu = d->lbu, ra.ubu = d->ubu, ra.lbu_mask = d->lbu_mask, ra.ubu_mask = d->ubu_mask;
    if (dm.ng > 0) ra.D = d->D, ra.lg = d->lg, ra.ug = d->ug, ra.lg_mask = d->lg_mask, ra.ug_mask = d->ug_mask;
    ra.act_tol = act_tol;
    ra.rank_tol = rank_tol;
    ra.B = d->B;
    ra.S = d->S;
    ra.R = d->R;
    ra.gu = gu;
    ra.count = reinterpret_cast<int*>(buf + L.active);
    if (e == hipSuccess) e = hipMemsetAsync(ra.count, 0, 3 * sizeof(int) * (size_t)batch, strm);
    if (e == hipSuccess && (dm.has_box_u || dm.ng > 0)) {
      ra.Bm = buf + L.Bm;
      ra.Sm = buf + L.Sm;
      ra.Rm = buf + L.Rm;
      ra.rm = buf + L.rm;
      e = srbd::launch_backward_project(ra, strm);
      a.B = ra.Bm;
      a.S = ra.Sm;
      a.R = ra.Rm;
      a.r = ra.rm;
    }
    h->bwd_active = batch;
  } else if (e == hipSuccess && dm.has_box_u) {
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
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  out->dx = a.x;
  out->du = a.u;
  out->dpi = a.pi;
  ra.x = s->x;
  ra.pi = s->pi;
  ra.r = d->r;
  ra.dx = a.x;
  ra.du = a.u;
  ra.dpi = a.pi;
  return SRBD_QP_OK;
}

}  // namespace capi
}  // namespace srbd

namespace {

int backward_impl(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const srbd_qp_data_f64* d,
                  const srbd_qp_solution_f64* s, const double* gx, const double* gu, double act_tol,
                  const srbd_qp_grad_f64* g, void* stream, bool rows = false, double rank_tol = 0.0,
                  const srbd_qp_grad_rows_f64* gr = nullptr) {
  if (const int rc = backward_check(h, batch, st, d, s, gx, gu, act_tol, rows, rank_tol, g || gr)) return rc;
  if (batch == 0) return SRBD_QP_OK;

  hipStream_t strm = stream_of(h, stream);
  srbd::DeviceGuard guard(h->device);
  const srbd_qp_dims& dm = h->dims;
  BackwardAdjoint adj;
  if (const int rc = backward_adjoint(h, batch, st, d, s, gx, gu, act_tol, rows, rank_tol, strm, &adj)) return rc;
  hipError_t e = hipSuccess;
  if (gr) {
    srbd::BackwardRowsArgs& ra = adj.rows;
    ra.gD = gr->D;
    ra.glg = gr->lg;
    ra.gug = gr->ug;
    ra.glbu = gr->lbu;
    ra.gubu = gr->ubu;
    e = srbd::launch_backward_lift(ra, strm);
  }
  if (e == hipSuccess && g) {
    srbd::BackwardGradArgs ga{};
    ga.batch = batch;
    ga.N = dm.N;
    ga.nx = dm.nx;
    ga.nu = dm.nu;
    ga.x = s->x;
    ga.u = s->u;
    ga.pi = s->pi;
    ga.dx = adj.dx;
    ga.du = adj.du;
    ga.dpi = adj.dpi;
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

int srbd_qp_solve_backward_rows_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                                    const srbd_qp_data_f64* d, const srbd_qp_solution_f64* s, const double* gx,
                                    const double* gu, double act_tol, double rank_tol, const srbd_qp_grad_f64* g,
                                    const srbd_qp_grad_rows_f64* gr, void* stream) {
  return backward_impl(h, batch, st, d, s, gx, gu, act_tol, g, stream, true, rank_tol, gr);
}

int srbd_qp_backward_active_f64(srbd_qp_handle h, int batch, int* count, void* stream) {
  if (!h) return fail(SRBD_QP_EINVAL, "handle is NULL");
  if (batch < 0) return fail(SRBD_QP_EINVAL, "batch must be >= 0");
  if (batch == 0) return SRBD_QP_OK;
  if (!count) return fail(SRBD_QP_EINVAL, "count is NULL");
  if (batch > h->bwd_active)
    return fail(SRBD_QP_EINVAL, "no active-set counts: the handle's last srbd_qp_solve_backward_rows_f64 covered " +
                                    std::to_string(h->bwd_active) + " QPs");
  srbd::DeviceGuard guard(h->device);
  const BackwardLayout L(h->dims, (size_t)h->capacity, true);
  const hipError_t e = hipMemcpyAsync(count, h->bwd.as<double>() + L.active, 3 * sizeof(int) * (size_t)batch,
                                      hipMemcpyDeviceToDevice, stream_of(h, stream));
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "active-set counts: ", e);
  return SRBD_QP_OK;
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
