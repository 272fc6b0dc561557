// capi_srbd.hip -- the SRBD entry points of the C-ABI (include/srbd_qp.h, srbd_qp_srbd_*):
// robots, terrain and the plant's contact model, linearisation and its backward passes, line search, the NMPC
// step, the plant step, the gait planner, the closed-loop rollout, and the open-loop plant rollout with its adjoint.
#include "capi_handle.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>

using namespace srbd::capi;

namespace {
// What the batched SRBD calls check first: 12 x 12 stages (`needs`: the call's own message) and
// the batch against the handle's capacity.
int check_srbd_call(srbd_qp_handle h, int batch, const char* needs) {
  if (h->dims.nx != 12 || h->dims.nu != 12) return fail(SRBD_QP_EDIM, needs);
  if (batch < 0 || batch > h->capacity) return fail(SRBD_QP_ECAPACITY, "batch exceeds capacity");
  return SRBD_QP_OK;
}
// the caller's parameters with qf_scale's default (N) filled in
srbd_model_params with_qf_scale(const srbd_model_params* params, int N) {
  srbd_model_params p = *params;
  if (p.qf_scale <= 0.0) p.qf_scale = (double)N;
  return p;
}
}  // namespace

extern "C" {

void srbd_qp_srbd_default_params(srbd_model_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  const double Q[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 10};
  const double Qf[12] = {0.5, 0.5, 0.5, 0.01, 0.01, 0.01, 100, 100, 100, 0.0, 0.0, 100.0};
  const double xr[12] = {0, 0, 0.2, 0, 0, 0, 0.5, 0, 1.0, 0, 0, 0};
  const double lo[6] = {-50.0, -50.0, 0.0, -5.0, -5.0, -5.0}, hi[6] = {50.0, 50.0, 300.0, 5.0, 5.0, 5.0};
  for (int i = 0; i < 12; ++i) {
    p->Q[i] = Q[i];
    p->Qf[i] = Qf[i];
    p->x_ref[i] = xr[i];
    p->u_lo[i] = lo[i % 6];
    p->u_hi[i] = hi[i % 6];
  }
  p->R = 0.0001;
  p->dt = 0.015;
  p->Lbody[0] = 0.541667;
  p->Lbody[1] = 0.516667;
  p->Lbody[2] = 1.0416667;
  p->mu_b = 0.1;
  p->theta_b = 5.0;
  p->mass = 15.0;
  p->foot_r[1] = -0.1;
  p->foot_l[1] = 0.1;
  p->mu = 0.5;
  p->Lfx = 0.05;
  p->Lfz = 0.05;
  p->fmax = 1000.0;
  p->fmin = 0.0;
  p->qf_scale = 0.0;  // N
}

int srbd_qp_srbd_set_robots_f64(srbd_qp_handle h, int role, const srbd_robots_f64* robots) {
  if (!h) return fail(SRBD_QP_EINVAL, "handle is NULL");
  if (role != SRBD_QP_ROBOTS_MODEL && role != SRBD_QP_ROBOTS_PLANT)
    return fail(SRBD_QP_EINVAL, "set_robots: unknown role " + std::to_string(role));
  if (h->dims.nx != 12 || h->dims.nu != 12) return fail(SRBD_QP_EDIM, "SRBD robots need nx = nu = 12");
  const srbd_robots_f64 r = robots ? *robots : srbd_robots_f64{};
  if (role == SRBD_QP_ROBOTS_PLANT && (r.mu || r.Q || r.Qf || r.R))
    return fail(SRBD_QP_EINVAL, "set_robots: the PLANT role takes mass and Lbody only");
  (role == SRBD_QP_ROBOTS_MODEL ? h->robots_model : h->robots_plant) = r;
  return SRBD_QP_OK;
}

}  // extern "C"

namespace {
// the checks of a height map's grid that set_terrain and set_contact (its true ground) share
int check_grid(const srbd_terrain_f64& t, const std::string& who) {
  if (t.maps < 1) return fail(SRBD_QP_EINVAL, who + ": maps must be at least 1");
  if (t.nx < 2 || t.ny < 2) return fail(SRBD_QP_EINVAL, who + ": nx and ny must be at least 2");
  if (!(t.cell > 0.0) || !std::isfinite(t.cell)) return fail(SRBD_QP_EINVAL, who + ": cell must be positive");
  if (!std::isfinite(t.x0) || !std::isfinite(t.y0)) return fail(SRBD_QP_EINVAL, who + ": x0, y0 must be finite");
  return SRBD_QP_OK;
}
}  // namespace

extern "C" {

int srbd_qp_srbd_set_terrain_f64(srbd_qp_handle h, const srbd_terrain_f64* terrain) {
  if (!h) return fail(SRBD_QP_EINVAL, "handle is NULL");
  if (h->dims.nx != 12 || h->dims.nu != 12) return fail(SRBD_QP_EDIM, "SRBD terrain needs nx = nu = 12");
  if (!terrain || !terrain->height) {
    h->terrain = srbd_terrain_f64{};
    return SRBD_QP_OK;
  }
  const srbd_terrain_f64& t = *terrain;
  if (const int rc = check_grid(t, "set_terrain")) return rc;
  if (t.search < 0 || t.search > 3) return fail(SRBD_QP_EINVAL, "set_terrain: search must be in 0..3");
  if (!(t.w_rough >= 0.0) || !std::isfinite(t.w_rough))
    return fail(SRBD_QP_EINVAL, "set_terrain: w_rough must be non-negative and finite");
  h->terrain = t;
  return SRBD_QP_OK;
}

int srbd_qp_srbd_terrain_height_f64(srbd_qp_handle h, int n, const double* xy, const int* map, double* out,
                                    void* stream) {
  if (!h) return fail(SRBD_QP_EINVAL, "handle is NULL");
  if (!h->terrain.height) return fail(SRBD_QP_EINVAL, "terrain_height: no terrain is set");
  if (n < 0) return fail(SRBD_QP_EINVAL, "terrain_height: n must be non-negative");
  if (n == 0) return SRBD_QP_OK;  // nothing is read: empty arrays may be NULL
  if (!xy || !out) return fail(SRBD_QP_EINVAL, "NULL argument");
  hipStream_t strm = stream_of(h, stream);
  srbd::DeviceGuard guard(h->device);
  const hipError_t e = srbd::launch_srbd_terrain_height(h->terrain, n, xy, map, out, strm);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  return SRBD_QP_OK;
}

int srbd_qp_srbd_set_contact_f64(srbd_qp_handle h, const srbd_contact_f64* contact) {
  if (!h) return fail(SRBD_QP_EINVAL, "handle is NULL");
  if (h->dims.nx != 12 || h->dims.nu != 12) return fail(SRBD_QP_EDIM, "the SRBD contact model needs nx = nu = 12");
  if (!contact) {
    h->contact = srbd_contact_f64{};
    h->has_contact = false;
    return SRBD_QP_OK;
  }
  const srbd_contact_f64& c = *contact;
  auto bound = [](double v) { return v >= 0.0 && std::isfinite(v); };  // (false for a NaN)
  if (!c.mu_r && !bound(c.mu)) return fail(SRBD_QP_EINVAL, "set_contact: mu must be non-negative and finite");
  if (!bound(c.Ltx) || !bound(c.Lty) || !bound(c.Ltz))
    return fail(SRBD_QP_EINVAL, "set_contact: Ltx, Lty, Ltz must be non-negative and finite");
  if (!(c.fz_hi > 0.0)) return fail(SRBD_QP_EINVAL, "set_contact: fz_hi must be positive");
  if (!bound(c.fz_contact)) return fail(SRBD_QP_EINVAL, "set_contact: fz_contact must be non-negative and finite");
  if (!std::isfinite(c.ground_z) || !std::isfinite(c.z_min))
    return fail(SRBD_QP_EINVAL, "set_contact: ground_z and z_min must be finite");
  if (!(c.cos_tilt_min >= -1.0 && c.cos_tilt_min <= 1.0))
    return fail(SRBD_QP_EINVAL, "set_contact: cos_tilt_min must be in [-1, 1]");
  if (c.alive && !c.fallen) return fail(SRBD_QP_EINVAL, "set_contact: alive needs fallen");
  if (c.ground.height) {
    if (const int rc = check_grid(c.ground, "set_contact: ground")) return rc;
  }
  h->contact = c;
  h->has_contact = true;
  return SRBD_QP_OK;
}

int srbd_qp_srbd_set_active_f64(srbd_qp_handle h, const srbd_active_f64* active) {
  if (!h) return fail(SRBD_QP_EINVAL, "handle is NULL");
  if (h->dims.nx != 12 || h->dims.nu != 12) return fail(SRBD_QP_EDIM, "an SRBD active set needs nx = nu = 12");
  const srbd_active_f64 a = active ? *active : srbd_active_f64{};
  if ((a.skip_fallen != 0 && a.skip_fallen != 1) || (a.compact != 0 && a.compact != 1))
    return fail(SRBD_QP_EINVAL, "set_active: skip_fallen and compact must be 0 or 1");
  h->active = a;
  h->has_active = a.mask || a.skip_fallen || a.compact;
  return SRBD_QP_OK;
}

int srbd_qp_srbd_step_work(srbd_qp_handle h, long long* qp_solves, long long* sqp_iterations) {
  if (!h) return fail(SRBD_QP_EINVAL, "handle is NULL");
  if (qp_solves) *qp_solves = h->work_qp_solves;
  if (sqp_iterations) *sqp_iterations = h->work_sqp_iterations;
  return SRBD_QP_OK;
}

// The _plan_ entry points hold the checks and the work; the plain ones forward a NULL plan.
// All of them read the handle's robots (srbd_qp_srbd_set_robots_f64).
int srbd_qp_srbd_linearize_plan_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                    const srbd_plan_f64* plan, int constraints, const double* xs,
                                    const double* us, const srbd_qp_data_f64* out, void* stream) {
  if (!h || !params || !xs || !us || !out) return fail(SRBD_QP_EINVAL, "NULL argument");
  const srbd_qp_dims& d = h->dims;
  if (const int rc = check_srbd_call(h, batch, "SRBD linearisation needs nx = nu = 12")) return rc;
  if (constraints < SRBD_QP_SRBD_NONE || constraints > SRBD_QP_SRBD_CONE)
    return fail(SRBD_QP_EINVAL, "unknown constraints mode");
  if (!out->A || !out->B || !out->b || !out->Q || !out->S || !out->R || !out->q || !out->r)
    return fail(SRBD_QP_EINVAL, "A, B, b, Q, S, R, q, r outputs are required");
  if (constraints == SRBD_QP_SRBD_BOX_U && (!out->lbu || !out->ubu))
    return fail(SRBD_QP_EINVAL, "BOX_U needs lbu / ubu outputs");
  if (constraints == SRBD_QP_SRBD_CONE &&
      (d.ng != 24 || !out->D || !out->lg || !out->ug || !out->lg_mask || !out->ug_mask))
    return fail(SRBD_QP_EINVAL, "CONE needs ng = 24 and D, lg, ug, lg_mask, ug_mask outputs (C optional)");
  const srbd_model_params p = with_qf_scale(params, d.N);
  hipStream_t strm = stream_of(h, stream);
  srbd::DeviceGuard guard(h->device);
  const hipError_t e = srbd::launch_srbd_linearize(p, batch, d.N, constraints, xs, us, *out, strm, plan,
                                                   &h->robots_model);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  return SRBD_QP_OK;
}
int srbd_qp_srbd_linearize_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                               int constraints, const double* xs, const double* us,
                               const srbd_qp_data_f64* out, void* stream) {
  return srbd_qp_srbd_linearize_plan_f64(h, batch, params, nullptr, constraints, xs, us, out, stream);
}

// The backward pass of the linearisation: the forward call's checks in its order, then the
// outputs; the robots' sums go through a scratch row per stage.
int srbd_qp_srbd_linearize_backward_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                        const srbd_plan_f64* plan, int constraints, const double* xs,
                                        const double* us, const srbd_qp_data_f64* cot,
                                        const srbd_lin_grad_f64* grad, void* stream) {
  if (!h || !params || !xs || !us || !cot || !grad) return fail(SRBD_QP_EINVAL, "NULL argument");
  const srbd_qp_dims& d = h->dims;
  if (const int rc = check_srbd_call(h, batch, "SRBD linearisation needs nx = nu = 12")) return rc;
  if (constraints < SRBD_QP_SRBD_NONE || constraints > SRBD_QP_SRBD_CONE)
    return fail(SRBD_QP_EINVAL, "unknown constraints mode");
  if (constraints == SRBD_QP_SRBD_CONE && d.ng != 24) return fail(SRBD_QP_EINVAL, "CONE needs ng = 24");
  const srbd_lin_grad_f64& g = *grad;
  const bool sums = g.mass || g.Lbody || g.mu || g.R;
  if (!sums && !g.Q && !g.Qf && !g.x_ref && !g.foot_r && !g.foot_l && !g.fz_max)
    return fail(SRBD_QP_EINVAL, "linearize_backward: every output of grad is NULL");
  if (batch == 0) return SRBD_QP_OK;
  const srbd_model_params p = with_qf_scale(params, d.N);
  hipStream_t strm = stream_of(h, stream);
  srbd::DeviceGuard guard(h->device);
  if (sums) {
    const hipError_t e = h->lin_bwd.reserve(srbd::lin_backward_part_elems(h->capacity, d.N) * sizeof(double));
    if (e != hipSuccess) return hip_fail(alloc_code(e), "linearize_backward scratch allocation failed: ", e);
  }
  const hipError_t e = srbd::launch_srbd_linearize_backward(p, batch, d.N, constraints, xs, us, *cot, g,
                                                            h->lin_bwd.as<double>(), strm, plan, &h->robots_model);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  return SRBD_QP_OK;
}

// The two backward passes in one: the linearisation's checks, then the solve's,
// then the outputs; the front half of srbd_qp_solve_backward_rows_f64, the lift kernel into the
// handle's compact rows, and the fused kernels that read the vectors where they are.
int srbd_qp_srbd_solve_backward_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* settings,
                                    const srbd_model_params* params, const srbd_plan_f64* plan, int constraints,
                                    const double* xs, const double* us, const srbd_qp_data_f64* data,
                                    const srbd_qp_solution_f64* sol, const double* gx, const double* gu,
                                    double act_tol, double rank_tol, const srbd_lin_grad_f64* grad,
                                    double* grad_x0, void* stream) {
  if (!h || !params || !xs || !us || !grad) return fail(SRBD_QP_EINVAL, "NULL argument");
  const srbd_qp_dims& d = h->dims;
  if (const int rc = check_srbd_call(h, batch, "SRBD linearisation needs nx = nu = 12")) return rc;
  if (constraints < SRBD_QP_SRBD_NONE || constraints > SRBD_QP_SRBD_CONE)
    return fail(SRBD_QP_EINVAL, "unknown constraints mode");
  if (constraints == SRBD_QP_SRBD_CONE && d.ng != 24) return fail(SRBD_QP_EINVAL, "CONE needs ng = 24");
  if (const int rc = backward_check(h, batch, settings, data, sol, gx, gu, act_tol, true, rank_tol, true)) return rc;
  const srbd_lin_grad_f64& g = *grad;
  const bool sums = g.mass || g.Lbody || g.mu || g.R;
  if (!sums && !g.Q && !g.Qf && !g.x_ref && !g.foot_r && !g.foot_l && !g.fz_max && !grad_x0)
    return fail(SRBD_QP_EINVAL, "srbd_solve_backward: every output of grad and grad_x0 are NULL");
  if (batch == 0) return SRBD_QP_OK;
  const srbd_model_params p = with_qf_scale(params, d.N);
  hipStream_t strm = stream_of(h, stream);
  srbd::DeviceGuard guard(h->device);
  // the compact rows: nu, dnu of the cone's rows, then the gradient of ubu
  const size_t stages = (size_t)h->capacity * (size_t)d.N;
  const size_t row_elems = stages * (size_t)d.ng, box_elems = d.has_box_u ? stages * (size_t)d.nu : 0;
  hipError_t e = hipSuccess;
  if (sums) e = h->lin_bwd.reserve(srbd::lin_backward_part_elems(h->capacity, d.N) * sizeof(double));
  if (e == hipSuccess) e = h->bwd_fused.reserve((2 * row_elems + box_elems) * sizeof(double));
  if (e != hipSuccess) return hip_fail(alloc_code(e), "srbd_solve_backward scratch allocation failed: ", e);
  BackwardAdjoint adj;
  if (const int rc = backward_adjoint(h, batch, settings, data, sol, gx, gu, act_tol, true, rank_tol, strm, &adj))
    return rc;
  srbd::SolveBwdVecs v{};
  v.x = sol->x;
  v.u = sol->u;
  v.pi = sol->pi;
  v.dx = adj.dx;
  v.du = adj.du;
  v.dpi = adj.dpi;
  v.gx0 = grad_x0;
  double* const rows = h->bwd_fused.as<double>();
  const bool stage_outputs = sums || g.foot_r || g.foot_l || g.fz_max;
  if (stage_outputs && constraints == SRBD_QP_SRBD_CONE) {  // (ng = 24: checked)
    adj.rows.nu_out = rows;
    adj.rows.dnu_out = rows + row_elems;
    v.nu = adj.rows.nu_out;
    v.dnu = adj.rows.dnu_out;
  }
  if (stage_outputs && constraints == SRBD_QP_SRBD_BOX_U && d.has_box_u) {
    adj.rows.gubu = rows + 2 * row_elems;
    v.gubu = adj.rows.gubu;
  }
  e = srbd::launch_backward_lift(adj.rows, strm);  // (no output: no launch)
  if (e == hipSuccess)
    e = srbd::launch_srbd_solve_backward(p, batch, d.N, constraints, xs, us, v, g, h->lin_bwd.as<double>(), strm, plan,
                                         &h->robots_model);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  return SRBD_QP_OK;
}

void srbd_qp_srbd_default_linesearch(srbd_linesearch_params* p) {
  if (!p) return;
  p->theta_max = 1e-6;
  p->theta_min = 5e-10;
  p->eta = 1e-4;
  p->beta_phi = 1e-6;
  p->beta_theta = 1e-6;
  p->beta_alpha = 0.5;
  p->alpha_min = 1e-4;
}

int srbd_qp_srbd_linesearch_plan_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                     const srbd_plan_f64* plan, const srbd_linesearch_params* ls,
                                     double* xs, double* us, const double* dx, const double* du,
                                     double* alpha, double* merit, int* converged, void* stream) {
  if (!h || !params || !ls || !xs || !us || !dx || !du || !alpha)
    return fail(SRBD_QP_EINVAL, "NULL argument");
  const srbd_qp_dims& d = h->dims;
  if (const int rc = check_srbd_call(h, batch, "SRBD line search needs nx = nu = 12")) return rc;
  if (!(ls->beta_alpha > 0.0 && ls->beta_alpha < 1.0) || !(ls->alpha_min > 0.0))
    return fail(SRBD_QP_EINVAL, "line search needs 0 < beta_alpha < 1 and alpha_min > 0");
  const srbd_model_params p = with_qf_scale(params, d.N);
  hipStream_t strm = stream_of(h, stream);
  srbd::DeviceGuard guard(h->device);
  const hipError_t e = srbd::launch_srbd_linesearch(p, *ls, batch, d.N, xs, us, dx, du, alpha,
                                                    merit, converged, strm, nullptr, plan, &h->robots_model);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  return SRBD_QP_OK;
}
int srbd_qp_srbd_linesearch_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                const srbd_linesearch_params* ls, double* xs, double* us,
                                const double* dx, const double* du, double* alpha, double* merit,
                                int* converged, void* stream) {
  return srbd_qp_srbd_linesearch_plan_f64(h, batch, params, nullptr, ls, xs, us, dx, du, alpha, merit,
                                          converged, stream);
}

}  // extern "C"

namespace {
// The NMPC step (srbd_qp_srbd_nmpc_plan_f64).  add_work: a rollout's tick, whose work is added
// to the handle's counters (srbd_qp_srbd_step_work); a step of its own starts them at zero.
int nmpc_step(srbd_qp_handle h, int batch, const srbd_model_params* params, const srbd_plan_f64* plan,
              const srbd_linesearch_params* ls, const srbd_qp_settings* settings, int constraints,
              int sqp_max_loop, double* xs, double* us, const double* x0, double* alpha, int* sqp_iter,
              int* converged, bool add_work) {
  if (!h || !params || !ls || !settings || !xs || !us || !x0 || !alpha || !sqp_iter || !converged)
    return fail(SRBD_QP_EINVAL, "NULL argument");
  const srbd_qp_dims& d = h->dims;
  int rc = check_srbd_call(h, batch, "the SRBD NMPC loop needs nx = nu = 12");
  if (rc) return rc;
  if (sqp_max_loop < 0) return fail(SRBD_QP_EINVAL, "sqp_max_loop must be non-negative");
  if (constraints < SRBD_QP_SRBD_NONE || constraints > SRBD_QP_SRBD_CONE)
    return fail(SRBD_QP_EINVAL, "unknown constraints mode");
  const bool box = constraints == SRBD_QP_SRBD_BOX_U, cone = constraints == SRBD_QP_SRBD_CONE;
  if ((d.has_box_u != 0) != box || (d.ng > 0) != cone || d.has_box_x || (cone && d.ng != 24))
    return fail(SRBD_QP_EINVAL, "the handle's dims do not match the constraints mode");
  rc = srbd_qp_check_settings(settings);
  if (rc) return rc;
  // the active set (srbd_qp_srbd_set_active_f64): act false is the step without one
  const bool act = h->has_active, compact = act && h->active.compact;
  if (act && h->active.skip_fallen && !(h->has_contact && h->contact.fallen))
    return fail(SRBD_QP_EINVAL, "active set: skip_fallen needs a contact with fallen on the handle");
  if (compact && settings->warm_start != 0)
    return fail(SRBD_QP_EINVAL, "active set: compact does not go with settings.warm_start");
  if (!add_work) h->work_qp_solves = h->work_sqp_iterations = 0;
  if (batch == 0 || sqp_max_loop == 0) return SRBD_QP_OK;
  srbd::DeviceGuard guard(h->device);
  hipStream_t strm = h->stream;
  // scratch: QP data (linearisation), x0 - x_nmpc(:,0), QP solution, loop state
  const size_t B = (size_t)h->capacity, N = (size_t)d.N;
  struct Buf { size_t off, n; };
  size_t top = 0;
  auto take = [&](size_t n) { Buf b{top, n}; top += (n + 31) / 32 * 32; return b; };
  const Buf bA = take(B * N * 144), bB = take(B * N * 144), bb = take(B * N * 12),
            bQ = take(B * (N + 1) * 144), bS = take(B * N * 144), bR = take(B * N * 144),
            bq = take(B * (N + 1) * 12), br = take(B * N * 12);
  const Buf blbu = take(box ? B * N * 12 : 0), bubu = take(box ? B * N * 12 : 0);
  const Buf bD = take(cone ? B * N * 288 : 0), blg = take(cone ? B * (N + 1) * 24 : 0),
            bug = take(cone ? B * (N + 1) * 24 : 0), blgm = take(cone ? B * (N + 1) * 24 : 0),
            bugm = take(cone ? B * (N + 1) * 24 : 0);
  const Buf bx0 = take(B * 12), bx = take(B * (N + 1) * 12), bu = take(B * N * 12),
            bpi = take(B * (N + 1) * 12);
  const Buf bint = take(B * 4 + 8);  // conv, done, status, iter (ints) + active
  const Buf bidx = take(act ? B : 0);  // an active set's two lists of B ints
  hipError_t e = h->nmpc.reserve(top * sizeof(double));
  if (e == hipSuccess && !h->nmpc_active_host)
    e = hipHostMalloc(reinterpret_cast<void**>(&h->nmpc_active_host), sizeof(int));
  if (e != hipSuccess) return hip_fail(alloc_code(e), "NMPC scratch allocation failed: ", e);
  double* base = h->nmpc.as<double>();
  auto at = [&](const Buf& b) -> double* { return b.n ? base + b.off : nullptr; };
  srbd_qp_data_f64 qd{};
  qd.A = at(bA); qd.B = at(bB); qd.b = at(bb); qd.Q = at(bQ); qd.S = at(bS); qd.R = at(bR);
  qd.q = at(bq); qd.r = at(br); qd.lbu = at(blbu); qd.ubu = at(bubu);
  qd.D = at(bD); qd.lg = at(blg); qd.ug = at(bug); qd.lg_mask = at(blgm); qd.ug_mask = at(bugm);
  qd.x0 = at(bx0);
  int* ints = reinterpret_cast<int*>(at(bint));
  int *conv = ints, *done = ints + B, *status = ints + 2 * B, *iters = ints + 3 * B,
      *active = ints + 4 * B;
  srbd_qp_solution_f64 sol{};
  sol.x = at(bx); sol.u = at(bu); sol.pi = at(bpi); sol.status = status; sol.iter = iters;
  const srbd_model_params p = with_qf_scale(params, d.N);
  // the count of robots still iterating, through the 4-byte read-back
  auto read_active = [&]() {
    hipError_t r = hipMemcpyAsync(h->nmpc_active_host, active, sizeof(int), hipMemcpyDeviceToHost, strm);
    return r == hipSuccess ? hipStreamSynchronize(strm) : r;
  };
  // With an active set the first list says who is stepped (and writes every robot's loop state);
  // n: the QPs of an iteration, cur / next: its robots and the next one's (compact only).
  int n = batch;
  int *cur = reinterpret_cast<int*>(at(bidx)), *next = cur ? cur + B : nullptr;
  if (act) {
    e = srbd::launch_nmpc_select_first(batch, h->active.mask, h->active.skip_fallen ? h->contact.fallen : nullptr,
                                       done, sqp_iter, converged, cur, active, strm);
    if (e == hipSuccess) e = read_active();
    if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "NMPC loop: ", e);
    if (*h->nmpc_active_host == 0) return SRBD_QP_OK;  // nobody is stepped
    if (compact) n = *h->nmpc_active_host;
  }
  // NMPC_solver.cpp:362-372: prepareQpStructures; solveQpProblems; if (checkConvergence()) break;
  for (int it = 0; it < sqp_max_loop && e == hipSuccess; ++it) {
    const int* idx = compact ? cur : nullptr;  // QP j is robot idx[j]; NULL: robot j
    e = srbd::launch_srbd_linearize(p, n, d.N, constraints, xs, us, qd, strm, plan, &h->robots_model, idx);
    if (e == hipSuccess)
      e = srbd::launch_nmpc_prep(n, d.N, !act && it == 0, xs, x0, at(bx0), done, sqp_iter, converged, strm, idx);
    if (e != hipSuccess) break;
    // A compacted unconstrained iteration is solved by the kernel the whole batch takes: the
    // streaming Riccati kernel also for the few QPs left of a batch above the single-QP kernels'
    // limit.  A robot then has the bits of the step without compaction, at any batch size.
    h->riccati_streaming = compact && !box && !cone && batch > srbd::riccati_single_qp_batch_max();
    rc = srbd_qp_solve_f64(h, n, settings, &qd, &sol, strm);
    h->riccati_streaming = false;
    if (rc) return rc;
    h->work_qp_solves += n;
    h->work_sqp_iterations += 1;
    e = srbd::launch_srbd_linesearch(p, *ls, n, d.N, xs, us, at(bx), at(bu), alpha, nullptr,
                                     conv, strm, done, plan, &h->robots_model, idx);
    if (e == hipSuccess)
      e = compact ? srbd::launch_nmpc_select_next(n, it, cur, conv, done, sqp_iter, converged, next, active, strm)
                  : srbd::launch_nmpc_after(batch, it, conv, done, sqp_iter, converged, active, strm);
    if (e == hipSuccess) e = read_active();
    if (e == hipSuccess && *h->nmpc_active_host == 0) break;  // every robot has converged
    if (e == hipSuccess && compact) {
      n = *h->nmpc_active_host;
      std::swap(cur, next);
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(strm);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "NMPC loop: ", e);
  return SRBD_QP_OK;
}
}  // namespace

extern "C" {

int srbd_qp_srbd_nmpc_plan_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                               const srbd_plan_f64* plan, const srbd_linesearch_params* ls,
                               const srbd_qp_settings* settings, int constraints, int sqp_max_loop,
                               double* xs, double* us, const double* x0, double* alpha,
                               int* sqp_iter, int* converged) {
  return nmpc_step(h, batch, params, plan, ls, settings, constraints, sqp_max_loop, xs, us, x0, alpha, sqp_iter,
                   converged, false);
}
int srbd_qp_srbd_nmpc_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                          const srbd_linesearch_params* ls, const srbd_qp_settings* settings,
                          int constraints, int sqp_max_loop, double* xs, double* us,
                          const double* x0, double* alpha, int* sqp_iter, int* converged) {
  return srbd_qp_srbd_nmpc_plan_f64(h, batch, params, nullptr, ls, settings, constraints, sqp_max_loop,
                                    xs, us, x0, alpha, sqp_iter, converged);
}

}  // extern "C"

// ---- the closed loop and the gait planner (4.7e) ----
// A single step is tick 0 of 1: tick t of a rollout of T reads column t of its per-tick
// inputs ([batch][T][...]) and writes column t of its logs, through the launches' strides.
namespace {
// the plant step of tick t of T: wrench [batch][T][6], u_out [batch][T][12] (either may be NULL)
srbd::AdvanceIo advance_io(int substeps, double* xs, double* us, double* x, const double* wrench, double* u_out,
                           int t, int T) {
  srbd::AdvanceIo io{};
  io.substeps = substeps;
  io.xs = xs;
  io.us = us;
  io.x = x;
  io.wrench = wrench ? wrench + (size_t)t * 6 : nullptr;
  io.wrench_stride = (long long)T * 6;
  io.u_out = u_out ? u_out + (size_t)t * 12 : nullptr;
  io.u_stride = (long long)T * 12;
  return io;
}

// the planner's launch of tick t of T: cmd [batch][T][4], the window it writes (all four arrays)
srbd::GaitIo gait_io(const double* cmd, const double* x, long long tick, double* ref_pose, double* foot_now,
                     const srbd_plan_f64& window, int t, int T) {
  srbd::GaitIo io{};
  io.cmd = cmd + (size_t)t * 4;
  io.cmd_stride = (long long)T * 4;
  io.x = x;
  io.tick = tick;
  io.ref_pose = ref_pose;
  io.foot_now = foot_now;
  io.x_ref = const_cast<double*>(window.x_ref);
  io.foot_r = const_cast<double*>(window.foot_r);
  io.foot_l = const_cast<double*>(window.foot_l);
  io.fz_max = const_cast<double*>(window.fz_max);
  return io;
}
}  // namespace

extern "C" {

// (these two have always been inside extern "C": the library exports their names)
namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the host checks of srbd_qp_srbd_gait_plan_f64 that the replanning rollout shares
int check_gait(srbd_qp_handle h, int batch, const srbd_gait_f64* g, long long tick) {
  if (const int rc = check_srbd_call(h, batch, "the SRBD gait planner needs nx = nu = 12")) return rc;
  if (tick < 0) return fail(SRBD_QP_EINVAL, "gait: tick must be non-negative");
  if (!g->period_r && g->period < 1) return fail(SRBD_QP_EINVAL, "gait: period must be at least 1");
  for (int f = 0; f < 2; ++f) {
    // against the scalar period only where every robot has that period
    if (!g->swing_r && (g->swing[f] < 0 || (!g->period_r && g->swing[f] >= g->period)))
      return fail(SRBD_QP_EINVAL, "gait: swing must be in [0, period)");
    if (!g->offset_r && g->offset[f] < 0) return fail(SRBD_QP_EINVAL, "gait: offset must be non-negative");
  }
  if (!(g->fz_swing > 0.0)) return fail(SRBD_QP_EINVAL, "gait: fz_swing must be positive");
  if (!(g->fz_stance > g->fz_swing)) return fail(SRBD_QP_EINVAL, "gait: fz_stance must exceed fz_swing");
  return SRBD_QP_OK;
}
}  // namespace

int srbd_qp_srbd_advance_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                             const srbd_plan_f64* plan, const srbd_advance_f64* adv, double* xs,
                             double* us, double* x, double* u_applied, void* stream) {
  if (!h || !params || !adv || !xs || !us) return fail(SRBD_QP_EINVAL, "NULL argument");
  if (adv->substeps < 1) return fail(SRBD_QP_EINVAL, "advance: substeps must be at least 1");
  if (const int rc = check_srbd_call(h, batch, "the SRBD plant step needs nx = nu = 12")) return rc;
  if (!aligned16(xs) || !aligned16(us)) return fail(SRBD_QP_EINVAL, "advance: xs / us must be 16-byte aligned");
  if (batch == 0) return SRBD_QP_OK;
  hipStream_t strm = stream_of(h, stream);
  srbd::DeviceGuard guard(h->device);
  const srbd::AdvanceIo io = advance_io(adv->substeps, xs, us, x, adv->wrench, u_applied, 0, 1);
  const hipError_t e = srbd::launch_srbd_advance(*params, batch, h->dims.N, io, plan, strm, &h->robots_model,
                                                 &h->robots_plant, h->has_contact ? &h->contact : nullptr);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  return SRBD_QP_OK;
}

int srbd_qp_srbd_gait_plan_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                               const srbd_gait_f64* gait, const double* cmd, const double* x, long long tick,
                               double* ref_pose, double* foot_now, double* x_ref, double* foot_r,
                               double* foot_l, double* fz_max, void* stream) {
  if (!h || !params || !gait || !cmd || !x || !ref_pose || !foot_now || !x_ref || !foot_r || !foot_l || !fz_max)
    return fail(SRBD_QP_EINVAL, "NULL argument");
  const int rc = check_gait(h, batch, gait, tick);
  if (rc) return rc;
  if (!aligned16(x_ref) || !aligned16(fz_max))
    return fail(SRBD_QP_EINVAL, "gait: x_ref / fz_max must be 16-byte aligned");
  if (batch == 0) return SRBD_QP_OK;
  hipStream_t strm = stream_of(h, stream);
  srbd::DeviceGuard guard(h->device);
  const srbd::GaitIo io =
      gait_io(cmd, x, tick, ref_pose, foot_now, srbd_plan_f64{x_ref, foot_r, foot_l, fz_max}, 0, 1);
  const hipError_t e =
      srbd::launch_srbd_gait(*params, batch, h->dims.N, *gait, io, strm, &h->robots_model, &h->terrain);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  return SRBD_QP_OK;
}

}  // extern "C"

// ---- T ticks of the closed loop: srbd_qp_srbd_rollout_f64 (gait == NULL: the window of tick t
// is gathered out of `plan`) and srbd_qp_srbd_rollout_gait_f64 (the planner writes it) ----
namespace {
// The checks of a rollout call, before any device work.  *with_plan: the steps run on a plan
// window (the gait's, or gathered from a plan that has at least one array).
int check_rollout(srbd_qp_handle h, int batch, const srbd_model_params* params, const srbd_plan_f64* plan,
                  const srbd_gait_f64* gait, const srbd_rollout_gait_f64* gio, const srbd_linesearch_params* ls,
                  const srbd_qp_settings* settings, int constraints, int sqp_max_loop,
                  const srbd_rollout_f64* roll, double* xs, double* us, double* x, double* alpha,
                  bool* with_plan) {
  if (!h || !params || !ls || !settings || !roll || !xs || !us || !x || !alpha)
    return fail(SRBD_QP_EINVAL, "NULL argument");
  if (gait) {
    // (no tick reads a command when there is none)
    if (!gio || (!gio->cmd && roll->ticks > 0) || !gio->ref_pose || !gio->foot_now)
      return fail(SRBD_QP_EINVAL, "NULL argument");
    const int rc = check_gait(h, batch, gait, gio->tick0);
    if (rc) return rc;
  }
  if (const int rc = check_srbd_call(h, batch, "the SRBD NMPC loop needs nx = nu = 12")) return rc;
  const int T = roll->ticks, P = roll->plan_stages, N = h->dims.N;
  if (T < 0) return fail(SRBD_QP_EINVAL, "rollout: ticks must be non-negative");
  if (roll->substeps < 1) return fail(SRBD_QP_EINVAL, "rollout: substeps must be at least 1");
  if (!(roll->alpha_reset >= 0.0)) return fail(SRBD_QP_EINVAL, "rollout: alpha_reset must be non-negative");
  *with_plan = gait || (plan && (plan->x_ref || plan->foot_r || plan->foot_l || plan->fz_max));
  if (!gait && *with_plan && (long long)P < (long long)N + T - 1)
    return fail(SRBD_QP_EINVAL, "rollout: the plan needs plan_stages >= N + ticks - 1");
  if (!aligned16(xs) || !aligned16(us)) return fail(SRBD_QP_EINVAL, "rollout: xs / us must be 16-byte aligned");
  // the step's own checks (settings, constraints against the handle's dims, ...): a step of
  // zero robots runs them and nothing else
  int none = 0;
  return srbd_qp_srbd_nmpc_plan_f64(h, 0, params, nullptr, ls, settings, constraints, sqp_max_loop, xs, us, x,
                                    alpha, &none, &none);
}

// One tick's dense plan window in the handle's roll_plan buffer (B = capacity robots of
// x_ref, foot_r, foot_l, fz_max, in that order).
struct Window {
  srbd_plan_f64 win{};      // the window's arrays: what the step and the plant step read
  srbd::RolloutRow rows[4]; // the gathers of tick 0, one per array of the long plan
  int stage_w[4];           // and their doubles per stage: tick t reads from src + t * stage_w
  int nrows = 0;
};
// Reserves the buffer and lays the window out.  `plan`: the long plan of plan_stages P to gather
// from; NULL: the gait planner writes all four arrays.
hipError_t rollout_window(srbd_qp_handle h, const srbd_plan_f64* plan, int P, Window* w) {
  const size_t B = (size_t)h->capacity, N = (size_t)h->dims.N;
  const size_t wx = 12 * (N + 1), wf = 3 * N, wz = 2 * N;
  const hipError_t e = h->roll_plan.reserve(B * (wx + 2 * wf + wz) * sizeof(double));
  if (e != hipSuccess) return e;
  double* const wxr = h->roll_plan.as<double>();
  double* const wfr = wxr + B * wx;
  double* const wfl = wfr + B * wf;
  double* const wfz = wfl + B * wf;
  if (!plan) {
    w->win = srbd_plan_f64{wxr, wfr, wfl, wfz};
    return hipSuccess;
  }
  auto gather = [&](const double* src, double* dst, const double** win, size_t width, int per_stage, long long pw) {
    if (!src) return;
    *win = dst;
    w->stage_w[w->nrows] = per_stage;
    w->rows[w->nrows++] = srbd::RolloutRow{src, dst, (int)width, per_stage * pw, (long long)width};
  };
  gather(plan->x_ref, wxr, &w->win.x_ref, wx, 12, (long long)P + 1);
  gather(plan->foot_r, wfr, &w->win.foot_r, wf, 3, P);
  gather(plan->foot_l, wfl, &w->win.foot_l, wf, 3, P);
  gather(plan->fz_max, wfz, &w->win.fz_max, wz, 2, P);
  return hipSuccess;
}
}  // namespace

static int rollout_impl(srbd_qp_handle h, int batch, const srbd_model_params* params,
                        const srbd_plan_f64* plan, const srbd_gait_f64* gait,
                        const srbd_rollout_gait_f64* gio, const srbd_linesearch_params* ls,
                        const srbd_qp_settings* settings, int constraints, int sqp_max_loop,
                        const srbd_rollout_f64* roll, double* xs, double* us, double* x, double* alpha) {
  bool with_plan = false;
  int rc = check_rollout(h, batch, params, plan, gait, gio, ls, settings, constraints, sqp_max_loop, roll, xs, us,
                         x, alpha, &with_plan);
  if (rc) return rc;
  if (batch == 0) return SRBD_QP_OK;
  const int T = roll->ticks, N = h->dims.N;
  srbd::DeviceGuard guard(h->device);
  hipStream_t strm = h->stream;
  const size_t B = (size_t)h->capacity;
  hipError_t e = hipSuccess;
  if (roll->x_log) {  // x_log[:, 0] = the x passed in
    const srbd::RolloutRow r0{x, roll->x_log, 12, 12, (long long)(T + 1) * 12};
    e = srbd::launch_rollout_rows(batch, &r0, 1, nullptr, 0.0, strm);
    if (e != hipSuccess) return hip_fail(alloc_code(e), "rollout: ", e);
  }
  if (T == 0) {
    e = hipStreamSynchronize(strm);
    return e == hipSuccess ? SRBD_QP_OK : hip_fail(alloc_code(e), "rollout: ", e);
  }
  // scratch: the step's sqp_iter / converged, and one tick's dense plan window
  e = h->roll.reserve(2 * B * sizeof(int));
  Window w;
  if (e == hipSuccess && with_plan) e = rollout_window(h, gait ? nullptr : plan, roll->plan_stages, &w);
  if (e != hipSuccess) return hip_fail(alloc_code(e), "rollout scratch allocation failed: ", e);
  int* it_step = h->roll.as<int>();
  int* cv_step = it_step + B;
  // a step that runs no SQP iteration (sqp_max_loop == 0) writes neither
  e = hipMemsetAsync(it_step, 0, 2 * B * sizeof(int), strm);
  if (e != hipSuccess) return hip_fail(alloc_code(e), "rollout: ", e);
  const srbd_plan_f64* wplan = with_plan ? &w.win : nullptr;
  for (int t = 0; t < T; ++t) {
    // W_t: stages t .. t + N of the long plan, gathered dense; alpha per the reset policy
    srbd::RolloutRow rt[4];
    if (gait) {  // W_t from the planner: cmd[:, t], the current x, tick0 + t; row 0 to the logs
      srbd::GaitIo gi = gait_io(gio->cmd, x, gio->tick0 + t, gio->ref_pose, gio->foot_now, w.win, t, T);
      gi.foot_log = gio->foot_log ? gio->foot_log + (size_t)t * 6 : nullptr;
      gi.foot_log_stride = (long long)T * 6;
      gi.fz_log = gio->fz_log ? gio->fz_log + (size_t)t * 2 : nullptr;
      gi.fz_log_stride = (long long)T * 2;
      e = srbd::launch_srbd_gait(*params, batch, N, *gait, gi, strm, &h->robots_model, &h->terrain);
      if (e != hipSuccess) return hip_fail(alloc_code(e), "rollout: ", e);
    }
    for (int i = 0; i < w.nrows; ++i) {
      rt[i] = w.rows[i];
      rt[i].src += (size_t)t * w.stage_w[i];
    }
    e = srbd::launch_rollout_rows(batch, rt, w.nrows, roll->alpha_reset > 0.0 ? alpha : nullptr,
                                  roll->alpha_reset, strm);
    if (e != hipSuccess) return hip_fail(alloc_code(e), "rollout: ", e);
    rc = nmpc_step(h, batch, params, wplan, ls, settings, constraints, sqp_max_loop, xs, us, x, alpha, it_step,
                   cv_step, true);
    if (rc) return rc;
    // the plant step, with column t of the logs (x_log's columns are one ahead: column 0 is the start)
    srbd::AdvanceIo io = advance_io(roll->substeps, xs, us, x, roll->wrench, roll->u_log, t, T);
    io.x_out = roll->x_log ? roll->x_log + (size_t)(t + 1) * 12 : nullptr;
    io.x_stride = (long long)(T + 1) * 12;
    io.it_src = it_step;
    io.cv_src = cv_step;
    io.it_log = roll->sqp_iter_log ? roll->sqp_iter_log + t : nullptr;
    io.cv_log = roll->converged_log ? roll->converged_log + t : nullptr;
    io.log_stride = T;
    e = srbd::launch_srbd_advance(*params, batch, N, io, wplan, strm, &h->robots_model, &h->robots_plant,
                                  h->has_contact ? &h->contact : nullptr);
    if (e != hipSuccess) return hip_fail(alloc_code(e), "rollout: ", e);
  }
  e = hipStreamSynchronize(strm);
  if (e != hipSuccess) return hip_fail(alloc_code(e), "rollout: ", e);
  return SRBD_QP_OK;
}

extern "C" {

int srbd_qp_srbd_rollout_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                             const srbd_plan_f64* plan, const srbd_linesearch_params* ls,
                             const srbd_qp_settings* settings, int constraints, int sqp_max_loop,
                             const srbd_rollout_f64* roll, double* xs, double* us, double* x,
                             double* alpha) {
  return rollout_impl(h, batch, params, plan, nullptr, nullptr, ls, settings, constraints, sqp_max_loop, roll,
                      xs, us, x, alpha);
}
int srbd_qp_srbd_rollout_gait_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                  const srbd_gait_f64* gait, const srbd_rollout_gait_f64* gio,
                                  const srbd_linesearch_params* ls, const srbd_qp_settings* settings,
                                  int constraints, int sqp_max_loop, const srbd_rollout_f64* roll,
                                  double* xs, double* us, double* x, double* alpha) {
  if (!gait || !gio) return fail(SRBD_QP_EINVAL, "NULL argument");
  return rollout_impl(h, batch, params, nullptr, gait, gio, ls, settings, constraints, sqp_max_loop, roll, xs,
                      us, x, alpha);
}

}  // extern "C"

// ---- the differentiable plant: the open-loop rollout and its adjoint ----
namespace {
// the checks both calls make of `roll`, after their NULL arguments
int check_plant_roll(const srbd_plant_rollout_f64* roll) {
  if (!roll->u && roll->ticks > 0) return fail(SRBD_QP_EINVAL, "plant_rollout: roll->u is NULL");
  if (roll->ticks < 0) return fail(SRBD_QP_EINVAL, "plant_rollout: ticks must be non-negative");
  if (roll->substeps < 1) return fail(SRBD_QP_EINVAL, "plant_rollout: substeps must be at least 1");
  if (roll->foot_stages < 0 || (roll->foot_stages > 0 && roll->foot_stages < roll->ticks))
    return fail(SRBD_QP_EINVAL, "plant_rollout: foot_stages must be 0 or at least ticks");
  return SRBD_QP_OK;
}
// mass and Lbody as the advance launcher resolves them for the plant: the PLANT role's, else the
// MODEL role's, else NULL (params')
void plant_robot(srbd_qp_handle h, const double** mass, const double** Lbody) {
  *mass = h->robots_plant.mass ? h->robots_plant.mass : h->robots_model.mass;
  *Lbody = h->robots_plant.Lbody ? h->robots_plant.Lbody : h->robots_model.Lbody;
}
}  // namespace

extern "C" {

int srbd_qp_srbd_plant_rollout_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                   const srbd_plant_rollout_f64* roll, const double* x0, double* x_traj,
                                   void* stream) {
  if (!h || !params || !roll || !x0) return fail(SRBD_QP_EINVAL, "NULL argument");
  if (!x_traj) return fail(SRBD_QP_EINVAL, "plant_rollout: x_traj is NULL");
  if (const int rc = check_plant_roll(roll)) return rc;
  if (const int rc = check_srbd_call(h, batch, "the SRBD plant rollout needs nx = nu = 12")) return rc;
  if (!aligned16(x0) || !aligned16(roll->u) || !aligned16(x_traj))
    return fail(SRBD_QP_EINVAL, "plant_rollout: x0 / u / x_traj must be 16-byte aligned");
  if (batch == 0) return SRBD_QP_OK;
  hipStream_t strm = stream_of(h, stream);
  srbd::DeviceGuard guard(h->device);
  const double *mass, *Lbody;
  plant_robot(h, &mass, &Lbody);
  const hipError_t e = srbd::launch_srbd_plant_rollout(*params, batch, *roll, mass, Lbody, x0, x_traj, strm);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  return SRBD_QP_OK;
}

int srbd_qp_srbd_plant_rollout_backward_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                            const srbd_plant_rollout_f64* roll, const double* x_traj,
                                            const double* gx, const srbd_plant_grad_f64* grad, void* stream) {
  if (!h || !params || !roll) return fail(SRBD_QP_EINVAL, "NULL argument");
  if (!x_traj) return fail(SRBD_QP_EINVAL, "plant_rollout_backward: x_traj is NULL");
  if (!gx || !grad) return fail(SRBD_QP_EINVAL, "plant_rollout_backward: gx or grad is NULL");
  if (const int rc = check_plant_roll(roll)) return rc;
  if (const int rc = check_srbd_call(h, batch, "the SRBD plant rollout needs nx = nu = 12")) return rc;
  if (!aligned16(roll->u) || !aligned16(x_traj) || !aligned16(gx))
    return fail(SRBD_QP_EINVAL, "plant_rollout_backward: u / x_traj / gx must be 16-byte aligned");
  if (batch == 0) return SRBD_QP_OK;
  hipStream_t strm = stream_of(h, stream);
  srbd::DeviceGuard guard(h->device);
  const double *mass, *Lbody;
  plant_robot(h, &mass, &Lbody);
  const hipError_t e =
      srbd::launch_srbd_plant_rollout_backward(*params, batch, *roll, mass, Lbody, x_traj, gx, *grad, strm);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  return SRBD_QP_OK;
}

}  // extern "C"
