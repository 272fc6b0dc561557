// capi_solve.hip -- the device-pointer solves of the C-ABI (include/srbd_qp.h): the checks of a
// call, its launch arguments, the dispatch to the HIP kernels (with the latency IPM's lq
// switch), the mixed-precision paths (f64_rescue, f32_iters) and the soft-box solve.
#include "capi_handle.h"

#include <cstring>
#include <string>
#include <type_traits>

using namespace srbd::capi;

namespace {
// visitor of a (source, destination) pair of structs: the destination points where the source does
constexpr auto copy_pointer = [](size_t, const auto& src, auto& dst) { dst = src; };
}  // namespace

template <typename DataT, typename SolT>
int srbd::capi::validate_call(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const DataT* d,
                              const SolT* s) {
  if (!h) return fail(SRBD_QP_EINVAL, "handle is NULL");
  if (!d || !s) return fail(SRBD_QP_EINVAL, "data/solution is NULL");
  if (batch < 0) return fail(SRBD_QP_EINVAL, "batch must be >= 0");
  if (batch > h->capacity)
    return fail(SRBD_QP_ECAPACITY, "batch " + std::to_string(batch) + " exceeds capacity " +
                                       std::to_string(h->capacity));
  int rc = srbd_qp_check_settings(st);
  if (rc) return rc;
  if (!d->A || !d->B || !d->b || !d->Q || !d->S || !d->R || !d->q || !d->r || !d->x0)
    return fail(SRBD_QP_EINVAL, "A, B, b, Q, S, R, q, r and x0 are required");
  if (!s->x || !s->u || !s->pi) return fail(SRBD_QP_EINVAL, "x, u and pi outputs are required");
  const srbd_qp_dims& dm = h->dims;
  if ((d->lbu != nullptr) != (dm.has_box_u != 0) || (d->lbx != nullptr) != (dm.has_box_x != 0))
    return fail(SRBD_QP_EINVAL, "box-constraint pointers do not match the handle's dims");
  if (dm.ng > 0 && (!d->lg || !d->ug))
    return fail(SRBD_QP_EINVAL, "ng > 0 needs lg and ug (C, D and the masks are optional)");
  return SRBD_QP_OK;
}
// (the host-buffer calls check with these)
template int srbd::capi::validate_call(srbd_qp_handle, int, const srbd_qp_settings*, const srbd_qp_data_f64*,
                                       const srbd_qp_solution_f64*);
template int srbd::capi::validate_call(srbd_qp_handle, int, const srbd_qp_settings*, const srbd_qp_data_f32*,
                                       const srbd_qp_solution_f32*);

static int rescue_f32(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const srbd_qp_data_f32* d,
                      const srbd_qp_solution_f32* s, const int* status, hipStream_t strm);
static int mixed_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                     const srbd_qp_data_f64* d, const srbd_qp_solution_f64* s, hipStream_t strm);
static int fallback_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                        const srbd_qp_data_f64* d, const srbd_qp_solution_f64* sc,
                        const srbd_qp_solution_f64* s, hipStream_t strm, int min_status, int* idx,
                        int* count, srbd::Buffer& buf, const double* warm_x = nullptr,
                        const double* warm_u = nullptr);

template <typename T, typename DataT, typename SolT>
srbd::ProblemArgsT<T> srbd::capi::build_args(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                                             const DataT* d, const SolT* s, int* status, const T* warm_bars,
                                             int skip_last_rb) {
  srbd::ProblemArgsT<T> a;
  std::memset(&a, 0, sizeof a);  // (padding too: the resident server compares launches bytewise)
  a.batch = batch;
  a.N = h->dims.N;
  a.nx = h->dims.nx;
  a.nu = h->dims.nu;
  a.ng = h->dims.ng;
  a.layout = h->dims.layout;
  fields::for_each_input(h->dims, copy_pointer, *d, a);
  fields::for_each_solution_field(h->dims, 0, copy_pointer, copy_pointer, *s, a);
  a.status = status;  // (the caller's, or the handle's own list)
  a.ws = reinterpret_cast<T*>(h->ws);
  a.ws_qp = h->ws_qp;
  a.reg = st->reg_prim;
  a.iter_max = st->iter_max;
  a.stat_rows = st->iter_max + 2;
  a.warm_bars = warm_bars;
  a.skip_last_rb = skip_last_rb;
  a.pred_corr = st->pred_corr;
  a.split_step = st->split_step;
  a.ric_alg = st->ric_alg != 0;  // HPIPM: any nonzero square_root_alg
  // HPIPM's mode-dependent iterative refinement of the corrector (d_ocp_qp_ipm_arg_set_default:
  // itref_corr_max 2 in Balance, 4 in Robust, 0 in Speed / SpeedAbs)
  a.itref_corr_max = st->mode == 2 ? 2 : st->mode == 3 ? 4 : 0;
  // and its lq_fact: 1 in Balance, 2 in Robust, with the square-root Riccati only
  // ("for square_root_alg==1", hpipm_d_ocp_qp_ipm.h:78)
  a.lq_fact = !st->ric_alg ? 0 : st->lq_fact >= 0 ? st->lq_fact : st->mode == 2 ? 1 : st->mode == 3 ? 2 : 0;
  a.lq_redo = 0;
  a.warm_start = st->warm_start;
  a.alpha_min = st->alpha_min;
  a.mu0 = st->mu0;
  a.tol_stat = st->tol_stat;
  a.tol_eq = st->tol_eq;
  a.tol_ineq = st->tol_ineq;
  a.tol_comp = st->tol_comp;
  if constexpr (std::is_same_v<T, double>) a.factors_ready = h->fac_arm;
  if (h->ctl) {
    a.ctl = h->ctl;
    a.ctl_cap = srbd::kCtlCap;
    a.qp_buf = h->qp_buf;
  }
  return a;
}
// (the resident server's request, capi_host.hip)
template srbd::ProblemArgsT<double> srbd::capi::build_args(srbd_qp_handle, int, const srbd_qp_settings*,
                                                           const srbd_qp_data_f64*, const srbd_qp_solution_f64*,
                                                           int*, const double*, int);

// clears the caller's stat table: st->iter_max + 2 rows per QP
template <typename T>
static hipError_t clear_stat_table(T* stat, const srbd_qp_settings* st, int batch, hipStream_t strm) {
  return hipMemsetAsync(stat, 0, sizeof(T) * srbd::kStatCols * (size_t)(st->iter_max + 2) * (size_t)batch, strm);
}

// warm_bars: warm_start 2 only (the fp64 continuation of rescue_f32), see ProblemArgsT;
// iter_cap >= 0 (the f32_iters continuation): at most that many iterations, while the stat
// table keeps the caller's st->iter_max + 2 rows
template <typename T, typename DataT, typename SolT>
static int solve_impl(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const DataT* d,
                      const SolT* s, void* stream, const T* warm_bars = nullptr,
                      int skip_last_rb = 0, int iter_cap = -1) {
  int rc = validate_call(h, batch, st, d, s);
  if (rc) return rc;
  if (batch == 0) return SRBD_QP_OK;
  hipStream_t strm = stream_of(h, stream);
  if constexpr (std::is_same_v<T, double>) {
    if (st->f32_iters > 0 && st->iter_max > 1 && constrained(h->dims) && h->dims.nx == 12 &&
        h->dims.nu == 12)
      return mixed_f64(h, batch, st, d, s, strm);
  }
  srbd::DeviceGuard guard(h->device);
  // fp32 with f64_rescue: the status the fp32 pass leaves decides what is solved again
  const bool rescue = std::is_same_v<T, float> && st->f64_rescue && constrained(h->dims);
  if (rescue) {
    const hipError_t ea = reserve_select(h, &h->resc_idx, false);
    if (ea != hipSuccess) return hip_fail(SRBD_QP_ENOMEM, "rescue buffers: ", ea);
  }
  int* status = s->status;
  if (rescue && !status) status = h->resc_idx + h->capacity;
  srbd::ProblemArgsT<T> a = build_args<T>(h, batch, st, d, s, status, warm_bars, skip_last_rb);
  // f64_rescue = n: the fp32 pass stops after n iterations at most, the rest is fp64's
  if (rescue && st->f64_rescue < a.iter_max) a.iter_max = st->f64_rescue;
  if (iter_cap >= 0 && iter_cap < a.iter_max) a.iter_max = iter_cap;
  hipError_t e = hipSuccess;
  // (unconstrained with residuals: unconstr_residuals_kernel clears and fills the table)
  if (s->stat && (constrained(h->dims) || !st->compute_residuals)) e = clear_stat_table(s->stat, st, batch, strm);
  // nx < 12 or nu < 12: solve the problem embedded in 12 x 12 stages
  const bool padded = a.nx != 12 || a.nu != 12;
  srbd::ProblemArgsT<T> run = a;
  if (e == hipSuccess && padded) {
    e = h->pad.reserve(srbd::pad_elems(h->capacity, a.N, a.ng) * sizeof(T));
    if (e == hipSuccess) e = srbd::pad_problem<T>(a, h->pad.as<T>(), run, strm);
  }
  if (e != hipSuccess) {
  } else if (constrained(h->dims)) {
    // ric_alg 1 with lq_fact 1 (Balance's default) on the latency IPM: its predictor check may
    // ask for HPIPM's switch to the LQ factorization, which only the batched kernels have.  Such
    // a QP ends with status kLatNeedsLq and raises the flag; the call then waits once for the
    // flag and, if it is up, solves those QPs (and only those) again on the batched kernels, so
    // each QP ends as it does in any batch
    bool lq_watch = false;
    if constexpr (std::is_same_v<T, double>) {
      if (run.ric_alg && run.lq_fact == 1 && iter_cap < 0 && !h->force_batched) {
        e = reserve_select(h, &h->lqsw_idx, true);
        run.lat_lq_flag = e == hipSuccess ? h->lat_flag : nullptr;
        lq_watch = e == hipSuccess && srbd::ipm_latency_ok(run, srbd::ipm_latency_max_batch());
        if (!lq_watch) {
          run.lat_lq_flag = nullptr;
        } else {
          if (!a.status) a.status = run.status = h->lqsw_idx + h->capacity;
          e = hipMemsetAsync(h->lat_flag, 0, sizeof(int), strm);
        }
      }
      if (e == hipSuccess)
        e = h->force_batched ? srbd::launch_ipm_box_batched(run, strm) : srbd::launch_ipm_box(run, strm);
    } else {
      if (e == hipSuccess) e = srbd::launch_ipm_box(run, strm);
    }
    if (e == hipSuccess && padded) e = srbd::unpad_solution<T>(a, run, strm);
    if constexpr (std::is_same_v<T, double>) {
      if (e == hipSuccess && lq_watch) {
        e = hipMemcpyAsync(h->lat_flag_host, h->lat_flag, sizeof(int), hipMemcpyDeviceToHost, strm);
        if (e == hipSuccess) e = hipStreamSynchronize(strm);
        if (e == hipSuccess && *h->lat_flag_host) {
          SolT sc = *s;
          sc.status = a.status;
          h->force_batched = true;
          rc = fallback_f64(h, batch, st, d, &sc, s, strm, srbd::kLatNeedsLq, h->lqsw_idx,
                            h->lqsw_idx + 2 * (size_t)h->capacity, h->lqsw);
          h->force_batched = false;
          return rc;
        }
      }
    }
    if constexpr (std::is_same_v<T, float>) {
      if (e == hipSuccess && rescue) return rescue_f32(h, batch, st, d, s, status, strm);
    }
  } else {
    // (the single-QP kernel computes the residuals itself when the problem is not embedded)
    run.fuse_res = st->compute_residuals && !padded;
    e = srbd::launch_riccati_unconstr(run, strm, h->riccati_streaming);
    if (e == hipSuccess && padded) e = srbd::unpad_solution<T>(a, run, strm);
    // residual norms / objective of the solution when asked for (HPIPM computes them
    // for nc = 0 too; an extra pass over the QP data, so only on request); the stat
    // table's row 0 gets them as well
    if (e == hipSuccess && (s->res || s->obj || s->stat) &&
        (h->riccati_streaming || !srbd::unconstr_fused_residuals(run))) {
      if (st->compute_residuals) {
        e = srbd::launch_unconstr_residuals<T>(a, strm);
      } else {
        if (s->res) e = hipMemsetAsync(s->res, 0, sizeof(T) * 4 * (size_t)batch, strm);
        if (e == hipSuccess && s->obj) e = hipMemsetAsync(s->obj, 0, sizeof(T) * (size_t)batch, strm);
      }
    }
  }
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  return SRBD_QP_OK;
}

// ---------------------------------------------------------------------------
// settings.f64_rescue: the QPs an fp32 pass left unsolved, solved again in fp64
// ---------------------------------------------------------------------------
// The compact fp64 batch of R selected QPs, shared by the rescue and the fallback: the values
// per QP of every input (d) and real-valued output (s) the caller passed ...
template <typename DataT, typename SolT>
static size_t passed_elems(const srbd_qp_dims& m, size_t stat_rows, const DataT& d, const SolT& s) {
  size_t total = 0;
  auto add = [&](size_t n, const auto& f) { total += f ? n : 0; };
  fields::for_each_input(m, add, d);
  fields::for_each_output(m, stat_rows, add, s);
  return total;
}
// ... and its layout from `cur` on: each input gathered by gather(src, dst, values per QP) with
// d2 pointing at it, then the outputs' places in s2.  Returns the end.
template <typename DataT, typename SolT, typename Gather>
static double* compact_batch(const srbd_qp_dims& m, size_t stat_rows, size_t R, double* cur, const DataT& d,
                             const SolT& s, srbd_qp_data_f64& d2, srbd_qp_solution_f64& s2, hipError_t& e,
                             Gather&& gather) {
  fields::for_each_input(m, [&](size_t n, const auto& src, auto& dst) {
    if (!src || e != hipSuccess) return;
    e = gather(src, cur, n);
    dst = cur;
    cur += n * R;
  }, d, d2);
  fields::for_each_output(m, stat_rows, [&](size_t n, const auto& dst, auto& src) {
    if (!dst) return;
    src = cur;
    cur += n * R;
  }, s, s2);
  return cur;
}

// The QPs of `status` that ended with status >= min_status, listed in idx (count: the list's
// length on the device), and their number in *R: one wait for the stream.
static hipError_t select_unsolved(srbd_qp_handle h, const int* status, int batch, int min_status, int* idx,
                                  int* count, hipStream_t strm, int* R) {
  hipError_t e = srbd::launch_select_unsolved(status, batch, min_status, idx, count, strm);
  if (e == hipSuccess) e = hipMemcpyAsync(h->resc_count_host, count, sizeof(int), hipMemcpyDeviceToHost, strm);
  if (e == hipSuccess) e = hipStreamSynchronize(strm);
  *R = e == hipSuccess ? *h->resc_count_host : 0;
  return e;
}

static int rescue_f32(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const srbd_qp_data_f32* d,
                      const srbd_qp_solution_f32* s, const int* status, hipStream_t strm) {
  srbd::DeviceGuard guard(h->device);
  int* idx = h->resc_idx;
  int R = 0;
  hipError_t e = select_unsolved(h, status, batch, 1, idx, h->resc_idx + 2 * (size_t)h->capacity, strm, &R);
  // (device errors of the rescue read as the fp32 solve's own)
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  if (R == 0) return SRBD_QP_OK;
  const srbd_qp_dims& m = h->dims;
  const size_t N = (size_t)m.N, nx = (size_t)m.nx, nu = (size_t)m.nu;
  const size_t stat_rows = (size_t)(st->iter_max + 2);
  srbd_qp_data_f64 d64{};
  srbd_qp_solution_f64 s64{};
  // fp64 continuation from the fp32 iterate (x, u, pi and the barrier state: HPIPM's
  // warm_start = 2) on 12 x 12 stages; a padded problem is re-solved cold
  const bool cont = m.nx == 12 && m.nu == 12;
  const size_t warm_e = cont ? (N + 1) * (96 + (size_t)((m.ng + 11) / 12) * 48) : 0;
  const size_t per_qp = warm_e + passed_elems(m, stat_rows, *d, *s);  // doubles
  e = h->resc.reserve(sizeof(double) * per_qp * (size_t)R + 2 * sizeof(int) * (size_t)R + 256);
  if (e != hipSuccess) return hip_fail(SRBD_QP_ENOMEM, "rescue batch: ", e);
  double* warm = compact_batch(m, stat_rows, (size_t)R, h->resc.as<double>(), *d, *s, d64, s64, e,
                               [&](const float* src, double* dst, size_t n) {
                                 return srbd::launch_gather_widen(src, dst, idx, R, n, strm);
                               });
  s64.status = reinterpret_cast<int*>(warm + warm_e * (size_t)R);
  s64.iter = s64.status + R;
  if (cont && e == hipSuccess) {
    // the iterate the fp32 pass ended on: x, u, pi (caller's buffers), barrier state (its
    // workspace, read before the fp64 solve reuses that memory)
    e = srbd::launch_gather_widen(s->x, s64.x, idx, R, (N + 1) * nx, strm);
    if (e == hipSuccess) e = srbd::launch_gather_widen(s->u, s64.u, idx, R, N * nu, strm);
    if (e == hipSuccess) e = srbd::launch_gather_widen(s->pi, s64.pi, idx, R, (N + 1) * nx, strm);
    if (e == hipSuccess)
      e = srbd::launch_gather_warm_bars(reinterpret_cast<const float*>(h->ws), h->ws_qp, m.N, m.ng, idx,
                                        R, warm, strm);
  }
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  srbd_qp_settings st64 = *st;
  st64.warm_start = cont ? 2 : 0;
  st64.f64_rescue = 0;
  st64.f32_iters = 0;
  int rc = solve_impl<double>(h, R, &st64, &d64, &s64, strm, cont ? warm : nullptr);
  if (rc) return rc;
  // A QP the continuation leaves unsolved (an fp32 pass can end far off, with the barrier
  // collapsed: t, lam -> 0 at a large stationarity residual, from where a warm-started IPM
  // does not recover) is solved again cold in fp64 (its own list, buffer and idx slots:
  // [capacity, 2 capacity) of resc_idx)
  if (cont) {
    rc = fallback_f64(h, R, &st64, &d64, &s64, &s64, strm, 1, h->resc_idx + h->capacity,
                      h->resc_idx + 2 * (size_t)h->capacity, h->resc2);
    if (rc) return rc;
  }
  fields::for_each_output(m, stat_rows, [&](size_t n, const auto& dst, const auto& src) {
    if (dst && e == hipSuccess) e = srbd::launch_scatter_narrow(src, dst, idx, R, n, strm);
  }, *s, s64);
  if (e == hipSuccess && s->status) e = srbd::launch_scatter_int(s64.status, s->status, idx, R, strm);
  if (e == hipSuccess && s->iter) e = srbd::launch_scatter_int(s64.iter, s->iter, idx, R, strm);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  return SRBD_QP_OK;
}

// ---------------------------------------------------------------------------
// settings.f32_iters: mixed-precision IPM (fp32 iterations, then fp64 to the end)
// ---------------------------------------------------------------------------
// A QP a warm-started fp64 continuation ends with status >= min_status is solved again in
// fp64 (compact batch in *buf, list in idx) exactly as the plain fp64 call solves it: the
// caller's iter_max, and its x / u warm start when warm_x / warm_u are given (the caller's
// buffers as they were on entry), cold otherwise.  Both users pass min_status 1, so neither
// the mixed path (f32_iters) nor the rescue (f64_rescue) ends a QP worse than fp64 does.
static int fallback_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                        const srbd_qp_data_f64* d, const srbd_qp_solution_f64* sc,
                        const srbd_qp_solution_f64* s, hipStream_t strm, int min_status, int* idx,
                        int* count, srbd::Buffer& buf, const double* warm_x, const double* warm_u) {
  srbd::DeviceGuard guard(h->device);
  int R = 0;
  hipError_t e = select_unsolved(h, sc->status, batch, min_status, idx, count, strm, &R);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "fallback: ", e);
  if (R == 0) return SRBD_QP_OK;
  const srbd_qp_dims& m = h->dims;
  const size_t N = (size_t)m.N, nx = (size_t)m.nx, nu = (size_t)m.nu;
  const size_t stat_rows = (size_t)(st->iter_max + 2);
  srbd_qp_data_f64 d2{};
  srbd_qp_solution_f64 s2{};
  const size_t per_qp = passed_elems(m, stat_rows, *d, *s);
  e = buf.reserve(sizeof(double) * per_qp * (size_t)R + 2 * sizeof(int) * (size_t)R + 256);
  if (e != hipSuccess) return hip_fail(SRBD_QP_ENOMEM, "fallback batch: ", e);
  double* end = compact_batch(m, stat_rows, (size_t)R, buf.as<double>(), *d, *s, d2, s2, e,
                              [&](const double* src, double* dst, size_t n) {
                                return srbd::launch_gather_rows(src, dst, idx, R, n, strm);
                              });
  s2.status = reinterpret_cast<int*>(end);
  s2.iter = s2.status + R;
  const bool warm = warm_x && warm_u && st->warm_start;
  if (warm && e == hipSuccess) e = srbd::launch_gather_rows(warm_x, s2.x, idx, R, (N + 1) * nx, strm);
  if (warm && e == hipSuccess) e = srbd::launch_gather_rows(warm_u, s2.u, idx, R, N * nu, strm);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "fallback: ", e);
  srbd_qp_settings st2 = *st;
  st2.warm_start = warm ? st->warm_start : 0;
  st2.f32_iters = 0;
  int rc = solve_impl<double>(h, R, &st2, &d2, &s2, strm);
  if (rc) return rc;
  fields::for_each_output(m, stat_rows, [&](size_t n, const auto& dst, const auto& src) {
    if (dst && e == hipSuccess) e = srbd::launch_scatter_rows(src, dst, idx, R, n, strm);
  }, *s, s2);
  if (e == hipSuccess) e = srbd::launch_scatter_int(s2.status, sc->status, idx, R, strm);
  if (e == hipSuccess && s->iter) e = srbd::launch_scatter_int(s2.iter, s->iter, idx, R, strm);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "fallback: ", e);
  return SRBD_QP_OK;
}

static int mixed_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                     const srbd_qp_data_f64* d, const srbd_qp_solution_f64* s, hipStream_t strm) {
  const srbd_qp_dims& m = h->dims;
  const size_t B = (size_t)batch, N = (size_t)m.N, nx = (size_t)m.nx, nu = (size_t)m.nu;
  const size_t ex = (N + 1) * nx, eu = N * nu;
  const size_t warm_e = (N + 1) * (96 + (size_t)((m.ng + 11) / 12) * 48);
  size_t floats = 2 * ex + eu;  // per QP: x, u, pi
  fields::for_each_input(m, [&](size_t n, const auto& src) { floats += src ? n : 0; }, *d);
  // warm_start: the caller's x / u as they are on entry (the fp64 fallback starts from them)
  const size_t keep_e = st->warm_start ? ex + eu : 0;
  srbd::DeviceGuard guard(h->device);
  hipError_t e = h->mixed.reserve(B * (floats * sizeof(float) + (warm_e + keep_e) * sizeof(double)) + 512);
  if (e != hipSuccess)
    return hip_fail(SRBD_QP_ENOMEM, "mixed-precision buffers: ", e);
  double* warm = h->mixed.as<double>();
  double* keep_x = keep_e ? warm + B * warm_e : nullptr;
  double* keep_u = keep_e ? keep_x + B * ex : nullptr;
  float* cur = reinterpret_cast<float*>(warm + B * (warm_e + keep_e));
  if (keep_e) {
    e = hipMemcpyAsync(keep_x, s->x, sizeof(double) * B * ex, hipMemcpyDeviceToDevice, strm);
    if (e == hipSuccess) e = hipMemcpyAsync(keep_u, s->u, sizeof(double) * B * eu, hipMemcpyDeviceToDevice, strm);
  }
  srbd_qp_data_f32 d32{};
  fields::for_each_input(m, [&](size_t n, const auto& src, auto& dst) {
    if (!src || e != hipSuccess) return;
    e = srbd::launch_narrow(src, cur, n * B, strm);
    dst = cur;
    cur += n * B;
  }, *d, d32);
  srbd_qp_solution_f32 s32{};
  s32.x = cur;
  s32.u = cur + ex * B;
  s32.pi = cur + (ex + eu) * B;
  if (e == hipSuccess && st->warm_start) {
    e = srbd::launch_narrow(s->x, s32.x, ex * B, strm);
    if (e == hipSuccess) e = srbd::launch_narrow(s->u, s32.u, eu * B, strm);
  }
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "mixed precision: ", e);
  // fp32 iterations: tolerances out of reach, so every QP runs them all (a QP that stops
  // early on NaN / min step continues cold in fp64: its iterate fails the finiteness test
  // or is simply where it stopped).  They count against iter_max: n = min(f32_iters,
  // iter_max - 1) fp32 iterations, then at most iter_max - n fp64 ones.
  const int n32 = st->f32_iters < st->iter_max - 1 ? st->f32_iters : st->iter_max - 1;
  srbd_qp_settings st32 = *st;
  st32.iter_max = n32;
  st32.tol_stat = st32.tol_eq = st32.tol_ineq = st32.tol_comp = 1e-30;
  st32.f64_rescue = 0;
  st32.f32_iters = 0;
  // (the loop ends after the last corrector step; its application rides on the widening)
  int rc = solve_impl<float>(h, batch, &st32, &d32, &s32, strm, nullptr, 1);
  if (rc) return rc;
  e = srbd::launch_gather_warm_apply(reinterpret_cast<const float*>(h->ws), h->ws_qp, m.N, m.ng, batch,
                                     s32.x, s32.u, s32.pi, s->x, s->u, s->pi, warm, strm);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "mixed precision: ", e);
  srbd_qp_settings st64 = *st;
  st64.warm_start = 2;
  st64.f32_iters = 0;
  e = reserve_select(h, &h->resc_idx, false);
  if (e != hipSuccess) return hip_fail(SRBD_QP_ENOMEM, "fallback buffers: ", e);
  srbd_qp_solution_f64 sc = *s;
  if (!sc.status) sc.status = h->resc_idx + h->capacity;
  rc = solve_impl<double>(h, batch, &st64, d, &sc, strm, warm, 0, st->iter_max - n32);
  if (rc) return rc;
  return fallback_f64(h, batch, st, d, &sc, s, strm, 1, h->resc_idx, h->resc_idx + 2 * (size_t)h->capacity,
                      h->resc, keep_x, keep_u);
}

// ---------------------------------------------------------------------------
// Soft box constraints (srbd_qp_solve_soft_f64): always the batched fp64 kernels
// ---------------------------------------------------------------------------
static int solve_soft_impl(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                           const srbd_qp_data_f64* d, const srbd_qp_soft_f64* sf,
                           const srbd_qp_solution_f64* s, const srbd_qp_slack_f64* sl, void* stream) {
  int rc = validate_call(h, batch, st, d, s);
  if (rc) return rc;
  if (!sf) return fail(SRBD_QP_EINVAL, "soft is NULL");
  const srbd_qp_dims& dm = h->dims;
  if (dm.ng > 0)
    return fail(SRBD_QP_EDIM, "soft boxes: general rows (ng > 0) are not supported, got ng = " +
                                  std::to_string(dm.ng));
  if (st->mode == SRBD_QP_MODE_BALANCE || st->mode == SRBD_QP_MODE_ROBUST)
    return fail(SRBD_QP_ESETTINGS, "soft boxes: mode Balance / Robust is not supported (the iterative "
                                   "refinement does not carry the slack rows); use Speed or SpeedAbs");
  if (st->f32_iters != 0 || st->f64_rescue != 0)
    return fail(SRBD_QP_ESETTINGS, "soft boxes: f32_iters and f64_rescue must be 0 (fp64 only)");
  if (st->ric_alg && st->lq_fact > 0)
    return fail(SRBD_QP_ESETTINGS, "soft boxes: lq_fact must be 0 or -1 (Cholesky factorizations only)");
  if (st->warm_start != 0 && st->warm_start != 1)
    return fail(SRBD_QP_ESETTINGS, "soft boxes: warm_start must be 0 or 1");
  if (sf->soft_u && !dm.has_box_u) return fail(SRBD_QP_EINVAL, "soft_u needs a handle with has_box_u");
  if (sf->soft_x && !dm.has_box_x) return fail(SRBD_QP_EINVAL, "soft_x needs a handle with has_box_x");
  if (!constrained(dm)) return fail(SRBD_QP_EINVAL, "soft boxes need a handle with has_box_u or has_box_x");
  if (sf->soft_u && (!sf->Zl_u || !sf->Zu_u || !sf->zl_u || !sf->zu_u))
    return fail(SRBD_QP_EINVAL, "soft_u needs Zl_u, Zu_u, zl_u and zu_u");
  if (sf->soft_x && (!sf->Zl_x || !sf->Zu_x || !sf->zl_x || !sf->zu_x))
    return fail(SRBD_QP_EINVAL, "soft_x needs Zl_x, Zu_x, zl_x and zu_x");
  if (batch == 0) return SRBD_QP_OK;
  hipStream_t strm = stream_of(h, stream);
  srbd::DeviceGuard guard(h->device);
  const bool padded = dm.nx != 12 || dm.nu != 12;
  hipError_t ea = h->soft_ws.reserve(srbd::ws_doubles_soft(dm.N) * sizeof(double) * (size_t)h->capacity);
  if (ea == hipSuccess && padded) ea = h->soft_pad.reserve(srbd::pad_soft_elems(h->capacity, dm.N) * sizeof(double));
  if (ea == hipSuccess && padded) ea = h->pad.reserve(srbd::pad_elems(h->capacity, dm.N, 0) * sizeof(double));
  if (ea != hipSuccess) return hip_fail(SRBD_QP_ENOMEM, "soft-box buffers: ", ea);
  srbd::ProblemArgsT<double> a = build_args<double>(h, batch, st, d, s, s->status, nullptr, 0);
  a.itref_corr_max = 0;
  a.lq_fact = 0;
  srbd::SoftArgsT<double> soft;
  std::memset(&soft, 0, sizeof soft);
  fields::for_each_soft_input(dm, copy_pointer, *sf, soft);
  if (sl) fields::for_each_slack_output(dm, copy_pointer, *sl, soft);
  soft.sws = h->soft_ws.as<double>();
  soft.sws_qp = srbd::ws_doubles_soft(dm.N);
  hipError_t e = hipSuccess;
  if (s->stat) e = clear_stat_table(s->stat, st, batch, strm);
  srbd::ProblemArgsT<double> run = a;
  srbd::SoftArgsT<double> srun = soft;
  if (e == hipSuccess && padded) {
    e = srbd::pad_problem<double>(a, h->pad.as<double>(), run, strm);
    if (e == hipSuccess) e = srbd::pad_soft(a, soft, h->soft_pad.as<double>(), srun, strm);
  }
  if (e == hipSuccess) e = srbd::launch_ipm_soft(run, srun, strm);
  if (e == hipSuccess && padded) {
    e = srbd::unpad_solution<double>(a, run, strm);
    if (e == hipSuccess) e = srbd::unpad_slack(a, soft, srun, strm);
  }
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "kernel launch: ", e);
  return SRBD_QP_OK;
}

extern "C" {

int srbd_qp_solve_soft_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                           const srbd_qp_data_f64* d, const srbd_qp_soft_f64* sf,
                           const srbd_qp_solution_f64* s, const srbd_qp_slack_f64* sl, void* stream) {
  return solve_soft_impl(h, batch, st, d, sf, s, sl, stream);
}
int srbd_qp_solve_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                      const srbd_qp_data_f64* d, const srbd_qp_solution_f64* s, void* stream) {
  return solve_impl<double>(h, batch, st, d, s, stream);
}
int srbd_qp_solve_f32(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                      const srbd_qp_data_f32* d, const srbd_qp_solution_f32* s, void* stream) {
  return solve_impl<float>(h, batch, st, d, s, stream);
}

}  // extern "C"
