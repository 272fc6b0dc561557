// srbd_qp_capi.hip -- implementation of the C-ABI in include/srbd_qp.h: the handle and the
// settings.  The solves are in capi_solve.hip (device pointers), capi_host.hip (host buffers,
// the resident server) and capi_srbd.hip (the SRBD entry points); capi_handle.h is what the
// four share.
//
// Host-side orchestration only: argument checks (the batched analogue of
// OcpQpDim::checkSize, hpipm-cpp/src/ocp_qp_dim.cpp:59-246, and
// OcpQpIpmSolverSettings::checkSettings, ocp_qp_ipm_solver_settings.cpp:7-38),
// workspace ownership (what d_ocp_qp_ipm_ws_wrapper did,
// src/detail/d_ocp_qp_ipm_ws_wrapper.cpp:141-155 -- sized once here instead of
// on every solve() as the reference does at ocp_qp_ipm_solver.cpp:185), and
// dispatch to the HIP kernels.  No CPU fallback exists: without a GPU every
// solve returns SRBD_QP_EDEVICE.
#include "capi_handle.h"

#include <string>

using namespace srbd::capi;

namespace {
thread_local std::string g_last_error = "";
}  // namespace

namespace srbd {
// the thread's last-error message, for every translation unit of the ABI (capi_handle.h: fail)
int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
}  // namespace srbd

extern "C" {

int srbd_qp_abi_version(void) { return SRBD_QP_ABI_VERSION; }

const char* srbd_qp_last_error(void) { return g_last_error.c_str(); }

const char* srbd_qp_status_string(int s) {
  switch (s) {
    case SRBD_QP_SUCCESS: return "HpipmStatus::Success";
    case SRBD_QP_MAX_ITER: return "HpipmStatus::MaxIterReached";
    case SRBD_QP_MIN_STEP: return "HpipmStatus::MinStepLengthReached";
    case SRBD_QP_NAN_SOL: return "HpipmStatus::NaNDetected";
    default: return "HpipmStatus::UnknownFailure";
  }
}

const char* srbd_qp_error_string(int e) {
  switch (e) {
    case SRBD_QP_OK: return "ok";
    case SRBD_QP_EINVAL: return "invalid argument";
    case SRBD_QP_EDIM: return "unsupported dimensions";
    case SRBD_QP_ENOMEM: return "device out of memory";
    case SRBD_QP_EDEVICE: return "HIP device error";
    case SRBD_QP_ECAPACITY: return "batch exceeds handle capacity";
    case SRBD_QP_ESETTINGS: return "invalid settings";
    default: return "unknown error";
  }
}

void srbd_qp_default_settings(srbd_qp_settings* s) {
  if (!s) return;
  // hpipm-cpp/include/hpipm-cpp/ocp_qp_ipm_solver_settings.hpp:26-86
  s->mode = SRBD_QP_MODE_SPEED;
  s->iter_max = 15;
  s->alpha_min = 1.0e-08;
  s->mu0 = 1.0e+02;
  s->tol_stat = 1.0e-08;
  s->tol_eq = 1.0e-08;
  s->tol_ineq = 1.0e-08;
  s->tol_comp = 1.0e-08;
  s->reg_prim = 1.0e-12;
  s->warm_start = 0;
  s->pred_corr = 1;
  s->ric_alg = 1;
  s->split_step = 0;
  s->compute_residuals = 1;  // HPIPM's comp_res_exit
  s->f64_rescue = 0;
  s->f32_iters = 0;
  s->lq_fact = -1;
}

int srbd_qp_check_settings(const srbd_qp_settings* s) {
  if (!s) return fail(SRBD_QP_EINVAL, "settings is NULL");
  // messages of OcpQpIpmSolverSettings::checkSettings (settings.cpp:7-38)
  if (s->iter_max < 0) return fail(SRBD_QP_ESETTINGS, "OcpQpIpmSolverSettings.iter_max must be non-negative");
  if (s->alpha_min <= 0) return fail(SRBD_QP_ESETTINGS, "OcpQpIpmSolverSettings.alpha_min must be positive");
  if (s->alpha_min > 1.0) return fail(SRBD_QP_ESETTINGS, "OcpQpIpmSolverSettings.alpha_min must be less than 1.0");
  if (s->mu0 <= 0.0) return fail(SRBD_QP_ESETTINGS, "OcpQpIpmSolverSettings.mu0 must be positive");
  if (s->tol_stat <= 0.0) return fail(SRBD_QP_ESETTINGS, "OcpQpIpmSolverSettings.tol_stat must be positive");
  if (s->tol_eq <= 0.0) return fail(SRBD_QP_ESETTINGS, "OcpQpIpmSolverSettings.tol_eq must be positive");
  if (s->tol_ineq <= 0.0) return fail(SRBD_QP_ESETTINGS, "OcpQpIpmSolverSettings.tol_ineq must be positive");
  if (s->tol_comp <= 0.0) return fail(SRBD_QP_ESETTINGS, "OcpQpIpmSolverSettings.tol_comp must be positive");
  if (s->reg_prim < 0.0) return fail(SRBD_QP_ESETTINGS, "OcpQpIpmSolverSettings.reg_prim must be non-negative");
  // extensions (srbd_qp.h)
  if (s->f64_rescue < 0) return fail(SRBD_QP_ESETTINGS, "srbd_qp_settings.f64_rescue must be non-negative");
  if (s->f32_iters < 0) return fail(SRBD_QP_ESETTINGS, "srbd_qp_settings.f32_iters must be non-negative");
  if (s->lq_fact < -1 || s->lq_fact > 2)
    return fail(SRBD_QP_ESETTINGS, "srbd_qp_settings.lq_fact must be -1 (the mode's), 0, 1 or 2");
  return SRBD_QP_OK;
}

static int check_dims(const srbd_qp_dims* d) {
  if (!d) return fail(SRBD_QP_EINVAL, "dims is NULL");
  if (d->layout != SRBD_QP_LAYOUT_QP_MAJOR && d->layout != SRBD_QP_LAYOUT_STAGE_MAJOR)
    return fail(SRBD_QP_EINVAL, "unknown layout " + std::to_string(d->layout));
  if (d->layout == SRBD_QP_LAYOUT_STAGE_MAJOR &&
      (d->has_box_u || d->has_box_x || d->ng > 0 || d->nx != 12 || d->nu != 12))
    return fail(SRBD_QP_EINVAL, "stage-major inputs are supported by the unconstrained 12 x 12 solve only");
  if (d->N < 1 || d->N > 1024)
    return fail(SRBD_QP_EDIM, "N must be in [1, 1024], got " + std::to_string(d->N));
  if (d->nx < 1 || d->nx > SRBD_QP_MAX_NX)
    return fail(SRBD_QP_EDIM, "nx must be in [1, 12], got " + std::to_string(d->nx));
  if (d->nu < 1 || d->nu > SRBD_QP_MAX_NU)
    return fail(SRBD_QP_EDIM, "nu must be in [1, 12], got " + std::to_string(d->nu));
  if (d->ng < 0 || d->ng > SRBD_QP_MAX_NG)
    return fail(SRBD_QP_EDIM, "ng must be in [0, 64], got " + std::to_string(d->ng));
  return SRBD_QP_OK;
}

static size_t ws_doubles_per_qp(const srbd_qp_dims& d) {
  return constrained(d) ? srbd::ws_doubles_ipm(d.N, d.ng) : srbd::ws_doubles_unconstr(d.N);
}

int srbd_qp_create(const srbd_qp_dims* dims, int batch_capacity, int device, srbd_qp_handle* out) {
  if (!out) return fail(SRBD_QP_EINVAL, "out handle pointer is NULL");
  *out = nullptr;
  int rc = check_dims(dims);
  if (rc) return rc;
  if (batch_capacity < 1) return fail(SRBD_QP_EINVAL, "batch_capacity must be >= 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SRBD_QP_EDEVICE, "no HIP device available (libsrbd_qp has no CPU fallback)");
  if (device < 0 || device >= ndev)
    return fail(SRBD_QP_EDEVICE, "device index " + std::to_string(device) + " out of range");
  srbd::DeviceGuard guard(device);
  if (guard.status() != hipSuccess) return fail(SRBD_QP_EDEVICE, "hipSetDevice failed");
  auto* h = new srbd_qp_handle_s();
  h->dims = *dims;
  h->capacity = batch_capacity;
  h->device = device;
  h->ws_qp = ws_doubles_per_qp(*dims);
  h->ws_bytes = h->ws_qp * sizeof(double) * (size_t)batch_capacity;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = srbd::prepare_riccati_device();  // per-device kernel attributes
  if (e == hipSuccess) e = srbd::prepare_ipm_latency_device();
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->ws), h->ws_bytes);
  if (e == hipSuccess && constrained(*dims)) {
    e = hipMalloc(reinterpret_cast<void**>(&h->ctl), sizeof(int) * srbd::kCtlInts);
    if (e == hipSuccess) e = hipMemset(h->ctl, 0, sizeof(int) * srbd::kCtlInts);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->qp_buf), sizeof(int) * ((size_t)batch_capacity + 1));
  }
  if (e != hipSuccess) {
    srbd_qp_destroy(h);
    return hip_fail(alloc_code(e), "workspace allocation failed: ", e);
  }
  *out = h;
  return SRBD_QP_OK;
}

}  // extern "C"

// a select-index list: QP list + status (capacity ints each), then the count
static size_t select_idx_bytes(srbd_qp_handle h) { return sizeof(int) * (2 * (size_t)h->capacity + 1); }

// (capi_handle.h)  What is missing is allocated into locals and committed only when every
// allocation succeeded, so no later call finds the set half there.
hipError_t srbd::capi::reserve_select(srbd_qp_handle h, int** idx, bool with_flag) {
  int *nidx = nullptr, *ncount = nullptr, *nflag = nullptr, *nflag_host = nullptr;
  hipError_t e = hipSuccess;
  auto dev = [&](int** p, size_t bytes) {
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(p), bytes);
  };
  auto host = [&](int** p) {
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(p), sizeof(int));
  };
  if (!*idx) dev(&nidx, select_idx_bytes(h));
  if (!h->resc_count_host) host(&ncount);
  if (with_flag && !h->lat_flag) {
    dev(&nflag, sizeof(int));
    host(&nflag_host);
  }
  if (e != hipSuccess) {
    if (nidx) hipFree(nidx);
    if (ncount) hipHostFree(ncount);
    if (nflag) hipFree(nflag);
    if (nflag_host) hipHostFree(nflag_host);
    return e;
  }
  if (nidx) *idx = nidx;
  if (ncount) h->resc_count_host = ncount;
  if (nflag) {
    h->lat_flag = nflag;
    h->lat_flag_host = nflag_host;
  }
  return hipSuccess;
}

extern "C" {

void srbd_qp_destroy(srbd_qp_handle h) {
  if (!h) return;
  srbd::DeviceGuard guard(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  server_stop(h);
  if (h->srv_stream) hipStreamDestroy(h->srv_stream);
  if (h->srv_mb) hipHostFree(h->srv_mb);
  if (h->ws) hipFree(h->ws);
  h->each_buffer([](srbd::Buffer& b) { b.release(); });
  for (int* dev : {h->resc_idx, h->lat_flag, h->lqsw_idx, h->ctl, h->qp_buf})
    if (dev) hipFree(dev);
  for (int* host : {h->nmpc_active_host, h->resc_count_host, h->lat_flag_host, h->fac_flags})
    if (host) hipHostFree(host);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
}

void* srbd_qp_stream(srbd_qp_handle h) { return h ? reinterpret_cast<void*>(h->stream) : nullptr; }

size_t srbd_qp_workspace_bytes(srbd_qp_handle h) { return h ? h->ws_bytes : 0; }

size_t srbd_qp_memory_bytes(srbd_qp_handle h) {
  if (!h) return 0;
  size_t total = h->ws_bytes + (h->ctl ? sizeof(int) * srbd::kCtlInts : 0) +
                 (h->qp_buf ? sizeof(int) * ((size_t)h->capacity + 1) : 0) +
                 (h->resc_idx ? select_idx_bytes(h) : 0) + (h->lqsw_idx ? select_idx_bytes(h) : 0);
  h->each_buffer([&](const srbd::Buffer& b) { total += b.bytes; });
  return total;
}

int srbd_qp_synchronize(srbd_qp_handle h) {
  if (!h) return fail(SRBD_QP_EINVAL, "handle is NULL");
  hipError_t e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "stream sync: ", e);
  return SRBD_QP_OK;
}

}  // extern "C"
