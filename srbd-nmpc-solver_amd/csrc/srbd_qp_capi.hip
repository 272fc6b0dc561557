// srbd_qp_capi.hip -- implementation of the C-ABI in include/srbd_qp.h.
//
// Host-side orchestration only: argument checks (the batched analogue of
// OcpQpDim::checkSize, hpipm-cpp/src/ocp_qp_dim.cpp:59-246, and
// OcpQpIpmSolverSettings::checkSettings, ocp_qp_ipm_solver_settings.cpp:7-38),
// workspace ownership (what d_ocp_qp_ipm_ws_wrapper did,
// src/detail/d_ocp_qp_ipm_ws_wrapper.cpp:141-155 -- sized once here instead of
// on every solve() as the reference does at ocp_qp_ipm_solver.cpp:185), and
// dispatch to the HIP kernels.  No CPU fallback exists: without a GPU every
// solve returns SRBD_QP_EDEVICE.
#include "../../include/srbd_qp.h"
#include "device_guard.h"
#include "kernels.h"
#include "qp_fields.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <string>
#include <type_traits>
#include <vector>

namespace {

thread_local std::string g_last_error = "";

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

}  // namespace

namespace srbd {
// the thread's last-error message, for the other translation units of the ABI (multi.hip)
int set_error(int code, const std::string& msg) { return fail(code, msg); }

// A buffer the handle allocates on first use and grows on demand (device memory, or pinned
// host memory).  Call with the handle's device current.
struct __attribute__((visibility("hidden"))) Buffer {
  void* p = nullptr;
  size_t bytes = 0;
  bool pinned_host = false;

  // at least `need` bytes; the old block is freed only once the new one is there (contents
  // are not carried over)
  hipError_t reserve(size_t need) {
    if (need <= bytes) return hipSuccess;
    void* fresh = nullptr;
    const hipError_t e = pinned_host ? hipHostMalloc(&fresh, need) : hipMalloc(&fresh, need);
    if (e != hipSuccess) return e;
    release();
    p = fresh;
    bytes = need;
    return hipSuccess;
  }
  void release() {
    if (p) (void)(pinned_host ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    bytes = 0;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};
}  // namespace srbd

struct srbd_qp_handle_s {
  __attribute__((visibility("hidden"))) srbd_qp_handle_s() = default;  // (no exported symbol)
  srbd_qp_dims dims{};
  int capacity = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  double* ws = nullptr;
  size_t ws_qp = 0;  // doubles per QP
  size_t ws_bytes = 0;
  // The buffers allocated on first use (each_buffer lists them)
  // host-solve staging (device)
  srbd::Buffer stage;
  // small host solves (batch 1: the reference's call pattern): pinned mirror of the
  // staging buffer, so inputs go over in one copy and the outputs come back in one
  srbd::Buffer pinned{nullptr, 0, true};
  // nx < 12 or nu < 12: the 12 x 12 embedding (pad.hip)
  srbd::Buffer pad;
  // srbd_qp_solve_soft_f64: the slack state (capacity QPs) and, for embedded problems, the
  // 12-wide soft arrays and slack outputs
  srbd::Buffer soft_ws, soft_pad;
  // srbd_qp_srbd_nmpc_f64: QP data, solution and loop state
  srbd::Buffer nmpc;
  // srbd_qp_srbd_rollout_f64: the step's sqp_iter / converged (capacity ints each), and the
  // dense plan window of one tick (first rollout with a plan or a gait)
  srbd::Buffer roll, roll_plan;
  // srbd_qp_srbd_set_robots_f64: the two roles' pointers (the caller's arrays; all NULL = clear)
  srbd_robots_f64 robots_model{}, robots_plant{};
  // srbd_qp_srbd_set_terrain_f64: the planner's height maps (height == NULL: none)
  srbd_terrain_f64 terrain{};
  // settings.f64_rescue: the compact fp64 batch, and that of the cold fp64 re-solve of
  // rescued QPs the continuation left unsolved
  srbd::Buffer resc, resc2;
  // settings.f32_iters: fp32 copy of the data, fp32 iterate, barrier state
  srbd::Buffer mixed;
  // the latency IPM's lq_fact 1 switch: the compact batch for the batched kernels
  srbd::Buffer lqsw;
  template <typename F>
  void each_buffer(F&& f) {
    for (srbd::Buffer* b : {&stage, &pinned, &pad, &soft_ws, &soft_pad, &nmpc, &roll, &roll_plan, &resc, &resc2, &mixed,
                            &lqsw})
      f(*b);
  }
  int* nmpc_active_host = nullptr;  // pinned
  // Select-index buffers (reserve_select): the unsolved-QP list + status (capacity ints each,
  // then the count) of settings.f64_rescue / f32_iters, and the count's read-back (pinned)
  int* resc_idx = nullptr;
  int* resc_count_host = nullptr;
  // the lq switch's flag (device) and read-back (pinned), and the list, status and count of
  // the QPs that raised it; force_batched while those are solved
  int* lat_flag = nullptr;
  int* lat_flag_host = nullptr;
  int* lqsw_idx = nullptr;
  bool force_batched = false;
  // live-QP control of the IPM launch sequence (ProblemArgsT::ctl): device counters and
  // control words, decided on the device (the host never waits on them)
  int* ctl = nullptr;
  int* qp_buf = nullptr;  // active-QP list of the IPM sweeps: capacity + 1 ints
  // srbd_qp_solve_host_cb_f64: per-QP "factors written" flags (pinned, coherent, first use)
  // and, for the one launch that arms them, their device address (ProblemArgsT::factors_ready)
  int* fac_flags = nullptr;
  int* fac_arm = nullptr;
  // the one-QP host call's resident server (riccati_latency_server_kernel; first use): its
  // mailbox in mapped coherent host memory, its own stream, the arguments it was launched
  // with, launches so far (epoch), requests posted so far
  srbd::LatMailbox* srv_mb = nullptr;
  srbd::LatMailbox* srv_mb_dev = nullptr;
  hipStream_t srv_stream = nullptr;
  srbd::ProblemArgsT<double> srv_args{};
  int srv_epoch = 0;
  int srv_seq = 0;
  bool srv_live = false;
};

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

static bool constrained(const srbd_qp_dims& d) { return d.has_box_u || d.has_box_x || d.ng > 0; }

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
    return fail(e == hipErrorOutOfMemory ? SRBD_QP_ENOMEM : SRBD_QP_EDEVICE,
                std::string("workspace allocation failed: ") + hipGetErrorString(e));
  }
  *out = h;
  return SRBD_QP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// The resident server of the one-QP host call (riccati_latency_server_kernel)
// ---------------------------------------------------------------------------
namespace {
// wall-clock idle time after which a server leaves its CU (the next call relaunches it)
constexpr int kServerIdleMs = 5;
// and leaves after its first answer once this long has passed since its launch: whatever
// shares its hardware queue (other high-priority streams) waits at most about this long
constexpr int kServerLifeMs = 20;
// SRBD_LAT_SERVER_IDLE_MS overrides it (0: the server leaves as soon as it finds no request,
// so a call's post usually lands after the server left -- the test of the relaunch path)
int server_idle_ms() {
  const char* v = std::getenv("SRBD_LAT_SERVER_IDLE_MS");  // (read per launch: tests set it)
  return v && *v ? std::max(0, std::atoi(v)) : kServerIdleMs;
}
// test hook: SRBD_LAT_SERVER_POST_DELAY_US holds the post back this long after the host found
// the server live, so that with a zero idle time the server leaves in between -- every call
// then takes the wait loop's relaunch-after-post branch
int server_post_delay_us() {
  const char* v = std::getenv("SRBD_LAT_SERVER_POST_DELAY_US");
  return v && *v ? std::max(0, std::atoi(v)) : 0;
}
// a request not answered in this long is a device failure (generous: a server launch can
// queue behind long kernels of other streams before it reaches a CU)
constexpr auto kServerTimeout = std::chrono::seconds(30);
std::mutex g_srv_mu;
std::vector<srbd_qp_handle> g_srv_live;  // handles whose server may be running
// at exit: ask every live server to leave and give it a moment to drain (no HIP calls: the
// runtime may already be going down)
void server_atexit() {
  std::lock_guard<std::mutex> lk(g_srv_mu);
  for (srbd_qp_handle h : g_srv_live) {
    volatile srbd::LatMailbox* mb = h->srv_mb;
    mb->flags = srbd::kLatQuit;
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(200);
    while (mb->exited != h->srv_epoch && std::chrono::steady_clock::now() < t_end) std::this_thread::yield();
  }
  g_srv_live.clear();
}
bool server_enabled() {
  const char* v = std::getenv("SRBD_LAT_SERVER");  // 0: every call launches its kernel
  return !(v && v[0] == '0');
}
}  // namespace

// on the handle's device
static void server_stop(srbd_qp_handle h) {
  if (h->srv_live) {
    reinterpret_cast<volatile srbd::LatMailbox*>(h->srv_mb)->flags = srbd::kLatQuit;
    hipStreamSynchronize(h->srv_stream);
    reinterpret_cast<volatile srbd::LatMailbox*>(h->srv_mb)->flags = 0;
    h->srv_live = false;
  }
  // always off the exit hook's list: a handle whose relaunch failed (srv_live false) may
  // still be listed, and srbd_qp_destroy frees it and its mailbox right after this
  std::lock_guard<std::mutex> lk(g_srv_mu);
  g_srv_live.erase(std::remove(g_srv_live.begin(), g_srv_live.end(), h), g_srv_live.end());
}

// (re)launch the server with `a` on the handle's device.  `last_done` is the last request
// number that was answered (or abandoned): the server serves the first mailbox seq that
// differs from it.  Before a post that is h->srv_seq; after the post (the wait loop's
// relaunch of a server that idled out just before it) it is h->srv_seq - 1, or the pending
// request would count as done and never be served.
static hipError_t server_launch(srbd_qp_handle h, const srbd::ProblemArgsT<double>& a, int last_done) {
  hipError_t e = hipSuccess;
  if (!h->srv_mb) {
    e = hipHostMalloc(reinterpret_cast<void**>(&h->srv_mb), sizeof(srbd::LatMailbox),
                      hipHostMallocCoherent | hipHostMallocMapped);
    if (e != hipSuccess) return e;
    std::memset(h->srv_mb, 0, sizeof(srbd::LatMailbox));
    void* dev = nullptr;
    e = hipHostGetDevicePointer(&dev, h->srv_mb, 0);
    if (e == hipSuccess) h->srv_mb_dev = reinterpret_cast<srbd::LatMailbox*>(dev);
    // The server's stream at the greatest priority: HIP maps a process's streams onto a few
    // hardware queues (GPU_MAX_HW_QUEUES, 4 here) per priority, each processing its packets in
    // order, so a kernel of another stream that shares the server's queue would wait until the
    // server leaves.  High-priority streams come from their own queue pool, which only other
    // high-priority streams share (scripts/dev/server_queue_probe.hip: with a plain stream 2 of
    // 8 other streams were held back by a resident kernel, with a high-priority one none).
    int prio_lo = 0, prio_hi = 0;
    if (e == hipSuccess && hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) prio_hi = 0;
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&h->srv_stream, hipStreamNonBlocking, prio_hi);
    if (e != hipSuccess) return e;
    static std::once_flag once;
    std::call_once(once, [] { std::atexit(server_atexit); });
  }
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) != hipSuccess || khz <= 0)
    khz = 100000;
  std::memcpy(&h->srv_args, &a, sizeof a);
  e = srbd::launch_latency_server(a, h->srv_mb_dev, ++h->srv_epoch, last_done, (long long)khz * server_idle_ms(),
                                  (long long)khz * kServerLifeMs, h->srv_stream);
  h->srv_live = e == hipSuccess;
  if (h->srv_live) {
    std::lock_guard<std::mutex> lk(g_srv_mu);
    if (std::find(g_srv_live.begin(), g_srv_live.end(), h) == g_srv_live.end()) g_srv_live.push_back(h);
  }
  return e;
}

// a select-index list: QP list + status (capacity ints each), then the count
static size_t select_idx_bytes(srbd_qp_handle h) { return sizeof(int) * (2 * (size_t)h->capacity + 1); }

// The select-index buffers of a fallback, on the handle's device: the list *idx (resc_idx or
// lqsw_idx), the count's read-back and, with_flag, the lq switch's flag and its read-back.
// What is missing is allocated into locals and committed only when every allocation succeeded,
// so no later call finds the set half there.
static hipError_t reserve_select(srbd_qp_handle h, int** idx, bool with_flag) {
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
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("stream sync: ") + hipGetErrorString(e));
  return SRBD_QP_OK;
}

}  // extern "C"

// The QP arrays of the ABI's structs are listed once, in qp_fields.h
namespace fields = srbd::fields;
static_assert(fields::kStatRowWidth == srbd::kStatCols, "qp_fields.h and kernels.h disagree on the stat row");
namespace {
// visitor of a (source, destination) pair of structs: the destination points where the source does
constexpr auto copy_pointer = [](size_t, const auto& src, auto& dst) { dst = src; };
}  // namespace

template <typename DataT, typename SolT>
static int validate_call(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const DataT* d,
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

static hipError_t rescue_f32(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                             const srbd_qp_data_f32* d, const srbd_qp_solution_f32* s,
                             const int* status, hipStream_t strm, int* rc);
static int mixed_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                     const srbd_qp_data_f64* d, const srbd_qp_solution_f64* s, hipStream_t strm);
static int fallback_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                        const srbd_qp_data_f64* d, const srbd_qp_solution_f64* sc,
                        const srbd_qp_solution_f64* s, hipStream_t strm, int min_status, int* idx,
                        int* count, srbd::Buffer& buf, const double* warm_x = nullptr,
                        const double* warm_u = nullptr);

// The launch arguments of a solve (solve_impl; the resident server's request).
template <typename T, typename DataT, typename SolT>
static srbd::ProblemArgsT<T> build_args(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const DataT* d,
                                        const SolT* s, int* status, const T* warm_bars, int skip_last_rb) {
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
  hipStream_t strm = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
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
    if (ea != hipSuccess) return fail(SRBD_QP_ENOMEM, std::string("rescue buffers: ") + hipGetErrorString(ea));
  }
  int* status = s->status;
  if (rescue && !status) status = h->resc_idx + h->capacity;
  srbd::ProblemArgsT<T> a = build_args<T>(h, batch, st, d, s, status, warm_bars, skip_last_rb);
  // f64_rescue = n: the fp32 pass stops after n iterations at most, the rest is fp64's
  if (rescue && st->f64_rescue < a.iter_max) a.iter_max = st->f64_rescue;
  if (iter_cap >= 0 && iter_cap < a.iter_max) a.iter_max = iter_cap;
  hipError_t e = hipSuccess;
  // (unconstrained with residuals: unconstr_residuals_kernel clears and fills the table)
  if (s->stat && (constrained(h->dims) || !st->compute_residuals))
    e = hipMemsetAsync(s->stat, 0,
                       sizeof(T) * srbd::kStatCols * (size_t)(st->iter_max + 2) * (size_t)batch, strm);
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
      if (e == hipSuccess && rescue) {
        e = rescue_f32(h, batch, st, d, s, status, strm, &rc);
        if (rc) return rc;
      }
    }
  } else {
    // (the single-QP kernel computes the residuals itself when the problem is not embedded)
    run.fuse_res = st->compute_residuals && !padded;
    e = srbd::launch_riccati_unconstr(run, strm);
    if (e == hipSuccess && padded) e = srbd::unpad_solution<T>(a, run, strm);
    // residual norms / objective of the solution when asked for (HPIPM computes them
    // for nc = 0 too; an extra pass over the QP data, so only on request); the stat
    // table's row 0 gets them as well
    if (e == hipSuccess && (s->res || s->obj || s->stat) && !srbd::unconstr_fused_residuals(run)) {
      if (st->compute_residuals) {
        e = srbd::launch_unconstr_residuals<T>(a, strm);
      } else {
        if (s->res) e = hipMemsetAsync(s->res, 0, sizeof(T) * 4 * (size_t)batch, strm);
        if (e == hipSuccess && s->obj) e = hipMemsetAsync(s->obj, 0, sizeof(T) * (size_t)batch, strm);
      }
    }
  }
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
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

static hipError_t rescue_f32(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                             const srbd_qp_data_f32* d, const srbd_qp_solution_f32* s,
                             const int* status, hipStream_t strm, int* rc) {
  *rc = SRBD_QP_OK;
  srbd::DeviceGuard guard(h->device);
  int* idx = h->resc_idx;
  int* count = h->resc_idx + 2 * (size_t)h->capacity;
  hipError_t e = srbd::launch_select_unsolved(status, batch, 1, idx, count, strm);
  if (e == hipSuccess) e = hipMemcpyAsync(h->resc_count_host, count, sizeof(int), hipMemcpyDeviceToHost, strm);
  if (e == hipSuccess) e = hipStreamSynchronize(strm);
  const int R = e == hipSuccess ? *h->resc_count_host : 0;
  if (e != hipSuccess || R == 0) return e;
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
  if (e != hipSuccess) {
    *rc = fail(SRBD_QP_ENOMEM, std::string("rescue batch: ") + hipGetErrorString(e));
    return e;
  }
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
  if (e != hipSuccess) return e;
  srbd_qp_settings st64 = *st;
  st64.warm_start = cont ? 2 : 0;
  st64.f64_rescue = 0;
  st64.f32_iters = 0;
  *rc = solve_impl<double>(h, R, &st64, &d64, &s64, strm, cont ? warm : nullptr);
  if (*rc) return hipSuccess;
  // A QP the continuation leaves unsolved (an fp32 pass can end far off, with the barrier
  // collapsed: t, lam -> 0 at a large stationarity residual, from where a warm-started IPM
  // does not recover) is solved again cold in fp64 (its own list, buffer and idx slots:
  // [capacity, 2 capacity) of resc_idx)
  if (cont) {
    *rc = fallback_f64(h, R, &st64, &d64, &s64, &s64, strm, 1, h->resc_idx + h->capacity,
                       h->resc_idx + 2 * (size_t)h->capacity, h->resc2);
    if (*rc) return hipSuccess;
  }
  fields::for_each_output(m, stat_rows, [&](size_t n, const auto& dst, const auto& src) {
    if (dst && e == hipSuccess) e = srbd::launch_scatter_narrow(src, dst, idx, R, n, strm);
  }, *s, s64);
  if (e == hipSuccess && s->status) e = srbd::launch_scatter_int(s64.status, s->status, idx, R, strm);
  if (e == hipSuccess && s->iter) e = srbd::launch_scatter_int(s64.iter, s->iter, idx, R, strm);
  return e;
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
  hipError_t e = srbd::launch_select_unsolved(sc->status, batch, min_status, idx, count, strm);
  if (e == hipSuccess) e = hipMemcpyAsync(h->resc_count_host, count, sizeof(int), hipMemcpyDeviceToHost, strm);
  if (e == hipSuccess) e = hipStreamSynchronize(strm);
  const int R = e == hipSuccess ? *h->resc_count_host : 0;
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("fallback: ") + hipGetErrorString(e));
  if (R == 0) return SRBD_QP_OK;
  const srbd_qp_dims& m = h->dims;
  const size_t N = (size_t)m.N, nx = (size_t)m.nx, nu = (size_t)m.nu;
  const size_t stat_rows = (size_t)(st->iter_max + 2);
  srbd_qp_data_f64 d2{};
  srbd_qp_solution_f64 s2{};
  const size_t per_qp = passed_elems(m, stat_rows, *d, *s);
  e = buf.reserve(sizeof(double) * per_qp * (size_t)R + 2 * sizeof(int) * (size_t)R + 256);
  if (e != hipSuccess) return fail(SRBD_QP_ENOMEM, std::string("fallback batch: ") + hipGetErrorString(e));
  double* end = compact_batch(m, stat_rows, (size_t)R, buf.as<double>(), *d, *s, d2, s2, e,
                              [&](const double* src, double* dst, size_t n) {
                                return srbd::launch_gather_rows(src, dst, idx, R, n, strm);
                              });
  s2.status = reinterpret_cast<int*>(end);
  s2.iter = s2.status + R;
  const bool warm = warm_x && warm_u && st->warm_start;
  if (warm && e == hipSuccess) e = srbd::launch_gather_rows(warm_x, s2.x, idx, R, (N + 1) * nx, strm);
  if (warm && e == hipSuccess) e = srbd::launch_gather_rows(warm_u, s2.u, idx, R, N * nu, strm);
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("fallback: ") + hipGetErrorString(e));
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
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("fallback: ") + hipGetErrorString(e));
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
    return fail(SRBD_QP_ENOMEM, std::string("mixed-precision buffers: ") + hipGetErrorString(e));
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
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("mixed precision: ") + hipGetErrorString(e));
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
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("mixed precision: ") + hipGetErrorString(e));
  srbd_qp_settings st64 = *st;
  st64.warm_start = 2;
  st64.f32_iters = 0;
  e = reserve_select(h, &h->resc_idx, false);
  if (e != hipSuccess) return fail(SRBD_QP_ENOMEM, std::string("fallback buffers: ") + hipGetErrorString(e));
  srbd_qp_solution_f64 sc = *s;
  if (!sc.status) sc.status = h->resc_idx + h->capacity;
  rc = solve_impl<double>(h, batch, &st64, d, &sc, strm, warm, 0, st->iter_max - n32);
  if (rc) return rc;
  return fallback_f64(h, batch, st, d, &sc, s, strm, 1, h->resc_idx, h->resc_idx + 2 * (size_t)h->capacity,
                      h->resc, keep_x, keep_u);
}

// ---------------------------------------------------------------------------
// host-buffer convenience path
// ---------------------------------------------------------------------------
namespace {
// one polling step of the zero-copy wait: a pause hint where the host has one
inline void spin_pause() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#else
  std::this_thread::yield();
#endif
}
// The single-QP launch is a few tens of microseconds: the zero-copy host solve polls for it
// (the blocking wait's wake-up costs about as much as the kernel), for at most this long; a
// longer solve (or a hung one) falls back to the blocking wait, so no host core spins for more.
constexpr auto kSpinBudget = std::chrono::milliseconds(2);
// flags of srbd_qp_solve_host_cb_f64's early factors: the single-QP kernels' batch limit
constexpr int kFacFlagsMax = 256;
// host solves whose staged bytes fit this go through the handle's pinned buffer
constexpr size_t kPinnedMaxBytes = size_t(8) << 20;
}  // namespace

// stage_d / stage_s set (srbd_qp_host_staging_*): only lay out the pinned staging buffer for
// the fields d / s mark and return pointers into it, so a caller can pack its QPs in place.
// A host pointer that already is its field's place in the staging buffer is not copied.
// on_factors (srbd_qp_solve_host_cb_f64): called once, on success, as soon as P, p, K, k are
// in the caller's buffers -- mid-kernel on the zero-copy single-QP path, else at the end.
template <typename T, typename DataT, typename SolT>
static int solve_host_impl(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                           const DataT* d, const SolT* s, DataT* stage_d = nullptr,
                           SolT* stage_s = nullptr, void (*on_factors)(void*) = nullptr,
                           void* ctx = nullptr) {
  int rc = validate_call(h, batch, st, d, s);
  if (rc) return rc;
  if (batch == 0) return SRBD_QP_OK;
  const srbd_qp_dims& m = h->dims;
  const size_t B = (size_t)batch;
  const size_t stat_rows = (size_t)(st->iter_max + 2);
  // every non-NULL field's range of the staging buffer: inputs in [0, in_end), then outputs
  const fields::StagePlan plan = fields::plan_stage<T>(m, B, stat_rows, *d, *s);
  const size_t off = plan.total, in_end = plan.in_end;
  const size_t ox = plan.x().off, ou = plan.u().off;

  srbd::DeviceGuard guard(h->device);
  hipError_t e = h->stage.reserve(off);
  char* base = h->stage.as<char>();
  // Small problems go through a pinned mirror of the staging buffer: the fields are
  // packed with memcpy and cross PCIe in one DMA each way (per-field pageable copies
  // cost ~10 us of driver latency apiece).  Large ones copy field by field: the
  // pageable path streams at PCIe rate with no extra host pass over the data.
  const bool small = off <= kPinnedMaxBytes;
  char* pin = nullptr;
  if (e == hipSuccess && small) {
    if (off > h->pinned.bytes) {
      server_stop(h);  // (it holds pointers into the old buffer)
      e = h->pinned.reserve(off);
    }
    pin = h->pinned.as<char>();
  }
  if (stage_d) {
    if (e != hipSuccess)
      return fail(SRBD_QP_ENOMEM, std::string("host staging: ") + hipGetErrorString(e));
    if (!small) return fail(SRBD_QP_ECAPACITY, "host staging: the batch's buffers exceed the pinned staging size");
    fields::stage_pointers(plan, pin, m, *stage_d, *stage_s);
    return SRBD_QP_OK;
  }
  // the caller's buffers against the plan's ranges, in the plan's slot order: fn(host pointer,
  // range) for every input the caller passed, fn(host pointer, range, is one of P, p, K, k) for
  // every output
  auto each_input = [&](auto&& fn) {
    int i = 0;
    fields::for_each_input(m, [&](size_t, const auto& f) {
      const fields::StagePlan::Range& g = plan.r[i++];
      if (f) fn(static_cast<const void*>(f), g);
    }, *d);
  };
  auto each_output = [&](auto&& fn) {
    int i = plan.n_in;
    auto visit = [&](size_t, const auto& f) {
      const fields::StagePlan::Range& g = plan.r[i++];
      const void* member = &f;
      if (f) fn(static_cast<void*>(f), g, member == &s->P || member == &s->p || member == &s->K || member == &s->k);
    };
    fields::for_each_solution_field(m, stat_rows, visit, visit, *s);
  };
  // Zero copy: when the launch reads each QP's data exactly once (the single-QP kernel's
  // copy into LDS) and writes each output once, the kernel reads the pinned staging buffer
  // over PCIe and writes its outputs straight into it -- no DMA either way, one launch, one
  // wait (the reference's one-QP-per-solve() call pattern, NMPC_solver.cpp:316-330).
  bool zero_copy = false;
  if (e == hipSuccess && small && !constrained(m)) {
    srbd::ProblemArgsT<T> probe{};
    probe.batch = batch;
    probe.N = m.N;
    probe.nx = m.nx;
    probe.nu = m.nu;
    probe.layout = m.layout;
    probe.fuse_res = st->compute_residuals;
    T dummy = T(0);
    probe.res = s->res ? &dummy : nullptr;
    probe.obj = s->obj ? &dummy : nullptr;
    probe.stat = s->stat ? &dummy : nullptr;
    zero_copy = srbd::unconstr_reads_once(probe);
  }
  if (zero_copy) {
    void* dev = nullptr;
    e = hipHostGetDevicePointer(&dev, pin, 0);
    if (e == hipSuccess) base = reinterpret_cast<char*>(dev);
  }
  // early factors: the latency kernel sets fac_flags[qp] once the QP's P, p, K, k are written
  // (system scope), and the caller's callback runs on them while the kernel finishes
  bool arm = false;
  if constexpr (std::is_same_v<T, double>) {
    if (e == hipSuccess && zero_copy && on_factors && (s->P || s->p || s->K || s->k)) {
      if (!h->fac_flags)
        e = hipHostMalloc(reinterpret_cast<void**>(&h->fac_flags), sizeof(int) * kFacFlagsMax,
                          hipHostMallocCoherent | hipHostMallocMapped);
      void* dev = nullptr;
      if (e == hipSuccess) e = hipHostGetDevicePointer(&dev, h->fac_flags, 0);
      if (e == hipSuccess && batch <= kFacFlagsMax) {
        for (int i = 0; i < batch; ++i) reinterpret_cast<volatile int*>(h->fac_flags)[i] = 0;
        h->fac_arm = reinterpret_cast<int*>(dev);
        arm = true;
      }
    }
  }
  if (e == hipSuccess && small) {
    each_input([&](const void* host, const fields::StagePlan::Range& g) {
      if (host != pin + g.off) std::memmove(pin + g.off, host, g.bytes);  // (staged in place: no copy)
    });
    if (!zero_copy) e = hipMemcpyAsync(base, pin, in_end, hipMemcpyHostToDevice, h->stream);
  } else if (!small) {
    each_input([&](const void* host, const fields::StagePlan::Range& g) {
      if (e == hipSuccess) e = hipMemcpyAsync(base + g.off, host, g.bytes, hipMemcpyHostToDevice, h->stream);
    });
  }
  // warm start: x/u outputs are inputs too
  if (e == hipSuccess && st->warm_start) {
    const size_t bx = plan.x().bytes, bu = plan.u().bytes;
    if (small) {
      if ((const void*)s->x != pin + ox) std::memmove(pin + ox, s->x, bx);
      if ((const void*)s->u != pin + ou) std::memmove(pin + ou, s->u, bu);
      // x and u are adjacent in the staging layout (StagePlan)
      if (!zero_copy) e = hipMemcpyAsync(base + ox, pin + ox, ou + bu - ox, hipMemcpyHostToDevice, h->stream);
    } else {
      e = hipMemcpyAsync(base + ox, s->x, bx, hipMemcpyHostToDevice, h->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(base + ou, s->u, bu, hipMemcpyHostToDevice, h->stream);
    }
  }
  if (e != hipSuccess) {
    // an earlier copy from the pinned buffer may still be queued: drain the stream before
    // the next call may overwrite (or free) that buffer
    hipStreamSynchronize(h->stream);
    return fail(SRBD_QP_EDEVICE, std::string("host->device copy: ") + hipGetErrorString(e));
  }
  DataT dd;
  SolT ss;
  fields::stage_pointers(plan, base, m, dd, ss);
  // One QP that the latency kernel would solve in place: post it to the resident server
  // instead of launching (no launch, dispatch or completion-signal latency).
  bool served = false;
  if constexpr (std::is_same_v<T, double>) {
    if (zero_copy && batch == 1 && server_enabled()) {
      const srbd::ProblemArgsT<double> a = build_args<double>(h, batch, st, &dd, &ss, ss.status, nullptr, 0);
      srbd::ProblemArgsT<double> ar = a;
      ar.fuse_res = st->compute_residuals;  // (not embedded: nx = nu = 12)
      served = srbd::latency_server_ok(ar);
      // the early-factor flags: a fixed pointer for the server's life, switched per request
      // through the mailbox (LatMailbox::arm), so callback and plain calls share one server
      if (served && !h->fac_flags) {
        if (hipHostMalloc(reinterpret_cast<void**>(&h->fac_flags), sizeof(int) * kFacFlagsMax,
                          hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
          h->fac_flags = nullptr;
      }
      void* fdev = nullptr;
      if (served && (!h->fac_flags || hipHostGetDevicePointer(&fdev, h->fac_flags, 0) != hipSuccess)) fdev = nullptr;
      ar.factors_ready = reinterpret_cast<int*>(fdev);
      if (served && arm && !fdev) served = false;  // (cannot happen: arm allocated the flags)
      if (served) {
        // the handle's workspace: earlier work queued on its stream finishes first
        if (hipStreamQuery(h->stream) != hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess && h->srv_live && std::memcmp(&ar, &h->srv_args, sizeof ar) != 0) server_stop(h);
        if (e == hipSuccess &&
            (!h->srv_live || reinterpret_cast<volatile srbd::LatMailbox*>(h->srv_mb)->exited == h->srv_epoch))
          e = server_launch(h, ar, h->srv_seq);  // (before the post: nothing pending)
        volatile srbd::LatMailbox* mb = h->srv_mb;
        if (e == hipSuccess) {
          if (const int us = server_post_delay_us()) std::this_thread::sleep_for(std::chrono::microseconds(us));
          std::atomic_thread_fence(std::memory_order_release);  // the staged QP before the post
          // seq and the request's flags in one 8-byte store (the server reads them as one word)
          const unsigned long long post =
              ((unsigned long long)(unsigned)(arm ? srbd::kLatArm : 0) << 32) | (unsigned)++h->srv_seq;
          *reinterpret_cast<volatile unsigned long long*>(mb) = post;
        }
      }
    }
  }
  if (!served) {
    rc = solve_impl<T>(h, batch, st, &dd, &ss, nullptr);
    if (rc) {
      h->fac_arm = nullptr;
      // copies from the pinned buffer may still be queued: the next call must not
      // overwrite (or free) it under a pending DMA
      hipStreamSynchronize(h->stream);
      return rc;
    }
  }
  h->fac_arm = nullptr;
  if (small) {
    if (e == hipSuccess && in_end < off && !zero_copy)
      e = hipMemcpyAsync(pin + in_end, base + in_end, off - in_end, hipMemcpyDeviceToHost, h->stream);
    // poll for the single-QP launch for at most kSpinBudget, then block (spin_pause above)
    bool fired = false;
    int seen = 0;  // QPs whose early-factor flag is up
    auto factors_check = [&]() {
      if (!arm || fired) return false;
      const volatile int* f = h->fac_flags;
      while (seen < batch && f[seen]) ++seen;
      if (seen < batch) return false;
      std::atomic_thread_fence(std::memory_order_acquire);
      each_output([&](void* host, const fields::StagePlan::Range& g, bool factor) {
        if (factor && host != pin + g.off) std::memmove(host, pin + g.off, g.bytes);
      });
      on_factors(ctx);
      fired = true;
      return true;
    };
    if (e == hipSuccess && served) {
      // wait for the server's answer; it may have left (idle) just before the post: relaunch
      volatile srbd::LatMailbox* mb = h->srv_mb;
      const auto t_end = std::chrono::steady_clock::now() + kServerTimeout;
      for (unsigned n = 1; e == hipSuccess && mb->done != h->srv_seq; ++n) {
        if (factors_check()) continue;
        if (mb->exited == h->srv_epoch) {
          // the server left: it writes `done` before `exited`, so read `done` again -- it may
          // have answered this request before leaving (then a relaunch would solve it twice,
          // the second time under the next call's packing)
          std::atomic_thread_fence(std::memory_order_acquire);
          if (mb->done == h->srv_seq) break;
          // it left before seeing the post: the request is still pending
          e = server_launch(h, h->srv_args, h->srv_seq - 1);
          continue;
        }
        if ((n & 1023) == 0) {
          const hipError_t q = hipStreamQuery(h->srv_stream);
          if (q != hipSuccess && q != hipErrorNotReady) e = q;
          if (e == hipSuccess && std::chrono::steady_clock::now() > t_end) e = hipErrorLaunchTimeOut;
        }
        spin_pause();
      }
      std::atomic_thread_fence(std::memory_order_acquire);
      if (e != hipSuccess) server_stop(h);  // leave no server behind a failed request
    }
    if (e == hipSuccess && zero_copy && !served) {
      const auto t_end = std::chrono::steady_clock::now() + kSpinBudget;
      hipError_t q;
      while ((q = hipStreamQuery(h->stream)) == hipErrorNotReady && std::chrono::steady_clock::now() < t_end) {
        if (factors_check()) continue;
        spin_pause();
      }
      if (q != hipSuccess && q != hipErrorNotReady) e = q;
    }
    if (e == hipSuccess && !served) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess)
      each_output([&](void* host, const fields::StagePlan::Range& g, bool factor) {
        if (host != pin + g.off && !(fired && factor)) std::memmove(host, pin + g.off, g.bytes);
      });
    if (e == hipSuccess && on_factors && !fired) on_factors(ctx);
  } else {
    each_output([&](void* host, const fields::StagePlan::Range& g, bool) {
      if (e == hipSuccess) e = hipMemcpyAsync(host, base + g.off, g.bytes, hipMemcpyDeviceToHost, h->stream);
    });
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && on_factors) on_factors(ctx);
  }
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("device->host copy: ") + hipGetErrorString(e));
  return SRBD_QP_OK;
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
  hipStream_t strm = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
  srbd::DeviceGuard guard(h->device);
  const bool padded = dm.nx != 12 || dm.nu != 12;
  hipError_t ea = h->soft_ws.reserve(srbd::ws_doubles_soft(dm.N) * sizeof(double) * (size_t)h->capacity);
  if (ea == hipSuccess && padded) ea = h->soft_pad.reserve(srbd::pad_soft_elems(h->capacity, dm.N) * sizeof(double));
  if (ea == hipSuccess && padded) ea = h->pad.reserve(srbd::pad_elems(h->capacity, dm.N, 0) * sizeof(double));
  if (ea != hipSuccess) return fail(SRBD_QP_ENOMEM, std::string("soft-box buffers: ") + hipGetErrorString(ea));
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
  if (s->stat)
    e = hipMemsetAsync(s->stat, 0,
                       sizeof(double) * srbd::kStatCols * (size_t)(st->iter_max + 2) * (size_t)batch, strm);
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
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
  return SRBD_QP_OK;
}

// The host-buffer call: one device buffer for the call's arrays, freed before it returns.
static int solve_soft_host_impl(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                                const srbd_qp_data_f64* d, const srbd_qp_soft_f64* sf,
                                const srbd_qp_solution_f64* s, const srbd_qp_slack_f64* sl) {
  int rc = validate_call(h, batch, st, d, s);
  if (rc) return rc;
  if (!sf) return fail(SRBD_QP_EINVAL, "soft is NULL");
  if (s->P || s->p || s->K || s->k || s->stat)
    return fail(SRBD_QP_EINVAL, "srbd_qp_solve_soft_host_f64 does not return P, p, K, k or stat");
  if (batch == 0) return SRBD_QP_OK;
  const srbd_qp_dims& dm = h->dims;
  const fields::StagePlan plan = fields::plan_stage<double>(dm, (size_t)batch, 0, *d, *s, sf, sl);
  srbd::DeviceGuard guard(h->device);
  char* buf = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&buf), plan.total);
  if (e != hipSuccess) return fail(SRBD_QP_ENOMEM, std::string("soft host solve buffer: ") + hipGetErrorString(e));
  srbd_qp_data_f64 dd;
  srbd_qp_soft_f64 ds;
  srbd_qp_solution_f64 dsol;
  srbd_qp_slack_f64 dsl;
  fields::stage_pointers(plan, buf, dm, dd, dsol, &ds, sl ? &dsl : nullptr);
  // the caller's arrays against the plan's ranges, in the plan's slot order
  int slot = 0;
  auto upload = [&](size_t, const auto& host) {
    const fields::StagePlan::Range& g = plan.r[slot++];
    if (host && e == hipSuccess) e = hipMemcpyAsync(buf + g.off, host, g.bytes, hipMemcpyHostToDevice, h->stream);
  };
  auto download = [&](size_t, const auto& host) {
    const fields::StagePlan::Range& g = plan.r[slot++];
    if (host && e == hipSuccess) e = hipMemcpyAsync(host, buf + g.off, g.bytes, hipMemcpyDeviceToHost, h->stream);
  };
  fields::for_each_input(dm, upload, *d);
  fields::for_each_soft_input(dm, upload, *sf);
  if (st->warm_start) {  // x / u outputs are inputs too (the next slots: the solution's first two)
    upload(0, s->x);
    upload(0, s->u);
  }
  if (e == hipSuccess) rc = solve_soft_impl(h, batch, st, &dd, &ds, &dsol, sl ? &dsl : nullptr, h->stream);
  if (e == hipSuccess && rc == SRBD_QP_OK) {
    slot = plan.n_in;
    fields::for_each_solution_field(dm, 0, download, download, *s);
    if (sl) fields::for_each_slack_output(dm, download, *sl);
  }
  const hipError_t es = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = es;
  hipFree(buf);
  if (rc) return rc;
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("soft host solve: ") + hipGetErrorString(e));
  return SRBD_QP_OK;
}

extern "C" {

int srbd_qp_solve_soft_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                           const srbd_qp_data_f64* d, const srbd_qp_soft_f64* sf,
                           const srbd_qp_solution_f64* s, const srbd_qp_slack_f64* sl, void* stream) {
  return solve_soft_impl(h, batch, st, d, sf, s, sl, stream);
}
int srbd_qp_solve_soft_host_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                                const srbd_qp_data_f64* d, const srbd_qp_soft_f64* sf,
                                const srbd_qp_solution_f64* s, const srbd_qp_slack_f64* sl) {
  return solve_soft_host_impl(h, batch, st, d, sf, s, sl);
}
int srbd_qp_solve_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                      const srbd_qp_data_f64* d, const srbd_qp_solution_f64* s, void* stream) {
  return solve_impl<double>(h, batch, st, d, s, stream);
}
int srbd_qp_solve_host_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                           const srbd_qp_data_f64* d, const srbd_qp_solution_f64* s) {
  return solve_host_impl<double>(h, batch, st, d, s);
}
int srbd_qp_solve_host_cb_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                              const srbd_qp_data_f64* d, const srbd_qp_solution_f64* s,
                              void (*on_factors)(void* ctx), void* ctx) {
  return solve_host_impl<double, srbd_qp_data_f64, srbd_qp_solution_f64>(h, batch, st, d, s, nullptr, nullptr,
                                                                       on_factors, ctx);
}
int srbd_qp_host_staging_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                             srbd_qp_data_f64* d, srbd_qp_solution_f64* s) {
  if (!d || !s) return fail(SRBD_QP_EINVAL, "host staging: data / solution struct is NULL");
  const srbd_qp_data_f64 want = *d;
  const srbd_qp_solution_f64 want_s = *s;
  return solve_host_impl<double>(h, batch, st, &want, &want_s, d, s);
}
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

int srbd_qp_srbd_set_terrain_f64(srbd_qp_handle h, const srbd_terrain_f64* terrain) {
  if (!h) return fail(SRBD_QP_EINVAL, "handle is NULL");
  if (h->dims.nx != 12 || h->dims.nu != 12) return fail(SRBD_QP_EDIM, "SRBD terrain needs nx = nu = 12");
  if (!terrain || !terrain->height) {
    h->terrain = srbd_terrain_f64{};
    return SRBD_QP_OK;
  }
  const srbd_terrain_f64& t = *terrain;
  if (t.maps < 1) return fail(SRBD_QP_EINVAL, "set_terrain: maps must be at least 1");
  if (t.nx < 2 || t.ny < 2) return fail(SRBD_QP_EINVAL, "set_terrain: nx and ny must be at least 2");
  if (!(t.cell > 0.0) || !std::isfinite(t.cell)) return fail(SRBD_QP_EINVAL, "set_terrain: cell must be positive");
  if (!std::isfinite(t.x0) || !std::isfinite(t.y0)) return fail(SRBD_QP_EINVAL, "set_terrain: x0, y0 must be finite");
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
  hipStream_t strm = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
  srbd::DeviceGuard guard(h->device);
  const hipError_t e = srbd::launch_srbd_terrain_height(h->terrain, n, xy, map, out, strm);
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
  return SRBD_QP_OK;
}

// The _plan_ entry points hold the checks and the work; the plain ones forward a NULL plan.
// All of them read the handle's robots (srbd_qp_srbd_set_robots_f64).
int srbd_qp_srbd_linearize_plan_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                    const srbd_plan_f64* plan, int constraints, const double* xs,
                                    const double* us, const srbd_qp_data_f64* out, void* stream) {
  if (!h || !params || !xs || !us || !out) return fail(SRBD_QP_EINVAL, "NULL argument");
  const srbd_qp_dims& d = h->dims;
  if (d.nx != 12 || d.nu != 12) return fail(SRBD_QP_EDIM, "SRBD linearisation needs nx = nu = 12");
  if (batch < 0 || batch > h->capacity) return fail(SRBD_QP_ECAPACITY, "batch exceeds capacity");
  if (constraints < SRBD_QP_SRBD_NONE || constraints > SRBD_QP_SRBD_CONE)
    return fail(SRBD_QP_EINVAL, "unknown constraints mode");
  if (!out->A || !out->B || !out->b || !out->Q || !out->S || !out->R || !out->q || !out->r)
    return fail(SRBD_QP_EINVAL, "A, B, b, Q, S, R, q, r outputs are required");
  if (constraints == SRBD_QP_SRBD_BOX_U && (!out->lbu || !out->ubu))
    return fail(SRBD_QP_EINVAL, "BOX_U needs lbu / ubu outputs");
  if (constraints == SRBD_QP_SRBD_CONE &&
      (d.ng != 24 || !out->D || !out->lg || !out->ug || !out->lg_mask || !out->ug_mask))
    return fail(SRBD_QP_EINVAL, "CONE needs ng = 24 and D, lg, ug, lg_mask, ug_mask outputs (C optional)");
  srbd_model_params p = *params;
  if (p.qf_scale <= 0.0) p.qf_scale = (double)d.N;
  hipStream_t strm = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
  srbd::DeviceGuard guard(h->device);
  const hipError_t e = srbd::launch_srbd_linearize(p, batch, d.N, constraints, xs, us, *out, strm, plan,
                                                   &h->robots_model);
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
  return SRBD_QP_OK;
}
int srbd_qp_srbd_linearize_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                               int constraints, const double* xs, const double* us,
                               const srbd_qp_data_f64* out, void* stream) {
  return srbd_qp_srbd_linearize_plan_f64(h, batch, params, nullptr, constraints, xs, us, out, stream);
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
  if (d.nx != 12 || d.nu != 12) return fail(SRBD_QP_EDIM, "SRBD line search needs nx = nu = 12");
  if (batch < 0 || batch > h->capacity) return fail(SRBD_QP_ECAPACITY, "batch exceeds capacity");
  if (!(ls->beta_alpha > 0.0 && ls->beta_alpha < 1.0) || !(ls->alpha_min > 0.0))
    return fail(SRBD_QP_EINVAL, "line search needs 0 < beta_alpha < 1 and alpha_min > 0");
  srbd_model_params p = *params;
  if (p.qf_scale <= 0.0) p.qf_scale = (double)d.N;
  hipStream_t strm = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
  srbd::DeviceGuard guard(h->device);
  const hipError_t e = srbd::launch_srbd_linesearch(p, *ls, batch, d.N, xs, us, dx, du, alpha,
                                                    merit, converged, strm, nullptr, plan, &h->robots_model);
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
  return SRBD_QP_OK;
}
int srbd_qp_srbd_linesearch_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                const srbd_linesearch_params* ls, double* xs, double* us,
                                const double* dx, const double* du, double* alpha, double* merit,
                                int* converged, void* stream) {
  return srbd_qp_srbd_linesearch_plan_f64(h, batch, params, nullptr, ls, xs, us, dx, du, alpha, merit,
                                          converged, stream);
}

int srbd_qp_srbd_nmpc_plan_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                               const srbd_plan_f64* plan, const srbd_linesearch_params* ls,
                               const srbd_qp_settings* settings, int constraints, int sqp_max_loop,
                               double* xs, double* us, const double* x0, double* alpha,
                               int* sqp_iter, int* converged) {
  if (!h || !params || !ls || !settings || !xs || !us || !x0 || !alpha || !sqp_iter || !converged)
    return fail(SRBD_QP_EINVAL, "NULL argument");
  const srbd_qp_dims& d = h->dims;
  if (d.nx != 12 || d.nu != 12) return fail(SRBD_QP_EDIM, "the SRBD NMPC loop needs nx = nu = 12");
  if (batch < 0 || batch > h->capacity) return fail(SRBD_QP_ECAPACITY, "batch exceeds capacity");
  if (sqp_max_loop < 0) return fail(SRBD_QP_EINVAL, "sqp_max_loop must be non-negative");
  if (constraints < SRBD_QP_SRBD_NONE || constraints > SRBD_QP_SRBD_CONE)
    return fail(SRBD_QP_EINVAL, "unknown constraints mode");
  const bool box = constraints == SRBD_QP_SRBD_BOX_U, cone = constraints == SRBD_QP_SRBD_CONE;
  if ((d.has_box_u != 0) != box || (d.ng > 0) != cone || d.has_box_x || (cone && d.ng != 24))
    return fail(SRBD_QP_EINVAL, "the handle's dims do not match the constraints mode");
  int rc = srbd_qp_check_settings(settings);
  if (rc) return rc;
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
  hipError_t e = h->nmpc.reserve(top * sizeof(double));
  if (e == hipSuccess && !h->nmpc_active_host)
    e = hipHostMalloc(reinterpret_cast<void**>(&h->nmpc_active_host), sizeof(int));
  if (e != hipSuccess) {
    return fail(e == hipErrorOutOfMemory ? SRBD_QP_ENOMEM : SRBD_QP_EDEVICE,
                std::string("NMPC scratch allocation failed: ") + hipGetErrorString(e));
  }
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
  srbd_model_params p = *params;
  if (p.qf_scale <= 0.0) p.qf_scale = (double)d.N;
  // NMPC_solver.cpp:362-372: prepareQpStructures; solveQpProblems; if (checkConvergence()) break;
  for (int it = 0; it < sqp_max_loop && e == hipSuccess; ++it) {
    e = srbd::launch_srbd_linearize(p, batch, d.N, constraints, xs, us, qd, strm, plan, &h->robots_model);
    if (e == hipSuccess)
      e = srbd::launch_nmpc_prep(batch, d.N, it, xs, x0, at(bx0), done, sqp_iter, converged, strm);
    if (e != hipSuccess) break;
    rc = solve_impl<double>(h, batch, settings, &qd, &sol, strm);
    if (rc) return rc;
    e = srbd::launch_srbd_linesearch(p, *ls, batch, d.N, xs, us, at(bx), at(bu), alpha, nullptr,
                                     conv, strm, done, plan, &h->robots_model);
    if (e == hipSuccess)
      e = srbd::launch_nmpc_after(batch, it, conv, done, sqp_iter, converged, active, strm);
    if (e == hipSuccess)
      e = hipMemcpyAsync(h->nmpc_active_host, active, sizeof(int), hipMemcpyDeviceToHost, strm);
    if (e == hipSuccess) e = hipStreamSynchronize(strm);
    if (e == hipSuccess && *h->nmpc_active_host == 0) break;  // every robot has converged
  }
  if (e == hipSuccess) e = hipStreamSynchronize(strm);
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("NMPC loop: ") + hipGetErrorString(e));
  return SRBD_QP_OK;
}
int srbd_qp_srbd_nmpc_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                          const srbd_linesearch_params* ls, const srbd_qp_settings* settings,
                          int constraints, int sqp_max_loop, double* xs, double* us,
                          const double* x0, double* alpha, int* sqp_iter, int* converged) {
  return srbd_qp_srbd_nmpc_plan_f64(h, batch, params, nullptr, ls, settings, constraints, sqp_max_loop,
                                    xs, us, x0, alpha, sqp_iter, converged);
}

// ---- the closed loop ----
namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

int srbd_qp_srbd_advance_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                             const srbd_plan_f64* plan, const srbd_advance_f64* adv, double* xs,
                             double* us, double* x, double* u_applied, void* stream) {
  if (!h || !params || !adv || !xs || !us) return fail(SRBD_QP_EINVAL, "NULL argument");
  if (adv->substeps < 1) return fail(SRBD_QP_EINVAL, "advance: substeps must be at least 1");
  const srbd_qp_dims& d = h->dims;
  if (d.nx != 12 || d.nu != 12) return fail(SRBD_QP_EDIM, "the SRBD plant step needs nx = nu = 12");
  if (batch < 0 || batch > h->capacity) return fail(SRBD_QP_ECAPACITY, "batch exceeds capacity");
  if (!aligned16(xs) || !aligned16(us)) return fail(SRBD_QP_EINVAL, "advance: xs / us must be 16-byte aligned");
  if (batch == 0) return SRBD_QP_OK;
  hipStream_t strm = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
  srbd::DeviceGuard guard(h->device);
  srbd::AdvanceIo io{};
  io.substeps = adv->substeps;
  io.xs = xs;
  io.us = us;
  io.x = x;
  io.wrench = adv->wrench;
  io.wrench_stride = 6;
  io.u_out = u_applied;
  io.u_stride = 12;
  const hipError_t e = srbd::launch_srbd_advance(*params, batch, d.N, io, plan, strm, &h->robots_model,
                                                 &h->robots_plant);
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
  return SRBD_QP_OK;
}

// ---- the gait planner ----
namespace {
// the host checks of srbd_qp_srbd_gait_plan_f64 that the replanning rollout shares
int check_gait(srbd_qp_handle h, int batch, const srbd_gait_f64* g, long long tick) {
  const srbd_qp_dims& d = h->dims;
  if (d.nx != 12 || d.nu != 12) return fail(SRBD_QP_EDIM, "the SRBD gait planner needs nx = nu = 12");
  if (batch < 0 || batch > h->capacity) return fail(SRBD_QP_ECAPACITY, "batch exceeds capacity");
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
  hipStream_t strm = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
  srbd::DeviceGuard guard(h->device);
  srbd::GaitIo io{};
  io.cmd = cmd;
  io.cmd_stride = 4;
  io.x = x;
  io.tick = tick;
  io.ref_pose = ref_pose;
  io.foot_now = foot_now;
  io.x_ref = x_ref;
  io.foot_r = foot_r;
  io.foot_l = foot_l;
  io.fz_max = fz_max;
  const hipError_t e =
      srbd::launch_srbd_gait(*params, batch, h->dims.N, *gait, io, strm, &h->robots_model, &h->terrain);
  if (e != hipSuccess) return fail(SRBD_QP_EDEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
  return SRBD_QP_OK;
}

// T ticks of the closed loop: srbd_qp_srbd_rollout_f64 (gait == NULL: the window of tick t is
// gathered out of `plan`) and srbd_qp_srbd_rollout_gait_f64 (the planner writes it).
static int rollout_impl(srbd_qp_handle h, int batch, const srbd_model_params* params,
                        const srbd_plan_f64* plan, const srbd_gait_f64* gait,
                        const srbd_rollout_gait_f64* gio, const srbd_linesearch_params* ls,
                        const srbd_qp_settings* settings, int constraints, int sqp_max_loop,
                        const srbd_rollout_f64* roll, double* xs, double* us, double* x, double* alpha) {
  if (!h || !params || !ls || !settings || !roll || !xs || !us || !x || !alpha)
    return fail(SRBD_QP_EINVAL, "NULL argument");
  if (gait) {
    // (no tick reads a command when there is none)
    if (!gio || (!gio->cmd && roll->ticks > 0) || !gio->ref_pose || !gio->foot_now)
      return fail(SRBD_QP_EINVAL, "NULL argument");
    const int rc = check_gait(h, batch, gait, gio->tick0);
    if (rc) return rc;
  }
  const srbd_qp_dims& d = h->dims;
  if (d.nx != 12 || d.nu != 12) return fail(SRBD_QP_EDIM, "the SRBD NMPC loop needs nx = nu = 12");
  if (batch < 0 || batch > h->capacity) return fail(SRBD_QP_ECAPACITY, "batch exceeds capacity");
  const int T = roll->ticks, P = roll->plan_stages, N = d.N;
  if (T < 0) return fail(SRBD_QP_EINVAL, "rollout: ticks must be non-negative");
  if (roll->substeps < 1) return fail(SRBD_QP_EINVAL, "rollout: substeps must be at least 1");
  if (!(roll->alpha_reset >= 0.0)) return fail(SRBD_QP_EINVAL, "rollout: alpha_reset must be non-negative");
  const bool with_plan = gait || (plan && (plan->x_ref || plan->foot_r || plan->foot_l || plan->fz_max));
  if (!gait && with_plan && (long long)P < (long long)N + T - 1)
    return fail(SRBD_QP_EINVAL, "rollout: the plan needs plan_stages >= N + ticks - 1");
  if (!aligned16(xs) || !aligned16(us)) return fail(SRBD_QP_EINVAL, "rollout: xs / us must be 16-byte aligned");
  {  // the step's own checks (settings, constraints against the handle's dims, ...): a step of
     // zero robots runs them and nothing else
    int none = 0;
    const int rc = srbd_qp_srbd_nmpc_plan_f64(h, 0, params, nullptr, ls, settings, constraints,
                                              sqp_max_loop, xs, us, x, alpha, &none, &none);
    if (rc) return rc;
  }
  if (batch == 0) return SRBD_QP_OK;
  srbd::DeviceGuard guard(h->device);
  hipStream_t strm = h->stream;
  const size_t B = (size_t)h->capacity;
  auto device_error = [&](hipError_t e, const char* what) {
    return fail(e == hipErrorOutOfMemory ? SRBD_QP_ENOMEM : SRBD_QP_EDEVICE,
                std::string(what) + hipGetErrorString(e));
  };
  hipError_t e = hipSuccess;
  if (roll->x_log) {  // x_log[:, 0] = the x passed in
    const srbd::RolloutRow r0{x, roll->x_log, 12, 12, (long long)(T + 1) * 12};
    e = srbd::launch_rollout_rows(batch, &r0, 1, nullptr, 0.0, strm);
    if (e != hipSuccess) return device_error(e, "rollout: ");
  }
  if (T == 0) {
    e = hipStreamSynchronize(strm);
    return e == hipSuccess ? SRBD_QP_OK : device_error(e, "rollout: ");
  }
  // scratch: the step's sqp_iter / converged, and one tick's dense plan window
  e = h->roll.reserve(2 * B * sizeof(int));
  const size_t wx = 12 * ((size_t)N + 1), wf = 3 * (size_t)N, wz = 2 * (size_t)N;
  if (e == hipSuccess && with_plan) e = h->roll_plan.reserve(B * (wx + 2 * wf + wz) * sizeof(double));
  if (e != hipSuccess) return device_error(e, "rollout scratch allocation failed: ");
  int* it_step = h->roll.as<int>();
  int* cv_step = it_step + B;
  // a step that runs no SQP iteration (sqp_max_loop == 0) writes neither
  e = hipMemsetAsync(it_step, 0, 2 * B * sizeof(int), strm);
  if (e != hipSuccess) return device_error(e, "rollout: ");
  srbd_plan_f64 win{};
  srbd::RolloutRow rows[4];
  int nrows = 0;
  if (with_plan) {
    double* w = h->roll_plan.as<double>();
    double* const wxr = w;
    double* const wfr = wxr + B * wx;
    double* const wfl = wfr + B * wf;
    double* const wfz = wfl + B * wf;
    if (gait) win = srbd_plan_f64{wxr, wfr, wfl, wfz};  // the planner writes all four
    const srbd_plan_f64 src = gait ? srbd_plan_f64{} : *plan;  // what is gathered
    if (src.x_ref) {
      win.x_ref = wxr;
      rows[nrows++] = srbd::RolloutRow{src.x_ref, wxr, (int)wx, 12 * ((long long)P + 1), (long long)wx};
    }
    if (src.foot_r) {
      win.foot_r = wfr;
      rows[nrows++] = srbd::RolloutRow{src.foot_r, wfr, (int)wf, 3 * (long long)P, (long long)wf};
    }
    if (src.foot_l) {
      win.foot_l = wfl;
      rows[nrows++] = srbd::RolloutRow{src.foot_l, wfl, (int)wf, 3 * (long long)P, (long long)wf};
    }
    if (src.fz_max) {
      win.fz_max = wfz;
      rows[nrows++] = srbd::RolloutRow{src.fz_max, wfz, (int)wz, 2 * (long long)P, (long long)wz};
    }
  }
  const int per_stage[4] = {12, 3, 3, 2};  // doubles per stage of x_ref, foot_r, foot_l, fz_max
  for (int t = 0; t < T; ++t) {
    // W_t: stages t .. t + N of the long plan, gathered dense; alpha per the reset policy
    srbd::RolloutRow rt[4];
    int n = 0;
    if (gait) {  // W_t from the planner: cmd[:, t], the current x, tick0 + t; row 0 to the logs
      srbd::GaitIo gi{};
      gi.cmd = gio->cmd + (size_t)t * 4;
      gi.cmd_stride = (long long)T * 4;
      gi.x = x;
      gi.tick = gio->tick0 + t;
      gi.ref_pose = gio->ref_pose;
      gi.foot_now = gio->foot_now;
      gi.x_ref = const_cast<double*>(win.x_ref);
      gi.foot_r = const_cast<double*>(win.foot_r);
      gi.foot_l = const_cast<double*>(win.foot_l);
      gi.fz_max = const_cast<double*>(win.fz_max);
      gi.foot_log = gio->foot_log ? gio->foot_log + (size_t)t * 6 : nullptr;
      gi.foot_log_stride = (long long)T * 6;
      gi.fz_log = gio->fz_log ? gio->fz_log + (size_t)t * 2 : nullptr;
      gi.fz_log_stride = (long long)T * 2;
      e = srbd::launch_srbd_gait(*params, batch, N, *gait, gi, strm, &h->robots_model, &h->terrain);
      if (e != hipSuccess) return device_error(e, "rollout: ");
    } else if (with_plan) {
      const double* fields[4] = {plan->x_ref, plan->foot_r, plan->foot_l, plan->fz_max};
      for (int fi = 0; fi < 4; ++fi)
        if (fields[fi]) {
          rt[n] = rows[n];
          rt[n].src = fields[fi] + (size_t)t * per_stage[fi];
          ++n;
        }
    }
    e = srbd::launch_rollout_rows(batch, rt, n, roll->alpha_reset > 0.0 ? alpha : nullptr,
                                  roll->alpha_reset, strm);
    if (e != hipSuccess) return device_error(e, "rollout: ");
    const srbd_plan_f64* wplan = with_plan ? &win : nullptr;
    const int rc = srbd_qp_srbd_nmpc_plan_f64(h, batch, params, wplan, ls, settings, constraints,
                                              sqp_max_loop, xs, us, x, alpha, it_step, cv_step);
    if (rc) return rc;
    srbd::AdvanceIo io{};
    io.substeps = roll->substeps;
    io.xs = xs;
    io.us = us;
    io.x = x;
    io.wrench = roll->wrench ? roll->wrench + (size_t)t * 6 : nullptr;
    io.wrench_stride = (long long)T * 6;
    io.u_out = roll->u_log ? roll->u_log + (size_t)t * 12 : nullptr;
    io.u_stride = (long long)T * 12;
    io.x_out = roll->x_log ? roll->x_log + (size_t)(t + 1) * 12 : nullptr;
    io.x_stride = (long long)(T + 1) * 12;
    io.it_src = it_step;
    io.cv_src = cv_step;
    io.it_log = roll->sqp_iter_log ? roll->sqp_iter_log + t : nullptr;
    io.cv_log = roll->converged_log ? roll->converged_log + t : nullptr;
    io.log_stride = T;
    e = srbd::launch_srbd_advance(*params, batch, N, io, wplan, strm, &h->robots_model, &h->robots_plant);
    if (e != hipSuccess) return device_error(e, "rollout: ");
  }
  e = hipStreamSynchronize(strm);
  if (e != hipSuccess) return device_error(e, "rollout: ");
  return SRBD_QP_OK;
}

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

int srbd_qp_solve_f32(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                      const srbd_qp_data_f32* d, const srbd_qp_solution_f32* s, void* stream) {
  return solve_impl<float>(h, batch, st, d, s, stream);
}
int srbd_qp_solve_host_f32(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                           const srbd_qp_data_f32* d, const srbd_qp_solution_f32* s) {
  return solve_host_impl<float>(h, batch, st, d, s);
}

}  // extern "C"
