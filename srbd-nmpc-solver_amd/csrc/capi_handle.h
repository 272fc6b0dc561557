// capi_handle.h -- what the translation units of the C-ABI (include/srbd_qp.h) share: the
// handle and its buffers, the error helpers, and the few functions that cross between
// srbd_qp_capi.hip (handle, settings), capi_solve.hip (device-pointer solves), capi_backward.hip
// (their backward pass), capi_host.hip (host-buffer solves, the resident server) and
// capi_srbd.hip (the SRBD entry points).
// Private to the library: nothing declared here is exported but srbd::set_error.
#pragma once

#include "../../include/srbd_qp.h"
#include "device_guard.h"
#include "kernels.h"
#include "qp_backward_rows.h"
#include "qp_fields.h"

#include <hip/hip_runtime.h>

#include <string>

namespace srbd {
// sets the thread's last-error message (defined once, srbd_qp_capi.hip) and returns `code`
int set_error(int code, const std::string& msg);

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
  // srbd_qp_srbd_set_contact_f64: the plant's contact model and fall detection (a copy of the
  // caller's struct; has_contact false: none)
  srbd_contact_f64 contact{};
  bool has_contact = false;
  // srbd_qp_srbd_set_active_f64: which robots the NMPC step steps (a copy of the caller's
  // struct; has_active false: all of them, the launches of a handle that never had one)
  srbd_active_f64 active{};
  bool has_active = false;
  // srbd_qp_srbd_step_work: the work of the last NMPC step, or of a rollout's steps
  long long work_qp_solves = 0, work_sqp_iterations = 0;
  // settings.f64_rescue: the compact fp64 batch, and that of the cold fp64 re-solve of
  // rescued QPs the continuation left unsolved
  srbd::Buffer resc, resc2;
  // settings.f32_iters: fp32 copy of the data, fp32 iterate, barrier state
  srbd::Buffer mixed;
  // the latency IPM's lq_fact 1 switch: the compact batch for the batched kernels
  srbd::Buffer lqsw;
  // srbd_qp_solve_backward_f64: the adjoint solution, its zero b / x0 and, with input boxes, the
  // masked stages and the pinned counts (capacity QPs); bwd_counted: the QPs whose counts the
  // last backward pass wrote (srbd_qp_backward_pinned_f64); bwd_active: the same for the three
  // counts of srbd_qp_solve_backward_rows_f64 (srbd_qp_backward_active_f64)
  srbd::Buffer bwd;
  int bwd_counted = 0;
  int bwd_active = 0;
  // srbd_qp_srbd_linearize_backward_f64: the per-stage parts of the robots' sums (capacity QPs)
  srbd::Buffer lin_bwd;
  // srbd_qp_srbd_solve_backward_f64: what the lift kernel hands to the fused stage kernel, per
  // stage nu, dnu (2 ng doubles, ng > 0) and the gradient of ubu (nu doubles, has_box_u); capacity QPs
  srbd::Buffer bwd_fused;
  template <typename F>
  void each_buffer(F&& f) {
    for (srbd::Buffer* b : {&stage, &pinned, &pad, &soft_ws, &soft_pad, &nmpc, &roll, &roll_plan, &resc, &resc2, &mixed,
                            &lqsw, &bwd, &lin_bwd, &bwd_fused})
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
  // the compacted NMPC step of a batch above the single-QP kernels' limit: its sub-batches are
  // solved by the streaming Riccati kernel too, whatever their size (set around those solves)
  bool riccati_streaming = false;
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

namespace srbd {
// (hidden: the library's own, not part of its exported symbols)
namespace capi __attribute__((visibility("hidden"))) {

// The QP arrays of the ABI's structs are listed once, in qp_fields.h
namespace fields = srbd::fields;
static_assert(fields::kStatRowWidth == srbd::kStatCols, "qp_fields.h and kernels.h disagree on the stat row");

inline int fail(int code, const std::string& msg) { return set_error(code, msg); }
// a failed HIP call: the site's error code and prefix, then HIP's text
inline int hip_fail(int code, const char* what, hipError_t e) {
  return set_error(code, std::string(what) + hipGetErrorString(e));
}
// the code of a failed allocation
inline int alloc_code(hipError_t e) { return e == hipErrorOutOfMemory ? SRBD_QP_ENOMEM : SRBD_QP_EDEVICE; }

inline bool constrained(const srbd_qp_dims& d) { return d.has_box_u || d.has_box_x || d.ng > 0; }

// the caller's stream, or the handle's own
inline hipStream_t stream_of(srbd_qp_handle h, void* stream) {
  return stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
}

// What crosses between the translation units.  (A device solve from another unit is a call of
// the public srbd_qp_solve_f64 / _f32 / _soft_f64: each is solve_impl or solve_soft_impl alone.)
// srbd_qp_capi.hip: the select-index buffers of a fallback, on the handle's device -- the list
// *idx (resc_idx or lqsw_idx), the count's read-back and, with_flag, the lq switch's flag
hipError_t reserve_select(srbd_qp_handle h, int** idx, bool with_flag);
// capi_solve.hip: the checks of a call (instantiated for the f64 and the f32 structs), and the
// launch arguments of a solve (solve_impl; <double>: the resident server's request)
template <typename DataT, typename SolT>
int validate_call(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const DataT* d, const SolT* s);
template <typename T, typename DataT, typename SolT>
srbd::ProblemArgsT<T> build_args(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const DataT* d,
                                 const SolT* s, int* status, const T* warm_bars, int skip_last_rb);
// capi_backward.hip: the checks of a backward call up to (not including) batch == 0 (rows: those of
// srbd_qp_solve_backward_rows_f64; have_grad: an output struct was passed), and the front half the
// backward entry points share -- counts, projection or mask, the adjoint Riccati solve -- for a
// call that has passed them with batch > 0, on the handle's device.  rows: the lift kernel's
// arguments with every output NULL.
struct BackwardAdjoint {
  const double *dx, *du, *dpi;
  srbd::BackwardRowsArgs rows;
};
int backward_check(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const srbd_qp_data_f64* d,
                   const srbd_qp_solution_f64* s, const double* gx, const double* gu, double act_tol, bool rows,
                   double rank_tol, bool have_grad);
int backward_adjoint(srbd_qp_handle h, int batch, const srbd_qp_settings* st, const srbd_qp_data_f64* d,
                     const srbd_qp_solution_f64* s, const double* gx, const double* gu, double act_tol, bool rows,
                     double rank_tol, hipStream_t strm, BackwardAdjoint* out);
// capi_host.hip: stops the handle's resident server, if any; on the handle's device
void server_stop(srbd_qp_handle h);

}  // namespace capi
}  // namespace srbd
