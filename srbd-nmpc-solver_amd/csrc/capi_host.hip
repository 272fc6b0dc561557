// capi_host.hip -- the host-buffer calls of the C-ABI (include/srbd_qp.h): staging of the
// caller's arrays (pinned mirror, zero copy), the early-factor callback, and the resident
// server that answers the one-QP call without a launch.
#include "capi_handle.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

using namespace srbd::capi;

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
void srbd::capi::server_stop(srbd_qp_handle h) {
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

// The early-factor flags (pinned, coherent; allocated on first use): their device address in
// *dev, NULL where there is none.
static hipError_t fac_flags_device(srbd_qp_handle h, int** dev) {
  *dev = nullptr;
  hipError_t e = hipSuccess;
  if (!h->fac_flags) {
    e = hipHostMalloc(reinterpret_cast<void**>(&h->fac_flags), sizeof(int) * kFacFlagsMax,
                      hipHostMallocCoherent | hipHostMallocMapped);
    if (e != hipSuccess) h->fac_flags = nullptr;
  }
  void* p = nullptr;
  if (e == hipSuccess) e = hipHostGetDevicePointer(&p, h->fac_flags, 0);
  if (e == hipSuccess) *dev = static_cast<int*>(p);
  return e;
}

namespace {
using Range = fields::StagePlan::Range;

// One host-buffer solve: the state its steps share, and the steps in the order solve_host_impl
// runs them.  Each returns the first HIP error; a step runs only while there is none.
template <typename T>
struct HostCall {
  using DataT = std::conditional_t<std::is_same_v<T, double>, srbd_qp_data_f64, srbd_qp_data_f32>;
  using SolT = std::conditional_t<std::is_same_v<T, double>, srbd_qp_solution_f64, srbd_qp_solution_f32>;
  // the call
  srbd_qp_handle h;
  int batch;
  const srbd_qp_settings* st;
  const DataT* d;
  const SolT* s;
  void (*on_factors)(void*);
  void* ctx;
  // every non-NULL field's range of the staging buffer: inputs in [0, in_end), then outputs
  fields::StagePlan plan;
  char* base = nullptr;    // the staging buffer as the device addresses it
  char* pin = nullptr;     // its pinned host mirror (small calls)
  bool small = false;      // through the pinned mirror
  bool zero_copy = false;  // the kernel reads and writes the pinned mirror itself
  bool arm = false;        // this call's launch sets the early-factor flags
  bool served = false;     // posted to the resident server instead of launched
  bool fired = false;      // on_factors has run (early)
  int seen = 0;            // QPs whose early-factor flag is up

  // Small problems go through a pinned mirror of the staging buffer: the fields are
  // packed with memcpy and cross PCIe in one DMA each way (per-field pageable copies
  // cost ~10 us of driver latency apiece).  Large ones copy field by field: the
  // pageable path streams at PCIe rate with no extra host pass over the data.
  hipError_t reserve_staging() {
    hipError_t e = h->stage.reserve(plan.total);
    base = h->stage.as<char>();
    small = plan.total <= kPinnedMaxBytes;
    if (e == hipSuccess && small) {
      if (plan.total > h->pinned.bytes) {
        server_stop(h);  // (it holds pointers into the old buffer)
        e = h->pinned.reserve(plan.total);
      }
      pin = h->pinned.as<char>();
    }
    return e;
  }
  // srbd_qp_host_staging_*: the call ends after reserve_staging (`e`: its result), with pointers
  // into the pinned buffer
  int hand_out_staging(hipError_t e, DataT* stage_d, SolT* stage_s) const {
    if (e != hipSuccess) return hip_fail(SRBD_QP_ENOMEM, "host staging: ", e);
    if (!small) return fail(SRBD_QP_ECAPACITY, "host staging: the batch's buffers exceed the pinned staging size");
    fields::stage_pointers(plan, pin, h->dims, *stage_d, *stage_s);
    return SRBD_QP_OK;
  }

  // Zero copy: when the launch reads each QP's data exactly once (the single-QP kernel's
  // copy into LDS) and writes each output once, the kernel reads the pinned staging buffer
  // over PCIe and writes its outputs straight into it -- no DMA either way, one launch, one
  // wait (the reference's one-QP-per-solve() call pattern, NMPC_solver.cpp:316-330).
  hipError_t decide_zero_copy() {
    const srbd_qp_dims& m = h->dims;
    if (!small || constrained(m)) return hipSuccess;
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
    if (!zero_copy) return hipSuccess;
    void* dev = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&dev, pin, 0);
    if (e == hipSuccess) base = reinterpret_cast<char*>(dev);
    return e;
  }

  // early factors: the latency kernel sets fac_flags[qp] once the QP's P, p, K, k are written
  // (system scope), and the caller's callback runs on them while the kernel finishes
  hipError_t arm_early_factors() {
    if constexpr (std::is_same_v<T, double>) {
      if (!zero_copy || !on_factors || !(s->P || s->p || s->K || s->k)) return hipSuccess;
      int* dev = nullptr;
      const hipError_t e = fac_flags_device(h, &dev);
      if (e == hipSuccess && batch <= kFacFlagsMax) {
        for (int i = 0; i < batch; ++i) reinterpret_cast<volatile int*>(h->fac_flags)[i] = 0;
        h->fac_arm = dev;
        arm = true;
      }
      return e;
    }
    return hipSuccess;
  }

  hipError_t upload_inputs() {
    hipError_t e = hipSuccess;
    if (small) {
      fields::each_staged_input(plan, h->dims, *d, nullptr, [&](const void* host, const Range& g) {
        if (host != pin + g.off) std::memmove(pin + g.off, host, g.bytes);  // (staged in place: no copy)
      });
      if (!zero_copy) e = hipMemcpyAsync(base, pin, plan.in_end, hipMemcpyHostToDevice, h->stream);
    } else {
      fields::each_staged_input(plan, h->dims, *d, nullptr, [&](const void* host, const Range& g) {
        if (e == hipSuccess) e = hipMemcpyAsync(base + g.off, host, g.bytes, hipMemcpyHostToDevice, h->stream);
      });
    }
    if (e == hipSuccess && st->warm_start) e = upload_warm_start();
    return e;
  }
  // warm start: x/u outputs are inputs too
  hipError_t upload_warm_start() {
    const size_t ox = plan.x().off, ou = plan.u().off, bx = plan.x().bytes, bu = plan.u().bytes;
    if (small) {
      if ((const void*)s->x != pin + ox) std::memmove(pin + ox, s->x, bx);
      if ((const void*)s->u != pin + ou) std::memmove(pin + ou, s->u, bu);
      // x and u are adjacent in the staging layout (StagePlan)
      return zero_copy ? hipSuccess
                       : hipMemcpyAsync(base + ox, pin + ox, ou + bu - ox, hipMemcpyHostToDevice, h->stream);
    }
    const hipError_t e = hipMemcpyAsync(base + ox, s->x, bx, hipMemcpyHostToDevice, h->stream);
    return e != hipSuccess ? e : hipMemcpyAsync(base + ou, s->u, bu, hipMemcpyHostToDevice, h->stream);
  }

  // One QP that the latency kernel would solve in place (dd, ss: the staged call): post it to
  // the resident server instead of launching (no launch, dispatch or completion-signal latency).
  hipError_t post_to_server(const DataT& dd, const SolT& ss) {
    hipError_t e = hipSuccess;
    if constexpr (std::is_same_v<T, double>) {
      if (!zero_copy || batch != 1 || !server_enabled()) return e;
      srbd::ProblemArgsT<double> ar = build_args<double>(h, batch, st, &dd, &ss, ss.status, nullptr, 0);
      ar.fuse_res = st->compute_residuals;  // (not embedded: nx = nu = 12)
      served = srbd::latency_server_ok(ar);
      if (!served) return e;
      // the early-factor flags: a fixed pointer for the server's life, switched per request
      // through the mailbox (LatMailbox::arm), so callback and plain calls share one server
      int* fdev = nullptr;
      (void)fac_flags_device(h, &fdev);
      ar.factors_ready = fdev;
      if (arm && !fdev) {  // (cannot happen: arm allocated the flags)
        served = false;
        return e;
      }
      // the handle's workspace: earlier work queued on its stream finishes first
      if (hipStreamQuery(h->stream) != hipSuccess) e = hipStreamSynchronize(h->stream);
      if (e == hipSuccess && h->srv_live && std::memcmp(&ar, &h->srv_args, sizeof ar) != 0) server_stop(h);
      if (e == hipSuccess &&
          (!h->srv_live || reinterpret_cast<volatile srbd::LatMailbox*>(h->srv_mb)->exited == h->srv_epoch))
        e = server_launch(h, ar, h->srv_seq);  // (before the post: nothing pending)
      if (e != hipSuccess) return e;
      volatile srbd::LatMailbox* mb = h->srv_mb;
      if (const int us = server_post_delay_us()) std::this_thread::sleep_for(std::chrono::microseconds(us));
      std::atomic_thread_fence(std::memory_order_release);  // the staged QP before the post
      // seq and the request's flags in one 8-byte store (the server reads them as one word)
      const unsigned long long post =
          ((unsigned long long)(unsigned)(arm ? srbd::kLatArm : 0) << 32) | (unsigned)++h->srv_seq;
      *reinterpret_cast<volatile unsigned long long*>(mb) = post;
    }
    return e;
  }

  // While waiting: once every QP's flag is up, P, p, K, k go to the caller's buffers and the
  // callback runs.  True when it ran in this check.
  bool early_factors() {
    if (!arm || fired) return false;
    const volatile int* f = h->fac_flags;
    while (seen < batch && f[seen]) ++seen;
    if (seen < batch) return false;
    std::atomic_thread_fence(std::memory_order_acquire);
    fields::each_staged_output(plan, h->dims, *s, nullptr, [&](void* host, const Range& g, bool factor) {
      if (factor && host != pin + g.off) std::memmove(host, pin + g.off, g.bytes);
    });
    on_factors(ctx);
    fired = true;
    return true;
  }
  // wait for the server's answer; it may have left (idle) just before the post: relaunch
  hipError_t wait_server() {
    hipError_t e = hipSuccess;
    volatile srbd::LatMailbox* mb = h->srv_mb;
    const auto t_end = std::chrono::steady_clock::now() + kServerTimeout;
    for (unsigned n = 1; e == hipSuccess && mb->done != h->srv_seq; ++n) {
      if (early_factors()) continue;
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
    return e;
  }
  // poll for the single-QP launch for at most kSpinBudget (the blocking wait follows)
  hipError_t wait_spin() {
    const auto t_end = std::chrono::steady_clock::now() + kSpinBudget;
    hipError_t q;
    while ((q = hipStreamQuery(h->stream)) == hipErrorNotReady && std::chrono::steady_clock::now() < t_end) {
      if (early_factors()) continue;
      spin_pause();
    }
    return q != hipErrorNotReady ? q : hipSuccess;
  }

  // The outputs of a small call: wait for them in the pinned mirror, then to the caller's buffers
  // (`e`: the post's result; on_factors runs now unless it ran early).
  hipError_t finish_small(hipError_t e) {
    if (e == hipSuccess && plan.in_end < plan.total && !zero_copy)
      e = hipMemcpyAsync(pin + plan.in_end, base + plan.in_end, plan.total - plan.in_end, hipMemcpyDeviceToHost,
                         h->stream);
    if (e == hipSuccess && served) e = wait_server();
    if (e == hipSuccess && zero_copy && !served) e = wait_spin();
    if (e == hipSuccess && !served) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return e;
    fields::each_staged_output(plan, h->dims, *s, nullptr, [&](void* host, const Range& g, bool factor) {
      if (host != pin + g.off && !(fired && factor)) std::memmove(host, pin + g.off, g.bytes);
    });
    if (on_factors && !fired) on_factors(ctx);
    return e;
  }
  // ... and of a large one: field by field from the device
  hipError_t finish_large(hipError_t e) {
    fields::each_staged_output(plan, h->dims, *s, nullptr, [&](void* host, const Range& g, bool) {
      if (e == hipSuccess) e = hipMemcpyAsync(host, base + g.off, g.bytes, hipMemcpyDeviceToHost, h->stream);
    });
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && on_factors) on_factors(ctx);
    return e;
  }
};
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
  HostCall<T> c{h, batch, st, d, s, on_factors, ctx};
  c.plan = fields::plan_stage<T>(h->dims, (size_t)batch, (size_t)(st->iter_max + 2), *d, *s);
  srbd::DeviceGuard guard(h->device);
  hipError_t e = c.reserve_staging();
  if (stage_d) return c.hand_out_staging(e, stage_d, stage_s);
  if (e == hipSuccess) e = c.decide_zero_copy();
  if (e == hipSuccess) e = c.arm_early_factors();
  if (e == hipSuccess) e = c.upload_inputs();
  if (e != hipSuccess) {
    // an earlier copy from the pinned buffer may still be queued: drain the stream before
    // the next call may overwrite (or free) that buffer
    hipStreamSynchronize(h->stream);
    return hip_fail(SRBD_QP_EDEVICE, "host->device copy: ", e);
  }
  DataT dd;
  SolT ss;
  fields::stage_pointers(c.plan, c.base, h->dims, dd, ss);
  e = c.post_to_server(dd, ss);
  if (!c.served) {
    if constexpr (std::is_same_v<T, double>) rc = srbd_qp_solve_f64(h, batch, st, &dd, &ss, nullptr);
    else rc = srbd_qp_solve_f32(h, batch, st, &dd, &ss, nullptr);
    if (rc) {
      h->fac_arm = nullptr;
      // copies from the pinned buffer may still be queued: the next call must not
      // overwrite (or free) it under a pending DMA
      hipStreamSynchronize(h->stream);
      return rc;
    }
  }
  h->fac_arm = nullptr;
  e = c.small ? c.finish_small(e) : c.finish_large(e);
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "device->host copy: ", e);
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
  if (e != hipSuccess) return hip_fail(SRBD_QP_ENOMEM, "soft host solve buffer: ", e);
  srbd_qp_data_f64 dd;
  srbd_qp_soft_f64 ds;
  srbd_qp_solution_f64 dsol;
  srbd_qp_slack_f64 dsl;
  fields::stage_pointers(plan, buf, dm, dd, dsol, &ds, sl ? &dsl : nullptr);
  auto upload = [&](const void* host, const Range& g) {
    if (e == hipSuccess) e = hipMemcpyAsync(buf + g.off, host, g.bytes, hipMemcpyHostToDevice, h->stream);
  };
  fields::each_staged_input(plan, dm, *d, sf, upload);
  if (st->warm_start) {  // x / u outputs are inputs too
    upload(s->x, plan.x());
    upload(s->u, plan.u());
  }
  if (e == hipSuccess) rc = srbd_qp_solve_soft_f64(h, batch, st, &dd, &ds, &dsol, sl ? &dsl : nullptr, h->stream);
  if (e == hipSuccess && rc == SRBD_QP_OK)
    fields::each_staged_output(plan, dm, *s, sl, [&](void* host, const Range& g, bool) {
      if (e == hipSuccess) e = hipMemcpyAsync(host, buf + g.off, g.bytes, hipMemcpyDeviceToHost, h->stream);
    });
  const hipError_t es = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = es;
  hipFree(buf);
  if (rc) return rc;
  if (e != hipSuccess) return hip_fail(SRBD_QP_EDEVICE, "soft host solve: ", e);
  return SRBD_QP_OK;
}

extern "C" {

int srbd_qp_solve_soft_host_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                                const srbd_qp_data_f64* d, const srbd_qp_soft_f64* sf,
                                const srbd_qp_solution_f64* s, const srbd_qp_slack_f64* sl) {
  return solve_soft_host_impl(h, batch, st, d, sf, s, sl);
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
int srbd_qp_solve_host_f32(srbd_qp_handle h, int batch, const srbd_qp_settings* st,
                           const srbd_qp_data_f32* d, const srbd_qp_solution_f32* s) {
  return solve_host_impl<float>(h, batch, st, d, s);
}

}  // extern "C"
