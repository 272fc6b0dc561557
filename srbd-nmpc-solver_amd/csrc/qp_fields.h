// qp_fields.h -- the arrays of the C-ABI's structs (include/srbd_qp.h), declared once.
//
// Each visitor calls f(elements per QP, member...) for every pointer member of its struct,
// in a fixed order.  The structs come after f, so the same visitor walks one struct
// (f(n, s.A)) or several in step (f(n, src.A, dst.A)): any types with members of these names
// do -- the _f64 and _f32 twins, mixed pairs of them (widen, narrow, gather), the kernels'
// argument structs.  A static_assert per struct ties the number of members visited to the
// struct's size, so a field added to srbd_qp.h but not here stops the build.
//
// Host code only (no HIP): the staging layout of the host-buffer entry points lives here too.
#pragma once

#include <cstddef>
#include <type_traits>

#include "../../include/srbd_qp.h"

namespace srbd {
// (hidden: the instantiations are the library's own, not part of its exported symbols)
namespace fields __attribute__((visibility("hidden"))) {

constexpr size_t kStatRowWidth = 18;  // values per row of the stat table (HPIPM ws->stat)

// The 23 input arrays of srbd_qp_data_*.
template <class F, class... S>
constexpr void for_each_input(const srbd_qp_dims& m, F&& f, S&... s) {
  const size_t N = (size_t)m.N, nx = (size_t)m.nx, nu = (size_t)m.nu, ng = (size_t)m.ng;
  const size_t xs = (N + 1) * nx, us = N * nu, gs = (N + 1) * ng;
  f(N * nx * nx, s.A...); f(N * nx * nu, s.B...); f(N * nx, s.b...);
  f(xs * nx, s.Q...); f(us * nx, s.S...); f(us * nu, s.R...);
  f(xs, s.q...); f(us, s.r...); f(nx, s.x0...);
  f(us, s.lbu...); f(us, s.ubu...); f(us, s.lbu_mask...); f(us, s.ubu_mask...);
  f(xs, s.lbx...); f(xs, s.ubx...); f(xs, s.lbx_mask...); f(xs, s.ubx_mask...);
  f(gs * nx, s.C...); f(N * ng * nu, s.D...);
  f(gs, s.lg...); f(gs, s.ug...); f(gs, s.lg_mask...); f(gs, s.ug_mask...);
}

// The 12 outputs of srbd_qp_solution_*: real(n, member...) for the ten real-valued ones (the
// stat table has stat_rows = iter_max + 2 rows), integer(1, member...) for status and iter.
template <class F, class G, class... S>
constexpr void for_each_solution_field(const srbd_qp_dims& m, size_t stat_rows, F&& real, G&& integer,
                                       S&... s) {
  const size_t N = (size_t)m.N, nx = (size_t)m.nx, nu = (size_t)m.nu;
  const size_t xs = (N + 1) * nx, us = N * nu;
  real(xs, s.x...); real(us, s.u...); real(xs, s.pi...);
  real(xs * nx, s.P...); real(xs, s.p...); real(us * nx, s.K...); real(us, s.k...);
  integer(size_t(1), s.status...); integer(size_t(1), s.iter...);
  real(size_t(4), s.res...); real(size_t(1), s.obj...); real(kStatRowWidth * stat_rows, s.stat...);
}

// The real-valued outputs only, for callers that place status and iter themselves.
template <class F, class... S>
constexpr void for_each_output(const srbd_qp_dims& m, size_t stat_rows, F&& f, S&... s) {
  for_each_solution_field(m, stat_rows, f, [](auto&&...) {}, s...);
}

// The 14 inputs of srbd_qp_soft_f64.
template <class F, class... S>
constexpr void for_each_soft_input(const srbd_qp_dims& m, F&& f, S&... s) {
  const size_t N = (size_t)m.N, xs = (N + 1) * (size_t)m.nx, us = N * (size_t)m.nu;
  f(us, s.soft_u...); f(us, s.Zl_u...); f(us, s.Zu_u...); f(us, s.zl_u...); f(us, s.zu_u...);
  f(us, s.lls_u...); f(us, s.lus_u...);
  f(xs, s.soft_x...); f(xs, s.Zl_x...); f(xs, s.Zu_x...); f(xs, s.zl_x...); f(xs, s.zu_x...);
  f(xs, s.lls_x...); f(xs, s.lus_x...);
}

// The 4 outputs of srbd_qp_slack_f64.
template <class F, class... S>
constexpr void for_each_slack_output(const srbd_qp_dims& m, F&& f, S&... s) {
  const size_t N = (size_t)m.N, xs = (N + 1) * (size_t)m.nx, us = N * (size_t)m.nu;
  f(us, s.sl_u...); f(us, s.su_u...); f(xs, s.sl_x...); f(xs, s.su_x...);
}

// The 4 arrays of srbd_plan_f64 (per-robot, per-stage overrides of srbd_model_params; 12 x 12
// stages: the SRBD entry points need nx = nu = 12).
template <class F, class... S>
constexpr void for_each_plan_field(const srbd_qp_dims& m, F&& f, S&... s) {
  const size_t N = (size_t)m.N;
  f((N + 1) * 12, s.x_ref...); f(N * 3, s.foot_r...); f(N * 3, s.foot_l...); f(N * 2, s.fz_max...);
}

namespace detail {
template <class DataT>
constexpr size_t count_inputs() {
  size_t n = 0;
  DataT d{};
  for_each_input(srbd_qp_dims{}, [&n](size_t, auto&) { ++n; }, d);
  return n;
}
template <class SolT>
constexpr size_t count_solution_fields() {
  size_t n = 0;
  SolT s{};
  for_each_solution_field(srbd_qp_dims{}, 0, [&n](size_t, auto&) { ++n; }, [&n](size_t, auto&) { ++n; }, s);
  return n;
}
constexpr size_t count_soft_inputs() {
  size_t n = 0;
  srbd_qp_soft_f64 s{};
  for_each_soft_input(srbd_qp_dims{}, [&n](size_t, auto&) { ++n; }, s);
  return n;
}
constexpr size_t count_slack_outputs() {
  size_t n = 0;
  srbd_qp_slack_f64 s{};
  for_each_slack_output(srbd_qp_dims{}, [&n](size_t, auto&) { ++n; }, s);
  return n;
}
constexpr size_t count_plan_fields() {
  size_t n = 0;
  srbd_plan_f64 s{};
  for_each_plan_field(srbd_qp_dims{}, [&n](size_t, auto&) { ++n; }, s);
  return n;
}
}  // namespace detail

constexpr size_t kDataFields = detail::count_inputs<srbd_qp_data_f64>();
constexpr size_t kSolutionFields = detail::count_solution_fields<srbd_qp_solution_f64>();
constexpr size_t kSoftFields = detail::count_soft_inputs();
constexpr size_t kSlackFields = detail::count_slack_outputs();
constexpr size_t kPlanFields = detail::count_plan_fields();
static_assert(kDataFields == sizeof(srbd_qp_data_f64) / sizeof(void*) &&
                  kDataFields == sizeof(srbd_qp_data_f32) / sizeof(void*),
              "for_each_input must visit every member of srbd_qp_data_*");
static_assert(kSolutionFields == sizeof(srbd_qp_solution_f64) / sizeof(void*) &&
                  kSolutionFields == sizeof(srbd_qp_solution_f32) / sizeof(void*),
              "for_each_solution_field must visit every member of srbd_qp_solution_*");
static_assert(kSoftFields == sizeof(srbd_qp_soft_f64) / sizeof(void*),
              "for_each_soft_input must visit every member of srbd_qp_soft_f64");
static_assert(kSlackFields == sizeof(srbd_qp_slack_f64) / sizeof(void*),
              "for_each_slack_output must visit every member of srbd_qp_slack_f64");

static_assert(kPlanFields == sizeof(srbd_plan_f64) / sizeof(void*),
              "for_each_plan_field must visit every member of srbd_plan_f64");

// ---------------------------------------------------------------------------
// The staging layout of a host-buffer call: one buffer, every non-NULL field of the call at a
// 256-byte-aligned offset.  Slots are in visiting order -- data, soft inputs (if any), then
// solution, slack outputs (if any) -- so all inputs lie in [0, in_end) and go over in one copy,
// and x and u are adjacent (the warm start uploads them as one range).
// ---------------------------------------------------------------------------
constexpr size_t kNoOffset = (size_t)-1;
constexpr size_t stage_round(size_t bytes) { return (bytes + 255) / 256 * 256; }

struct StagePlan {
  struct Range {
    size_t off = kNoOffset;  // kNoOffset: the caller passed NULL, no range
    size_t bytes = 0;
  };
  Range r[kDataFields + kSoftFields + kSolutionFields + kSlackFields];
  int n = 0;          // slots used
  int n_in = 0;       // of which inputs
  size_t in_end = 0;  // bytes of the inputs' ranges
  size_t total = 0;

  const Range& x() const { return r[n_in]; }  // the solution's first two slots
  const Range& u() const { return r[n_in + 1]; }

  void add(bool present, size_t bytes) {
    Range& g = r[n++];
    if (!present) return;
    g.off = total;
    g.bytes = bytes;
    total += stage_round(bytes);
  }
};

// T: the call's real type.  sf / sl: the soft-box call's extra structs, or NULL.
template <class T, class DataT, class SolT>
StagePlan plan_stage(const srbd_qp_dims& m, size_t batch, size_t stat_rows, const DataT& d, const SolT& s,
                     const srbd_qp_soft_f64* sf = nullptr, const srbd_qp_slack_f64* sl = nullptr) {
  StagePlan p;
  auto real = [&](size_t n, const auto& f) { p.add(f != nullptr, batch * n * sizeof(T)); };
  auto integer = [&](size_t n, const auto& f) { p.add(f != nullptr, batch * n * sizeof(int)); };
  for_each_input(m, real, d);
  if (sf) for_each_soft_input(m, real, *sf);
  p.n_in = p.n;
  p.in_end = p.total;
  for_each_solution_field(m, stat_rows, real, integer, s);
  if (sl) for_each_slack_output(m, real, *sl);
  return p;
}

// The structs of pointers at base + offset (NULL where the plan has no range), in the plan's
// slot order.
template <class DataT, class SolT>
void stage_pointers(const StagePlan& p, char* base, const srbd_qp_dims& m, DataT& d, SolT& s,
                    srbd_qp_soft_f64* sf = nullptr, srbd_qp_slack_f64* sl = nullptr) {
  int i = 0;
  auto at = [&](size_t, auto& f) {
    const size_t off = p.r[i++].off;
    f = off == kNoOffset ? nullptr : reinterpret_cast<std::remove_reference_t<decltype(f)>>(base + off);
  };
  for_each_input(m, at, d);
  if (sf) for_each_soft_input(m, at, *sf);
  for_each_solution_field(m, 0, at, at, s);
  if (sl) for_each_slack_output(m, at, *sl);
}

// The caller's host arrays against the plan's ranges, in the plan's slot order (d, s, sf and sl
// as plan_stage got them): fn(host pointer, range) for every non-NULL input ...
template <class DataT, class Fn>
void each_staged_input(const StagePlan& p, const srbd_qp_dims& m, const DataT& d, const srbd_qp_soft_f64* sf,
                       Fn&& fn) {
  int i = 0;
  auto visit = [&](size_t, const auto& f) {
    const StagePlan::Range& g = p.r[i++];
    if (f) fn(static_cast<const void*>(f), g);
  };
  for_each_input(m, visit, d);
  if (sf) for_each_soft_input(m, visit, *sf);
}

// ... and fn(host pointer, range, is one of P, p, K, k) for every non-NULL output.  The factors
// are the solution's slots 3 to 6:
constexpr int kFactorSlot0 = 3, kFactorSlots = 4;
namespace detail {
constexpr bool factor_slots_are_PpKk() {
  srbd_qp_solution_f64 s{};
  int i = 0;
  bool ok = true;
  auto visit = [&](size_t, auto& f) {
    const void* member = &f;
    const bool factor = member == static_cast<const void*>(&s.P) || member == static_cast<const void*>(&s.p) ||
                        member == static_cast<const void*>(&s.K) || member == static_cast<const void*>(&s.k);
    ok = ok && factor == (i >= kFactorSlot0 && i < kFactorSlot0 + kFactorSlots);
    ++i;
  };
  for_each_solution_field(srbd_qp_dims{}, 0, visit, visit, s);
  return ok;
}
}  // namespace detail
static_assert(detail::factor_slots_are_PpKk(), "kFactorSlot0 / kFactorSlots must name P, p, K, k");

template <class SolT, class Fn>
void each_staged_output(const StagePlan& p, const srbd_qp_dims& m, const SolT& s, const srbd_qp_slack_f64* sl,
                        Fn&& fn) {
  int i = p.n_in;
  auto visit = [&](size_t, const auto& f) {
    const int slot = i - p.n_in;
    const StagePlan::Range& g = p.r[i++];
    if (f) fn(static_cast<void*>(f), g, slot >= kFactorSlot0 && slot < kFactorSlot0 + kFactorSlots);
  };
  for_each_solution_field(m, 0, visit, visit, s);
  if (sl) for_each_slack_output(m, visit, *sl);
}

}  // namespace fields
}  // namespace srbd
