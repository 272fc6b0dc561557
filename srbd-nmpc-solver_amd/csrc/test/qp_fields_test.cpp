// qp_fields_test.cpp -- host-only checks of csrc/qp_fields.h (no GPU): every visitor reaches
// each pointer member of its struct exactly once, the per-QP counts equal literals written out
// here, the staging plan is aligned, disjoint, inputs-first, with x and u adjacent, and the
// walkers of a host-buffer call pair each non-NULL field with its range of that plan.
#include "../qp_fields.h"

#include <cstdio>
#include <cstring>
#include <vector>

namespace f = srbd::fields;

static int g_fail = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      ++g_fail;                                                         \
    }                                                                   \
  } while (0)

// N = 3, nx = 5, nu = 2, ng = 4; 7 stat rows
static srbd_qp_dims dims() {
  srbd_qp_dims m{};
  m.N = 3;
  m.nx = 5;
  m.nu = 2;
  m.ng = 4;
  return m;
}
constexpr size_t kStatRows = 7;

// slot i of a struct of pointers holds the sentinel 0x1000 + 8 i
template <class S>
static void fill_sentinels(S& s) {
  for (size_t i = 0; i < sizeof(S) / sizeof(void*); ++i) {
    void* v = reinterpret_cast<void*>(0x1000 + 8 * i);
    std::memcpy(reinterpret_cast<char*>(&s) + i * sizeof(void*), &v, sizeof v);
  }
}

// Counts the visits of each slot of `s`, by the visited member's address and sentinel.
template <class S>
struct Visits {
  const S& s;
  std::vector<int> seen = std::vector<int>(sizeof(S) / sizeof(void*), 0);
  template <class P>
  void operator()(size_t, const P& member) {
    const size_t byte = reinterpret_cast<const char*>(&member) - reinterpret_cast<const char*>(&s);
    CHECK(byte % sizeof(void*) == 0 && byte < sizeof(S));
    if (byte >= sizeof(S)) return;
    CHECK(reinterpret_cast<size_t>(member) == 0x1000 + 8 * (byte / sizeof(void*)));
    ++seen[byte / sizeof(void*)];
  }
  void expect_each_once() const {
    for (int n : seen) CHECK(n == 1);
  }
};

template <class DataT, class SolT>
static void test_visits_twins() {
  const srbd_qp_dims m = dims();
  DataT d;
  fill_sentinels(d);
  Visits<DataT> vd{d};
  f::for_each_input(m, vd, d);
  vd.expect_each_once();
  SolT s;
  fill_sentinels(s);
  Visits<SolT> vs{s};
  f::for_each_solution_field(m, kStatRows, vs, vs, s);
  vs.expect_each_once();
  // the real-valued outputs alone: all but status and iter
  Visits<SolT> vr{s};
  f::for_each_output(m, kStatRows, vr, s);
  int reals = 0;
  for (int n : vr.seen) reals += n;
  CHECK(reals == 10);
  CHECK(vr.seen[(reinterpret_cast<char*>(&s.status) - reinterpret_cast<char*>(&s)) / sizeof(void*)] == 0);
  CHECK(vr.seen[(reinterpret_cast<char*>(&s.iter) - reinterpret_cast<char*>(&s)) / sizeof(void*)] == 0);
}

static void test_visits_soft() {
  const srbd_qp_dims m = dims();
  srbd_qp_soft_f64 sf;
  fill_sentinels(sf);
  Visits<srbd_qp_soft_f64> v{sf};
  f::for_each_soft_input(m, v, sf);
  v.expect_each_once();
  srbd_qp_slack_f64 sl;
  fill_sentinels(sl);
  Visits<srbd_qp_slack_f64> w{sl};
  f::for_each_slack_output(m, w, sl);
  w.expect_each_once();
}

// (member address, expected elements per QP), the expectations written out as literals
struct Want {
  const void* member;
  size_t count;
};
struct CountCheck {
  std::vector<Want> want;
  size_t hits = 0;
  template <class P>
  void operator()(size_t n, const P& member) {
    for (const Want& w : want)
      if (w.member == &member) {
        if (w.count != n) std::printf("count %zu, expected %zu (slot %zu)\n", n, w.count, hits);
        CHECK(w.count == n);
        ++hits;
        return;
      }
    CHECK(!"visited a member the test does not list");
  }
};

static void test_counts() {
  const srbd_qp_dims m = dims();
  srbd_qp_data_f64 d{};
  CountCheck cd{{{&d.A, 75}, {&d.B, 30}, {&d.b, 15}, {&d.Q, 100}, {&d.S, 30}, {&d.R, 12}, {&d.q, 20},
                 {&d.r, 6}, {&d.x0, 5}, {&d.lbu, 6}, {&d.ubu, 6}, {&d.lbu_mask, 6}, {&d.ubu_mask, 6},
                 {&d.lbx, 20}, {&d.ubx, 20}, {&d.lbx_mask, 20}, {&d.ubx_mask, 20}, {&d.C, 80},
                 {&d.D, 24}, {&d.lg, 16}, {&d.ug, 16}, {&d.lg_mask, 16}, {&d.ug_mask, 16}}};
  f::for_each_input(m, cd, d);
  CHECK(cd.hits == 23);
  srbd_qp_data_f32 d32{};
  CountCheck cd32{{{&d32.A, 75}, {&d32.S, 30}, {&d32.C, 80}, {&d32.D, 24}, {&d32.x0, 5}}};
  f::for_each_input(m, [&](size_t n, const auto& p) {
    if (&p == &d32.A || &p == &d32.S || &p == &d32.C || &p == &d32.D || &p == &d32.x0) cd32(n, p);
  }, d32);
  CHECK(cd32.hits == 5);
  srbd_qp_solution_f64 s{};
  CountCheck cs{{{&s.x, 20}, {&s.u, 6}, {&s.pi, 20}, {&s.P, 100}, {&s.p, 20}, {&s.K, 30}, {&s.k, 6},
                 {&s.status, 1}, {&s.iter, 1}, {&s.res, 4}, {&s.obj, 1}, {&s.stat, 126 /* 18 * 7 */}}};
  f::for_each_solution_field(m, kStatRows, cs, cs, s);
  CHECK(cs.hits == 12);
  srbd_qp_soft_f64 sf{};
  CountCheck cf{{{&sf.soft_u, 6}, {&sf.Zl_u, 6}, {&sf.Zu_u, 6}, {&sf.zl_u, 6}, {&sf.zu_u, 6}, {&sf.lls_u, 6},
                 {&sf.lus_u, 6}, {&sf.soft_x, 20}, {&sf.Zl_x, 20}, {&sf.Zu_x, 20}, {&sf.zl_x, 20},
                 {&sf.zu_x, 20}, {&sf.lls_x, 20}, {&sf.lus_x, 20}}};
  f::for_each_soft_input(m, cf, sf);
  CHECK(cf.hits == 14);
  srbd_qp_slack_f64 sl{};
  CountCheck cl{{{&sl.sl_u, 6}, {&sl.su_u, 6}, {&sl.sl_x, 20}, {&sl.su_x, 20}}};
  f::for_each_slack_output(m, cl, sl);
  CHECK(cl.hits == 4);
  // a pair of structs is walked in step
  srbd_qp_data_f32 src{};
  srbd_qp_data_f64 dst{};
  size_t pairs = 0;
  f::for_each_input(m, [&](size_t, const auto& a, auto& b) {
    pairs += (reinterpret_cast<const char*>(&a) - reinterpret_cast<const char*>(&src)) ==
             (reinterpret_cast<char*>(&b) - reinterpret_cast<char*>(&dst));
  }, src, dst);
  CHECK(pairs == 23);
}

// The plan of a batch-2 fp64 call without input boxes and general rows, lbx family present,
// and with some optional outputs left out.
static void test_stage_plan() {
  const srbd_qp_dims m = dims();
  static double mem[1];  // any non-NULL address
  srbd_qp_data_f64 d{};
  d.A = d.B = d.b = d.Q = d.S = d.R = d.q = d.r = d.x0 = mem;
  d.lbx = d.ubx = d.lbx_mask = d.ubx_mask = mem;
  srbd_qp_solution_f64 s{};
  static int imem[1];
  s.x = s.u = s.pi = s.P = s.res = s.stat = mem;
  s.status = imem;
  const size_t batch = 2;
  const f::StagePlan p = f::plan_stage<double>(m, batch, kStatRows, d, s);
  CHECK(p.n == 35 && p.n_in == 23);
  // bytes of the ranges, in slot order, written out: batch * count * 8 (status: * 4); 0 = NULL
  const size_t want[35] = {
      2 * 75 * 8, 2 * 30 * 8, 2 * 15 * 8, 2 * 100 * 8, 2 * 30 * 8, 2 * 12 * 8, 2 * 20 * 8, 2 * 6 * 8, 2 * 5 * 8,
      0, 0, 0, 0,                                      // lbu, ubu and their masks
      2 * 20 * 8, 2 * 20 * 8, 2 * 20 * 8, 2 * 20 * 8,  // lbx, ubx and their masks
      0, 0, 0, 0, 0, 0,                                // C, D, lg, ug and their masks
      2 * 20 * 8, 2 * 6 * 8, 2 * 20 * 8, 2 * 100 * 8, 0, 0, 0,  // x u pi P p K k
      2 * 1 * 4, 0,                                             // status iter
      2 * 4 * 8, 0, 2 * 126 * 8};                               // res obj stat
  size_t sum = 0, sum_in = 0;
  for (int i = 0; i < p.n; ++i) {
    const f::StagePlan::Range& r = p.r[i];
    if (!want[i]) {
      CHECK(r.off == f::kNoOffset);
      continue;
    }
    CHECK(r.off != f::kNoOffset && r.off % 256 == 0);
    CHECK(r.bytes == want[i]);
    const size_t rounded = (want[i] + 255) / 256 * 256;
    sum += rounded;
    if (i < p.n_in) sum_in += rounded;
    for (int j = 0; j < p.n; ++j) {
      if (j == i || p.r[j].off == f::kNoOffset) continue;
      CHECK(r.off + r.bytes <= p.r[j].off || p.r[j].off + p.r[j].bytes <= r.off);  // disjoint
      if (i < p.n_in && j >= p.n_in) CHECK(r.off + r.bytes <= p.r[j].off);        // inputs below outputs
    }
    if (i < p.n_in) CHECK(r.off + r.bytes <= p.in_end);
    else CHECK(r.off >= p.in_end);
  }
  CHECK(p.total == sum);
  CHECK(p.in_end == sum_in);
  CHECK(p.x().bytes == 2 * 20 * 8 && p.u().bytes == 2 * 6 * 8);
  CHECK(p.u().off == p.x().off + 512);  // x: 320 bytes, rounded to 512

  // the structs of pointers at base + offset
  static char base[1];
  srbd_qp_data_f64 dd;
  srbd_qp_solution_f64 ss;
  fill_sentinels(dd);
  fill_sentinels(ss);
  f::stage_pointers(p, base, m, dd, ss);
  CHECK(reinterpret_cast<const char*>(dd.A) == base + p.r[0].off);
  CHECK(reinterpret_cast<const char*>(dd.x0) == base + p.r[8].off);
  CHECK(dd.lbu == nullptr && dd.C == nullptr && dd.ug_mask == nullptr);
  CHECK(reinterpret_cast<const char*>(dd.lbx) == base + p.r[13].off);
  CHECK(reinterpret_cast<char*>(ss.x) == base + p.x().off && reinterpret_cast<char*>(ss.u) == base + p.u().off);
  CHECK(reinterpret_cast<char*>(ss.status) == base + p.r[23 + 7].off);
  CHECK(reinterpret_cast<char*>(ss.stat) == base + p.r[34].off);
  CHECK(ss.p == nullptr && ss.K == nullptr && ss.k == nullptr && ss.iter == nullptr && ss.obj == nullptr);

  // the fp32 twins: half the bytes for the real-valued fields
  srbd_qp_data_f32 d32{};
  static float fmem[1];
  d32.A = d32.B = d32.b = d32.Q = d32.S = d32.R = d32.q = d32.r = d32.x0 = fmem;
  srbd_qp_solution_f32 s32{};
  s32.x = s32.u = s32.pi = fmem;
  s32.iter = imem;
  const f::StagePlan q = f::plan_stage<float>(m, batch, kStatRows, d32, s32);
  CHECK(q.r[0].bytes == 2 * 75 * 4 && q.x().bytes == 2 * 20 * 4 && q.r[23 + 8].bytes == 2 * 1 * 4);
  CHECK(q.u().off == q.x().off + 256);

  // the soft-box call: soft inputs after the data, slack outputs after the solution
  srbd_qp_soft_f64 sf{};
  sf.soft_x = sf.Zl_x = sf.Zu_x = sf.zl_x = sf.zu_x = mem;
  srbd_qp_slack_f64 sl{};
  sl.sl_x = sl.su_x = mem;
  const f::StagePlan t = f::plan_stage<double>(m, batch, kStatRows, d, s, &sf, &sl);
  CHECK(t.n == 53 && t.n_in == 37);
  CHECK(t.r[23].off == f::kNoOffset);                           // soft_u
  CHECK(t.r[23 + 7].off != f::kNoOffset && t.r[23 + 7].off + t.r[23 + 7].bytes <= t.in_end);  // soft_x
  CHECK(t.u().off == t.x().off + 512);
  CHECK(t.r[49].off == f::kNoOffset && t.r[51].off >= t.in_end && t.r[51].bytes == 2 * 20 * 8);  // sl_u, sl_x
  CHECK(t.total == p.total + 5 * 512 + 2 * 512);
}

// The walkers of a host-buffer call: a call with some fields NULL, without and with the soft and
// slack structs.  They visit exactly the non-NULL fields, in slot order, each with the range
// that stage_pointers turns into that field's pointer, and flag exactly P, p, K, k.
struct Visit {
  const void* host;
  const void* staged;  // where stage_pointers puts the field
  bool factor;
};
static void test_walkers(bool with_soft) {
  const srbd_qp_dims m = dims();
  static double mem[64];  // a distinct host address per field
  static int imem[2];
  int next = 0;
  auto fresh = [&] { return &mem[next++]; };
  srbd_qp_data_f64 d{};
  for (const double** p : {&d.A, &d.B, &d.b, &d.Q, &d.S, &d.R, &d.q, &d.r, &d.x0, &d.lbx, &d.ubx, &d.lg, &d.ug})
    *p = fresh();
  srbd_qp_solution_f64 s{};
  for (double** p : {&s.x, &s.u, &s.pi, &s.P, &s.p, &s.k, &s.obj}) *p = fresh();  // no K, res, stat
  s.iter = imem;                                                                  // no status
  srbd_qp_soft_f64 sf{};
  for (const double** p : {&sf.soft_x, &sf.Zl_x, &sf.Zu_x, &sf.zl_x, &sf.zu_x, &sf.lus_x}) *p = fresh();
  srbd_qp_slack_f64 sl{};
  for (double** p : {&sl.sl_x, &sl.su_u}) *p = fresh();
  const srbd_qp_soft_f64* psf = with_soft ? &sf : nullptr;
  const srbd_qp_slack_f64* psl = with_soft ? &sl : nullptr;

  const f::StagePlan p = f::plan_stage<double>(m, 2, kStatRows, d, s, psf, psl);
  std::vector<char> base(p.total);
  srbd_qp_data_f64 dd;
  srbd_qp_solution_f64 ss;
  srbd_qp_soft_f64 dsf;
  srbd_qp_slack_f64 dsl;
  f::stage_pointers(p, base.data(), m, dd, ss, with_soft ? &dsf : nullptr, with_soft ? &dsl : nullptr);

  // what to expect: the non-NULL fields of the caller's structs, paired with the staged ones
  std::vector<Visit> want_in, want_out;
  auto pair_in = [&](size_t, const auto& host, const auto& staged) {
    if (host) want_in.push_back({host, staged, false});
  };
  auto pair_out = [&](size_t, const auto& host, const auto& staged) {
    const void* v = host;
    if (host) want_out.push_back({v, staged, v == s.P || v == s.p || v == s.K || v == s.k});
  };
  f::for_each_input(m, pair_in, d, dd);
  if (with_soft) f::for_each_soft_input(m, pair_in, sf, dsf);
  f::for_each_solution_field(m, kStatRows, pair_out, pair_out, s, ss);
  if (with_soft) f::for_each_slack_output(m, pair_out, sl, dsl);
  CHECK(want_in.size() == (with_soft ? 13u + 6u : 13u));
  CHECK(want_out.size() == (with_soft ? 8u + 2u : 8u));

  std::vector<Visit> got_in, got_out;
  f::each_staged_input(p, m, d, psf, [&](const void* host, const f::StagePlan::Range& g) {
    CHECK(g.off != f::kNoOffset && g.off + g.bytes <= p.in_end && g.bytes > 0);
    got_in.push_back({host, base.data() + g.off, false});
  });
  f::each_staged_output(p, m, s, psl, [&](void* host, const f::StagePlan::Range& g, bool factor) {
    CHECK(g.off != f::kNoOffset && g.off >= p.in_end && g.off + g.bytes <= p.total && g.bytes > 0);
    got_out.push_back({host, base.data() + g.off, factor});
  });
  auto same = [](const std::vector<Visit>& a, const std::vector<Visit>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
      if (a[i].host != b[i].host || a[i].staged != b[i].staged || a[i].factor != b[i].factor) return false;
    return true;
  };
  CHECK(same(got_in, want_in));
  CHECK(same(got_out, want_out));
  int factors = 0;
  for (const Visit& v : got_out) factors += v.factor;
  CHECK(factors == 3);  // P, p, k (K is NULL)
  CHECK(f::kFactorSlot0 == 3 && f::kFactorSlots == 4);
}

int main() {
  test_walkers(false);
  test_walkers(true);
  test_visits_twins<srbd_qp_data_f64, srbd_qp_solution_f64>();
  test_visits_twins<srbd_qp_data_f32, srbd_qp_solution_f32>();
  test_visits_soft();
  test_counts();
  test_stage_plan();
  if (g_fail) {
    std::printf("qp_fields_test: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("qp_fields_test: ok\n");
  return 0;
}
