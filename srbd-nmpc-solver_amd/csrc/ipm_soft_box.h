// ipm_soft_box.h -- the soft-box algebra of the batched IPM (SOFT kernels; ipm_soft.hip).
// No include guard: included by ipm_box_impl.h inside the precision namespace.

// ---- soft boxes (SOFT kernels only; HPIPM's Zl / Zu / zl / zu / lls / lus) ----
// A soft bound on v has a slack s >= sb on each active side, penalised by 1/2 Z s^2 + z s:
//   t = w + s - bound (w = v - lb below, ub - v above),  t_s = s - sb,
//   r_s = Z s + z - lam - lam_s                 (stationarity in s),
//   dlam = -g - Gamma (dw + ds),  dlam_s = -g_s - Gamma_s ds   (Gamma = lam / t, g as gamma_of).
// The slack's row Z ds - dlam - dlam_s + r_s = 0 is solved lane-locally,
//   ds = -(r_s + g + g_s + Gamma dw) / Zt,  Zt = Z + Gamma + Gamma_s,
// which leaves the variable's own row with
//   Gamma_eff = Gamma (Z + Gamma_s) / Zt,  g_eff = g - Gamma (r_s + g + g_s) / Zt
// in place of Gamma, g: the Riccati recursion sees a diagonal barrier Hessian as before.
struct SoftIn {   // the variable's soft data: on = 1 if soft, penalties, slack bounds
  real on, Zl, Zu, zl, zu, bl, bu;
};
struct SoftSt {   // slacks, and the slack bounds' t and lam
  real sl, su, tl, tu, ll, lu;
};
struct SoftStep {
  real dsl, dsu, dtl, dtu, dll, dlu;
};
__device__ __forceinline__ SoftSt load_soft(const real* p, int i) {
  p += kSoftSt;
  return SoftSt{p[i], p[12 + i], p[24 + i], p[36 + i], p[48 + i], p[60 + i]};
}
__device__ __forceinline__ void store_soft(real* p, int i, const SoftSt& s) {
  p += kSoftSt;
  p[i] = s.sl; p[12 + i] = s.su; p[24 + i] = s.tl; p[36 + i] = s.tu; p[48 + i] = s.ll; p[60 + i] = s.lu;
}
__device__ __forceinline__ SoftStep load_sstep(const real* p, int i) {
  p += kSoftDlt;
  return SoftStep{p[i], p[12 + i], p[24 + i], p[36 + i], p[48 + i], p[60 + i]};
}
__device__ __forceinline__ void store_sstep(real* p, int i, const SoftStep& d) {
  p += kSoftDlt;
  p[i] = d.dsl; p[12 + i] = d.dsu; p[24 + i] = d.dtl; p[36 + i] = d.dtu; p[48 + i] = d.dll; p[60 + i] = d.dlu;
}
// The soft arrays of one QP (dense per variable like the bounds; every load at a valid
// address, masked after: see Ctx::side_at)
struct SoftView {
  const SoftArgsT<real>& s;
  int N, nx, nu;
  size_t q;
  __device__ real* st(int k, int which) const {
    return s.sws + q * s.sws_qp + (size_t)k * kSoftStage + which * kSoftFam;
  }
  __device__ static SoftIn in_at(const real* soft, const real* Zl, const real* Zu, const real* zl,
                                 const real* zu, const real* bl, const real* bu, size_t o, bool ok) {
    const real m = soft[o], a = Zl[o], b = Zu[o], c = zl[o], d = zu[o];
    const real e = (bl ? bl : soft)[o], f = (bu ? bu : soft)[o];
    const bool on = ok && m != real(0.0);
    const real z = real(0.0);
    return SoftIn{on ? real(1.0) : z, on ? a : z, on ? b : z, on ? c : z, on ? d : z,
                  on && bl ? e : z, on && bu ? f : z};
  }
  __device__ SoftIn in_u(int k, int i) const {
    if (!s.soft_u) return SoftIn{0, 0, 0, 0, 0, 0, 0};
    const bool ok = i < nu && k < N;
    const size_t o = (q * N + (k < N ? k : N - 1)) * nu + (ok ? i : 0);
    return in_at(s.soft_u, s.Zl_u, s.Zu_u, s.zl_u, s.zu_u, s.lls_u, s.lus_u, o, ok);
  }
  __device__ SoftIn in_x(int k, int i) const {
    if (!s.soft_x) return SoftIn{0, 0, 0, 0, 0, 0, 0};
    const bool ok = i < nx && k > 0;  // stage-0 x bounds dropped
    const size_t o = (q * (N + 1) + k) * nx + (ok ? i : 0);
    return in_at(s.soft_x, s.Zl_x, s.Zu_x, s.zl_x, s.zu_x, s.lls_x, s.lus_x, o, ok);
  }
};
// One active side of a soft variable in side-local terms (w, lam, t: the bound's pair; s, ts,
// ls: the slack and its bound's pair; ext / exs: the corrector's predictor products).
struct SoftOne {
  real Gl, rd, rm, rds, rms, rsum, Zt, Geff, geff;
};
__device__ __forceinline__ SoftOne soft_one(real w, real lam, real t, real s, real ts, real ls, real Z,
                                            real z, real sb, real ext, real exs, real smu) {
  SoftOne o;
  o.rd = w + s - t;
  o.rm = lam * t + ext - smu;
  o.Gl = lam / t;
  const real gl = (o.rm + lam * o.rd) / t;
  o.rds = s - sb - ts;
  o.rms = ls * ts + exs - smu;
  const real Gs = ls / ts;
  const real gs = (o.rms + ls * o.rds) / ts;
  o.rsum = Z * s + z - lam - ls + gl + gs;
  o.Zt = Z + o.Gl + Gs;
  o.Geff = o.Gl * (Z + Gs) / o.Zt;
  o.geff = gl - o.Gl * o.rsum / o.Zt;
  return o;
}
// gamma_of for a variable that may be soft
__device__ __forceinline__ void gamma_soft(const Side& s, const Bar& b, const SoftIn& si, const SoftSt& ss,
                                           real v, real ext_l, real ext_u, real exs_l, real exs_u, real smu,
                                           real& G, real& g) {
  if (si.on == real(0.0)) {
    gamma_of(s, b, v, ext_l, ext_u, smu, G, g);
    return;
  }
  G = real(0.0);
  g = real(0.0);
  if (s.ml != real(0.0)) {
    const SoftOne o = soft_one(v - s.lb, b.ll, b.tl, ss.sl, ss.tl, ss.ll, si.Zl, si.zl, si.bl, ext_l, exs_l, smu);
    G += o.Geff;
    g += o.geff;
  }
  if (s.mu != real(0.0)) {
    const SoftOne o = soft_one(s.ub - v, b.lu, b.tu, ss.su, ss.tu, ss.lu, si.Zu, si.zu, si.bu, ext_u, exs_u, smu);
    G += o.Geff;
    g -= o.geff;
  }
}
// bar_step for a variable that may be soft: ds from dv, then dt / dlam of both pairs
__device__ __forceinline__ void soft_step(const Side& s, const Bar& b, const SoftIn& si, const SoftSt& ss,
                                          real v, real dv, real ext_l, real ext_u, real exs_l, real exs_u,
                                          real smu, BarStep& d, SoftStep& e) {
  e = SoftStep{0, 0, 0, 0, 0, 0};
  if (si.on == real(0.0)) {
    d = bar_step(s, b, v, dv, ext_l, ext_u, smu);
    return;
  }
  d = BarStep{0, 0, 0, 0};
  if (s.ml != real(0.0)) {
    const SoftOne o = soft_one(v - s.lb, b.ll, b.tl, ss.sl, ss.tl, ss.ll, si.Zl, si.zl, si.bl, ext_l, exs_l, smu);
    e.dsl = -(o.rsum + o.Gl * dv) / o.Zt;
    d.dtl = o.rd + dv + e.dsl;
    d.dll = -(o.rm + b.ll * d.dtl) / b.tl;
    e.dtl = o.rds + e.dsl;
    e.dll = -(o.rms + ss.ll * e.dtl) / ss.tl;
  }
  if (s.mu != real(0.0)) {
    const SoftOne o = soft_one(s.ub - v, b.lu, b.tu, ss.su, ss.tu, ss.lu, si.Zu, si.zu, si.bu, ext_u, exs_u, smu);
    e.dsu = -(o.rsum - o.Gl * dv) / o.Zt;
    d.dtu = o.rd - dv + e.dsu;
    d.dlu = -(o.rm + b.lu * d.dtu) / b.tu;
    e.dtu = o.rds + e.dsu;
    e.dlu = -(o.rms + ss.lu * e.dtu) / ss.tu;
  }
}
// the slack bounds' pairs in the step ratios and the predictor sums
__device__ __forceinline__ void ratio_soft(const Side& s, const SoftIn& si, const SoftSt& ss, const SoftStep& e,
                                           real& ap, real& ad) {
  if (si.on == real(0.0)) return;
  if (s.ml != real(0.0)) {
    if (e.dtl < real(0.0)) ap = fmin(ap, -ss.tl / e.dtl);
    if (e.dll < real(0.0)) ad = fmin(ad, -ss.ll / e.dll);
  }
  if (s.mu != real(0.0)) {
    if (e.dtu < real(0.0)) ap = fmin(ap, -ss.tu / e.dtu);
    if (e.dlu < real(0.0)) ad = fmin(ad, -ss.lu / e.dlu);
  }
}
__device__ __forceinline__ void aff_soft(const Side& s, const SoftIn& si, const SoftSt& ss, const SoftStep& e,
                                         real& s1, real& s2) {
  if (si.on == real(0.0)) return;
  if (s.ml != real(0.0)) {
    s1 += ss.ll * e.dtl + ss.tl * e.dll;
    s2 += e.dll * e.dtl;
  }
  if (s.mu != real(0.0)) {
    s1 += ss.lu * e.dtu + ss.tu * e.dlu;
    s2 += e.dlu * e.dtu;
  }
}
__device__ __forceinline__ bool huge_soft(const SoftStep& e) {
  return huge(e.dsl) || huge(e.dsu) || huge(e.dtl) || huge(e.dtu) || huge(e.dll) || huge(e.dlu);
}
// RB's box terms of one variable that may be soft: the multipliers in its gradient residual
// rg, and the norms of res_d (md), res_m (mm, musum), the slacks' stationarity r_s (mg) and
// the slack penalty (obj)
__device__ __forceinline__ void rb_soft_terms(const Side& s, const Bar& b, const SoftIn& si, const SoftSt& ss,
                                              real v, real& rg, real& mg, real& md, real& mm, real& musum,
                                              real& obj) {
  const bool on = si.on != real(0.0);
  if (s.ml != real(0.0)) {
    rg -= b.ll;
    const real rd = v + (on ? ss.sl : real(0.0)) - s.lb - b.tl, rm = b.ll * b.tl;
    md = fmax(md, nabs(rd));
    mm = fmax(mm, nabs(rm));
    musum += rm;
    if (on) {
      const real rms = ss.ll * ss.tl;
      md = fmax(md, nabs(ss.sl - si.bl - ss.tl));
      mm = fmax(mm, nabs(rms));
      musum += rms;
      mg = fmax(mg, nabs(si.Zl * ss.sl + si.zl - b.ll - ss.ll));
      obj += ss.sl * (real(0.5) * si.Zl * ss.sl + si.zl);
    }
  }
  if (s.mu != real(0.0)) {
    rg += b.lu;
    const real rd = s.ub - v + (on ? ss.su : real(0.0)) - b.tu, rm = b.lu * b.tu;
    md = fmax(md, nabs(rd));
    mm = fmax(mm, nabs(rm));
    musum += rm;
    if (on) {
      const real rms = ss.lu * ss.tu;
      md = fmax(md, nabs(ss.su - si.bu - ss.tu));
      mm = fmax(mm, nabs(rms));
      musum += rms;
      mg = fmax(mg, nabs(si.Zu * ss.su + si.zu - b.lu - ss.lu));
      obj += ss.su * (real(0.5) * si.Zu * ss.su + si.zu);
    }
  }
}
// Cold start of a soft variable (the init of the same problem with its slacks written as
// inputs boxed below by sb and the bound as a general row): v stays where it is, s = max(0,
// sb + thr0), t_s = s - sb, t = max(w + s, thr0), lam = mu0 / t for both pairs.  Returns
// the number of slack-bound pairs (one per active side).
__device__ __forceinline__ real soft_init(const Side& s, const SoftIn& si, real v, real mu0, Bar& b, SoftSt& ss) {
  ss = SoftSt{real(0.0), real(0.0), real(1.0), real(1.0), real(0.0), real(0.0)};
  if (si.on == real(0.0)) return real(0.0);
  b = Bar{real(0.0), real(0.0), real(1.0), real(1.0)};
  real n = real(0.0);
  if (s.ml != real(0.0)) {
    ss.sl = fmax(real(0.0), si.bl + kThr0);
    ss.tl = ss.sl - si.bl;
    ss.ll = mu0 / ss.tl;
    b.tl = fmax(v - s.lb + ss.sl, kThr0);
    b.ll = mu0 / b.tl;
    n += real(1.0);
  }
  if (s.mu != real(0.0)) {
    ss.su = fmax(real(0.0), si.bu + kThr0);
    ss.tu = ss.su - si.bu;
    ss.lu = mu0 / ss.tu;
    b.tu = fmax(s.ub - v + ss.su, kThr0);
    b.lu = mu0 / b.tu;
    n += real(1.0);
  }
  return n;
}
