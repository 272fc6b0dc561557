// ipm_barrier.h -- the barrier algebra of one inequality pair, shared by the batched IPM
// (ipm_box_impl.h, both precisions) and the one-launch latency IPM (ipm_latency.hip), whose
// results the suite compares bit for bit.  Functions of values only: how a kernel loads and
// stores its sides, bars and steps (layout, masking) stays with that kernel.
#pragma once
#include "qp_group.h"

namespace srbd {
namespace barrier {

// scalar arguments take their type from the structs (a literal converts)
template <typename T>
struct same {
  using type = T;
};
template <typename T>
using same_t = typename same<T>::type;

template <typename T>
constexpr T kThr0 = T(0.1);  // minimum initial slack (HPIPM init_var)
template <typename T>
constexpr T kStepTau = T(0.995);  // fraction to the boundary

// One inequality side pair on one variable / row.
template <typename T>
struct Side {
  T lb, ub;  // bounds
  T ml, mu;  // 1 if the lower / upper bound is active, else 0
};
// barrier state of one variable: lam_l, lam_u, t_l, t_u
template <typename T>
struct Bar {
  T ll, lu, tl, tu;
};
// step of one variable's barrier pair: dt_l, dt_u, dlam_l, dlam_u
template <typename T>
struct BarStep {
  T dtl, dtu, dll, dlu;
};

// 16-lane group reductions (every lane gets the result)
template <typename T>
__device__ __forceinline__ T gsum(T v) {
  v += __shfl_xor(v, 8, kGroup);
  v += __shfl_xor(v, 4, kGroup);
  v += __shfl_xor(v, 2, kGroup);
  v += __shfl_xor(v, 1, kGroup);
  return v;
}
template <typename T>
__device__ __forceinline__ T gmax(T v) {
  v = fmax(v, __shfl_xor(v, 8, kGroup));
  v = fmax(v, __shfl_xor(v, 4, kGroup));
  v = fmax(v, __shfl_xor(v, 2, kGroup));
  v = fmax(v, __shfl_xor(v, 1, kGroup));
  return v;
}
template <typename T>
__device__ __forceinline__ T gmin(T v) {
  v = fmin(v, __shfl_xor(v, 8, kGroup));
  v = fmin(v, __shfl_xor(v, 4, kGroup));
  v = fmin(v, __shfl_xor(v, 2, kGroup));
  v = fmin(v, __shfl_xor(v, 1, kGroup));
  return v;
}
// NaN, or too large to square in this precision (sqrt(max) / 1e4: 1.8e15 in fp32)
template <typename T>
__device__ __forceinline__ bool huge(T v) {
  constexpr T kHuge = sizeof(T) == 4 ? T(1.8e15) : T(1.3e150);
  return !(__builtin_fabs(v) < kHuge);
}
// v + a d, with a = 0 (no step taken) leaving v as it is whatever d holds
template <typename T>
__device__ __forceinline__ T step(T v, T a, T d) {
  return a != T(0.0) ? fmadd(a, d, v) : v;
}
// |v| propagating NaN (max with NaN would drop it)
template <typename T>
__device__ __forceinline__ T nabs(T v) {
  return v == v ? fabs(v) : T(__builtin_inf());
}

// HPIPM init_var for one box-bounded variable: v projected into the box by thr0, t from the
// projected v, lam = mu0 / t (inactive sides: lam 0, t 1)
template <typename T>
__device__ __forceinline__ Bar<T> init_box(const Side<T>& s, T& v, same_t<T> mu0) {
  Bar<T> bb{T(0.0), T(0.0), T(1.0), T(1.0)};
  if (s.ml == T(0.0) && s.mu == T(0.0)) return bb;
  T tl = v - s.lb, tu = s.ub - v;
  if (s.ml != T(0.0) && s.mu != T(0.0)) {
    if (tl < kThr0<T>) {
      if (tu < kThr0<T>) {
        v = T(0.5) * (s.lb + s.ub);
        tl = tu = kThr0<T>;
      } else {
        tl = kThr0<T>;
        v = s.lb + kThr0<T>;
        tu = s.ub - v;
      }
    } else if (tu < kThr0<T>) {
      tu = kThr0<T>;
      v = s.ub - kThr0<T>;
      tl = v - s.lb;
    }
  } else if (s.ml != T(0.0)) {
    if (tl < kThr0<T>) {
      tl = kThr0<T>;
      v = s.lb + kThr0<T>;
    }
  } else if (tu < kThr0<T>) {
    tu = kThr0<T>;
    v = s.ub - kThr0<T>;
  }
  bb.tl = s.ml != T(0.0) ? tl : T(1.0);
  bb.tu = s.mu != T(0.0) ? tu : T(1.0);
  bb.ll = s.ml != T(0.0) ? mu0 / tl : T(0.0);
  bb.lu = s.mu != T(0.0) ? mu0 / tu : T(0.0);
  return bb;
}

// Gamma (Hessian add) and gamma (gradient add) of one variable:
// Gamma = lam_l/t_l + lam_u/t_u,
// gamma = (rm_l + lam_l rd_l)/t_l - (rm_u + lam_u rd_u)/t_u, with
// rm = lam t + extra - sigma_mu (extra = dlam_aff dt_aff in the corrector).
template <typename T>
__device__ __forceinline__ void gamma_of(const Side<T>& s, const Bar<T>& b, same_t<T> v, same_t<T> ext_l,
                                         same_t<T> ext_u, same_t<T> smu, T& G, T& g) {
  G = T(0.0);
  g = T(0.0);
  if (s.ml != T(0.0)) {
    const T rd = v - s.lb - b.tl;
    const T rm = b.ll * b.tl + ext_l - smu;
    G += b.ll / b.tl;
    g += (rm + b.ll * rd) / b.tl;
  }
  if (s.mu != T(0.0)) {
    const T rd = s.ub - v - b.tu;
    const T rm = b.lu * b.tu + ext_u - smu;
    G += b.lu / b.tu;
    g -= (rm + b.lu * rd) / b.tu;
  }
}

// dt / dlam of one variable given its primal step dv.
template <typename T>
__device__ __forceinline__ BarStep<T> bar_step(const Side<T>& s, const Bar<T>& b, same_t<T> v, same_t<T> dv,
                                               same_t<T> ext_l, same_t<T> ext_u, same_t<T> smu) {
  BarStep<T> d{T(0.0), T(0.0), T(0.0), T(0.0)};
  if (s.ml != T(0.0)) {
    const T rd = v - s.lb - b.tl;
    d.dtl = rd + dv;
    d.dll = -(b.ll * b.tl + ext_l - smu + b.ll * d.dtl) / b.tl;
  }
  if (s.mu != T(0.0)) {
    const T rd = s.ub - v - b.tu;
    d.dtu = rd - dv;
    d.dlu = -(b.lu * b.tu + ext_u - smu + b.lu * d.dtu) / b.tu;
  }
  return d;
}

// step ratios to the boundary: ap over the t's, ad over the lam's (active sides)
template <typename T>
__device__ __forceinline__ void ratio(const Side<T>& s, const Bar<T>& b, const BarStep<T>& d, T& ap, T& ad) {
  if (s.ml != T(0.0)) {
    if (d.dtl < T(0.0)) ap = fmin(ap, -b.tl / d.dtl);
    if (d.dll < T(0.0)) ad = fmin(ad, -b.ll / d.dll);
  }
  if (s.mu != T(0.0)) {
    if (d.dtu < T(0.0)) ap = fmin(ap, -b.tu / d.dtu);
    if (d.dlu < T(0.0)) ad = fmin(ad, -b.lu / d.dlu);
  }
}

// predictor sums for mu_aff: s1 += lam dt + t dlam, s2 += dlam dt (active sides)
template <typename T>
__device__ __forceinline__ void aff_sums(const Side<T>& s, const Bar<T>& b, const BarStep<T>& d, T& s1, T& s2) {
  if (s.ml != T(0.0)) {
    s1 += b.ll * d.dtl + b.tl * d.dll;
    s2 += d.dll * d.dtl;
  }
  if (s.mu != T(0.0)) {
    s1 += b.lu * d.dtu + b.tu * d.dlu;
    s2 += d.dlu * d.dtu;
  }
}

}  // namespace barrier
}  // namespace srbd
