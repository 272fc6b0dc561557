// srbd_gait.hip -- the producer of a tick's plan window (srbd_qp_srbd_gait_plan_f64,
// DESIGN.md 4.7e): from a per-robot velocity command, a per-robot gait and the measured state,
// the reference trajectory, the contact schedule and the footsteps over the horizon, with
// Raibert foothold feedback.  The definition is include/srbd_qp.h's; the host restatement that
// pins it is srbd_model.py (gait_plan).
//
// One wave per robot, like srbd_advance_kernel.  Two phases:
//   1. Lanes run over stages k = 0..N in chunks of 64.  Lane k forms yaw_k, (cos, sin)(yaw_k)
//      and its displacement dt Rz(yaw_k)(vx, vy); an inclusive scan over the lanes (shuffles;
//      the chunk's total is carried into the next chunk) gives p_{k+1} - p_0.  (p_k, cos, sin)
//      go to LDS: a foot row needs the pose of another stage, the touchdown's.
//   2. The wave stores the four output rows as consecutive doubles, adjacent lanes on adjacent
//      addresses, 16 bytes per lane where the row allows (x_ref: 12 doubles per stage;
//      fz_max: 2; the feet: 3 per stage, so only a robot row of an even N starts aligned).
//      Each lane forms the values of its own elements from closed-form integers (the stage,
//      its phase, the touchdown stage) and the staged poses: no lane walks the schedule.
#include "../../include/srbd_qp.h"
#include "kernels.h"

namespace srbd {
namespace {

constexpr int kWave = 64;
constexpr int kGaitWaves = 4;      // robots per block ...
constexpr int kGaitLdsStage = 4;   // ... each with (px, py, cos, sin) per stage in LDS
constexpr size_t kGaitLdsMax = 64 * 1024;

struct GaitArgs {
  int batch, N;
  srbd_gait_f64 g;
  GaitIo io;
  double dt, Lz;
  const double* Lbody;  // the MODEL role's [batch][3] (NULL: Lz)
  int feet16;           // the foot rows go out as double2
};

// what a foot's rows need of the robot, the same for every stage
struct FootConst {
  unsigned period, swing, phi0;  // phi0 = (tick + offset) mod period
  double hx, hy;                 // hip + (S dt / 2)(vx, vy)
  double nx, ny, nz;             // foot_now
};

__device__ __forceinline__ double yaw_at(double yaw, int k, double dwz) { return fma((double)k, dwz, yaw); }

// Element `comp` of foot row k: foot_now while the foot has not left the ground it stands on,
// else the foothold of the stage's (next or current) touchdown.  (fbx, fby) is the feedback
// term k_raibert (vm - Rz(yaw_0)(vx, vy)).
__device__ __forceinline__ double foot_elem(const FootConst& f, const double* lds, int N, int k, int comp,
                                            double cx, double cy, double p0x, double p0y, double fbx,
                                            double fby, double ground_z) {
  const unsigned phi = (f.phi0 + (unsigned)k) % f.period;
  long long j;  // the touchdown's window stage
  if (phi < f.swing) {
    j = (long long)k + (long long)(f.swing - phi);
  } else {
    j = (long long)k - (long long)(phi - f.swing);
    if (f.swing == 0 || j <= 0) {
      const double n0 = f.nx, n1 = f.ny, n2 = f.nz;  // values, so that the struct stays in registers
      return comp == 0 ? n0 : comp == 1 ? n1 : n2;
    }
  }
  if (comp == 2) return ground_z;
  const int jc = j < N ? (int)j : N;
  const double* st = lds + (size_t)jc * kGaitLdsStage;
  const double c = st[2], s = st[3];
  if (comp == 0) return cx + (st[0] - p0x) + (c * f.hx - s * f.hy) + fbx;
  return cy + (st[1] - p0y) + (s * f.hx + c * f.hy) + fby;
}

__global__ void __launch_bounds__(kWave* kGaitWaves) srbd_gait_kernel(GaitArgs a) {
  extern __shared__ double gait_lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const long long qp = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  const bool live = qp < a.batch;  // wave-uniform
  const int N = a.N;
  double* lds = gait_lds + (size_t)wave * (N + 1) * kGaitLdsStage;
  double vx = 0.0, vy = 0.0, wz = 0.0, zh = 0.0, yaw0 = 0.0, p0x = 0.0, p0y = 0.0, cx = 0.0, cy = 0.0;
  double vmx = 0.0, vmy = 0.0;
  FootConst ftr{}, ftl{};  // right, left
  if (live) {
    // ---- the robot's inputs: every lane reads them (one address per wave) before any store ----
    const double* cmd = a.io.cmd + (size_t)qp * a.io.cmd_stride;
    vx = cmd[0];
    vy = cmd[1];
    wz = cmd[2];
    zh = cmd[3];
    const double* x = a.io.x + (size_t)qp * 12;
    cx = x[6];
    cy = x[7];
    vmx = x[9];
    vmy = x[10];
    const double* rp = a.io.ref_pose + (size_t)qp * 3;
    yaw0 = rp[2];
    p0x = a.g.anchor ? cx : rp[0];
    p0y = a.g.anchor ? cy : rp[1];
    const long long period = a.g.period_r ? a.g.period_r[qp] : a.g.period;
    auto foot_const = [&](int f, FootConst& fc) __attribute__((always_inline)) {
      const long long sw = a.g.swing_r ? a.g.swing_r[(size_t)qp * 2 + f] : a.g.swing[f];
      const long long off = a.g.offset_r ? a.g.offset_r[(size_t)qp * 2 + f] : a.g.offset[f];
      fc.period = (unsigned)period;
      fc.swing = (unsigned)sw;
      fc.phi0 = (unsigned)((a.io.tick + off) % period);
      const double half = (double)(period - sw) * a.dt / 2.0;
      fc.hx = a.g.hip[f][0] + half * vx;
      fc.hy = a.g.hip[f][1] + half * vy;
      const double* now = a.io.foot_now + (size_t)qp * 6 + f * 3;
      fc.nx = now[0];
      fc.ny = now[1];
      fc.nz = now[2];
    };
    foot_const(0, ftr);
    foot_const(1, ftl);
    // ---- phase 1: the poses of stages 0..N ----
    const double dwz = a.dt * wz;
    double carry_x = 0.0, carry_y = 0.0;  // p_c - p_0 at the chunk's first stage
    for (int c0 = 0; c0 <= N; c0 += kWave) {
      const int k = c0 + lane;
      double sn, cs;
      sincos(yaw_at(yaw0, k, dwz), &sn, &cs);
      double dx = a.dt * (cs * vx - sn * vy), dy = a.dt * (sn * vx + cs * vy);
#pragma unroll
      for (int d = 1; d < kWave; d <<= 1) {
        const double ux = __shfl_up(dx, d, kWave), uy = __shfl_up(dy, d, kWave);
        if (lane >= d) {
          dx += ux;
          dy += uy;
        }
      }
      dx += carry_x;  // p_{k+1} - p_0
      dy += carry_y;
      if (k <= N) {
        lds[(size_t)k * kGaitLdsStage + 2] = cs;
        lds[(size_t)k * kGaitLdsStage + 3] = sn;
        if (k == 0) {
          lds[0] = p0x;
          lds[1] = p0y;
        }
        if (k < N) {
          lds[(size_t)(k + 1) * kGaitLdsStage + 0] = p0x + dx;
          lds[(size_t)(k + 1) * kGaitLdsStage + 1] = p0y + dy;
        }
      }
      carry_x = __shfl(dx, kWave - 1, kWave);
      carry_y = __shfl(dy, kWave - 1, kWave);
    }
  }
  __syncthreads();  // the staged poses are read by other lanes (no wave has left the kernel)
  if (!live) return;
  // ---- phase 2: the rows ----
  const double dwz = a.dt * wz;
  const double Lz = a.Lbody ? a.Lbody[(size_t)qp * 3 + 2] : a.Lz;
  const double lzw = Lz * wz;
  // the feedback term: k_raibert (vm - Rz(yaw_0)(vx, vy))
  const double fbx = a.g.k_raibert * (vmx - (lds[2] * vx - lds[3] * vy));
  const double fby = a.g.k_raibert * (vmy - (lds[3] * vx + lds[2] * vy));
  auto xref_elem = [&](int k, int e) __attribute__((always_inline)) -> double {
    const double* st = lds + (size_t)k * kGaitLdsStage;
    switch (e) {
      case 2: return yaw_at(yaw0, k, dwz);
      case 5: return lzw;
      case 6: return st[0];
      case 7: return st[1];
      case 8: return zh;
      case 9: return st[2] * vx - st[3] * vy;
      case 10: return st[3] * vx + st[2] * vy;
      default: return 0.0;
    }
  };
  auto foot = [&](const FootConst& fc, int k, int comp) __attribute__((always_inline)) -> double {
    return foot_elem(fc, lds, N, k, comp, cx, cy, p0x, p0y, fbx, fby, a.g.ground_z);
  };
  {  // x_ref: 6 (N + 1) double2
    double2* out = reinterpret_cast<double2*>(a.io.x_ref + (size_t)qp * (N + 1) * 12);
    const int n2 = 6 * (N + 1);
    for (int i = lane; i < n2; i += kWave) {
      const int k = i / 6, e = 2 * (i - 6 * k);
      out[i] = make_double2(xref_elem(k, e), xref_elem(k, e + 1));
    }
  }
  {  // fz_max: N double2 (right, left)
    double2* out = reinterpret_cast<double2*>(a.io.fz_max + (size_t)qp * N * 2);
    for (int k = lane; k < N; k += kWave) {
      const bool sr = (ftr.phi0 + (unsigned)k) % ftr.period < ftr.swing;
      const bool sl = (ftl.phi0 + (unsigned)k) % ftl.period < ftl.swing;
      out[k] = make_double2(sr ? a.g.fz_swing : a.g.fz_stance, sl ? a.g.fz_swing : a.g.fz_stance);
    }
  }
  // one foot: 3 N doubles (inlined: the foot's constants stay in registers)
  auto foot_rows = [&](const FootConst& fc, double* out) __attribute__((always_inline)) {
    const int n = 3 * N;
    if (a.feet16) {
      double2* out2 = reinterpret_cast<double2*>(out);
      for (int i = lane; i < n / 2; i += kWave) {
        const int e0 = 2 * i, e1 = e0 + 1;
        out2[i] = make_double2(foot(fc, e0 / 3, e0 % 3), foot(fc, e1 / 3, e1 % 3));
      }
    } else {
      for (int e = lane; e < n; e += kWave) out[e] = foot(fc, e / 3, e % 3);
    }
  };
  foot_rows(ftr, a.io.foot_r + (size_t)qp * N * 3);
  foot_rows(ftl, a.io.foot_l + (size_t)qp * N * 3);
  // ---- the carried state and the logs: row 0 of the feet and fz_max, (p_1, yaw_1) ----
  // (every lane has read ref_pose and foot_now above; a wave's accesses take effect in order)
  if (lane < 6) {
    const int f = lane / 3, comp = lane - 3 * f;
    const double vr = foot(ftr, 0, comp), vl = foot(ftl, 0, comp);
    const double v = f == 0 ? vr : vl;
    a.io.foot_now[(size_t)qp * 6 + lane] = v;
    if (a.io.foot_log) a.io.foot_log[(size_t)qp * a.io.foot_log_stride + lane] = v;
  } else if (lane < 8) {
    const int f = lane - 6;
    if (a.io.fz_log)
      a.io.fz_log[(size_t)qp * a.io.fz_log_stride + f] =
          (f == 0 ? ftr.phi0 < ftr.swing : ftl.phi0 < ftl.swing) ? a.g.fz_swing : a.g.fz_stance;
  } else if (lane < 11) {
    const int i = lane - 8;
    a.io.ref_pose[(size_t)qp * 3 + i] = i == 2 ? yaw_at(yaw0, 1, dwz) : lds[kGaitLdsStage + i];
  }
}

}  // namespace

hipError_t launch_srbd_gait(const srbd_model_params& p, int batch, int N, const srbd_gait_f64& gait,
                            const GaitIo& io, hipStream_t stream, const srbd_robots_f64* robots) {
  if (batch <= 0) return hipSuccess;
  GaitArgs a{};
  a.batch = batch;
  a.N = N;
  a.g = gait;
  a.io = io;
  a.dt = p.dt;
  a.Lz = p.Lbody[2];
  a.Lbody = robots ? robots->Lbody : nullptr;
  auto aligned16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  a.feet16 = N % 2 == 0 && aligned16(io.foot_r) && aligned16(io.foot_l);
  // four robots per block while their staged poses fit, else one
  const size_t per_wave = (size_t)(N + 1) * kGaitLdsStage * sizeof(double);
  const int waves = per_wave * kGaitWaves <= kGaitLdsMax ? kGaitWaves : 1;
  if (per_wave * waves > kGaitLdsMax) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((batch + waves - 1) / waves)), block(kWave * waves);
  hipLaunchKernelGGL(srbd_gait_kernel, grid, block, per_wave * waves, stream, a);
  return hipGetLastError();
}

}  // namespace srbd
