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
// With a terrain on the handle (srbd_qp_srbd_set_terrain_f64) the kernel's other
// instantiation runs a phase between the two: the wave enumerates each foot's distinct
// touchdowns of the window (closed form: j_1 + m period), groups of lanes evaluate one touchdown
// each with one foothold candidate per lane, a segmented argmin over the key (J, q) picks the
// foothold, and one lane writes (x, y, z) into a table in LDS that phase 2 reads.
#include "../../include/srbd_qp.h"
#include "kernels.h"
#include "srbd_terrain.h"

namespace srbd {
namespace {

constexpr int kWave = 64;
constexpr int kGaitWaves = 4;      // robots per block ...
constexpr int kGaitLdsStage = 4;   // ... each with (px, py, cos, sin) per stage in LDS
constexpr size_t kGaitLdsMax = 64 * 1024;

// entries of one foot's foothold table: the touchdowns j_1 + m period < N + swing, period >= 2
__host__ __device__ constexpr int gait_table_rows(int N) { return N / 2 + 1; }

struct GaitArgs {
  int batch, N;
  srbd_gait_f64 g;
  srbd_terrain_f64 t;   // read by the terrain instantiation only
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
  const double* tab;             // terrain: the foot's foothold table in LDS, (x, y, z) per touchdown
};

// the first touchdown after stage 0: the smallest j >= 1 with (phi0 + j) mod period == swing
__device__ __forceinline__ unsigned first_touchdown(const FootConst& f) {
  const unsigned r = (f.swing + f.period - f.phi0) % f.period;
  return r ? r : f.period;
}

__device__ __forceinline__ double yaw_at(double yaw, int k, double dwz) { return fma((double)k, dwz, yaw); }

// Element `comp` of foot row k: foot_now while the foot has not left the ground it stands on,
// else the foothold of the stage's (next or current) touchdown.  (fbx, fby) is the feedback
// term k_raibert (vm - Rz(yaw_0)(vx, vy)).
template <bool TERRAIN>
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
  if constexpr (TERRAIN) {  // the table's row of this touchdown
    const unsigned m = (unsigned)((unsigned long long)(j - (long long)first_touchdown(f)) / f.period);
    return f.tab[(size_t)m * 3 + comp];
  }
  if (comp == 2) return ground_z;
  const int jc = j < N ? (int)j : N;
  const double* st = lds + (size_t)jc * kGaitLdsStage;
  const double c = st[2], s = st[3];
  if (comp == 0) return cx + (st[0] - p0x) + (c * f.hx - s * f.hy) + fbx;
  return cy + (st[1] - p0y) + (s * f.hx + c * f.hy) + fby;
}

// The nominal foothold of the touchdown whose clamped stage is jc (foot_elem's expression).
__device__ __forceinline__ void nominal_foothold(const FootConst& f, const double* lds, int jc, double cx, double cy,
                                                 double p0x, double p0y, double fbx, double fby, double& x,
                                                 double& y) {
  const double* st = lds + (size_t)jc * kGaitLdsStage;
  const double c = st[2], s = st[3];
  x = cx + (st[0] - p0x) + (c * f.hx - s * f.hy) + fbx;
  y = cy + (st[1] - p0y) + (s * f.hx + c * f.hy) + fby;
}

// One foot's foothold table.  Groups of `width` lanes (the power of two that holds the
// (2 search + 1)^2 candidates) take one touchdown each, lane q of the group its candidate q;
// a butterfly inside the group leaves the smallest key (J, q) in all of its lanes, and the
// lane that holds the winner writes its foothold.  The wave runs this uniformly: every lane
// takes part in every shuffle.
__device__ __forceinline__ void select_footholds(const FootConst& f, const srbd_terrain_f64& t, const double* H,
                                                 const double* lds, double* tab, int N, int lane, double cx,
                                                 double cy, double p0x, double p0y, double fbx, double fby,
                                                 double ground_z) {
  if (f.swing == 0) return;  // the foot never lands
  const int side = 2 * t.search + 1, cand = side * side;
  const int width = t.search == 0 ? 1 : t.search == 1 ? 16 : t.search == 2 ? 32 : 64;
  const int group = lane / width, q = lane - group * width;
  const long long j1 = first_touchdown(f), end = (long long)N + f.swing;  // touchdowns j1 + m period < end
  // at most gait_table_rows(N) for swing < period (the gait's contract); the min keeps a gait
  // that breaks it inside the table
  const int count = j1 < end ? (int)min((end - 1 - j1) / f.period + 1, (long long)gait_table_rows(N)) : 0;
  const int dj = q / side - t.search, di = q - (q / side) * side - t.search;
  for (int m0 = 0; m0 < count; m0 += kWave / width) {
    const int m = m0 + group;
    const bool valid = m < count && q < cand;
    double J = __builtin_inf(), x = 0.0, y = 0.0;
    if (valid) {
      const long long j = j1 + (long long)m * f.period;
      nominal_foothold(f, lds, j < N ? (int)j : N, cx, cy, p0x, p0y, fbx, fby, x, y);
      J = 0.0;
      if (t.search > 0) {
        x += t.cell * (double)di;
        y += t.cell * (double)dj;
        const double h0 = terrain_bilinear(H, t.nx, t.ny, t.x0, t.y0, t.cell, x, y);
        double rho = fabs(terrain_bilinear(H, t.nx, t.ny, t.x0, t.y0, t.cell, x + t.cell, y) - h0);
        rho = fmax(rho, fabs(terrain_bilinear(H, t.nx, t.ny, t.x0, t.y0, t.cell, x - t.cell, y) - h0));
        rho = fmax(rho, fabs(terrain_bilinear(H, t.nx, t.ny, t.x0, t.y0, t.cell, x, y + t.cell) - h0));
        rho = fmax(rho, fabs(terrain_bilinear(H, t.nx, t.ny, t.x0, t.y0, t.cell, x, y - t.cell) - h0));
        J = t.cell * t.cell * (double)(di * di + dj * dj) + t.w_rough * (rho * rho);
      }
    }
    double Jb = J;
    int qb = q;
    for (int d = width >> 1; d > 0; d >>= 1) {
      const double Jo = __shfl_xor(Jb, d, kWave);
      const int qo = __shfl_xor(qb, d, kWave);
      if (Jo < Jb || (Jo == Jb && qo < qb)) {
        Jb = Jo;
        qb = qo;
      }
    }
    if (valid && qb == q) {
      double* row = tab + (size_t)m * 3;
      row[0] = x;
      row[1] = y;
      row[2] = ground_z + terrain_bilinear(H, t.nx, t.ny, t.x0, t.y0, t.cell, x, y);
    }
  }
}

template <bool TERRAIN>
__global__ void __launch_bounds__(kWave* kGaitWaves) srbd_gait_kernel(GaitArgs a) {
  extern __shared__ double gait_lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const long long qp = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  const bool live = qp < a.batch;  // wave-uniform
  const int N = a.N;
  // a robot's LDS: the staged poses, then (terrain) the two feet's foothold tables
  const size_t per_wave = (size_t)(N + 1) * kGaitLdsStage + (TERRAIN ? (size_t)2 * gait_table_rows(N) * 3 : 0);
  double* lds = gait_lds + (size_t)wave * per_wave;
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
  const double* H = nullptr;  // the robot's map
  if constexpr (TERRAIN) {
    // ---- the footholds of the window's touchdowns, one candidate per lane ----
    if (live) {
      H = a.t.height + (size_t)(a.t.map_r ? a.t.map_r[qp] : 0) * a.t.ny * a.t.nx;
      double* tab = lds + (size_t)(N + 1) * kGaitLdsStage;
      ftr.tab = tab;
      ftl.tab = tab + (size_t)gait_table_rows(N) * 3;
      const double fx = a.g.k_raibert * (vmx - (lds[2] * vx - lds[3] * vy));
      const double fy = a.g.k_raibert * (vmy - (lds[3] * vx + lds[2] * vy));
      select_footholds(ftr, a.t, H, lds, tab, N, lane, cx, cy, p0x, p0y, fx, fy, a.g.ground_z);
      select_footholds(ftl, a.t, H, lds, tab + (size_t)gait_table_rows(N) * 3, N, lane, cx, cy, p0x, p0y, fx, fy,
                       a.g.ground_z);
    }
    __syncthreads();  // the tables are read by other lanes
  }
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
      case 8:
        if constexpr (TERRAIN) return zh + terrain_bilinear(H, a.t.nx, a.t.ny, a.t.x0, a.t.y0, a.t.cell, st[0], st[1]);
        return zh;
      case 9: return st[2] * vx - st[3] * vy;
      case 10: return st[3] * vx + st[2] * vy;
      default: return 0.0;
    }
  };
  auto foot = [&](const FootConst& fc, int k, int comp) __attribute__((always_inline)) -> double {
    return foot_elem<TERRAIN>(fc, lds, N, k, comp, cx, cy, p0x, p0y, fbx, fby, a.g.ground_z);
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

// srbd_qp_srbd_terrain_height_f64: one point per thread
__global__ void srbd_terrain_height_kernel(srbd_terrain_f64 t, int n, const double* xy, const int* map, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* H = t.height + (size_t)(map ? map[i] : 0) * t.ny * t.nx;
  out[i] = terrain_bilinear(H, t.nx, t.ny, t.x0, t.y0, t.cell, xy[2 * (size_t)i], xy[2 * (size_t)i + 1]);
}

}  // namespace

hipError_t launch_srbd_terrain_height(const srbd_terrain_f64& terrain, int n, const double* xy, const int* map,
                                      double* out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(srbd_terrain_height_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, terrain,
                     n, xy, map, out);
  return hipGetLastError();
}

hipError_t launch_srbd_gait(const srbd_model_params& p, int batch, int N, const srbd_gait_f64& gait,
                            const GaitIo& io, hipStream_t stream, const srbd_robots_f64* robots,
                            const srbd_terrain_f64* terrain) {
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
  const bool with_terrain = terrain && terrain->height;
  if (with_terrain) a.t = *terrain;
  // four robots per block while their staged poses (and, with a terrain, their foothold
  // tables: 56 N + 80 bytes a robot, four up to N = 291, one up to N = 1024) fit, else one
  const size_t per_wave =
      ((size_t)(N + 1) * kGaitLdsStage + (with_terrain ? (size_t)2 * gait_table_rows(N) * 3 : 0)) * sizeof(double);
  const int waves = per_wave * kGaitWaves <= kGaitLdsMax ? kGaitWaves : 1;
  if (per_wave * waves > kGaitLdsMax) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((batch + waves - 1) / waves)), block(kWave * waves);
  if (with_terrain)
    hipLaunchKernelGGL(srbd_gait_kernel<true>, grid, block, per_wave * waves, stream, a);
  else
    hipLaunchKernelGGL(srbd_gait_kernel<false>, grid, block, per_wave * waves, stream, a);
  return hipGetLastError();
}

}  // namespace srbd
