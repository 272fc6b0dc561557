/*
 * srbd_qp.h -- C-ABI of the MI355X-native batched OCP-QP solver (libsrbd_qp.so).
 *
 * This is the drop-in boundary for the reference's hot path: everything
 * hpipm::OcpQpIpmSolver::solve() does below the Eigen marshalling
 * (hpipm-cpp/src/ocp_qp_ipm_solver.cpp:181-414) -- d_ocp_qp_set_all (:283),
 * d_ocp_qp_ipm_solve (:334, decl hpipm_d_ocp_qp_ipm.h:238), the solution and
 * Riccati getters (:337-346) and the stage-0 rebuild (:347-373) -- batched
 * over thousands of independent QPs and run by hand-written HIP kernels for
 * gfx950.  Plain C types only; no exceptions cross this boundary.
 *
 * Entry point -> reference interface it replaces:
 *   srbd_qp_create       OcpQpIpmSolver(qp, settings) ctor + resize()
 *                        (ocp_qp_ipm_solver.cpp:60-68, :120-178): dims check,
 *                        workspace sizing (d_ocp_qp_ipm_ws_create).
 *   srbd_qp_solve_f64    OcpQpIpmSolver::solve (ocp_qp_ipm_solver.cpp:181-414)
 *                        on a batch of device-resident QPs, asynchronous.
 *   srbd_qp_solve_host_f64  the same from host buffers, synchronous (what the
 *                        hpipm-cpp shim calls for one QP or a small batch).
 *   srbd_qp_solve_f32 / _host_f32  the fp32 twins (HPIPM's s_ocp_qp_ipm_solve,
 *                        hpipm_s_ocp_qp_ipm.h:238).
 *   srbd_qp_solve_backward_f64  nothing in the reference: the gradients of the QP data through
 *                        the solve (one more Riccati solve and outer products).
 *   srbd_qp_destroy      ~OcpQpIpmSolver (d_ocp_qp_*_wrapper frees).
 *   srbd_qp_status_string  hpipm::to_string(HpipmStatus) (:19-33).
 * The steps either side of the solve in the reference's SQP iteration, batched:
 *   srbd_qp_srbd_linearize_f64   NMPCSolver::prepareQpStructures (NMPC_solver.cpp:276-314)
 *   srbd_qp_srbd_linesearch_f64  NMPCSolver::linearSearch (NMPC_solver.cpp:149-274)
 *   srbd_qp_srbd_nmpc_f64        the SQP loop of NMPCSolver::controlLoop
 *                                (NMPC_solver.cpp:362-372) around all three.
 *   srbd_qp_srbd_*_plan_f64      the same three with a srbd_plan_f64: a reference trajectory
 *                                (NMPCSolver::x_ref_), a footstep plan and a contact schedule
 *                                per robot and stage.
 *   srbd_qp_srbd_advance_f64     what a controller does between two steps: apply u[0], move the
 *                                plant, shift the previous solution by one stage.
 *   srbd_qp_srbd_rollout_f64     T ticks of the closed receding-horizon loop around the step.
 *   srbd_qp_srbd_set_robots_f64  per-robot mass, inertia, friction and weights for all of the
 *                                above: what the controller believes, and the true robot.
 *   srbd_qp_srbd_linearize_backward_f64  nothing in the reference: the gradients of the robots'
 *                                and the plan's values from the cotangents of the QP arrays.
 *   srbd_qp_srbd_solve_backward_f64  the same gradients straight from the solve and its adjoint:
 *                                the two backward passes in one, no QP gradient in between.
 *   srbd_qp_srbd_plant_rollout_f64  the true robot alone: T ticks of the plant step from given
 *                                inputs; srbd_qp_srbd_plant_rollout_backward_f64 is its adjoint.
 *   srbd_qp_srbd_gait_plan_f64   the producer of a tick's plan: a velocity command, a gait and
 *                                the measured state in, the window out (Raibert footholds).
 *   srbd_qp_srbd_rollout_gait_f64  the rollout that replans every tick.
 *   srbd_qp_srbd_set_terrain_f64 height maps under the gait planner: foothold height, reference
 *                                body height and foothold selection; srbd_qp_srbd_terrain_height_f64
 *                                samples them.
 *   srbd_qp_srbd_set_contact_f64 the plant's contact model and fall detection.
 *   srbd_qp_srbd_set_active_f64  which robots a step steps (a mask, not the fallen ones), and its
 *                                SQP iterations over the robots that still iterate only;
 *                                srbd_qp_srbd_step_work counts the QPs that were solved.
 *
 * ------------------------------------------------------------------------
 * Problem (per QP, stages k = 0..N), identical to hpipm::OcpQp
 * (hpipm-cpp/include/hpipm-cpp/ocp_qp.hpp:15-177):
 *   min  sum_k 1/2 x'Q x + u'S x + 1/2 u'R u + q'x + r'u
 *   s.t. x[k+1] = A x[k] + B u[k] + b,  x[0] = x0,
 *        lbu <= u <= ubu, lbx <= x <= ubx (k >= 1), lg <= C x + D u <= ug.
 * Box bounds may be soft (HPIPM's Zl / Zu / zl / zu / idxs / lls / lus):
 * srbd_qp_solve_soft_f64 below; general rows are hard.
 * x0 is embedded like hpipm-cpp does it (nx[0] = nbx[0] = 0,
 * ocp_qp_ipm_solver.cpp:128-130): box-x bounds and C at stage 0 are ignored.
 *
 * Memory layout (every pointer may be host or device memory as the entry
 * point says; 16-byte aligned base pointers are required for the fast path):
 *   batch-major, then stage-major, then one dense block per stage.  Matrix
 *   blocks are column-major (Eigen's default, what d_ocp_qp_set_all reads):
 *     A [batch][N  ][nx*nx]   B [batch][N][nx*nu]   b [batch][N][nx]
 *     Q [batch][N+1][nx*nx]   S [batch][N][nu*nx]   R [batch][N][nu*nu]
 *     q [batch][N+1][nx]      r [batch][N][nu]      x0 [batch][nx]
 *   Box constraints are dense per variable: one bound per variable plus an
 *   optional 0/1 mask per bound (a NULL mask means "all bounds active"; a
 *   masked bound is absent, exactly like hpipm's d_ocp_qp_set_l*_mask).  The
 *   reference's index form (idxbu/idxbx) maps onto this by setting mask 0 for
 *   variables not in the index list (the hpipm-cpp shim does this).
 *     lbu, ubu, lbu_mask, ubu_mask [batch][N][nu]        (NULL lbu: no box)
 *     lbx, ubx, lbx_mask, ubx_mask [batch][N+1][nx]      (NULL lbx: no box)
 *   General constraints (ng rows per stage, pad with masked rows):
 *     C [batch][N+1][ng*nx]  D [batch][N][ng*nu]  lg, ug, lg_mask, ug_mask [batch][N+1][ng]
 *   C = NULL means C = 0 (rows on u only, e.g. the friction cone) and selects
 *   the kernels without the C products; D = NULL means D = 0.
 * Outputs:
 *     x [batch][N+1][nx]  u [batch][N][nu]  pi [batch][N+1][nx]   (required)
 *     P [batch][N+1][nx*nx]  p [batch][N+1][nx]  K [batch][N][nu*nx]  k [batch][N][nu]
 *     status [batch] (HpipmStatus codes)  iter [batch]  res [batch][4]  obj [batch]
 *     stat [batch][iter_max+2][18]
 *   Conventions (ocp_qp_ipm_solver.cpp:337-373, test/ocp_qp_ipm_solver.cpp:60-109):
 *     x[0] = x0; pi[k] is the multiplier of x[k] = A x[k-1] + ... (hpipm pi[k-1]),
 *     pi[k] = P[k] x[k] + p[k]; u[k] = K[k] x[k] + k[k]; stage 0 as rebuilt.
 *
 * Dimensions: 1 <= nx, nu <= 12, 1 <= N <= 1024, 0 <= ng <= 64.  nx = nu = 12
 * (the SRBD model) takes the fast path; smaller problems are zero-padded
 * inside the kernel (exact: padded states stay 0, padded inputs get R = 1).
 */
#ifndef SRBD_QP_H_
#define SRBD_QP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRBD_QP_ABI_VERSION 12
#define SRBD_QP_MAX_NX 12
#define SRBD_QP_MAX_NU 12
#define SRBD_QP_MAX_NG 64

/* error codes (returned by every entry point) */
enum {
  SRBD_QP_OK = 0,
  SRBD_QP_EINVAL = -1,      /* NULL / inconsistent argument                 */
  SRBD_QP_EDIM = -2,        /* dimensions outside the supported range        */
  SRBD_QP_ENOMEM = -3,      /* device allocation failed                      */
  SRBD_QP_EDEVICE = -4,     /* HIP runtime error / no GPU                     */
  SRBD_QP_ECAPACITY = -5,   /* batch larger than the handle's capacity        */
  SRBD_QP_ESETTINGS = -6    /* settings rejected (checkSettings rules)        */
};

/* per-QP solver status, same codes as hpipm::HpipmStatus
 * (hpipm-cpp/include/hpipm-cpp/ocp_qp_ipm_solver.hpp:24-30)                */
enum {
  SRBD_QP_SUCCESS = 0,
  SRBD_QP_MAX_ITER = 1,
  SRBD_QP_MIN_STEP = 2,
  SRBD_QP_NAN_SOL = 3,
  SRBD_QP_UNKNOWN_FAILURE = 4
};

/* hpipm::HpipmMode (ocp_qp_ipm_solver_settings.hpp:10-15) */
enum { SRBD_QP_MODE_SPEED_ABS = 0, SRBD_QP_MODE_SPEED = 1, SRBD_QP_MODE_BALANCE = 2,
       SRBD_QP_MODE_ROBUST = 3 };

typedef struct srbd_qp_dims {
  int N;          /* horizon                                                */
  int nx, nu;     /* uniform state / input dimensions                        */
  int ng;         /* general constraints per stage (0 = none)                */
  int has_box_u;  /* 1 if lbu/ubu will be passed                             */
  int has_box_x;  /* 1 if lbx/ubx will be passed                             */
  int layout;     /* SRBD_QP_LAYOUT_QP_MAJOR (0, default) or _STAGE_MAJOR (1) */
} srbd_qp_dims;

/* Input layouts.  QP-major: every array [batch][stage][block] (Eigen order,
 * what the hpipm-cpp shim packs).  Stage-major: [stage][batch][block], so the
 * QPs of one wavefront are adjacent in HBM (longer contiguous streams); the
 * unconstrained solve reads it (the IPM and the linearisation write / read
 * QP-major only for now: srbd_qp_create rejects stage-major with
 * constraints).  Outputs are always QP-major.                              */
enum { SRBD_QP_LAYOUT_QP_MAJOR = 0, SRBD_QP_LAYOUT_STAGE_MAJOR = 1 };

/* hpipm::OcpQpIpmSolverSettings (ocp_qp_ipm_solver_settings.hpp:26-86);
 * srbd_qp_default_settings() gives the same defaults.                     */
typedef struct srbd_qp_settings {
  int mode;       /* HpipmMode: 0 SpeedAbs, 1 Speed, 2 Balance, 3 Robust; selects
                  * itref_corr_max 0 / 0 / 2 / 4             */
  int iter_max;
  double alpha_min;
  double mu0;
  double tol_stat, tol_eq, tol_ineq, tol_comp;
  double reg_prim;
  int warm_start;   /* 1: x/u output buffers hold the primal warm start     */
  int pred_corr;
  int ric_alg;      /* 0: classical Riccati; else the square-root recursion  */
  int split_step;
  int compute_residuals; /* unconstrained QPs (nc = 0): 1 (default) = res/obj, when
                          * given, hold the solution's KKT residual norms and
                          * objective (HPIPM's comp_res_exit; one extra pass over
                          * the QP data); 0 = they are zero-filled              */
  int f64_rescue;   /* fp32 solves with constraints only (ignored otherwise):
                     * 0 (default) = HPIPM's s_ocp_qp_ipm behaviour; n > 0 =
                     * the fp32 pass runs min(n, iter_max) iterations, then
                     * every QP it left with status != Success continues in
                     * fp64 (iter_max as given) on its data widened to fp64,
                     * starting from the fp32 iterate (x, u, pi, lam, t; cold
                     * when nx or nu < 12 or the iterate is not finite), and
                     * its outputs (x, u, pi, P, p, K, k, status, iter, res,
                     * obj, stat) are the fp64 solve's, narrowed.  The call
                     * then waits for the fp32 pass (it counts the QPs to
                     * re-solve on the host).                               */
  int f32_iters;    /* fp64 solves with constraints on 12 x 12 stages and
                     * iter_max >= 2 only (ignored otherwise): 0 (default) =
                     * fp64 throughout; n > 0 = a mixed-precision IPM: the data
                     * is narrowed once to fp32, the first m = min(n,
                     * iter_max - 1) iterations run in fp32 (half the bytes per
                     * sweep), and the fp64 IPM continues from that iterate (x,
                     * u, pi, lam, t) on the caller's fp64 data to the fp64
                     * tolerances for at most iter_max - m iterations; iter and
                     * stat count the fp64 iterations.  Contract: the mixed path
                     * never ends a QP worse than the fp64 path.  Every QP the
                     * continuation does not end with Success is solved again
                     * in fp64 exactly as the plain fp64 call would solve it
                     * (iter_max iterations, from the caller's x / u when
                     * warm_start is set, cold otherwise) and then carries that
                     * solve's outputs, bit for bit; the call waits once to
                     * count them.  Worst case per QP: iter_max iterations (m of
                     * them fp32) plus iter_max fp64 ones.                  */
  int lq_fact;      /* HPIPM's lq_fact (d_ocp_qp_ipm_arg_set "lq_fact",
                     * hpipm_d_ocp_qp_ipm.h:78,147), square-root Riccati only:
                     * -1 (default) = the mode's, as d_ocp_qp_ipm_arg_set_default
                     * sets it (Balance 1, Robust 2, else 0); 0 = Cholesky
                     * factorizations; 1 = Cholesky until a predictor step's
                     * linear residual exceeds 1e-5, then LQ for the rest of
                     * the solve; 2 = every stage factorization by LQ (the
                     * barrier Hessians are absorbed as columns, never summed).
                     * Ignored with ric_alg = 0. (ABI 11)                    */
} srbd_qp_settings;

typedef struct srbd_qp_data_f64 {
  const double *A, *B, *b, *Q, *S, *R, *q, *r;
  const double *lbu, *ubu, *lbu_mask, *ubu_mask;
  const double *lbx, *ubx, *lbx_mask, *ubx_mask;
  const double *C, *D, *lg, *ug, *lg_mask, *ug_mask;
  const double *x0;
} srbd_qp_data_f64;

typedef struct srbd_qp_solution_f64 {
  double *x, *u, *pi;      /* required                                     */
  double *P, *p, *K, *k;   /* optional Riccati outputs (may be NULL)        */
  int *status, *iter;      /* optional                                     */
  double *res;             /* optional [batch][4] max |res_stat|,|res_eq|,|res_ineq|,|res_comp| */
  double *obj;             /* optional [batch]                              */
  double *stat;            /* optional [batch][iter_max+2][18]: per-iteration
                            * statistics in HPIPM's ws->stat row layout, the
                            * rows hpipm-cpp copies into OcpQpIpmSolverStatistics
                            * (ocp_qp_ipm_solver.cpp:381-403): alpha_aff, mu_aff,
                            * sigma, alpha_prim, alpha_dual, mu, res_stat, res_eq,
                            * res_ineq, res_comp, obj, lq_fact (0: none),
                            * itref_pred (0), itref_corr (corrections of the
                            * step, mode Balance / Robust with boxes), then
                            * lin_res_stat, lin_res_eq of the last refinement
                            * check, lin_res_ineq, lin_res_comp (0: exact).    */
} srbd_qp_solution_f64;

/* fp32 twins (BASELINE config 5; HPIPM's s_ocp_qp_ipm, hpipm_s_ocp_qp_ipm.h:238):
 * same fields, same layout, float elements.  Tolerances below ~1e-6 are not
 * reachable in fp32; use the NMPC settings (1e-4). */
typedef struct srbd_qp_data_f32 {
  const float *A, *B, *b, *Q, *S, *R, *q, *r;
  const float *lbu, *ubu, *lbu_mask, *ubu_mask;
  const float *lbx, *ubx, *lbx_mask, *ubx_mask;
  const float *C, *D, *lg, *ug, *lg_mask, *ug_mask;
  const float *x0;
} srbd_qp_data_f32;

typedef struct srbd_qp_solution_f32 {
  float *x, *u, *pi;
  float *P, *p, *K, *k;
  int *status, *iter;
  float *res;
  float *obj;
  float *stat;
} srbd_qp_solution_f32;

typedef struct srbd_qp_handle_s* srbd_qp_handle;

/* Fill *s with hpipm-cpp's defaults (Speed, iter_max 15, tol 1e-8, mu0 100,
 * alpha_min 1e-8, reg_prim 1e-12, pred_corr 1, ric_alg 1, split_step 0).   */
void srbd_qp_default_settings(srbd_qp_settings* s);

/* Validate settings like OcpQpIpmSolverSettings::checkSettings
 * (ocp_qp_ipm_solver_settings.cpp:7-38); returns SRBD_QP_ESETTINGS with a
 * message retrievable by srbd_qp_last_error().                              */
int srbd_qp_check_settings(const srbd_qp_settings* s);

/* Create a solver for `dims` able to solve up to `batch_capacity` QPs per call
 * on HIP device `device`.  Allocates the device workspace and one stream.  */
int srbd_qp_create(const srbd_qp_dims* dims, int batch_capacity, int device,
                   srbd_qp_handle* out);

/* Device-resident batch solve, asynchronous on `stream` (a hipStream_t; NULL
 * = the handle's own stream): the call enqueues the whole solve and returns
 * without waiting -- the IPM's stop decision is taken on the device -- except
 * that settings->f64_rescue / f32_iters wait once for their first pass.
 * Every data/solution pointer is device memory.  With settings->warm_start the
 * x/u buffers are read as the warm start.  One handle serves one solve at a
 * time (its workspace); several handles run concurrently.
 * Cost of the asynchronous stop: the batched IPM enqueues all iter_max
 * iterations up front; the iterations after the device has stopped the solve
 * cost their dispatch only (about 2 to 6 launches per iteration, a few
 * microseconds each, so ~0.1 ms for the NMPC's iter_max 30).  fp64 solves of
 * up to 512 QPs with the classical Riccati (ric_alg 0), or the square root
 * without C rows (any mode: Balance / Robust refine in the same launch) run as
 * one launch instead (the latency IPM), which stops where it
 * converges.  With the square root and lq_fact 1 (Balance's) that call waits
 * for its stream once: a QP asking for the LQ factorization is solved again,
 * alone, on the batched kernels before the call returns.
 * SRBD_IPM_LATENCY_MAX (environment, QPs; 0 = off) moves that switch.     */
int srbd_qp_solve_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* settings,
                      const srbd_qp_data_f64* data, const srbd_qp_solution_f64* sol,
                      void* stream);

/* Host-buffer batch solve: copies to device, solves, copies back, waits.
 * Small unconstrained batches (<= 256 QPs, nx = nu = 12, N <= 26) are zero copy:
 * the kernel reads the handle's pinned staging buffer and writes the outputs
 * into it.  A single such QP with the classical Riccati (ric_alg 0, N <= 20:
 * the reference's call pattern) goes to the handle's resident server: a
 * one-workgroup kernel on its own stream that polls a mailbox in mapped host
 * memory, so a call costs no launch; it leaves its CU after 5 ms without a
 * request, after its first answer once it has been up 20 ms, or at
 * srbd_qp_destroy / process exit, and the next call relaunches it (also when
 * it left between the call's check and its post).  While it is up it holds
 * one CU, and a device-wide synchronize waits for it to leave.  Its stream
 * has the greatest priority: HIP maps a process's streams onto a few hardware
 * queues per priority that run their packets in order, so a kernel queued
 * behind the server on a shared queue would wait for it; default-priority
 * streams never share its queue, and another high-priority stream that does
 * waits at most the 20 ms lifetime.  SRBD_LAT_SERVER=0 (environment) launches
 * per call; SRBD_LAT_SERVER_IDLE_MS overrides the 5 ms (tests).          */
int srbd_qp_solve_host_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* settings,
                           const srbd_qp_data_f64* data, const srbd_qp_solution_f64* sol);

/* srbd_qp_solve_host_f64 that hands the caller the Riccati outputs early:
 * `on_factors(ctx)` runs at most once on the calling thread, before the call
 * returns, as soon as sol->P, p, K, k have been written to the caller's
 * buffers.  The call's return code and sol->status then decide whether they
 * are valid: the callback can run and the call still return an error (a
 * device failure after the factors were written) or a QP end with status 3
 * (NaN: the status is set after the callback), so a caller keeps what it
 * unpacked only on SRBD_QP_OK and status 0.  On the zero-copy single-QP path (above; fp64 classical
 * Riccati, N <= 20) that is while the kernel still runs its forward sweep,
 * u / pi and residual passes, so a caller can unpack the factors (the bulk of
 * the outputs) under the kernel's tail; elsewhere it runs after the solve.
 * The callback must not call into the handle.  Replaces the
 * d_ocp_qp_ipm_get_ric_P / _p / _K / _k reads of ocp_qp_ipm_solver.cpp:342-345
 * for the hpipm-cpp shim.  (ABI 12)                                          */
int srbd_qp_solve_host_cb_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* settings,
                              const srbd_qp_data_f64* data, const srbd_qp_solution_f64* sol,
                              void (*on_factors)(void* ctx), void* ctx);

/* The handle's pinned host staging for a srbd_qp_solve_host_f64 call of `batch`
 * QPs with `settings`: every field that *data / *sol have non-NULL (any value,
 * e.g. (void*)1: a marker) is replaced by its place in the staging buffer, the
 * others set NULL.  A caller that packs its QPs there and then passes the same
 * two structs to srbd_qp_solve_host_f64 saves both staging copies (the solve
 * skips a copy whose source already is its place); the outputs are left there.
 * The pointers are invalidated by the handle's destruction and by ANY later
 * srbd_qp_solve_host_* or srbd_qp_host_staging_* call on the handle that needs a
 * larger staging buffer (the old pinned buffer is freed): re-stage after such a
 * call, as the hpipm-cpp shim does on every solve.  SRBD_QP_ECAPACITY
 * when the call's buffers exceed the pinned staging size (8 MiB).  Replaces the
 * Eigen-pointer marshalling of ocp_qp_ipm_solver.cpp:226-289 for the shim.
 * (ABI 10)                                                                  */
int srbd_qp_host_staging_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* settings,
                             srbd_qp_data_f64* data, srbd_qp_solution_f64* sol);

/* fp32 twins of the two solve entry points (the handle serves both).      */
int srbd_qp_solve_f32(srbd_qp_handle h, int batch, const srbd_qp_settings* settings,
                      const srbd_qp_data_f32* data, const srbd_qp_solution_f32* sol,
                      void* stream);
int srbd_qp_solve_host_f32(srbd_qp_handle h, int batch, const srbd_qp_settings* settings,
                           const srbd_qp_data_f32* data, const srbd_qp_solution_f32* sol);

/* ------------------------------------------------------------------------
 * Soft box constraints (soft, additive to ABI 12): HPIPM's OCP-QP slack
 * variables (Zl / Zu / zl / zu / idxs / lls / lus, nsbx / nsbu) on box bounds.
 * A box bound marked soft gets a slack on each active side,
 *     lbx - sl <= x <= ubx + su,   sl >= lls,  su >= lus,
 * penalised in the cost by 1/2 Zl sl^2 + zl sl + 1/2 Zu su^2 + zu su (the same
 * for u), so a bound that x0 or a disturbance violates costs instead of making
 * the QP infeasible.  Dense per variable like the box masks: soft_* = 1 marks
 * the variable's box as soft; a side whose mask is 0 has no slack.  Z is the
 * diagonal of HPIPM's Zl / Zu (stored there as a vector too).
 * Caller's contract (device data, not checked): Z >= 0, z >= 0, Z + z > 0 on
 * every active soft side, and lls / lus finite.
 * (soft, additive to ABI 12)                                                 */
typedef struct srbd_qp_soft_f64 {      /* dense per variable, like the box masks            */
  const double *soft_u, *soft_x;       /* [batch][N][nu], [batch][N+1][nx]: 1 = this box is soft (NULL: none) */
  const double *Zl_u, *Zu_u, *zl_u, *zu_u;   /* [batch][N][nu]   diagonal Z (HPIPM stores Z as a vector) */
  const double *Zl_x, *Zu_x, *zl_x, *zu_x;   /* [batch][N+1][nx] stage 0 ignored, like lbx   */
  const double *lls_u, *lus_u, *lls_x, *lus_x; /* slack lower bounds, NULL = 0                */
} srbd_qp_soft_f64;
/* optional slack outputs, shaped like the bounds (any may be NULL); 0 where the
 * variable is not soft or the side is masked.  (soft, additive to ABI 12)     */
typedef struct srbd_qp_slack_f64 { double *sl_u, *su_u, *sl_x, *su_x; } srbd_qp_slack_f64;

/* srbd_qp_solve_f64 with soft boxes: device memory, asynchronous on `stream`.
 * soft->soft_u needs a handle with has_box_u (and Zl_u, Zu_u, zl_u, zu_u),
 * soft->soft_x one with has_box_x (and Zl_x ... zu_x); `slack` may be NULL.
 * Always runs the batched fp64 kernels (never the latency IPM).  Rejected:
 * ng > 0 (SRBD_QP_EDIM: soft general rows are not built); mode Balance /
 * Robust, f32_iters and f64_rescue (SRBD_QP_ESETTINGS: the refinement and the
 * fp32 kernels do not carry the slack rows).  warm_start = 1 warms x / u only;
 * the slacks always start cold.  iter, res and obj count the slack rows and
 * the penalty.  The slack state lives in a buffer the handle allocates on
 * first use (srbd_qp_memory_bytes counts it).  (soft, additive to ABI 12)    */
int srbd_qp_solve_soft_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* settings,
                           const srbd_qp_data_f64* data, const srbd_qp_soft_f64* soft,
                           const srbd_qp_solution_f64* sol, const srbd_qp_slack_f64* slack,
                           void* stream);
/* The same from host buffers: copies to the device, solves, copies back, waits
 * (a per-call device buffer; Riccati outputs and stat are not returned: pass
 * them NULL).  (soft, additive to ABI 12)                                     */
int srbd_qp_solve_soft_host_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* settings,
                                const srbd_qp_data_f64* data, const srbd_qp_soft_f64* soft,
                                const srbd_qp_solution_f64* sol, const srbd_qp_slack_f64* slack);

/* ------------------------------------------------------------------------
 * Backward pass (additive to ABI 12): the gradients of a scalar l of the solution with respect
 * to the QP data, from the cotangents gx = dl/dx [batch][N+1][nx] and gu = dl/du [batch][N][nu]
 * (the mpc.pytorch / OptNet pattern: learn cost weights or model matrices through the QP).
 * pi[k+1] multiplies A x[k] + B u[k] + b[k] - x[k+1] = 0 and pi[0] multiplies x0 - x[0] = 0.
 * The adjoint QP has the same A, B, Q, S, R with q := gx, r := gu, b := 0, x0 := 0; with its
 * solution (dx, du, dpi) and the forward solution (x, u, pi), per stage k:
 *   grad q = dx                  grad r = du           grad b = dpi[k+1]       grad x0 = dpi[0]
 *   grad Q = 1/2 (dx x' + x dx')   (k = 0..N)          grad R = 1/2 (du u' + u du')
 *   grad S = du x' + u dx'   (nu x nx)
 *   grad A = pi[k+1] dx' + dpi[k+1] x'                 grad B = pi[k+1] du' + dpi[k+1] u'
 * dx[0] = 0, so grad q and grad Q are exactly zero at stage 0.  grad Q and grad R are the
 * gradients with respect to a symmetric matrix: a caller who moves Q_ij and Q_ji together sees
 * grad Q_ij + grad Q_ji.
 * Input boxes (a handle with has_box_u): input (k, i) is active iff its bound is unmasked and
 * u - lbu < act_tol or ubu - u < act_tol.  The adjoint QP is then solved on a masked copy of the
 * stages that pins du = 0 there, the way a missing input is padded: column i of B and row i of S
 * cleared, row and column i of R cleared with 1 on the diagonal, entry i of r cleared.  The
 * formulas are unchanged.  The result is the gradient of the problem with that active set held
 * fixed; where a bound is weakly active it is undefined, which is the caller's concern.
 * The grad arrays are device memory in the layout of the inputs they belong to (column-major
 * blocks); any may be NULL and is then neither formed nor written.  gx or gu may be NULL (zero),
 * not both.  data is the forward call's, sol its x, u, pi (read only; the other fields are not
 * read).  Of the settings only reg_prim and ric_alg are read: the adjoint factorises what the
 * forward solve factorised.
 * Asynchronous on `stream` like srbd_qp_solve_f64, whose workspace it uses: it follows the
 * forward solve on the same stream, one call at a time per handle.  The adjoint solution and
 * the masked stages live in a buffer the handle allocates on first use (srbd_qp_memory_bytes
 * counts it): per QP 2 (N+1) nx + N nu doubles and (N+1) max(nx, nu) zeros, and with has_box_u
 * N (2 nx nu + nu nu + nu) more, 71 KB per QP at N = 20, nx = nu = 12.
 * Checks: a NULL handle, data, sol, grad or settings, A...x0 or x / u / pi missing, lbu / ubu
 * missing on a handle with has_box_u, both cotangents NULL, act_tol negative or not finite:
 * SRBD_QP_EINVAL; a handle with ng > 0, has_box_x or the stage-major layout: SRBD_QP_EDIM; batch
 * above the capacity: SRBD_QP_ECAPACITY; batch == 0: SRBD_QP_OK.  A failed check launches and
 * writes nothing.
 * General rows on the inputs and the gradients of D and the bounds: srbd_qp_solve_backward_rows_f64
 * below.  Out of scope: rows on the states (C), state boxes, soft boxes, a
 * cotangent for pi, P or K, fp32 and the mixed-precision settings, the stage-major layout,
 * srbd_qp_multi_*, the hpipm-cpp shim, and the NMPC step (its SQP loop and line search).
 * ---------------------------------------------------------------------- */
typedef struct srbd_qp_grad_f64 {   /* device, outputs, same layout as the inputs; any may be NULL */
  double *A, *B, *b, *Q, *S, *R, *q, *r, *x0;
} srbd_qp_grad_f64;

int srbd_qp_solve_backward_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* settings,
                               const srbd_qp_data_f64* data,        /* the forward call's data            */
                               const srbd_qp_solution_f64* sol,     /* the forward x, u, pi (read only)   */
                               const double* gx, const double* gu,  /* cotangents; either may be NULL = 0 */
                               double act_tol,                      /* >= 0, finite; read with has_box_u  */
                               const srbd_qp_grad_f64* grad, void* stream);
/* The number of inputs the last srbd_qp_solve_backward_f64 on this handle pinned, per QP:
 * count [batch] (device), copied on `stream` behind that call.  SRBD_QP_EINVAL without
 * has_box_u, or for more QPs than that call had; batch == 0 returns SRBD_QP_OK.               */
int srbd_qp_backward_pinned_f64(srbd_qp_handle h, int batch, int* count, void* stream);

/* ------------------------------------------------------------------------
 * Backward pass through general rows on the inputs, and the gradients of D and of the bounds
 * (additive to ABI 12).  srbd_qp_solve_backward_f64 with two more outputs structs and any ng in
 * 0..64 with C == NULL (rows on u only: the friction cone of SRBD_QP_SRBD_CONE), with or without
 * has_box_u, in the QP-major layout.
 * Signs are those above; the Lagrangian gains  + nu_k' (E_k u_k - e_k).  E_k holds the active
 * rows of stage k = 0..N-1: a unit row for each pinned input (the rule above), then row j of D_k
 * for each active general row: its bound is unmasked and D_j u - lg_j < act_tol or
 * ug_j - D_j u < act_tol.  e_k is the bound that is active: the nearer one, the lower on a tie.
 * lg[N], ug[N] are never active (C == NULL) and get gradient 0.
 * The adjoint QP is the one above with E_k du_k = 0 added; dnu_k are its multipliers.  The nine
 * formulas are unchanged (the true A ... R, the forward x, u, pi, the adjoint dx, du, dpi), and
 *   grad D_j = dnu_j u' + nu_j du'        for an active general row j
 *   grad lg_j = -dnu_j  if the lower bound is the active one,  grad ug_j = -dnu_j  if the upper
 *   grad lbu_i, grad ubu_i: the same for a pinned input
 * and every entry of an inactive row or bound is exactly 0.  Neither multiplier needs the IPM's
 * lam.  With E_k' = Y T (Y orthonormal, T upper triangular):
 *   rho  = R u  + S x  + r  + B' pi[k+1]      nu  = -T^-1 Y' rho
 *   rho~ = R du + S dx + gu + B' dpi[k+1]     dnu = -T^-1 Y' rho~
 * The constrained adjoint is still one unconstrained Riccati solve, on the stages
 *   B~ = B P,  S~ = P S,  R~ = P R P + (I - P),  r~ = P gu,   P = I - Y Y'
 * (the rotated form with Qf = [Z Y], its Y part cleared like a missing input, written in the
 * caller's coordinates: du = Z w comes out of the solve).  A stage without an accepted general
 * row is cleared exactly as above, so on a handle with ng == 0, or when no row is active, the
 * nine gradients are bit for bit those of srbd_qp_solve_backward_f64.
 * Dependent rows: pins come first, ascending; then the active general rows, ascending, each
 * restricted to the unpinned coordinates.  A row is accepted iff the norm of its part orthogonal
 * to the rows already accepted exceeds rank_tol times its own norm and fewer than nu rows are
 * accepted so far; otherwise it is dropped: nu = dnu = 0 and its gradients are 0.  The gradient
 * at such a point is not defined (the caller's concern, like a weakly active bound); the result
 * is finite.
 * grad and grad_rows: device memory in the layout of the inputs (grad D: [batch][N][ng*nu],
 * grad lg / ug: [batch][N+1][ng], grad lbu / ubu: [batch][N][nu]); any field may be NULL and
 * costs nothing then; one that is passed is fully written, zeros included.  Either struct may be
 * NULL, not both.
 * Checks, in this order: those of srbd_qp_solve_backward_f64 with the same codes and messages,
 * except that ng > 0 is accepted; in addition a rank_tol outside [0, 1) or not finite is
 * SRBD_QP_EINVAL (after act_tol), data->C != NULL on a handle with ng > 0 is SRBD_QP_EDIM (where
 * ng > 0 was rejected), and D, lg or ug missing with ng > 0 is SRBD_QP_EINVAL (after lbu / ubu).
 * A failed check launches and writes nothing.
 * Asynchronous on `stream`, like srbd_qp_solve_backward_f64 and under the same contract.  The
 * handle's backward buffer holds the projected stages whenever has_box_u or ng > 0, and three
 * ints per QP; no factor is stored: the kernel that writes grad_rows forms it again from D.
 * ---------------------------------------------------------------------- */
typedef struct srbd_qp_grad_rows_f64 {   /* device, outputs, layout of the inputs; any may be NULL */
  double *D, *lg, *ug, *lbu, *ubu;
} srbd_qp_grad_rows_f64;

int srbd_qp_solve_backward_rows_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* settings,
                                    const srbd_qp_data_f64* data, const srbd_qp_solution_f64* sol,
                                    const double* gx, const double* gu, double act_tol,
                                    double rank_tol,                     /* in [0, 1)                   */
                                    const srbd_qp_grad_f64* grad,        /* the nine; may be NULL       */
                                    const srbd_qp_grad_rows_f64* grad_rows, /* may be NULL, not both    */
                                    void* stream);
/* What the last srbd_qp_solve_backward_rows_f64 on this handle found, per QP: count [batch][3]
 * (device): inputs pinned, general rows accepted, general rows dropped; copied on `stream` behind
 * that call.  SRBD_QP_EINVAL for more QPs than that call had; batch == 0 returns SRBD_QP_OK.   */
int srbd_qp_backward_active_f64(srbd_qp_handle h, int batch, int* count, void* stream);

/* ------------------------------------------------------------------------
 * Device-side SRBD linearisation: the producer of the QP data, i.e.
 * NMPCSolver::prepareQpStructures (NMPC_solver.cpp:276-314) with the model of
 * dynamics/SRBD_model.cpp:75-295 (RK4 defect with Euler Jacobians, friction
 * cone as a relaxed log barrier in the cost), for a batch of linearisation
 * points, written straight into the solver's input buffers.
 * Parameters: config/mpc_option.yaml:2-18, NMPC_solver.cpp:53-82, :332-351.
 * ---------------------------------------------------------------------- */
typedef struct srbd_model_params {
  double Q[12], Qf[12];   /* diagonal state weights (mpc_option.yaml Q, Qf)    */
  double R;               /* input weight                                      */
  double dt;              /* discretisation step                               */
  double Lbody[3];        /* body inertia diagonal (the model stores L^-1)     */
  double mu_b, theta_b;   /* relaxed-barrier weight / threshold                */
  double mass;
  double foot_r[3], foot_l[3];  /* foot positions in the body frame          */
  double mu, Lfx, Lfz, fmax, fmin;  /* friction cone / torque limits         */
  double x_ref[12];       /* reference state                                   */
  double qf_scale;        /* terminal weight factor (<= 0: N, NMPC_solver.cpp:58) */
  double u_lo[12], u_hi[12];  /* box on u + du for SRBD_QP_SRBD_BOX_U         */
} srbd_model_params;

enum { SRBD_QP_SRBD_NONE = 0, SRBD_QP_SRBD_BOX_U = 1, SRBD_QP_SRBD_CONE = 2 };

/* mpc_option.yaml / setupDynamics defaults (box: (+-50, +-50, 0..300 N,
 * +-5 Nm) per foot). */
void srbd_qp_srbd_default_params(srbd_model_params* p);

/* Linearise `batch` SRBD trajectories on the handle's device and stream (or
 * `stream`): xs [batch][N+1][12], us [batch][N][12] (device).  Fills A, B, b,
 * Q, S, R, q, r of `out` and, per `constraints`, lbu/ubu (BOX_U) or D, lg,
 * ug, lg_mask, ug_mask (CONE: ng = 24, lg = -f(u), ug masked; C = 0 is
 * written only if out->C is given -- pass C = NULL to the solve).  The handle's
 * dims must be N, nx = nu = 12 (and ng = 24 for CONE).  Asynchronous.       */
int srbd_qp_srbd_linearize_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                               int constraints, const double* xs, const double* us,
                               const srbd_qp_data_f64* out, void* stream);

/* Batched filter line search of the SQP iteration (NMPCSolver::linearSearch,
 * NMPC_solver.cpp:149-274): per QP, merit phi (cost + friction barrier) and
 * theta (shooting defect) at xs/us, trial steps alpha, beta alpha, ... along
 * the QP solution (dx [B][N+1][12], du [B][N][12]) until the filter accepts;
 * xs/us (device, in place) move to the accepted point.  alpha [B] is read and
 * written like the reference's persistent alpha_ (NMPC_solver.h:104); merit
 * [B][3] (phi, theta, dphi) and converged [B] (dphi > -1e-3 && theta < 1e-6)
 * are optional.  Constants: NMPC_solver.h:97-103.                         */
typedef struct srbd_linesearch_params {
  double theta_max, theta_min, eta, beta_phi, beta_theta, beta_alpha, alpha_min;
} srbd_linesearch_params;
void srbd_qp_srbd_default_linesearch(srbd_linesearch_params* p);
int srbd_qp_srbd_linesearch_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                const srbd_linesearch_params* ls, double* xs, double* us,
                                const double* dx, const double* du, double* alpha, double* merit,
                                int* converged, void* stream);

/* The SQP loop of NMPCSolver::controlLoop (NMPC_solver.cpp:362-372) for a batch
 * of robots: for it < sqp_max_loop (mpc_option.yaml sqp_max_loop):
 * prepareQpStructures (srbd_qp_srbd_linearize_f64 at xs, us), solveQpProblems
 * (srbd_qp_solve_f64 with settings and x0 - xs[:, 0], NMPC_solver.cpp:316-330),
 * checkConvergence = linearSearch (srbd_qp_srbd_linesearch_f64: xs, us move to
 * the accepted point, alpha persists); a robot whose line search reports
 * convergence stops there (`if (checkConvergence()) break;`) and is not changed
 * again.  xs [batch][N+1][12], us [batch][N][12] (in/out), x0 [batch][12],
 * alpha [batch] (in/out), sqp_iter [batch] (SQP iterations run) and converged
 * [batch] (out): device memory.  The QP data, solution and loop state live in
 * a scratch buffer of the handle (allocated on first use, capacity-sized).
 * Runs on the handle's stream and returns when every robot has stopped or
 * sqp_max_loop iterations ran (one 4-byte read-back per iteration).  The
 * handle's dims: N, nx = nu = 12, and has_box_u / ng = 24 per `constraints`. */
int srbd_qp_srbd_nmpc_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                          const srbd_linesearch_params* ls, const srbd_qp_settings* settings,
                          int constraints, int sqp_max_loop, double* xs, double* us,
                          const double* x0, double* alpha, int* sqp_iter, int* converged);

/* Plans (additive to ABI 12): per-robot, per-stage overrides of srbd_model_params
 * (device memory, fp64, dense).  A NULL field means "the value in srbd_model_params
 * for every robot and stage".  One robot's x_ref block is NMPCSolver::x_ref_, the
 * column-major 12 x (N+1) reference trajectory (NMPC_solver.cpp:67, :306, :313).
 *   x_ref   replaces params->x_ref in the cost (q = w (x - x_ref[k]), the terminal
 *           stage with qf_scale Qf included) and in the line search's merit phi and
 *           gradient Jphi_x;
 *   foot_*  replace params->foot_* at that stage wherever the model forms foot - pos:
 *           the dynamics (all four RK4 slopes), its Jacobians A / B and the line
 *           search's shooting defect;
 *   fz_max  replaces params->fmax for that foot and stage in row 4 (fz <= fmax) of the
 *           foot's twelve cone rows: the relaxed barrier in R / r, lg = -f(u) with
 *           CONE, and the line search's merit.  With BOX_U the upper bound of that
 *           foot's fz becomes min(u_hi[fz], fz_max).
 * Caller's contract (device data, not checked): fz_max > fmin and fz_max > u_lo[fz];
 * a swing foot gets a small positive limit, not 0.                               */
typedef struct srbd_plan_f64 {
  const double* x_ref;   /* [batch][N+1][12]  reference state per stage               */
  const double* foot_r;  /* [batch][N][3]     right-foot position at stage k          */
  const double* foot_l;  /* [batch][N][3]     left-foot position                      */
  const double* fz_max;  /* [batch][N][2]     normal-force limit (right, left): the
                          *                   contact schedule                         */
} srbd_plan_f64;

/* The three entry points above with a plan; the other arguments and their checks are
 * the same.  plan == NULL, or a plan whose fields are all NULL, is the call without a
 * plan: the same kernels, the same bits.  The plan's arrays are read by the launched
 * kernels: keep them alive like xs / us.                                          */
int srbd_qp_srbd_linearize_plan_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                    const srbd_plan_f64* plan, int constraints, const double* xs,
                                    const double* us, const srbd_qp_data_f64* out, void* stream);
int srbd_qp_srbd_linesearch_plan_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                     const srbd_plan_f64* plan, const srbd_linesearch_params* ls,
                                     double* xs, double* us, const double* dx, const double* du,
                                     double* alpha, double* merit, int* converged, void* stream);
int srbd_qp_srbd_nmpc_plan_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                               const srbd_plan_f64* plan, const srbd_linesearch_params* ls,
                               const srbd_qp_settings* settings, int constraints, int sqp_max_loop,
                               double* xs, double* us, const double* x0, double* alpha,
                               int* sqp_iter, int* converged);

/* ------------------------------------------------------------------------
 * The closed loop (additive to ABI 12): what a controller or a batched simulation does
 * between two NMPC steps, and T ticks of the whole receding-horizon loop.  The reference
 * stops at one step (NMPCSolver::controlLoop repeats it N_rep times for timing); the loop
 * every caller writes around a step is hpipm-cpp/examples/example_mpc.cpp's: apply u[0],
 * move the plant, shift the previous solution by one stage, slide the plan's window.
 * ---------------------------------------------------------------------- */
typedef struct srbd_advance_f64 {
  int substeps;          /* plant RK4 steps per tick, each dt / substeps; >= 1            */
  const double* wrench;  /* [batch][6] external torque (3) and force (3) on the body, world
                          * frame, held over the tick; NULL = none                         */
} srbd_advance_f64;

/* One tick's plant step and shift of the guess.  Asynchronous on `stream` (NULL = the
 * handle's own stream); all memory is device memory, xs / us 16-byte aligned.  Per robot, in
 * this order:
 *  1. Applied input: u0 = us[0], written to u_applied ([batch][12]) when that is given.
 *  2. Plant step, when x ([batch][12], in place) is given: x is replaced by `substeps`
 *     classical RK4 steps of length dt / substeps of xdot = f(x, u0) + w.  f is the SRBD
 *     continuous model (SRBDModel::GetContinuousDynamic) with the feet of stage 0 of
 *     plan->foot_r / foot_l, or params->foot_* where that field or the plan is NULL; w adds
 *     wrench[0:3] to rows 3..5 (the angular-momentum rate) and wrench[3:6] / mass to rows
 *     9..11.  The plant applies u0 as it is: it clamps nothing and applies no fz_max -- unless
 *     a contact model is set on the handle (srbd_qp_srbd_set_contact_f64 below), which
 *     replaces this step and step 1's u0 by its own statement.
 *  3. New last stage: xN = one RK4 step of the model over dt from the old xs[N] with the old
 *     us[N-1] and the feet of the plan's stage N-1, no wrench: the shifted guess has zero
 *     shooting defect at its last stage.
 *  4. Shift: xs[k] <- xs[k+1] for k = 0..N-1, then xs[N] <- xN; us[k] <- us[k+1] for
 *     k = 0..N-2, us[N-1] stays.  Shifted entries are bit copies.  xs[0] is the old xs[1], not
 *     x: the step forms x0 - xs[:, 0] itself (NMPC_solver.cpp:320).
 * `plan` is this tick's window (may be NULL); only its feet are read (and, with a contact
 * model, row 0 of fz_max).
 * Checks: NULL h / params / adv / xs / us and substeps < 1 are SRBD_QP_EINVAL; the handle
 * needs nx = nu = 12 (SRBD_QP_EDIM); batch above the capacity is SRBD_QP_ECAPACITY;
 * batch == 0 returns SRBD_QP_OK.                                                    */
int srbd_qp_srbd_advance_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                             const srbd_plan_f64* plan,   /* this tick's window, may be NULL */
                             const srbd_advance_f64* adv,
                             double* xs, double* us,      /* [batch][N+1][12], [batch][N][12], in place */
                             double* x,                   /* [batch][12] plant state, in place; NULL = shift only */
                             double* u_applied,           /* [batch][12] out, optional       */
                             void* stream);

typedef struct srbd_rollout_f64 {
  int ticks;             /* T >= 0                                                         */
  int plan_stages;       /* P: stages per robot in the plan's arrays (x_ref [batch][P+1][12],
                          * foot_* [batch][P][3], fz_max [batch][P][2]); P >= N + T - 1.
                          * Ignored when plan is NULL / all fields NULL.                    */
  int substeps;          /* as srbd_advance_f64                                            */
  const double* wrench;  /* [batch][T][6], NULL = none                                     */
  double alpha_reset;    /* > 0: every tick starts its line search from this alpha;
                          * 0: alpha persists across ticks like the reference's alpha_      */
  double* x_log;         /* [batch][T+1][12] optional: x_log[0] = the x passed in           */
  double* u_log;         /* [batch][T][12]   optional: the applied inputs                   */
  int* sqp_iter_log;     /* [batch][T] optional                                             */
  int* converged_log;    /* [batch][T] optional                                             */
} srbd_rollout_f64;

/* T ticks of the closed loop.  Synchronous (it inherits the step's per-iteration read-back),
 * on the handle's stream.  For t = 0..T-1:
 *  1. the window W_t = stages t..t+N of the long plan (x_ref rows t..t+N, feet and fz_max
 *     rows t..t+N-1; NULL fields stay NULL) is gathered dense into a scratch buffer of the
 *     handle (allocated on the first rollout with a plan, capacity-sized; counted by
 *     srbd_qp_memory_bytes);
 *  2. if alpha_reset > 0, every robot's alpha is set to it.  The line search leaves a
 *     shrunken alpha behind and nothing restores it: with alpha_reset = 0 (the reference's
 *     persistent alpha_) later ticks may start from a step length too small to converge;
 *  3. srbd_qp_srbd_nmpc_plan_f64 runs with W_t and x0 = x;
 *  4. its sqp_iter / converged go to column t of the logs;
 *  5. srbd_qp_srbd_advance_f64 runs with W_t and wrench[:, t];
 *  6. u_log[:, t] and x_log[:, t+1] are written.
 * On return x is the plant state after T ticks, xs / us the shifted guess for tick T and alpha
 * as the last step left it.  The results are the bits of a caller's loop over 1-6 through the
 * two public entry points.  ticks == 0 or batch == 0 returns SRBD_QP_OK (x_log[:, 0] written
 * when given and batch > 0); plan_stages < N + T - 1 with a non-empty plan, substeps < 1 and a
 * negative alpha_reset are SRBD_QP_EINVAL; the other checks are the step's.            */
int srbd_qp_srbd_rollout_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                             const srbd_plan_f64* plan, const srbd_linesearch_params* ls,
                             const srbd_qp_settings* settings, int constraints, int sqp_max_loop,
                             const srbd_rollout_f64* roll,
                             double* xs, double* us, double* x, double* alpha);

/* ------------------------------------------------------------------------
 * Robots (additive to ABI 12): per-robot overrides of six constants of srbd_model_params,
 * for batches whose robots differ (domain randomisation: the plant is not the model the
 * controller believes) or that sweep a weight or a friction coefficient over one plan.
 * They attach to the handle in one of two roles, and every SRBD entry point issued
 * afterwards on that handle (linearise, line search, NMPC step, advance, rollout; plain and
 * _plan_ alike) reads robot i's values at row i.
 *   SRBD_QP_ROBOTS_MODEL  what the controller believes; all six fields apply.
 *     Linearisation: A through L^-1, B through 1 / mass, b through the RK4 of the dynamics;
 *     the friction barrier's part of R / r with the robot's mu and R; Q, q with the robot's
 *     Q and Qf (qf_scale stays params->qf_scale); with CONE, the mu entries of D and lg.
 *     Line search: merit, gradient and shooting defect.  Advance: the model step that
 *     makes the new last stage xs[N].
 *   SRBD_QP_ROBOTS_PLANT  the true robot; only mass and Lbody may be given.  Read by the
 *     plant step of srbd_qp_srbd_advance_f64 (and so by the rollout's) and by nothing else;
 *     the wrench's force / mass uses the plant's mass.  A field that is NULL here, or the
 *     whole role when it is not set, is the MODEL role's value, then params'.
 * The call copies the six pointers and does no device work.  The arrays are device memory
 * with at least `batch` rows of each later call; they are read by the launched kernels: keep
 * them alive and unchanged until those have finished.  robots == NULL, or a struct whose
 * fields are all NULL, clears the role; with both roles clear the calls are what they are
 * without this entry point: the same kernels, the same bits.
 * Caller's contract (device data, not checked): mass, Lbody, mu, R > 0 and Q, Qf >= 0.
 * Checks: NULL handle, a role other than the two, or a PLANT role with mu, Q, Qf or R are
 * SRBD_QP_EINVAL; a handle without nx = nu = 12 is SRBD_QP_EDIM.
 * Not per robot (out of scope): u_lo / u_hi, fmin, Lfx / Lfz, dt, the barrier constants;
 * srbd_qp_multi_* (a multi-device handle has no roles) and the hpipm-cpp shim.
 * ---------------------------------------------------------------------- */
typedef struct srbd_robots_f64 { /* device memory, fp64, dense; NULL field = the value in srbd_model_params */
  const double* mass;    /* [batch]      */
  const double* Lbody;   /* [batch][3]   body inertia diagonal */
  const double* mu;      /* [batch]      friction coefficient  */
  const double* Q;       /* [batch][12]  */
  const double* Qf;      /* [batch][12]  (qf_scale stays the one in srbd_model_params) */
  const double* R;       /* [batch]      */
} srbd_robots_f64;
enum { SRBD_QP_ROBOTS_MODEL = 0, SRBD_QP_ROBOTS_PLANT = 1 };
int srbd_qp_srbd_set_robots_f64(srbd_qp_handle h, int role, const srbd_robots_f64* robots);

/* ------------------------------------------------------------------------
 * Backward pass of the linearisation (additive to ABI 12): the gradients of a scalar l with
 * respect to what a caller sets per robot (srbd_robots_f64: mass, Lbody, mu, Q, Qf, R) and per
 * robot and stage (srbd_plan_f64: x_ref, foot_r, foot_l, fz_max), from the cotangents of the QP
 * arrays srbd_qp_srbd_linearize_plan_f64 writes -- what srbd_qp_solve_backward_f64 /
 * srbd_qp_solve_backward_rows_f64 return.  With them the chain robots / plan -> linearise ->
 * solve -> loss is differentiable end to end, one call per link.  The linearisation point xs, us
 * is held fixed.
 * For every array X the linearisation writes, cot->X is dl/dX in X's own layout (column-major
 * blocks).  The result for a parameter theta of robot i is the element-wise inner product
 * sum_X <cot->X, dX/dtheta> over that robot's blocks as the linearisation writes them: both
 * (i, j) and (j, i) of a symmetric block count, the convention of grad Q / grad R above.
 * The gradient is per robot (plan quantities: per robot and stage) whether the forward value came
 * from the robots / the plan or from srbd_model_params; a caller with one shared value sums over
 * the batch.  With s = qf_scale (N when <= 0), w_k = Q (k < N) or s Qf (k = N), e = xs - x_ref:
 *   grad Q_j  = sum_{k<N} (cot Q[k][j][j] + cot q[k][j] e_kj)
 *   grad Qf_j = s (cot Q[N][j][j] + cot q[N][j] e_Nj)         grad x_ref[k][j] = -w_kj cot q[k][j]
 * Input cost and friction barrier (stage k < N): v_c (c = 0..23) are the cone rows f(u), a_c row c
 * of Ac, b', b'' the relaxed barrier's derivatives and b''' = -2 mu_b / v^3 (v > theta_b; else
 * 0).  The linearisation writes r = R u + sum_c b'_c a_c and R = R I + sum_c b''_c a_c a_c'.  With
 * s1_c = a_c' cot r, s2_c = a_c' (cot R) a_c and vbar_c = b''_c s1_c + b'''_c s2_c (CONE:
 * - cot lg[k][c]):
 *   grad R       = sum_k (tr cot R + cot r . u)
 *   grad fz_max[k][leg] = vbar_{12 leg + 4}; BOX_U with a plan: + cot ubu[k][6 leg + 2] where
 *                  fz_max < u_hi[fz] strictly (a tie belongs to u_hi); cot lbu reaches nothing
 *   grad mu      = sum_k sum_{c % 12 < 4} (vbar_c fz_leg + b'_c cot r[fz_leg]
 *                  + b''_c e_fz' (cot R + cot R') a_c); CONE: + cot D where D holds mu
 * Dynamics: A = I + dt J_x is linear in 1 / Lbody (blocks J00, J01), B = dt J_u in the feet
 * ([p]x blocks) and in 1 / mass; b (the RK4 defect) depends on 1 / Lbody, 1 / mass and the feet
 * through all four slopes, differentiated in reverse.  grad Lbody_j = -grad (1 / Lbody_j) /
 * Lbody_j^2 and grad mass = -grad (1 / mass) / mass^2.
 * Forward values are read exactly as srbd_qp_srbd_linearize_plan_f64 reads them: the handle's
 * MODEL role, the plan, then params.  Of cot, A, B, b, Q, R, q, r are read, ubu with BOX_U, D and
 * lg with CONE; any may be NULL (zero); the other fields (S, C, ug, the masks, ...) are ignored.
 * cot's A, B, R and D are read 16 bytes at a time and must be 16-byte aligned.
 * An output of grad that is passed is fully written, zeros included; a NULL one costs nothing.
 * The sums over a robot's stages are formed in a fixed order: the same inputs give the same
 * bits.  Per-stage partial sums (6 doubles per stage) live in a buffer the handle allocates on
 * first use, capacity-sized (srbd_qp_memory_bytes counts it).
 * Asynchronous on the handle's stream or `stream`, like the forward call.  An active set on the
 * handle is not consulted: the call covers QPs 0..batch-1 of a dense batch.
 * Checks, before any device work, in the forward call's order and with its codes: NULL h,
 * params, xs, us, cot or grad: SRBD_QP_EINVAL; a handle without nx = nu = 12: SRBD_QP_EDIM; batch
 * above the capacity: SRBD_QP_ECAPACITY; unknown constraints, or CONE on a handle without ng = 24:
 * SRBD_QP_EINVAL.  Then a grad whose fields are all NULL: SRBD_QP_EINVAL; batch == 0: SRBD_QP_OK.
 * A failed check launches and writes nothing.
 * Out of scope: gradients with respect to xs, us and x0; the constants that are not per robot
 * (dt, mu_b, theta_b, Lfx, Lfz, fmin, u_lo, u_hi, qf_scale); the PLANT role, the plant step and
 * the rollouts; subsets / active sets; fp32; srbd_qp_multi_* and the hpipm-cpp shim.
 * ---------------------------------------------------------------------- */
typedef struct srbd_lin_grad_f64 {   /* device, outputs; any may be NULL and then costs nothing */
  double *mass;            /* [batch]        */
  double *Lbody;           /* [batch][3]     */
  double *mu;              /* [batch]        */
  double *Q, *Qf;          /* [batch][12]    */
  double *R;               /* [batch]        */
  double *x_ref;           /* [batch][N+1][12] */
  double *foot_r, *foot_l; /* [batch][N][3]  */
  double *fz_max;          /* [batch][N][2]  */
} srbd_lin_grad_f64;

int srbd_qp_srbd_linearize_backward_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                        const srbd_plan_f64* plan /* may be NULL */, int constraints,
                                        const double* xs, const double* us,
                                        const srbd_qp_data_f64* cot /* cotangents, fields as in `out` */,
                                        const srbd_lin_grad_f64* grad, void* stream);

/* ------------------------------------------------------------------------
 * The two backward passes in one (additive to ABI 12): robot and plan gradients straight from the
 * solve.  The ten outputs of grad are what
 *   1. srbd_qp_solve_backward_rows_f64(h, batch, settings, data, sol, gx, gu, act_tol, rank_tol,
 *      &all_nine, &rows, stream)
 *   2. srbd_qp_srbd_linearize_backward_f64(h, batch, params, plan, constraints, xs, us,
 *      cot = those arrays, grad, stream)
 * return at the same act_tol, rank_tol and settings, and grad_x0 is the first call's grad x0; the
 * gradients of A, B, Q, S, R and D are never formed.  Every block of them is two outer products
 * of vectors the handle holds, so the linearisation's reverse model reads, for stage k < N, with
 * pi+ = pi[k+1], dpi+ = dpi[k+1] and x, u, dx, du of stage k:
 *   cot A_ij = pi+_i dx_j + dpi+_i x_j        cot B_ij = pi+_i du_j + dpi+_i u_j
 *   cot R_ii = du_i u_i,  cot R_ij + cot R_ji = du_i u_j + u_i du_j      cot Q[k]_jj = dx_kj x_kj
 *   cot q[k] = dx_k (k <= N)     cot r = du     cot b = dpi+     grad x0 = dpi[0]
 *   CONE: cot D_jc = dnu_j u_c + nu_j du_c,  cot lg_j = -dnu_j  (nu, dnu: the multipliers of the
 *         rows and of their adjoint; the cone's rows have no upper side, ug_mask = 0)
 *   BOX_U: cot ubu_i = -dnu_i of an input pinned at its upper bound
 * only where the linearisation depends on a robot's or a plan's value: 47 sums per stage.
 * Modes and handle: SRBD_QP_SRBD_NONE, _BOX_U and _CONE with nx = nu = 12 in the QP-major layout.
 * data is what srbd_qp_srbd_linearize[_plan]_f64 wrote at xs, us with the same params, plan and
 * MODEL role, which are read as the linearisation reads them; sol is the forward x, u, pi.  x, u,
 * pi, xs, us need only be 8-byte aligned.  An active set on the handle is not consulted.
 * An output that is passed is fully written; a NULL one costs nothing.  The same inputs give the
 * same bits.  srbd_qp_backward_active_f64 reports this call's counts.
 * Checks, in this order, before any device work, with the codes and messages of the two calls:
 *   1. those of srbd_qp_srbd_linearize_backward_f64: NULL h, params, xs, us or grad: SRBD_QP_EINVAL;
 *      a handle without nx = nu = 12: SRBD_QP_EDIM; batch above the capacity: SRBD_QP_ECAPACITY;
 *      unknown constraints, or CONE on a handle without ng = 24: SRBD_QP_EINVAL;
 *   2. those of srbd_qp_solve_backward_rows_f64 on settings, data, sol, gx, gu, act_tol, rank_tol;
 *   3. a grad whose fields are all NULL together with grad_x0 == NULL: SRBD_QP_EINVAL;
 *   4. batch == 0: SRBD_QP_OK.
 * A failed check launches and writes nothing.
 * Buffers: the backward buffer of srbd_qp_solve_backward_rows_f64 and the scratch rows of
 * srbd_qp_srbd_linearize_backward_f64, and between the lift kernel and the fused kernels a
 * compact buffer of capacity N (2 ng + (has_box_u ? nu : 0)) doubles -- nu and dnu of the rows,
 * the gradient of ubu -- allocated on first use (srbd_qp_memory_bytes counts it): 384 bytes per
 * stage with the cone against the 2304 of grad D, nothing on a handle without constraints.
 * Nothing of 144 or ng nu doubles per stage is written anywhere.
 * Asynchronous on `stream` like the two calls, under the contract of srbd_qp_solve_backward_f64.
 * Out of scope: gradients with respect to xs, us; the constants that are not per robot; the PLANT
 * role, the advance and the rollouts; active sets; fp32 and the mixed-precision settings;
 * srbd_qp_multi_* and the hpipm-cpp shim; state boxes, rows on the states and soft boxes
 * (rejected with the codes of the two calls).
 * ---------------------------------------------------------------------- */
int srbd_qp_srbd_solve_backward_f64(srbd_qp_handle h, int batch, const srbd_qp_settings* settings,
                                    const srbd_model_params* params, const srbd_plan_f64* plan /* may be NULL */,
                                    int constraints,
                                    const double* xs, const double* us,  /* the linearisation point          */
                                    const srbd_qp_data_f64* data,        /* what the linearisation wrote     */
                                    const srbd_qp_solution_f64* sol,     /* the forward x, u, pi (read only) */
                                    const double* gx, const double* gu,  /* cotangents; either may be NULL   */
                                    double act_tol, double rank_tol,
                                    const srbd_lin_grad_f64* grad,       /* the ten outputs, any may be NULL */
                                    double* grad_x0,                     /* [batch][12] = dpi[0]; may be NULL */
                                    void* stream);

/* ------------------------------------------------------------------------
 * Differentiable plant (additive to ABI 12): the open-loop rollout of the true robot and its
 * adjoint through time.  Nothing in the reference.  The forward call is the plant of the closed
 * loop without the controller around it: the inputs are data (a rollout's u_log, for instance),
 * so a logged trajectory can be replayed under other plant parameters, and the backward call
 * gives the gradient of any trajectory loss with respect to the start, the inputs, the feet, the
 * wrench, the mass and the inertia: what system identification from logs needs.
 * Forward, per robot: x_traj[0] = x0, and x_traj[t+1] is x_traj[t] after `substeps` classical RK4
 * steps of length dt / substeps of xdot = f(x, u[t]) + w[t], with f, the feet and w as in step 2
 * of srbd_qp_srbd_advance_f64 (w adds wrench[t][0:3] to rows 3..5 and wrench[t][3:6] / mass to
 * rows 9..11): the plant step of srbd_qp_srbd_advance_f64 without a contact model.  The input is
 * applied as it is.  Host statement: srbd_model.py's plant_step, tick by tick.
 * Mass and inertia are resolved per field as the plant step of srbd_qp_srbd_advance_f64 resolves
 * them: the handle's PLANT role, else its MODEL role, else params.
 * Neither call reads the handle's contact model, terrain or active set: they integrate the inputs
 * they are given (a rollout's u_log already holds the projected inputs), and with any of the three
 * set the results are the bits they are with it cleared.  So the frozen ticks of a fallen robot in
 * a log are not reproduced (the plant keeps integrating), and the true-ground foot height of a
 * contact model is the caller's to put into foot_r / foot_l.
 * Backward: the outputs are the gradients of a loss l with d l / d x_traj = gx, all T + 1 rows
 * (row 0 included: grad x0 = lambda_0 + gx[0]), by the adjoint recursion lambda_t = gx[t] +
 * (d x_traj[t+1] / d x_traj[t])' lambda_(t+1) with every RK4 step reversed slope by slope; the
 * substeps of a tick are recomputed from x_traj[t] (O(substeps^2) model evaluations per tick, no
 * buffer).  grad mass and grad Lbody are per robot whether or not a role supplies the value; grad
 * foot_r / foot_l have T dense rows whatever foot_stages is.  An output that is passed is fully
 * written; a NULL one costs nothing; with every output NULL the call does nothing.  The sums run
 * in a fixed order without atomics: the same inputs give the same bits, and an output has the
 * bits it has when the others are asked for too.
 * Both calls are asynchronous on `stream` (NULL = the handle's own stream), allocate no handle
 * memory (srbd_qp_memory_bytes does not grow), and take device memory only.  x0, roll->u, x_traj
 * and gx are accessed 16 bytes at a time and must be 16-byte aligned; the feet, the wrench and
 * the outputs of grad need only be 8-byte aligned.
 * Checks, in this order, before any device work:
 *   1. SRBD_QP_EINVAL: a NULL h, params, roll or x0 (backward: h, params, roll); a NULL x_traj
 *      (backward: also a NULL gx or grad); a NULL roll->u with ticks > 0; ticks < 0; substeps < 1;
 *      foot_stages < 0 or 0 < foot_stages < ticks;
 *   2. SRBD_QP_EDIM unless the handle has nx = nu = 12;
 *   3. SRBD_QP_ECAPACITY for a batch above the capacity;
 *   4. SRBD_QP_EINVAL for an x0, roll->u, x_traj or gx that is not 16-byte aligned;
 *   5. batch == 0: SRBD_QP_OK.
 * ticks == 0 writes x_traj[:, 0] = x0; the backward call then writes grad x0 = gx[:, 0] and
 * zeros to grad mass and grad Lbody.  A failed check launches and writes nothing.
 * Out of scope: the derivative of a contact model's projection, the gait rollout's internal
 * feet, a tick-parallel adjoint for small batches, fp32, srbd_qp_multi_* and the hpipm-cpp shim.
 * ---------------------------------------------------------------------- */
typedef struct srbd_plant_rollout_f64 {
  int ticks;            /* T >= 0 */
  int substeps;         /* RK4 steps per tick, each dt / substeps; >= 1 (as srbd_advance_f64) */
  int foot_stages;      /* rows per robot in foot_r / foot_l, >= T; 0 = T (a long plan's arrays pass as they are) */
  const double* u;      /* [batch][T][12] the inputs, each held over its tick (a rollout's u_log) */
  const double* foot_r; /* [batch][foot_stages][3], row t = the feet during tick t; NULL = params->foot_r */
  const double* foot_l; /* the same for the left foot; NULL = params->foot_l */
  const double* wrench; /* [batch][T][6], srbd_rollout_f64's layout; NULL = none */
} srbd_plant_rollout_f64;

int srbd_qp_srbd_plant_rollout_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                   const srbd_plant_rollout_f64* roll,
                                   const double* x0 /*[batch][12]*/, double* x_traj /*[batch][T+1][12]*/,
                                   void* stream);

typedef struct srbd_plant_grad_f64 {  /* device, outputs; any may be NULL and then costs nothing */
  double *x0;              /* [batch][12]    */
  double *u;               /* [batch][T][12] */
  double *foot_r, *foot_l; /* [batch][T][3] (dense T rows, whatever foot_stages is) */
  double *wrench;          /* [batch][T][6]  */
  double *mass;            /* [batch]        */
  double *Lbody;           /* [batch][3]     */
} srbd_plant_grad_f64;

int srbd_qp_srbd_plant_rollout_backward_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                            const srbd_plant_rollout_f64* roll,
                                            const double* x_traj /* the forward's output */,
                                            const double* gx /*[batch][T+1][12] dl/dx_traj */,
                                            const srbd_plant_grad_f64* grad, void* stream);

/* ------------------------------------------------------------------------
 * Gait planner (additive to ABI 12): the producer of a tick's plan window.  From a per-robot
 * velocity command, a per-robot gait (period, swing length and phase offset of each foot, in
 * stages) and the measured state it writes the window the step and the advance read
 * (srbd_plan_f64's four arrays for the handle's N), with Raibert foothold feedback: a swinging
 * foot's touchdown point follows the measured position and velocity until it lands.
 * Write (vx, vy, wz, zh) for the command, c = x[6:8], vm = x[9:11], dt = params->dt, Rz(a) for
 * the 2 x 2 rotation and (px, py, yaw) = ref_pose.  Per robot:
 *   Reference, k = 0..N:  yaw_k = yaw + k (dt wz);  p_0 = anchor ? c : (px, py),
 *     p_{k+1} = p_k + dt Rz(yaw_k)(vx, vy);
 *     x_ref[k] = (0, 0, yaw_k, 0, 0, Lz wz, p_k.x, p_k.y, zh, Rz(yaw_k)(vx, vy), 0), Lz the
 *     MODEL role's Lbody[2] where set (srbd_qp_srbd_set_robots_f64), else params->Lbody[2].
 *   Contact schedule, k = 0..N-1, foot f (0 right, 1 left), exact 64-bit integers:
 *     phi = (tick + k + offset_f) mod period; the foot swings at stage k iff phi < swing_f;
 *     fz_max[k][f] = swing ? fz_swing : fz_stance.
 *   Foothold of a touchdown at window stage j, with j' = min(j, N), S_f = period - swing_f:
 *     F_f(j).xy = c + (p_j' - p_0) + Rz(yaw_j')(hip_f + (S_f dt / 2)(vx, vy))
 *                 + k_raibert (vm - Rz(yaw_0)(vx, vy)),   F_f(j).z = ground_z.
 *   Foot rows: a swing stage k holds F_f(k + swing_f - phi), its next touchdown.  A stance
 *     stage k has s = k - (phi - swing_f), the first stage of that stance; with swing_f == 0 or
 *     s <= 0 the foot is already down and the stage holds foot_now[f]; otherwise F_f(s).
 *   State: foot_now[f] becomes row 0 of that foot's plan (a stance foot keeps its bits, a
 *     swinging foot's target follows the measured state until touchdown and is latched from
 *     then on); ref_pose becomes (p_1, yaw_1).
 * One call is one tick's planning step: issue it once per tick.  Asynchronous on `stream`
 * (NULL = the handle's own); all memory is device memory; the window's arrays must not
 * overlap the inputs.
 * Caller's contract (device data, not checked): the values of the _r arrays, in the ranges
 * the scalar fields are checked for.
 * Checks: a NULL pointer other than the three _r arrays, tick < 0, and, where the _r array is
 * NULL, period < 1, swing[f] outside [0, period) or offset[f] < 0 are SRBD_QP_EINVAL; so are
 * fz_swing <= 0 and fz_stance <= fz_swing; the handle needs nx = nu = 12 (SRBD_QP_EDIM);
 * batch above the capacity is SRBD_QP_ECAPACITY; batch == 0 returns SRBD_QP_OK.
 * Not per robot (out of scope): hip, the gains, fz_stance / fz_swing; swing-foot trajectories
 * (the model has no foot states).  Terrain height under a foothold: srbd_qp_srbd_set_terrain_f64.
 * ---------------------------------------------------------------------- */
typedef struct srbd_gait_f64 {
  int period, swing[2], offset[2];  /* in stages; every robot's where the arrays below are NULL */
  const int* period_r;              /* [batch]     device, optional */
  const int* swing_r;               /* [batch][2]  (right, left)    */
  const int* offset_r;              /* [batch][2]                   */
  double hip[2][2];                 /* (right, left) x (x, y): nominal foothold relative to the body, heading frame */
  double ground_z, k_raibert;       /* foothold height; velocity-error gain (s) */
  double fz_stance, fz_swing;       /* fz_max of a stance / swing stage; fz_swing small and positive */
  int anchor;                       /* 0: the carried reference position; 1: restart it from the measured xy each tick */
} srbd_gait_f64;

int srbd_qp_srbd_gait_plan_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                               const srbd_gait_f64* gait,
                               const double* cmd,      /* [batch][4]  vx, vy (heading frame), wz, body height */
                               const double* x,        /* [batch][12] measured state */
                               long long tick,
                               double* ref_pose,       /* [batch][3]  px, py, yaw: in/out */
                               double* foot_now,       /* [batch][2][3] where each foot stands or is heading: in/out */
                               double* x_ref, double* foot_r, double* foot_l, double* fz_max,  /* the window, out */
                               void* stream);

typedef struct srbd_rollout_gait_f64 {
  const double* cmd;     /* [batch][T][4]  the command of every tick (may be NULL when T == 0) */
  double* ref_pose;      /* [batch][3]     in/out, as srbd_qp_srbd_gait_plan_f64            */
  double* foot_now;      /* [batch][2][3]  in/out                                           */
  long long tick0;       /* tick t plans with tick0 + t; >= 0                               */
  double* foot_log;      /* [batch][T][2][3] optional: row 0 of each tick's feet            */
  double* fz_log;        /* [batch][T][2]    optional: row 0 of each tick's fz_max          */
} srbd_rollout_gait_f64;

/* srbd_qp_srbd_rollout_f64 that replans every tick: the plan is replaced by the gait and its
 * io.  For t = 0..T-1: (1) the planner runs with cmd[:, t], the current x and tick0 + t and
 * writes W_t into the handle's plan-window scratch (the buffer of a rollout with a full plan,
 * the same size); (2)-(6) are srbd_qp_srbd_rollout_f64's, with foot_log[:, t] / fz_log[:, t] =
 * row 0 of W_t among the logs.  roll->plan_stages is ignored.  The results are the bits of a
 * caller's loop over srbd_qp_srbd_gait_plan_f64, srbd_qp_srbd_nmpc_plan_f64 and
 * srbd_qp_srbd_advance_f64.  Checks: the planner's and the rollout's; ticks == 0 or
 * batch == 0 plan nothing.  A failed check leaves every array as it was.               */
int srbd_qp_srbd_rollout_gait_f64(srbd_qp_handle h, int batch, const srbd_model_params* params,
                                  const srbd_gait_f64* gait, const srbd_rollout_gait_f64* gio,
                                  const srbd_linesearch_params* ls, const srbd_qp_settings* settings,
                                  int constraints, int sqp_max_loop, const srbd_rollout_f64* roll,
                                  double* xs, double* us, double* x, double* alpha);

/* ------------------------------------------------------------------------
 * Terrain (additive to ABI 12): a shared set of height maps under the gait planner, with a
 * per-robot map index, so that one batch walks slopes, stairs and rough ground.  It attaches
 * to the handle; srbd_qp_srbd_gait_plan_f64 and srbd_qp_srbd_rollout_gait_f64 issued afterwards
 * on that handle read it.  The call copies the struct and does no device work; the arrays are
 * device memory read by the launched kernels: keep them alive and unchanged until those have
 * finished.  terrain == NULL, or a NULL height, clears it; with the terrain cleared the
 * planner is what it is without this entry point: the same kernel code, the same bits.
 * Height of map m at (x, y), clamped bilinear, H = height + m ny nx:
 *   s = (x - x0) / cell, clamped to [0, nx - 1];  i = min(floor(s), nx - 2),  a = s - i;
 *   t = (y - y0) / cell, clamped to [0, ny - 1];  j = min(floor(t), ny - 2),  b = t - j;
 *   h = (1 - b)((1 - a) H[j][i] + a H[j][i+1]) + b ((1 - a) H[j+1][i] + a H[j+1][i+1]).
 *   Outside the grid the edge value extends.
 * The planner with a terrain set, robot r on map m = map_r[r] (everything not named here is
 * the gait planner's definition above):
 *   Reference height: x_ref[k][8] = zh + h(p_k), k = 0..N; the other entries are unchanged.
 *   Foothold of a touchdown: n = the planner's F_f(j).xy, the nominal foothold.  Candidates
 *     d = (di, dj), |di|, |dj| <= search, with index q = (dj + search)(2 search + 1) + (di + search)
 *     and position c_d = n + cell (di, dj).  Roughness rho(c) = the largest of
 *     |h(c +- cell e_x) - h(c)| and |h(c +- cell e_y) - h(c)|;  cost
 *     J_d = cell^2 (di^2 + dj^2) + w_rough rho(c_d)^2.  The chosen d* has the smallest J, ties
 *     go to the smallest q.  F_f(j).xy = c_d*,  F_f(j).z = ground_z + h(c_d*).  With search == 0
 *     no roughness is evaluated and F.xy has the bits of n.
 *   Rows and state: which rows hold foot_now and which hold F_f of which touchdown stays as it
 *     is, and so do the latch and ref_pose: a foot in stance keeps the height it landed on, bit
 *     for bit; a swinging foot's target, z included, is recomputed every tick.
 * Caller's contract (device data, not checked): map_r's values in [0, maps), finite heights.
 * Checks: NULL handle, maps < 1, nx or ny < 2, cell not > 0, search outside 0..3, w_rough < 0
 * or not finite, x0 or y0 not finite are SRBD_QP_EINVAL; a handle without nx = nu = 12 is
 * SRBD_QP_EDIM.
 * Out of scope: the ground under the plant (that is the contact model's own true ground,
 * srbd_qp_srbd_set_contact_f64), swing clearance and swing trajectories, a vertical-velocity or tilt reference on
 * slopes, one private map per robot (the map index covers it), srbd_qp_multi_*, the
 * hpipm-cpp shim, fp32.
 * ---------------------------------------------------------------------- */
typedef struct srbd_terrain_f64 {
  const double* height;  /* device, [maps][ny][nx]; sample (j, i) lies at (x0 + i cell, y0 + j cell) */
  int maps, nx, ny;      /* maps >= 1; nx, ny >= 2 */
  double x0, y0, cell;   /* cell > 0 */
  const int* map_r;      /* device [batch], optional: robot i's map in [0, maps); NULL = map 0 */
  int search;            /* 0..3: foothold candidates within +-search cells of the nominal one */
  double w_rough;        /* >= 0: weight of the local roughness in the candidate's cost */
} srbd_terrain_f64;
int srbd_qp_srbd_set_terrain_f64(srbd_qp_handle h, const srbd_terrain_f64* terrain);

/* The public sampler: out[i] = the height of map[i] (NULL: map 0) at xy[i], the formula above.
 * Asynchronous on `stream` (NULL = the handle's own); xy, map, out are device memory.  Caller's
 * contract: map's values in [0, maps), finite coordinates.  Checks: a NULL handle, no terrain
 * set, n < 0 and, for n > 0, a NULL xy or out are SRBD_QP_EINVAL; n == 0 returns SRBD_QP_OK. */
int srbd_qp_srbd_terrain_height_f64(srbd_qp_handle h, int n, const double* xy /*[n][2]*/,
                                    const int* map /*[n], NULL = 0*/, double* out /*[n]*/, void* stream);

/* ------------------------------------------------------------------------
 * Contact model and fall detection (additive to ABI 12): what the plant of
 * srbd_qp_srbd_advance_f64, and so of both rollouts, does to the commanded input before it
 * integrates it, and what it reports per robot.  Without a contact the plant applies us[0] as it
 * is; with one, a foot can only push, only while the schedule has it on the ground, only inside
 * the TRUE friction cone and moment limits, and it stands on the TRUE ground, which may differ
 * from the map the planner believes in (srbd_qp_srbd_set_terrain_f64).  A fall detector freezes
 * fallen robots and counts the plant steps each robot survived.
 * The call attaches to the handle like set_robots / set_terrain: it copies the struct and does
 * no device work; contact == NULL clears it, and with the contact cleared every call launches
 * the kernels it launched before and gives the same bits.  It is read by the plant step of
 * srbd_qp_srbd_advance_f64, srbd_qp_srbd_rollout_f64 and srbd_qp_srbd_rollout_gait_f64 issued
 * afterwards, and by nothing else: the controller (linearisation, line search, NMPC step, the
 * model step that makes the new xs[N]) never sees it.  A call without a plant state (x == NULL:
 * shift only) does not read it either.  The arrays are device memory with at least `batch`
 * rows, read and written by the launched kernels: keep them alive until those have finished.
 *
 * Plant step of robot i with a contact set (step 2 of srbd_qp_srbd_advance_f64), with u = us[0],
 * clamp(v, lo, hi) = fmin(fmax(v, lo), hi), mu_i = mu_r ? mu_r[i] : mu, and u' the applied input
 * (u_applied, the rollout's u_log):
 *  1. Already fallen (fallen != NULL and fallen[i] != 0 on entry): x keeps its bits, u' is
 *     twelve zeros, alive[i] and sat[i] are unchanged.  The shift of xs / us runs as always.
 *  2. Non-finite input: if any of the twelve entries of u is not finite the robot falls now:
 *     fallen[i] = 1 (when given), x keeps its bits, u' is twelve zeros, alive[i] and sat[i] are
 *     unchanged.  (With fallen == NULL finite inputs are the caller's contract.)
 *  3. Contact flags: foot f (0 right, 1 left) is in contact, c_f, iff the plan's
 *     fz_max[0][f] > fz_contact; without a plan, or with plan->fz_max == NULL, both feet are.
 *  4. Projection, per foot f (o = 6 f), each bound ONE multiplication, nothing fused:
 *       fz'    = c_f ? clamp(u[o+2], 0, fz_hi) : 0
 *       b      = mu_i * fz'
 *       fx'    = clamp(u[o], -b, b),   fy' = clamp(u[o+1], -b, b)
 *       tau_a' = clamp(u[o+3+a], -(Lt_a * fz'), Lt_a * fz')   for a = x, y, z (Ltx, Lty, Ltz)
 *     (the sign of a zero result is not specified).
 *  5. sat: bit 4 f + kind is OR-ed into sat[i] iff the projected values of that group differ
 *     (!=) from the commanded ones:
 *       kind 0  fz' != u[o+2] and (not c_f, or fz' > u[o+2]): raised to 0, or zeroed by swing
 *       kind 1  c_f and fz' < u[o+2]: lowered to fz_hi
 *       kind 2  fx' != u[o] or fy' != u[o+1]
 *       kind 3  tau_a' != u[o+3+a] for some a
 *  6. Feet: with ground.height set, a foot in contact stands at (planned x, planned y,
 *     ground_z + h_true(x, y)), h_true the clamped bilinear of srbd_terrain_f64 above on map
 *     ground.map_r[i] (NULL: map 0); a foot not in contact, and every foot without
 *     ground.height, stays at the planned point (the plan's stage 0, or params->foot_*).
 *  7. Integration: x <- the `substeps` RK4 steps of srbd_qp_srbd_advance_f64 with u', those feet,
 *     the wrench, and the PLANT role's mass and inertia.
 *  8. Fall test on the new state, only when fallen is given.  The robot falls (fallen[i] = 1) if
 *       any entry of x is not finite -- then x keeps its bits of before the step; or
 *       x[8] - (ground_z + h_true(x[6], x[7])) < z_min   (h_true = 0 without ground.height); or
 *       expm(x[0:3])[2][2] < cos_tilt_min.
 *     A robot that falls on a finite state keeps that state.  alive[i] += 1 iff the robot is
 *     not fallen after this step.
 * Checks: a NULL handle; mu negative or not finite where mu_r is NULL; an Lt* negative or not
 * finite; fz_hi NaN or <= 0 (+inf is allowed); fz_contact negative or not finite; ground_z or
 * z_min not finite; cos_tilt_min outside [-1, 1]; alive without fallen; and, with ground.height
 * given, set_terrain's checks of maps, nx, ny, cell, x0, y0 are SRBD_QP_EINVAL; a handle
 * without nx = nu = 12 is SRBD_QP_EDIM.  ground.search / ground.w_rough are ignored.
 * Caller's contract (device data, not checked): mu_r finite and >= 0, map indices in range.
 * Out of scope: feet that slide when friction saturates (the foot stays where the plan put it);
 * any body-ground collision; re-arming a fallen robot inside a rollout (the caller resets x and
 * fallen between rollouts); srbd_qp_multi_*, the hpipm-cpp shim, fp32.  (Whether the NMPC step
 * still runs for a fallen robot is srbd_active_f64.skip_fallen's choice, below.)
 * ---------------------------------------------------------------------- */
typedef struct srbd_contact_f64 {
  double mu;              /* plant friction coefficient of every robot where mu_r is NULL      */
  const double* mu_r;     /* device [batch], optional                                          */
  double Ltx, Lty, Ltz;   /* |tau_a| <= Lt_a * fz per foot; the model's own rows are (0, Lfx, Lfz) */
  double fz_hi;           /* largest normal force a foot in contact can take; > 0, +inf allowed */
  double fz_contact;      /* foot f is in contact this tick iff the plan's fz_max[0][f] > fz_contact;
                             without a plan or without fz_max both feet are in contact          */
  double ground_z;        /* as srbd_gait_f64.ground_z                                          */
  srbd_terrain_f64 ground;/* the TRUE ground; height == NULL: flat at ground_z and the feet keep
                             their planned z.  search / w_rough are ignored.                    */
  double z_min;           /* fall: body height above the true ground under it < z_min           */
  double cos_tilt_min;    /* fall: expm(x[0:3])[2][2] < cos_tilt_min                            */
  int* fallen;            /* device [batch] in/out, optional; NULL = no fall detection          */
  int* alive;             /* device [batch] in/out, optional (needs fallen): plant steps survived */
  unsigned* sat;          /* device [batch] in/out, optional: OR of the limits that were active */
} srbd_contact_f64;
int srbd_qp_srbd_set_contact_f64(srbd_qp_handle h, const srbd_contact_f64* contact);

/* ------------------------------------------------------------------------
 * Active sets (additive to ABI 12): which robots of the batch an NMPC step steps, and whether
 * its SQP iterations are launched over the robots that still iterate only.  Without one, every
 * SQP iteration linearises and solves the whole batch until the slowest robot has converged: a
 * step costs (largest sqp_iter) x batch QP solves where sum_i sqp_iter[i] are needed.
 * The call attaches to the handle like set_robots / set_terrain / set_contact: it copies the
 * struct and does no device work; active == NULL, or a struct with mask == NULL, skip_fallen == 0
 * and compact == 0, clears it, and with it cleared every call launches the kernels it launched
 * before and gives the same bits.  It is read by the NMPC step only: srbd_qp_srbd_nmpc_f64,
 * srbd_qp_srbd_nmpc_plan_f64 and so both rollouts.  The advance, the planner, the plain
 * linearisation and line search and the solves do not read it.  mask is device memory with at
 * least `batch` rows, read when the step starts: keep it alive until the step has returned.
 *
 * Robot i is active in a step iff, when the step starts, (mask == NULL or mask[i] != 0) and
 * (skip_fallen == 0 or contact.fallen[i] == 0), contact the handle's srbd_contact_f64.  This is
 * the only place where the controller reads anything of the contact model, and it reads fallen
 * only.  A robot that is not active: xs, us and alpha keep their bits, sqp_iter[i] = 0 and
 * converged[i] = 0.  In a rollout the advance runs for it as always (the shift happens; a fallen
 * robot's plant is frozen) and the logs hold those zeros for that tick.
 *
 * compact == 0: the kernels and launch shapes of a step without an active set; a robot that is
 * not active rides along as a robot does whose loop has stopped.  An active robot gets the bits
 * it gets without an active set.
 * compact == 1: SQP iteration `it` builds the QPs of the n_it robots still iterating as a dense
 * batch of n_it, in ascending robot order, solves that batch with srbd_qp_solve_f64 and
 * line-searches those robots; with n_0 == 0 the call returns after the selection.  A robot's
 * result is what the solve gives its QP in a batch of n_it: bit-identical to compact == 0 wherever
 * the solve's kernel choice is the same for n_it and for `batch`.  That holds for
 * SRBD_QP_SRBD_NONE at any size: the step solves the n_it QPs with the Riccati kernel the whole
 * batch takes (the streaming kernel also for the few QPs left of a batch of more than 256, where
 * srbd_qp_solve_f64 on its own would take the single-QP kernels, which sum in another order),
 * and a Riccati solve of a subset has the full batch's bits.  For BOX_U and CONE it holds while
 * n_it and `batch` lie on the same side of the latency IPM's limit (512 QPs).  Across that
 * limit the stragglers are solved by the latency IPM, the faster kernel for few QPs, and the two
 * settings agree to the solver's tolerance, not to the bit.
 * The step costs one more 4-byte read-back (the count of active robots) when an active set is
 * attached, and two index lists of `capacity` ints in its scratch.
 *
 * Checks.  At set time: a NULL handle, skip_fallen or compact not 0 or 1: SRBD_QP_EINVAL; a
 * handle without nx = nu = 12: SRBD_QP_EDIM.  At the step or rollout, before any device work
 * (every array is left as it was): skip_fallen without a contact on the handle, or with a contact
 * whose fallen is NULL: SRBD_QP_EINVAL; compact == 1 with settings->warm_start != 0:
 * SRBD_QP_EINVAL (the warm start reads the previous iterate at the QP's position, which under
 * compaction belongs to another robot).
 * Out of scope: compaction with an IPM warm start; a step without read-backs; skipping the
 * planner or the advance of a robot that is not active; srbd_qp_multi_*, the hpipm-cpp shim, fp32.
 * ---------------------------------------------------------------------- */
typedef struct srbd_active_f64 {
  const int* mask;   /* device [batch], optional: robot i is stepped iff mask[i] != 0; NULL = all  */
  int skip_fallen;   /* 1: a robot with contact.fallen[i] != 0 when the step starts is not stepped */
  int compact;       /* 0: full-batch launches (a robot that is not stepped rides along);
                        1: every SQP iteration is launched over the robots still iterating only   */
} srbd_active_f64;
int srbd_qp_srbd_set_active_f64(srbd_qp_handle h, const srbd_active_f64* active);
/* The work of the last NMPC step on this handle (of a rollout: summed over its ticks), host
 * counters that are always kept: *sqp_iterations the SQP loop iterations that ran, *qp_solves the
 * sum over them of the batch size passed to the solve -- iterations x batch without compaction,
 * and exactly sum_i sqp_iter[i] with compact == 1.  Either pointer may be NULL; a NULL handle is
 * SRBD_QP_EINVAL. */
int srbd_qp_srbd_step_work(srbd_qp_handle h, long long* qp_solves, long long* sqp_iterations);

/* ------------------------------------------------------------------------
 * One solver over several devices, driven from one host thread (SURVEY.md 5,
 * "one process, 8 devices"; BASELINE config 4: a batch sharded over 8 MI355X
 * with the solutions gathered to one device).  A handle per device; the
 * shards' solves are all queued before any is waited for, and x, u, pi are
 * gathered to the root device (devices[0]) by peer copies over xGMI, each
 * behind its shard's solve on that shard's stream.  (ABI 10)
 * ---------------------------------------------------------------------- */
typedef struct srbd_qp_multi_s* srbd_qp_multi;

/* A handle of `capacity_per_device` QPs on each of devices[0..ndev) (a device
 * may repeat: two shards on one GPU).  Peer access root <-> shard is enabled
 * where the devices support it.                                              */
int srbd_qp_multi_create(const srbd_qp_dims* dims, int capacity_per_device, const int* devices,
                         int ndev, srbd_qp_multi* out);
void srbd_qp_multi_destroy(srbd_qp_multi m);
/* Shard i's handle (its stream, workspace size, ...); NULL past the end.    */
srbd_qp_handle srbd_qp_multi_handle(srbd_qp_multi m, int i);
/* Shard i: batch[i] QPs with data[i] / sol[i] in devices[i]'s memory.  Every
 * shard is solved with `settings`; then, when root_x / root_u / root_pi are
 * given (root-device memory for sum(batch) QPs, the C-ABI layout), the shards'
 * x, u, pi land there in shard order.  Returns when all of it has finished. */
int srbd_qp_multi_solve_f64(srbd_qp_multi m, const int* batch, const srbd_qp_settings* settings,
                            const srbd_qp_data_f64* data, const srbd_qp_solution_f64* sol,
                            double* root_x, double* root_u, double* root_pi);
/* The fp32 twin (BASELINE config 5 sharded; HPIPM's s_ocp_qp_ipm), the same
 * contract with srbd_qp_solve_f32 on every shard.  (ABI 11)                   */
int srbd_qp_multi_solve_f32(srbd_qp_multi m, const int* batch, const srbd_qp_settings* settings,
                            const srbd_qp_data_f32* data, const srbd_qp_solution_f32* sol,
                            float* root_x, float* root_u, float* root_pi);

/* Blocks until all work queued on the handle's stream is done.            */
int srbd_qp_synchronize(srbd_qp_handle h);

/* The handle's hipStream_t (for event timing / stream interop).           */
void* srbd_qp_stream(srbd_qp_handle h);

/* Device workspace bytes the handle holds.                                */
size_t srbd_qp_workspace_bytes(srbd_qp_handle h);

/* Every byte the handle holds right now: the workspace plus the buffers it
 * allocates on first use (host-solve staging and its pinned host mirror, the
 * 12 x 12 embedding, the NMPC loop state, the rollout's plan window, the
 * f64_rescue / f32_iters batches).  A pool of handles (hpipm-cpp's, which re-implements the
 * reference's construct-per-solve pattern, NMPC_solver.cpp:318-319) sizes
 * itself by this.  (ABI 9)                                                  */
size_t srbd_qp_memory_bytes(srbd_qp_handle h);

void srbd_qp_destroy(srbd_qp_handle h);

/* "HpipmStatus::Success" ... like hpipm::to_string (ocp_qp_ipm_solver.cpp:19-33) */
const char* srbd_qp_status_string(int status);
const char* srbd_qp_error_string(int err);
/* Message of the last error raised on this thread (never NULL).           */
const char* srbd_qp_last_error(void);

int srbd_qp_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SRBD_QP_H_ */
