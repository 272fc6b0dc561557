"""TEST INFRASTRUCTURE ONLY -- the host closed loop the device rollout
(srbd_qp_srbd_rollout_f64) is compared against: per tick the host SQP loop of
tests/nmpc_plan_host.py on the tick's plan window, then srbd_model.plant_step and
srbd_model.shift_guess, in the order include/srbd_qp.h states."""
from __future__ import annotations

import numpy as np

import nmpc_plan_host as PH

__all__ = ["window", "closed_loop", "walking_case"]

FIELDS = ("x_ref", "foot_r", "foot_l", "fz_max")


def window(sm, plan, t, N):
    """Stages t .. t + N of a long plan (arrays [B][P+1][12] / [B][P][3] / [B][P][2]): x_ref rows
    t .. t + N, feet and fz_max rows t .. t + N - 1; None fields stay None, None stays None."""
    if plan is None:
        return None
    return sm.SrbdPlan(**{k: (None if getattr(plan, k) is None
                              else np.ascontiguousarray(getattr(plan, k)[:, t:t + N + (k == "x_ref")]))
                          for k in FIELDS})


def closed_loop(sm, oracle, p, plan, xs, us, x, alpha, ticks, settings, sqp_max_loop,
                constraints="none", wrench=None, substeps=1, alpha_reset=0.0):
    """`ticks` ticks from the guess xs [B][N+1][12], us [B][N][12], the plant state x [B][12] and
    alpha [B] under the long plan (None: none) and wrench [B][ticks][6] (None: none).
    Returns a dict: x_log [B][ticks+1][12], u_log [B][ticks][12], sqp_iter / converged [B][ticks],
    xs / us (the shifted guess for the next tick), x, alpha, margin (the smallest comparison
    margin of all line searches) and steps (per tick, per robot, what sqp_loop returned)."""
    B, N = us.shape[0], us.shape[1]
    xs, us, x = xs.copy(), us.copy(), x.copy()
    alpha = np.array(alpha, dtype=np.float64)
    x_log = np.empty((B, ticks + 1, 12))
    u_log = np.empty((B, ticks, 12))
    it_log = np.zeros((B, ticks), dtype=np.int32)
    cv_log = np.zeros((B, ticks), dtype=np.int32)
    x_log[:, 0] = x
    margin, steps = np.inf, []
    for t in range(ticks):
        w = window(sm, plan, t, N)
        if alpha_reset > 0.0:
            alpha[:] = alpha_reset
        res = [PH.sqp_loop(sm, oracle, p, None if w is None else w.robot(i), xs[i], us[i], x[i],
                           float(alpha[i]), settings, sqp_max_loop, constraints) for i in range(B)]
        steps.append(res)
        xs = np.stack([r[0] for r in res])
        us = np.stack([r[1] for r in res])
        alpha = np.array([r[2] for r in res], dtype=np.float64)
        it_log[:, t] = [r[3] for r in res]
        cv_log[:, t] = [int(r[4]) for r in res]
        margin = min([margin] + [r[5] for r in res])
        u0 = us[:, 0].copy()
        x = sm.plant_step(x, u0, p, None if w is None or w.foot_r is None else w.foot_r[:, 0],
                          None if w is None or w.foot_l is None else w.foot_l[:, 0],
                          None if wrench is None else wrench[:, t], substeps)
        xs, us = sm.shift_guess(xs, us, p, w)
        u_log[:, t] = u0
        x_log[:, t + 1] = x
    return dict(x_log=x_log, u_log=u_log, sqp_iter=it_log, converged=cv_log, xs=xs, us=us, x=x,
                alpha=alpha, margin=margin, steps=steps)


def walking_case(sm, p, B, N, T, seed):
    """B robots walking for N + T - 1 plan stages, after tests/test_gpu_plan.py's walking_batch:
    each with its own velocity command (a reference that moves at that velocity) and stepping
    pattern (each foot swinging -- fz_max = 1 -- for five stages, then set down ahead along the
    command), from perturbed starts.  Returns (xs, us, x, alpha, long plan)."""
    rng = np.random.default_rng(seed)
    P = N + T - 1
    xs, us, dx0 = sm.sample_trajectories(B, N, seed, p)
    x = xs[:, 0] + dx0
    k = np.arange(P + 1)
    x_ref = np.tile(np.array(p.x_ref, dtype=np.float64), (B, P + 1, 1))
    foot_r = np.tile(np.array(p.foot_r, dtype=np.float64), (B, P, 1))
    foot_l = np.tile(np.array(p.foot_l, dtype=np.float64), (B, P, 1))
    fz = np.empty((B, P, 2))
    for i in range(B):
        v = rng.uniform(-0.3, 0.3, size=2)  # commanded (vx, vy)
        x_ref[i, :, 6:8] += np.outer(k * p.dt, v)
        x_ref[i, :, 9:11] = v
        x_ref[i] += rng.uniform(-0.01, 0.01, size=(P + 1, 12))
        fz[i] = rng.uniform(150.0, 300.0, size=(P, 2))
        s0 = int(rng.integers(1, 4))  # right foot swings s0 .. s0+4, left s0+6 .. s0+10
        step = 10.0 * p.dt * v
        for foot, lo in ((0, s0), (1, s0 + 6)):
            f = foot_r if foot == 0 else foot_l
            fz[i, lo:lo + 5, foot] = 1.0
            f[i, lo + 5:, 0:2] += step  # set down ahead
            f[i] += rng.uniform(-0.005, 0.005, size=(P, 3))
    plan = sm.SrbdPlan(x_ref=x_ref, foot_r=foot_r, foot_l=foot_l, fz_max=fz)
    alpha = np.where(np.arange(B) % 4 == 1, 0.5, 1.0)
    return xs, us, x, alpha, plan
