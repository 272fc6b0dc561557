"""TEST INFRASTRUCTURE ONLY -- the host closed loop, the one statement of the loop
include/srbd_qp.h describes, that every device rollout (srbd_qp_srbd_rollout_f64,
srbd_qp_srbd_rollout_gait_f64, with or without robots, terrain and a contact on the handle) is
compared against.  Per tick: the plan window (a long plan's stages, or srbd_model.gait_plan from
the measured state), the host SQP loop of tests/nmpc_plan_host.py per robot on that window, then
srbd_model.plant_step and srbd_model.shift_guess.  Next to it the per-robot wrappers: the host
model called once per robot with that robot's SrbdParams."""
from __future__ import annotations

import dataclasses

import numpy as np

import contact_host as CH
import nmpc_plan_host as PH
import terrain_host as TH

__all__ = ["FIELDS", "window", "sqp_loops", "plant_step", "shift_guess", "robot_contact", "closed_loop",
           "start", "feet_plan", "walking_case"]

FIELDS = ("x_ref", "foot_r", "foot_l", "fz_max")


def window(sm, plan, t, N):
    """Stages t .. t + N of a long plan (arrays [B][P+1][12] / [B][P][3] / [B][P][2]): x_ref rows
    t .. t + N, feet and fz_max rows t .. t + N - 1; None fields stay None, None stays None."""
    if plan is None:
        return None
    return sm.SrbdPlan(**{k: (None if getattr(plan, k) is None
                              else np.ascontiguousarray(getattr(plan, k)[:, t:t + N + (k == "x_ref")]))
                          for k in FIELDS})


# ---- per robot: `params` is one SrbdParams for every robot, or a list of one per robot ----
def _per_robot(params):
    return isinstance(params, (list, tuple))


def _batch_of_one(sm, plan, i):
    if plan is None:
        return None
    return sm.SrbdPlan(*[None if getattr(plan, k) is None else getattr(plan, k)[i:i + 1] for k in FIELDS])


def robot_contact(contact, i):
    """The contact of a batch that holds robot i alone (mu_r and the true ground's map_r sliced)."""
    g = contact.ground
    if g is not None and g.map_r is not None:
        g = dataclasses.replace(g, map_r=np.asarray(g.map_r)[i:i + 1])
    return dataclasses.replace(contact, mu_r=None if contact.mu_r is None else np.asarray(contact.mu_r)[i:i + 1],
                               ground=g)


def sqp_loops(sm, oracle, params, plan, xs, us, x0, alpha, settings, sqp_max_loop, constraints):
    """PH.sqp_loop per robot: a list of its return tuples."""
    each = params if _per_robot(params) else [params] * xs.shape[0]
    return [PH.sqp_loop(sm, oracle, q, None if plan is None else plan.robot(i), xs[i], us[i], x0[i], float(alpha[i]),
                        settings, sqp_max_loop, constraints) for i, q in enumerate(each)]


def plant_step(sm, params, x, u, foot_r=None, foot_l=None, wrench=None, substeps=1, contact=None, in_contact=None,
               state=None):
    """srbd_model.plant_step: on the whole batch with one SrbdParams, robot by robot with a list
    (the PLANT role).  Returns what it returns: x', or (x', u', state') with a contact."""
    if not _per_robot(params):
        return sm.plant_step(x, u, params, foot_r, foot_l, wrench, substeps, contact=contact, in_contact=in_contact,
                             state=state)
    assert len(params) == x.shape[0]
    state = {k: np.array(v) for k, v in (state or {}).items()}
    xo, uo = np.empty_like(x), np.empty_like(u)
    for i, q in enumerate(params):
        one = lambda a: None if a is None else np.asarray(a)[i:i + 1]
        out = sm.plant_step(x[i:i + 1], u[i:i + 1], q, one(foot_r), one(foot_l), one(wrench), substeps,
                            contact=None if contact is None else robot_contact(contact, i), in_contact=one(in_contact),
                            state={k: v[i:i + 1] for k, v in state.items()})
        if contact is None:
            xo[i:i + 1] = out
            continue
        xo[i:i + 1], uo[i:i + 1], st = out
        for k in state:
            state[k][i] = st[k][0]
    return xo if contact is None else (xo, uo, state)


def shift_guess(sm, params, xs, us, plan=None):
    """srbd_model.shift_guess: on the whole batch with one SrbdParams, robot by robot with a list
    (the MODEL role)."""
    if not _per_robot(params):
        return sm.shift_guess(xs, us, params, plan)
    parts = [sm.shift_guess(xs[i:i + 1], us[i:i + 1], q, _batch_of_one(sm, plan, i))
             for i, q in enumerate(params)]
    return np.concatenate([a for a, _ in parts], axis=0), np.concatenate([b for _, b in parts], axis=0)


# ---- the loop ----
def closed_loop(sm, oracle, xs, us, x, alpha, ticks, settings, sqp_max_loop, constraints="none", *, p=None,
                model=None, plant=None, plan=None, gait=None, cmd=None, ref_pose=None, foot_now=None, tick0=0,
                terrain=None, wrench=None, substeps=1, contact=None, state=None, alpha_reset=0.0):
    """`ticks` ticks from the guess xs [B][N+1][12], us [B][N][12], the plant state x [B][12] and
    alpha [B].

    Parameters: p, one SrbdParams for every robot (the model is then called on the whole batch);
    or model and plant, lists of one SrbdParams per robot (called robot by robot): the SQP loop,
    the planner's Lbody z and the new last stage of the guess use model[i], the plant step plant[i].
    Window: plan, a long plan windowed with window(); or gait with cmd [B][ticks][4], ref_pose
    [B][3], foot_now [B][2][3] and tick0, then srbd_model.gait_plan runs every tick from the
    measured state, on `terrain` if given; neither: no plan.
    Plant: wrench [B][ticks][6] (None: none), substeps, and contact with state (the fallen / alive
    / sat arrays on entry; None: zero_state): then the plant step is plant_step(contact=...) with
    the contact flags of the window's fz_max row 0, and u_log holds the applied input.

    Returns a dict: x_log [B][ticks+1][12], u_log [B][ticks][12], sqp_iter / converged [B][ticks],
    xs / us (the shifted guess for the next tick), x, alpha, margin (the smallest comparison
    margin of all line searches) and steps (per tick, per robot, what sqp_loop returned).  With a
    gait also foot_log [B][ticks][2][3], fz_log [B][ticks][2], ref_pose, foot_now and windows (each
    tick's SrbdPlan); with terrain q_log [B][ticks][2] (the chosen candidate of row 0's touchdown,
    -1 for a foot that is down), select_margin (the smallest best-to-second-best cost gap over
    every touchdown of every tick) and poses / feet (ref_pose and foot_now after each tick's
    planning step); with a contact state (after the last tick), fallen_log [B][ticks] (fallen
    after each tick) and values (per tick, fall_values of the new states)."""
    B, N = us.shape[0], us.shape[1]
    if (p is None) == (model is None) or (model is None) != (plant is None):
        raise ValueError("parameters: p, or model and plant")
    if plan is not None and gait is not None:
        raise ValueError("window: plan or gait, not both")
    if terrain is not None and gait is None:
        raise ValueError("terrain goes with gait")
    believed, true = (p, p) if model is None else (model, plant)
    # the planner reads dt and Lbody z: the MODEL role's, robot by robot
    p_plan, Lz = (p, None) if model is None else (model[0], np.array([m.Lbody[2] for m in model]))
    xs, us, x = xs.copy(), us.copy(), x.copy()
    alpha = np.array(alpha, dtype=np.float64)
    x_log = np.empty((B, ticks + 1, 12))
    u_log = np.empty((B, ticks, 12))
    it_log = np.zeros((B, ticks), dtype=np.int32)
    cv_log = np.zeros((B, ticks), dtype=np.int32)
    x_log[:, 0] = x
    margin, steps = np.inf, []
    if gait is not None:
        ref_pose, foot_now = np.array(ref_pose, dtype=np.float64), np.array(foot_now, dtype=np.float64)
        foot_log, fz_log = np.empty((B, ticks, 2, 3)), np.empty((B, ticks, 2))
        q_log = np.empty((B, ticks, 2), dtype=np.int64)
        select_margin, windows, poses, feet = np.inf, [], [], []
    if contact is not None:
        state = CH.zero_state(B) if state is None else {k: np.array(v) for k, v in state.items()}
        fallen_log = np.zeros((B, ticks), dtype=np.int32)
        values = []
    for t in range(ticks):
        if gait is None:
            w = window(sm, plan, t, N)
        else:
            if terrain is not None:
                q, m, _, _ = TH.selection(sm, p_plan, gait, terrain, cmd[:, t], x, tick0 + t, ref_pose, foot_now, N)
                q_log[:, t], select_margin = q[:, 0], min(select_margin, m)
            w, ref_pose, foot_now = sm.gait_plan(p_plan, gait, cmd[:, t], x, tick0 + t, ref_pose, foot_now, N,
                                                 Lbody_z=Lz, terrain=terrain)
            windows.append(w)
            poses.append(ref_pose)
            feet.append(foot_now)
            foot_log[:, t, 0], foot_log[:, t, 1], fz_log[:, t] = w.foot_r[:, 0], w.foot_l[:, 0], w.fz_max[:, 0]
        if alpha_reset > 0.0:
            alpha[:] = alpha_reset
        res = sqp_loops(sm, oracle, believed, w, xs, us, x, alpha, settings, sqp_max_loop, constraints)
        steps.append(res)
        xs = np.stack([r[0] for r in res])
        us = np.stack([r[1] for r in res])
        alpha = np.array([r[2] for r in res], dtype=np.float64)
        it_log[:, t] = [r[3] for r in res]
        cv_log[:, t] = [int(r[4]) for r in res]
        margin = min([margin] + [r[5] for r in res])
        row0 = lambda k: None if w is None or getattr(w, k) is None else getattr(w, k)[:, 0]
        u0 = us[:, 0].copy()
        during = (row0("foot_r"), row0("foot_l"), None if wrench is None else wrench[:, t], substeps)
        if contact is None:
            x = plant_step(sm, true, x, u0, *during)
        else:
            on = sm.contact_flags(contact, row0("fz_max"), B)
            x, u0, state = plant_step(sm, true, x, u0, *during, contact=contact, in_contact=on, state=state)
            if "fallen" in state:
                fallen_log[:, t] = state["fallen"]
            values.append(sm.fall_values(x, contact))
        xs, us = shift_guess(sm, believed, xs, us, w)
        u_log[:, t] = u0
        x_log[:, t + 1] = x
    out = dict(x_log=x_log, u_log=u_log, sqp_iter=it_log, converged=cv_log, xs=xs, us=us, x=x, alpha=alpha,
               margin=margin, steps=steps)
    if gait is not None:
        out.update(foot_log=foot_log, fz_log=fz_log, ref_pose=ref_pose, foot_now=foot_now, windows=windows)
    if terrain is not None:
        out.update(q_log=q_log, select_margin=select_margin, poses=poses, feet=feet)
    if contact is not None:
        out.update(state=state, fallen_log=fallen_log, values=values)
    return out


# ---- the inputs several test modules share ----
def start(sm, p, B, N, seed):
    xs, us, dx0 = sm.sample_trajectories(B, N, seed, p)
    return xs, us, xs[:, 0] + dx0


def feet_plan(sm, p, B, N, seed):
    """nmpc_plan_host.random_plan's values for any N >= 1 (random_plan marks swing stages that
    need N >= 4)."""
    rng = np.random.default_rng(seed)
    return sm.SrbdPlan(x_ref=np.array(p.x_ref) + rng.uniform(-0.3, 0.3, size=(B, N + 1, 12)),
                       foot_r=np.array(p.foot_r) + rng.uniform(-0.15, 0.15, size=(B, N, 3)),
                       foot_l=np.array(p.foot_l) + rng.uniform(-0.15, 0.15, size=(B, N, 3)),
                       fz_max=rng.uniform(50.0, 300.0, size=(B, N, 2)))


def walking_case(sm, p, B, N, T, seed):
    """B robots walking for N + T - 1 plan stages, after nmpc_plan_host.walking_batch: each with
    its own velocity command (a reference that moves at that velocity) and stepping pattern (each
    foot swinging -- fz_max = 1 -- for five stages, then set down ahead along the command), from
    perturbed starts.  Returns (xs, us, x, alpha, long plan)."""
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
