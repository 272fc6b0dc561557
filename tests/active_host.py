"""TEST INFRASTRUCTURE ONLY -- the host statement of active sets (srbd_qp_srbd_set_active_f64).
The step over a mask is tests/nmpc_plan_host.py's sqp_loop run for the active robots only, the
others returned unchanged with sqp_iter = converged = 0; the rollout with skip_fallen is
tests/rollout_host.py's closed loop with that step, the active robots of a tick being those that
had not fallen when it started.  Next to it the starts the GPU tests share: a few base robots
whose SQP iteration counts differ, tiled over a batch."""
from __future__ import annotations

import contextlib

import numpy as np

import nmpc_plan_host as PH
import rollout_host as RH

__all__ = ["sqp_loops", "step", "closed_loop", "reference_start", "base_starts", "tiled", "BASE_K"]


def sqp_loops(sm, oracle, params, plan, xs, us, x0, alpha, settings, sqp_max_loop, constraints, active=None):
    """rollout_host.sqp_loops over the robots with active[i] (None: all); a robot that is not
    active returns its inputs, 0 iterations, not converged, and no comparison margin."""
    B = xs.shape[0]
    each = params if isinstance(params, (list, tuple)) else [params] * B
    out = []
    for i, q in enumerate(each):
        if active is not None and not active[i]:
            out.append((xs[i].copy(), us[i].copy(), float(alpha[i]), 0, False, np.inf))
        else:
            out.append(PH.sqp_loop(sm, oracle, q, None if plan is None else plan.robot(i), xs[i], us[i], x0[i],
                                   float(alpha[i]), settings, sqp_max_loop, constraints))
    return out


def step(sm, oracle, params, plan, xs, us, x0, alpha, settings, sqp_max_loop, constraints, active=None):
    """One NMPC step of a batch over an active set.  Returns a dict: xs, us, alpha, sqp_iter,
    converged (arrays over the batch) and margin (the smallest comparison margin)."""
    res = sqp_loops(sm, oracle, params, plan, xs, us, x0, alpha, settings, sqp_max_loop, constraints, active)
    return dict(xs=np.stack([r[0] for r in res]), us=np.stack([r[1] for r in res]),
                alpha=np.array([r[2] for r in res], dtype=np.float64),
                sqp_iter=np.array([r[3] for r in res], dtype=np.int32),
                converged=np.array([int(r[4]) for r in res], dtype=np.int32), margin=min(r[5] for r in res))


@contextlib.contextmanager
def _stepping(active):
    """rollout_host.closed_loop with its step replaced by the step over `active`."""
    plain = RH.sqp_loops
    RH.sqp_loops = lambda *a: sqp_loops(*a, active=active)
    try:
        yield
    finally:
        RH.sqp_loops = plain


def closed_loop(sm, oracle, xs, us, x, alpha, ticks, settings, sqp_max_loop, constraints="none", *, mask=None,
                skip_fallen=False, plan=None, gait=None, cmd=None, ref_pose=None, foot_now=None, tick0=0,
                wrench=None, contact=None, state=None, **kw):
    """rollout_host.closed_loop, one tick at a time, each tick's step run over the robots with
    mask[i] != 0 (None: all) that, with skip_fallen, had not fallen when the tick started.
    Returns its dict (the logs joined over the ticks; steps, windows and values as lists per
    tick)."""
    B, N = us.shape[0], us.shape[1]
    out = None
    for t in range(ticks):
        active = np.ones(B, dtype=bool) if mask is None else np.asarray(mask) != 0
        if skip_fallen:
            active &= (np.zeros(B, dtype=np.int32) if state is None else np.asarray(state["fallen"])) == 0
        sub = lambda a: None if a is None else a[:, t:]
        long_plan = None if plan is None else sm.SrbdPlan(**{k: sub(getattr(plan, k)) for k in RH.FIELDS})
        with _stepping(active):
            one = RH.closed_loop(sm, oracle, xs, us, x, alpha, 1, settings, sqp_max_loop, constraints, plan=long_plan,
                                 gait=gait, cmd=None if cmd is None else cmd[:, t:t + 1], ref_pose=ref_pose,
                                 foot_now=foot_now, tick0=tick0 + t,
                                 wrench=None if wrench is None else wrench[:, t:t + 1], contact=contact, state=state,
                                 **kw)
        xs, us, x, alpha = one["xs"], one["us"], one["x"], one["alpha"]
        state = one.get("state")
        ref_pose, foot_now = one.get("ref_pose"), one.get("foot_now")
        if out is None:
            out = dict(one)
            continue
        for k, v in one.items():
            if k == "x_log":
                out[k] = np.concatenate([out[k], v[:, 1:]], axis=1)
            elif k in ("u_log", "sqp_iter", "converged", "foot_log", "fz_log", "fallen_log", "q_log"):
                out[k] = np.concatenate([out[k], v], axis=1)
            elif k in ("steps", "windows", "values", "poses", "feet"):
                out[k] = out[k] + v
            elif k in ("margin", "select_margin"):
                out[k] = min(out[k], v)
            else:
                out[k] = v
    return out


# ---- starts whose SQP iteration counts differ ----
BASE_K = 8


def reference_start(N):
    """NMPCSolver::initialize / setupReference (NMPC_solver.cpp:56-64, 341-350), as
    tests/test_gpu_nmpc.py: x_nmpc = 0, u_nmpc = 100, x0 = (0, .., z = 1, 0, 0, 0), alpha_ = 1."""
    xs, us, x0 = np.zeros((N + 1, 12)), np.full((N, 12), 100.0), np.zeros(12)
    x0[8] = 1.0
    return xs, us, x0


def base_starts(sm, oracle, p, N, seed, settings, sqp_max_loop, constraints):
    """BASE_K robots and what the host loop does with each: robots 0 and 4 the reference's cold
    start, robots 1, 3, 5, 7 perturbed sample trajectories (robot 5 with alpha = 0.25: it runs to
    sqp_max_loop), robots 2 and 6 the result of an already-converged host step (from the same x0:
    one iteration is left to do).  Returns (xs, us, x0, alpha, host): host the dict of step() on
    them."""
    xs, us, x0 = RH.start(sm, p, BASE_K, N, seed)
    alpha = np.where(np.arange(BASE_K) % 4 == 1, 0.5, 1.0)
    for i in (0, 4):
        xs[i], us[i], x0[i] = reference_start(N)
    for i in (2, 6):
        r = PH.sqp_loop(sm, oracle, p, None, xs[i], us[i], x0[i], float(alpha[i]), settings, 4 * sqp_max_loop,
                        constraints)
        xs[i], us[i], alpha[i] = r[0], r[1], r[2]
    x0[4, 6:8] += 0.01  # (two cold starts that are not the same robot)
    alpha[5] = 0.25     # a line search that starts this short does not converge within sqp_max_loop
    host = step(sm, oracle, p, None, xs, us, x0, alpha, settings, sqp_max_loop, constraints)
    return xs, us, x0, alpha, host


def tiled(B, *arrays):
    """Robot i of a batch of B is base robot (5 i + i // BASE_K) % BASE_K: from B = 7 on every
    base robot but one occurs, and neighbours differ, in an order that does not repeat with the
    wave or the tile.  Returns (the base index of every robot, the arrays gathered)."""
    i = np.arange(B)
    base = (5 * i + i // BASE_K) % BASE_K
    return (base,) + tuple(np.ascontiguousarray(a[base]) for a in arrays)
