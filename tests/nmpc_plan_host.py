"""TEST INFRASTRUCTURE ONLY -- the host restatement of the filter line search and of the SQP
loop (oracle/nmpc_linesearch.py) with a plan: a per-stage reference x_ref[k], per-stage feet
and per-stage, per-foot force limits fz_max[k] (srbd_model.SrbdPlan, one robot's rows).

With a plan that repeats SrbdParams' constants every function here performs the operations of
its twin in oracle/nmpc_linesearch.py in the same order, so the results are the same bits
(tests/test_plan_cpu.py holds it to that).

`line_search` also returns the smallest relative margin |a - b| / max(|a|, |b|) over every
comparison between computed quantities that it evaluated (the filter's accept / reject tests
and the convergence test).  A device run may differ from the host in the last bits of phi and
theta; it takes the same decisions whenever that margin is far above those bits."""
from __future__ import annotations

import sys
from collections import namedtuple
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))
from nmpc_linesearch import LS_DEFAULTS, _barrier_value  # noqa: E402

__all__ = ["LS_DEFAULTS", "merit", "line_search", "sqp_loop", "random_plan", "constant_plan", "walking_batch",
           "NMPC_SEED"]

NMPC_SEED = 26  # walking_batch's, chosen on the CPU: the host loops' smallest comparison margin is >= 1e-6


def merit(srbd_model, p, plan, xs, us, N, Ac, bc):
    """(phi, theta, Jphi_x, Jphi_u) of one robot's trajectory under its plan."""
    Qd = np.array(p.Q, dtype=np.float64)
    Qf = float(N) * np.array(p.Qf, dtype=np.float64)
    xr = np.array(p.x_ref, dtype=np.float64)
    xr = np.broadcast_to(xr, (N + 1, 12)) if plan is None or plan.x_ref is None else plan.x_ref
    bck = np.broadcast_to(srbd_model.plan_cone_offsets(bc, plan), (N, 24))
    phi = 0.0
    theta = 0.0
    Jx = np.zeros((N + 1, 12))
    Ju = np.zeros((N, 12))
    _, _, b = srbd_model.shooting_dynamics(xs[:N], xs[1:], us, p, plan)  # b = -f per stage
    for k in range(N + 1):
        e = xs[k] - xr[k]
        if k == N:
            phi += 0.5 * e @ (Qf * e)
            Jx[k] = Qf * e
            continue
        f = -b[k]
        theta += 0.5 * f @ f
        phi += 0.5 * e @ (Qd * e)
        Jx[k] = Qd * e
        fc = Ac @ us[k] + bck[k]
        bsum, db = 0.0, np.zeros(24)
        for c in range(24):
            bv, db[c] = _barrier_value(fc[c], p.mu_b, p.theta_b)
            bsum += bv
        phi += bsum + 0.5 * p.R * (us[k] @ us[k])
        Ju[k] = Ac.T @ db + p.R * us[k]
    return phi, theta, Jx, Ju


class _Margin:
    """Runs the comparisons and remembers the tightest one."""

    def __init__(self):
        self.smallest = np.inf

    def lt(self, a, b):
        scale = max(abs(a), abs(b))
        self.smallest = min(self.smallest, abs(a - b) / scale if scale > 0.0 else np.inf)
        return a < b


Trial = namedtuple("Trial", "alpha branch accepted phi_a theta_a phi_clause theta_clause")
Trial.__doc__ = """One trial step of line_search's trace: its step length, the filter branch it took
("theta": theta_a > theta_max; "armijo"; "mixed": the rest), whether it was accepted, the merit at
the trial point, and for the mixed branch each accept clause on its own (phi_a < phi - beta_phi
theta; theta_a < (1 - beta_theta) theta), else None."""


def line_search(srbd_model, p, plan, xs, us, dx, du, alpha, ls=None, trace=None):
    """One robot.  Returns (xs_new, us_new, alpha_new, phi, theta, dphi, converged, margin).
    trace: a list that receives one Trial per trial step (none when alpha <= alpha_min on
    entry); it changes neither the operations nor the margin."""
    ls = dict(LS_DEFAULTS, **(ls or {}))
    N = us.shape[0]
    Ac, bc = srbd_model.friction_cone(p)
    phi, theta, Jx, Ju = merit(srbd_model, p, plan, xs, us, N, Ac, bc)
    dphi = float(np.sum(dx * Jx) + np.sum(du * Ju))
    m = _Margin()
    xs_new, us_new = xs, us
    while alpha > ls["alpha_min"]:
        xa = xs + alpha * dx
        ua = us + alpha * du
        phi_a, theta_a, _, _ = merit(srbd_model, p, plan, xa, ua, N, Ac, bc)
        clauses = (None, None)
        if m.lt(ls["theta_max"], theta_a):
            branch = "theta"
            ok = m.lt(theta_a, (1.0 - ls["beta_theta"]) * theta)
        elif m.lt(max(theta_a, theta), ls["theta_min"]) and m.lt(dphi, 0.0):
            branch = "armijo"
            ok = m.lt(phi_a, phi + ls["eta"] * alpha * dphi)
        else:
            branch = "mixed"
            ok = m.lt(phi_a, phi - ls["beta_phi"] * theta) or m.lt(theta_a, (1.0 - ls["beta_theta"]) * theta)
            if trace is not None:  # plain comparisons: the second one is not part of the decision above
                clauses = (phi_a < phi - ls["beta_phi"] * theta, theta_a < (1.0 - ls["beta_theta"]) * theta)
        if trace is not None:
            trace.append(Trial(alpha, branch, ok, phi_a, theta_a, *clauses))
        if ok:
            xs_new, us_new = xa, ua
            break
        alpha = ls["beta_alpha"] * alpha
    converged = m.lt(-1e-3, dphi) and m.lt(theta, 1e-6)
    return xs_new, us_new, alpha, phi, theta, dphi, converged, m.smallest


def sqp_loop(srbd_model, oracle, p, plan, xs, us, x0, alpha, settings, sqp_max_loop, constraints="none"):
    """One robot through the SQP loop under its plan (rows without the batch dimension).
    Returns (xs, us, alpha, sqp_iterations, converged, smallest margin of all line searches)."""
    xs, us = xs.copy(), us.copy()
    batched = None if plan is None else srbd_model.SrbdPlan(
        *[None if a is None else a[None] for a in (plan.x_ref, plan.foot_r, plan.foot_l, plan.fz_max)])
    it, conv, margin = 0, False, np.inf
    for it in range(1, sqp_max_loop + 1):
        qp, _ = srbd_model.build_qp(xs[None], us[None], p, constraints, plan=batched)
        sol = oracle.solve(qp, settings, x0=(x0 - xs[0])[None])
        xs, us, alpha, _, _, _, conv, mg = line_search(srbd_model, p, plan, xs, us, sol["x"][0],
                                                       sol["u"][0], alpha)
        margin = min(margin, mg)
        if conv:
            break
    return xs, us, alpha, it, conv, margin


# ---- the plans several test modules share ----
def random_plan(sm, p, B, N, seed, fields=("x_ref", "foot_r", "foot_l", "fz_max")):
    """Distinct values for every robot and stage: references within +-0.3 of the default, feet
    within +-0.15 m, fz_max in [50, 300] with a few swing stages at 1.0."""
    rng = np.random.default_rng(seed)
    x_ref = np.array(p.x_ref) + rng.uniform(-0.3, 0.3, size=(B, N + 1, 12))
    foot_r = np.array(p.foot_r) + rng.uniform(-0.15, 0.15, size=(B, N, 3))
    foot_l = np.array(p.foot_l) + rng.uniform(-0.15, 0.15, size=(B, N, 3))
    fz = rng.uniform(50.0, 300.0, size=(B, N, 2))
    swing = rng.uniform(size=(B, N, 2)) < 0.15
    swing[0, 3, 0] = swing[B - 1, N - 1, 1] = True
    fz[swing] = 1.0
    full = dict(x_ref=x_ref, foot_r=foot_r, foot_l=foot_l, fz_max=fz)
    return sm.SrbdPlan(**{k: (v if k in fields else None) for k, v in full.items()})


def constant_plan(sm, p, B, N):
    return sm.SrbdPlan(x_ref=np.tile(np.array(p.x_ref, dtype=np.float64), (B, N + 1, 1)),
                       foot_r=np.tile(np.array(p.foot_r, dtype=np.float64), (B, N, 1)),
                       foot_l=np.tile(np.array(p.foot_l, dtype=np.float64), (B, N, 1)),
                       fz_max=np.full((B, N, 2), float(p.fmax)))


def walking_batch(sm, p, B, N, seed):
    """B robots, each with its own velocity command (a reference that moves at that velocity)
    and a stepping pattern (feet that are set down ahead along the command, each foot
    swinging -- fz_max = 1 -- for part of the horizon), from perturbed starts."""
    rng = np.random.default_rng(seed)
    xs, us, dx0 = sm.sample_trajectories(B, N, seed, p)
    x0 = xs[:, 0] + dx0
    k = np.arange(N + 1)
    x_ref = np.tile(np.array(p.x_ref, dtype=np.float64), (B, N + 1, 1))
    foot_r = np.tile(np.array(p.foot_r, dtype=np.float64), (B, N, 1))
    foot_l = np.tile(np.array(p.foot_l, dtype=np.float64), (B, N, 1))
    fz = np.empty((B, N, 2))
    for i in range(B):
        v = rng.uniform(-0.3, 0.3, size=2)  # commanded (vx, vy)
        x_ref[i, :, 6:8] += np.outer(k * p.dt, v)
        x_ref[i, :, 9:11] = v
        x_ref[i] += rng.uniform(-0.01, 0.01, size=(N + 1, 12))
        fz[i] = rng.uniform(150.0, 300.0, size=(N, 2))
        s0 = int(rng.integers(2, 6))  # right foot swings s0 .. s0+4, left s0+9 .. s0+13
        step = 10.0 * p.dt * v
        for foot, lo in ((0, s0), (1, s0 + 9)):
            f = foot_r if foot == 0 else foot_l
            fz[i, lo:lo + 5, foot] = 1.0
            f[i, lo + 5:, 0:2] += step  # set down ahead
            f[i] += rng.uniform(-0.005, 0.005, size=(N, 3))
    plan = sm.SrbdPlan(x_ref=x_ref, foot_r=foot_r, foot_l=foot_l, fz_max=fz)
    alpha = np.where(np.arange(B) % 4 == 1, 0.5, 1.0)
    return xs, us, x0, alpha, plan
