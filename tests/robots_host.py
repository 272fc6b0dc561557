"""TEST INFRASTRUCTURE ONLY -- the host side of the per-robot parameters
(srbd_qp_srbd_set_robots_f64): the existing host model called once per robot with that robot's
SrbdParams.  A batch is a list of SrbdParams, one per robot; the closed loop takes two, what the
controller believes (the MODEL role) and the true robot (the PLANT role), and runs the
operations of tests/rollout_host.py's closed_loop in its order."""
from __future__ import annotations

import dataclasses

import numpy as np

import nmpc_plan_host as PH
import rollout_host as RH

__all__ = ["draw", "draw_plant", "arrays", "build_qp", "line_search", "sqp_loops", "plant_step",
           "shift_guess", "closed_loop"]

MODEL_FIELDS = ("mass", "Lbody", "mu", "Q", "Qf", "R")
PLANT_FIELDS = ("mass", "Lbody")


def draw(p, B, seed):
    """The parameter draw of every robots test: per robot, in this order, mass, Lbody, mu, Q, Qf, R."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        mass = rng.uniform(10.0, 20.0)
        Lbody = np.array(p.Lbody) * rng.uniform(0.7, 1.3, 3)
        mu = rng.uniform(0.3, 0.8)
        Q = np.array(p.Q, dtype=np.float64) * rng.uniform(0.5, 2.0, 12)
        Qf = np.array(p.Qf, dtype=np.float64) * rng.uniform(0.5, 2.0, 12)
        R = p.R * rng.uniform(0.5, 2.0)
        out.append(dataclasses.replace(p, mass=float(mass), Lbody=tuple(Lbody.tolist()), mu=float(mu),
                                       Q=tuple(Q.tolist()), Qf=tuple(Qf.tolist()), R=float(R)))
    return out


def draw_plant(model, seed):
    """The true robots: per robot the model's mass x uniform(0.8, 1.25), then its Lbody x
    uniform(0.8, 1.25, 3); everything else is the model's."""
    rng = np.random.default_rng(seed)
    out = []
    for m in model:
        mass = m.mass * rng.uniform(0.8, 1.25)
        Lbody = np.array(m.Lbody) * rng.uniform(0.8, 1.25, 3)
        out.append(dataclasses.replace(m, mass=float(mass), Lbody=tuple(Lbody.tolist())))
    return out


def only(p, params, fields):
    """`params` with every field outside `fields` put back to p's."""
    keep = {f: getattr(p, f) for f in MODEL_FIELDS if f not in fields}
    return [dataclasses.replace(q, **keep) for q in params]


def arrays(params, fields=MODEL_FIELDS):
    """The srbd_robots_f64 arrays of a list of SrbdParams: {field: [B] or [B][3] or [B][12]}."""
    return {f: np.ascontiguousarray(np.array([getattr(q, f) for q in params], dtype=np.float64))
            for f in fields}


def _rows(plan, i):
    return None if plan is None else plan.robot(i)


def _batch_of_one(sm, plan, i):
    if plan is None:
        return None
    return sm.SrbdPlan(*[None if a is None else a[i:i + 1]
                         for a in (plan.x_ref, plan.foot_r, plan.foot_l, plan.fz_max)])


def build_qp(sm, params, xs, us, constraints, plan=None):
    """build_qp per robot; returns {key: [B]...} in the packed (C-ABI) layout."""
    packed = [sm.build_qp(xs[i:i + 1], us[i:i + 1], q, constraints, plan=_batch_of_one(sm, plan, i))[0].packed()
              for i, q in enumerate(params)]
    return {k: None if v is None else np.concatenate([pk[k] for pk in packed], axis=0)
            for k, v in packed[0].items()}


def line_search(sm, params, plan, xs, us, dx, du, alpha):
    """PH.line_search per robot: a list of its return tuples."""
    return [PH.line_search(sm, q, _rows(plan, i), xs[i], us[i], dx[i], du[i], float(alpha[i]))
            for i, q in enumerate(params)]


def sqp_loops(sm, oracle, params, plan, xs, us, x0, alpha, settings, sqp_max_loop, constraints):
    """PH.sqp_loop per robot: a list of its return tuples."""
    return [PH.sqp_loop(sm, oracle, q, _rows(plan, i), xs[i], us[i], x0[i], float(alpha[i]), settings,
                        sqp_max_loop, constraints) for i, q in enumerate(params)]


def plant_step(sm, params, x, u, foot_r=None, foot_l=None, wrench=None, substeps=1):
    """srbd_model.plant_step with robot i's params."""
    return np.concatenate([sm.plant_step(x[i:i + 1], u[i:i + 1], q,
                                         None if foot_r is None else foot_r[i:i + 1],
                                         None if foot_l is None else foot_l[i:i + 1],
                                         None if wrench is None else wrench[i:i + 1], substeps)
                           for i, q in enumerate(params)], axis=0)


def shift_guess(sm, params, xs, us, plan=None):
    """srbd_model.shift_guess with robot i's params."""
    parts = [sm.shift_guess(xs[i:i + 1], us[i:i + 1], q, _batch_of_one(sm, plan, i))
             for i, q in enumerate(params)]
    return np.concatenate([a for a, _ in parts], axis=0), np.concatenate([b for _, b in parts], axis=0)


def closed_loop(sm, oracle, model, plant, plan, xs, us, x, alpha, ticks, settings, sqp_max_loop,
                constraints="none", wrench=None, substeps=1, alpha_reset=0.0):
    """rollout_host.closed_loop with per-robot parameters: the SQP loop and the new last stage of
    the guess use model[i], the plant step uses plant[i].  The same dict is returned."""
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
        w = RH.window(sm, plan, t, N)
        if alpha_reset > 0.0:
            alpha[:] = alpha_reset
        res = sqp_loops(sm, oracle, model, w, xs, us, x, alpha, settings, sqp_max_loop, constraints)
        steps.append(res)
        xs = np.stack([r[0] for r in res])
        us = np.stack([r[1] for r in res])
        alpha = np.array([r[2] for r in res], dtype=np.float64)
        it_log[:, t] = [r[3] for r in res]
        cv_log[:, t] = [int(r[4]) for r in res]
        margin = min([margin] + [r[5] for r in res])
        u0 = us[:, 0].copy()
        x = plant_step(sm, plant, x, u0, None if w is None or w.foot_r is None else w.foot_r[:, 0],
                       None if w is None or w.foot_l is None else w.foot_l[:, 0],
                       None if wrench is None else wrench[:, t], substeps)
        xs, us = shift_guess(sm, model, xs, us, w)
        u_log[:, t] = u0
        x_log[:, t + 1] = x
    return dict(x_log=x_log, u_log=u_log, sqp_iter=it_log, converged=cv_log, xs=xs, us=us, x=x,
                alpha=alpha, margin=margin, steps=steps)
