"""TEST INFRASTRUCTURE ONLY -- the host side of the per-robot parameters
(srbd_qp_srbd_set_robots_f64): the existing host model called once per robot with that robot's
SrbdParams.  A batch is a list of SrbdParams, one per robot: the draws of the robots tests, their
device arrays, and the linearisation and the line search per robot.  The closed loop and the
per-robot SQP loop, plant step and shift are tests/rollout_host.py's; its closed_loop takes two
lists, what the controller believes (the MODEL role) and the true robot (the PLANT role)."""
from __future__ import annotations

import dataclasses

import numpy as np

import nmpc_plan_host as PH
from rollout_host import _batch_of_one

__all__ = ["draw", "draw_plant", "only", "arrays", "build_qp", "line_search"]

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


def build_qp(sm, params, xs, us, constraints, plan=None):
    """build_qp per robot; returns {key: [B]...} in the packed (C-ABI) layout."""
    packed = [sm.build_qp(xs[i:i + 1], us[i:i + 1], q, constraints, plan=_batch_of_one(sm, plan, i))[0].packed()
              for i, q in enumerate(params)]
    return {k: None if v is None else np.concatenate([pk[k] for pk in packed], axis=0)
            for k, v in packed[0].items()}


def line_search(sm, params, plan, xs, us, dx, du, alpha):
    """PH.line_search per robot: a list of its return tuples."""
    return [PH.line_search(sm, q, None if plan is None else plan.robot(i), xs[i], us[i], dx[i], du[i], float(alpha[i]))
            for i, q in enumerate(params)]
