"""TEST INFRASTRUCTURE ONLY -- the adjoint of the open-loop plant rollout in numpy, robot by robot
(the yardstick of srbd_qp_srbd_plant_rollout_backward_f64, itself held to central
differences of the srbd_model.plant_step loop by tests/test_plant_backward_cpu.py).

The forward statement is rollout(): srbd_model.plant_step tick by tick.  The adjoint follows the
kernel's recursion: lambda starts at gx[T]; per tick, last first, per substep, last first, the
state at the substep's start is recomputed from the tick's checkpoint x_traj[t]; the RK4 step is
reversed through its four slopes,
    kb_j = (h w_j / 6) lambda + a_(j+1) pb_(j+1),   pb_j = J_x(p_j)' kb_j,   lambda += sum_j pb_j,
with J_x and J_u of srbd_model.continuous(jac=True); then lambda += gx[t].
"""
from __future__ import annotations

import dataclasses

import numpy as np

import rollout_host as RH

__all__ = ["OUTPUTS", "rollout", "plant_vjp"]

OUTPUTS = ("x0", "u", "foot_r", "foot_l", "wrench", "mass", "Lbody")


def _rows(a, t):
    return None if a is None else np.asarray(a)[:, t]


def rollout(sm, params, x0, u, foot_r=None, foot_l=None, wrench=None, substeps=1):
    """x_traj [B][T+1][12]: srbd_model.plant_step tick by tick (rollout_host.plant_step: robot by
    robot when params is a list of one SrbdParams per robot).  Feet [B][P][3], P >= T: row t."""
    B, T = u.shape[0], u.shape[1]
    x_traj = np.empty((B, T + 1, 12))
    x_traj[:, 0] = x0
    for t in range(T):
        x_traj[:, t + 1] = RH.plant_step(sm, params, x_traj[:, t], u[:, t], _rows(foot_r, t), _rows(foot_l, t),
                                         _rows(wrench, t), substeps)
    return x_traj


def _robot(sm, q, x_traj, u, foot_r, foot_l, wrench, gx, substeps):
    """One robot: q its SrbdParams, x_traj [T+1][12], u [T][12], foot_r / foot_l [T][3] or None,
    wrench [T][6] or None, gx [T+1][12]."""
    T = u.shape[0]
    h = q.dt / substeps
    a_of = (0.0, 0.5 * h, 0.5 * h, h)
    w_of = (1.0, 2.0, 2.0, 1.0)
    out = {"u": np.zeros((T, 12)), "foot_r": np.zeros((T, 3)), "foot_l": np.zeros((T, 3)), "wrench": np.zeros((T, 6))}
    giL, gim = np.zeros(3), 0.0
    lam = gx[T].copy()
    for t in range(T - 1, -1, -1):
        fr = None if foot_r is None else foot_r[t][None]
        fl = None if foot_l is None else foot_l[t][None]
        feet = None if fr is None and fl is None else sm.SrbdPlan(foot_r=fr, foot_l=fl)
        w = None if wrench is None else wrench[t]
        ut = u[t][None]
        f0, f1 = u[t, 0:3], u[t, 6:9]

        def slope(xa, jac):
            k, jx, ju = sm.continuous(xa, ut, q, jac, feet)
            if w is not None:
                k[:, 3:6] += w[0:3]
                k[:, 9:12] += w[3:6] / q.mass
            return k, jx, ju

        for s in range(substeps - 1, -1, -1):
            x = x_traj[t][None]
            if s > 0:  # s steps of h from the checkpoint
                x = sm.plant_step(x, ut, dataclasses.replace(q, dt=h * s), fr, fl, None if w is None else w[None], s)
            pts = [x]
            for j in range(3):
                pts.append(x + a_of[j + 1] * slope(pts[j], False)[0])
            pb, total = np.zeros(12), np.zeros(12)
            for j in range(3, -1, -1):
                kb = (h * w_of[j] / 6.0) * lam + (a_of[j + 1] * pb if j < 3 else 0.0)
                _, jx, ju = slope(pts[j], True)
                pb = jx[0].T @ kb
                total += pb
                out["u"][t] += ju[0].T @ kb
                out["wrench"][t, 0:3] += kb[3:6]
                out["wrench"][t, 3:6] += kb[9:12] / q.mass
                out["foot_r"][t] += np.cross(f0, kb[3:6])
                out["foot_l"][t] += np.cross(f1, kb[3:6])
                gim += float((f0 + f1 + (0.0 if w is None else w[3:6])) @ kb[9:12])
                r, l = pts[j][0, 0:3], pts[j][0, 3:6]
                R, Jlt = sm.expm(r), sm.jlt(r)
                for c in range(3):  # f[0:3] = Jlt R diag(1 / Lbody) R' l
                    giL[c] += float((Jlt @ R[:, c]) @ kb[0:3]) * float(R[:, c] @ l)
            lam = lam + total
        lam = lam + gx[t]
    out["x0"] = lam
    out["mass"] = -gim / q.mass ** 2
    out["Lbody"] = -giL / np.array(q.Lbody, dtype=np.float64) ** 2
    return out


def plant_vjp(sm, params, x_traj, u, gx, foot_r=None, foot_l=None, wrench=None, substeps=1):
    """The seven gradients {name: [B]...} (OUTPUTS; the shapes of srbd_plant_grad_f64, the feet's
    with T dense rows) of sum <gx, x_traj> at the trajectory x_traj = rollout(...).  params: one
    SrbdParams for every robot, or a list of one per robot; mass and Lbody are per robot either way."""
    B = u.shape[0]
    each = params if isinstance(params, (list, tuple)) else [params] * B
    one = lambda a, i: None if a is None else np.asarray(a, dtype=np.float64)[i]
    per = [_robot(sm, each[i], x_traj[i], u[i], one(foot_r, i), one(foot_l, i), one(wrench, i), gx[i], substeps)
           for i in range(B)]
    return {k: np.array([r[k] for r in per], dtype=np.float64) for k in OUTPUTS}
