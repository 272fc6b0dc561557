"""TEST INFRASTRUCTURE ONLY -- the host side of the plant's contact model
(srbd_qp_srbd_set_contact_f64): srbd_model.plant_step(contact=...) with one SrbdParams per robot,
and the host closed loop with a contact -- per tick the host SQP loop of tests/nmpc_plan_host.py
on the tick's plan window, then plant_step(contact=...) and srbd_model.shift_guess, in the order
include/srbd_qp.h states.  tests/rollout_host.py is the loop without a contact."""
from __future__ import annotations

import dataclasses

import numpy as np

import nmpc_plan_host as PH
import rollout_host as RH

__all__ = ["zero_state", "robot_contact", "plant_step", "closed_loop"]


def zero_state(B, fallen=True, alive=True, sat=True):
    """The fallen / alive / sat arrays of a batch that has not started."""
    s = {}
    if fallen:
        s["fallen"] = np.zeros(B, dtype=np.int32)
    if alive:
        s["alive"] = np.zeros(B, dtype=np.int32)
    if sat:
        s["sat"] = np.zeros(B, dtype=np.uint32)
    return s


def robot_contact(contact, i):
    """The contact of a batch that holds robot i alone (mu_r and the true ground's map_r sliced)."""
    g = contact.ground
    if g is not None and g.map_r is not None:
        g = dataclasses.replace(g, map_r=np.asarray(g.map_r)[i:i + 1])
    return dataclasses.replace(contact, mu_r=None if contact.mu_r is None else np.asarray(contact.mu_r)[i:i + 1],
                               ground=g)


def plant_step(sm, params, x, u, foot_r=None, foot_l=None, wrench=None, substeps=1, contact=None, in_contact=None,
               state=None):
    """srbd_model.plant_step(contact=...) with robot i's params (a list of SrbdParams: the PLANT
    role, or one SrbdParams for every robot).  Returns (x', u', state')."""
    B = x.shape[0]
    if not isinstance(params, (list, tuple)):
        return sm.plant_step(x, u, params, foot_r, foot_l, wrench, substeps, contact=contact, in_contact=in_contact,
                             state=state)
    state = {k: np.array(v) for k, v in (state or {}).items()}
    xo, uo = np.empty_like(x), np.empty_like(u)
    for i, q in enumerate(params):
        one = lambda a: None if a is None else np.asarray(a)[i:i + 1]
        xo[i:i + 1], uo[i:i + 1], st = sm.plant_step(
            x[i:i + 1], u[i:i + 1], q, one(foot_r), one(foot_l), one(wrench), substeps,
            contact=robot_contact(contact, i), in_contact=one(in_contact), state={k: v[i:i + 1] for k, v in state.items()})
        for k in state:
            state[k][i] = st[k][0]
    assert len(params) == B
    return xo, uo, state


def closed_loop(sm, oracle, p, plan, xs, us, x, alpha, ticks, settings, sqp_max_loop, contact, constraints="none",
                wrench=None, substeps=1, alpha_reset=0.0, state=None):
    """rollout_host.closed_loop with a contact: the plant step of every tick is
    plant_step(contact=...) with the contact flags of the window's fz_max row 0, and u_log holds
    the applied (projected) inputs.  `state`: the fallen / alive / sat arrays on entry (None:
    zero_state).  The same dict is returned, plus state (after the last tick), fallen_log
    [B][ticks] (fallen after each tick) and values (per tick, fall_values of the new states)."""
    B, N = us.shape[0], us.shape[1]
    xs, us, x = xs.copy(), us.copy(), x.copy()
    alpha = np.array(alpha, dtype=np.float64)
    state = zero_state(B) if state is None else {k: np.array(v) for k, v in state.items()}
    x_log = np.empty((B, ticks + 1, 12))
    u_log = np.empty((B, ticks, 12))
    it_log = np.zeros((B, ticks), dtype=np.int32)
    cv_log = np.zeros((B, ticks), dtype=np.int32)
    fallen_log = np.zeros((B, ticks), dtype=np.int32)
    x_log[:, 0] = x
    margin, steps, values = np.inf, [], []
    for t in range(ticks):
        w = RH.window(sm, plan, t, N)
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
        on = sm.contact_flags(contact, None if w is None or w.fz_max is None else w.fz_max[:, 0], B)
        x, u0, state = plant_step(sm, p, x, us[:, 0].copy(), None if w is None or w.foot_r is None else w.foot_r[:, 0],
                                  None if w is None or w.foot_l is None else w.foot_l[:, 0],
                                  None if wrench is None else wrench[:, t], substeps, contact=contact, in_contact=on,
                                  state=state)
        xs, us = sm.shift_guess(xs, us, p, w)
        u_log[:, t] = u0
        x_log[:, t + 1] = x
        if "fallen" in state:
            fallen_log[:, t] = state["fallen"]
        values.append(sm.fall_values(x, contact))
    return dict(x_log=x_log, u_log=u_log, sqp_iter=it_log, converged=cv_log, xs=xs, us=us, x=x, alpha=alpha,
                margin=margin, steps=steps, state=state, fallen_log=fallen_log, values=values)
