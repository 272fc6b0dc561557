"""TEST INFRASTRUCTURE ONLY -- the device side of the closed-loop GPU tests, each helper once: the
settings and tolerances they share, host values as device tensors and capi objects, and the
caller's own loop over the public entry points that the rollouts are compared with bit for bit.
torch is imported where it is used, so the constants are there without it."""
from __future__ import annotations

import numpy as np

import nmpc_plan_host as PH
import robots_host as BH
from rollout_host import FIELDS

# NMPC_solver.cpp:70-82, as tests/test_gpu_nmpc.py
NMPC = dict(mode="Speed", iter_max=30, alpha_min=1e-8, mu0=1e2, tol_stat=1e-4, tol_eq=1e-4,
            tol_ineq=1e-4, tol_comp=1e-4, reg_prim=1e-12, warm_start=0, pred_corr=1, ric_alg=0,
            split_step=1)
SQP_MAX_LOOP = 15
STEP_ATOL_X, STEP_ATOL_U = 1e-9, 1e-6  # the step test's (tests/test_gpu_plan.py test 5)
# d_t of tests/test_gpu_rollout.py's comparison with the host closed loop: the
# largest change of the host loop's x_log[t] / u_log[t-1] when the loop is rerun with x, xs, us
# perturbed by relative 1e-7 -- the largest device-host gap the step test's tolerance admits
# after one step -- measured on the CPU (scripts/rollout_sensitivity.py) per case (constraints,
# alpha_reset), t = 1..4: (d_t of x, d_t of u).
ROLLOUT_D_T = {
    ("none", 0.0): ((2.7e-07, 5.1e-07, 7.4e-07, 8.3e-07), (2.3e-05, 1.7e-05, 1.4e-05, 8.8e-06)),
    ("none", 1.0): ((2.7e-07, 5.1e-07, 7.4e-07, 8.3e-07), (2.3e-05, 1.7e-05, 1.4e-05, 8.8e-06)),
    ("box_u", 0.0): ((2.8e-07, 5.3e-07, 7.7e-07, 8.5e-07), (2.4e-05, 1.7e-05, 1.4e-05, 8.7e-06)),
    ("box_u", 1.0): ((2.8e-07, 5.3e-07, 7.7e-07, 8.5e-07), (2.3e-05, 1.7e-05, 1.4e-05, 8.7e-06)),
}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def handle(capi, N, B, constraints):
    return capi.Handle(N, 12, 12, 24 if constraints == "cone" else 0, constraints == "box_u", False,
                       capacity=B)


def close(got, want, what):
    """The linearisation test's tolerance for the same RK4 (and the planner's one sincos and
    <= N + 1 additions)."""
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-11, atol=1e-12 * max(np.abs(want).max(), 1.0),
                               err_msg=str(what))


def host_nmpc(sm, oracle, p, batch, constraints):
    xs, us, x0, alpha, plan = batch
    return [PH.sqp_loop(sm, oracle, p, plan.robot(i), xs[i], us[i], x0[i], float(alpha[i]), NMPC,
                        SQP_MAX_LOOP, constraints) for i in range(xs.shape[0])]


def linesearch_matches_host(xs, us, xs_t, us_t, al_t, merit, conv, host):
    """What srbd_linesearch left on the device against the host restatement, robot by robot.
    xs, us: the inputs (numpy); xs_t, us_t, al_t: the device tensors after the call, merit and
    conv its results; host: per robot nmpc_plan_host.line_search's tuple.  Merit rtol 1e-9,
    alpha and converged exact, an accepted point to 1e-13; a robot without an accepted step
    (exhausted, or no trial at all) keeps its xs, us bit for bit."""
    import torch
    xs_in, us_in = _dev(xs), _dev(us)
    got_m, got_a, got_c = merit.cpu().numpy(), al_t.cpu().numpy(), conv.cpu().numpy()
    got_x, got_u = xs_t.cpu().numpy(), us_t.cpu().numpy()
    assert len(host) == xs.shape[0]
    for i, (xn, un, an, phi, theta, dphi, cv, margin) in enumerate(host):
        assert margin > 1e-8, (i, margin)  # the inputs are off every decision boundary
        np.testing.assert_allclose(got_m[i], [phi, theta, dphi], rtol=1e-9, atol=1e-12, err_msg=str(i))
        assert got_a[i] == an, (i, got_a[i], an)
        assert bool(got_c[i]) == cv, i
        if np.array_equal(xn, xs[i]) and np.array_equal(un, us[i]):  # no step was accepted
            assert torch.equal(xs_t[i], xs_in[i]) and torch.equal(us_t[i], us_in[i]), i
        else:
            np.testing.assert_allclose(got_x[i], xn, rtol=1e-13, atol=1e-13, err_msg=str(i))
            np.testing.assert_allclose(got_u[i], un, rtol=1e-13, atol=1e-13, err_msg=str(i))


# ---- host values as the binding's objects ----
def device_plan(capi, plan):
    return capi.Plan(**{k: (None if getattr(plan, k) is None else _dev(getattr(plan, k))) for k in FIELDS})


def device_gait(capi, g):
    """capi.Gait of a srbd_model.SrbdGait: an integer field given per robot (period [B], swing /
    offset [B][2]) becomes an int32 device tensor (the struct's _r array), one given for every
    robot stays the scalars."""
    ints = {}
    for name, rank in (("period", 1), ("swing", 2), ("offset", 2)):
        v = np.asarray(getattr(g, name))
        if v.ndim == rank:
            ints[name] = _dev_i32(v)
        else:
            ints[name] = int(v) if rank == 1 else tuple(int(e) for e in v)
    return capi.Gait(hip=g.hip, ground_z=g.ground_z, k_raibert=g.k_raibert, fz_stance=g.fz_stance,
                     fz_swing=g.fz_swing, anchor=g.anchor, **ints)


def device_robots(capi, params, fields=BH.MODEL_FIELDS):
    return capi.Robots(**{k: _dev(v) for k, v in BH.arrays(params, fields).items()})


def device_terrain(capi, t, map_r=None):
    """capi.Terrain of a srbd_model.SrbdTerrain."""
    m = t.map_r if map_r is None else map_r
    return capi.Terrain(_dev(np.asarray(t.height, dtype=np.float64)), t.x0, t.y0, t.cell,
                        map_r=None if m is None else _dev_i32(np.asarray(m)), search=t.search, w_rough=t.w_rough)


def device_contact(capi, c, state=None):
    """(capi.Contact of a srbd_model.SrbdContact, the device state): `state` as contact_host's
    dicts (None: no arrays); sat travels as int32, the same 32 bits."""
    import torch
    st = {k: torch.from_numpy(np.ascontiguousarray(v).astype(np.int32)).cuda() for k, v in (state or {}).items()}
    return capi.Contact(mu=c.mu, mu_r=None if c.mu_r is None else _dev(np.asarray(c.mu_r, dtype=np.float64)),
                        Lt=c.Lt, fz_hi=c.fz_hi, fz_contact=c.fz_contact, ground_z=c.ground_z,
                        ground=None if c.ground is None else device_terrain(capi, c.ground), z_min=c.z_min,
                        cos_tilt_min=c.cos_tilt_min, **st), st


# ---- the caller's loop ----
def caller_loop(capi, h, B, N, T, constraints, xs, us, x, alpha, wrench_t, substeps, alpha_reset, *, plan_t=None,
                gait_t=None, cmd_t=None, pose=None, feet=None, tick0=0):
    """The steps of a rollout's contract through the public entry points, on the caller's tensors
    (wrench_t [B][T][6] or None).  With plan_t (a device plan of at least N + T - 1 stages; None:
    no plan) srbd_qp_srbd_rollout_f64's through srbd_nmpc and srbd_advance, returning its four
    logs; with gait_t, cmd_t [B][T][4], pose, feet and tick0 srbd_qp_srbd_rollout_gait_f64's,
    srbd_gait_plan first, returning its six."""
    import torch
    f = dict(dtype=torch.float64, device="cuda")
    x_log, u_log = torch.zeros(B, T + 1, 12, **f), torch.zeros(B, T, 12, **f)
    it_log = torch.zeros(B, T, dtype=torch.int32, device="cuda")
    cv_log = torch.zeros(B, T, dtype=torch.int32, device="cuda")
    foot_log, fz_log = torch.zeros(B, T, 2, 3, **f), torch.zeros(B, T, 2, **f)
    x_log[:, 0] = x
    for t in range(T):
        if gait_t is not None:
            w = capi.srbd_gait_plan(h, gait_t, cmd_t[:, t].contiguous(), x, tick0 + t, pose, feet)
        elif plan_t is not None:
            w = capi.Plan(**{k: (None if getattr(plan_t, k) is None else
                                 getattr(plan_t, k)[:, t:t + N + (k == "x_ref")].contiguous()) for k in FIELDS})
        else:
            w = None
        if alpha_reset > 0.0:
            alpha.fill_(alpha_reset)
        it, cv = capi.srbd_nmpc(h, xs, us, x, alpha, constraints, NMPC, SQP_MAX_LOOP, plan=w)
        if gait_t is not None:
            foot_log[:, t, 0], foot_log[:, t, 1], fz_log[:, t] = w.foot_r[:, 0], w.foot_l[:, 0], w.fz_max[:, 0]
        u0 = capi.srbd_advance(h, xs, us, x=x, plan=w,
                               wrench=None if wrench_t is None else wrench_t[:, t].contiguous(),
                               substeps=substeps)
        h.synchronize()
        it_log[:, t], cv_log[:, t], u_log[:, t], x_log[:, t + 1] = it, cv, u0, x
    logs = (x_log, u_log, it_log, cv_log)
    return logs if gait_t is None else logs + (foot_log, fz_log)
