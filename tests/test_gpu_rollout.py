"""The closed loop on the device (srbd_qp_srbd_advance_f64: one tick's plant step and shift of the
guess; srbd_qp_srbd_rollout_f64: T ticks of step + advance with a sliding plan window) against
the host model (srbd_model.plant_step / shift_guess), against the caller's own loop over the two
public entry points (bit for bit) and against the host closed loop of tests/rollout_host.py."""
import numpy as np
import pytest

import rollout_host as RH
from nmpc_plan_host import random_plan
from rollout_host import feet_plan, start
from srbd_device import (NMPC, ROLLOUT_D_T as D_T, SQP_MAX_LOOP, STEP_ATOL_U, STEP_ATOL_X, _dev, caller_loop, close,
                         device_plan, handle)

pytestmark = pytest.mark.gpu


# ---- 1. one tick against the host model ----
# N = 33: a 408-double xs row = 204 double2, three full 64-lane chunks and a partial one (and the
# us row two chunks and a partial one); N = 1: nothing of us moves; N = 2: one stage of us moves.
@pytest.mark.parametrize("N", [33, 1, 2])
def test_advance_matches_the_host_model(pkg, N):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B = 5
    p = sm.SrbdParams()
    xs, us, x = start(sm, p, B, N, 700 + N)
    plan = feet_plan(sm, p, B, N, 21)
    plan_t = device_plan(capi, plan)
    wrench = np.random.default_rng(22).uniform(-20.0, 20.0, size=(B, 6))
    h = handle(capi, N, B, "none")
    for substeps in (1, 4):
        for use_w in (False, True):
            for use_plan in (True, False):
                for use_x in (True, False):
                    case = (substeps, use_w, use_plan, use_x)
                    xs_t, us_t, x_t = _dev(xs), _dev(us), _dev(x)
                    u0 = capi.srbd_advance(h, xs_t, us_t, x=x_t if use_x else None,
                                           plan=plan_t if use_plan else None,
                                           wrench=_dev(wrench) if use_w else None, substeps=substeps)
                    h.synchronize()
                    # bit copies
                    assert torch.equal(u0, _dev(us[:, 0])), case
                    assert torch.equal(xs_t[:, :N], _dev(xs[:, 1:])), case
                    assert torch.equal(us_t[:, :N - 1], _dev(us[:, 1:])), case
                    assert torch.equal(us_t[:, N - 1], _dev(us[:, N - 1])), case
                    # the two model steps
                    pl = plan if use_plan else None
                    want_xs, want_us = sm.shift_guess(xs, us, p, pl)
                    close(xs_t[:, N], want_xs[:, N], case)
                    assert np.array_equal(want_us, us_t.cpu().numpy())
                    if use_x:
                        want_x = sm.plant_step(x, us[:, 0], p, pl.foot_r[:, 0] if pl else None,
                                               pl.foot_l[:, 0] if pl else None,
                                               wrench if use_w else None, substeps)
                        close(x_t, want_x, case)
                    else:  # shift only: the plant state is not touched
                        assert torch.equal(x_t, _dev(x)), case


# ---- 2. a rollout is the caller's loop over the two public entry points, bit for bit ----
@pytest.mark.parametrize("alpha_reset", [0.0, 1.0])
@pytest.mark.parametrize("constraints", ["none", "box_u", "cone"])
def test_rollout_is_the_callers_loop_bit_for_bit(pkg, constraints, alpha_reset):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N = 6, 10
    p = sm.SrbdParams()
    xs, us, x = start(sm, p, B, N, 41)
    alpha = np.where(np.arange(B) % 3 == 1, 0.5, 1.0)
    h = handle(capi, N, B, constraints)
    for T in (3, 1):
        P = N + T + 1  # longer than the rollout needs: the window's stride is the plan's
        plan_t = device_plan(capi, random_plan(sm, p, B, P, 42))
        wrench_t = _dev(np.random.default_rng(43).uniform(-15.0, 15.0, size=(B, T, 6)))
        a = [_dev(v) for v in (xs, us, x, alpha)]
        logs_a = capi.srbd_rollout(h, *a, T, constraints, NMPC, SQP_MAX_LOOP, plan=plan_t, plan_stages=P,
                                   wrench=wrench_t, substeps=2, alpha_reset=alpha_reset)
        b = [_dev(v) for v in (xs, us, x, alpha)]
        logs_b = caller_loop(capi, h, B, N, T, constraints, *b, wrench_t, 2, alpha_reset, plan_t=plan_t)
        names = ("xs", "us", "x", "alpha", "x_log", "u_log", "sqp_iter_log", "converged_log")
        for name, u, v in zip(names, a + list(logs_a), b + list(logs_b)):
            assert bool(torch.isfinite(u.double()).all()), (T, name)
            assert torch.equal(u, v), (T, name)
        assert int(logs_a[2].min()) >= 1  # the steps ran
        assert not torch.equal(a[0], _dev(xs))


def test_rollout_of_zero_ticks_touches_nothing(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N = 6, 10
    p = sm.SrbdParams()
    xs, us, x = start(sm, p, B, N, 41)
    a = [_dev(v) for v in (xs, us, x, np.full(B, 0.5))]
    h = handle(capi, N, B, "none")
    x_log, u_log, it_log, cv_log = capi.srbd_rollout(h, *a, 0, "none", NMPC, SQP_MAX_LOOP, alpha_reset=1.0)
    for u, v in zip(a, (xs, us, x, np.full(B, 0.5))):
        assert torch.equal(u, _dev(v))
    assert x_log.shape == (B, 1, 12) and torch.equal(x_log[:, 0], a[2])
    assert u_log.shape == (B, 0, 12) and it_log.shape == (B, 0) and cv_log.shape == (B, 0)


# ---- 3. a rollout against the host closed loop ----
# ROLLOUT_SEED was chosen on the CPU: with it the host loop's smallest comparison margin over all
# ticks is >= 1e-6 and at least two distinct SQP iteration counts occur, in all four cases below
# (both are asserted).
ROLLOUT_SEED = 30  # scripts/rollout_sensitivity.py --search 24 34: margins 3.3e-6 (none), 4.5e-6 (box_u)
# D_T and the step tolerances: tests/srbd_device.py


@pytest.mark.parametrize("alpha_reset", [0.0, 1.0])
@pytest.mark.parametrize("constraints", ["none", "box_u"])
def test_rollout_matches_the_host_closed_loop(pkg, oracle, constraints, alpha_reset):
    capi, sm = pkg.capi, pkg.srbd_model
    B, N, T = 4, 10, 4
    p = sm.SrbdParams()
    xs, us, x, alpha, plan = RH.walking_case(sm, p, B, N, T, ROLLOUT_SEED)
    host = RH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, SQP_MAX_LOOP, constraints, p=p, plan=plan,
                          alpha_reset=alpha_reset)
    # conditions on the inputs: no host decision on a boundary, and robots that stop at different
    # iterations
    assert host["margin"] >= 1e-6, host["margin"]
    assert len(set(host["sqp_iter"].ravel().tolist())) >= 2, host["sqp_iter"]
    h = handle(capi, N, B, constraints)
    xs_t, us_t, x_t, al_t = _dev(xs), _dev(us), _dev(x), _dev(alpha)
    x_log, u_log, it_log, cv_log = capi.srbd_rollout(h, xs_t, us_t, x_t, al_t, T, constraints, NMPC,
                                                     SQP_MAX_LOOP, plan=device_plan(capi, plan),
                                                     alpha_reset=alpha_reset)
    x_log, u_log = x_log.cpu().numpy(), u_log.cpu().numpy()
    print("sqp_iter device", it_log.cpu().numpy().tolist(), "host", host["sqp_iter"].tolist())
    for t in range(1, T + 1):
        print(f"tick {t}: max |x_log - host| {np.abs(x_log[:, t] - host['x_log'][:, t]).max():.3e}, "
              f"max |u_log - host| {np.abs(u_log[:, t - 1] - host['u_log'][:, t - 1]).max():.3e}")
    assert np.array_equal(it_log.cpu().numpy(), host["sqp_iter"])
    assert np.array_equal(cv_log.cpu().numpy(), host["converged"])
    assert np.array_equal(al_t.cpu().numpy(), host["alpha"])
    assert np.array_equal(x_log[:, 0], x)
    dt_x, dt_u = D_T[(constraints, alpha_reset)]
    for t in range(1, T + 1):
        # tick 1 is one step: the step test's tolerance; later ticks compound, by at most d_t
        ax = STEP_ATOL_X if t == 1 else max(STEP_ATOL_X, 10.0 * dt_x[t - 1])
        au = STEP_ATOL_U if t == 1 else max(STEP_ATOL_U, 10.0 * dt_u[t - 1])
        np.testing.assert_allclose(x_log[:, t], host["x_log"][:, t], rtol=1e-7, atol=ax, err_msg=f"x {t}")
        np.testing.assert_allclose(u_log[:, t - 1], host["u_log"][:, t - 1], rtol=1e-7, atol=au,
                                   err_msg=f"u {t}")
    assert np.array_equal(x_t.cpu().numpy(), x_log[:, T])


# ---- 4. the wrench does what it says ----
def test_a_force_on_one_tick_moves_the_velocity_by_dt_F_over_mass(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N, T = 4, 10, 3
    p = sm.SrbdParams()
    xs, us, x, alpha, plan = RH.walking_case(sm, p, B, N, T, ROLLOUT_SEED)
    F = np.random.default_rng(5).uniform(20.0, 50.0, size=(B, 3)) * np.array([1.0, -1.0, 1.0])
    wrench = np.zeros((B, T, 6))
    pushed = wrench.copy()
    pushed[:, 1, 3:6] = F
    h = handle(capi, N, B, "none")
    plan_t = device_plan(capi, plan)
    logs = []
    for w in (wrench, pushed):
        a = [_dev(v) for v in (xs, us, x, alpha)]
        logs.append(capi.srbd_rollout(h, *a, T, "none", NMPC, SQP_MAX_LOOP, plan=plan_t, wrench=_dev(w),
                                      substeps=1, alpha_reset=1.0)[0])
    assert torch.equal(logs[0][:, :2], logs[1][:, :2])  # nothing before the push
    # the velocity rows of the model are affine in the force: dt F / mass after the tick
    dv = (logs[1][:, 2, 9:12] - logs[0][:, 2, 9:12]).cpu().numpy()
    np.testing.assert_allclose(dv, p.dt * F / p.mass, rtol=1e-12, atol=0.0)
    assert not torch.equal(logs[0][:, 3], logs[1][:, 3])  # and the controller reacts to it


# ---- 5. errors, and the window scratch ----
def test_rollout_errors_and_scratch(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N, T = 4, 10, 2
    p = sm.SrbdParams()
    xs, us, x = start(sm, p, B, N, 41)
    fresh = lambda: [_dev(v) for v in (xs, us, x, np.ones(B))]
    cap = 8
    h = capi.Handle(N, 12, 12, capacity=cap)
    short = device_plan(capi, random_plan(sm, p, B, N + T - 2, 42))
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*plan_stages"):  # SRBD_QP_EINVAL
        capi.srbd_rollout(h, *fresh(), T, "none", NMPC, plan=short, plan_stages=N + T - 2)
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*substeps"):
        capi.srbd_rollout(h, *fresh(), T, "none", NMPC, substeps=0)
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*substeps"):
        capi.srbd_advance(h, *fresh()[:3], substeps=0)
    with pytest.raises(capi.SrbdQpError, match=r"\(-6\)"):  # the step's checks: SRBD_QP_ESETTINGS
        capi.srbd_rollout(h, *fresh(), T, "none", dict(NMPC, mu0=0.0))
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*constraints mode"):
        capi.srbd_rollout(h, *fresh(), T, "box_u", NMPC)
    h4 = capi.Handle(N, 4, 4, capacity=cap)
    with pytest.raises(capi.SrbdQpError, match=r"\(-2\)"):  # SRBD_QP_EDIM
        capi.srbd_rollout(h4, *fresh(), T, "none", NMPC)
    with pytest.raises(capi.SrbdQpError, match=r"\(-2\)"):
        capi.srbd_advance(h4, *fresh()[:3])
    small = capi.Handle(N, 12, 12, capacity=B - 1)
    with pytest.raises(capi.SrbdQpError, match=r"\(-5\)"):  # SRBD_QP_ECAPACITY
        capi.srbd_rollout(small, *fresh(), T, "none", NMPC)
    with pytest.raises(capi.SrbdQpError, match=r"\(-5\)"):
        capi.srbd_advance(small, *fresh()[:3])
    # nothing above ran a tick: the guesses a failed call was given are as they were
    a = fresh()
    with pytest.raises(capi.SrbdQpError):
        capi.srbd_rollout(h, *a, T, "none", NMPC, substeps=0)
    assert torch.equal(a[0], _dev(xs)) and torch.equal(a[2], _dev(x))
    # the window scratch: allocated by the first rollout with a plan, sized to the capacity
    capi.srbd_rollout(h, *fresh(), T, "none", NMPC)
    m0 = h.memory_bytes()
    plan_t = device_plan(capi, random_plan(sm, p, B, N + T - 1, 42))
    capi.srbd_rollout(h, *fresh(), T, "none", NMPC, plan=plan_t)
    m1 = h.memory_bytes()
    assert m1 - m0 == cap * (12 * (N + 1) + 8 * N) * 8, (m0, m1)
    capi.srbd_rollout(h, *fresh(), T, "none", NMPC, plan=plan_t)
    assert h.memory_bytes() == m1
