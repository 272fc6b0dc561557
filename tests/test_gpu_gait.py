"""The gait planner on the device (srbd_qp_srbd_gait_plan_f64: one tick's plan window from a
command, a gait and the measured state; srbd_qp_srbd_rollout_gait_f64: the closed loop that
replans every tick) against the host statement srbd_model.gait_plan, against the caller's own
loop over the three public entry points (bit for bit) and against the host closed loop of
tests/rollout_host.py with a gait."""
import ctypes as C

import numpy as np
import pytest

import gait_host as GH
import rollout_host as RH
from nmpc_plan_host import constant_plan
from srbd_device import (FIELDS, NMPC, SQP_MAX_LOOP, STEP_ATOL_U, STEP_ATOL_X, _dev, caller_loop, close, device_gait,
                         device_plan, handle)

pytestmark = pytest.mark.gpu


# ---- 1. the planner against the host statement ----
# (5, 1): a one-stage window, every touchdown clamped to j' = N; (5, 2): the smallest even N (the
# feet's 16-byte stores); (5, 33): odd N, scalar foot stores; (3, 70): 71 stages, two chunks of the
# scan; (70, 10): 18 blocks of four robots, the last one partial; (5, 511): the longest horizon
# whose staged poses fit four robots to a block (64 KiB of LDS); (2, 600): one robot per block.
@pytest.mark.parametrize("B,N", [(5, 1), (5, 2), (5, 33), (3, 70), (70, 10), (5, 511), (2, 600)])
def test_planner_matches_the_host_statement(pkg, B, N):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    p = sm.SrbdParams()
    h = handle(capi, N, B, "none")
    cmd, x, ref_pose, foot_now = GH.random_inputs(sm, p, B, 100 + N)
    scalar = dict(period=7, swing=(3, 2), offset=(1, 4))  # the _r arrays NULL: one gait for all
    for tick in (0, 10**12 + 3):
        period, swing, offset = GH.special_gaits(max(B, 5), N, tick, 200 + N)
        per_robot = dict(period=period[:B], swing=swing[:B], offset=offset[:B])
        for anchor in (0, 1):
            for ints in (per_robot, scalar):
                case = (tick, anchor, ints is scalar)
                g = sm.SrbdGait(hip=((0.02, -0.11), (0.01, 0.12)), ground_z=0.03, k_raibert=0.07,
                                fz_stance=250.0, fz_swing=1.5, anchor=anchor, **ints)
                want, want_pose, want_feet = sm.gait_plan(p, g, cmd, x, tick, ref_pose, foot_now, N)
                pose_t, feet_t = _dev(ref_pose), _dev(foot_now)
                got = capi.srbd_gait_plan(h, device_gait(capi, g), _dev(cmd), _dev(x), tick,
                                          pose_t, feet_t)
                h.synchronize()
                assert np.array_equal(got.fz_max.cpu().numpy(), want.fz_max), case
                for k in ("x_ref", "foot_r", "foot_l"):
                    close(getattr(got, k), getattr(want, k), (case, k))
                close(pose_t, want_pose, case)
                close(feet_t, want_feet, case)
                # bit identities on the device's own outputs
                assert torch.equal(feet_t[:, 0], got.foot_r[:, 0]) and torch.equal(feet_t[:, 1], got.foot_l[:, 0])
                assert torch.equal(pose_t, got.x_ref[:, 1, [6, 7, 2]]), case
                stance = torch.from_numpy(~GH.schedule(*[np.broadcast_to(np.asarray(v), s) for v, s in
                                                         zip((g.period, g.swing, g.offset), ((B,), (B, 2), (B, 2)))],
                                                       tick, N)[0][:, 0]).cuda()
                assert bool(stance.any()), case
                assert torch.equal(feet_t[stance], _dev(foot_now)[stance]), case
    # the per-robot gaits hold what the cases need (right foot of robots 0..4 at the last tick)
    swinging, j, down = GH.schedule(period[:B], swing[:B], offset[:B], tick, N)
    if B >= 5:
        assert down[0].all()                                  # a standing robot
        assert swinging[1, 0, 0]                              # in swing at stage 0
        assert not swinging[2, 0, 0] and j[2, 0, 0] == 0      # a touchdown exactly at stage 0
        assert swinging[4, :, 0].all() and j[4, 0, 0] > N     # a period above N: the clamp j' = N
        if N >= 6:  # a period below N: two touchdowns of one foot in the window
            assert len(set(j[3, :, 0][swinging[3, :, 0]].tolist())) >= 2


def test_the_reference_uses_the_model_roles_inertia(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N = 5, 4
    p = sm.SrbdParams()
    h = handle(capi, N, B, "none")
    cmd, x, ref_pose, foot_now = GH.random_inputs(sm, p, B, 300)
    Lbody = np.array(p.Lbody) * np.random.default_rng(301).uniform(0.7, 1.4, size=(B, 3))
    g = sm.SrbdGait(period=6, swing=(3, 3), offset=(0, 3), fz_stance=250.0)
    h.set_robots(model=capi.Robots(Lbody=_dev(Lbody)))
    got = capi.srbd_gait_plan(h, device_gait(capi, g), _dev(cmd), _dev(x), 2, _dev(ref_pose), _dev(foot_now))
    h.synchronize()
    want = sm.gait_plan(p, g, cmd, x, 2, ref_pose, foot_now, N, Lbody_z=Lbody[:, 2])[0]
    close(got.x_ref, want.x_ref, "x_ref")
    assert torch.equal(got.x_ref[:, :, 5], _dev(np.tile((Lbody[:, 2] * cmd[:, 2])[:, None], (1, N + 1))))
    default = sm.gait_plan(p, g, cmd, x, 2, ref_pose, foot_now, N)[0]
    assert not np.allclose(want.x_ref[:, :, 5], default.x_ref[:, :, 5], rtol=1e-3)


# ---- 2. a standing gait is the plan of tiled constants, and the step on it the same step ----
@pytest.mark.parametrize("N", [10, 33])
def test_standing_gait_is_the_constant_plan_on_the_device(pkg, N):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B = 6
    p = sm.SrbdParams()
    xr = np.array(p.x_ref, dtype=np.float64)
    g = sm.SrbdGait(period=4, swing=(0, 0), offset=(0, 2), fz_stance=p.fmax, fz_swing=1.0, anchor=0)
    cmd = np.tile(np.array([0.0, 0.0, 0.0, xr[8]]), (B, 1))
    ref_pose = np.tile(np.array([xr[6], xr[7], xr[2]]), (B, 1))
    foot_now = np.tile(np.array([p.foot_r, p.foot_l], dtype=np.float64), (B, 1, 1))
    xs, us, dx0 = sm.sample_trajectories(B, N, 400 + N, p)
    x = xs[:, 0] + dx0
    h = handle(capi, N, B, "none")
    pose_t, feet_t = _dev(ref_pose), _dev(foot_now)
    win = capi.srbd_gait_plan(h, device_gait(capi, g), _dev(cmd), _dev(x), 10**12 + 3, pose_t, feet_t)
    h.synchronize()
    const = device_plan(capi, constant_plan(sm, p, B, N))
    for k in FIELDS:
        assert torch.equal(getattr(win, k), getattr(const, k)), k
    assert torch.equal(pose_t, _dev(ref_pose)) and torch.equal(feet_t, _dev(foot_now))
    runs = []
    for plan in (win, const):
        a = [_dev(v) for v in (xs, us, x, np.ones(B))]
        it, cv = capi.srbd_nmpc(h, *a, "none", NMPC, SQP_MAX_LOOP, plan=plan)
        runs.append(a + [it, cv])
    for u, v in zip(*runs):
        assert torch.equal(u, v)
    assert int(runs[0][4].min()) >= 1


# ---- 3. the replanning rollout is the caller's loop over the three entry points, bit for bit ----
@pytest.mark.parametrize("alpha_reset", [0.0, 1.0])
@pytest.mark.parametrize("constraints", ["none", "box_u", "cone"])
def test_gait_rollout_is_the_callers_loop_bit_for_bit(pkg, constraints, alpha_reset):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N, tick0 = 6, 10, 10**12 + 3
    p = sm.SrbdParams()
    h = handle(capi, N, B, constraints)
    for T in (3, 1):
        xs, us, x, alpha, gait, cmd, ref_pose, foot_now = GH.walking_case(sm, p, B, N, T, 41)
        cmd[:, 1:] += np.random.default_rng(44).uniform(-0.1, 0.1, size=(B, 1, 4))  # a new command at tick 1
        gait_t, cmd_t = device_gait(capi, gait), _dev(cmd)
        wrench_t = _dev(np.random.default_rng(43).uniform(-15.0, 15.0, size=(B, T, 6)))
        a = [_dev(v) for v in (xs, us, x, alpha, ref_pose, foot_now)]
        logs_a = capi.srbd_rollout_gait(h, gait_t, cmd_t, *a, T, tick0, constraints, NMPC, SQP_MAX_LOOP,
                                        wrench=wrench_t, substeps=2, alpha_reset=alpha_reset)
        b = [_dev(v) for v in (xs, us, x, alpha, ref_pose, foot_now)]
        logs_b = caller_loop(capi, h, B, N, T, constraints, *b[:4], wrench_t, 2, alpha_reset, gait_t=gait_t,
                             cmd_t=cmd_t, pose=b[4], feet=b[5], tick0=tick0)
        names = ("xs", "us", "x", "alpha", "ref_pose", "foot_now", "x_log", "u_log", "sqp_iter_log",
                 "converged_log", "foot_log", "fz_log")
        for name, u, v in zip(names, a + list(logs_a), b + list(logs_b)):
            assert bool(torch.isfinite(u.double()).all()), (T, name)
            assert torch.equal(u, v), (T, name)
        assert int(logs_a[2].min()) >= 1  # the steps ran
        assert not torch.equal(a[0], _dev(xs)) and not torch.equal(a[4], _dev(ref_pose))


def test_gait_rollout_of_zero_ticks_touches_nothing(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N = 6, 10
    p = sm.SrbdParams()
    xs, us, x, alpha, gait, cmd, ref_pose, foot_now = GH.walking_case(sm, p, B, N, 0, 41)
    state = (xs, us, x, alpha, ref_pose, foot_now)
    a = [_dev(v) for v in state]
    h = handle(capi, N, B, "none")
    logs = capi.srbd_rollout_gait(h, device_gait(capi, gait), _dev(cmd), *a, 0, 5, "none", NMPC, SQP_MAX_LOOP,
                                  alpha_reset=1.0)
    for u, v in zip(a, state):
        assert torch.equal(u, _dev(v))
    assert logs[0].shape == (B, 1, 12) and torch.equal(logs[0][:, 0], a[2])
    assert logs[4].shape == (B, 0, 2, 3) and logs[5].shape == (B, 0, 2)


# ---- 4. the replanning rollout against the host gait loop ----
# GAIT_SEED was chosen on the CPU: with it the host loop's smallest comparison margin over all
# ticks is >= 1e-6 and at least two distinct SQP iteration counts occur, in all four cases below
# (both are asserted).
GAIT_SEED = 28  # scripts/rollout_sensitivity.py --gait --search 20 32: margins 1.0e-6 .. 1.5e-6
# d_t: the largest change of the host gait loop's x_log[t] / u_log[t-1] when the
# loop is rerun with x, xs, us perturbed by relative 1e-7, the plan following through the feedback;
# measured on the CPU (scripts/rollout_sensitivity.py --gait --seed 28) per case (constraints,
# alpha_reset), t = 1..4: (d_t of x, d_t of u).
D_T = {
    ("none", 0.0): ((3.2e-07, 5.6e-07, 6.9e-07, 7.4e-07), (2.9e-05, 2.2e-05, 1.8e-05, 1.4e-05)),
    ("none", 1.0): ((3.2e-07, 5.6e-07, 6.9e-07, 7.4e-07), (2.9e-05, 2.2e-05, 1.8e-05, 1.4e-05)),
    ("box_u", 0.0): ((3.3e-07, 5.7e-07, 7.1e-07, 7.6e-07), (2.9e-05, 2.3e-05, 1.8e-05, 1.4e-05)),
    ("box_u", 1.0): ((3.3e-07, 5.7e-07, 7.1e-07, 7.6e-07), (2.9e-05, 2.3e-05, 1.8e-05, 1.4e-05)),
}


@pytest.mark.parametrize("alpha_reset", [0.0, 1.0])
@pytest.mark.parametrize("constraints", ["none", "box_u"])
def test_gait_rollout_matches_the_host_gait_loop(pkg, oracle, constraints, alpha_reset):
    capi, sm = pkg.capi, pkg.srbd_model
    B, N, T = 4, 10, 4
    p = sm.SrbdParams()
    xs, us, x, alpha, gait, cmd, ref_pose, foot_now = GH.walking_case(sm, p, B, N, T, GAIT_SEED)
    host = RH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, SQP_MAX_LOOP, constraints, p=p, gait=gait, cmd=cmd,
                          ref_pose=ref_pose, foot_now=foot_now, alpha_reset=alpha_reset)
    # conditions on the inputs: no host decision on a boundary, robots that stop at different
    # iterations, and every robot has a liftoff and a touchdown inside the four ticks
    assert host["margin"] >= 1e-6, host["margin"]
    assert len(set(host["sqp_iter"].ravel().tolist())) >= 2, host["sqp_iter"]
    swing = host["fz_log"] == gait.fz_swing  # [B][T][2]
    lift = (~swing[:, :-1] & swing[:, 1:]).any(axis=(1, 2))
    land = (swing[:, :-1] & ~swing[:, 1:]).any(axis=(1, 2))
    assert lift.all() and land.all(), (lift, land)
    h = handle(capi, N, B, constraints)
    a = [_dev(v) for v in (xs, us, x, alpha, ref_pose, foot_now)]
    x_log, u_log, it_log, cv_log, foot_log, fz_log = capi.srbd_rollout_gait(
        h, device_gait(capi, gait), _dev(cmd), *a, T, 0, constraints, NMPC, SQP_MAX_LOOP, alpha_reset=alpha_reset)
    x_log, u_log = x_log.cpu().numpy(), u_log.cpu().numpy()
    print("sqp_iter device", it_log.cpu().numpy().tolist(), "host", host["sqp_iter"].tolist())
    for t in range(1, T + 1):
        print(f"tick {t}: max |x_log - host| {np.abs(x_log[:, t] - host['x_log'][:, t]).max():.3e}, "
              f"max |u_log - host| {np.abs(u_log[:, t - 1] - host['u_log'][:, t - 1]).max():.3e}, "
              f"max |foot_log - host| {np.abs(foot_log[:, t - 1].cpu().numpy() - host['foot_log'][:, t - 1]).max():.3e}")
    assert np.array_equal(it_log.cpu().numpy(), host["sqp_iter"])
    assert np.array_equal(cv_log.cpu().numpy(), host["converged"])
    assert np.array_equal(a[3].cpu().numpy(), host["alpha"])
    assert np.array_equal(fz_log.cpu().numpy(), host["fz_log"])
    assert np.array_equal(x_log[:, 0], x)
    close(foot_log[:, 0], host["foot_log"][:, 0], "tick 0's feet")  # planned from the same x
    dt_x, dt_u = D_T[(constraints, alpha_reset)]
    for t in range(1, T + 1):
        # tick 1 is one step: the step test's tolerance; later ticks compound, by at most d_t
        ax = STEP_ATOL_X if t == 1 else max(STEP_ATOL_X, 10.0 * dt_x[t - 1])
        au = STEP_ATOL_U if t == 1 else max(STEP_ATOL_U, 10.0 * dt_u[t - 1])
        np.testing.assert_allclose(x_log[:, t], host["x_log"][:, t], rtol=1e-7, atol=ax, err_msg=f"x {t}")
        np.testing.assert_allclose(u_log[:, t - 1], host["u_log"][:, t - 1], rtol=1e-7, atol=au, err_msg=f"u {t}")
    assert np.array_equal(a[2].cpu().numpy(), x_log[:, T])


# ---- 5. the feedback is felt ----
def test_a_push_moves_the_swinging_foots_target(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N, T = 4, 10, 5
    p = sm.SrbdParams()
    xs, us, x, alpha, _, cmd, ref_pose, foot_now = GH.walking_case(sm, p, B, N, T, GAIT_SEED)
    # the right foot swings over ticks 1..3 (phi = 0, 1, 2); the left lands at tick 1, lifts at 4
    gait = sm.SrbdGait(period=6, swing=(3, 3), offset=(5, 2), k_raibert=0.1, fz_stance=250.0, anchor=1)
    Fy = np.array([40.0, -40.0, 30.0, -30.0])
    wrench = np.zeros((B, T, 6))
    pushed = wrench.copy()
    pushed[:, 1, 4] = Fy
    h = handle(capi, N, B, "none")
    gait_t, cmd_t = device_gait(capi, gait), _dev(cmd)
    logs = []
    for w in (wrench, pushed):
        a = [_dev(v) for v in (xs, us, x, alpha, ref_pose, foot_now)]
        logs.append(capi.srbd_rollout_gait(h, gait_t, cmd_t, *a, T, 0, "none", NMPC, SQP_MAX_LOOP, wrench=_dev(w),
                                           alpha_reset=1.0))
    (xa, ua, _, _, fa, za), (xb, ub, _, _, fb, zb) = logs
    assert torch.equal(za, zb)
    assert torch.equal(za[:, :, 0] == gait.fz_swing,
                       torch.tensor([False, True, True, True, False], device="cuda").expand(B, T))
    # up to and including tick 1's window nothing differs: its planner has not seen the push
    assert torch.equal(xa[:, :2], xb[:, :2]) and torch.equal(ua[:, :2], ub[:, :2])
    assert torch.equal(fa[:, :2], fb[:, :2])
    # from tick 2 on the swinging (right) foot's target moves with the push
    dy = (fb[:, 2:4, 0, 1] - fa[:, 2:4, 0, 1]).cpu().numpy()
    print("right foot target dy at ticks 2, 3:", dy.tolist())
    assert (np.sign(dy) == np.sign(Fy)[:, None]).all(), dy
    # the stance (left) foot: latched at its touchdown in tick 1, the same bits until it lifts off
    assert torch.equal(fa[:, 1:4, 1], fb[:, 1:4, 1])
    assert torch.equal(fa[:, 1, 1], fa[:, 2, 1]) and torch.equal(fa[:, 1, 1], fa[:, 3, 1])


# ---- 6. errors, and the window scratch ----
def test_gait_errors_and_scratch(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N, T = 4, 10, 2
    p = sm.SrbdParams()
    xs, us, x, alpha, gait, cmd, ref_pose, foot_now = GH.walking_case(sm, p, B, N, T, 41)
    state = (xs, us, x, np.ones(B), ref_pose, foot_now)
    fresh = lambda: [_dev(v) for v in state]
    cap = 8
    h = capi.Handle(N, 12, 12, capacity=cap)
    good = dict(period=6, swing=(3, 3), offset=(0, 3), fz_stance=250.0, fz_swing=1.0)
    per_t = torch.full((B,), 6, dtype=torch.int32, device="cuda")

    def plan_call(gait_t, tick=0, handle_=h):
        return capi.srbd_gait_plan(handle_, gait_t, _dev(cmd[:, 0]), _dev(x), tick, _dev(ref_pose), _dev(foot_now))

    def roll_call(gait_t, a, handle_=h, tick0=0, **kw):
        return capi.srbd_rollout_gait(handle_, gait_t, _dev(cmd), *a, T, tick0, "none", NMPC, **kw)

    bad_gaits = [(dict(good, period=0), "period"), (dict(good, swing=(3, 6)), "swing"),
                 (dict(good, swing=(-1, 3)), "swing"), (dict(good, offset=(0, -1)), "offset"),
                 (dict(good, fz_swing=0.0), "fz_swing"), (dict(good, fz_stance=1.0), "fz_stance")]
    for kw, word in bad_gaits:  # SRBD_QP_EINVAL, from both entry points
        with pytest.raises(capi.SrbdQpError, match=rf"\(-1\).*{word}"):
            plan_call(capi.Gait(**kw))
        with pytest.raises(capi.SrbdQpError, match=rf"\(-1\).*{word}"):
            roll_call(capi.Gait(**kw), fresh())
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*tick"):
        plan_call(capi.Gait(**good), tick=-1)
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*tick"):
        roll_call(capi.Gait(**good), fresh(), tick0=-1)
    # a scalar is checked only where its _r array is NULL: with period_r the scalar period (and
    # the swing's upper end, which belongs to it) is not read
    plan_call(capi.Gait(**dict(good, period=per_t)))
    # NULL pointers (the three _r arrays aside)
    L, mp, gs = capi.lib(), capi.default_model_params(), capi.Gait(**good).struct(B)
    bufs = [_dev(cmd[:, 0]), _dev(x), _dev(ref_pose), _dev(foot_now)] + [
        torch.zeros(B, N + 1, 12, dtype=torch.float64, device="cuda"), torch.zeros(B, N, 3, dtype=torch.float64, device="cuda"),
        torch.zeros(B, N, 3, dtype=torch.float64, device="cuda"), torch.zeros(B, N, 2, dtype=torch.float64, device="cuda")]
    ptrs = [C.c_void_p(t.data_ptr()) for t in bufs]
    call = lambda q, hp=h.ptr, b=B, g=C.byref(gs): L.srbd_qp_srbd_gait_plan_f64(hp, b, C.byref(mp), g, q[0], q[1], 0,
                                                                               *q[2:], None)
    for i in range(len(ptrs)):
        assert call(ptrs[:i] + [None] + ptrs[i + 1:]) == -1, i
    assert call(ptrs, g=None) == -1
    assert call(ptrs, b=0) == 0  # batch == 0: SRBD_QP_OK
    assert call(ptrs) == 0
    h.synchronize()
    # the rollout's own checks, the step's, the dims and the capacity
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*substeps"):
        roll_call(capi.Gait(**good), fresh(), substeps=0)
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*alpha_reset"):
        roll_call(capi.Gait(**good), fresh(), alpha_reset=-1.0)
    with pytest.raises(capi.SrbdQpError, match=r"\(-6\)"):  # SRBD_QP_ESETTINGS
        capi.srbd_rollout_gait(h, capi.Gait(**good), _dev(cmd), *fresh(), T, 0, "none", dict(NMPC, mu0=0.0))
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*constraints mode"):
        capi.srbd_rollout_gait(h, capi.Gait(**good), _dev(cmd), *fresh(), T, 0, "box_u", NMPC)
    h4 = capi.Handle(N, 4, 4, capacity=cap)
    small = capi.Handle(N, 12, 12, capacity=B - 1)
    for hh, code in ((h4, -2), (small, -5)):  # SRBD_QP_EDIM, SRBD_QP_ECAPACITY
        with pytest.raises(capi.SrbdQpError, match=rf"\({code}\)"):
            plan_call(capi.Gait(**good), handle_=hh)
        with pytest.raises(capi.SrbdQpError, match=rf"\({code}\)"):
            roll_call(capi.Gait(**good), fresh(), handle_=hh)
    # a failed call leaves the state as it was
    for kw in (dict(substeps=0), dict(tick0=-1)):
        a = fresh()
        with pytest.raises(capi.SrbdQpError):
            roll_call(capi.Gait(**good), a, **kw)
        for u, v in zip(a, state):
            assert torch.equal(u, _dev(v))
    # the window scratch is the plan rollout's: allocated once, sized to the capacity
    capi.srbd_rollout(h, *fresh()[:4], T, "none", NMPC)
    m0 = h.memory_bytes()
    roll_call(device_gait(capi, gait), fresh())
    m1 = h.memory_bytes()
    assert m1 - m0 == cap * (12 * (N + 1) + 8 * N) * 8, (m0, m1)
    roll_call(device_gait(capi, gait), fresh())
    assert h.memory_bytes() == m1
    long_plan = device_plan(capi, constant_plan(sm, p, B, N + T - 1))
    capi.srbd_rollout(h, *fresh()[:4], T, "none", NMPC, plan=long_plan)
    assert h.memory_bytes() == m1
