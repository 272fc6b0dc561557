"""The closed loop (srbd_qp_srbd_advance_f64 / srbd_qp_srbd_rollout_f64) without a GPU: the two
entry points exist and validate, the host model's plant_step and shift_guess are the operations
include/srbd_qp.h states, the host closed loop of tests/rollout_host.py is the host SQP loop
when it runs one tick, and with every feature on its tick 0 is the primitives in order."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import contact_host as CH
import nmpc_plan_host as PH
import robots_host as BH
import rollout_host as RH
import terrain_host as TH
from srbd_device import NMPC

ROLLOUT_SYMBOLS = ("srbd_qp_srbd_advance_f64", "srbd_qp_srbd_rollout_f64")
EINVAL = -1  # SRBD_QP_EINVAL


def random_feet(p, B, seed):
    rng = np.random.default_rng(seed)
    return (np.array(p.foot_r) + rng.uniform(-0.15, 0.15, size=(B, 3)),
            np.array(p.foot_l) + rng.uniform(-0.15, 0.15, size=(B, 3)))


def test_rollout_entry_points_are_exported_and_reject_null_arguments(pkg):
    capi = pkg.capi
    assert set(ROLLOUT_SYMBOLS) <= set(capi.exported_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ROLLOUT_SYMBOLS) <= exported
    L = capi.lib()
    p, ls, st = capi.default_model_params(), capi.default_linesearch(), capi.settings_struct()
    adv, roll = capi.AdvanceStruct(1, None), capi.RolloutStruct(ticks=1, substeps=1)
    assert L.srbd_qp_srbd_advance_f64(None, 1, C.byref(p), None, C.byref(adv), *([None] * 5)) == EINVAL
    assert L.srbd_qp_srbd_rollout_f64(None, 1, C.byref(p), None, C.byref(ls), C.byref(st), 0, 15,
                                      C.byref(roll), *([None] * 4)) == EINVAL
    assert L.srbd_qp_abi_version() == 12  # additive to ABI 12


def test_rollout_binding_checks_its_tensors(pkg):
    """srbd_rollout hands Plan.struct the plan's stage count P, so a plan shaped for the horizon
    is rejected before the library sees it."""
    import torch
    capi = pkg.capi
    B, N, T = 2, 5, 3
    f = dict(dtype=torch.float64)
    xs, us = torch.zeros(B, N + 1, 12, **f), torch.zeros(B, N, 12, **f)
    x, alpha = torch.zeros(B, 12, **f), torch.ones(B, **f)
    short = capi.Plan(x_ref=torch.zeros(B, N + 1, 12, **f))
    with pytest.raises(ValueError, match="x_ref has shape"):
        capi.srbd_rollout(None, xs, us, x, alpha, T, plan=short)
    with pytest.raises(ValueError, match="x_ref has shape"):
        capi.srbd_rollout(None, xs, us, x, alpha, T, plan=short, plan_stages=N + T + 1)
    with pytest.raises(ValueError, match="wrench has shape"):
        capi.srbd_rollout(None, xs, us, x, alpha, T, wrench=torch.zeros(B, 6, **f))
    with pytest.raises(ValueError, match="x has shape"):
        capi.srbd_advance(None, xs, us, x=torch.zeros(B, 6, **f))


def test_plant_step_is_the_shooting_model(pkg):
    """One substep, no wrench: the RK4 of shooting_dynamics (b with x_next = 0), bit for bit."""
    sm = pkg.srbd_model
    B = 6
    p = sm.SrbdParams()
    xs, us, _ = sm.sample_trajectories(B, 1, 77, p)
    x, u = xs[:, 0], us[:, 0]
    fr, fl = random_feet(p, B, 78)
    for feet in (dict(), dict(foot_r=fr, foot_l=fl), dict(foot_l=fl)):
        plan = sm.SrbdPlan(**feet) if feet else None
        want = sm.shooting_dynamics(x, np.zeros_like(x), u, p, plan)[2]
        got = sm.plant_step(x, u, p, **feet)
        assert np.array_equal(got, want), feet.keys()
    assert not np.array_equal(sm.plant_step(x, u, p, foot_r=fr), sm.plant_step(x, u, p))
    with pytest.raises(ValueError):
        sm.plant_step(x, u, p, substeps=0)


def test_zero_wrench_is_no_wrench(pkg):
    sm = pkg.srbd_model
    B = 6
    p = sm.SrbdParams()
    xs, us, _ = sm.sample_trajectories(B, 1, 79, p)
    for substeps in (1, 3):
        a = sm.plant_step(xs[:, 0], us[:, 0], p, substeps=substeps)
        b = sm.plant_step(xs[:, 0], us[:, 0], p, wrench=np.zeros((B, 6)), substeps=substeps)
        assert np.array_equal(a, b)
    # and a wrench is felt: the velocity rows are affine in the force
    F = np.array([0.0, 0.0, 0.0, 30.0, -20.0, 45.0])
    c = sm.plant_step(xs[:, 0], us[:, 0], p, wrench=np.tile(F, (B, 1)))
    a = sm.plant_step(xs[:, 0], us[:, 0], p)
    np.testing.assert_allclose(c[:, 9:12] - a[:, 9:12], np.tile(p.dt * F[3:] / p.mass, (B, 1)), rtol=1e-12)


def test_plant_step_has_order_four(pkg):
    """Against 64 substeps as the truth, halving the step divides the error by 16 (order 4);
    the test allows a factor of 2 for rounding: err(2) < err(1) / 8."""
    sm = pkg.srbd_model
    B = 6
    p = sm.SrbdParams()
    xs, us, _ = sm.sample_trajectories(B, 1, 80, p)
    rng = np.random.default_rng(81)
    w = rng.uniform(-20.0, 20.0, size=(B, 6))
    fr, fl = random_feet(p, B, 82)
    step = lambda n: sm.plant_step(xs[:, 0], us[:, 0], p, fr, fl, w, n)
    truth = step(64)
    e1 = np.abs(step(1) - truth).max()
    e2 = np.abs(step(2) - truth).max()
    print(f"RK4 error: substeps 1 {e1:.3e}, substeps 2 {e2:.3e}, ratio {e1 / e2:.2f}")
    assert e1 > 0.0 and e2 < e1 / 8.0, (e1, e2)


@pytest.mark.parametrize("N", [1, 2, 7])
@pytest.mark.parametrize("with_plan", [False, True])
def test_shift_guess(pkg, N, with_plan):
    sm = pkg.srbd_model
    B = 4
    p = sm.SrbdParams()
    xs, us, _ = sm.sample_trajectories(B, N, 90 + N, p)
    plan = None
    if with_plan:
        rng = np.random.default_rng(91)
        plan = sm.SrbdPlan(foot_r=np.array(p.foot_r) + rng.uniform(-0.15, 0.15, size=(B, N, 3)),
                           foot_l=np.array(p.foot_l) + rng.uniform(-0.15, 0.15, size=(B, N, 3)))
    xs0, us0 = xs.copy(), us.copy()
    xn, un = sm.shift_guess(xs, us, p, plan)
    assert np.array_equal(xs, xs0) and np.array_equal(us, us0)  # the inputs are left alone
    assert xn.shape == xs.shape and un.shape == us.shape
    assert np.array_equal(xn[:, :N], xs[:, 1:])          # rows 0..N-1 are bit copies
    assert np.array_equal(un[:, :N - 1], us[:, 1:])      # rows 0..N-2
    assert np.array_equal(un[:, N - 1], us[:, N - 1])    # the last input stays
    # the new last stage: one model step from the old one with the old last input and the feet
    # of stage N-1 ...
    last = None if plan is None else sm.SrbdPlan(foot_r=plan.foot_r[:, N - 1], foot_l=plan.foot_l[:, N - 1])
    want = sm.shooting_dynamics(xs[:, N], np.zeros((B, 12)), us[:, N - 1], p, last)[2]
    assert np.array_equal(xn[:, N], want)
    # ... so its shooting defect is the model's own b for (old xs[N], new xs[N], us[N-1]): zero
    b = sm.shooting_dynamics(xs[:, N], xn[:, N], un[:, N - 1], p, last)[2]
    assert np.array_equal(b, np.zeros((B, 12)))
    if with_plan:  # the feet matter
        assert not np.array_equal(xn[:, N], sm.shift_guess(xs, us, p, None)[0][:, N])


@pytest.mark.parametrize("alpha_reset", [0.0, 1.0])
def test_one_tick_of_the_host_loop_is_the_host_sqp_loop(pkg, oracle, alpha_reset):
    sm = pkg.srbd_model
    B, N, T = 2, 6, 1
    p = sm.SrbdParams()
    xs, us, x, alpha, plan = RH.walking_case(sm, p, B, N, T, 5)
    out = RH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, 15, "none", p=p, plan=plan,
                         alpha_reset=alpha_reset)
    w = RH.window(sm, plan, 0, N)
    assert w.x_ref.shape == (B, N + 1, 12) and w.foot_r.shape == (B, N, 3) and w.fz_max.shape == (B, N, 2)
    for i in range(B):
        a0 = alpha_reset if alpha_reset > 0.0 else float(alpha[i])
        hx, hu, ha, hit, hcv, hm = PH.sqp_loop(sm, oracle, p, w.robot(i), xs[i], us[i], x[i], a0, NMPC,
                                               15, "none")
        sx, su, sa, sit, scv, smg = out["steps"][0][i]
        assert np.array_equal(sx, hx) and np.array_equal(su, hu)
        assert (sa, sit, scv, smg) == (ha, hit, hcv, hm)
        assert out["sqp_iter"][i, 0] == hit and bool(out["converged"][i, 0]) == hcv
        assert out["alpha"][i] == ha
        assert np.array_equal(out["u_log"][i, 0], hu[0])
    assert np.array_equal(out["x_log"][:, 0], x)
    hxs = np.stack([r[0] for r in out["steps"][0]])
    hus = np.stack([r[1] for r in out["steps"][0]])
    assert np.array_equal(out["x_log"][:, 1], sm.plant_step(x, hus[:, 0], p, w.foot_r[:, 0], w.foot_l[:, 0]))
    sx, su = sm.shift_guess(hxs, hus, p, w)
    assert np.array_equal(out["xs"], sx) and np.array_equal(out["us"], su)


def test_tick_0_of_the_combined_loop_is_the_primitives_in_order(pkg, oracle):
    """A gait on terrain, a contact with that terrain as the true ground and per-robot plants,
    all at once: tick 0 is gait_plan(terrain=), the host SQP loop per robot, contact_flags,
    plant_step(contact=) per robot and shift_guess, called directly in that order."""
    sm = pkg.srbd_model
    B, N, T = 2, 6, 2
    p = sm.SrbdParams()
    xs, us, x, alpha, gait, cmd, ref_pose, foot_now = TH.stairs_case(sm, p, B, N, T, 5)
    ter = TH.stairs_terrain(sm)
    contact = sm.SrbdContact(mu=0.3, fz_hi=400.0, fz_contact=0.5 * (gait.fz_swing + gait.fz_stance),
                             ground_z=gait.ground_z, ground=ter, z_min=0.3, cos_tilt_min=0.5)
    model = [p] * B
    plant = BH.draw_plant(model, 6)
    out = RH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, 15, "none", model=model, plant=plant, gait=gait,
                         cmd=cmd, ref_pose=ref_pose, foot_now=foot_now, tick0=4, terrain=ter, contact=contact,
                         state=CH.zero_state(B))
    assert set(out) >= {"foot_log", "windows", "q_log", "poses", "state", "fallen_log", "values"}
    # 1. the window
    w, pose, feet = sm.gait_plan(p, gait, cmd[:, 0], x, 4, ref_pose, foot_now, N, terrain=ter)
    for k in RH.FIELDS:
        assert np.array_equal(getattr(out["windows"][0], k), getattr(w, k)), k
    assert np.array_equal(out["poses"][0], pose) and np.array_equal(out["feet"][0], feet)
    assert np.array_equal(out["foot_log"][:, 0], feet) and np.array_equal(out["fz_log"][:, 0], w.fz_max[:, 0])
    # 2. the SQP loop per robot
    res = [PH.sqp_loop(sm, oracle, model[i], w.robot(i), xs[i], us[i], x[i], float(alpha[i]), NMPC, 15, "none")
           for i in range(B)]
    for i, (hx, hu, ha, hit, hcv, hm) in enumerate(res):
        sx, su, sa, sit, scv, smg = out["steps"][0][i]
        assert np.array_equal(sx, hx) and np.array_equal(su, hu)
        assert (sa, sit, scv, smg) == (ha, hit, hcv, hm)
        assert out["sqp_iter"][i, 0] == hit and bool(out["converged"][i, 0]) == hcv
    hxs, hus = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    # 3. the contact flags, 4. the plant step per robot with the true robot's parameters
    on = sm.contact_flags(contact, w.fz_max[:, 0], B)
    assert not on.all() and on.any()  # a swing foot and a stance foot at tick 0
    state = CH.zero_state(B)
    for i in range(B):
        x1, ua, st = sm.plant_step(x[i:i + 1], hus[i:i + 1, 0], plant[i], w.foot_r[i:i + 1, 0], w.foot_l[i:i + 1, 0],
                                   contact=RH.robot_contact(contact, i), in_contact=on[i:i + 1],
                                   state={k: v[i:i + 1] for k, v in state.items()})
        assert np.array_equal(out["x_log"][i, 1], x1[0]) and np.array_equal(out["u_log"][i, 0], ua[0])
        assert not np.array_equal(ua[0], hus[i, 0])  # the applied input is the projected one
        for k in state:
            state[k][i] = st[k][0]
    assert np.array_equal(out["fallen_log"][:, 0], state["fallen"])
    for got, want in zip(out["values"][0], sm.fall_values(out["x_log"][:, 1], contact)):
        assert np.array_equal(got, want)
    # 5. the shift, with the model's parameters, after which tick 1 starts
    parts = [sm.shift_guess(hxs[i:i + 1], hus[i:i + 1], model[i], sm.SrbdPlan(*[getattr(w, k)[i:i + 1] for k in RH.FIELDS]))
             for i in range(B)]
    # (tick 1's SQP loop starts from the shifted guess: its result pins the shift)
    w1 =sm.gait_plan(p, gait, cmd[:, 1], out["x_log"][:, 1], 5, pose, feet, N, terrain=ter)[0]
    for k in RH.FIELDS:
        assert np.array_equal(getattr(out["windows"][1], k), getattr(w1, k)), k
    for i in range(B):
        r = PH.sqp_loop(sm, oracle, model[i], w1.robot(i), parts[i][0][0], parts[i][1][0], out["x_log"][i, 1],
                        out["steps"][0][i][2], NMPC, 15, "none")
        assert np.array_equal(out["steps"][1][i][0], r[0]) and np.array_equal(out["steps"][1][i][1], r[1])
