"""The gait planner (srbd_qp_srbd_gait_plan_f64 / srbd_qp_srbd_rollout_gait_f64) without a GPU:
the entry points exist and validate, and the host statement srbd_model.gait_plan has the
properties include/srbd_qp.h states: a standing gait is the constant plan, the contact schedule
is the integer formula, successive windows agree, the feedback moves the footholds and nothing
else, and one tick of tests/rollout_host.py's loop with a gait is gait_plan followed by the host
SQP loop."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import gait_host as GH
import nmpc_plan_host as PH
import rollout_host as RH
from gait_host import rot
from srbd_device import FIELDS, NMPC

GAIT_SYMBOLS = ("srbd_qp_srbd_gait_plan_f64", "srbd_qp_srbd_rollout_gait_f64")
EINVAL = -1  # SRBD_QP_EINVAL


def feet_of(plan):
    return np.stack([plan.foot_r, plan.foot_l], axis=2)  # [B][N][2][3]


# ---- 1. the entry points ----
def test_gait_entry_points_are_exported_and_reject_null_arguments(pkg):
    capi = pkg.capi
    assert set(GAIT_SYMBOLS) <= set(capi.exported_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(GAIT_SYMBOLS) <= exported
    L = capi.lib()
    p, ls, st = capi.default_model_params(), capi.default_linesearch(), capi.settings_struct()
    gs = capi.Gait(period=6, swing=(3, 3), offset=(0, 3)).struct(1)
    roll, gio = capi.RolloutStruct(ticks=1, substeps=1), capi.RolloutGaitStruct()
    assert L.srbd_qp_srbd_gait_plan_f64(None, 1, C.byref(p), C.byref(gs), None, None, 0, *([None] * 7)) == EINVAL
    assert L.srbd_qp_srbd_rollout_gait_f64(None, 1, C.byref(p), C.byref(gs), C.byref(gio), C.byref(ls),
                                           C.byref(st), 0, 15, C.byref(roll), *([None] * 4)) == EINVAL
    assert L.srbd_qp_abi_version() == 12  # additive to ABI 12


# ---- 2. the bindings check their tensors before the library is called ----
def test_gait_bindings_check_their_tensors(pkg):
    import torch
    capi = pkg.capi
    B, N, T = 2, 5, 3
    f = dict(dtype=torch.float64)
    z = lambda *shape: torch.zeros(*shape, **f)
    gait = capi.Gait(period=6, swing=(3, 3), offset=(0, 3))
    good = dict(cmd=z(B, 4), x=z(B, 12), ref_pose=z(B, 3), foot_now=z(B, 2, 3))
    for name, bad in (("cmd", z(B, 3)), ("ref_pose", z(B, 2)), ("foot_now", z(B, 6)), ("x", z(B, 6))):
        with pytest.raises(ValueError, match=f"{name} has shape"):
            capi.srbd_gait_plan(None, gait, tick=0, **dict(good, **{name: bad}))
    xs, us, alpha = z(B, N + 1, 12), z(B, N, 12), torch.ones(B, **f)
    roll = dict(good, cmd=z(B, T, 4))
    for name, bad in (("cmd", z(B, 4)), ("cmd", z(B, T + 1, 4)), ("ref_pose", z(B, 2)), ("foot_now", z(B, 6))):
        a = dict(roll, **{name: bad})
        with pytest.raises(ValueError, match=f"{name} has shape"):
            capi.srbd_rollout_gait(None, gait, a["cmd"], xs, us, a["x"], alpha, a["ref_pose"], a["foot_now"], T)
    with pytest.raises(ValueError, match="period has shape"):
        capi.srbd_gait_plan(None, capi.Gait(period=torch.ones(B + 1, dtype=torch.int32)), tick=0, **good)
    with pytest.raises(ValueError, match="swing must be a torch.int32"):
        capi.srbd_gait_plan(None, capi.Gait(swing=torch.ones(B, 2, dtype=torch.int64)), tick=0, **good)


# ---- 3. a standing gait is the plan of tiled constants ----
def standing(sm, p, B):
    xr = np.array(p.x_ref, dtype=np.float64)
    gait = sm.SrbdGait(period=4, swing=(0, 0), offset=(0, 2), fz_stance=p.fmax, fz_swing=1.0, anchor=0)
    cmd = np.tile(np.array([0.0, 0.0, 0.0, xr[8]]), (B, 1))
    ref_pose = np.tile(np.array([xr[6], xr[7], xr[2]]), (B, 1))
    foot_now = np.tile(np.array([p.foot_r, p.foot_l], dtype=np.float64), (B, 1, 1))
    return gait, cmd, ref_pose, foot_now


@pytest.mark.parametrize("N", [1, 7])
def test_a_standing_gait_is_the_constant_plan(pkg, N):
    sm = pkg.srbd_model
    B = 3
    p = sm.SrbdParams()
    gait, cmd, ref_pose, foot_now = standing(sm, p, B)
    x = sm.sample_trajectories(B, N, 3, p)[0][:, 0]  # the measured state does not matter
    for tick in (0, 5, 10**12 + 3):
        plan, pose, feet = sm.gait_plan(p, gait, cmd, x, tick, ref_pose, foot_now, N)
        assert np.array_equal(plan.x_ref, np.tile(np.array(p.x_ref, dtype=np.float64), (B, N + 1, 1)))
        assert np.array_equal(plan.foot_r, np.tile(np.array(p.foot_r, dtype=np.float64), (B, N, 1)))
        assert np.array_equal(plan.foot_l, np.tile(np.array(p.foot_l, dtype=np.float64), (B, N, 1)))
        assert np.array_equal(plan.fz_max, np.full((B, N, 2), float(p.fmax)))
        assert np.array_equal(pose, ref_pose) and np.array_equal(feet, foot_now)


# ---- 4. the contact schedule ----
@pytest.mark.parametrize("tick", [0, 7, 10**12 + 3])
def test_contact_schedule_is_the_integer_formula(pkg, tick):
    sm = pkg.srbd_model
    B, N = 12, 9
    p = sm.SrbdParams()
    period, swing, offset = GH.special_gaits(B, N, tick, 50)
    assert period.min() < N < period.max()  # periods below and above the horizon
    gait = sm.SrbdGait(period=period, swing=swing, offset=offset, fz_stance=250.0, fz_swing=2.0)
    cmd, x, ref_pose, foot_now = GH.random_inputs(sm, p, B, 51)
    plan = sm.gait_plan(p, gait, cmd, x, tick, ref_pose, foot_now, N)[0]
    swinging = GH.schedule(period, swing, offset, tick, N)[0]
    assert np.array_equal(plan.fz_max, np.where(swinging, 2.0, 250.0))
    assert swinging.any() and not swinging.all()
    # periodic: one period later the schedule is the same
    later = [sm.gait_plan(p, sm.SrbdGait(period=period[i:i + 1], swing=swing[i:i + 1], offset=offset[i:i + 1],
                                         fz_stance=250.0, fz_swing=2.0), cmd[i:i + 1], x[i:i + 1],
                          tick + int(period[i]), ref_pose[i:i + 1], foot_now[i:i + 1], N)[0].fz_max[0]
             for i in range(B)]
    assert np.array_equal(np.stack(later), plan.fz_max)


# ---- 5. successive windows agree while the robot moves along the reference ----
@pytest.mark.parametrize("anchor", [0, 1])
def test_successive_windows_are_consistent(pkg, anchor):
    sm = pkg.srbd_model
    B, N, tick0 = 10, 12, 1000
    p = sm.SrbdParams()
    period, swing, offset = GH.special_gaits(B, N, tick0, 60)
    gait = sm.SrbdGait(period=period, swing=swing, offset=offset, k_raibert=0.05, fz_stance=250.0, anchor=anchor)
    cmd, x, ref_pose, foot_now = GH.random_inputs(sm, p, B, 61)
    v = cmd[:, 0:2]

    def on_reference(pose):  # c = p_0, vm = Rz(yaw_0)(vx, vy)
        xa = x.copy()
        xa[:, 6:8], xa[:, 9:11] = pose[:, 0:2], rot(pose[:, 2], v)
        return xa

    ticks = int(period.max()) + 2  # a whole stance of every foot
    prev = None
    for t in range(ticks):
        tick = tick0 + t
        plan, pose1, feet1 = sm.gait_plan(p, gait, cmd, on_reference(ref_pose), tick, ref_pose, foot_now, N)
        swinging, j, down = GH.schedule(period, swing, offset, tick, N)
        # a foot in stance at stage 0 keeps foot_now, bit for bit
        stance0 = ~swinging[:, 0]
        assert np.array_equal(feet1[stance0], foot_now[stance0])
        if prev is not None:
            old, j_old, down_old = prev
            np.testing.assert_allclose(plan.x_ref[:, :N], old.x_ref[:, 1:], rtol=1e-12, atol=1e-15)
            assert np.array_equal(plan.fz_max[:, :N - 1], old.fz_max[:, 1:])
            ok = down_old[:, 1:] | (j_old[:, 1:] < N)  # the touchdown is inside both windows
            assert ok.sum() > ok.size // 2
            a, b = feet_of(plan)[:, :N - 1][ok], feet_of(old)[:, 1:][ok]
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-15)
        prev = (plan, j, down)
        ref_pose, foot_now = pose1, feet1


# ---- 6. the feedback ----
def test_feedback_moves_the_footholds_and_nothing_else(pkg):
    sm = pkg.srbd_model
    B, N, tick = 10, 12, 77
    p = sm.SrbdParams()
    period, swing, offset = GH.special_gaits(B, N, tick, 70)
    cmd, x, ref_pose, foot_now = GH.random_inputs(sm, p, B, 71)
    down = GH.schedule(period, swing, offset, tick, N)[2]
    future = ~down[..., None] & np.array([True, True, False])  # the xy of every foothold still to come
    assert future.any() and down.any()
    rng = np.random.default_rng(72)
    e, d = rng.uniform(-0.3, 0.3, size=(B, 2)), rng.uniform(-0.2, 0.2, size=(B, 2))
    k_r = 0.04
    for anchor in (0, 1):
        gait = sm.SrbdGait(period=period, swing=swing, offset=offset, k_raibert=k_r, fz_stance=250.0, anchor=anchor)
        base = sm.gait_plan(p, gait, cmd, x, tick, ref_pose, foot_now, N)[0]
        # the measured velocity: every future foothold moves by k_raibert e
        xv = x.copy()
        xv[:, 9:11] += e
        got = sm.gait_plan(p, gait, cmd, xv, tick, ref_pose, foot_now, N)[0]
        assert np.array_equal(got.x_ref, base.x_ref) and np.array_equal(got.fz_max, base.fz_max)
        want = feet_of(base) + np.where(future, np.concatenate([k_r * e, np.zeros((B, 1))], 1)[:, None, None, :], 0.0)
        np.testing.assert_allclose(feet_of(got)[future], want[future], rtol=1e-12)
        assert np.array_equal(feet_of(got)[~future], feet_of(base)[~future])
        # the measured position: the footholds move by d; the reference only when it is anchored there
        xc = x.copy()
        xc[:, 6:8] += d
        got = sm.gait_plan(p, gait, cmd, xc, tick, ref_pose, foot_now, N)[0]
        want = feet_of(base) + np.where(future, np.concatenate([d, np.zeros((B, 1))], 1)[:, None, None, :], 0.0)
        np.testing.assert_allclose(feet_of(got)[future], want[future], rtol=1e-12)
        assert np.array_equal(feet_of(got)[~future], feet_of(base)[~future])
        assert np.array_equal(got.fz_max, base.fz_max)
        if anchor:
            moved = base.x_ref.copy()
            moved[:, :, 6:8] += d[:, None]
            np.testing.assert_allclose(got.x_ref, moved, rtol=1e-12)
            assert not np.array_equal(got.x_ref, base.x_ref)
        else:
            assert np.array_equal(got.x_ref, base.x_ref)


# ---- 7. one tick of the host gait loop ----
@pytest.mark.parametrize("alpha_reset", [0.0, 1.0])
def test_one_tick_of_the_host_gait_loop_is_gait_plan_then_the_host_sqp_loop(pkg, oracle, alpha_reset):
    sm = pkg.srbd_model
    B, N, T = 2, 6, 1
    p = sm.SrbdParams()
    xs, us, x, alpha, gait, cmd, ref_pose, foot_now = GH.walking_case(sm, p, B, N, T, 5)
    out = RH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, 15, "none", p=p, gait=gait, cmd=cmd,
                         ref_pose=ref_pose, foot_now=foot_now, tick0=4, alpha_reset=alpha_reset)
    w, pose, feet = sm.gait_plan(p, gait, cmd[:, 0], x, 4, ref_pose, foot_now, N)
    for k in FIELDS:
        assert np.array_equal(getattr(out["windows"][0], k), getattr(w, k)), k
    assert np.array_equal(out["ref_pose"], pose) and np.array_equal(out["foot_now"], feet)
    assert np.array_equal(out["foot_log"][:, 0], feet) and np.array_equal(out["fz_log"][:, 0], w.fz_max[:, 0])
    for i in range(B):
        a0 = alpha_reset if alpha_reset > 0.0 else float(alpha[i])
        hx, hu, ha, hit, hcv, hm = PH.sqp_loop(sm, oracle, p, w.robot(i), xs[i], us[i], x[i], a0, NMPC, 15, "none")
        sx, su, sa, sit, scv, smg = out["steps"][0][i]
        assert np.array_equal(sx, hx) and np.array_equal(su, hu)
        assert (sa, sit, scv, smg) == (ha, hit, hcv, hm)
        assert out["sqp_iter"][i, 0] == hit and bool(out["converged"][i, 0]) == hcv
        assert out["alpha"][i] == ha
        assert np.array_equal(out["u_log"][i, 0], hu[0])
    hxs = np.stack([r[0] for r in out["steps"][0]])
    hus = np.stack([r[1] for r in out["steps"][0]])
    assert np.array_equal(out["x_log"][:, 1], sm.plant_step(x, hus[:, 0], p, w.foot_r[:, 0], w.foot_l[:, 0]))
    sx, su = sm.shift_guess(hxs, hus, p, w)
    assert np.array_equal(out["xs"], sx) and np.array_equal(out["us"], su)
