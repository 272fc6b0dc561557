"""TEST INFRASTRUCTURE ONLY -- the host side of the gait planner (srbd_qp_srbd_gait_plan_f64,
srbd_qp_srbd_rollout_gait_f64): the gaits and inputs of the gait tests and the contact
schedule's integers restated.  The host closed loop that replans every tick is
tests/rollout_host.py's closed_loop(gait=...)."""
from __future__ import annotations

import numpy as np

__all__ = ["rot", "walking_gait", "walking_case", "special_gaits", "schedule", "random_inputs"]


def rot(yaw, v):
    """Rz(yaw) v for v [...][2]."""
    c, s = np.cos(yaw), np.sin(yaw)
    return np.stack([c * v[..., 0] - s * v[..., 1], s * v[..., 0] + c * v[..., 1]], axis=-1)


def walking_gait(sm, p, B, k_raibert=0.03, anchor=0):
    """Period 6, swing 3, the feet half a period apart, robot i shifted by i stages: within four
    ticks every robot has a liftoff and a touchdown.  fz_stance is inside the input box."""
    shift = np.arange(B) % 3
    offset = np.stack([shift, shift + 3], axis=1)
    return sm.SrbdGait(period=6, swing=(3, 3), offset=offset, hip=((0.0, -0.1), (0.0, 0.1)), ground_z=0.0,
                       k_raibert=k_raibert, fz_stance=250.0, fz_swing=1.0, anchor=anchor)


def walking_case(sm, p, B, N, T, seed):
    """B robots from perturbed starts, each with its own velocity command (constant over the T
    ticks, with a yaw rate), walking_gait's gait, the reference pose at the default reference
    and the feet under the hips.  Returns (xs, us, x, alpha, gait, cmd, ref_pose, foot_now)."""
    rng = np.random.default_rng(seed)
    xs, us, dx0 = sm.sample_trajectories(B, N, seed, p)
    x = xs[:, 0] + dx0
    xr = np.array(p.x_ref, dtype=np.float64)
    cmd = np.empty((B, T, 4))
    cmd[:, :, 0:2] = rng.uniform(-0.3, 0.3, size=(B, 1, 2))
    cmd[:, :, 2] = rng.uniform(-0.2, 0.2, size=(B, 1))
    cmd[:, :, 3] = xr[8]
    ref_pose = np.tile(np.array([xr[6], xr[7], xr[2]]), (B, 1)) + rng.uniform(-0.01, 0.01, size=(B, 3))
    foot_now = np.empty((B, 2, 3))
    foot_now[:, 0] = xr[6:9] * np.array([1.0, 1.0, 0.0]) + np.array(p.foot_r)
    foot_now[:, 1] = xr[6:9] * np.array([1.0, 1.0, 0.0]) + np.array(p.foot_l)
    foot_now += rng.uniform(-0.005, 0.005, size=(B, 2, 3))
    alpha = np.where(np.arange(B) % 4 == 1, 0.5, 1.0)
    return xs, us, x, alpha, walking_gait(sm, p, B), cmd, ref_pose, foot_now


def special_gaits(B, N, tick, seed):
    """Per-robot (period [B], swing [B][2], offset [B][2]) int64 arrays for a window planned at
    `tick`.  Robots 0..4 (B >= 5) are, for the right foot: a standing robot (swing 0); a foot
    in swing at stage 0; a touchdown exactly at stage 0 (phi = swing there, s = 0); a period
    below N (from N = 6 on) with several touchdowns in the window; a period above N.  The left
    foot of each is half a period apart; the other robots are random."""
    rng = np.random.default_rng(seed)
    period = rng.integers(1, 2 * N + 4, size=B)
    swing = np.stack([rng.integers(0, period), rng.integers(0, period)], axis=1)
    phi0 = np.stack([rng.integers(0, period), rng.integers(0, period)], axis=1)  # wanted at stage 0
    short = max(2, N // 3)
    special = [(4, 0, 0), (6, 3, 1), (6, 3, 3), (short, short // 2, 0), (2 * N + 5, N + 2, 0)]
    for i, (per, sw, ph) in enumerate(special[:B]):
        period[i], swing[i], phi0[i] = per, (sw, sw), (ph, (ph + per // 2) % per)
    offset = (phi0 - tick) % period[:, None] + period[:, None] * rng.integers(0, 3, size=(B, 2))
    return period.astype(np.int64), swing.astype(np.int64), offset.astype(np.int64)


def schedule(period, swing, offset, tick, N):
    """The contact schedule's integers, restated with Python ints: (swinging [B][N][2] bool,
    j [B][N][2] the touchdown stage of a swing stage or the first stage s of a stance stage,
    down [B][N][2] bool: the stage holds foot_now)."""
    B = len(period)
    swinging = np.zeros((B, N, 2), dtype=bool)
    down = np.zeros((B, N, 2), dtype=bool)
    j = np.zeros((B, N, 2), dtype=np.int64)
    for i in range(B):
        for f in range(2):
            per, sw, off = int(period[i]), int(swing[i, f]), int(offset[i, f])
            for k in range(N):
                phi = (int(tick) + k + off) % per
                if phi < sw:
                    swinging[i, k, f], j[i, k, f] = True, k + sw - phi
                else:
                    s = k - (phi - sw)
                    j[i, k, f] = s
                    down[i, k, f] = sw == 0 or s <= 0
    return swinging, j, down


def random_inputs(sm, p, B, seed):
    """(cmd [B][4], x [B][12], ref_pose [B][3], foot_now [B][2][3]) around the default reference."""
    rng = np.random.default_rng(seed)
    xr = np.array(p.x_ref, dtype=np.float64)
    cmd = np.stack([rng.uniform(-0.5, 0.5, B), rng.uniform(-0.3, 0.3, B), rng.uniform(-1.0, 1.0, B),
                    xr[8] + rng.uniform(-0.1, 0.1, B)], axis=1)
    x = xr + rng.normal(size=(B, 12)) * sm.SIGMA_X
    ref_pose = np.stack([xr[6] + rng.uniform(-0.2, 0.2, B), xr[7] + rng.uniform(-0.2, 0.2, B),
                         xr[2] + rng.uniform(-0.5, 0.5, B)], axis=1)
    foot_now = np.stack([xr[6:9] * [1, 1, 0] + np.array(p.foot_r), xr[6:9] * [1, 1, 0] + np.array(p.foot_l)])
    foot_now = foot_now + rng.uniform(-0.05, 0.05, size=(B, 2, 3))
    return cmd, x, ref_pose, foot_now
