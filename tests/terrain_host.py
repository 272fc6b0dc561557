"""TEST INFRASTRUCTURE ONLY -- the terrains of the terrain tests, generated from seeds, what the
planner selected on them restated from the planner without terrain, and the stairs the
closed-loop tests walk up.  The host closed loop with the terrain under the planner is
tests/rollout_host.py's closed_loop(gait=..., terrain=...)."""
from __future__ import annotations

import numpy as np

import gait_host as GH

__all__ = ["flat0", "plane", "stairs", "rough", "lipschitz", "nominal", "selection", "stairs_terrain",
           "stairs_level", "stairs_case", "STAIRS"]


# ---- the terrains: height arrays [ny][nx]; sample (j, i) lies at (x0 + i cell, y0 + j cell) ----
def flat0(ny, nx):
    return np.zeros((ny, nx))


def plane(ny, nx, x0, y0, cell, alpha, beta, gamma):
    """H[j][i] = alpha x_i + beta y_j + gamma: the bilinear is exact on it."""
    xs, ys = x0 + cell * np.arange(nx), y0 + cell * np.arange(ny)
    return alpha * xs[None, :] + beta * ys[:, None] + gamma


def stairs(ny, nx, run, rise, first=0):
    """Treads of `run` samples along x, each `rise` above the one before; the riser is the cell
    between the last sample of a tread and the first of the next.  Tread 0 ends at sample `first`."""
    level = np.maximum(0, (np.arange(nx) - first - 1 + run) // run)
    return np.tile(rise * level.astype(np.float64), (ny, 1))


def rough(ny, nx, seed, amplitude=0.03):
    """Uniform random heights in [0, amplitude)."""
    return np.random.default_rng(seed).uniform(0.0, amplitude, size=(ny, nx))


def lipschitz(height, cell):
    """G: the largest difference between adjacent samples over cell.  The bilinear changes by at
    most G (|dx| + |dy|) between two points."""
    H = np.asarray(height, dtype=np.float64)
    H = H[None] if H.ndim == 2 else H
    return max(np.abs(np.diff(H, axis=1)).max(), np.abs(np.diff(H, axis=2)).max()) / cell


# ---- what the planner selected, restated from the planner without terrain ----
def nominal(sm, p, gait, cmd, x, tick, ref_pose, foot_now, N):
    """(n [B][N][2][2], down [B][N][2]): the nominal footholds, which are the feet's xy of the
    planner without terrain, and the rows that hold foot_now instead of a touchdown."""
    B = np.asarray(cmd).shape[0]
    w = sm.gait_plan(p, gait, cmd, x, tick, ref_pose, foot_now, N)[0]
    period, swing, offset = (np.broadcast_to(np.asarray(v, dtype=np.int64), s) for v, s in
                             zip((gait.period, gait.swing, gait.offset), ((B,), (B, 2), (B, 2))))
    down = GH.schedule(period, swing, offset, tick, N)[2]
    return np.stack([w.foot_r[:, :, 0:2], w.foot_l[:, :, 0:2]], axis=2), down


def selection(sm, p, gait, terrain, cmd, x, tick, ref_pose, foot_now, N, map_r=None):
    """(q [B][N][2] the chosen candidate of every row's touchdown, -1 where the row holds
    foot_now; margin: the smallest gap between the best and the second-best cost over all
    touchdowns, inf where nothing is selected; n, down of nominal())."""
    n, down = nominal(sm, p, gait, cmd, x, tick, ref_pose, foot_now, N)
    maps = terrain.map_r if map_r is None else map_r
    maps = np.zeros(n.shape[0], dtype=np.int64) if maps is None else np.asarray(maps, dtype=np.int64)
    _, _, q, margin = sm.foothold_select(terrain, n, maps[:n.shape[0], None, None])
    return np.where(down, -1, q), np.where(down, np.inf, margin).min(initial=np.inf), n, down


# the stairs the closed-loop tests walk up: 2 cm cells, treads of three samples (6 cm), 3 cm risers
STAIRS = dict(ny=9, nx=40, x0=0.2, y0=-0.4, cell=0.02, run=3, rise=0.03, first=14)


def stairs_terrain(sm, search=1, w_rough=10.0, map_r=None):
    s = STAIRS
    return sm.SrbdTerrain(height=stairs(s["ny"], s["nx"], s["run"], s["rise"], s["first"]), x0=s["x0"], y0=s["y0"],
                          cell=s["cell"], map_r=map_r, search=search, w_rough=w_rough)


def stairs_level(x):
    """The tread under x (its index; -1 on a riser), from STAIRS' definition and not the sampler."""
    s = STAIRS
    u = (np.asarray(x, dtype=np.float64) - s["x0"]) / s["cell"]  # in samples
    i = np.floor(u).astype(np.int64)
    lo = np.maximum(0, (i - s["first"] - 1 + s["run"]) // s["run"])
    hi = np.maximum(0, (i + 1 - s["first"] - 1 + s["run"]) // s["run"])
    return np.where((lo == hi) | (u == i), lo, -1)


def stairs_case(sm, p, B, N, T, seed, vx=1.0):
    """gait_host.walking_case's robots and gait, commanded straight up the stairs: vx for every
    robot, no lateral velocity and no yaw rate.  Returns walking_case's tuple."""
    xs, us, x, alpha, gait, cmd, ref_pose, foot_now = GH.walking_case(sm, p, B, N, T, seed)
    cmd[:, :, 0], cmd[:, :, 1], cmd[:, :, 2] = vx, 0.0, 0.0
    return xs, us, x, alpha, gait, cmd, ref_pose, foot_now
