"""Batched SRBD QP-data generator (numpy): the producer of the hot path's inputs.

Restates, vectorised over (batch, stage), how the reference builds the QP the
solver receives:

* dynamics ``SRBDModel::GetContinuousDynamic`` / ``GetShootingDynamic``
  (dynamics/SRBD_model.cpp:75-235): RK4 defect with *Euler* Jacobians
  (:179-181), A = j_x, B = j_u, b = -f;
* SO(3) helpers expm / jl / jlt / djl / djlt (dynamics/orientation_tool.h:76-227);
* friction cone ``GetConstrain`` (SRBD_model.cpp:237-260) and the relaxed
  log-barrier ``Barrier`` (:262-295);
* QP assembly ``NMPCSolver::prepareQpStructures`` (NMPC_solver.cpp:276-314):
  Q, q = Q (x - x_ref), S = 0, R = R_ + Ac' diag(ddb) Ac, r = R_ u + Ac' db,
  terminal Qf, qf;
* parameters: config/mpc_option.yaml:2-18, setupDynamics (NMPC_solver.cpp:332-339),
  setupReference (:341-351), SRBDModel() defaults (SRBD_model.cpp:5-24).

Inputs are drawn per QP from a counter-based seed (``seed + qp_index``), as
SURVEY.md section 8(d) prescribes, so any shard of a batch can be generated
independently.  The generator is the workload, not the product path.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from .qp import OcpQpBatch

__all__ = ["SrbdParams", "SrbdPlan", "generate_batch", "build_qp", "sample_trajectories", "shooting_dynamics", "friction_cone", "barrier",
           "plant_step", "shift_guess", "SrbdGait", "gait_plan", "SrbdTerrain",
           "terrain_height", "foothold_select", "SrbdContact", "contact_flags", "contact_project", "fall_values"]


@dataclass(frozen=True)
class SrbdParams:
    # config/mpc_option.yaml:2-18
    Q: Tuple[float, ...] = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 10)
    Qf: Tuple[float, ...] = (0.5, 0.5, 0.5, 0.01, 0.01, 0.01, 100, 100, 100, 0.0, 0.0, 100.0)
    R: float = 0.0001
    dt: float = 0.015
    N: int = 20
    Lbody: Tuple[float, float, float] = (0.541667, 0.516667, 1.0416667)
    mu_b: float = 0.1
    theta_b: float = 5.0
    # NMPC_solver.cpp:332-339 / SRBD_model.cpp:5-24
    mass: float = 15.0
    foot_r: Tuple[float, float, float] = (0.0, -0.1, 0.0)
    foot_l: Tuple[float, float, float] = (0.0, 0.1, 0.0)
    mu: float = 0.5
    Lfx: float = 0.05
    Lfz: float = 0.05
    fmax: float = 1000.0
    fmin: float = 0.0
    # NMPC_solver.cpp:344-345
    x_ref: Tuple[float, ...] = (0, 0, 0.2, 0, 0, 0, 0.5, 0, 1.0, 0, 0, 0)


@dataclass(frozen=True)
class SrbdPlan:
    """Per-robot, per-stage overrides of SrbdParams (the C-ABI's srbd_plan_f64): numpy
    arrays, each optional (None: SrbdParams' value on every stage).

    x_ref  [B][N+1][12]  reference state per stage (NMPCSolver::x_ref_, 12 x (N+1))
    foot_r [B][N][3]     right-foot position at stage k
    foot_l [B][N][3]     left-foot position
    fz_max [B][N][2]     normal-force limit (right, left): the contact schedule"""
    x_ref: Optional[np.ndarray] = None
    foot_r: Optional[np.ndarray] = None
    foot_l: Optional[np.ndarray] = None
    fz_max: Optional[np.ndarray] = None

    def robot(self, i: int) -> "SrbdPlan":
        """Robot i's rows (the arrays without the batch dimension)."""
        return SrbdPlan(*[None if a is None else a[i]
                          for a in (self.x_ref, self.foot_r, self.foot_l, self.fz_max)])


def plan_feet(p: "SrbdParams", plan: Optional[SrbdPlan]):
    """(foot_r, foot_l) per stage, or SrbdParams' constants."""
    pf0 = np.array(p.foot_r) if plan is None or plan.foot_r is None else np.asarray(plan.foot_r)
    pf1 = np.array(p.foot_l) if plan is None or plan.foot_l is None else np.asarray(plan.foot_l)
    return pf0, pf1


def plan_cone_offsets(bc, plan: Optional[SrbdPlan]):
    """The cone rows' constant term with the plan's force limits: row 4 of each foot
    (fz <= fmax) takes fz_max of that foot and stage.  [..., 24] with a plan, bc without."""
    if plan is None or plan.fz_max is None:
        return bc
    fz = np.asarray(plan.fz_max)
    out = np.broadcast_to(bc, fz.shape[:-1] + (24,)).copy()
    out[..., 4] = fz[..., 0]
    out[..., 16] = fz[..., 1]
    return out


def load_mpc_option(source) -> Tuple["SrbdParams", Dict]:
    """The reference's config file (config/mpc_option.yaml), read with the keys of
    NMPCSolver::readYaml (NMPC_solver.cpp:22-46): MPC.{Q, Qf, R, dt_MPC, horizon_MPC,
    sqp_max_loop}, Physical.Lbody, mu_b, theta_b, N_rep.  `source` is a path or the
    YAML text.  Returns (SrbdParams, {"sqp_max_loop", "N_rep"}); a missing key raises
    KeyError like yaml-cpp's as<>() on an absent node throws."""
    import os
    import yaml
    text = source
    if isinstance(source, (str, os.PathLike)) and os.path.exists(source):
        with open(source) as f:
            text = f.read()
    cfg = yaml.safe_load(text)
    mpc, phys = cfg["MPC"], cfg["Physical"]
    def vec(v, n, name):
        if len(v) != n:
            raise ValueError(f"{name} needs {n} values, got {len(v)}")
        return tuple(float(x) for x in v)

    p = SrbdParams(Q=vec(mpc["Q"], 12, "MPC.Q"), Qf=vec(mpc["Qf"], 12, "MPC.Qf"), R=float(mpc["R"]),
                   dt=float(mpc["dt_MPC"]), N=int(mpc["horizon_MPC"]),
                   Lbody=vec(phys["Lbody"], 3, "Physical.Lbody"), mu_b=float(cfg["mu_b"]),
                   theta_b=float(cfg["theta_b"]))
    return p, {"sqp_max_loop": int(mpc["sqp_max_loop"]), "N_rep": int(cfg["N_rep"])}


# ---------------------------------------------------------------------------
# SO(3) helpers, orientation_tool.h (batched over leading dims)
# ---------------------------------------------------------------------------
def skew(v):
    z = np.zeros(v.shape[:-1])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1),
                     np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def _theta(v):
    th = np.sqrt(np.sum(v * v, axis=-1))
    return np.maximum(th, 1e-10)  # h = 1e-10 clamp (orientation_tool.h:82-86)


def expm(v):
    th = _theta(v)[..., None, None]
    V = skew(v)
    I = np.eye(3)
    return I + (np.sin(th) / th) * V + ((1.0 - np.cos(th)) / (th * th)) * (V @ V)


def jl(v):
    th = _theta(v)[..., None, None]
    V = skew(v) / th
    I = np.eye(3)
    return (np.sin(th) / th) * I + (1.0 - np.sin(th) / th) * (V @ V + I) + ((1.0 - np.cos(th)) / th) * V


def jlt(v):
    th = _theta(v)[..., None, None]
    V = skew(v) / th
    I = np.eye(3)
    cot = 1.0 / np.tan(0.5 * th)
    return (0.5 * cot * th) * I + (1.0 - 0.5 * cot * th) * (V @ V + I) - (0.5 * th) * V


def djl(v):
    th = _theta(v)[..., None, None]
    V = skew(v) / th
    s, c = np.sin(th), np.cos(th)
    th2, th3 = th * th, th * th * th
    base = ((th * s + 2.0 * (c - 1.0)) / th3) * V + (-(2.0 * th - 3.0 * s + th * c) / th3) * (V @ V)
    sv = skew(v)
    out = []
    for a in range(3):
        e = np.zeros(3)
        e[a] = 1.0
        se = skew(e)
        d = ((th - s) / th3) * (se @ sv + sv @ se) + ((1.0 - c) / th2) * se
        out.append(d + base * v[..., a][..., None, None])
    return out


def djlt(v):
    J = jlt(v)
    return [-(J @ d @ J) for d in djl(v)]


# ---------------------------------------------------------------------------
# dynamics, SRBD_model.cpp:75-235
# ---------------------------------------------------------------------------
def _consts(p: SrbdParams):
    Lb = np.diag(1.0 / np.array(p.Lbody))  # SetInertia(L) stores L^-1 (SRBD_model.cpp:46-49)
    pf0 = np.array(p.foot_r)
    pf1 = np.array(p.foot_l)
    return Lb, pf0, pf1


def continuous(x, u, p: SrbdParams, jac: bool, plan: Optional[SrbdPlan] = None):
    Lb, _, _ = _consts(p)
    pf0, pf1 = plan_feet(p, plan)
    r, l, pos, v = x[..., 0:3], x[..., 3:6], x[..., 6:9], x[..., 9:12]
    R = expm(r)
    Jlt = jlt(r)
    RLR = R @ Lb @ np.swapaxes(R, -1, -2)
    w = np.einsum("...ij,...j->...i", RLR, l)
    dx = np.empty(x.shape)
    dx[..., 0:3] = np.einsum("...ij,...j->...i", Jlt, w)
    dx[..., 3:6] = (u[..., 3:6] + u[..., 9:12]
                    + np.einsum("...ij,...j->...i", skew(pf0 - pos), u[..., 0:3])
                    + np.einsum("...ij,...j->...i", skew(pf1 - pos), u[..., 6:9]))
    dx[..., 6:9] = v
    dx[..., 9:12] = (u[..., 0:3] + u[..., 6:9]) / p.mass + np.array([0.0, 0.0, -9.8])
    if not jac:
        return dx, None, None
    dJ = djlt(r)
    djw = np.stack([np.einsum("...ij,...j->...i", dJ[a], w) for a in range(3)], -1)
    Jl = jl(r)
    jfx = np.zeros(x.shape[:-1] + (12, 12))
    jfx[..., 0:3, 0:3] = djw + Jlt @ (RLR @ skew(l) - skew(w)) @ Jl
    jfx[..., 0:3, 3:6] = Jlt @ RLR
    jfx[..., 3:6, 6:9] = skew(u[..., 0:3] + u[..., 6:9])
    jfx[..., 6:9, 9:12] = np.eye(3)
    jfu = np.zeros(x.shape[:-1] + (12, 12))
    jfu[..., 3:6, 0:3] = skew(pf0 - pos)
    jfu[..., 3:6, 3:6] = np.eye(3)
    jfu[..., 3:6, 6:9] = skew(pf1 - pos)
    jfu[..., 3:6, 9:12] = np.eye(3)
    jfu[..., 9:12, 0:3] = np.eye(3) / p.mass
    jfu[..., 9:12, 6:9] = np.eye(3) / p.mass
    return dx, jfx, jfu


def shooting_dynamics(x, x_next, u, p: SrbdParams, plan: Optional[SrbdPlan] = None):
    """A = I + dt jfx, B = dt jfu (Euler Jacobians, :179-181), b = RK4(x,u) - x_next.
    plan: its feet (one row per stage of x) replace SrbdParams'."""
    dt = p.dt
    k1, jfx, jfu = continuous(x, u, p, True, plan)
    k2, _, _ = continuous(x + 0.5 * dt * k1, u, p, False, plan)
    k3, _, _ = continuous(x + 0.5 * dt * k2, u, p, False, plan)
    k4, _, _ = continuous(x + dt * k3, u, p, False, plan)
    x_get = x + (dt / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    A = np.eye(12) + dt * jfx
    B = dt * jfu
    b = x_get - x_next  # b = -f, f = x_next - x_get (:194-197, :225-229)
    return A, B, b


# ---------------------------------------------------------------------------
# the closed loop between two NMPC steps (the C-ABI's srbd_qp_srbd_advance_f64)
# ---------------------------------------------------------------------------
def _rk4_step(x, u, p: SrbdParams, h: float, plan: Optional[SrbdPlan], wrench=None):
    """One classical RK4 step of length h of xdot = f(x, u) + w: the operations of
    shooting_dynamics' x_get, in its order.  wrench [..., 6] (torque, force; world frame) adds
    wrench[0:3] to rows 3..5 and wrench[3:6] / mass to rows 9..11 of every slope."""
    def slope(xa):
        dx = continuous(xa, u, p, False, plan)[0]
        if wrench is not None:
            dx[..., 3:6] += wrench[..., 0:3]
            dx[..., 9:12] += wrench[..., 3:6] / p.mass
        return dx

    k1 = slope(x)
    k2 = slope(x + 0.5 * h * k1)
    k3 = slope(x + 0.5 * h * k2)
    k4 = slope(x + h * k3)
    return x + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)


def contact_flags(contact: "SrbdContact", fz_max0, B: int):
    """The contact flags [B][2] of one tick: foot f is in contact iff the plan's fz_max[:, 0, f]
    (fz_max0 [B][2]) exceeds contact.fz_contact; without it (None) both feet are."""
    if fz_max0 is None:
        return np.ones((B, 2), dtype=bool)
    return np.asarray(fz_max0, dtype=np.float64) > contact.fz_contact


def contact_project(u, contact: "SrbdContact", in_contact, mu):
    """The projection of include/srbd_qp.h's contact model, operation for operation: the
    commanded input u [B][12] onto what the feet can transmit, with the contact flags in_contact
    [B][2] and the plant's friction coefficient mu (a float or [B]).  Per foot f (o = 6 f):
    fz' = c_f ? clamp(fz, 0, fz_hi) : 0;  fx', fy' clamped to +-(mu fz');  tau_a' to +-(Lt_a fz');
    clamp(v, lo, hi) = fmin(fmax(v, lo), hi), each bound one multiplication.  Returns (u' [B][12],
    sat [B] uint32): bit 4 f + kind is set iff that group's projected values differ from the
    commanded ones -- kind 0: fz raised to 0 or zeroed by swing, 1: fz lowered to fz_hi, 2: fx or
    fy, 3: a torque."""
    u = np.asarray(u, dtype=np.float64)
    B = u.shape[0]
    on = np.broadcast_to(np.asarray(in_contact, dtype=bool), (B, 2))
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), (B,))
    clamp = lambda v, lo, hi: np.fmin(np.fmax(v, lo), hi)
    out = np.empty_like(u)
    sat = np.zeros(B, dtype=np.uint32)
    for f in range(2):
        o = 6 * f
        fz = u[:, o + 2]
        fzp = np.where(on[:, f], clamp(fz, 0.0, contact.fz_hi), 0.0)
        b = mu * fzp
        out[:, o] = clamp(u[:, o], -b, b)
        out[:, o + 1] = clamp(u[:, o + 1], -b, b)
        out[:, o + 2] = fzp
        for a in range(3):
            bt = contact.Lt[a] * fzp
            out[:, o + 3 + a] = clamp(u[:, o + 3 + a], -bt, bt)
        differs = out[:, o:o + 6] != u[:, o:o + 6]
        kinds = (differs[:, 2] & (~on[:, f] | (fzp > fz)), on[:, f] & (fzp < fz),
                 differs[:, 0] | differs[:, 1], differs[:, 3:6].any(axis=1))
        for kind, hit in enumerate(kinds):
            sat |= np.where(hit, np.uint32(1 << (4 * f + kind)), np.uint32(0))
    return out, sat


def fall_values(x, contact: "SrbdContact", map_r=None):
    """What the fall test of the contact model compares, for the states x [B][12] on the true
    ground's maps map_r ([B]; None: contact.ground.map_r, then map 0): (x[8] - (ground_z +
    h_true(x[6], x[7])), expm(x[0:3])[2][2]), h_true = 0 without a true ground.  A robot falls
    where the first is below contact.z_min or the second below contact.cos_tilt_min."""
    x = np.asarray(x, dtype=np.float64)
    hg = 0.0
    if contact.ground is not None:
        m = contact.ground.map_r if map_r is None else map_r
        hg = terrain_height(contact.ground, x[:, 6:8], None if m is None else np.asarray(m)[:x.shape[0]])
    return x[:, 8] - (contact.ground_z + hg), expm(x[:, 0:3])[:, 2, 2]


def plant_step(x, u, p: SrbdParams, foot_r=None, foot_l=None, wrench=None, substeps: int = 1,
               contact: Optional["SrbdContact"] = None, in_contact=None, state=None):
    """The plant over one control tick: x [B][12] after `substeps` RK4 steps of dt / substeps of
    xdot = f(x, u) + w with the input u [B][12] held (applied as it is: nothing is clamped).
    foot_r / foot_l [B][3]: the feet during the tick (None: SrbdParams'); wrench [B][6]: an
    external torque and force on the body, world frame, held over the tick (None: none).

    contact (a SrbdContact): the plant step of include/srbd_qp.h's contact model, with the
    contact flags in_contact [B][2] (None: both feet; contact_flags makes them from the plan) and
    state = {"fallen": [B] int, "alive": [B] int, "sat": [B] uint32}, each optional (None: {}).
    Returns (x', u', state'): u' the applied input, state' new arrays; the inputs are left alone.
    A robot already fallen, or whose u is not finite, keeps x and applies zeros; the others apply
    contact_project(u), stand their feet in contact on the true ground, integrate, and are
    tested for a fall (only with "fallen" in the state)."""
    if substeps < 1:
        raise ValueError("substeps must be at least 1")
    h = p.dt / substeps
    if contact is None:
        feet = None if foot_r is None and foot_l is None else SrbdPlan(foot_r=foot_r, foot_l=foot_l)
        for _ in range(substeps):
            x = _rk4_step(x, u, p, h, feet, wrench)
        return x
    x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
    B = x.shape[0]
    state = {k: np.array(v) for k, v in (state or {}).items() if v is not None}
    if "alive" in state and "fallen" not in state:
        raise ValueError("alive needs fallen")
    on = np.ones((B, 2), dtype=bool) if in_contact is None else np.broadcast_to(np.asarray(in_contact, dtype=bool), (B, 2))
    mu = np.broadcast_to(np.asarray(contact.mu if contact.mu_r is None else np.asarray(contact.mu_r)[:B],
                                    dtype=np.float64), (B,))
    frozen = state["fallen"] != 0 if "fallen" in state else np.zeros(B, dtype=bool)
    bad = ~frozen & ~np.isfinite(u).all(axis=1)
    if "fallen" in state:
        state["fallen"][bad] = 1
    go = ~frozen & ~bad
    x_new, u_app = x.copy(), np.zeros_like(u)
    if not go.any():
        return x_new, u_app, state
    up, bits = contact_project(u[go], contact, on[go], mu[go])
    u_app[go] = up
    if "sat" in state:
        state["sat"][go] |= bits.astype(state["sat"].dtype)
    n = int(go.sum())
    fr = np.tile(np.array(p.foot_r, dtype=np.float64), (n, 1)) if foot_r is None else np.array(foot_r, dtype=np.float64)[go]
    fl = np.tile(np.array(p.foot_l, dtype=np.float64), (n, 1)) if foot_l is None else np.array(foot_l, dtype=np.float64)[go]
    maps = None
    if contact.ground is not None:
        g = contact.ground
        maps = np.zeros(B, dtype=np.int64) if g.map_r is None else np.asarray(g.map_r, dtype=np.int64)[:B]
        for f, ft in enumerate((fr, fl)):
            z = contact.ground_z + terrain_height(g, ft[:, 0:2], maps[go])
            ft[:, 2] = np.where(on[go][:, f], z, ft[:, 2])
    feet = SrbdPlan(foot_r=fr, foot_l=fl)
    xg = x[go]
    w = None if wrench is None else np.asarray(wrench, dtype=np.float64)[go]
    with np.errstate(all="ignore"):
        for _ in range(substeps):
            xg = _rk4_step(xg, up, p, h, feet, w)
        if "fallen" in state:
            finite = np.isfinite(xg).all(axis=1)
            xg[~finite] = x[go][~finite]
            above, r33 = fall_values(xg, contact, None if maps is None else maps[go])
            fell = ~finite | (above < contact.z_min) | (r33 < contact.cos_tilt_min)
            idx = np.nonzero(go)[0]
            state["fallen"][idx[fell]] = 1
            if "alive" in state:
                state["alive"][idx[~fell]] += 1
    x_new[go] = xg
    return x_new, u_app, state


def shift_guess(xs, us, p: SrbdParams, plan: Optional[SrbdPlan] = None):
    """The previous solution shifted by one stage, the warm start of the next tick: xs [B][N+1][12],
    us [B][N][12] -> (xs', us') with xs'[k] = xs[k+1] (k < N), us'[k] = us[k+1] (k < N-1),
    us'[N-1] = us[N-1] and xs'[N] one RK4 step of the model over dt from xs[N] with us[N-1] and
    the feet of the plan's stage N-1, so the new last stage has no shooting defect.  xs'[0] is
    the old xs[1], not the plant's state: the step forms x0 - xs[:, 0] itself."""
    N = us.shape[1]
    last = None
    if plan is not None and (plan.foot_r is not None or plan.foot_l is not None):
        last = SrbdPlan(foot_r=None if plan.foot_r is None else np.asarray(plan.foot_r)[:, N - 1],
                        foot_l=None if plan.foot_l is None else np.asarray(plan.foot_l)[:, N - 1])
    xN = _rk4_step(xs[:, N], us[:, N - 1], p, p.dt, last)
    xs_new = np.concatenate([xs[:, 1:], xN[:, None]], axis=1)
    us_new = np.concatenate([us[:, 1:], us[:, N - 1:]], axis=1)
    return xs_new, us_new


# ---------------------------------------------------------------------------
# the gait planner (the C-ABI's srbd_qp_srbd_gait_plan_f64)
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class SrbdGait:
    """The C-ABI's srbd_gait_f64.  period, swing, offset are in stages: an int / a pair
    (right, left) for every robot, or arrays [B] / [B][2] (the struct's _r arrays)."""
    period: object = 1
    swing: object = (0, 0)
    offset: object = (0, 0)
    hip: Tuple[Tuple[float, float], Tuple[float, float]] = ((0.0, -0.1), (0.0, 0.1))
    ground_z: float = 0.0
    k_raibert: float = 0.0
    fz_stance: float = 1000.0
    fz_swing: float = 1.0
    anchor: int = 0


@dataclass(frozen=True)
class SrbdTerrain:
    """The C-ABI's srbd_terrain_f64, as numpy: height [maps][ny][nx] (or [ny][nx] for one map),
    sample (j, i) at (x0 + i cell, y0 + j cell); map_r [B] the robots' maps (None: map 0);
    search in 0..3 and w_rough >= 0 for the foothold selection."""
    height: object
    x0: float
    y0: float
    cell: float
    map_r: object = None
    search: int = 0
    w_rough: float = 0.0


@dataclass(frozen=True)
class SrbdContact:
    """The C-ABI's srbd_contact_f64, as numpy: the plant's contact model and fall thresholds.
    mu: the true friction coefficient of every robot, or mu_r [B]; Lt = (Ltx, Lty, Ltz); ground: a
    SrbdTerrain, the TRUE ground with its own map_r (None: flat at ground_z, the feet keep their
    planned z).  The fallen / alive / sat arrays are plant_step's `state`."""
    mu: float = 0.5
    mu_r: object = None
    Lt: Tuple[float, float, float] = (0.0, 0.05, 0.05)
    fz_hi: float = math.inf
    fz_contact: float = 0.0
    ground_z: float = 0.0
    ground: Optional[SrbdTerrain] = None
    z_min: float = 0.0
    cos_tilt_min: float = 0.0


def terrain_height(terrain: SrbdTerrain, xy, map=None):
    """Height of map `map` (an int array that broadcasts against xy's leading shape; None: map
    0) at the points xy [...][2]: include/srbd_qp.h's clamped bilinear, operation for operation."""
    H = np.asarray(terrain.height, dtype=np.float64)
    H = H[None] if H.ndim == 2 else H
    ny, nx = H.shape[1], H.shape[2]
    xy = np.asarray(xy, dtype=np.float64)
    m = np.zeros(xy.shape[:-1], dtype=np.int64) if map is None else \
        np.broadcast_to(np.asarray(map, dtype=np.int64), xy.shape[:-1])
    s = np.minimum(np.maximum((xy[..., 0] - terrain.x0) / terrain.cell, 0.0), float(nx - 1))
    t = np.minimum(np.maximum((xy[..., 1] - terrain.y0) / terrain.cell, 0.0), float(ny - 1))
    i = np.minimum(np.floor(s).astype(np.int64), nx - 2)
    j = np.minimum(np.floor(t).astype(np.int64), ny - 2)
    a, b = s - i, t - j
    return (1.0 - b) * ((1.0 - a) * H[m, j, i] + a * H[m, j, i + 1]) + \
        b * ((1.0 - a) * H[m, j + 1, i] + a * H[m, j + 1, i + 1])


def foothold_select(terrain: SrbdTerrain, n, map=None):
    """The foothold selection of include/srbd_qp.h's terrain for the nominal footholds n
    [...][2] on map `map`: candidate q = (dj + search)(2 search + 1) + (di + search) lies at
    n + cell (di, dj) and costs J = cell^2 (di^2 + dj^2) + w_rough rho^2, rho the largest height
    difference to the four points one cell away; the smallest J wins, ties go to the smallest q.
    Returns (xy [...][2], z [...] the height there, q [...] the winner, margin [...] the second
    smallest J minus the smallest; inf with search == 0, where nothing is evaluated)."""
    n = np.asarray(n, dtype=np.float64)
    S, cell = int(terrain.search), terrain.cell
    lead = n.shape[:-1]
    if S == 0:
        return n.copy(), terrain_height(terrain, n, map), np.zeros(lead, dtype=np.int64), np.full(lead, np.inf)
    ex, ey = np.array([cell, 0.0]), np.array([0.0, cell])
    best = np.full(lead, np.inf)
    second = np.full(lead, np.inf)
    qbest = np.zeros(lead, dtype=np.int64)
    xy = n.copy()
    q = 0
    for dj in range(-S, S + 1):
        for di in range(-S, S + 1):
            c = n + cell * np.array([float(di), float(dj)])
            h0 = terrain_height(terrain, c, map)
            rho = np.abs(terrain_height(terrain, c + ex, map) - h0)
            rho = np.maximum(rho, np.abs(terrain_height(terrain, c - ex, map) - h0))
            rho = np.maximum(rho, np.abs(terrain_height(terrain, c + ey, map) - h0))
            rho = np.maximum(rho, np.abs(terrain_height(terrain, c - ey, map) - h0))
            J = cell * cell * float(di * di + dj * dj) + terrain.w_rough * (rho * rho)
            win = J < best  # strictly: a tie stays with the smaller q
            second = np.where(win, best, np.minimum(second, J))
            best = np.where(win, J, best)
            qbest = np.where(win, q, qbest)
            xy = np.where(win[..., None], c, xy)
            q += 1
    return xy, terrain_height(terrain, xy, map), qbest, second - best


def gait_plan(p: SrbdParams, gait: SrbdGait, cmd, x, tick: int, ref_pose, foot_now, N: Optional[int] = None,
              Lbody_z=None, terrain: Optional[SrbdTerrain] = None, map_r=None):
    """One tick's plan window, the statement of include/srbd_qp.h's gait planner: cmd [B][4]
    (vx, vy in the heading frame, wz, body height), x [B][12] the measured state, tick >= 0,
    ref_pose [B][3] (px, py, yaw), foot_now [B][2][3].  N: the horizon (None: p.N); Lbody_z [B]:
    the robots' Lbody[2] (None: p.Lbody[2]).  terrain: a SrbdTerrain (None: flat ground at
    gait.ground_z, the planner without terrain); map_r [B]: the robots' maps (None:
    terrain.map_r, then map 0).  Returns (SrbdPlan, new ref_pose, new foot_now); the inputs
    are left alone."""
    cmd, x = np.asarray(cmd, dtype=np.float64), np.asarray(x, dtype=np.float64)
    ref_pose, foot_now = np.asarray(ref_pose, dtype=np.float64), np.asarray(foot_now, dtype=np.float64)
    B = cmd.shape[0]
    N = p.N if N is None else int(N)
    if tick < 0:
        raise ValueError("tick must be non-negative")
    if not gait.fz_swing > 0.0 or not gait.fz_stance > gait.fz_swing:
        raise ValueError("fz_swing must be positive and fz_stance above it")
    period = np.broadcast_to(np.asarray(gait.period, dtype=np.int64), (B,))
    swing = np.broadcast_to(np.asarray(gait.swing, dtype=np.int64), (B, 2))
    offset = np.broadcast_to(np.asarray(gait.offset, dtype=np.int64), (B, 2))
    dt = p.dt
    vx, vy, wz, zh = (cmd[:, i, None] for i in range(4))  # [B][1]
    c, vm = x[:, 6:8], x[:, 9:11]
    k = np.arange(N + 1)
    # reference
    yaw = ref_pose[:, 2, None] + k * (dt * wz)  # [B][N+1]
    cs, sn = np.cos(yaw), np.sin(yaw)
    vw = np.stack([cs * vx - sn * vy, sn * vx + cs * vy], axis=-1)  # Rz(yaw_k)(vx, vy)
    p0 = c if gait.anchor else ref_pose[:, 0:2]
    pk = np.empty((B, N + 1, 2))
    pk[:, 0] = p0
    for i in range(N):
        pk[:, i + 1] = pk[:, i] + dt * vw[:, i]
    Lz = p.Lbody[2] if Lbody_z is None else np.asarray(Lbody_z, dtype=np.float64)[:, None]
    x_ref = np.zeros((B, N + 1, 12))
    x_ref[:, :, 2] = yaw
    x_ref[:, :, 5] = Lz * wz
    x_ref[:, :, 6:8] = pk
    x_ref[:, :, 8] = zh
    x_ref[:, :, 9:11] = vw
    if terrain is not None:
        if map_r is None:
            map_r = terrain.map_r
        maps = np.zeros(B, dtype=np.int64) if map_r is None else np.asarray(map_r, dtype=np.int64)[:B]
        x_ref[:, :, 8] = zh + terrain_height(terrain, pk, maps[:, None])
    # contact schedule and feet
    ks = k[:N]
    fz = np.empty((B, N, 2))
    feet = []
    fb = gait.k_raibert * (vm - vw[:, 0])  # [B][2]
    for f in range(2):
        sw = swing[:, f, None]
        phi = (int(tick) + ks + offset[:, f, None]) % period[:, None]  # [B][N], int64
        swinging = phi < sw
        fz[:, :, f] = np.where(swinging, gait.fz_swing, gait.fz_stance)
        s = ks - (phi - sw)  # a stance stage: the first stage of that stance
        down = ~swinging & ((sw == 0) | (s <= 0))
        j = np.where(swinging, ks + sw - phi, s)
        jc = np.clip(j, 0, N)  # j' = min(j, N); j < 0 only where the foot is down
        half = (period - swing[:, f])[:, None] * dt / 2.0
        hx = gait.hip[f][0] + half * vx  # [B][1]
        hy = gait.hip[f][1] + half * vy
        cj, sj = np.take_along_axis(cs, jc, 1), np.take_along_axis(sn, jc, 1)
        pj = np.take_along_axis(pk, jc[:, :, None], 1)  # [B][N][2]
        F = np.empty((B, N, 3))
        F[:, :, 0] = c[:, None, 0] + (pj[:, :, 0] - p0[:, None, 0]) + (cj * hx - sj * hy) + fb[:, None, 0]
        F[:, :, 1] = c[:, None, 1] + (pj[:, :, 1] - p0[:, None, 1]) + (sj * hx + cj * hy) + fb[:, None, 1]
        F[:, :, 2] = gait.ground_z
        if terrain is not None:  # the touchdown moves to the best candidate and takes its height
            sel_xy, sel_z, _, _ = foothold_select(terrain, F[:, :, 0:2], maps[:, None])
            F[:, :, 0:2] = sel_xy
            F[:, :, 2] = gait.ground_z + sel_z
        feet.append(np.where(down[:, :, None], foot_now[:, f, None, :], F))
    plan = SrbdPlan(x_ref=x_ref, foot_r=feet[0], foot_l=feet[1], fz_max=fz)
    new_pose = np.concatenate([pk[:, 1], yaw[:, 1:2]], axis=1)
    new_feet = np.stack([feet[0][:, 0], feet[1][:, 0]], axis=1)
    return plan, new_pose, new_feet


def friction_cone(p: SrbdParams):
    """Ac (24 x 12) and constant term bc of GetConstrain (SRBD_model.cpp:237-260), R_f = I."""
    Rf = np.eye(3)
    Ac = np.zeros((24, 12))
    bc = np.zeros(24)
    for leg in range(2):
        blk = np.zeros((12, 6))
        blk[0] = [-1, 0, p.mu, 0, 0, 0]
        blk[1] = [0, -1, p.mu, 0, 0, 0]
        blk[2] = [1, 0, p.mu, 0, 0, 0]
        blk[3] = [0, 1, p.mu, 0, 0, 0]
        blk[4] = [0, 0, -1, 0, 0, 0]
        blk[5] = [0, 0, 1, 0, 0, 0]
        blk[6] = np.concatenate([p.Lfx * Rf[:, 2], -Rf[:, 1]])
        blk[7] = np.concatenate([p.Lfx * Rf[:, 2], Rf[:, 1]])
        blk[8] = np.concatenate([p.Lfz * Rf[:, 2], -Rf[:, 2]])
        blk[9] = np.concatenate([p.Lfz * Rf[:, 2], Rf[:, 2]])
        blk[10] = np.concatenate([np.zeros(3), -Rf[:, 0]])
        blk[11] = np.concatenate([np.zeros(3), Rf[:, 0]])
        Ac[12 * leg:12 * leg + 12, 6 * leg:6 * leg + 6] = blk
        bc[12 * leg + 4] = p.fmax
        bc[12 * leg + 5] = -p.fmin
    return Ac, bc


def barrier(value, mu, theta):
    """Relaxed log-barrier (SRBD_model.cpp:262-295): returns b, db, ddb."""
    inside = value > theta
    safe = np.where(inside, value, 1.0)
    b_in = -mu * np.log(safe)
    db_in = -mu / safe
    ddb_in = mu / (safe * safe)
    z = (value - 2.0 * theta) / theta
    b_out = 0.5 * mu * (z * z - 1.0) - mu * math.log(theta)
    db_out = mu * (value - 2.0 * theta) / (theta * theta)
    ddb_out = np.full_like(value, mu / (theta * theta))
    return (np.where(inside, b_in, b_out), np.where(inside, db_in, db_out),
            np.where(inside, ddb_in, ddb_out))


# ---------------------------------------------------------------------------
# batch generator
# ---------------------------------------------------------------------------
SIGMA_X = np.array([0.05] * 3 + [0.2] * 3 + [0.02] * 3 + [0.1] * 3)
U_BOX_LO = np.array([-50.0, -50.0, 0.0, -5.0, -5.0, -5.0] * 2)
U_BOX_HI = np.array([50.0, 50.0, 300.0, 5.0, 5.0, 5.0] * 2)


def sample_trajectories(batch, N, seed, p: SrbdParams, first: int = 0):
    """Per-QP linearisation points from seed + global QP index (counter-based)."""
    xr = np.array(p.x_ref, dtype=np.float64)
    xs = np.empty((batch, N + 1, 12))
    us = np.empty((batch, N, 12))
    x0 = np.empty((batch, 12))
    for i in range(batch):
        rng = np.random.default_rng([seed, first + i])
        xs[i] = xr + rng.normal(size=(N + 1, 12)) * SIGMA_X
        f = np.empty((N, 2, 6))
        f[..., 0:2] = rng.uniform(-15.0, 15.0, size=(N, 2, 2))
        f[..., 2] = rng.uniform(40.0, 110.0, size=(N, 2))
        f[..., 3:6] = rng.uniform(-2.0, 2.0, size=(N, 2, 3))
        us[i] = f.reshape(N, 12)
        x0[i] = rng.normal(size=12) * SIGMA_X  # x0 - x_nmpc(:,0) (NMPC_solver.cpp:320)
    return xs, us, x0


def build_qp(xs, us, p: Optional[SrbdParams] = None, constraints: str = "none", meta=None,
             plan: Optional[SrbdPlan] = None):
    """QP data of NMPCSolver::prepareQpStructures (NMPC_solver.cpp:276-314) at the
    linearisation points xs [B][N+1][12], us [B][N][12].  plan (SrbdPlan): per-robot,
    per-stage reference, feet and force limits in place of SrbdParams' constants.
    Returns (OcpQpBatch, fc)."""
    p = p or SrbdParams()
    batch, N = us.shape[0], us.shape[1]
    A, B, b = shooting_dynamics(xs[:, :-1], xs[:, 1:], us, p, plan)
    Ac, bc = friction_cone(p)
    fc = np.einsum("ij,bkj->bki", Ac, us) + plan_cone_offsets(bc, plan)
    _, db, ddb = barrier(fc, p.mu_b, p.theta_b)
    Qd = np.diag(np.array(p.Q, dtype=np.float64))
    Qf = float(N) * np.diag(np.array(p.Qf, dtype=np.float64))  # Qf_ = N * Qf (NMPC_solver.cpp:58)
    Rm = p.R * np.eye(12)
    xr = np.array(p.x_ref, dtype=np.float64)
    xr_k, xr_N = xr, xr
    if plan is not None and plan.x_ref is not None:
        xr_k, xr_N = np.asarray(plan.x_ref)[:, :N], np.asarray(plan.x_ref)[:, N]
    Q = np.empty((batch, N + 1, 12, 12))
    Q[:, :N] = Qd
    Q[:, N] = Qf
    q = np.empty((batch, N + 1, 12))
    q[:, :N] = np.einsum("ij,bkj->bki", Qd, xs[:, :N] - xr_k)
    q[:, N] = np.einsum("ij,bj->bi", Qf, xs[:, N] - xr_N)
    R = Rm + np.einsum("ci,bkc,cj->bkij", Ac, ddb, Ac)
    r = np.einsum("ij,bkj->bki", Rm, us) + np.einsum("ci,bkc->bki", Ac, db)
    S = np.zeros((batch, N, 12, 12))
    qp = OcpQpBatch(N=N, nx=12, nu=12, A=A, B=B, b=b, Q=Q, S=S, R=R, q=q, r=r,
                    meta=dict(meta or {}, constraints=constraints))
    if constraints == "box_u":
        qp.lbu = U_BOX_LO - us
        hi = U_BOX_HI
        if plan is not None and plan.fz_max is not None:  # the schedule caps each foot's fz
            hi = np.broadcast_to(U_BOX_HI, us.shape).copy()
            hi[..., 2] = np.minimum(hi[..., 2], plan.fz_max[..., 0])
            hi[..., 8] = np.minimum(hi[..., 8], plan.fz_max[..., 1])
        qp.ubu = hi - us
    elif constraints == "cone":
        qp.ng = 24
        qp.D = np.broadcast_to(Ac, (batch, N, 24, 12)).copy()
        qp.C = None  # the cone constrains u only (C = 0): passed as NULL, the C-free kernel path
        qp.lg = np.zeros((batch, N + 1, 24))
        qp.lg[:, :N] = -fc
        qp.ug = np.full((batch, N + 1, 24), 1e10)
        qp.lg_mask = np.zeros((batch, N + 1, 24))
        qp.lg_mask[:, :N] = 1.0
        qp.ug_mask = np.zeros((batch, N + 1, 24))
    elif constraints != "none":
        raise ValueError(f"unknown constraints {constraints!r}")
    return qp, fc


def generate_batch(batch: int, N: int = 20, seed: int = 1001, constraints: str = "none",
                   p: Optional[SrbdParams] = None, first: int = 0):
    """Build `batch` SRBD OCP-QPs exactly as prepareQpStructures does.

    constraints: "none" (the reference's own QP: friction cone as a barrier in
    the cost, no inequalities), "box_u" (config 3: u + du inside per-foot force /
    torque boxes), "cone" (config 5: lg <= Ac du with lg = -f(u), ug masked).
    Returns (OcpQpBatch, x0)."""
    p = p or SrbdParams()
    xs, us, x0 = sample_trajectories(batch, N, seed, p, first)
    qp, _ = build_qp(xs, us, p, constraints, meta={"seed": seed, "first": first})
    return qp, x0
