"""TEST INFRASTRUCTURE ONLY -- the inputs of the linearisation's backward tests (CPU and GPU):
robots from robots_host.draw, a plan with distinct values per robot and stage, random cotangents.

The relaxed barrier's third derivative jumps at v = theta_b and min(u_hi, fz_max) has a kink, so
the builder asserts, for every element, |v_c - theta_b| >= MARGIN and |fz_max - u_hi[fz]| >= MARGIN,
and that both barrier branches (and, with a plan's fz_max, both sides of the min) occur.  SEEDS
holds, per (B, N), a seed for which that is so with no element excluded, for robots and plan
given, either alone, and neither (found on the CPU)."""
from __future__ import annotations

import numpy as np

import nmpc_plan_host as PH
import robots_host as BH
from linearize_vjp_host import COTANGENTS
from rollout_host import FIELDS as PLAN_FIELDS

MARGIN = 1e-2
SEEDS = {(3, 3): 0, (3, 2): 0, (5, 13): 1, (2, 33): 0, (4, 1): 0, (70, 1): 1, (3, 4): 0}
# what puts every output at O(1) or above for unit normal draws: A, B and b carry a factor dt, and
# R, r reach mu and fz_max through the barrier's curvature mu_b / v^2 with v of order 30
SCALE = {"A": 60.0, "B": 60.0, "b": 60.0, "R": 1e3, "r": 1e3}


def case_plan(sm, p, B, N, seed, fields=PLAN_FIELDS):
    """random_plan's references and feet; fz_max on both sides of u_hi[fz] = 300: a swing foot at
    1.0, a stance foot in [150, 290] or in [310, 600]."""
    rng = np.random.default_rng(seed)
    kind = rng.uniform(size=(B, N, 2))
    fz = np.where(kind < 0.2, 1.0, np.where(kind < 0.6, rng.uniform(150.0, 290.0, size=(B, N, 2)),
                                            rng.uniform(310.0, 600.0, size=(B, N, 2))))
    fz[0, 0, 0], fz[0, 0, 1], fz[B - 1, N - 1, 0] = 1.0, 450.0, 200.0  # every kind occurs
    # references within +-0.3 of the default and feet within +-0.15 m, as nmpc_plan_host.random_plan
    x_ref = np.array(p.x_ref) + rng.uniform(-0.3, 0.3, size=(B, N + 1, 12))
    foot_r = np.array(p.foot_r) + rng.uniform(-0.15, 0.15, size=(B, N, 3))
    foot_l = np.array(p.foot_l) + rng.uniform(-0.15, 0.15, size=(B, N, 3))
    vals = dict(x_ref=x_ref, foot_r=foot_r, foot_l=foot_l, fz_max=fz)
    return sm.SrbdPlan(**{k: (v if k in fields else None) for k, v in vals.items()})


def margins(sm, params, plan, us):
    """(smallest |v_c - theta_b|, smallest |fz_max - u_hi[fz]|, both barrier branches occur, both
    sides of the min occur) over every robot, stage and row."""
    B, N = us.shape[0], us.shape[1]
    fz_max = None if plan is None else plan.fz_max
    dv, below, above = np.inf, False, False
    for i, q in enumerate(params):
        Ac, bc = sm.friction_cone(q)
        off = np.tile(bc, (N, 1))
        if fz_max is not None:
            off[:, 4], off[:, 16] = fz_max[i, :, 0], fz_max[i, :, 1]
        v = us[i] @ Ac.T + off
        dv = min(dv, float(np.abs(v - q.theta_b).min()))
        below, above = below or bool((v <= q.theta_b).any()), above or bool((v > q.theta_b).any())
    fz = np.array([[q.fmax] for q in params]) if fz_max is None else fz_max
    u_hi = float(sm.U_BOX_HI[2])
    return dv, float(np.abs(fz - u_hi).min()), below and above, bool((fz < u_hi).any() and (fz > u_hi).any())


def make_case(sm, B, N, seed=None, robots=BH.MODEL_FIELDS, plan=PLAN_FIELDS):
    """(p, params, plan, xs, us): params one SrbdParams per robot (the draw's `robots` fields, the
    others p's), plan a SrbdPlan of the `plan` fields or None.  Asserts the margins."""
    p = sm.SrbdParams()
    seed = SEEDS[(B, N)] if seed is None else seed
    xs, us, _ = sm.sample_trajectories(B, N, 7000 + seed, p)
    params = BH.only(p, BH.draw(p, B, 8000 + seed), robots)
    pl = case_plan(sm, p, B, N, 9000 + seed, plan) if plan else None
    dv, dz, branches, sides = margins(sm, params, pl, us)
    assert dv >= MARGIN and dz >= MARGIN, (B, N, seed, dv, dz)
    assert branches, "one barrier branch is missing"
    assert sides or pl is None or pl.fz_max is None, "one side of min(u_hi, fz_max) is missing"
    return p, params, pl, xs, us


def cotangents(B, N, constraints, seed, only=None):
    """Random normal cotangents in the packed layout for COTANGENTS[constraints] (`only`: those
    names alone), scaled so that every output is O(1) or larger."""
    rng = np.random.default_rng(seed)
    shapes = {"A": (N, 12, 12), "B": (N, 12, 12), "b": (N, 12), "Q": (N + 1, 12, 12), "R": (N, 12, 12),
              "q": (N + 1, 12), "r": (N, 12), "ubu": (N, 12), "D": (N, 12, 24), "lg": (N + 1, 24)}
    out = {}
    for name in COTANGENTS[constraints]:
        g = SCALE.get(name, 1.0) * rng.normal(size=(B,) + shapes[name])
        if only is None or name in only:
            out[name] = g
    return out
