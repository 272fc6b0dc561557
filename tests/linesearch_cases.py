"""TEST INFRASTRUCTURE ONLY -- designed inputs of the filter line search (CPU and GPU tests): a
named table of single-robot cases (xs, us, dx, du, alpha0) that together take every branch of the
filter and every way a search can stop, batched so that neighbouring robots of one launch take
different branches and different numbers of trials.

A case is a recipe (`kind`), a seed and the recipe's numbers; the numbers were chosen on the CPU
(scripts/linesearch_case_search.py) per batch, because the open-loop rollout behind most recipes
changes with the horizon, the model's parameters, the robot and the plan.  `outcomes` names what
a host trace reached; tests/test_linesearch_cases_cpu.py holds every batch to the outcomes listed
in OUTCOMES, so the table cannot lose one silently.

The recipes:
  a feasible base point: xs rolled out of xs[0] under us with the model's own RK4 step: theta = 0
    up to rounding, so the Armijo branch is open;
  a feasible direction: for a random du, dx = (rollout(us + h du) - rollout(us - h du)) / 2h,
    signed for descent (dphi < 0) or ascent;
  a nearly feasible base point: the rolled-out xs plus Gaussian noise of a given sigma;
  a restoring direction: dx = c (rollout(us + du) - xs) from a base point far from feasible: the
    trial's theta is about (1 - c alpha)^2 theta."""
from __future__ import annotations

import dataclasses
import functools
import json
from pathlib import Path

import numpy as np

import nmpc_plan_host as PH
import robots_host as BH

LS_FIELDS = ("theta_max", "theta_min", "eta", "beta_phi", "beta_theta", "beta_alpha", "alpha_min")
MODEL_FIELDS = ("mu_b", "theta_b", "dt", "R")
# the two parameter sets: the defaults, and every srbd_linesearch_params field and the model's
# mu_b, theta_b, dt, R changed (beta_phi != beta_theta; beta_alpha = 0.7: alpha no longer halves)
PARAM_SETS = {
    "default": dict(ls={}, model={}),
    "changed": dict(ls=dict(theta_max=1e-3, theta_min=1e-7, eta=0.3, beta_phi=0.5, beta_theta=0.05,
                            beta_alpha=0.7, alpha_min=3e-3),
                    model=dict(mu_b=0.05, theta_b=8.0, dt=0.01, R=3e-4)),
}
MARGIN = 1e-8  # of every comparison the host search evaluates: check_linesearch's bound
# |v_c - theta_b| at every evaluated point.  The relaxed barrier is twice continuously
# differentiable at theta_b, so the wrong formula there would cost nothing the tests could see;
# the bound keeps the statement "the device took the host's formula" true all the same: a device
# v differs from the host's by a few ulp of |v| <= 1e3, that is by <= 1e-12.
BARRIER_MARGIN = 1e-6

# the cone rows that read a force (rows 10, 11 of each foot are -tx, tx: one of them is always <= 0)
FORCE_ROWS = [c for c in range(24) if c % 12 < 10]

OUTCOMES = (
    "theta:accept-first", "theta:accept-after-2-rejects", "theta:exhaust",
    "armijo:accept-first", "armijo:reject-then-accept",
    "mixed:accept-phi-only", "mixed:accept-theta-only", "mixed:exhaust",
    "feasible-not-descent", "switch", "floor:at", "floor:below", "exhausted",
    "converged:yes", "converged:no-dphi", "converged:no-theta",
    "barrier:below", "barrier:above", "barrier:negative", "barrier:crossing",
)


def model_of(sm, set_name, base=None):
    """The SrbdParams of a parameter set (on top of `base`: one robot's parameters)."""
    return dataclasses.replace(base or sm.SrbdParams(), **PARAM_SETS[set_name]["model"])


def ls_of(set_name):
    return dict(PH.LS_DEFAULTS, **PARAM_SETS[set_name]["ls"])


# ---- the recipes' parts ----
def _stage_plan(sm, plan, k):
    if plan is None or (plan.foot_r is None and plan.foot_l is None):
        return None
    return sm.SrbdPlan(foot_r=None if plan.foot_r is None else plan.foot_r[k],
                       foot_l=None if plan.foot_l is None else plan.foot_l[k])


def rollout(sm, p, plan, x0, us):
    """xs [N+1][12] from x0 under us with the model's RK4 step (the plan's feet per stage)."""
    xs = np.empty((us.shape[0] + 1, 12))
    xs[0] = x0
    for k in range(us.shape[0]):
        xs[k + 1] = sm._rk4_step(xs[k], us[k], p, p.dt, _stage_plan(sm, plan, k))
    return xs


def _start(sm, p, plan, N, rng):
    """(x0, us): sample_trajectories' draw of one robot's first state and inputs."""
    xr = np.array(p.x_ref, dtype=np.float64) if plan is None or plan.x_ref is None else plan.x_ref[0]
    x0 = xr + rng.normal(size=12) * sm.SIGMA_X
    f = np.empty((N, 2, 6))
    f[..., 0:2] = rng.uniform(-15.0, 15.0, size=(N, 2, 2))
    f[..., 2] = rng.uniform(40.0, 110.0, size=(N, 2))
    f[..., 3:6] = rng.uniform(-2.0, 2.0, size=(N, 2, 3))
    return x0, f.reshape(N, 12)


def _feasible_direction(sm, p, plan, x0, us, du, h=1e-6):
    return (rollout(sm, p, plan, x0, us + h * du) - rollout(sm, p, plan, x0, us - h * du)) / (2.0 * h)


def _dphi(sm, p, plan, xs, us, dx, du):
    N = us.shape[0]
    Ac, bc = sm.friction_cone(p)
    _, _, Jx, Ju = PH.merit(sm, p, plan, xs, us, N, Ac, bc)
    return float(np.sum(dx * Jx) + np.sum(du * Ju))


def _signed_direction(sm, p, plan, x0, xs, us, rng, sign, stages=None):
    """A feasible direction (dx, du) at the rolled-out point with sign(dphi) = sign, and its dphi;
    stages: du moves the last `stages` stages only."""
    du = rng.normal(size=us.shape)
    if stages is not None:
        du[:us.shape[0] - stages] = 0.0
    dx = _feasible_direction(sm, p, plan, x0, us, du)
    g = _dphi(sm, p, plan, xs, us, dx, du)
    flip = 1.0 if g * sign > 0.0 else -1.0
    return flip * dx, flip * du, flip * g


def build_case(sm, p, plan, N, kind, seed, **v):
    """One robot's (xs, us, dx, du) by recipe `kind` under the model p and the robot's plan rows.
      descent / ascent   feasible base, feasible direction x scale; sigma > 0 adds N(0, sigma^2)
                         noise to the base point's xs[1:]; dphi = the target: the scale that gives it;
                         kink > 0 adds N(0, kink^2) to dx[1:]: the trial's theta is about
                         6 N (alpha kink)^2, above theta_max at a long alpha and below it at a short one
      combo              feasible base, scale (d1 - c d2) of two descent directions with c such
                         that dphi is `frac` of d1's
      overshoot          as combo with du on the last `stages` stages only (the dynamics are affine in
                         u, so theta stays small while the terminal cost bends phi), scaled so that
                         the minimiser of phi's quadratic model along the step is at alpha = `at`:
                         the Armijo test fails beyond about twice that (2 (1 - eta) times); sigma > 0
                         as above: a theta between two values of theta_min, where one takes the
                         Armijo test and the other the mixed one, which accepts any decrease
      restore            base point sample_trajectories' (far from feasible), du = scale x random,
                         dx = c (rollout(us + du) - xs); push: du also drives stage 0's right fz
                         to -5 (below fmin) and stage N-1's left fz to 2 (below theta_b)
      restore_ascent     nearly feasible base (sigma), dx = (rollout(us) - xs) + scale x an
                         ascent direction's, du = scale x its du
      random             base point sample_trajectories', dx = 0.05 N(0, 1), du = 2 N(0, 1)"""
    rng = np.random.default_rng([seed, N])
    x0, us = _start(sm, p, plan, N, rng)
    xs = rollout(sm, p, plan, x0, us)
    if kind in ("descent", "ascent"):
        dx, du, g = _signed_direction(sm, p, plan, x0, xs, us, rng, -1.0 if kind == "descent" else 1.0)
        if v.get("sigma", 0.0) > 0.0:
            xs = xs.copy()
            xs[1:] += v["sigma"] * rng.normal(size=(N, 12))
        s = v["dphi"] / _dphi(sm, p, plan, xs, us, dx, du) if "dphi" in v else v["scale"]
        dx = s * dx
        if v.get("kink", 0.0) > 0.0:
            dx[1:] += v["kink"] * rng.normal(size=(N, 12))
        return xs, us, dx, s * du
    if kind == "combo":
        dx1, du1, g1 = _signed_direction(sm, p, plan, x0, xs, us, rng, -1.0)
        dx2, du2, g2 = _signed_direction(sm, p, plan, x0, xs, us, rng, -1.0)
        c = (1.0 - v["frac"]) * g1 / g2
        return xs, us, v["scale"] * (dx1 - c * dx2), v["scale"] * (du1 - c * du2)
    if kind == "overshoot":
        dx1, du1, g1 = _signed_direction(sm, p, plan, x0, xs, us, rng, -1.0, v["stages"])
        dx2, du2, g2 = _signed_direction(sm, p, plan, x0, xs, us, rng, -1.0, v["stages"])
        c = (1.0 - v["frac"]) * g1 / g2
        dx, du = dx1 - c * dx2, du1 - c * du2
        Ac, bc = sm.friction_cone(p)
        phi = [PH.merit(sm, p, plan, xs + e * dx, us + e * du, N, Ac, bc)[0] for e in (-1.0, 0.0, 1.0)]
        H = phi[0] - 2.0 * phi[1] + phi[2]
        s = -v["frac"] * g1 / H / v["at"] if H > 0.0 else 1.0
        if v.get("sigma", 0.0) > 0.0:
            xs = xs.copy()
            xs[1:] += v["sigma"] * rng.normal(size=(N, 12))
        return xs, us, s * dx, s * du
    if kind == "restore_ascent":
        dx, du, _ = _signed_direction(sm, p, plan, x0, xs, us, rng, 1.0)
        noisy = xs.copy()
        noisy[1:] += v["sigma"] * rng.normal(size=(N, 12))
        return noisy, us, (xs - noisy) + v["scale"] * dx, v["scale"] * du
    xr = np.array(p.x_ref, dtype=np.float64) if plan is None or plan.x_ref is None else plan.x_ref
    far = xr + rng.normal(size=(N + 1, 12)) * sm.SIGMA_X
    if kind == "restore":
        du = v["scale"] * rng.normal(size=us.shape)
        if v.get("push"):
            du[0, 2] = -5.0 - us[0, 2]
            du[N - 1, 8] = 2.0 - us[N - 1, 8]
        return far, us, v["c"] * (rollout(sm, p, plan, far[0], us + du) - far), du
    if kind == "random":
        return far, us, 0.05 * rng.normal(size=far.shape), 2.0 * rng.normal(size=us.shape)
    raise ValueError(kind)


# ---- what a host search reached ----
def cone_values(sm, p, plan, u):
    """v [N][24] = Ac u + bc with the plan's fz_max: the barrier's arguments."""
    Ac, bc = sm.friction_cone(p)
    return u @ Ac.T + np.broadcast_to(sm.plan_cone_offsets(bc, plan), (u.shape[0], 24))


def run_host(sm, p, plan, case, ls):
    """The host search of one case with its trace and what the barrier saw.  Returns a dict:
    the line_search tuple's entries by name, trace, outcomes, barrier_margin."""
    xs, us, dx, du, alpha0 = case
    trace = []
    xn, un, alpha, phi, theta, dphi, conv, margin = PH.line_search(sm, p, plan, xs, us, dx, du, float(alpha0),
                                                                  ls=ls, trace=trace)
    accepted = trace[-1].alpha if trace and trace[-1].accepted else None
    out = outcomes(trace, alpha0, alpha, theta, dphi, conv, ls)
    v0 = cone_values(sm, p, plan, us)
    points = [v0] + [cone_values(sm, p, plan, us + t.alpha * du) for t in trace]
    trial = np.stack(points[1:]) if trace else v0[None]
    if (trial <= p.theta_b).any():
        out.add("barrier:below")
    if (trial > p.theta_b).any():
        out.add("barrier:above")
    if trace and (trial[..., FORCE_ROWS] < 0.0).any():
        out.add("barrier:negative")
    if accepted is not None and ((v0 > p.theta_b) != (points[-1] > p.theta_b)).any():
        out.add("barrier:crossing")
    return dict(xs=xn, us=un, alpha=alpha, phi=phi, theta=theta, dphi=dphi, converged=conv, margin=margin,
                trace=trace, accepted=accepted, outcomes=out,
                barrier_margin=float(np.abs(np.stack(points) - p.theta_b).min()))


def outcomes(trace, alpha0, alpha, theta, dphi, converged, ls):
    """The names in OUTCOMES (the barrier's apart) that one search reached."""
    out = set()
    if not trace:
        out.add("floor:at" if alpha0 == ls["alpha_min"] else "floor:below")
    else:
        last = trace[-1]
        rejects = trace[:-1] if last.accepted else trace
        if last.accepted:
            if len(trace) == 1 and last.branch in ("theta", "armijo"):
                out.add(last.branch + ":accept-first")
            if last.branch == "theta" and sum(t.branch == "theta" for t in rejects) >= 2:
                out.add("theta:accept-after-2-rejects")
            if last.branch == "armijo" and any(t.branch == "armijo" for t in rejects):
                out.add("armijo:reject-then-accept")
            if last.branch == "mixed" and last.phi_clause != last.theta_clause:
                out.add("mixed:accept-phi-only" if last.phi_clause else "mixed:accept-theta-only")
        else:
            # the returned alpha is the first of alpha0 beta_alpha^j that is <= alpha_min
            a, n = float(alpha0), 0
            while a > ls["alpha_min"]:
                a, n = ls["beta_alpha"] * a, n + 1
            if a == alpha and n == len(trace):
                out.add("exhausted")
            if all(t.branch == "theta" for t in trace):
                out.add("theta:exhaust")
            if len(trace) >= 3 and all(t.branch == "mixed" for t in trace[-3:]):  # mixed rejects to the end
                out.add("mixed:exhaust")
        if theta < ls["theta_min"] and dphi >= 0.0 and any(
                t.branch == "mixed" and t.theta_a < ls["theta_min"] for t in trace):
            out.add("feasible-not-descent")
        if trace[0].branch == "theta" and last.branch in ("mixed", "armijo"):
            out.add("switch")
    if converged:
        out.add("converged:yes")
    elif theta < 1e-6 and -2e-3 < dphi <= -1e-3:  # theta alone would have passed
        out.add("converged:no-dphi")
    elif theta >= 1e-6 and abs(dphi) < 1e-3:  # dphi alone would have passed
        out.add("converged:no-theta")
    return out


# ---- the table ----
# one launch's robots, in this order: neighbours take different branches and trial counts.
# name: (what the case must reach under the default set, under the changed set)
_BOTH = lambda *names: (frozenset(names), frozenset(names))
CASES = {
    "theta_first": _BOTH("theta:accept-first", "barrier:crossing", "barrier:negative"),
    "armijo_first": _BOTH("armijo:accept-first"),
    "theta_rejects": _BOTH("theta:accept-after-2-rejects"),
    "armijo_reject": _BOTH("armijo:reject-then-accept"),
    "theta_exhaust": _BOTH("theta:exhaust", "exhausted"),
    "mixed_phi": _BOTH("mixed:accept-phi-only"),
    "floor_at": _BOTH("floor:at"),
    # (1 - c)^2 = 0.96 of theta at the first trial: inside beta_theta = 1e-6, outside 0.05
    "theta_slow": (frozenset(["theta:accept-first"]), frozenset(["theta:exhaust", "exhausted"])),
    "switch": _BOTH("switch"),
    "mixed_theta": _BOTH("mixed:accept-theta-only"),
    "mixed_exhaust": _BOTH("mixed:exhaust", "exhausted"),
    "conv_no_dphi": _BOTH("converged:no-dphi", "armijo:accept-first"),
    "not_descent": _BOTH("feasible-not-descent", "exhausted", "converged:yes"),
    "floor_below": _BOTH("floor:below"),
    "conv_no_theta": _BOTH("converged:no-theta"),
}
# name: (parameter set, N, variant): "plan" a random_plan (the PLAN kernels), "robots" per-robot
# mass, Lbody, mu, Q, Qf, R (the ROBOT kernels), "one" the batch of one robot
BATCHES = {
    "default-N20": ("default", 20, None), "changed-N20": ("changed", 20, None),
    "default-N1": ("default", 1, None), "changed-N1": ("changed", 1, None),
    "default-N31": ("default", 31, None), "changed-N31": ("changed", 31, None),
    "default-N32": ("default", 32, None), "changed-N32": ("changed", 32, None),
    "changed-N20-plan": ("changed", 20, "plan"), "default-N20-robots": ("default", 20, "robots"),
    "default-N20-one": ("default", 20, "one"),
}
ONE = "armijo_reject"  # the robot of the batch of one
TABLE_PATH = Path(__file__).resolve().parent / "golden" / "linesearch_cases.json"
PLAN_SEED, ROBOTS_SEED = 12, 102


def batch_names(batch_name):
    return (ONE,) if BATCHES[batch_name][2] == "one" else tuple(CASES)


def batch_models(sm, batch_name):
    """(params: one SrbdParams per robot, plan: a SrbdPlan or None) of a batch."""
    set_name, N, variant = BATCHES[batch_name]
    B = len(batch_names(batch_name))
    p = model_of(sm, set_name)
    params = BH.draw(p, B, ROBOTS_SEED) if variant == "robots" else [p] * B
    plan = PH.random_plan(sm, p, B, N, PLAN_SEED) if variant == "plan" else None
    return params, plan


def start_alpha(alpha0, ls):
    """A row's alpha0: a number, or "floor" (alpha_min exactly) or "below" (half of it)."""
    return {"floor": ls["alpha_min"], "below": 0.5 * ls["alpha_min"]}.get(alpha0, alpha0)


@functools.lru_cache(maxsize=None)
def _table():
    return json.loads(TABLE_PATH.read_text())


_BATCH = {}


def batch(sm, batch_name):
    """One launch: dict(names, params, plan, ls, xs [B][N+1][12], us, dx, du, alpha0 [B], host: the
    run_host dict per robot).  Built once; the arrays are shared, so leave them unchanged."""
    if batch_name in _BATCH:
        return _BATCH[batch_name]
    set_name, N, variant = BATCHES[batch_name]
    ls = ls_of(set_name)
    params, plan = batch_models(sm, batch_name)
    rows = {r["name"]: r for r in _table()["default-N20" if variant == "one" else batch_name]}
    names, arrays, host, left_out = batch_names(batch_name), [], [], []
    for i, name in enumerate(names):
        r = rows.get(name)
        if r is None:  # the search found no inputs with the margins: the CPU test names it
            left_out.append(name)
            continue
        pl = None if plan is None else plan.robot(i)
        case = build_case(sm, params[i], pl, N, r["kind"], r["seed"], **r["args"]) + (start_alpha(r["alpha0"], ls),)
        arrays.append(case)
        host.append(run_host(sm, params[i], pl, case, ls))
    keep = [i for i, n in enumerate(names) if n not in left_out]
    if plan is not None:
        plan = sm.SrbdPlan(*[a[keep] for a in (plan.x_ref, plan.foot_r, plan.foot_l, plan.fz_max)])
    out = dict(names=[names[i] for i in keep], left_out=left_out, params=[params[i] for i in keep], plan=plan,
               ls=ls, set=set_name, N=N, variant=variant, host=host,
               **{k: np.ascontiguousarray(np.stack([c[j] for c in arrays]))
                  for j, k in enumerate(("xs", "us", "dx", "du"))},
               alpha0=np.array([c[4] for c in arrays], dtype=np.float64))
    _BATCH[batch_name] = out
    return out
