"""TEST INFRASTRUCTURE ONLY -- the backward pass of the SRBD linearisation in numpy, per robot
(the yardstick of srbd_qp_srbd_linearize_backward_f64, itself held to central
differences of robots_host.build_qp by tests/test_linearize_backward_cpu.py).

For every array X that build_qp writes the caller passes a cotangent in X's packed (C-ABI)
layout; the result for a parameter theta of robot i is sum_X <G_X, dX / d theta> over that
robot's blocks.  The linearisation point xs, us is held fixed.  The dynamics' part is stated in
forward mode (tangents of the ten directions through the RK4), the opposite of what the kernel does.
"""
from __future__ import annotations

import dataclasses

import numpy as np

__all__ = ["OUTPUTS", "COTANGENTS", "linearize_vjp", "contraction"]

OUTPUTS = ("mass", "Lbody", "mu", "Q", "Qf", "R", "x_ref", "foot_r", "foot_l", "fz_max")
# the cotangents that are read, per constraints mode
COTANGENTS = {"none": ("A", "B", "b", "Q", "R", "q", "r"),
              "box_u": ("A", "B", "b", "Q", "R", "q", "r", "ubu"),
              "cone": ("A", "B", "b", "Q", "R", "q", "r", "D", "lg")}
_FZ = (2, 8)  # fz of the right and of the left foot in u


def _skew_basis():
    e = np.eye(3)
    S = np.zeros((3, 3, 3))  # S[a] = d skew(p) / d p_a
    for a in range(3):
        S[a] = np.array([[0.0, -e[a, 2], e[a, 1]], [e[a, 2], 0.0, -e[a, 0]], [-e[a, 1], e[a, 0], 0.0]])
    return S


def _slope_partials(sm, q, x, u):
    """d f / d theta at the stages' (x, u) [N][12] for theta = (1 / Lbody[0..2], 1 / mass,
    foot_r[0..2], foot_l[0..2]): [N][12][10], one line each."""
    N = x.shape[0]
    r, l = x[:, 0:3], x[:, 3:6]
    R, Jlt = sm.expm(r), sm.jlt(r)
    P = np.zeros((N, 12, 10))
    for j in range(3):  # f[0:3] = Jlt R diag(iL) R' l
        P[:, 0:3, j] = np.einsum("kab,kb->ka", Jlt, R[:, :, j]) * np.einsum("kb,kb->k", R[:, :, j], l)[:, None]
    P[:, 9:12, 3] = u[:, 0:3] + u[:, 6:9]  # f[9:12] = (f0 + f1) / m + g
    S = _skew_basis()
    for a in range(3):  # f[3:6] = ... + (foot - pos) x f
        P[:, 3:6, 4 + a] = u[:, 0:3] @ S[a].T
        P[:, 3:6, 7 + a] = u[:, 6:9] @ S[a].T
    return P


def _defect_tangents(sm, q, plan, x, u):
    """d b / d theta [N][12][10] of b = RK4(x, u) - x_next (shooting_dynamics), the tangents
    carried forward through the four slopes."""
    dt = q.dt
    f = lambda xa: sm.continuous(xa, u, q, True, plan)
    k1, J1, _ = f(x)
    T1 = _slope_partials(sm, q, x, u)
    x2 = x + 0.5 * dt * k1
    k2, J2, _ = f(x2)
    T2 = _slope_partials(sm, q, x2, u) + J2 @ (0.5 * dt * T1)
    x3 = x + 0.5 * dt * k2
    k3, J3, _ = f(x3)
    T3 = _slope_partials(sm, q, x3, u) + J3 @ (0.5 * dt * T2)
    x4 = x + dt * k3
    _, J4, _ = f(x4)
    T4 = _slope_partials(sm, q, x4, u) + J4 @ (dt * T3)
    return (dt / 6.0) * (T1 + 2.0 * T2 + 2.0 * T3 + T4)


def _robot(sm, q, plan, plan_mode, xs, us, constraints, G, qf_scale):
    """One robot: q its SrbdParams, plan its rows (SrbdPlan.robot) or None, xs [N+1][12], us [N][12],
    G the cotangents of its blocks in math orientation (a missing one is zero)."""
    N = us.shape[0]
    z = lambda *shape: np.zeros(shape)
    GA, GB, GR = G.get("A", z(N, 12, 12)), G.get("B", z(N, 12, 12)), G.get("R", z(N, 12, 12))
    Gb, Gr = G.get("b", z(N, 12)), G.get("r", z(N, 12))
    GQ, Gq = G.get("Q", z(N + 1, 12, 12)), G.get("q", z(N + 1, 12))
    out = {}
    # ---- cost: Q = diag(w), q = diag(w) (x - x_ref), w = Q (k < N), s Qf (k = N) ----
    s = float(N) if qf_scale is None or qf_scale <= 0 else float(qf_scale)
    xr = np.tile(np.array(q.x_ref, dtype=np.float64), (N + 1, 1))
    if plan is not None and plan.x_ref is not None:
        xr = np.asarray(plan.x_ref, dtype=np.float64)
    e = xs - xr
    diag = np.einsum("kjj->kj", GQ)
    term = diag + Gq * e
    out["Q"] = term[:N].sum(axis=0)
    out["Qf"] = s * term[N]
    w = np.vstack([np.tile(np.array(q.Q, dtype=np.float64), (N, 1)), s * np.array(q.Qf, dtype=np.float64)[None]])
    out["x_ref"] = -w * Gq
    # ---- input cost and friction barrier ----
    Ac, bc = sm.friction_cone(q)
    fz_max = np.full((N, 2), float(q.fmax))
    if plan is not None and plan.fz_max is not None:
        fz_max = np.asarray(plan.fz_max, dtype=np.float64)
    off = np.tile(bc, (N, 1))
    off[:, 4], off[:, 16] = fz_max[:, 0], fz_max[:, 1]
    v = us @ Ac.T + off
    _, db, ddb = sm.barrier(v, q.mu_b, q.theta_b)
    d3b = np.where(v > q.theta_b, -2.0 * q.mu_b / np.where(v > q.theta_b, v, 1.0) ** 3, 0.0)
    s1 = Gr @ Ac.T
    s2 = np.einsum("ci,kij,cj->kc", Ac, GR, Ac)
    out["R"] = float(np.einsum("kii->", GR) + np.sum(Gr * us))
    vbar = ddb * s1 + d3b * s2
    if constraints == "cone":
        vbar = vbar - G.get("lg", z(N + 1, 24))[:N]
    gfz = np.stack([vbar[:, 4], vbar[:, 16]], axis=1)
    if constraints == "box_u" and plan_mode and "ubu" in G:
        u_hi = sm.U_BOX_HI
        for leg in range(2):
            gfz[:, leg] += np.where(fz_max[:, leg] < u_hi[_FZ[leg]], G["ubu"][:, _FZ[leg]], 0.0)
    out["fz_max"] = gfz
    gmu = 0.0
    GRs = GR + np.swapaxes(GR, -1, -2)
    for leg in range(2):
        fz = _FZ[leg]
        for c in range(12 * leg, 12 * leg + 4):
            gmu += np.sum(vbar[:, c] * us[:, fz] + db[:, c] * Gr[:, fz] + ddb[:, c] * (GRs[:, fz, :] @ Ac[c]))
            if constraints == "cone" and "D" in G:
                gmu += np.sum(G["D"][:, c, fz])
    out["mu"] = float(gmu)
    # ---- dynamics: A affine in 1 / Lbody, B linear in the feet and in 1 / mass, b through the RK4 ----
    x, xn = xs[:N], xs[1:]
    inf = float("inf")
    A0 = sm.shooting_dynamics(x, xn, us, dataclasses.replace(q, Lbody=(inf, inf, inf)), plan)[0]
    giL = np.zeros(3)
    for j in range(3):
        Lb = tuple(1.0 if i == j else inf for i in range(3))
        Aj = sm.shooting_dynamics(x, xn, us, dataclasses.replace(q, Lbody=Lb), plan)[0]
        giL[j] = np.sum(GA * (Aj - A0))
    S = _skew_basis()
    gfr = q.dt * np.einsum("kij,aij->ka", GB[:, 3:6, 0:3], S)
    gfl = q.dt * np.einsum("kij,aij->ka", GB[:, 3:6, 6:9], S)
    gim = q.dt * float(np.einsum("kii->", GB[:, 9:12, 0:3]) + np.einsum("kii->", GB[:, 9:12, 6:9]))
    T = np.einsum("ki,kit->kt", Gb, _defect_tangents(sm, q, plan, x, us))  # [N][10]
    giL += T[:, 0:3].sum(axis=0)
    gim += T[:, 3].sum()
    out["foot_r"] = gfr + T[:, 4:7]
    out["foot_l"] = gfl + T[:, 7:10]
    out["Lbody"] = -giL / np.array(q.Lbody, dtype=np.float64) ** 2
    out["mass"] = float(-gim / q.mass ** 2)
    return out


def linearize_vjp(sm, params, xs, us, constraints, cot, plan=None, qf_scale=None):
    """The ten gradients {name: [B]...} (OUTPUTS; shapes of srbd_lin_grad_f64) of
    sum_X <cot[X], X> over the arrays robots_host.build_qp(sm, params, xs, us, constraints, plan)
    returns.  params: one SrbdParams per robot; plan: a SrbdPlan or None; cot: {name: array in
    the packed layout}, a missing or None entry is zero; only COTANGENTS[constraints] are read."""
    B, N = us.shape[0], us.shape[1]
    plan_mode = plan is not None and any(getattr(plan, k) is not None for k in ("x_ref", "foot_r", "foot_l", "fz_max"))
    rows = {"A": 12, "B": 12, "Q": 12, "R": 12, "D": 24}
    G = {}
    for name in COTANGENTS[constraints]:
        g = cot.get(name)
        if g is None:
            continue
        g = np.asarray(g, dtype=np.float64)
        if name in rows:
            g = np.swapaxes(g.reshape(B, g.shape[1], 12, rows[name]), -1, -2)  # math: [rows][12 columns]
        G[name] = g
    per = [_robot(sm, params[i], plan.robot(i) if plan_mode else None, plan_mode, xs[i], us[i],
                  constraints, {k: g[i] for k, g in G.items()}, qf_scale) for i in range(B)]
    return {k: np.array([r[k] for r in per], dtype=np.float64) for k in OUTPUTS}


def contraction(cot, plus, minus, constraints):
    """sum_X <cot[X], plus[X] - minus[X]> over COTANGENTS[constraints] (packed arrays of equal
    shapes): the difference is taken element by element first, so what does not move cancels exactly."""
    tot = 0.0
    for name in COTANGENTS[constraints]:
        g = cot.get(name)
        if g is None:
            continue
        d = np.asarray(plus[name], dtype=np.float64) - np.asarray(minus[name], dtype=np.float64)
        tot += float(np.sum(d.reshape(-1) * np.asarray(g, dtype=np.float64).reshape(-1)))
    return tot
