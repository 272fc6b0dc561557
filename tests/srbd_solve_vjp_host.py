"""TEST INFRASTRUCTURE ONLY -- the fused backward pass robots / plan <- solve in numpy (DESIGN.md
4.13d; the yardstick of srbd_qp_srbd_solve_backward_f64).

The chained statement forms the gradients of A, B, Q, R, D as outer products (adjoint_rows_host)
and contracts them again (linearize_vjp_host.linearize_vjp).  This one never forms a block: from
the vectors of the solve (x, u, pi), of its adjoint (dx, du, dpi) and the multipliers of the active
rows (nu, dnu) it builds, per stage, the 47 slots of the device's cotangent descriptor and the
cost's two vectors, and runs linearize_vjp_host's reverse model on those.

The adjoint is stated by the route the device takes, not by adjoint_rows_host's (one KKT system
with the active rows appended): the stages are projected on the null space of the active rows,
P = I - Y Y', the adjoint QP is an unconstrained solve on B P, P S, P R P + (I - P), P gu, and both
multipliers follow from stationarity.  Only the rule that says which rows are active
(adjoint_rows_host.active_rows) is shared.  Arrays are in math orientation unless said otherwise.
"""
from __future__ import annotations

import numpy as np

import adjoint_host
import adjoint_rows_host as arh
import linearize_vjp_host as VH

__all__ = ["OUTPUTS", "adjoint_vectors", "descriptor", "solve_vjp"]

OUTPUTS = VH.OUTPUTS
_FZ = (2, 8)  # fz of the right and of the left foot in u
# the descriptor's slots (csrc/srbd_lin_backward.h)
J00, J01, P0, P1, IM, RD, RP, D0, NSLOT = 0, 9, 18, 21, 24, 25, 37, 45, 47


def adjoint_vectors(qp, x, u, pi, gx, gu, i=0, act_tol=0.0, rank_tol=1e-8):
    """QP i at its forward solution: {dx [N+1][nx], du [N][nu], dpi [N+1][nx], nu, dnu [N][ng] (0 for
    an inactive or dropped row), glbu, gubu [N][nu] (-dnu of a pin, on its active side), counts}."""
    N, nx, nu, ng = qp.N, qp.nx, qp.nu, qp.ng
    A, B, _, Q, S, R = (np.asarray(getattr(qp, n)[i], dtype=np.float64) for n in arh.NAMES[:6])
    r = np.asarray(qp.r[i], dtype=np.float64)
    gx, gu = np.asarray(gx, dtype=np.float64), np.asarray(gu, dtype=np.float64)
    stages, counts, _ = arh.active_rows(qp, u, act_tol, rank_tol, i)
    Bm, Sm, Rm, rm = B.copy(), S.copy(), R.copy(), gu.copy()
    for k, acc in enumerate(stages):
        if not acc:
            continue
        Y = np.linalg.qr(np.array([a[3] for a in acc]).T)[0]  # an orthonormal basis of the rows' span
        P = np.eye(nu) - Y @ Y.T
        Bm[k], Sm[k], Rm[k], rm[k] = B[k] @ P, P @ S[k], P @ R[k] @ P + (np.eye(nu) - P), P @ gu[k]
    dx, du, dpi = adjoint_host._solve(A, Bm, np.zeros((N, nx)), Q, Sm, Rm, gx, rm, np.zeros(nx))
    out = dict(dx=dx, du=du, dpi=dpi, nu=np.zeros((N, ng)), dnu=np.zeros((N, ng)), glbu=np.zeros((N, nu)),
               gubu=np.zeros((N, nu)), counts=counts)
    for k, acc in enumerate(stages):
        if not acc:
            continue
        Et = np.array([a[3] for a in acc]).T
        rho = R[k] @ u[k] + S[k] @ x[k] + r[k] + B[k].T @ pi[k + 1]
        rhot = R[k] @ du[k] + S[k] @ dx[k] + gu[k] + B[k].T @ dpi[k + 1]
        nuk, dnuk = -np.linalg.lstsq(Et, rho, rcond=None)[0], -np.linalg.lstsq(Et, rhot, rcond=None)[0]
        for n, (kind, idx, upper, _, _) in enumerate(acc):
            if kind == "pin":
                out["gubu" if upper else "glbu"][k, idx] = -dnuk[n]
            else:
                out["nu"][k, idx], out["dnu"][k, idx] = nuk[n], dnuk[n]
    return out


def descriptor(x, u, pi, dx, du, dpi, nu=None, dnu=None):
    """[N][47]: the slots of one robot's stages from its vectors, each a sum of at most twelve
    products (the device's slot_of, csrc/srbd_solve_backward.hip)."""
    N = u.shape[0]
    pip, dpip = pi[1:], dpi[1:]
    GA = lambda i, j: pip[:, i] * dx[:N, j] + dpip[:, i] * x[:N, j]
    GB = lambda i, j: pip[:, i] * du[:, j] + dpip[:, i] * u[:, j]
    d = np.zeros((N, NSLOT))
    for e in range(9):
        d[:, J00 + e] = GA(e // 3, e % 3)
        d[:, J01 + e] = GA(e // 3, 3 + e % 3)
    for leg, (slot, cb) in enumerate(((P0, 0), (P1, 6))):
        for a in range(3):
            r1, c1 = (a + 1) % 3, (a + 2) % 3
            d[:, slot + a] = GB(3 + c1, cb + r1) - GB(3 + r1, cb + c1)
    d[:, IM] = sum(GB(9 + i, i) + GB(9 + i, 6 + i) for i in range(3))
    for i in range(12):
        d[:, RD + i] = du[:, i] * u[:, i]
    for leg in range(2):
        for pr, (lo, hi) in enumerate(((0, 2), (1, 2), (2, 4), (2, 5))):
            lo, hi = 6 * leg + lo, 6 * leg + hi
            d[:, RP + 4 * leg + pr] = du[:, lo] * u[:, hi] + u[:, lo] * du[:, hi]
        if nu is not None:
            rows = slice(12 * leg, 12 * leg + 4)
            d[:, D0 + leg] = (dnu[:, rows] * u[:, [_FZ[leg]]] + nu[:, rows] * du[:, [_FZ[leg]]]).sum(axis=1)
    return d


def _scatter(desc, constraints):
    """The descriptor as the cotangents linearize_vjp_host's reverse model reads: each slot at one
    element its sum stands for, every other element zero."""
    N = desc.shape[0]
    GA, GB, GR = np.zeros((N, 12, 12)), np.zeros((N, 12, 12)), np.zeros((N, 12, 12))
    for e in range(9):
        GA[:, e // 3, e % 3] = desc[:, J00 + e]
        GA[:, e // 3, 3 + e % 3] = desc[:, J01 + e]
    for slot, cb in ((P0, 0), (P1, 6)):
        for a in range(3):
            GB[:, 3 + (a + 2) % 3, cb + (a + 1) % 3] = desc[:, slot + a]  # where d skew(p) / d p_a is +1
    GB[:, 9, 0] = desc[:, IM]
    for i in range(12):
        GR[:, i, i] = desc[:, RD + i]
    for leg in range(2):
        for pr, (lo, hi) in enumerate(((0, 2), (1, 2), (2, 4), (2, 5))):
            GR[:, 6 * leg + lo, 6 * leg + hi] = desc[:, RP + 4 * leg + pr]
    G = {"A": GA, "B": GB, "R": GR}
    if constraints == "cone":
        GD = np.zeros((N, 24, 12))
        for leg in range(2):
            GD[:, 12 * leg, _FZ[leg]] = desc[:, D0 + leg]
        G["D"] = GD
    return G


def solve_vjp(sm, params, xs, us, constraints, vecs, plan=None, qf_scale=None):
    """The ten gradients {name: [B]...} and grad x0 [B][12] from the vectors.  vecs: per name a
    [B]... array -- x, pi, dx, dpi [B][N+1][12], u, du [B][N][12], and for the cone nu, dnu
    [B][N][24], for box_u gubu [B][N][12] (adjoint_vectors' per robot, stacked)."""
    B, N = us.shape[0], us.shape[1]
    plan_mode = plan is not None and any(getattr(plan, k) is not None for k in ("x_ref", "foot_r", "foot_l", "fz_max"))
    per = []
    for i in range(B):
        v = {k: np.asarray(a[i], dtype=np.float64) for k, a in vecs.items()}
        cone = constraints == "cone"
        desc = descriptor(v["x"], v["u"], v["pi"], v["dx"], v["du"], v["dpi"], v["nu"] if cone else None,
                          v["dnu"] if cone else None)
        G = _scatter(desc, constraints)
        GQ = np.zeros((N + 1, 12, 12))
        GQ[:, np.arange(12), np.arange(12)] = v["dx"] * v["x"]
        G.update(Q=GQ, q=v["dx"], r=v["du"], b=v["dpi"][1:])
        if cone:  # the cone's rows have no upper side: cot lg = -dnu
            G["lg"] = np.vstack([-v["dnu"], np.zeros((1, 24))])
        if constraints == "box_u":
            G["ubu"] = v["gubu"]
        per.append(VH._robot(sm, params[i], plan.robot(i) if plan_mode else None, plan_mode, xs[i], us[i], constraints,
                             G, qf_scale))
    out = {k: np.array([r[k] for r in per], dtype=np.float64) for k in OUTPUTS}
    out["x0"] = np.array([np.asarray(vecs["dpi"][i][0], dtype=np.float64) for i in range(B)])
    return out
