"""A QP with soft boxes written as a hard QP the CPU oracle solves as it stands.

Every (family, index) that is soft anywhere in the batch gets two extra inputs per stage,
its slacks: u' = [u; sl_0, su_0; sl_1, su_1; ...] with R' = blkdiag(R, Zl, Zu), r' = [r; zl;
zu], zero columns in B and S, a lower box lls / lus on the new inputs, and the bound itself
as two general rows,
    lb <= e_i'v + sl   (ug masked),      e_i'v - su <= ub   (lg masked).
Where the variable is not soft at a stage (or the side is masked) the slack input is free
with unit cost (so it is 0) and its row is masked.  The terminal stage has no inputs: when
x_N has a soft bound, one dummy stage is appended (A_N = B_N = 0, b_N = 0, Q_{N+1} = I,
R_N = blkdiag(I, Zl, Zu)), so stage N owns its slacks and x_{N+1} = 0 costs nothing.
"""
from __future__ import annotations

import numpy as np


def _mask(m, like, given):
    if not given:
        return np.zeros(like, dtype=bool)
    return np.ones(like, dtype=bool) if m is None else (np.asarray(m) != 0)


def _arr(v, shape):
    return np.zeros(shape) if v is None else np.asarray(v, dtype=np.float64)


def lift(qp, OcpQpBatch):
    """Returns (lifted OcpQpBatch, split): split(out) maps the lifted solve's output dict to
    {"x", "u", "sl_u", "su_u", "sl_x", "su_x", ...} in the soft problem's shapes."""
    assert qp.ng == 0, "the lift uses the general rows itself"
    nb, N, nx, nu = qp.batch, qp.N, qp.nx, qp.nu
    shu, shx = (nb, N, nu), (nb, N + 1, nx)
    soft_u = _mask(qp.soft_u, shu, qp.soft_u is not None)
    soft_x = _mask(qp.soft_x, shx, qp.soft_x is not None)
    soft_x[:, 0] = False  # stage-0 x bounds are dropped
    lmu, umu = _mask(qp.lbu_mask, shu, qp.has_box_u), _mask(qp.ubu_mask, shu, qp.has_box_u)
    lmx, umx = _mask(qp.lbx_mask, shx, qp.has_box_x), _mask(qp.ubx_mask, shx, qp.has_box_x)
    lbu, ubu = _arr(qp.lbu, shu), _arr(qp.ubu, shu)
    lbx, ubx = _arr(qp.lbx, shx), _arr(qp.ubx, shx)
    pen = {n: _arr(getattr(qp, n), shu if n.endswith("_u") else shx)
           for n in ("Zl_u", "Zu_u", "zl_u", "zu_u", "lls_u", "lus_u",
                     "Zl_x", "Zu_x", "zl_x", "zu_x", "lls_x", "lus_x")}
    slots = [("u", i) for i in range(nu) if soft_u[:, :, i].any()] + \
            [("x", i) for i in range(nx) if soft_x[:, :, i].any()]
    ns = len(slots)
    nu2, ng = nu + 2 * ns, 2 * ns
    assert nu2 <= 31, "nu + 2 (soft count) must stay within the oracle's 31 inputs"
    terminal = bool(soft_x[:, N].any())
    N2 = N + 1 if terminal else N

    A = np.zeros((nb, N2, nx, nx)); A[:, :N] = qp.A
    B = np.zeros((nb, N2, nx, nu2)); B[:, :N, :, :nu] = qp.B
    b = np.zeros((nb, N2, nx)); b[:, :N] = qp.b
    Q = np.zeros((nb, N2 + 1, nx, nx)); Q[:, :N + 1] = qp.Q
    q = np.zeros((nb, N2 + 1, nx)); q[:, :N + 1] = qp.q
    S = np.zeros((nb, N2, nu2, nx)); S[:, :N, :nu] = qp.S
    R = np.zeros((nb, N2, nu2, nu2)); R[:, :N, :nu, :nu] = qp.R
    r = np.zeros((nb, N2, nu2)); r[:, :N, :nu] = qp.r
    if terminal:
        Q[:, N + 1] = np.eye(nx)
        R[:, N, :nu, :nu] = np.eye(nu)
    lbu2 = np.zeros((nb, N2, nu2)); ubu2 = np.zeros((nb, N2, nu2))
    lmu2 = np.zeros((nb, N2, nu2)); umu2 = np.zeros((nb, N2, nu2))
    lbu2[:, :N, :nu] = lbu; ubu2[:, :N, :nu] = ubu
    lmu2[:, :N, :nu] = lmu & ~soft_u; umu2[:, :N, :nu] = umu & ~soft_u
    lbx2 = np.zeros((nb, N2 + 1, nx)); ubx2 = np.zeros((nb, N2 + 1, nx))
    lmx2 = np.zeros((nb, N2 + 1, nx)); umx2 = np.zeros((nb, N2 + 1, nx))
    lbx2[:, :N + 1] = lbx; ubx2[:, :N + 1] = ubx
    lmx2[:, :N + 1] = lmx & ~soft_x; umx2[:, :N + 1] = umx & ~soft_x
    C = np.zeros((nb, N2 + 1, ng, nx)); D = np.zeros((nb, N2, ng, nu2))
    lg = np.zeros((nb, N2 + 1, ng)); ug = np.zeros((nb, N2 + 1, ng))
    lgm = np.zeros((nb, N2 + 1, ng)); ugm = np.zeros((nb, N2 + 1, ng))
    for k in range(N2):
        for j, (fam, i) in enumerate(slots):
            if fam == "u":
                if k >= N:
                    on = np.zeros(nb, dtype=bool)
                    al = au = on
                else:
                    on = soft_u[:, k, i]
                    al, au = on & lmu[:, k, i], on & umu[:, k, i]
                lo, hi = (lbu[:, k, i], ubu[:, k, i]) if k < N else (0.0, 0.0)
                sfx = "_u"
            else:
                on = soft_x[:, k, i]
                al, au = on & lmx[:, k, i], on & umx[:, k, i]
                lo, hi = lbx[:, k, i], ubx[:, k, i]
                sfx = "_x"
            kk = min(k, N - 1) if fam == "u" else k
            Zl, Zu = pen["Zl" + sfx][:, kk, i], pen["Zu" + sfx][:, kk, i]
            zl, zu = pen["zl" + sfx][:, kk, i], pen["zu" + sfx][:, kk, i]
            ll, lu = pen["lls" + sfx][:, kk, i], pen["lus" + sfx][:, kk, i]
            cl, cu = nu + 2 * j, nu + 2 * j + 1  # the slot's slack inputs
            R[:, k, cl, cl] = np.where(al, Zl, 1.0)
            R[:, k, cu, cu] = np.where(au, Zu, 1.0)
            r[:, k, cl] = np.where(al, zl, 0.0)
            r[:, k, cu] = np.where(au, zu, 0.0)
            lbu2[:, k, cl] = np.where(al, ll, 0.0); lmu2[:, k, cl] = al
            lbu2[:, k, cu] = np.where(au, lu, 0.0); lmu2[:, k, cu] = au
            rl, ru = 2 * j, 2 * j + 1
            if fam == "u":
                D[:, k, rl, i] = 1.0
                D[:, k, ru, i] = 1.0
            else:
                C[:, k, rl, i] = 1.0
                C[:, k, ru, i] = 1.0
            D[:, k, rl, cl] = 1.0
            D[:, k, ru, cu] = -1.0
            lg[:, k, rl] = np.where(al, lo, 0.0); lgm[:, k, rl] = al
            ug[:, k, ru] = np.where(au, hi, 0.0); ugm[:, k, ru] = au
    out = OcpQpBatch(N=N2, nx=nx, nu=nu2, A=A, B=B, b=b, Q=Q, S=S, R=R, q=q, r=r,
                     lbu=lbu2, ubu=ubu2, lbu_mask=lmu2, ubu_mask=umu2,
                     lbx=lbx2, ubx=ubx2, lbx_mask=lmx2, ubx_mask=umx2,
                     ng=ng, C=C, D=D, lg=lg, ug=ug, lg_mask=lgm, ug_mask=ugm)

    def split(sol):
        res = {k: v for k, v in sol.items() if k in ("status", "iter", "res", "obj")}
        res["x"] = sol["x"][:, :N + 1]
        res["pi"] = sol["pi"][:, :N + 1]
        res["u"] = sol["u"][:, :N, :nu]
        res["sl_u"] = np.zeros(shu); res["su_u"] = np.zeros(shu)
        res["sl_x"] = np.zeros(shx); res["su_x"] = np.zeros(shx)
        for j, (fam, i) in enumerate(slots):
            cl, cu = nu + 2 * j, nu + 2 * j + 1
            if fam == "u":
                res["sl_u"][:, :, i] = sol["u"][:, :N, cl]
                res["su_u"][:, :, i] = sol["u"][:, :N, cu]
            else:
                res["sl_x"][:, :N2, i] = sol["u"][:, :N2, cl]
                res["su_x"][:, :N2, i] = sol["u"][:, :N2, cu]
        return res

    return out, split


def tighten(qp, idx=(1, 3), width=0.02, first=1):
    """The x-box on `idx` tightened to +-width at stages first..N (in place): with
    random_constrained's data most of these QPs are infeasible as hard constraints."""
    for i in idx:
        if i < qp.nx:
            qp.lbx[:, first:, i] = -width
            qp.ubx[:, first:, i] = width
    return qp


def soften_x(qp, idx, z, Z, stages=None):
    """Mark the x-box on `idx` soft at `stages` (default 1..N) with penalties z, Z (in place)."""
    nb, N, nx = qp.batch, qp.N, qp.nx
    stages = range(1, N + 1) if stages is None else stages
    qp.soft_x = np.zeros((nb, N + 1, nx))
    for k in stages:
        for i in idx:
            qp.soft_x[:, k, i] = 1.0
    for name, v in (("Zl_x", Z), ("Zu_x", Z), ("zl_x", z), ("zu_x", z)):
        setattr(qp, name, np.full((nb, N + 1, nx), float(v)))
    return qp
