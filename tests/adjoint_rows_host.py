"""The backward pass with general rows on the inputs in numpy, one dense KKT
solve per QP with the active rows E_k u_k = e_k as equality rows.

Independent of the nullspace route, of Riccati and of the HIP path.  E_k holds a unit row for
every pinned input and row j of D_k for every active general row; the adjoint QP is the one of
adjoint_host with E_k du_k = 0 added, and its multipliers are dnu.  The forward multipliers nu
follow from stationarity (a least-squares solve of E' nu = -rho).  Arrays are in math orientation.
"""
import numpy as np

import adjoint_host

NAMES = adjoint_host.NAMES
ROW_NAMES = ("D", "lg", "ug", "lbu", "ubu")
ALL_NAMES = NAMES + ROW_NAMES


def _mask(m, i, shape):
    return np.ones(shape, dtype=bool) if m is None else np.asarray(m[i]) != 0


def active_rows(qp, u, act_tol, rank_tol, i=0):
    """The active set of QP i at u, by the rule the device uses.  Per stage a list of accepted
    rows (kind, index, upper, E row [nu], bound e), kind "pin" or "row"; and the counts
    (pinned, rows accepted, rows dropped) with the dropped rows as (k, j, upper)."""
    N, nu, ng = qp.N, qp.nu, qp.ng
    pins = adjoint_host.active_inputs(qp, u, act_tol, i)
    stages, dropped = [], []
    counts = [int(pins.sum()), 0, 0]
    for k in range(N):
        acc, basis = [], []
        for c in np.flatnonzero(pins[k]):  # pins first, ascending
            lo = (qp.lbu_mask is None or qp.lbu_mask[i][k, c] != 0) and u[k, c] - qp.lbu[i][k, c] < act_tol
            hi = (qp.ubu_mask is None or qp.ubu_mask[i][k, c] != 0) and qp.ubu[i][k, c] - u[k, c] < act_tol
            upper = not (lo and (not hi or u[k, c] - qp.lbu[i][k, c] <= qp.ubu[i][k, c] - u[k, c]))
            acc.append(("pin", int(c), upper, np.eye(nu)[c], (qp.ubu if upper else qp.lbu)[i][k, c]))
        if ng > 0 and qp.D is not None:
            free = ~pins[k]
            g = qp.D[i][k] @ u[k]
            lm, um = _mask(qp.lg_mask, i, (N + 1, ng))[k], _mask(qp.ug_mask, i, (N + 1, ng))[k]
            for j in range(ng):
                dl, dh = g[j] - qp.lg[i][k, j], qp.ug[i][k, j] - g[j]
                lo, hi = lm[j] and dl < act_tol, um[j] and dh < act_tol
                if not (lo or hi):
                    continue
                upper = not (lo and (not hi or dl <= dh))
                w = np.where(free, qp.D[i][k, j], 0.0)  # restricted to the unpinned coordinates
                own = np.linalg.norm(w)
                v = w.copy()
                for y in basis:  # modified Gram-Schmidt against the rows accepted so far
                    v = v - (y @ v) * y
                nv = np.linalg.norm(v)
                if nv > rank_tol * own and len(acc) < nu:
                    basis.append(v / nv)
                    acc.append(("row", j, upper, qp.D[i][k, j].copy(), (qp.ug if upper else qp.lg)[i][k, j]))
                    counts[1] += 1
                else:
                    dropped.append((k, j, upper))
                    counts[2] += 1
        stages.append(acc)
    return stages, tuple(counts), dropped


def _kkt_rows(qp, i, stages):
    """The KKT matrix of adjoint_host with the accepted rows appended: [[K, E'], [E, 0]]."""
    A, B, _, Q, S, R = (np.asarray(getattr(qp, n)[i], dtype=np.float64) for n in NAMES[:6])
    K, X, U, nv = adjoint_host._kkt(A, B, Q, S, R)
    rows = [(k, a) for k, acc in enumerate(stages) for a in acc]
    E = np.zeros((len(rows), K.shape[0]))
    for m, (k, a) in enumerate(rows):
        E[m, U(k)] = a[3]
    Kp = np.block([[K, E.T], [E, np.zeros((len(rows), len(rows)))]])
    return Kp, rows, K.shape[0], nv


def forward_rows_host(qp, x0, stages, i=0):
    """(x, u, pi) of QP i with the accepted rows held as equalities E u = e (bounds read from the
    QP's arrays, so that a perturbed D, lg, ug, lbu or ubu moves the solution)."""
    N, nx, nu = qp.N, qp.nx, qp.nu
    live = []
    for k, acc in enumerate(stages):
        cur = []
        for kind, idx, upper, _, _ in acc:
            if kind == "pin":
                cur.append((kind, idx, upper, np.eye(nu)[idx], (qp.ubu if upper else qp.lbu)[i][k, idx]))
            else:
                cur.append((kind, idx, upper, qp.D[i][k, idx], (qp.ug if upper else qp.lg)[i][k, idx]))
        live.append(cur)
    Kp, rows, nk, nv = _kkt_rows(qp, i, live)
    rhs = np.concatenate([-qp.q[i].ravel(), -qp.r[i].ravel(), -np.asarray(x0, dtype=np.float64), -qp.b[i].ravel(),
                          np.array([a[4] for _, a in rows])])
    z = np.linalg.solve(Kp, rhs)
    return (z[:(N + 1) * nx].reshape(N + 1, nx), z[(N + 1) * nx:nv].reshape(N, nu),
            z[nv:nk].reshape(N + 1, nx))


def adjoint_rows_host(qp, x, u, pi, gx, gu, i=0, act_tol=0.0, rank_tol=1e-8):
    """The fourteen gradients of l (dl/dx = gx, dl/du = gu) at the forward solution (x, u, pi) of
    QP i, and the counts (pinned, rows accepted, rows dropped)."""
    N, nx, nu, ng = qp.N, qp.nx, qp.nu, qp.ng
    stages, counts, _ = active_rows(qp, u, act_tol, rank_tol, i)
    Kp, rows, nk, nv = _kkt_rows(qp, i, stages)
    rhs = np.concatenate([-np.asarray(gx, dtype=np.float64).ravel(), -np.asarray(gu, dtype=np.float64).ravel(),
                          np.zeros(Kp.shape[0] - nv)])
    z = np.linalg.solve(Kp, rhs)
    dx, du = z[:(N + 1) * nx].reshape(N + 1, nx), z[(N + 1) * nx:nv].reshape(N, nu)
    dpi, dnu = z[nv:nk].reshape(N + 1, nx), z[nk:]
    out = adjoint_host.gradients(x, u, pi, dx, du, dpi)
    out["D"] = np.zeros((N, ng, nu))
    out["lg"], out["ug"] = np.zeros((N + 1, ng)), np.zeros((N + 1, ng))
    out["lbu"], out["ubu"] = np.zeros((N, nu)), np.zeros((N, nu))
    m = 0
    for k, acc in enumerate(stages):
        if not acc:
            continue
        # nu from stationarity: rho + E' nu = 0
        rho = qp.R[i][k] @ u[k] + qp.S[i][k] @ x[k] + qp.r[i][k] + qp.B[i][k].T @ pi[k + 1]
        Ek = np.array([a[3] for a in acc])
        nuk = -np.linalg.lstsq(Ek.T, rho, rcond=None)[0]
        for n, (kind, idx, upper, _, _) in enumerate(acc):
            if kind == "pin":
                out["ubu" if upper else "lbu"][k, idx] = -dnu[m]
            else:
                out["D"][k, idx] = dnu[m] * u[k] + nuk[n] * du[k]
                out["ug" if upper else "lg"][k, idx] = -dnu[m]
            m += 1
    return out, counts
