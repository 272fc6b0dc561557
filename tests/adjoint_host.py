"""The backward pass of the OCP-QP in numpy, one dense KKT solve per QP.

Independent of the Riccati recursion and of the HIP path: the KKT matrix of the whole horizon is
assembled with x_0 as a variable, so that pi_0 (the multiplier of x0 - x_0 = 0) is a row of it.
Arrays are in math orientation (A[k][i][j] = row i, column j), like OcpQpBatch.
"""
import numpy as np

NAMES = ("A", "B", "b", "Q", "S", "R", "q", "r", "x0")


def active_inputs(qp, u, act_tol, i=0):
    """[N][nu] bool: input (k, j) of QP i is active at u (the forward solution) iff its bound is
    unmasked and u - lbu < act_tol or ubu - u < act_tol."""
    if qp.lbu is None:
        return np.zeros((qp.N, qp.nu), dtype=bool)
    lm = np.ones((qp.N, qp.nu), dtype=bool) if qp.lbu_mask is None else qp.lbu_mask[i] != 0
    um = np.ones((qp.N, qp.nu), dtype=bool) if qp.ubu_mask is None else qp.ubu_mask[i] != 0
    return (lm & (u - qp.lbu[i] < act_tol)) | (um & (qp.ubu[i] - u < act_tol))


def _kkt(A, B, Q, S, R):
    """K = [[H, G'], [G, 0]] over v = (x_0..x_N, u_0..u_{N-1}) and the rows x0 - x_0 = 0 (pi_0),
    A x_k + B u_k + b_k - x_{k+1} = 0 (pi_{k+1}); also the index helpers."""
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    nv, ne = (N + 1) * nx + N * nu, (N + 1) * nx
    X = lambda k: slice(k * nx, (k + 1) * nx)
    U = lambda k: slice((N + 1) * nx + k * nu, (N + 1) * nx + (k + 1) * nu)
    K = np.zeros((nv + ne, nv + ne))
    for k in range(N + 1):
        K[X(k), X(k)] = Q[k]
    for k in range(N):
        K[U(k), U(k)] = R[k]
        K[U(k), X(k)] = S[k]
        K[X(k), U(k)] = S[k].T
    G = np.zeros((ne, nv))
    G[X(0), X(0)] = -np.eye(nx)
    for k in range(N):
        G[X(k + 1), X(k)] = A[k]
        G[X(k + 1), U(k)] = B[k]
        G[X(k + 1), X(k + 1)] = -np.eye(nx)
    K[nv:, :nv] = G
    K[:nv, nv:] = G.T
    return K, X, U, nv


def _solve(A, B, b, Q, S, R, q, r, x0):
    """(x, u, pi) of the equality-constrained QP: K [v; pi] = [-g; h]."""
    N, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    K, X, U, nv = _kkt(A, B, Q, S, R)
    rhs = np.concatenate([-q.ravel(), -r.ravel(), -x0, -b.ravel()])
    z = np.linalg.solve(K, rhs)
    return z[:(N + 1) * nx].reshape(N + 1, nx), z[(N + 1) * nx:nv].reshape(N, nu), z[nv:].reshape(N + 1, nx)


def _pin(B, S, R, r, pinned):
    """The masked copy of the stages: a pinned input gets a zero column of B, a zero row of S, a
    zero row and column of R with 1 on the diagonal, and r = 0, so that its step is 0."""
    B, S, R, r = B.copy(), S.copy(), R.copy(), r.copy()
    for k, j in zip(*np.nonzero(pinned)):
        B[k][:, j] = 0.0
        S[k][j, :] = 0.0
        R[k][j, :] = 0.0
        R[k][:, j] = 0.0
        R[k][j, j] = 1.0
        r[k][j] = 0.0
    return B, S, R, r


def forward_host(qp, x0, i=0, pinned=None, u_pin=None):
    """(x, u, pi) of QP i by the dense KKT system; with `pinned` ([N][nu] bool) those inputs are
    held at u_pin (the active-set-fixed problem: the pin is one more equality row)."""
    A, B, b, Q, S, R, q, r = (np.asarray(getattr(qp, n)[i], dtype=np.float64) for n in NAMES[:8])
    if pinned is None or not pinned.any():
        return _solve(A, B, b, Q, S, R, q, r, np.asarray(x0, dtype=np.float64))
    N, nx, nu = qp.N, qp.nx, qp.nu
    K, X, U, nv = _kkt(A, B, Q, S, R)
    idx = [(N + 1) * nx + k * nu + j for k, j in zip(*np.nonzero(pinned))]
    E = np.zeros((len(idx), K.shape[0]))
    E[np.arange(len(idx)), idx] = 1.0
    Kp = np.block([[K, E.T], [E, np.zeros((len(idx), len(idx)))]])
    rhs = np.concatenate([-q.ravel(), -r.ravel(), -np.asarray(x0, dtype=np.float64), -b.ravel(), u_pin[pinned]])
    z = np.linalg.solve(Kp, rhs)
    return z[:(N + 1) * nx].reshape(N + 1, nx), z[(N + 1) * nx:nv].reshape(N, nu), z[nv:nv + (N + 1) * nx].reshape(N + 1, nx)


def adjoint_qp(qp, gx, gu, i=0, pinned=None):
    """(dx, du, dpi): the solution of the adjoint QP of QP i -- the same A, B, Q, S, R with
    q := gx, r := gu, b := 0, x0 := 0, on the masked stages where `pinned` says so."""
    A, B, _, Q, S, R = (np.asarray(getattr(qp, n)[i], dtype=np.float64) for n in NAMES[:6])
    r = np.array(gu, dtype=np.float64)
    if pinned is not None and pinned.any():
        B, S, R, r = _pin(B, S, R, r, pinned)
    return _solve(A, B, np.zeros((qp.N, qp.nx)), Q, S, R, np.asarray(gx, dtype=np.float64), r, np.zeros(qp.nx))


def gradients(x, u, pi, dx, du, dpi):
    """The nine gradients from the forward solution and the adjoint QP's."""
    sym = lambda a, b: 0.5 * (np.einsum("ki,kj->kij", a, b) + np.einsum("ki,kj->kij", b, a))
    out = lambda a, b: np.einsum("ki,kj->kij", a, b)
    return {
        "q": dx.copy(), "r": du.copy(), "b": dpi[1:].copy(), "x0": dpi[0].copy(),
        "Q": sym(dx, x), "R": sym(du, u),
        "S": out(du, x[:-1]) + out(u, dx[:-1]),
        "A": out(pi[1:], dx[:-1]) + out(dpi[1:], x[:-1]),
        "B": out(pi[1:], du) + out(dpi[1:], u),
    }


def adjoint_host(qp, x, u, pi, gx, gu, i=0, act_tol=None):
    """Gradients of l with dl/dx = gx, dl/du = gu with respect to the nine inputs of QP i, at its
    forward solution (x, u, pi).  With input boxes (act_tol given and qp.lbu set) the active
    inputs are pinned.  Returns (dict of gradients, number of pinned inputs)."""
    pinned = None if act_tol is None else active_inputs(qp, u, act_tol, i)
    dx, du, dpi = adjoint_qp(qp, gx, gu, i, pinned)
    return gradients(x, u, pi, dx, du, dpi), 0 if pinned is None else int(pinned.sum())
