"""The backward pass through general rows on the GPU (srbd_qp_solve_backward_rows_f64,
diff.solve_qp with D, lg, ug) against the numpy statement of its math
(tests/adjoint_rows_host.py: one dense KKT solve per QP with the active rows as equality rows; no
nullspace projection, no Riccati recursion).

Tests 1 to 4 feed the numpy side the GPU's own forward solution, so they compare linear algebra
only: Eigen's isApprox at 1e-9 per QP and gradient array, as tests/test_gpu_backward.py does, and
the three counts exactly.  Test 8 goes end to end against the CPU oracle with a measured
allowance (10 d per array, d between the oracle at 1e-8 and at 1e-10).

Tightening the row bounds: helpers.random_constrained draws lg / ug 10 wide, which never binds,
so they are redrawn as -(0.05 + s |U|), +(0.05 + s |U|).  s (S_SCALE) and the SRBD test's state
perturbation (SRBD_SCALE) were chosen on the CPU with the oracle by one rule: the largest value
of a short ladder at which the batch keeps >= 75% of its QPs (a QP is kept iff no distance to an
unmasked bound lies in (1e-6, 1e-2), so that its active set is beyond doubt) and at least half of
those kept have an active row.  Counts seen with the oracle are in the docstrings of the tests.

Seen on an MI355X: worst relative error per QP and array 5.8e-13 ... 1.5e-12 in test 1 and 1.7e-14
in test 3, so 1e-9 holds as stated on all fourteen arrays, grad D included, and no wider allowance
was needed.  Test 8 finds d between 1.8e-8 and 2.8e-7 on A, B, Q, S, R, D (errors at most d) and
d = 0 on the other eight (errors below 2e-12).
"""
import ctypes as C

import numpy as np
import pytest

import adjoint_host
import adjoint_rows_host as arh
import helpers

pytestmark = pytest.mark.gpu

NAMES = adjoint_host.NAMES
ALL = arh.ALL_NAMES
MATRICES = ("A", "B", "Q", "S", "R", "D")
ROWS_ST = dict(iter_max=50, tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8, tol_comp=1e-8)
TIGHT_ST = dict(ROWS_ST, iter_max=100, tol_stat=1e-10, tol_eq=1e-10, tol_ineq=1e-10, tol_comp=1e-10)
ACT_TOL = 1e-4
RANK_TOL = 1e-8
POISON = 777.25
_cache = {}

# (batch, N, nx, nu, ng, has_box_u, seed): the aligned path; the generic path; pins and rows in
# one stage; ng = 64 with all but six rows per stage masked (the LDS sizing)
ROW_CASES = [(48, 3, 12, 12, 4, False, 5), (48, 4, 5, 3, 2, False, 7), (48, 3, 12, 12, 4, True, 11),
             (8, 2, 12, 12, 64, False, 13)]
S_SCALE = {case: 1.0 for case in ROW_CASES}  # of the ladder 0.1, 0.2, 0.3, 0.5, 1.0


def make_rows_batch(OcpQpBatch, case, s):
    batch, N, nx, nu, ng, box, seed = case
    qp, x0 = helpers.random_constrained(batch, N, nx, nu, ng, seed, OcpQpBatch)
    qp.C = None
    qp.lbx = qp.ubx = qp.lbx_mask = qp.ubx_mask = None
    if not box:
        qp.lbu = qp.ubu = qp.lbu_mask = qp.ubu_mask = None
    rng = np.random.default_rng(seed + 31)
    qp.lg = -(0.05 + s * np.abs(rng.uniform(-1, 1, (batch, N + 1, ng))))
    qp.ug = 0.05 + s * np.abs(rng.uniform(-1, 1, (batch, N + 1, ng)))
    if ng == 64:  # six live rows per stage
        mask = np.zeros((batch, N + 1, ng))
        for idx in np.ndindex(batch, N + 1):
            mask[idx][rng.choice(ng, 6, replace=False)] = 1.0
        qp.lg_mask, qp.ug_mask = mask, mask.copy()
    return qp, x0


def classify(qp, u):
    """(the QPs whose active set is beyond doubt, the number of active rows per QP)."""
    batch, N = qp.batch, qp.N
    dist = []
    g = np.einsum("bkgj,bkj->bkg", qp.D, u)
    lm = np.ones_like(g) if qp.lg_mask is None else qp.lg_mask[:, :N]
    um = np.ones_like(g) if qp.ug_mask is None else qp.ug_mask[:, :N]
    dl, dh = np.where(lm != 0, g - qp.lg[:, :N], np.inf), np.where(um != 0, qp.ug[:, :N] - g, np.inf)
    dist += [dl.reshape(batch, -1), dh.reshape(batch, -1)]
    if qp.lbu is not None:
        bl = np.ones_like(u) if qp.lbu_mask is None else qp.lbu_mask
        bu = np.ones_like(u) if qp.ubu_mask is None else qp.ubu_mask
        dist += [np.where(bl != 0, u - qp.lbu, np.inf).reshape(batch, -1),
                 np.where(bu != 0, qp.ubu - u, np.inf).reshape(batch, -1)]
    dist = np.concatenate(dist, axis=1)
    unclear = np.any((dist > 1e-6) & (dist < 1e-2), axis=1)
    active = ((dl < ACT_TOL) | (dh < ACT_TOL)).reshape(batch, -1).sum(axis=1)
    return np.flatnonzero(~unclear), active


def cotangents(qp, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (qp.batch, qp.N + 1, qp.nx)), rng.uniform(-1, 1, (qp.batch, qp.N, qp.nu))


def math_orientation(name, g):
    return np.swapaxes(g, -1, -2) if name in MATRICES else g


class Run:
    """One forward solve on the GPU and the device state a backward call needs."""

    def __init__(self, pkg, qp, x0, st=None, handle=None, tensors=None):
        import torch
        self.torch, self.capi, self.qp = torch, pkg.capi, qp
        self.h = handle or pkg.capi.Handle(qp.N, qp.nx, qp.nu, qp.ng, qp.has_box_u, qp.has_box_x, capacity=qp.batch)
        self.st = pkg.capi.settings_struct(st)
        self.dt, self.sol_t, self.data, self.sol = pkg.capi.device_buffers(qp, x0)
        if tensors is not None:  # data that is on the device already (the SRBD linearisation)
            self.dt = dict(tensors, x0=self.dt["x0"])
            self.data = pkg.capi.Data(**{k: pkg.capi._tensor_ptr(self.dt.get(k)) or None for k in pkg.capi.DATA_FIELDS})
        self.h.solve_device(qp.batch, self.st, self.data, self.sol)
        self.h.synchronize()
        self.fwd = {k: v.cpu().numpy() for k, v in self.sol_t.items()}

    def shapes(self):
        qp = self.qp
        return {**{n: tuple(self.dt[n].shape) for n in NAMES}, "D": (qp.batch, qp.N, qp.nu * qp.ng),
                "lg": (qp.batch, qp.N + 1, qp.ng), "ug": (qp.batch, qp.N + 1, qp.ng),
                "lbu": (qp.batch, qp.N, qp.nu), "ubu": (qp.batch, qp.N, qp.nu)}

    def backward(self, gx, gu, want=ALL, act_tol=ACT_TOL, rank_tol=RANK_TOL):
        """(dict name -> gradient in the C-ABI layout as numpy, every array poisoned first and only
        `want` passed; the counts [batch][3])."""
        torch, qp = self.torch, self.qp
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        g = {n: torch.full(s, POISON, dtype=torch.float64, device="cuda:0") for n, s in self.shapes().items()}
        nine, rows = [n for n in want if n in NAMES], [n for n in want if n in arh.ROW_NAMES]
        grad = self.capi.Grad(**{n: g[n].data_ptr() for n in nine}) if nine else None
        grows = self.capi.GradRows(**{n: g[n].data_ptr() for n in rows}) if rows else None
        self.gx_t, self.gu_t = dev(gx), dev(gu)
        self.h.solve_backward_rows_device(qp.batch, self.st, self.data, self.sol, self.gx_t, self.gu_t, grad, grows,
                                          act_tol=act_tol, rank_tol=rank_tol)
        counts = self.h.backward_active(qp.batch).cpu().numpy()
        self.h.synchronize()
        out = {n: t.cpu().numpy() for n, t in g.items()}
        # column-major blocks as row-major arrays (flat from the SRBD linearisation)
        blocks = {"A": (qp.nx, qp.nx), "B": (qp.nu, qp.nx), "Q": (qp.nx, qp.nx), "S": (qp.nx, qp.nu),
                  "R": (qp.nu, qp.nu), "D": (qp.nu, qp.ng)}
        for n, (cols, rows) in blocks.items():
            out[n] = out[n].reshape(qp.batch, qp.N + (n == "Q"), cols, rows)
        return out, counts


def reference(qp, fwd, gx, gu, i):
    return arh.adjoint_rows_host(qp, fwd["x"][i], fwd["u"][i], fwd["pi"][i], gx[i], gu[i], i, ACT_TOL, RANK_TOL)


def compare_qp(got, want, i, prec=1e-9, names=ALL, what=""):
    """isApprox per array.  An array that vanishes in the math (a stage with every input held has
    du = 0, and with every stage held dx = 0) is exactly zero on the device and rounding of the
    dense solve in the statement, which isApprox cannot compare: an array below 1e-12 of the QP's
    whole gradient on either side must be below `prec` of it on both."""
    worst = 0.0
    scale = np.sqrt(sum(np.linalg.norm(want[n]) ** 2 for n in ALL))
    for n in names:
        a, b = math_orientation(n, got[n][i]), want[n]
        if n in ("q", "Q"):  # stage 0 is exactly zero (dx_0 = 0): compared from stage 1 on
            assert np.all(a[0] == 0.0), (what, n, i)
            a, b = a[1:], b[1:]
        if n in arh.ROW_NAMES:  # what is zero in the statement is exactly zero on the device
            assert np.all(a[b == 0.0] == 0.0), (what, n, i)
        na, nb = np.linalg.norm(a), np.linalg.norm(b)
        if a.size == 0 or (na == 0.0 and nb == 0.0):
            continue
        if min(na, nb) < 1e-12 * scale:
            assert max(na, nb) < prec * scale, (what, n, i, na, nb, scale)
            continue
        rel = np.linalg.norm(a - b) / min(na, nb)
        worst = max(worst, rel)
        assert helpers.is_approx(a, b, prec), (what, n, i, rel)
    return worst


# ---------------------------------------------------------------------------
# 1. linear-algebra parity
# ---------------------------------------------------------------------------
def rows_run(pkg, OcpQpBatch, case):
    if case not in _cache:
        qp, x0 = make_rows_batch(OcpQpBatch, case, S_SCALE[case])
        gx, gu = cotangents(qp, case[-1] + 1)
        run = Run(pkg, qp, x0, ROWS_ST)
        got, counts = run.backward(gx, gu)
        run.h.close()
        kept, active = classify(qp, run.fwd["u"])
        _cache[case] = (qp, x0, gx, gu, run.fwd, got, counts, kept, active)
    return _cache[case]


@pytest.mark.parametrize("case", ROW_CASES)
def test_rows_parity(pkg, OcpQpBatch, case):
    """With the CPU oracle at S_SCALE the four batches keep 46, 44, 40, 7 of 48, 48, 48, 8 QPs, and
    45, 32, 39, 7 of those have an active row (152, 60, 128, 24 active rows in all, none dropped;
    34 pinned inputs in the third, 19 of whose kept QPs have a pin and a row in one stage).  The
    GPU's forward solve gives the same counts."""
    qp, x0, gx, gu, fwd, got, counts, kept, active = rows_run(pkg, OcpQpBatch, case)
    assert len(kept) >= 0.75 * qp.batch, len(kept)
    assert np.all(fwd["status"][kept] == 0), fwd["status"]
    assert np.sum(active[kept] > 0) >= 0.5 * len(kept), (np.sum(active[kept] > 0), len(kept))
    worst = 0.0
    for i in range(qp.batch):
        want, cnt = reference(qp, fwd, gx, gu, i)
        assert tuple(counts[i]) == cnt, (i, counts[i], cnt)
        if i in kept:
            worst = max(worst, compare_qp(got, want, i, what=case))
    print(f"[backward rows] {case}: kept {len(kept)} of {qp.batch}, {int(np.sum(active[kept] > 0))} with an active "
          f"row; pinned / accepted / dropped {counts[kept].sum(axis=0)}; worst relative error {worst:.2e}")
    if case[5]:  # pins and rows in one stage
        both = 0
        for i in kept:
            stages, _, _ = arh.active_rows(qp, fwd["u"][i], ACT_TOL, RANK_TOL, i)
            both += any({"pin", "row"} <= {a[0] for a in acc} for acc in stages)
        assert both > 0


# ---------------------------------------------------------------------------
# 2. ties to srbd_qp_solve_backward_f64, bit for bit
# ---------------------------------------------------------------------------
def old_backward(pkg, run, gx, gu, act_tol):
    import torch
    g = {n: torch.full_like(run.dt[n], POISON) for n in NAMES}
    grad = pkg.capi.Grad(**{n: g[n].data_ptr() for n in NAMES})
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    gx_t, gu_t = dev(gx), dev(gu)
    run.h.solve_backward_device(run.qp.batch, run.st, run.data, run.sol, gx_t, gu_t, grad, act_tol=act_tol)
    pins = run.h.backward_pinned(run.qp.batch).cpu().numpy() if run.qp.has_box_u else None
    run.h.synchronize()
    return {n: t.cpu().numpy() for n, t in g.items()}, pins


@pytest.mark.parametrize("nx,nu,ng", [(12, 12, 4), (5, 3, 2)])
def test_wide_rows_equal_the_entry_point_without_rows(pkg, OcpQpBatch, nx, nu, ng):
    """lg, ug so wide that nothing is active: the nine gradients are those of
    srbd_qp_solve_backward_f64 on an ng = 0 handle with the same data and the same forward
    solution, and grad D, lg, ug are exactly zero."""
    case = (6, 3, nx, nu, ng, False, 3)
    qp, x0 = make_rows_batch(OcpQpBatch, case, 0.3)
    qp.lg[:], qp.ug[:] = -1e6, 1e6
    gx, gu = cotangents(qp, 8)
    run = Run(pkg, qp, x0, ROWS_ST)
    got, counts = run.backward(gx, gu)
    assert not counts.any()
    for n in ("D", "lg", "ug", "lbu", "ubu"):
        assert not got[n].any(), n
    plain = OcpQpBatch(N=qp.N, nx=nx, nu=nu, **{n: getattr(qp, n) for n in NAMES[:8]})
    old = Run(pkg, plain, x0, ROWS_ST)
    for k in ("x", "u", "pi"):  # the rows run's forward solution, bit for bit
        old.sol_t[k].copy_(run.sol_t[k])
    want, _ = old_backward(pkg, old, gx, gu, ACT_TOL)
    for n in NAMES:
        assert np.array_equal(got[n], want[n]), n
    run.h.close()
    old.h.close()


@pytest.mark.parametrize("nx,nu", [(12, 12), (5, 3)])
def test_box_handle_equals_the_entry_point_without_rows(pkg, OcpQpBatch, nx, nu):
    """has_box_u, ng = 0: the nine equal the existing entry point's, the pinned count equals
    backward_pinned, and grad lbu / ubu match numpy at 1e-9."""
    qp, x0 = helpers.random_constrained(48, 3, nx, nu, 0, 5, OcpQpBatch)
    qp.lbx = qp.ubx = qp.lbx_mask = qp.ubx_mask = None
    gx, gu = cotangents(qp, 6)
    run = Run(pkg, qp, x0, ROWS_ST)
    got, counts = run.backward(gx, gu)
    want, pins = old_backward(pkg, run, gx, gu, ACT_TOL)
    for n in NAMES:
        assert np.array_equal(got[n], want[n]), n
    assert np.array_equal(counts[:, 0], pins) and not counts[:, 1:].any()
    assert pins.sum() > 0
    kept, _ = classify_boxes(qp, run.fwd["u"])
    for i in kept:
        ref, cnt = reference(qp, run.fwd, gx, gu, i)
        assert cnt == tuple(counts[i])
        compare_qp(got, ref, i, names=("lbu", "ubu"), what=(nx, nu))
    run.h.close()


def classify_boxes(qp, u):
    dist = np.concatenate([np.where(qp.lbu_mask != 0, u - qp.lbu, np.inf),
                           np.where(qp.ubu_mask != 0, qp.ubu - u, np.inf)], axis=-1).reshape(qp.batch, -1)
    return np.flatnonzero(~np.any((dist > 1e-6) & (dist < 1e-2), axis=1)), None


# ---------------------------------------------------------------------------
# 3. SRBD cone QPs from the device linearisation
# ---------------------------------------------------------------------------
SRBD_SCALE = 30.0  # of the ladder 1, 2, 3, 5, 10, 20, 30
# the NMPC's settings (tests/srbd_device.py) at test 1's tolerances, without regularisation
SRBD_ST = dict(mode="Speed", iter_max=100, alpha_min=1e-8, mu0=1e2, tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8,
               tol_comp=1e-8, reg_prim=0.0, warm_start=0, pred_corr=1, ric_alg=0, split_step=1)
SRBD_PAIRS = (10, 11, 22, 23)  # the rows that are active everywhere: an equality as two inequalities


def srbd_cone_batch(pkg, scale):
    """(xs, us, x0) of 16 robots, N = 3: sample_trajectories with the states' deviation from the
    reference scaled by `scale`, x0 likewise."""
    sm = pkg.srbd_model
    p = sm.SrbdParams()
    xs, us, x0 = sm.sample_trajectories(16, 3, 2024, p)
    xr = np.array(p.x_ref, dtype=np.float64)
    return xr + scale * (xs - xr), us, scale * x0


def qp_from_device(OcpQpBatch, t, N):
    """The linearisation's device tensors as an OcpQpBatch (math orientation)."""
    mat = lambda n, rows, cols: np.swapaxes(t[n].cpu().numpy().reshape(-1, t[n].shape[1], cols, rows), -1, -2)
    vec = lambda n: t[n].cpu().numpy()
    return OcpQpBatch(N=N, nx=12, nu=12, ng=24, A=mat("A", 12, 12), B=mat("B", 12, 12), b=vec("b"),
                      Q=mat("Q", 12, 12), S=mat("S", 12, 12), R=mat("R", 12, 12), q=vec("q"), r=vec("r"),
                      D=mat("D", 24, 12), lg=vec("lg"), ug=vec("ug"), lg_mask=vec("lg_mask"), ug_mask=vec("ug_mask"))


def test_srbd_cone_parity(pkg, OcpQpBatch):
    """Data from srbd_qp_srbd_linearize_f64 (CONE: ng = 24, twelve rows on each foot's six inputs,
    so active sets are rank deficient: a foot whose force goes to zero sits on all twelve).
    Solved with the NMPC's settings at test 1's tolerances, so that the active sets are beyond doubt (at the NMPC's 1e-4
    every QP with a friction row near its bound is unclear), and with reg_prim = 0: the numpy
    statement has no regularisation, and with the SRBD model's R = 1e-4 the NMPC's 1e-12 is a
    relative 1e-8 on R's diagonal (with it the worst relative error seen was 5.1e-9, on grad A).
    Rows 10 / 11 and 22 / 23 of every stage are two opposite rows with opposite bounds (an equality
    written as two inequalities): they are active in every QP, one of each pair accepted and its
    twin dropped.  Friction rows proper bind once the states are far enough from the reference:
    with the CPU oracle, along the ladder 1, 2, 3, 5, 10, 20, 30 the batch keeps 16, 16, 16, 14,
    16, 16, 15 of 16 QPs and 1, 2, 3, 3, 5, 8, 9 of those have such a row active; at 30 the kept
    QPs accept 278 rows and drop 218.
    ric_alg = 0 as in the NMPC: Q of the SRBD model is singular (one nonzero weight), and without
    regularisation the square-root recursion (ric_alg = 1) of the adjoint solve is off by 1e-3."""
    import torch

    import srbd_device
    xs, us, x0 = srbd_cone_batch(pkg, SRBD_SCALE)
    h = srbd_device.handle(pkg.capi, 3, 16, "cone")
    xs_t, us_t = torch.from_numpy(xs).cuda(), torch.from_numpy(us).cuda()
    t, _ = pkg.capi.srbd_linearize(h, xs_t, us_t, "cone")
    h.synchronize()
    qp = qp_from_device(OcpQpBatch, t, 3)
    run = Run(pkg, qp, x0, SRBD_ST, handle=h, tensors=t)
    gx, gu = cotangents(qp, 77)
    got, counts = run.backward(gx, gu)
    kept, active = classify(qp, run.fwd["u"])
    assert len(kept) >= 0.75 * qp.batch, len(kept)
    assert np.sum(active[kept] > 0) >= 0.5 * len(kept), (np.sum(active[kept] > 0), len(kept))
    assert np.all(run.fwd["status"][kept] == 0), run.fwd["status"]
    # friction rows proper: active in at least a third of the QPs kept (9 of 15 with the oracle)
    dist = np.einsum("bkgj,bkj->bkg", qp.D, run.fwd["u"]) - qp.lg[:, :3]
    proper = np.any(np.delete(dist, SRBD_PAIRS, axis=2).reshape(16, -1) < ACT_TOL, axis=1)
    assert np.sum(proper[kept]) >= len(kept) / 3, (np.sum(proper[kept]), len(kept))
    worst = 0.0
    for i in range(qp.batch):
        want, cnt = reference(qp, run.fwd, gx, gu, i)
        assert tuple(counts[i]) == cnt, (i, counts[i], cnt)
        if i in kept:
            worst = max(worst, compare_qp(got, want, i, what="srbd cone"))
    print(f"[backward rows] srbd cone: kept {len(kept)} of 16, {int(np.sum(proper[kept]))} with a friction row active, accepted / dropped {counts[kept, 1:].sum(axis=0)}; "
          f"worst relative error {worst:.2e}")
    assert np.any(counts[:, 2] > 0)
    h.close()


# ---------------------------------------------------------------------------
# 4. dependent rows on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu", [(12, 12), (5, 3)])
def test_duplicated_active_row_is_dropped(pkg, OcpQpBatch, nx, nu):
    case = (4, 3, nx, nu, 3, False, 17)
    qp, x0 = make_rows_batch(OcpQpBatch, case, 0.3)
    qp.lg[:], qp.ug[:] = -1e6, 1e6
    gx, gu = cotangents(qp, 2)
    free = Run(pkg, qp, x0, ROWS_ST)  # where row 0 of stage 1 sits without bounds
    g = np.einsum("bgj,bj->bg", qp.D[:, 1], free.fwd["u"][:, 1])
    free.h.close()
    qp.lg[:, 1, 0] = g[:, 0] + 0.1  # row 0 binds; row 2 is a copy of it
    qp.D[:, 1, 2], qp.lg[:, 1, 2] = qp.D[:, 1, 0], qp.lg[:, 1, 0]
    run = Run(pkg, qp, x0, ROWS_ST)
    assert np.all(run.fwd["status"] == 0)
    got, counts = run.backward(gx, gu)
    assert np.array_equal(counts, np.tile([0, 1, 1], (4, 1))), counts
    assert all(np.all(np.isfinite(v)) for v in got.values())
    D = math_orientation("D", got["D"])
    assert not D[:, 1, 2].any() and not got["lg"][:, 1, 2].any() and not got["ug"][:, 1, 2].any()
    assert np.all(got["lg"][:, 1, 0] != 0.0)
    for i in range(4):
        want, cnt = reference(qp, run.fwd, gx, gu, i)
        assert cnt == (0, 1, 1)
        compare_qp(got, want, i, what="duplicate")
    run.h.close()


# ---------------------------------------------------------------------------
# 5. outputs and cotangents
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ROW_CASES[2], (6, 4, 5, 3, 2, True, 7)])
def test_null_outputs_and_cotangents(pkg, OcpQpBatch, case):
    qp, x0 = make_rows_batch(OcpQpBatch, case, 0.3)
    gx, gu = cotangents(qp, 4)
    run = Run(pkg, qp, x0, ROWS_ST)
    before = {k: v.clone() for k, v in {**run.dt, **run.sol_t}.items() if v is not None}
    full, _ = run.backward(gx, gu)
    assert not any(np.any(full[n] == POISON) for n in ALL)
    for want in (("q", "D"), ("lg",), ("A", "ubu"), ("lbu", "ug")):
        part, _ = run.backward(gx, gu, want=want)
        for n in ALL:
            if n in want:
                assert np.array_equal(part[n], full[n]), n
            else:
                assert np.all(part[n] == POISON), n
    null, _ = run.backward(None, gu)
    zero, _ = run.backward(np.zeros_like(gx), gu)
    for n in ALL:
        assert np.array_equal(null[n], zero[n]), n
    for k, v in {**run.dt, **run.sol_t}.items():
        if v is not None:
            assert run.torch.equal(v, before[k]), k
    run.h.close()


# ---------------------------------------------------------------------------
# 6. checks on the device path
# ---------------------------------------------------------------------------
def test_device_checks(pkg, OcpQpBatch):
    import torch
    capi = pkg.capi
    L = capi.lib()
    st = capi.settings_struct()
    some = torch.full((4096,), POISON, dtype=torch.float64, device="cuda:0")
    grad, rows = capi.Grad(q=some.data_ptr()), capi.GradRows(lg=some.data_ptr())

    def call(h, batch, data, sol):
        return L.srbd_qp_solve_backward_rows_f64(h.ptr, batch, C.byref(st), C.byref(data), C.byref(sol),
                                                 C.c_void_p(some.data_ptr()), None, 0.0, 1e-8, C.byref(grad),
                                                 C.byref(rows), None)

    qp, x0 = make_rows_batch(OcpQpBatch, (2, 3, 12, 12, 4, False, 5), 0.3)
    run = Run(pkg, qp, x0, ROWS_ST)
    with_c = capi.Data.from_buffer_copy(run.data)
    with_c.C = some.data_ptr()
    assert call(run.h, 1, with_c, run.sol) == -2  # SRBD_QP_EDIM: rows on the states
    for kw in (dict(has_box_x=True), dict(layout=1)):
        h = capi.Handle(3, 12, 12, capacity=2, **kw)
        assert call(h, 1, capi.Data(), capi.Solution()) == -2, kw
        h.close()
    assert call(run.h, 3, run.data, run.sol) == -5  # SRBD_QP_ECAPACITY
    assert call(run.h, 0, run.data, run.sol) == 0
    no_d = capi.Data.from_buffer_copy(run.data)
    no_d.D = None
    assert call(run.h, 2, no_d, run.sol) == -1
    assert "D, lg and ug" in L.srbd_qp_last_error().decode()
    run.h.synchronize()
    assert bool((some == POISON).all())
    run.h.close()


# ---------------------------------------------------------------------------
# 7. autograd
# ---------------------------------------------------------------------------
def test_loss_backward_fills_row_gradients(pkg, OcpQpBatch):
    import torch
    case = ROW_CASES[2]
    qp, x0 = make_rows_batch(OcpQpBatch, case, S_SCALE[case])
    gx, gu = cotangents(qp, 17)
    p = qp.packed()
    p["x0"] = np.ascontiguousarray(x0)
    names = NAMES + ("lbu", "ubu", "lbu_mask", "ubu_mask", "D", "lg", "ug")
    t = {n: torch.from_numpy(p[n]).to("cuda:0") for n in names}
    t["D"] = t["D"].reshape(qp.batch, qp.N, qp.nu, qp.ng)
    for n in ("D", "lg", "lbu"):
        t[n].requires_grad_(True)
    h = pkg.capi.Handle(qp.N, qp.nx, qp.nu, qp.ng, True, capacity=qp.batch)
    x, u, pi = pkg.diff.solve_qp(h, *[t[n] for n in NAMES], lbu=t["lbu"], ubu=t["ubu"], lbu_mask=t["lbu_mask"],
                                 ubu_mask=t["ubu_mask"], settings=ROWS_ST, act_tol=ACT_TOL, D=t["D"], lg=t["lg"],
                                 ug=t["ug"], rank_tol=RANK_TOL)
    loss = (x * torch.from_numpy(gx).to(x.device)).sum() + (u * torch.from_numpy(gu).to(x.device)).sum()
    loss.backward()
    assert all(t[n].grad is None for n in names if n not in ("D", "lg", "lbu"))
    run = Run(pkg, qp, x0, ROWS_ST, handle=h)
    want, _ = run.backward(gx, gu, want=("D", "lg", "lbu"))
    for n in ("D", "lg", "lbu"):
        assert np.array_equal(t[n].grad.cpu().numpy(), want[n]), n
    assert t["D"].grad.abs().sum() > 0 and t["lg"].grad.abs().sum() > 0 and t["lbu"].grad.abs().sum() > 0
    h.close()


# ---------------------------------------------------------------------------
# 8. end to end against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ROW_CASES[:3])
def test_rows_against_oracle(pkg, OcpQpBatch, oracle, case):
    """GPU forward + backward against adjoint_rows_host on the oracle's solution at 1e-10.  d, per
    array, is adjoint_rows_host on the oracle at 1e-8 minus the same at 1e-10; 10 d is allowed.
    Arrays with d = 0 (they do not depend on the forward solution once the active set agrees) are
    held to test 1's precision."""
    qp, x0, gx, gu, fwd, got, counts, kept, _ = rows_run(pkg, OcpQpBatch, case)
    loose, fine = oracle.solve(qp, ROWS_ST, x0=x0, riccati=False), oracle.solve(qp, TIGHT_ST, x0=x0, riccati=False)
    assert np.all(loose["status"][kept] == 0) and np.all(fine["status"][kept] == 0)
    d = {n: 0.0 for n in ALL}
    err = {n: 0.0 for n in ALL}
    for i in kept:
        a, na = reference(qp, loose, gx, gu, i)
        b, nb = reference(qp, fine, gx, gu, i)
        assert na == nb == tuple(counts[i]), (i, na, nb, counts[i])
        for n in ALL:
            d[n] = max(d[n], float(np.max(np.abs(a[n] - b[n]), initial=0.0)))
            err[n] = max(err[n], float(np.max(np.abs(math_orientation(n, got[n][i]) - b[n]), initial=0.0)))
    for n in ALL:
        print(f"[backward rows oracle] {case} {n}: d {d[n]:.2e} err {err[n]:.2e}")
    for n in ALL:
        if d[n] > 0.0:
            assert err[n] <= 10 * d[n], (n, err[n], d[n])
        else:
            for i in kept:
                compare_qp(got, reference(qp, fine, gx, gu, i)[0], i, names=(n,), what=case)
