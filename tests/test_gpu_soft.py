"""Soft box constraints on the GPU (srbd_qp_solve_soft_f64) against the CPU oracle.

The oracle has no soft constraints; it solves the same problem with the slacks written as
extra inputs (tests/soft_lift.py).  The GPU eliminates the slacks, the oracle carries them:
two paths to one optimum, each stopped at its tolerances.  The comparison tolerance is
therefore measured, not assumed: d = the distance between the lifted oracle at the test's
tolerances and the lifted oracle at tol 1e-10 (iter_max 100), on the test's own inputs, and
the test allows 10 d per quantity (2 from the triangle inequality, 5 for the other path).

Where some QP of a family stalls above 1e-10 in the oracle, the family's tight solve is at
1e-9 (tight_tol below).  The test computes d itself; the values it finds (x / u / slacks /
obj, both ric_alg values alike):
  1  nx 4 nu 2   (1, 1)        tight 1e-9   1.3e-7 / 1.7e-7 / 1.3e-7 / 1.8e-9
                 (100, 1e-2)                2.1e-7 / 1.8e-7 / 1.4e-10 / 2.4e-8
                 (1e3, 1e-4)                1.0e-7 / 8.9e-8 / 3.2e-11 / 4.2e-8
  2  nx 12 nu 4  (1, 1)        tight 1e-10  1.0e-7 / 1.3e-7 / 5.9e-8 / 4.9e-8
                 (100, 1e-2)                2.4e-7 / 2.7e-7 / 6.6e-10 / 2.8e-8
                 (1e3, 1e-4)                1.7e-8 / 1.9e-8 / 2.4e-11 / 3.1e-8
  2b nx = nu = 12 (10, 0.1)    tight 1e-10  1.7e-7 / 2.1e-7 / 4.8e-9 / 3.1e-8
  3  terminal, N = 1           tight 1e-9   9.0e-8 / 7.5e-8 / 6.1e-8 / 1.0e-8
               N = 2                        7.3e-7 / 1.1e-6 / 1.1e-6 / 1.9e-8
               N = 5                        7.5e-8 / 5.4e-8 / 5.0e-8 / 6.6e-8
  4  one-sided / mixed         tight 1e-9   5.1e-7 / 6.0e-7 / 5.1e-7 / 8.5e-9
  5  exact penalty (1e4, 0)    tight 1e-10  4.2e-7 / 6.2e-7 / 4.7e-15 / 9.3e-9 (hard oracle: 2.8e-7 / 5.8e-7)
  7  compaction sample         tight 1e-9   8.1e-7 / 3.7e-7 / 9.2e-9 / 4.4e-8
"""
import numpy as np
import pytest

import helpers
import soft_lift

pytestmark = pytest.mark.gpu

ST = dict(iter_max=50)
SLACKS = ("sl_u", "su_u", "sl_x", "su_x")
_cache = {}


def _tight(st, tol=1e-10):
    return dict(st, iter_max=100, tol_stat=tol, tol_eq=tol, tol_ineq=tol, tol_comp=tol)


def _dist(a, b):
    d = {k: float(np.max(np.abs(a[k] - b[k]))) for k in ("x", "u", "obj")}
    d["s"] = max(float(np.max(np.abs(a[k] - b[k]))) for k in SLACKS)
    return d


def reference(key, qp, x0, st, OcpQpBatch, oracle, tight_tol=1e-10):
    """The lifted oracle's solution at the test's settings and the measured d (cached by key)."""
    if key not in _cache:
        lifted, split = soft_lift.lift(qp, OcpQpBatch)
        a = split(oracle.solve(lifted, st, x0=x0, riccati=False))
        b = split(oracle.solve(lifted, _tight(st, tight_tol), x0=x0, riccati=False))
        assert np.all(a["status"] == 0), a["status"]
        assert np.all(b["status"] == 0), (tight_tol, b["status"])
        d = _dist(a, b)
        print(f"[soft d] {key} (tight {tight_tol:g}): x {d['x']:.2e} u {d['u']:.2e} slacks {d['s']:.2e} obj {d['obj']:.2e} "
              f"iters {a['iter'].min()}-{a['iter'].max()}")
        _cache[key] = (a, d)
    return _cache[key]


def compare(out, ref, d, what=""):
    for k in ("x", "u"):
        err = float(np.max(np.abs(out[k] - ref[k])))
        print(f"[soft err] {what} {k}: {err:.2e} (10 d = {10 * d[k]:.2e})")
    for k in SLACKS:
        err = float(np.max(np.abs(out[k] - ref[k])))
        print(f"[soft err] {what} {k}: {err:.2e} (10 d = {10 * d['s']:.2e})")
    print(f"[soft err] {what} obj: {float(np.max(np.abs(out['obj'] - ref['obj']))):.2e} (10 d = {10 * d['obj']:.2e})")
    for k in ("x", "u"):
        assert np.max(np.abs(out[k] - ref[k])) <= 10 * d[k], (what, k)
    for k in SLACKS:
        assert np.max(np.abs(out[k] - ref[k])) <= 10 * d["s"], (what, k)
    assert np.max(np.abs(out["obj"] - ref["obj"])) <= 10 * d["obj"], (what, "obj")


def check_solution(out, ref, x0, st, window=3):
    assert np.all(out["status"] == 0), out["status"]
    tol = np.array([st.get(k, 1e-8) for k in ("tol_stat", "tol_eq", "tol_ineq", "tol_comp")])
    assert np.all(out["res"] <= tol), out["res"].max(axis=0)
    assert np.array_equal(out["x"][:, 0], x0)
    assert np.all(np.abs(out["iter"].astype(int) - ref["iter"].astype(int)) <= window), (out["iter"], ref["iter"])


def family(OcpQpBatch, nx=4, nu=2, N=5, batch=16, seed=3, idx=(1, 3), stages=None, z=1.0, Z=1.0,
           x0_scale=1.0, width=0.02):
    """random_constrained with the x-box on idx at +-width on `stages` (default 1..N-1: the
    terminal box keeps its wide hard bound), soft there with penalties z, Z."""
    qp, x0 = helpers.random_constrained(batch, N, nx, nu, 0, seed, OcpQpBatch, x0_scale=x0_scale)
    stages = list(range(1, N)) if stages is None else list(stages)
    for k in stages:
        for i in idx:
            qp.lbx[:, k, i], qp.ubx[:, k, i] = -width, width
            qp.lbx_mask[:, k, i] = qp.ubx_mask[:, k, i] = 1.0
    soft_lift.soften_x(qp, idx, z, Z, stages=stages)
    return qp, x0


PAIRS = [(1.0, 1.0), (100.0, 1e-2), (1e3, 1e-4)]


@pytest.mark.parametrize("ric_alg", [0, 1])
@pytest.mark.parametrize("z,Z", PAIRS)
def test_lifted_parity_embedded(pkg, OcpQpBatch, oracle, z, Z, ric_alg):
    """1. nx = 4, nu = 2 (the 12 x 12 embedding carries the soft arrays), soft x on {1, 3}
    at stages 1..N-1."""
    qp, x0 = family(OcpQpBatch, z=z, Z=Z)
    st = dict(ST, ric_alg=ric_alg)
    ref, d = reference(("emb", z, Z, ric_alg), qp, x0, st, OcpQpBatch, oracle, tight_tol=1e-9)
    out = pkg.capi.solve(qp, x0, st)
    check_solution(out, ref, x0, st)
    compare(out, ref, d, f"emb z={z} Z={Z} ric={ric_alg}")


@pytest.mark.parametrize("ric_alg", [0, 1])
@pytest.mark.parametrize("z,Z", PAIRS)
def test_lifted_parity_fast_path(pkg, OcpQpBatch, oracle, z, Z, ric_alg):
    """2. nx = 12, nu = 4, soft on 4 states (box +-0.5: with +-0.02 on four states the oracle
    itself stalls above 1e-9 on some QP for every seed tried, so no d could be measured)."""
    qp, x0 = family(OcpQpBatch, nx=12, nu=4, idx=(1, 3, 5, 7), z=z, Z=Z, seed=4, width=0.5)
    st = dict(ST, ric_alg=ric_alg)
    ref, d = reference(("fast", z, Z, ric_alg), qp, x0, st, OcpQpBatch, oracle)
    out = pkg.capi.solve(qp, x0, st)
    check_solution(out, ref, x0, st)
    compare(out, ref, d, f"fast z={z} Z={Z} ric={ric_alg}")


@pytest.mark.parametrize("ric_alg", [0, 1])
def test_lifted_parity_12x12(pkg, OcpQpBatch, oracle, ric_alg):
    """2b. nx = nu = 12: no embedding at all (the oracle takes the lift's 20 inputs)."""
    qp, x0 = family(OcpQpBatch, nx=12, nu=12, idx=(1, 3, 5, 7), z=10.0, Z=0.1, seed=2)
    st = dict(ST, ric_alg=ric_alg)
    ref, d = reference(("full", ric_alg), qp, x0, st, OcpQpBatch, oracle)
    out = pkg.capi.solve(qp, x0, st)
    check_solution(out, ref, x0, st)
    compare(out, ref, d, f"12x12 ric={ric_alg}")


@pytest.mark.parametrize("N", [1, 2, 5])
def test_terminal_stage_and_soft_u(pkg, OcpQpBatch, oracle, N):
    """3. Soft bounds at stage N too (the lift's dummy stage) and one soft input bound."""
    qp, x0 = family(OcpQpBatch, N=N, stages=range(1, N + 1), z=10.0, Z=0.5)
    nb, nu = qp.batch, qp.nu
    qp.lbu[:, :, 0], qp.ubu[:, :, 0] = -0.01, 0.01
    qp.soft_u = np.zeros((nb, N, nu)); qp.soft_u[:, :, 0] = 1.0
    qp.Zl_u = np.full((nb, N, nu), 2.0); qp.Zu_u = np.full((nb, N, nu), 3.0)
    qp.zl_u = np.full((nb, N, nu), 0.5); qp.zu_u = np.full((nb, N, nu), 0.25)
    ref, d = reference(("term", N), qp, x0, ST, OcpQpBatch, oracle, tight_tol=1e-9)
    out = pkg.capi.solve(qp, x0, ST)
    check_solution(out, ref, x0, ST)
    compare(out, ref, d, f"terminal N={N}")
    assert np.max(out["sl_u"] + out["su_u"]) > 1e-3  # the soft input bound is in use
    if N <= 2:  # (at N = 5 the terminal box is met without its slack)
        assert np.max(out["sl_x"][:, N] + out["su_x"][:, N]) > 1e-3  # and the terminal one


def test_one_sided_and_mixed(pkg, OcpQpBatch, oracle):
    """4. x_1 soft with only its lower side (raised to 0.3, so it is violated), x_3 a hard
    box, the other states unbounded; slack bounds lls = -0.05 on x_1."""
    qp, x0 = helpers.random_constrained(16, 5, 4, 2, 0, 5, OcpQpBatch)
    qp.lbx[:, 1:, 1] = 0.3
    qp.ubx_mask[:, :, 1] = 0.0
    soft_lift.soften_x(qp, (1,), 5.0, 1.0)
    qp.lls_x = np.full(qp.soft_x.shape, -0.05)
    ref, d = reference(("mixed",), qp, x0, ST, OcpQpBatch, oracle, tight_tol=1e-9)
    out = pkg.capi.solve(qp, x0, ST)
    check_solution(out, ref, x0, ST)
    compare(out, ref, d, "mixed")
    assert np.all(out["su_x"] == 0.0)  # masked side: exactly 0
    assert np.all(out["sl_x"][:, :, [0, 2, 3]] == 0.0) and np.all(out["sl_x"][:, 0] == 0.0)
    assert np.all(out["sl_u"] == 0.0) and np.all(out["su_u"] == 0.0)
    assert np.max(out["sl_x"]) > 1e-2 and np.all(out["sl_x"][:, 1:, 1] >= -0.05)
    # the hard box on x_3 holds
    assert np.all(out["x"][:, 1:, 3] >= qp.lbx[:, 1:, 3] - 1e-9) and np.all(out["x"][:, 1:, 3] <= qp.ubx[:, 1:, 3] + 1e-9)


def test_exact_penalty(pkg, OcpQpBatch, oracle):
    """5. Hard-feasible boxes with z = 1e4, Z = 0: an exact penalty, so the optimum is the
    hard QP's with zero slacks.  Tolerance for x, u: 10 x the larger of the two references'
    own errors (the lifted oracle's d and the hard oracle's); for the slacks 10 d of the
    lifted oracle (d = 4.7e-15: both paths run 13-19 iterations here and leave the inactive
    slacks at mu / z; measured on the GPU: 4.7e-15)."""
    qp, x0 = helpers.random_constrained(16, 5, 4, 2, 0, 3, OcpQpBatch)
    hard = oracle.solve(qp, ST, x0=x0, riccati=False)
    hard_t = oracle.solve(qp, _tight(ST), x0=x0, riccati=False)
    assert np.all(hard["status"] == 0) and np.all(hard_t["status"] == 0)
    soft_lift.soften_x(qp, (1, 3), 1e4, 0.0)
    ref, d = reference(("exact",), qp, x0, ST, OcpQpBatch, oracle)
    out = pkg.capi.solve(qp, x0, ST)
    assert np.all(out["status"] == 0), out["status"]
    tol = {k: 10 * max(d[k], float(np.max(np.abs(hard[k] - hard_t[k])))) for k in ("x", "u")}
    for k in ("x", "u"):
        err = float(np.max(np.abs(out[k] - hard[k])))
        print(f"[soft err] exact {k} vs hard: {err:.2e} (tol {tol[k]:.2e})")
    stol = 10 * d["s"]
    for k in SLACKS:
        print(f"[soft err] exact {k}: {float(np.max(np.abs(out[k]))):.2e} (tol {stol:.2e})")
    for k in ("x", "u"):
        assert np.max(np.abs(out[k] - hard[k])) <= tol[k], k
    for k in SLACKS:
        assert np.max(np.abs(out[k])) <= stol, k


def test_no_soft_variable_matches_hard_solve(pkg, OcpQpBatch, monkeypatch):
    """6. Every soft mask 0 through srbd_qp_solve_soft_f64 against srbd_qp_solve_f64 on the
    batched kernels: one algorithm in two arrangements."""
    monkeypatch.setenv("SRBD_IPM_LATENCY_MAX", "0")
    for nx, nu in ((12, 12), (4, 2)):
        for ric_alg in (0, 1):
            qp, x0 = helpers.random_constrained(16, 5, nx, nu, 0, 11, OcpQpBatch)
            st = dict(ST, ric_alg=ric_alg)
            hard = pkg.capi.solve(qp, x0, st)
            qp.soft_x = np.zeros((16, 6, nx)); qp.soft_u = np.zeros((16, 5, nu))
            soft = pkg.capi.solve(qp, x0, st)
            assert np.array_equal(soft["status"], hard["status"]) and np.all(hard["status"] == 0)
            assert np.array_equal(soft["iter"], hard["iter"])
            for k in ("x", "u", "pi"):
                assert np.max(np.abs(soft[k] - hard[k])) <= 1e-10, (nx, ric_alg, k)
            for k in SLACKS:
                assert np.all(soft[k] == 0.0)


def test_compaction(pkg, OcpQpBatch, oracle):
    """7. 2048 QPs (128 workgroups: the smallest grids that compact have 64), x0 scaled per
    QP so the iteration counts differ and the live list thins out."""
    nb = 2048
    scale = np.linspace(0.05, 3.0, nb)[:, None]
    qp, x0 = family(OcpQpBatch, nx=12, nu=12, batch=nb, seed=21, z=10.0, Z=0.1, x0_scale=scale)
    out = pkg.capi.solve(qp, x0, ST)
    assert np.all(out["status"] == 0), np.unique(out["status"], return_counts=True)
    assert out["iter"].max() - out["iter"].min() >= 3, (out["iter"].min(), out["iter"].max())
    idx = np.arange(7, nb, 64)
    assert idx.size == 32
    ref, d = reference(("compact",), qp.subset(idx), x0[idx], ST, OcpQpBatch, oracle, tight_tol=1e-9)
    sub = {k: v[idx] for k, v in out.items()}
    check_solution(sub, ref, x0[idx], ST)
    compare(sub, ref, d, "compaction")
    perm = np.random.default_rng(0).permutation(nb)
    outp = pkg.capi.solve(qp.subset(perm), x0[perm], ST)
    for k in ("x", "u", "pi", "status", "iter", "obj") + SLACKS:
        assert np.array_equal(outp[k], out[k][perm]), k


def test_nan_isolation(pkg, OcpQpBatch):
    """8. A NaN in one QP's Zl_x ends that QP with status 3 and leaves the others alone."""
    qp, x0 = family(OcpQpBatch, nx=12, nu=12, batch=8, seed=4)
    good = pkg.capi.solve(qp, x0, ST)
    assert np.all(good["status"] == 0)
    qp.Zl_x[5, 2, 3] = np.nan
    out = pkg.capi.solve(qp, x0, ST)
    assert out["status"][5] == 3
    keep = np.arange(8) != 5
    assert np.all(out["status"][keep] == 0)
    for k in ("x", "u", "pi", "iter", "obj") + SLACKS:
        assert np.array_equal(out[k][keep], good[k][keep]), k


def test_rejections(pkg, OcpQpBatch):
    """9. What the soft entry point does not build is rejected with its cause."""
    import torch
    capi = pkg.capi
    qp, x0 = family(OcpQpBatch)
    with pytest.raises(capi.SrbdQpError, match=r"\(-6\).*Balance"):
        capi.solve(qp, x0, dict(ST, mode="Balance"))
    with pytest.raises(capi.SrbdQpError, match=r"\(-6\).*f32_iters"):
        capi.solve(qp, x0, dict(ST, f32_iters=3))
    qg, xg = helpers.random_constrained(4, 5, 4, 2, 3, 3, OcpQpBatch)
    soft_lift.soften_x(qg, (1, 3), 1.0, 1.0)
    with pytest.raises(capi.SrbdQpError, match=r"\(-2\).*ng"):
        capi.solve(qg, xg, ST)
    # soft_x on a handle without has_box_x
    qu, xu = helpers.random_constrained(4, 5, 4, 2, 0, 3, OcpQpBatch)
    qu.lbx = qu.ubx = qu.lbx_mask = qu.ubx_mask = None
    h = capi.Handle(5, 4, 2, 0, True, False, capacity=4)
    dt, st, data, sol = capi.device_buffers(qu, xu)
    ones = torch.ones(4, 6, 4, dtype=torch.float64, device="cuda:0")
    soft = capi.Soft(soft_x=ones.data_ptr(), Zl_x=ones.data_ptr(), Zu_x=ones.data_ptr(),
                     zl_x=ones.data_ptr(), zu_x=ones.data_ptr())
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*has_box_x"):
        h.solve_soft_device(4, capi.settings_struct(ST), data, soft, sol)
    h.close()


def test_python_surface(pkg, OcpQpBatch):
    """10. capi.solve returns the slacks; the soft buffers are first-use allocations the
    handle counts; a hard solve on the handle afterwards is what it was before."""
    capi = pkg.capi
    hardqp, x0 = helpers.random_constrained(16, 5, 4, 2, 0, 3, OcpQpBatch)
    qp, _ = family(OcpQpBatch)
    h = capi.Handle(5, 4, 2, 0, True, True, capacity=16)
    before = capi.solve(hardqp, x0, ST, handle=h)
    m0 = h.memory_bytes()
    out = capi.solve(qp, x0, ST, handle=h)
    m1 = h.memory_bytes()
    for k in SLACKS:
        assert k in out
    assert out["sl_x"].shape == (16, 6, 4) and out["sl_u"].shape == (16, 5, 2)
    assert np.all(out["status"] == 0) and np.max(out["sl_x"] + out["su_x"]) > 1e-3
    # the slack state (N + 1 stages x 288 doubles per QP) and the 12-wide soft arrays
    assert m1 >= m0 + 16 * 6 * 288 * 8, (m0, m1)
    capi.solve(qp, x0, ST, handle=h)
    assert h.memory_bytes() == m1
    after = capi.solve(hardqp, x0, ST, handle=h)
    assert h.memory_bytes() == m1
    for k in ("x", "u", "pi", "status", "iter", "res", "obj"):
        assert np.array_equal(after[k], before[k]), k
    h.close()


def test_host_entry_point(pkg, OcpQpBatch):
    """srbd_qp_solve_soft_host_f64 from numpy buffers gives the device call's result."""
    capi = pkg.capi
    qp, x0 = family(OcpQpBatch)
    dev = capi.solve(qp, x0, ST)
    p = qp.packed()
    p["x0"] = np.ascontiguousarray(x0)
    ptr = lambda a: None if a is None else a.ctypes.data
    nb, N, nx, nu = qp.batch, qp.N, qp.nx, qp.nu
    out = {"x": np.zeros((nb, N + 1, nx)), "u": np.zeros((nb, N, nu)), "pi": np.zeros((nb, N + 1, nx)),
           "status": np.full(nb, -1, dtype=np.int32), "iter": np.full(nb, -1, dtype=np.int32),
           "res": np.zeros((nb, 4)), "obj": np.zeros(nb)}
    sk = {"sl_u": np.ones((nb, N, nu)), "su_u": np.ones((nb, N, nu)),
          "sl_x": np.ones((nb, N + 1, nx)), "su_x": np.ones((nb, N + 1, nx))}
    data = capi.Data(**{k: ptr(p.get(k)) for k in capi.DATA_FIELDS})
    soft = capi.Soft(**{k: ptr(p.get(k)) for k in capi.SOFT_FIELDS})
    sol = capi.Solution(**{k: ptr(out.get(k)) for k in capi.SOL_FIELDS})
    slack = capi.Slack(**{k: ptr(v) for k, v in sk.items()})
    h = capi.Handle(N, nx, nu, 0, True, True, capacity=nb)
    h.solve_soft_host(nb, capi.settings_struct(ST), data, soft, sol, slack)
    h.close()
    for k, v in dict(out, **sk).items():
        assert np.array_equal(v, dev[k]), k
