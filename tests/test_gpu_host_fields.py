"""The host-buffer entry points stage every field of the call: each case solves once through
device buffers (capi.solve) and once through Handle.solve_host with every optional output
requested (P, p, K, k, status, iter, res, obj, stat), and the two agree bit for bit, field by
field.  The cases cover the paths of the staging code: the one-QP resident server, the
zero-copy launch, the pinned one-copy-each-way path (constrained, embedded, with and without
the adjacent x / u warm-start upload, fp64 and fp32) and the field-by-field copies of a batch
whose staged bytes exceed the pinned limit."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

OUTPUTS = ("x", "u", "pi", "P", "p", "K", "k", "status", "iter", "res", "obj", "stat")
PINNED_MAX_BYTES = 8 << 20  # kPinnedMaxBytes (capi_host.hip)


def _host_solve(capi, qp, x0, st, dtype=np.float64, x_init=None, u_init=None):
    """Handle.solve_host on numpy buffers, all outputs; returns (outputs, staged bytes)."""
    f32 = np.dtype(dtype) == np.float32
    DataT, SolT = (capi.Data32, capi.Solution32) if f32 else (capi.Data, capi.Solution)
    s = capi.settings_struct(st)
    nb, N, nx, nu = qp.batch, qp.N, qp.nx, qp.nu
    p = {k: (None if v is None else np.ascontiguousarray(v, dtype=dtype)) for k, v in qp.packed().items()}
    p["x0"] = np.ascontiguousarray(x0, dtype=dtype).reshape(nb, nx)
    out = {
        "x": np.zeros((nb, N + 1, nx), dtype) if x_init is None else np.ascontiguousarray(x_init, dtype=dtype),
        "u": np.zeros((nb, N, nu), dtype) if u_init is None else np.ascontiguousarray(u_init, dtype=dtype),
        "pi": np.zeros((nb, N + 1, nx), dtype),
        "P": np.zeros((nb, N + 1, nx, nx), dtype), "p": np.zeros((nb, N + 1, nx), dtype),
        "K": np.zeros((nb, N, nx, nu), dtype), "k": np.zeros((nb, N, nu), dtype),
        "status": np.full((nb,), -1, np.int32), "iter": np.full((nb,), -1, np.int32),
        "res": np.zeros((nb, 4), dtype), "obj": np.zeros((nb,), dtype),
        "stat": np.zeros((nb, s.iter_max + 2, 18), dtype),
    }
    assert set(out) == set(OUTPUTS) == set(capi.SOL_FIELDS)
    data = DataT(**{k: (None if p.get(k) is None else p[k].ctypes.data) for k in capi.DATA_FIELDS})
    sol = SolT(**{k: v.ctypes.data for k, v in out.items()})
    h = capi.Handle(N, nx, nu, qp.ng, qp.has_box_u, qp.has_box_x, capacity=nb)
    try:
        h.solve_host(nb, s, data, sol)
    finally:
        h.close()
    staged = sum((a.nbytes + 255) // 256 * 256
                 for a in [p.get(k) for k in capi.DATA_FIELDS] + list(out.values()) if a is not None)
    # (capi.solve returns P and K with their last two axes swapped)
    out["P"] = np.swapaxes(out["P"], -1, -2)
    out["K"] = np.swapaxes(out["K"], -1, -2)
    return out, staged


def _check(pkg, qp, x0, st, **kw):
    dev = pkg.capi.solve(qp, x0, st, riccati=True, stats=True, **kw)
    host, staged = _host_solve(pkg.capi, qp, x0, st, **kw)
    # (every QP ran: the buffers start at -1; whether it converged is not this test's matter)
    assert np.all(dev["status"] >= 0) and np.all(dev["iter"] >= 0), (dev["status"], dev["iter"])
    for key in OUTPUTS:
        assert host[key].shape == dev[key].shape and host[key].dtype == dev[key].dtype, key
        assert np.array_equal(host[key], dev[key]), key
    return staged


@pytest.mark.parametrize("batch", [1, 2])
def test_unconstrained_small(pkg, batch):
    """batch 1: the resident server; batch 2: the zero-copy launch."""
    qp, x0 = helpers.random_unconstrained(batch, 3, 12, 12, 31, pkg.OcpQpBatch)
    assert _check(pkg, qp, x0, {}) <= PINNED_MAX_BYTES


@pytest.mark.parametrize("case", ["cold", "warm", "cold_f32"])
def test_constrained_embedded(pkg, case):
    """Boxes with masks on u and x, general rows, nx = 8 and nu = 4 embedded in 12 x 12 stages:
    the pinned staging buffer, one copy each way; `warm` adds the x / u upload."""
    qp, x0 = helpers.random_constrained(3, 4, 8, 4, 6, 47, pkg.OcpQpBatch)
    kw = {}
    st = dict(iter_max=30)
    if case == "warm":
        rng = np.random.default_rng(5)
        st["warm_start"] = 1
        kw = dict(x_init=0.1 * rng.uniform(-1, 1, (3, 5, 8)), u_init=0.1 * rng.uniform(-1, 1, (3, 4, 4)))
    if case == "cold_f32":
        kw = dict(dtype=np.float32)
        st = dict(iter_max=30, tol_stat=1e-3, tol_eq=1e-3, tol_ineq=1e-3, tol_comp=1e-3)
    assert _check(pkg, qp, x0, st, **kw) <= PINNED_MAX_BYTES


def test_large_batch_copies_field_by_field(pkg):
    """96 QPs of N = 20 with P and K: more than the pinned limit, so every field is copied
    on its own, both ways."""
    qp, x0 = helpers.random_unconstrained(96, 20, 12, 12, 13, pkg.OcpQpBatch)
    assert _check(pkg, qp, x0, {}) > PINNED_MAX_BYTES
