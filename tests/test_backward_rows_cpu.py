"""The backward pass with general rows on the CPU: the numpy statement of its math
(tests/adjoint_rows_host.py) against central finite differences of a dense forward solve that
holds the same rows as equalities, the rule for dependent rows, and the binding's checks that
need no GPU.

Seen: the largest FD error over the fourteen gradients is 1.2e-9 (rows only) and 1.7e-9 (rows and
pins), against abs 1e-7 asked.
"""
import ctypes as C

import numpy as np
import pytest

import adjoint_host
import adjoint_rows_host as arh
import helpers

N, NX, NU, NG, H = 3, 3, 4, 3, 1e-6
ACT_TOL = 1e-6


def _problem(OcpQpBatch, rows, pins, seed=1):
    """A QP whose active set at its own (equality-held) solution is exactly `rows` ((k, j, upper))
    and `pins` ((k, c)): the bounds of those are put 0.1 inside the free solution, all others 1
    away from the held one."""
    qp, x0 = helpers.random_unconstrained(1, N, NX, NU, seed, OcpQpBatch)
    rng = np.random.default_rng(seed + 100)
    qp.ng = NG
    qp.D = rng.uniform(-1, 1, (1, N, NG, NU))
    _, uf, _ = adjoint_host.forward_host(qp, x0[0])
    gf = np.einsum("kgj,kj->kg", qp.D[0], uf)
    qp.lg, qp.ug = np.zeros((1, N + 1, NG)), np.zeros((1, N + 1, NG))
    qp.lbu, qp.ubu = np.zeros((1, N, NU)), np.zeros((1, N, NU))
    stages = [[] for _ in range(N)]
    for k, c in pins:
        qp.lbu[0, k, c] = uf[k, c] + 0.1
        stages[k].append(("pin", c, False, None, None))
    for k, j, upper in rows:
        (qp.ug if upper else qp.lg)[0, k, j] = gf[k, j] + (-0.1 if upper else 0.1)
        stages[k].append(("row", j, upper, None, None))
    x, u, pi = arh.forward_rows_host(qp, x0[0], stages)
    g = np.einsum("kgj,kj->kg", qp.D[0], u)
    act_l = np.zeros((N + 1, NG), dtype=bool)
    act_u = np.zeros((N + 1, NG), dtype=bool)
    for k, j, upper in rows:
        (act_u if upper else act_l)[k, j] = True
    pin = np.zeros((N, NU), dtype=bool)
    for k, c in pins:
        pin[k, c] = True
    qp.lg[0, :N] = np.where(act_l[:N], qp.lg[0, :N], g - 1.0)
    qp.ug[0, :N] = np.where(act_u[:N], qp.ug[0, :N], g + 1.0)
    qp.lg[0, N], qp.ug[0, N] = -1.0, 1.0
    qp.lbu[0] = np.where(pin, qp.lbu[0], u - 1.0)
    qp.ubu[0] = u + 1.0
    return qp, x0[0], stages, (x, u, pi), rng.uniform(-1, 1, (N + 1, NX)), rng.uniform(-1, 1, (N, NU))


def _fd(qp, x0, gx, gu, stages):
    """Central differences (h = 1e-6) of l = <gx, x> + <gu, u> over every entry of the fourteen
    inputs; Q and R are moved symmetrically, as in test_backward_cpu.py."""
    def loss():
        x, u, _ = arh.forward_rows_host(qp, x0, stages)
        return float(np.sum(gx * x) + np.sum(gu * u))

    out = {}
    for name in arh.ALL_NAMES:
        arr = x0 if name == "x0" else getattr(qp, name)[0]
        g = np.zeros_like(arr)
        for idx in np.ndindex(*arr.shape):
            twin = idx[:-2] + (idx[-1], idx[-2]) if name in ("Q", "R") else idx
            if name in ("Q", "R") and idx[-2] > idx[-1]:
                continue
            vals = []
            for sgn in (1.0, -1.0):
                keep = arr[idx], arr[twin]
                arr[idx] += sgn * H
                if twin != idx:
                    arr[twin] += sgn * H
                vals.append(loss())
                arr[idx], arr[twin] = keep
            d = (vals[0] - vals[1]) / (2 * H)
            if twin != idx:
                g[idx] = g[twin] = 0.5 * d
            else:
                g[idx] = d
        out[name] = g
    return out


ROWS = ((0, 1, False), (1, 0, True), (1, 2, False), (2, 2, False))


@pytest.mark.parametrize("pins", [(), ((0, 1), (2, 0))])
def test_adjoint_rows_match_finite_differences(OcpQpBatch, pins):
    """All fourteen gradients to abs 1e-7: four active rows, without and with two pinned inputs."""
    qp, x0, stages, (x, u, pi), gx, gu = _problem(OcpQpBatch, ROWS, pins)
    got, counts = arh.adjoint_rows_host(qp, x, u, pi, gx, gu, 0, ACT_TOL, 1e-8)
    assert counts == (len(pins), len(ROWS), 0)
    want = _fd(qp, x0, gx, gu, stages)
    worst = 0.0
    for name in arh.ALL_NAMES:
        err = float(np.max(np.abs(got[name] - want[name])))
        worst = max(worst, err)
        print(f"[backward rows fd] pins {len(pins)} {name}: |grad| max {np.max(np.abs(want[name])):.2e} err {err:.2e}")
        assert err <= 1e-7, (name, err)
    print(f"[backward rows fd] pins {len(pins)}: worst {worst:.2e}")
    # inactive rows and bounds are exactly zero
    active = {(k, j) for k, j, _ in ROWS}
    for k in range(N):
        for j in range(NG):
            if (k, j) not in active:
                assert not got["D"][k, j].any() and got["lg"][k, j] == 0.0 and got["ug"][k, j] == 0.0
    assert not got["lg"][N].any() and not got["ug"][N].any()
    for k, j, upper in ROWS:
        assert got["ug" if upper else "lg"][k, j] != 0.0 and got["lg" if upper else "ug"][k, j] == 0.0
    assert np.count_nonzero(got["lbu"]) == len(pins) and not got["ubu"].any()


def test_dependent_rows_are_dropped(OcpQpBatch):
    """A duplicated active row: the second copy is dropped, its gradients are zero, all finite."""
    qp, x0, stages, (x, u, pi), gx, gu = _problem(OcpQpBatch, ((1, 0, False),), ())
    qp.D[0, 1, 2] = qp.D[0, 1, 0]
    qp.lg[0, 1, 2] = qp.lg[0, 1, 0]
    qp.ug[0, 1, 2] = qp.lg[0, 1, 2] + 2.0
    got, counts = arh.adjoint_rows_host(qp, x, u, pi, gx, gu, 0, ACT_TOL, 1e-8)
    assert counts == (0, 1, 1)
    assert all(np.all(np.isfinite(v)) for v in got.values())
    assert not got["D"][1, 2].any() and got["lg"][1, 2] == 0.0 and got["ug"][1, 2] == 0.0
    assert got["D"][1, 0].any() and got["lg"][1, 0] != 0.0


def test_more_active_rows_than_inputs(OcpQpBatch):
    """nu + 1 rows active in one stage (ng = 5 > nu = 4): four accepted, one dropped."""
    qp, x0 = helpers.random_unconstrained(1, N, NX, NU, 3, OcpQpBatch)
    rng = np.random.default_rng(7)
    ng = NU + 1
    qp.ng = ng
    qp.D = rng.uniform(-1, 1, (1, N, ng, NU))
    _, u, _ = adjoint_host.forward_host(qp, x0[0])
    x, _, pi = adjoint_host.forward_host(qp, x0[0])
    g = np.einsum("kgj,kj->kg", qp.D[0], u)
    qp.lg, qp.ug = np.full((1, N + 1, ng), -50.0), np.full((1, N + 1, ng), 50.0)
    qp.lg[0, 1] = g[1]  # every row of stage 1 sits on its lower bound
    got, counts = arh.adjoint_rows_host(qp, x, u, pi, rng.uniform(-1, 1, (N + 1, NX)), rng.uniform(-1, 1, (N, NU)),
                                        0, ACT_TOL, 1e-8)
    assert counts == (0, NU, 1)
    assert all(np.all(np.isfinite(v)) for v in got.values())
    assert not got["D"][1, ng - 1].any() and got["lg"][1, ng - 1] == 0.0
    assert np.max(np.abs(got["r"][1])) <= 1e-12  # du_1 = 0: no direction is left


def test_symbols_are_exported_and_bound(pkg):
    capi = pkg.capi
    for name in ("srbd_qp_solve_backward_rows_f64", "srbd_qp_backward_active_f64"):
        assert name in capi.exported_symbols() and name in capi.PROTOTYPES
        assert hasattr(capi.lib(), name)
    assert capi.lib().srbd_qp_abi_version() == 12
    assert [n for n, _ in capi.GradRows._fields_] == ["D", "lg", "ug", "lbu", "ubu"]
    assert hasattr(capi.Handle, "solve_backward_rows_device") and hasattr(capi.Handle, "backward_active")


def test_argument_checks_return_einval(pkg):
    """A NULL handle, both grad structs NULL and a bad rank_tol are SRBD_QP_EINVAL; these checks
    read the arguments alone, so they are reached with a handle that is only an address."""
    capi = pkg.capi
    L = capi.lib()
    st, data, sol, grad, rows = capi.settings_struct(), capi.Data(), capi.Solution(), capi.Grad(), capi.GradRows()
    gx = C.c_void_p(8)

    def call(h, grad, rows, rank_tol):
        return L.srbd_qp_solve_backward_rows_f64(h, 1, C.byref(st), C.byref(data), C.byref(sol), gx, None, 0.0,
                                                 rank_tol, grad, rows, None)

    assert call(None, C.byref(grad), C.byref(rows), 1e-8) == -1
    assert "handle" in L.srbd_qp_last_error().decode()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    assert call(h, None, None, 1e-8) == -1
    assert "grad" in L.srbd_qp_last_error().decode()
    for tol in (-1e-3, 1.0, float("nan"), float("inf")):
        assert call(h, C.byref(grad), None, tol) == -1
        assert "rank_tol" in L.srbd_qp_last_error().decode()
    assert L.srbd_qp_backward_active_f64(None, 1, None, None) == -1


def test_solve_qp_checks_the_row_tensors(pkg):
    import types

    import torch
    capi, diff = pkg.capi, pkg.diff
    handle = types.SimpleNamespace(dims=capi.Dims(N, NX, NU, NG, 0, 0, 0), device=0)
    shapes = diff._shapes(handle.dims)
    assert shapes["D"] == (N, NU, NG) and shapes["lg"] == (N + 1, NG)
    cpu = [torch.zeros(2, *shapes[n], dtype=torch.float64) for n in adjoint_host.NAMES]
    with pytest.raises(ValueError, match="A is on cpu"):
        diff.solve_qp(handle, *cpu, D=torch.zeros(2, *shapes["D"], dtype=torch.float64))
