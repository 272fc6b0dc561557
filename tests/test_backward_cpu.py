"""The backward pass on the CPU: the numpy statement of its math (tests/adjoint_host.py) against
central finite differences of dense KKT solves, and the binding's checks that need no GPU."""
import ctypes as C
import types

import numpy as np
import pytest

import adjoint_host
import helpers

N, NX, NU, H = 3, 3, 2, 1e-6


def _problem(OcpQpBatch, seed=1):
    qp, x0 = helpers.random_unconstrained(1, N, NX, NU, seed, OcpQpBatch)
    rng = np.random.default_rng(seed + 100)
    return qp, x0[0], rng.uniform(-1, 1, (N + 1, NX)), rng.uniform(-1, 1, (N, NU))


def _fd(qp, x0, gx, gu, pinned, u_pin):
    """Central differences (h = 1e-6) of l = <gx, x> + <gu, u> over every entry of the nine
    inputs; Q and R are moved symmetrically (entry ij and ji together, and the pair's derivative
    is shared between the two entries)."""
    def loss(x0_):
        x, u, _ = adjoint_host.forward_host(qp, x0_, 0, pinned, u_pin)
        return float(np.sum(gx * x) + np.sum(gu * u))

    out = {}
    for name in adjoint_host.NAMES:
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
                vals.append(loss(x0))
                arr[idx], arr[twin] = keep
            d = (vals[0] - vals[1]) / (2 * H)
            if twin != idx:  # d = grad_ij + grad_ji, and the symmetric gradient has them equal
                g[idx] = g[twin] = 0.5 * d
            else:
                g[idx] = d
        out[name] = g
    return out


@pytest.mark.parametrize("pins", [(), ((0, 1), (2, 0))])
def test_adjoint_matches_finite_differences(OcpQpBatch, pins):
    """All nine gradients to abs 1e-7, free and with two inputs pinned at a bound (the
    active-set-fixed problem: the forward solve holds them there as equality rows)."""
    qp, x0, gx, gu = _problem(OcpQpBatch)
    pinned = np.zeros((N, NU), dtype=bool)
    for k, j in pins:
        pinned[k, j] = True
    xf, uf, _ = adjoint_host.forward_host(qp, x0)
    if not pins:  # the dense solve with x_0 as a variable is helpers.dense_kkt's
        xr, ur, pr = helpers.dense_kkt(qp, x0)
        _, _, pf = adjoint_host.forward_host(qp, x0)
        assert np.allclose(xf, xr, atol=1e-11) and np.allclose(uf, ur, atol=1e-11)
        assert np.allclose(pf[1:], pr[1:], atol=1e-10)
    # bounds that make exactly the pinned inputs active at the pinned forward solution
    u_pin = uf - 0.1 * pinned
    x, u, pi = adjoint_host.forward_host(qp, x0, 0, pinned, u_pin)
    qp.lbu = np.where(pinned, u_pin, u - 1.0)[None]
    qp.ubu = (u + 1.0)[None]
    got, npin = adjoint_host.adjoint_host(qp, x, u, pi, gx, gu, act_tol=1e-6 if pins else None)
    assert npin == len(pins)
    want = _fd(qp, x0, gx, gu, pinned, u_pin)
    for name in adjoint_host.NAMES:
        err = float(np.max(np.abs(got[name] - want[name])))
        print(f"[backward fd] pins {len(pins)} {name}: |grad| max {np.max(np.abs(want[name])):.2e} err {err:.2e}")
        assert err <= 1e-7, (name, err)
    # dx_0 = 0 and a pinned du = 0, to the rounding of the dense solve
    assert np.max(np.abs(got["q"][0])) <= 1e-13 and np.max(np.abs(got["Q"][0])) <= 1e-13
    for k, j in pins:
        assert abs(got["r"][k, j]) <= 1e-13


def test_symbol_is_exported_and_bound(pkg):
    capi = pkg.capi
    for name in ("srbd_qp_solve_backward_f64", "srbd_qp_backward_pinned_f64"):
        assert name in capi.exported_symbols() and name in capi.PROTOTYPES
        assert hasattr(capi.lib(), name)
    assert capi.lib().srbd_qp_abi_version() == 12
    assert [n for n, _ in capi.Grad._fields_] == ["A", "B", "b", "Q", "S", "R", "q", "r", "x0"]


def test_argument_checks_return_einval(pkg):
    """A NULL handle, both cotangents NULL and a negative act_tol are SRBD_QP_EINVAL.  The checks
    that read the arguments alone come before the handle is read, so the last two are reached
    with a handle that is only an address (zeroed memory that is never a real handle)."""
    capi = pkg.capi
    L = capi.lib()
    st, data, sol, grad = capi.settings_struct(), capi.Data(), capi.Solution(), capi.Grad()
    call = lambda h, gx, gu, tol: L.srbd_qp_solve_backward_f64(h, 1, C.byref(st), C.byref(data), C.byref(sol), gx,
                                                               gu, tol, C.byref(grad), None)
    assert call(None, C.c_void_p(8), None, 0.0) == -1
    assert "handle" in L.srbd_qp_last_error().decode()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    assert call(h, None, None, 0.0) == -1
    assert "cotangent" in L.srbd_qp_last_error().decode()
    for tol in (-1e-3, float("nan"), float("inf")):
        assert call(h, C.c_void_p(8), None, tol) == -1
        assert "act_tol" in L.srbd_qp_last_error().decode()
    assert L.srbd_qp_backward_pinned_f64(None, 1, None, None) == -1


def test_solve_qp_rejects_cpu_and_float32_tensors(pkg):
    import torch
    capi, diff = pkg.capi, pkg.diff
    handle = types.SimpleNamespace(dims=capi.Dims(N, NX, NU, 0, 0, 0, 0), device=0)
    shapes = diff._shapes(handle.dims)
    names = ("A", "B", "b", "Q", "S", "R", "q", "r", "x0")
    cpu = [torch.zeros(2, *shapes[n], dtype=torch.float64) for n in names]
    with pytest.raises(ValueError, match="A is on cpu"):
        diff.solve_qp(handle, *cpu)
    f32 = [torch.zeros(2, *shapes[n], dtype=torch.float32) for n in names]
    with pytest.raises(ValueError, match="A must be a torch.float64 tensor"):
        diff.solve_qp(handle, *f32)
