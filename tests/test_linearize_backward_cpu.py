"""The backward pass of the SRBD linearisation without a GPU: the numpy
statement tests/linearize_vjp_host.py against central differences of robots_host.build_qp in
every one of its ten outputs, the argument checks of srbd_qp_srbd_linearize_backward_f64 in the
order the header lists them, and the ctypes mirror against the header."""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest

import helpers
import linearize_backward_cases as LC
import linearize_vjp_host as VH
import robots_host as BH

EINVAL, EDIM, ECAPACITY = -1, -2, -5
SYMBOL = "srbd_qp_srbd_linearize_backward_f64"
B, N = 3, 3
FD_REL_STEP = 1e-6
FD_BOUND = 1e-6  # |g - fd| <= FD_BOUND max|fd| per output array


def _step(value):
    return FD_REL_STEP * abs(value) if value != 0.0 else FD_REL_STEP


def fd_gradients(sm, p, params, plan, xs, us, constraints, cot):
    """Central differences of sum_X <cot[X], X> over robots_host.build_qp's arrays, one entry of
    one robot's parameters at a time (relative step 1e-6; 1e-6 absolute at a zero).  A robot's
    parameters reach its own blocks only, so robot i alone is rebuilt.  Without robots or without a
    plan the entry is moved in a copy that holds the shared value for every robot and stage."""
    if plan is None:
        plan = sm.SrbdPlan()
    full = LC.PH.constant_plan(sm, p, B, N)
    plan = sm.SrbdPlan(**{k: (getattr(full, k) if getattr(plan, k) is None else getattr(plan, k))
                          for k in LC.PLAN_FIELDS})
    shapes = {"mass": (), "Lbody": (3,), "mu": (), "Q": (12,), "Qf": (12,), "R": (), "x_ref": (N + 1, 12),
              "foot_r": (N, 3), "foot_l": (N, 3), "fz_max": (N, 2)}
    out = {k: np.zeros((B,) + s) for k, s in shapes.items()}

    def build(i, q, pl):
        one = sm.SrbdPlan(**{k: getattr(pl, k)[i:i + 1] for k in LC.PLAN_FIELDS})
        return BH.build_qp(sm, [q], xs[i:i + 1], us[i:i + 1], constraints, one)

    for i in range(B):
        cot_i = {k: v[i:i + 1] for k, v in cot.items()}
        for name, shape in shapes.items():
            for idx in np.ndindex(*shape):
                sides = []
                if name in BH.MODEL_FIELDS:
                    value = np.array(getattr(params[i], name), dtype=np.float64)
                    h = _step(float(value[idx]))
                    for sgn in (1.0, -1.0):
                        v = value.copy()
                        v[idx] += sgn * h
                        q = dataclasses.replace(params[i], **{name: float(v) if v.ndim == 0 else tuple(v.tolist())})
                        sides.append(build(i, q, plan))
                else:
                    h = _step(float(getattr(plan, name)[(i,) + idx]))
                    for sgn in (1.0, -1.0):
                        arr = getattr(plan, name).copy()
                        arr[(i,) + idx] += sgn * h
                        sides.append(build(i, params[i], dataclasses.replace(plan, **{name: arr})))
                out[name][(i,) + idx] = VH.contraction(cot_i, sides[0], sides[1], constraints) / (2.0 * h)
    return out


@pytest.mark.parametrize("given", ["robots and plan", "neither"])
@pytest.mark.parametrize("constraints", ["none", "box_u", "cone"])
def test_statement_matches_central_differences(pkg, constraints, given):
    """Every output of the statement against central differences of the forward host model.
    Seen (largest |g - fd| / max|fd| over the six cases): mass 9.5e-10, Lbody 3.9e-9, mu 2.0e-10,
    Q 1.3e-11, Qf 8.5e-11, R 1.6e-10, x_ref 8.7e-11, foot_r 1.2e-8, foot_l 9.1e-9, fz_max 1.2e-8."""
    sm = pkg.srbd_model
    with_both = given == "robots and plan"
    p, params, plan, xs, us = LC.make_case(sm, B, N, robots=BH.MODEL_FIELDS if with_both else (),
                                           plan=LC.PLAN_FIELDS if with_both else ())
    cot = LC.cotangents(B, N, constraints, 5)
    got = VH.linearize_vjp(sm, params, xs, us, constraints, cot, plan)
    want = fd_gradients(sm, p, params, plan, xs, us, constraints, cot)
    for name in VH.OUTPUTS:
        scale = np.abs(want[name]).max()
        err = np.abs(got[name] - want[name]).max()
        print(f"{constraints} {given} {name}: max|fd| {scale:.3g}, |g - fd| / max|fd| {err / scale:.2e}")
        # the cotangents' scaling: every output is O(1) or larger.  One cannot be: without a plan
        # fz_max is fmax = 1000, where the barrier's curvature is 1e-7 and, without CONE's lg, nothing else reaches it
        small_by_nature = name == "fz_max" and not with_both and constraints != "cone"
        assert scale >= (1e-6 if small_by_nature else 0.5), (name, scale)
        assert err <= FD_BOUND * scale, (name, err, scale)


def test_symbol_is_exported_and_bound(pkg):
    capi = pkg.capi
    assert SYMBOL in capi.exported_symbols() and SYMBOL in capi.PROTOTYPES
    assert hasattr(capi.lib(), SYMBOL)
    assert capi.lib().srbd_qp_abi_version() == 12  # additive to ABI 12
    assert hasattr(capi, "srbd_linearize_backward") and hasattr(pkg.diff, "srbd_linearize")


def test_ctypes_mirror_is_the_headers_struct(pkg):
    capi = pkg.capi
    hdr = (helpers.REPO / "include" / "srbd_qp.h").read_text()
    body = re.search(r"typedef struct srbd_lin_grad_f64 \{(.*?)\} srbd_lin_grad_f64;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            assert decl.strip().startswith("double"), decl
            fields += re.findall(r"\*\s*(\w+)", decl)
    assert fields == [n for n, _ in capi.LinGrad._fields_] == list(capi.LIN_GRAD_FIELDS)
    assert C.sizeof(capi.LinGrad) == len(fields) * C.sizeof(C.c_void_p)


def _fake_handle(capi, dims, capacity):
    """Memory that begins like the library's handle (dims, then capacity): the checks below are
    all made before any device work and read nothing else of it."""
    buf = C.create_string_buffer(1 << 16)
    C.memmove(buf, C.byref(dims), C.sizeof(dims))
    C.memmove(C.byref(buf, C.sizeof(dims)), C.byref(C.c_int(capacity)), C.sizeof(C.c_int))
    return buf


def test_argument_checks_in_the_headers_order(pkg):
    capi = pkg.capi
    L = capi.lib()
    p, plan, cot = capi.default_model_params(), capi.PlanStruct(), capi.Data()
    none, one = capi.LinGrad(), capi.LinGrad(mass=8)
    xs = us = C.c_void_p(16)
    keep = _fake_handle(capi, capi.Dims(N, 12, 12, 0, 0, 0, 0), 4)
    h = C.cast(keep, C.c_void_p)

    def call(h=h, batch=1, params=C.byref(p), constraints=0, xs=xs, us=us, cot=C.byref(cot), grad=C.byref(one)):
        return getattr(L, SYMBOL)(h, batch, params, C.byref(plan), constraints, xs, us, cot, grad, None)

    # 1. NULL h, params, xs, us, cot, grad -- before anything else (the other arguments are bad too)
    for kw in (dict(h=None), dict(params=None), dict(xs=None), dict(us=None), dict(cot=None), dict(grad=None)):
        assert call(batch=99, constraints=7, **kw) == EINVAL, kw
        assert "NULL" in L.srbd_qp_last_error().decode()
    # 2. check_srbd_call: the dimensions, then the capacity -- before the constraints mode
    keep13 = _fake_handle(capi, capi.Dims(N, 13, 12, 0, 0, 0, 0), 4)
    assert call(h=C.cast(keep13, C.c_void_p), batch=99, constraints=7) == EDIM
    assert call(batch=5, constraints=7) == ECAPACITY
    assert call(batch=-1, constraints=7) == ECAPACITY
    # 3. an unknown constraints mode, 4. CONE without ng = 24 -- before the outputs
    for mode in (-1, 3):
        assert call(constraints=mode, grad=C.byref(none)) == EINVAL
        assert "constraints" in L.srbd_qp_last_error().decode()
    assert call(constraints=2, grad=C.byref(none)) == EINVAL
    assert "ng = 24" in L.srbd_qp_last_error().decode()
    # 5. every output NULL -- before batch == 0
    assert call(batch=0, grad=C.byref(none)) == EINVAL
    assert "grad" in L.srbd_qp_last_error().decode()
    # 6. batch == 0 is a success that does nothing (CONE on a handle with ng = 24 too)
    assert call(batch=0) == 0
    keep24 = _fake_handle(capi, capi.Dims(N, 12, 12, 24, 0, 0, 0), 4)
    assert call(h=C.cast(keep24, C.c_void_p), batch=0, constraints=2) == 0


def test_binding_checks_its_tensors(pkg):
    import types

    import torch
    capi = pkg.capi
    handle = types.SimpleNamespace(dims=capi.Dims(N, 12, 12, 0, 0, 0, 0), device=0)
    xs, us = torch.zeros(B, N + 1, 12, dtype=torch.float64), torch.zeros(B, N, 12, dtype=torch.float64)
    with pytest.raises(ValueError, match="xs is on cpu"):
        capi.srbd_linearize_backward(handle, xs, us, {})
    with pytest.raises(ValueError, match="xs must be"):
        capi.srbd_linearize_backward(handle, xs.float(), us, {})
    with pytest.raises(ValueError, match="unknown constraints"):
        capi.srbd_linearize_backward(handle, xs, us, {}, constraints="soft")
