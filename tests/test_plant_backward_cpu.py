"""The differentiable plant without a GPU: the two symbols and their ctypes
mirrors against the header, the argument checks of both calls in the order the header lists them,
and the numpy adjoint tests/plant_vjp_host.py against central differences of the
srbd_model.plant_step loop in every one of its seven outputs."""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest

import helpers
import plant_vjp_host as PV
import robots_host as BH
import rollout_host as RH

EINVAL, EDIM, ECAPACITY = -1, -2, -5
FORWARD, BACKWARD = "srbd_qp_srbd_plant_rollout_f64", "srbd_qp_srbd_plant_rollout_backward_f64"
B, T = 3, 3
FD_REL_STEP = 1e-4  # (1e-6 reaches the bound by difference noise: foot_l 7.8e-7, u 2.9e-7)
FD_BOUND = 1e-6  # |g - fd| <= FD_BOUND max|fd| per output array


def make_case(sm, per_robot=False):
    """x0 and a base input from rollout_host.start(sm, p, 3, 4, 5); u = its first stage repeated
    plus N(0, 5); the feet the params' plus N(0, 0.05); the wrench U(-20, 20); gx N(0, 1) on all
    T + 1 rows: one default_rng(1), in this order."""
    p = sm.SrbdParams()
    _, us, x0 = RH.start(sm, p, B, 4, 5)
    rng = np.random.default_rng(1)
    u = np.repeat(us[:, :1], T, axis=1) + rng.normal(0.0, 5.0, size=(B, T, 12))
    foot_r = np.array(p.foot_r) + rng.normal(0.0, 0.05, size=(B, T, 3))
    foot_l = np.array(p.foot_l) + rng.normal(0.0, 0.05, size=(B, T, 3))
    wrench = rng.uniform(-20.0, 20.0, size=(B, T, 6))
    gx = rng.normal(0.0, 1.0, size=(B, T + 1, 12))
    params = BH.draw_plant(BH.draw(p, B, 11), 12) if per_robot else [p] * B
    return params, x0, u, foot_r, foot_l, wrench, gx


def _step(value):
    return FD_REL_STEP * abs(value) if value != 0.0 else FD_REL_STEP


def fd_gradients(sm, params, x0, u, foot_r, foot_l, wrench, gx, substeps):
    """Central differences of sum <gx, x_traj> over the srbd_model.plant_step loop, one entry of
    one robot's inputs or parameters at a time; robot i alone is rolled out again."""
    arrays = {"x0": x0, "u": u, "foot_r": foot_r, "foot_l": foot_l, "wrench": wrench}
    out = {k: np.zeros_like(v) for k, v in arrays.items()}
    out["mass"], out["Lbody"] = np.zeros(B), np.zeros((B, 3))

    def loss(i, q, a):
        xt = PV.rollout(sm, q, a["x0"][i:i + 1], a["u"][i:i + 1], a["foot_r"][i:i + 1], a["foot_l"][i:i + 1],
                        a["wrench"][i:i + 1], substeps)
        return float(np.sum(gx[i] * xt[0]))

    for i in range(B):
        for name, arr in arrays.items():
            for idx in np.ndindex(*arr.shape[1:]):
                h = _step(float(arr[(i,) + idx]))
                sides = []
                for sgn in (1.0, -1.0):
                    moved = arr.copy()
                    moved[(i,) + idx] += sgn * h
                    sides.append(loss(i, params[i], {**arrays, name: moved}))
                out[name][(i,) + idx] = (sides[0] - sides[1]) / (2.0 * h)
        for name in ("mass", "Lbody"):
            value = np.array(getattr(params[i], name), dtype=np.float64)
            for idx in np.ndindex(*value.shape):
                h = _step(float(value[idx]))
                sides = []
                for sgn in (1.0, -1.0):
                    v = value.copy()
                    v[idx] += sgn * h
                    q = dataclasses.replace(params[i], **{name: float(v) if v.ndim == 0 else tuple(v.tolist())})
                    sides.append(loss(i, q, arrays))
                out[name][(i,) + idx] = (sides[0] - sides[1]) / (2.0 * h)
    return out


@pytest.mark.parametrize("substeps", [2, 1])
def test_statement_matches_central_differences(pkg, substeps):
    """Every output of the statement against central differences of the forward host loop, at a
    relative step of 1e-4.  Seen (largest |g - fd| / max|fd| of the two cases): x0 8.3e-11, u 5.3e-10,
    foot_r 8.9e-10, foot_l 5.9e-9, wrench 8.9e-10, mass 1.0e-8, Lbody 1.0e-8."""
    sm = pkg.srbd_model
    params, x0, u, foot_r, foot_l, wrench, gx = make_case(sm)
    x_traj = PV.rollout(sm, params[0], x0, u, foot_r, foot_l, wrench, substeps)
    got = PV.plant_vjp(sm, params[0], x_traj, u, gx, foot_r, foot_l, wrench, substeps)
    want = fd_gradients(sm, params, x0, u, foot_r, foot_l, wrench, gx, substeps)
    for name in PV.OUTPUTS:
        scale = np.abs(want[name]).max()
        err = np.abs(got[name] - want[name]).max()
        print(f"substeps {substeps} {name}: max|fd| {scale:.3g}, |g - fd| / max|fd| {err / scale:.2e}")
        assert scale > 0.0, name
        assert got[name].shape == want[name].shape, name
        assert err <= FD_BOUND * scale, (name, err, scale)


def test_per_robot_parameters_are_the_scalar_statement_robot_by_robot(pkg):
    sm = pkg.srbd_model
    params, x0, u, foot_r, foot_l, wrench, gx = make_case(sm, per_robot=True)
    x_traj = PV.rollout(sm, params, x0, u, foot_r, foot_l, wrench, 2)
    got = PV.plant_vjp(sm, params, x_traj, u, gx, foot_r, foot_l, wrench, 2)
    for i, q in enumerate(params):
        s = slice(i, i + 1)
        xt = PV.rollout(sm, q, x0[s], u[s], foot_r[s], foot_l[s], wrench[s], 2)
        np.testing.assert_array_equal(xt, x_traj[s])
        one = PV.plant_vjp(sm, q, xt, u[s], gx[s], foot_r[s], foot_l[s], wrench[s], 2)
        for name in PV.OUTPUTS:
            np.testing.assert_array_equal(one[name][0], got[name][i], err_msg=name)
    # and the robots differ: the draw reaches the gradients
    assert np.ptp(got["mass"]) > 0.0


def test_symbols_are_exported_and_bound(pkg):
    capi = pkg.capi
    for name in (FORWARD, BACKWARD):
        assert name in capi.exported_symbols() and name in capi.PROTOTYPES
        assert hasattr(capi.lib(), name)
    assert capi.lib().srbd_qp_abi_version() == 12  # additive to ABI 12
    assert hasattr(capi, "srbd_plant_rollout") and hasattr(capi, "srbd_plant_rollout_backward")
    assert hasattr(pkg.diff, "plant_rollout")


def _header_struct(name):
    hdr = (helpers.REPO / "include" / "srbd_qp.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            kind = "int" if decl.startswith("int") else "ptr"
            assert kind == "int" or decl.startswith(("double", "const double")), decl
            names = re.findall(r"\*\s*(\w+)", decl) if kind == "ptr" else [decl.split()[-1]]
            fields += [(n, kind) for n in names]
    return fields


def test_ctypes_mirrors_are_the_headers_structs(pkg):
    capi = pkg.capi
    kind = lambda t: "int" if t is C.c_int else "ptr"
    for name, mirror in (("srbd_plant_rollout_f64", capi.PlantRolloutStruct), ("srbd_plant_grad_f64", capi.PlantGrad)):
        assert _header_struct(name) == [(n, kind(t)) for n, t in mirror._fields_], name
    assert [n for n, _ in capi.PlantGrad._fields_] == list(capi.PLANT_GRAD_FIELDS)
    assert C.sizeof(capi.PlantGrad) == 7 * C.sizeof(C.c_void_p)
    assert C.sizeof(capi.PlantRolloutStruct) == 16 + 4 * C.sizeof(C.c_void_p)  # three ints, padding, four pointers
    P, i, vp = C.POINTER, C.c_int, C.c_void_p
    head = [vp, i, P(capi.ModelParams), P(capi.PlantRolloutStruct)]
    assert capi.PROTOTYPES[FORWARD][:2] == (i, head + [vp, vp, vp])
    assert capi.PROTOTYPES[BACKWARD][:2] == (i, head + [vp, vp, P(capi.PlantGrad), vp])


def _fake_handle(capi, dims, capacity):
    """Memory that begins like the library's handle (dims, then capacity): the checks below are
    all made before any device work and read nothing else of it."""
    buf = C.create_string_buffer(1 << 16)
    C.memmove(buf, C.byref(dims), C.sizeof(dims))
    C.memmove(C.byref(buf, C.sizeof(dims)), C.byref(C.c_int(capacity)), C.sizeof(C.c_int))
    return buf


@pytest.mark.parametrize("symbol", [FORWARD, BACKWARD])
def test_argument_checks_in_the_headers_order(pkg, symbol):
    capi = pkg.capi
    L = capi.lib()
    p = capi.default_model_params()
    ok, odd = C.c_void_p(64), C.c_void_p(72)  # 16-byte aligned; 8-byte aligned only
    good = dict(ticks=2, substeps=1, foot_stages=0, u=64)
    keep = _fake_handle(capi, capi.Dims(4, 12, 12, 0, 0, 0, 0), 4)
    keep13 = _fake_handle(capi, capi.Dims(4, 13, 12, 0, 0, 0, 0), 4)
    h = C.cast(keep, C.c_void_p)
    grad = capi.PlantGrad(mass=8)
    backward = symbol == BACKWARD

    def call(h=h, batch=1, params=C.byref(p), roll=good, x0=ok, x_traj=ok, gx=ok, grad=C.byref(grad)):
        r = None if roll is None else C.byref(capi.PlantRolloutStruct(**roll))
        if backward:
            return getattr(L, symbol)(h, batch, params, r, x_traj, gx, grad, None)
        return getattr(L, symbol)(h, batch, params, r, x0, x_traj, None)

    bad_roll = dict(good, ticks=-1, substeps=0)
    # 1. NULL h, params, roll (forward: x0) -- before anything else (the other arguments are bad too)
    for kw in (dict(h=None), dict(params=None), dict(roll=None)) + (() if backward else (dict(x0=None),)):
        assert call(**{"batch": 99, "roll": bad_roll, "x_traj": None, **kw}) == EINVAL, kw
        assert "NULL argument" in L.srbd_qp_last_error().decode()
    # then a NULL x_traj (backward: gx, grad) -- before roll's values
    assert call(batch=99, roll=bad_roll, x_traj=None) == EINVAL
    assert "x_traj" in L.srbd_qp_last_error().decode()
    if backward:
        for kw in (dict(gx=None), dict(grad=None)):
            assert call(batch=99, roll=bad_roll, **kw) == EINVAL, kw
            assert "gx or grad" in L.srbd_qp_last_error().decode()
    # roll, field by field: u with ticks > 0, ticks, substeps, foot_stages -- before the handle's dims
    h13 = C.cast(keep13, C.c_void_p)
    for roll, word in ((dict(bad_roll, ticks=2, u=None), "roll->u"), (dict(bad_roll, u=None), "ticks"),
                       (dict(good, substeps=0, foot_stages=1), "substeps"), (dict(good, foot_stages=1), "foot_stages")):
        assert call(h=h13, batch=99, roll=roll) == EINVAL, roll
        assert word in L.srbd_qp_last_error().decode(), (roll, L.srbd_qp_last_error().decode())
    # 2. the dimensions, 3. the capacity -- before the alignment
    assert call(h=h13, batch=99, x_traj=odd) == EDIM
    assert call(batch=5, x_traj=odd) == ECAPACITY
    assert call(batch=-1, x_traj=odd) == ECAPACITY
    # 4. 16-byte alignment of x0 (forward), u, x_traj, gx (backward) -- before batch == 0
    for kw in (dict(roll=dict(good, u=72)), dict(x_traj=odd), dict(gx=odd) if backward else dict(x0=odd)):
        assert call(batch=0, **kw) == EINVAL, kw
        assert "16-byte aligned" in L.srbd_qp_last_error().decode()
    # 5. batch == 0 is a success that does nothing; foot_stages 0, = ticks and above it pass; ticks == 0 needs no u
    assert call(batch=0) == 0
    assert call(batch=0, roll=dict(good, foot_stages=2)) == 0
    assert call(batch=0, roll=dict(good, foot_stages=7)) == 0
    assert call(batch=0, roll=dict(ticks=0, substeps=3, foot_stages=0, u=None)) == 0


def test_binding_checks_its_tensors(pkg):
    import types

    import torch
    capi = pkg.capi
    handle = types.SimpleNamespace(dims=capi.Dims(4, 12, 12, 0, 0, 0, 0), device=0)
    x0, u = torch.zeros(B, 12, dtype=torch.float64), torch.zeros(B, T, 12, dtype=torch.float64)
    with pytest.raises(ValueError, match="x0 is on cpu"):
        capi.srbd_plant_rollout(handle, x0, u)
    with pytest.raises(ValueError, match="x0 must be"):
        capi.srbd_plant_rollout(handle, x0.float(), u)
    with pytest.raises(ValueError, match="x0 has shape"):
        capi.srbd_plant_rollout_backward(handle, x0[:, :6], u, x_traj=None, gx=None)
