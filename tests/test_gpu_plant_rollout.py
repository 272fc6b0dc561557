"""The differentiable plant on the device: srbd_qp_srbd_plant_rollout_f64 tick by
tick against srbd_model.plant_step and against a closed-loop rollout's own log, its adjoint
srbd_qp_srbd_plant_rollout_backward_f64 against the numpy statement tests/plant_vjp_host.py and
against central differences of the device forward, what the header promises of both calls (bits,
outputs, attachments, memory, alignment, checks), and diff.plant_rollout.

Shapes: (B, T, substeps) = (1, 1, 1) a lone thread, (5, 3, 4), (65, 2, 1) a second workgroup of one
thread, (70, 5, 3) a partial second workgroup; the role and input grid runs on (5, 3, 4)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import contact_host as CH
import plant_vjp_host as PV
import robots_host as BH
import rollout_host as RH
import terrain_host as TH
from srbd_device import NMPC, SQP_MAX_LOOP, _dev, _dev_i32, close, device_contact, device_plan, device_terrain, handle

pytestmark = pytest.mark.gpu

EINVAL, EDIM, ECAPACITY = -1, -2, -5
SENTINEL = -7.25e77
STATEMENT_BOUND = 1e-9  # |device - statement| <= STATEMENT_BOUND max|statement| per output
SHAPES = [(1, 1, 1), (5, 3, 4), (65, 2, 1), (70, 5, 3)]
ROLES = ["none", "model", "plant mass", "both"]
# (feet, wrench): feet "long" = both arrays with T + 3 rows per robot, "left" = foot_l alone with T rows
INPUTS = [("long", True), ("long", False), (None, True), (None, False), ("left", True)]
GRID = [((5, 3, 4), inputs, role) for inputs in INPUTS[:4] for role in ROLES] + [((5, 3, 4), INPUTS[4], "model")]
GRID += [(shape, inputs, role) for shape in SHAPES for inputs, role in ((INPUTS[0], "both"), (INPUTS[3], "none"))
         if (shape, inputs, role) not in GRID]
IDS = [f"B{s[0]}-T{s[1]}-S{s[2]}-feet_{i[0]}-wrench_{int(i[1])}-{r.replace(' ', '_')}" for s, i, r in GRID]


class Case:
    """One call's inputs on the host and on the device, the handle with its roles, and the host
    parameters the plant step resolves to (one SrbdParams, or a list of one per robot)."""

    def __init__(self, pkg, shape, inputs=("long", True), role="none", seed=1, capacity=None):
        self.capi, self.sm = pkg.capi, pkg.srbd_model
        sm, capi = self.sm, self.capi
        self.B, self.T, self.substeps = B, T, S = shape
        p = sm.SrbdParams()
        _, us, x0 = RH.start(sm, p, B, 4, 5)
        rng = np.random.default_rng(seed)
        feet, with_wrench = inputs
        P = T + 3 if feet == "long" else T
        self.x0 = x0
        self.u = np.repeat(us[:, :1], T, axis=1) + rng.normal(0.0, 5.0, size=(B, T, 12))
        fr = np.array(p.foot_r) + rng.normal(0.0, 0.05, size=(B, P, 3))
        fl = np.array(p.foot_l) + rng.normal(0.0, 0.05, size=(B, P, 3))
        w = rng.uniform(-20.0, 20.0, size=(B, T, 6))
        self.gx = rng.normal(0.0, 1.0, size=(B, T + 1, 12))
        self.foot_r = fr if feet == "long" else None
        self.foot_l = fl if feet in ("long", "left") else None
        self.wrench = w if with_wrench else None
        self.h = handle(capi, 4, capacity or B, "none")
        model = BH.draw(p, B, 11)
        plant = BH.draw_plant(model, 12)
        self.params = p
        if role == "model":
            self.h.set_robots(model=capi.Robots(**{k: _dev(v) for k, v in BH.arrays(model).items()}))
            self.params = model
        elif role == "plant mass":  # the inertia falls back, here to the params'
            self.h.set_robots(plant=capi.Robots(mass=_dev(BH.arrays(plant, ("mass",))["mass"])))
            self.params = [dataclasses.replace(p, mass=q.mass) for q in plant]
        elif role == "both":  # the PLANT role's values win over the MODEL role's
            self.h.set_robots(model=capi.Robots(**{k: _dev(v) for k, v in BH.arrays(model).items()}),
                              plant=capi.Robots(**{k: _dev(v) for k, v in BH.arrays(plant, BH.PLANT_FIELDS).items()}))
            self.params = plant
        dev = lambda a: None if a is None else _dev(a)
        self.t = dict(x0=dev(self.x0), u=dev(self.u), foot_r=dev(self.foot_r), foot_l=dev(self.foot_l),
                      wrench=dev(self.wrench))
        self.gx_t = _dev(self.gx)

    def forward(self, **kw):
        return self.capi.srbd_plant_rollout(self.h, substeps=self.substeps, **{**self.t, **kw})

    def backward(self, x_traj, gx=None, **kw):
        return self.capi.srbd_plant_rollout_backward(self.h, substeps=self.substeps, x_traj=x_traj,
                                                     gx=self.gx_t if gx is None else gx, **{**self.t, **kw})

    def rows(self, name, t):
        a = getattr(self, name)
        return None if a is None else a[:, t]


# ---- 1. the forward call, one tick at a time, against srbd_model.plant_step ----
@pytest.mark.parametrize("shape,inputs,role", GRID, ids=IDS)
def test_forward_tick_by_tick_against_plant_step(pkg, shape, inputs, role):
    c = Case(pkg, shape, inputs, role)
    x_traj = c.forward()
    c.h.synchronize()
    got = x_traj.cpu().numpy()
    assert got.shape == (c.B, c.T + 1, 12) and np.array_equal(got[:, 0], c.x0)
    for t in range(c.T):
        want = RH.plant_step(c.sm, c.params, got[:, t], c.u[:, t], c.rows("foot_r", t), c.rows("foot_l", t),
                             c.rows("wrench", t), c.substeps)
        close(x_traj[:, t + 1], want, (shape, inputs, role, t))
        assert np.abs(want - got[:, t]).max() > 1e-6  # the robot moves
    c.h.close()


def test_forward_with_zero_ticks_writes_row_zero_only(pkg):
    import torch
    c = Case(pkg, (5, 0, 2), (None, False))
    out = torch.full((5, 1, 12), SENTINEL, dtype=torch.float64, device="cuda")
    assert c.forward(out=out) is out
    c.h.synchronize()
    assert torch.equal(out[:, 0], c.t["x0"])
    g = c.backward(out)
    c.h.synchronize()
    assert torch.equal(g["x0"], c.gx_t[:, 0]) and not g["mass"].any() and not g["Lbody"].any()
    assert g["u"].shape == (5, 0, 12) and g["wrench"].shape == (5, 0, 6)
    c.h.close()


# ---- 2. a closed-loop rollout's log is reproduced ----
def test_a_rollouts_log_is_reproduced_tick_by_tick(pkg):
    """srbd_rollout with a contact model (no true ground), a wrench and a feet plan: for the robots
    that stood through all T ticks, one tick of the plant rollout from x_log[:, t] with the applied
    input u_log[:, t], row t of the plan's feet and wrench[:, t] gives x_log[:, t + 1]."""
    capi, sm = pkg.capi, pkg.srbd_model
    B, N, T = 6, 10, 4
    p = sm.SrbdParams()
    xs, us, x = RH.start(sm, p, B, N, 21)
    plan = RH.feet_plan(sm, p, B, N + T - 1, 22)
    wrench = np.random.default_rng(23).uniform(-20.0, 20.0, size=(B, T, 6))
    contact = sm.SrbdContact(mu=0.3, Lt=(0.0, 0.05, 0.05), fz_hi=400.0, fz_contact=5.0, z_min=0.3, cos_tilt_min=0.3)
    h = handle(capi, N, B, "box_u")
    ct, st = device_contact(capi, contact, CH.zero_state(B))
    h.set_contact(ct)
    plan_t, wrench_t = device_plan(capi, plan), _dev(wrench)
    x_log, u_log, _, _ = capi.srbd_rollout(h, _dev(xs), _dev(us), _dev(x), _dev(np.ones(B)), T, "box_u", NMPC,
                                           SQP_MAX_LOOP, plan=plan_t, wrench=wrench_t)
    stood = st["alive"].cpu().numpy() == T
    assert stood.any(), st["alive"]
    print(f"[plant rollout] log: {int(stood.sum())} of {B} robots stood, sat {st['sat'].cpu().numpy()}")
    for t in range(T):
        one = capi.srbd_plant_rollout(h, x_log[:, t].contiguous(), u_log[:, t:t + 1].contiguous(),
                                      plan_t.foot_r[:, t:t + 1].contiguous(), plan_t.foot_l[:, t:t + 1].contiguous(),
                                      wrench_t[:, t:t + 1].contiguous())
        h.synchronize()
        close(one[:, 1].cpu()[stood], x_log[:, t + 1].cpu().numpy()[stood], t)
    # and in one call over all T ticks with the long plan's arrays as they are (foot_stages = N + T - 1)
    whole = capi.srbd_plant_rollout(h, x_log[:, 0].contiguous(), u_log, plan_t.foot_r, plan_t.foot_l, wrench_t)
    h.synchronize()
    np.testing.assert_allclose(whole.cpu().numpy()[stood], x_log.cpu().numpy()[stood], rtol=1e-9, atol=1e-10)
    h.close()


# ---- 3. the backward call against the host statement ----
@pytest.mark.parametrize("shape,inputs,role", GRID, ids=IDS)
def test_backward_against_the_host_statement(pkg, shape, inputs, role):
    """Seen (largest error / max|statement| over the grid): 5.0e-16 (foot_l)."""
    c = Case(pkg, shape, inputs, role)
    x_traj = c.forward()
    got = c.backward(x_traj)
    c.h.synchronize()
    T = c.T
    cut = lambda a: None if a is None else a[:, :T]
    want = PV.plant_vjp(c.sm, c.params, x_traj.cpu().numpy(), c.u, c.gx, cut(c.foot_r), cut(c.foot_l), c.wrench,
                        c.substeps)
    assert set(got) == set(PV.OUTPUTS)
    for name in PV.OUTPUTS:
        g = got[name].cpu().numpy()
        scale = np.abs(want[name]).max()
        err = np.abs(g - want[name]).max()
        print(f"[plant backward] {shape} {inputs} {role} {name}: max|statement| {scale:.3g}, error / max {err / scale:.2e}")
        assert g.shape == want[name].shape and scale > 0.0, name
        assert err <= STATEMENT_BOUND * scale, (name, err, scale)
    c.h.close()


# ---- 4. the backward call against central differences of the device forward ----
def test_backward_against_differences_of_the_device_forward(pkg):
    """Three probes per leaf, a relative step of 1e-4 (absolute at a zero), the bound 1e-6 of the
    array's largest gradient.  Seen: 1.0e-8 (mass), the truncation error of the differences."""
    import torch
    c = Case(pkg, (2, 3, 2), ("long", True), "both")
    x_traj = c.forward()
    grads = c.backward(x_traj)
    c.h.synchronize()
    model, plant = c.h._robots
    leaves = dict(c.t, mass=plant.mass, Lbody=plant.Lbody)
    probes = {"x0": [(0, 0), (1, 4), (0, 8)], "u": [(0, 0, 2), (1, 2, 4), (0, 1, 7)],
              "foot_r": [(0, 0, 2), (1, 2, 0), (0, 1, 1)], "foot_l": [(1, 0, 0), (0, 2, 1), (1, 1, 2)],
              "wrench": [(0, 0, 0), (1, 2, 5), (0, 1, 3)], "mass": [(0,), (1,), (0,)],
              "Lbody": [(0, 0), (1, 2), (0, 1)]}
    worst = 0.0
    for name, entries in probes.items():
        leaf, grad = leaves[name], grads[name].cpu().numpy()
        scale = np.abs(grad).max()
        assert scale > 0.0, name
        for idx in entries:
            v0 = float(leaf[idx])
            hstep = 1e-4 * abs(v0) if v0 != 0.0 else 1e-4
            sides = []
            for sgn in (1.0, -1.0):
                leaf[idx] = v0 + sgn * hstep
                sides.append(c.forward())
            leaf[idx] = v0
            fd = float((c.gx_t * (sides[0] - sides[1])).sum()) / (2.0 * hstep)
            err = abs(grad[idx] - fd)
            print(f"[plant backward] differences {name}{idx}: adjoint {grad[idx]:.6e}, differences {fd:.6e}, "
                  f"error / max|grad| {err / scale:.2e}")
            assert err <= 1e-6 * scale, (name, idx, grad[idx], fd, scale)
            worst = max(worst, err / scale)
    print(f"[plant backward] differences: worst {worst:.2e}")
    assert torch.equal(c.forward(), x_traj)  # every leaf is back
    c.h.close()


# ---- 5. what the header promises of the outputs ----
def test_outputs_alone_sentinels_and_repeatability(pkg):
    import torch
    c = Case(pkg, (5, 3, 2), ("long", True), "both")
    x_traj = c.forward()
    every = c.backward(x_traj)
    again = c.backward(x_traj)
    c.h.synchronize()
    assert torch.equal(c.forward(), x_traj)
    for name in PV.OUTPUTS:  # two calls: the same bits
        assert torch.equal(every[name], again[name]), name
        assert bool(torch.isfinite(every[name]).all()), name
    pad = 16  # doubles of sentinel either side of an output
    for name in PV.OUTPUTS:  # one output alone: the bits it has with all seven, and nothing else is written
        shape = every[name].shape
        big = torch.full((every[name].numel() + 2 * pad,), SENTINEL, dtype=torch.float64, device="cuda")
        view = big[pad:pad + every[name].numel()].view(shape)
        others = {n: torch.full_like(every[n], SENTINEL) for n in PV.OUTPUTS if n != name}
        out = c.backward(x_traj, want=[name], out={name: view, **others})
        c.h.synchronize()
        assert set(out) == {name} and out[name] is view
        assert torch.equal(view, every[name]), name
        assert bool((big[:pad] == SENTINEL).all()) and bool((big[pad + every[name].numel():] == SENTINEL).all()), name
        for n, o in others.items():
            assert bool((o == SENTINEL).all()), (name, n)
    c.h.close()


def test_a_cotangent_on_row_zero_alone_reaches_x0_alone(pkg):
    import torch
    c = Case(pkg, (5, 3, 2), ("long", True), "both")
    gx = torch.zeros_like(c.gx_t)
    gx[:, 0] = c.gx_t[:, 0]
    g = c.backward(c.forward(), gx=gx)
    c.h.synchronize()
    assert torch.equal(g["x0"], gx[:, 0])
    for name in PV.OUTPUTS[1:]:
        assert not g[name].any(), name
    c.h.close()


def test_one_step_is_the_transpose_of_the_forward_derivative(pkg):
    """T = 1, substeps = 1, the cotangent on row T alone: <gx[1], D x_1 (dv, du)> = <grad x0, dv> +
    <grad u, du>, the left side by central differences of the device forward along (dv, du)."""
    import torch
    c = Case(pkg, (3, 1, 1), ("long", True), "model")
    gx = torch.zeros_like(c.gx_t)
    gx[:, 1] = c.gx_t[:, 1]
    g = c.backward(c.forward(), gx=gx)
    rng = np.random.default_rng(3)
    dv, du = _dev(rng.normal(size=(3, 12))), _dev(10.0 * rng.normal(size=(3, 1, 12)))
    eps = 1e-4
    plus = c.forward(x0=c.t["x0"] + eps * dv, u=c.t["u"] + eps * du)
    minus = c.forward(x0=c.t["x0"] - eps * dv, u=c.t["u"] - eps * du)
    c.h.synchronize()
    lhs = (gx * (plus - minus)).sum(dim=(1, 2)).cpu().numpy() / (2.0 * eps)
    a, b = (g["x0"] * dv).sum(dim=1).cpu().numpy(), (g["u"] * du).sum(dim=(1, 2)).cpu().numpy()
    print(f"[plant backward] transpose: {lhs} against {a + b}")
    assert np.all(np.abs(lhs - (a + b)) <= 1e-6 * np.maximum(np.abs(a), np.abs(b)))
    c.h.close()


def test_the_handles_attachments_and_memory_are_left_alone(pkg):
    """With a contact model (every robot fallen), a terrain and an active set (nobody stepped) on
    the handle both calls give the bits they give without, and neither allocates handle memory."""
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    c = Case(pkg, (5, 3, 2), ("long", True), "both")
    before = c.h.memory_bytes()
    x_traj = c.forward()
    g = c.backward(x_traj)
    c.h.synchronize()
    assert c.h.memory_bytes() == before
    ground = sm.SrbdTerrain(height=np.stack([TH.rough(5, 6, 7, 0.06)]), x0=-0.3, y0=-0.4, cell=0.2)
    contact = sm.SrbdContact(mu=0.01, Lt=(0.0, 0.0, 0.0), fz_hi=1.0, fz_contact=5.0, ground=ground, z_min=5.0)
    state = CH.zero_state(c.B)
    state["fallen"][:] = 1
    ct, st = device_contact(capi, contact, state)
    c.h.set_contact(ct)
    c.h.set_terrain(device_terrain(capi, ground))
    c.h.set_active(capi.Active(mask=_dev_i32(np.zeros(c.B)), skip_fallen=True))
    x_with = c.forward()
    g_with = c.backward(x_with)
    c.h.synchronize()
    assert torch.equal(x_with, x_traj)
    for name in PV.OUTPUTS:
        assert torch.equal(g_with[name], g[name]), name
    assert not st["alive"].any() and not st["sat"].any()  # the contact's state was not touched
    assert c.h.memory_bytes() == before
    c.h.close()


# ---- 6. alignment: x0, u, x_traj and gx must be 16-byte aligned; 8-byte aligned views are rejected ----
def test_views_offset_by_one_double_are_rejected(pkg):
    import torch
    c = Case(pkg, (3, 2, 1), (None, False))

    def odd(t):  # the same values, 8 bytes past a 16-byte boundary
        big = torch.full((t.numel() + 1,), SENTINEL, dtype=torch.float64, device="cuda")
        v = big[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return v

    x_traj = c.forward()
    out = torch.full_like(x_traj, SENTINEL)
    for kw in (dict(x0=odd(c.t["x0"]), out=out), dict(u=odd(c.t["u"]), out=out), dict(out=odd(out))):
        with pytest.raises(capi_error(pkg), match="16-byte aligned"):
            c.forward(**kw)
        c.h.synchronize()
        assert bool((kw["out"] == SENTINEL).all())
    gout = {"x0": torch.full((3, 12), SENTINEL, dtype=torch.float64, device="cuda")}
    for kw in (dict(x_traj=odd(x_traj)), dict(x_traj=x_traj, gx=odd(c.gx_t)), dict(x_traj=x_traj, u=odd(c.t["u"]))):
        with pytest.raises(capi_error(pkg), match="16-byte aligned"):
            c.backward(want=["x0"], out=gout, **kw)
        c.h.synchronize()
        assert bool((gout["x0"] == SENTINEL).all())
    # the feet, the wrench and the outputs of grad need 8 bytes only
    c2 = Case(pkg, (3, 2, 1), ("long", True))
    ref_x = c2.forward()
    ref_g = c2.backward(ref_x)
    shifted = {k: odd(c2.t[k]) for k in ("foot_r", "foot_l", "wrench")}
    x2 = c2.forward(**shifted)
    g2 = c2.backward(x2, out={n: odd(torch.zeros_like(v)) for n, v in ref_g.items()}, **shifted)
    c2.h.synchronize()
    assert torch.equal(x2, ref_x)
    for name in PV.OUTPUTS:
        assert torch.equal(g2[name], ref_g[name]), name
    c.h.close()
    c2.h.close()


def capi_error(pkg):
    return pkg.capi.SrbdQpError


# ---- 7. one argument check per error code: nothing is written ----
def test_failed_checks_write_nothing(pkg):
    import torch
    capi = pkg.capi
    L = capi.lib()
    c = Case(pkg, (3, 2, 1), (None, False), capacity=3)
    small = capi.Handle(4, 4, 4, capacity=3)
    p = capi.default_model_params()
    x_traj = c.forward()
    out = torch.full_like(x_traj, SENTINEL)
    gx0 = torch.full((3, 12), SENTINEL, dtype=torch.float64, device="cuda")
    grad = capi.PlantGrad(x0=gx0.data_ptr())
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def calls(h, batch, substeps):
        roll = capi.PlantRolloutStruct(2, substeps, 0, c.t["u"].data_ptr(), None, None, None)
        return (L.srbd_qp_srbd_plant_rollout_f64(h.ptr, batch, C.byref(p), C.byref(roll), ptr(c.t["x0"]), ptr(out), None),
                L.srbd_qp_srbd_plant_rollout_backward_f64(h.ptr, batch, C.byref(p), C.byref(roll), ptr(x_traj),
                                                          ptr(c.gx_t), C.byref(grad), None))

    assert calls(c.h, 3, 0) == (EINVAL, EINVAL)
    assert calls(small, 3, 1) == (EDIM, EDIM)
    assert calls(c.h, 4, 1) == (ECAPACITY, ECAPACITY)
    c.h.synchronize()
    assert bool((out == SENTINEL).all()) and bool((gx0 == SENTINEL).all())
    assert calls(c.h, 3, 1) == (0, 0)  # and the same calls pass once the argument is right
    c.h.synchronize()
    assert torch.equal(out, x_traj) and not bool((gx0 == SENTINEL).any())
    small.close()
    c.h.close()


# ---- 8. diff.plant_rollout ----
def _identification(pkg):
    """A plant of mass 15 and the params' inertia asked to explain the trajectory of one of mass 18
    and a scaled inertia: (case, leaves, x_target)."""
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    c = Case(pkg, (4, 3, 2), ("long", True))
    p = sm.SrbdParams()
    true = capi.Robots(mass=_dev(np.full(c.B, 18.0)), Lbody=_dev(np.tile(np.array(p.Lbody) * (1.2, 0.9, 1.1), (c.B, 1))))
    c.h.set_robots(plant=true)
    x_target = c.forward()
    c.h.synchronize()
    plant = capi.Robots(mass=_dev(np.full(c.B, 15.0)).requires_grad_(), Lbody=_dev(np.tile(p.Lbody, (c.B, 1))).requires_grad_())
    c.h.set_robots(plant=plant)
    leaves = {k: c.t[k].clone().requires_grad_() for k in ("x0", "u", "foot_r", "foot_l", "wrench")}
    return c, plant, leaves, x_target


def test_autograd_is_the_capi_call(pkg):
    import torch
    c, plant, leaves, x_target = _identification(pkg)
    x_traj = pkg.diff.plant_rollout(c.h, substeps=c.substeps, **leaves)
    loss = ((x_traj - x_target) ** 2).sum()
    loss.backward()
    want = c.backward(x_traj.detach(), gx=(2.0 * (x_traj.detach() - x_target)).contiguous())
    c.h.synchronize()
    got = {**{k: v.grad for k, v in leaves.items()}, "mass": plant.mass.grad, "Lbody": plant.Lbody.grad}
    for name in PV.OUTPUTS:
        g, w = got[name], want[name]
        assert g is not None and float(g.abs().max()) > 0.0, name
        if name in ("foot_r", "foot_l"):  # the long plan's rows past T get zeros
            assert g.shape == leaves[name].shape and not g[:, c.T:].any()
            g = g[:, :c.T]
        assert float((g - w).abs().max()) <= 1e-12 * float(w.abs().max()), name
    # mass 15 against a trajectory of mass 18: descent raises the mass
    assert bool((plant.mass.grad < 0.0).all()), plant.mass.grad
    c.h.close()


def test_autograd_raises_after_a_role_was_replaced(pkg):
    c, plant, leaves, x_target = _identification(pkg)
    loss = ((pkg.diff.plant_rollout(c.h, substeps=c.substeps, **leaves) - x_target) ** 2).sum()
    c.h.set_robots(plant=pkg.capi.Robots(mass=plant.mass.detach().clone()))
    with pytest.raises(RuntimeError, match="robots were replaced"):
        loss.backward()
    c.h.close()
