"""Per-robot model and plant parameters on the device (srbd_qp_srbd_set_robots_f64: the MODEL
role is what the controller believes, the PLANT role the true robot) against the host model
called once per robot with that robot's SrbdParams (tests/robots_host.py, tests/rollout_host.py)."""
import dataclasses

import numpy as np
import pytest

import robots_host as BH
import rollout_host as RH
from nmpc_plan_host import NMPC_SEED, random_plan, walking_batch
from rollout_host import feet_plan, start
from srbd_device import (NMPC, SQP_MAX_LOOP, STEP_ATOL_U, STEP_ATOL_X, _dev, caller_loop, close, device_plan,
                         device_robots, handle, host_nmpc, linesearch_matches_host)

pytestmark = pytest.mark.gpu


def check_linearize(pkg, B, N, seed, constraints, params, robots_t, plan=None):
    """srbd_linearize on a handle with the MODEL role set against build_qp per robot, at the
    tolerances of test_gpu_linearize.py.  Returns the device outputs."""
    import torch
    sm = pkg.srbd_model
    xs, us, _ = sm.sample_trajectories(B, N, seed, sm.SrbdParams())
    want = BH.build_qp(sm, params, xs, us, constraints, plan)
    h = handle(pkg.capi, N, B, constraints)
    h.set_robots(model=robots_t)
    plan_t = None if plan is None else device_plan(pkg.capi, plan)
    t, _ = pkg.capi.srbd_linearize(h, _dev(xs), _dev(us), constraints, plan=plan_t)
    torch.cuda.synchronize()
    for k, v in t.items():
        got = v.cpu().numpy().reshape(want[k].shape)
        scale = max(np.abs(want[k]).max(), 1.0)
        np.testing.assert_allclose(got, want[k], rtol=1e-11, atol=1e-12 * scale, err_msg=k)
    return t


def check_linesearch(pkg, B, N, seed, params, robots_t, plan=None):
    """srbd_linesearch on a handle with the MODEL role set against the host line search per
    robot, at the tolerances of test_gpu_plan.check_linesearch."""
    sm = pkg.srbd_model
    xs, us, _ = sm.sample_trajectories(B, N, seed, sm.SrbdParams())
    rng = np.random.default_rng(seed + 1)
    dx = rng.normal(size=xs.shape) * 0.05
    du = rng.normal(size=us.shape) * 2.0
    alpha0 = np.where(np.arange(B) % 3 == 0, 0.25, 1.0)
    h = handle(pkg.capi, N, B, "none")
    h.set_robots(model=robots_t)
    xs_t, us_t, al_t = _dev(xs), _dev(us), _dev(alpha0)
    plan_t = None if plan is None else device_plan(pkg.capi, plan)
    merit, conv = pkg.capi.srbd_linesearch(h, xs_t, us_t, _dev(dx), _dev(du), al_t, plan=plan_t)
    h.synchronize()
    host = BH.line_search(sm, params, plan, xs, us, dx, du, alpha0)
    linesearch_matches_host(xs, us, xs_t, us_t, al_t, merit, conv, host)


# ---- 1. linearisation: 140 stage threads in three 64-thread blocks, the last partial; robots
# share waves and robot 3 (stages 60..79) straddles two ----
@pytest.mark.parametrize("with_plan", [False, True])
@pytest.mark.parametrize("constraints", ["none", "box_u", "cone"])
def test_linearize_with_robots_matches_the_host_model(pkg, constraints, with_plan):
    sm = pkg.srbd_model
    B, N = 7, 20
    p = sm.SrbdParams()
    params = BH.draw(p, B, 101)
    plan = random_plan(sm, p, B, N, 11) if with_plan else None
    t = check_linearize(pkg, B, N, 4242, constraints, params, device_robots(pkg.capi, params), plan)
    if constraints == "cone":  # D (24 x 12, column-major) and lg carry each robot's mu
        D = t["D"].cpu().numpy().reshape(B, N, 12, 24)
        mu = np.array([q.mu for q in params])
        for leg in (0, 1):
            for row in range(4):
                assert np.array_equal(D[:, :, 6 * leg + 2, 12 * leg + row], np.tile(mu[:, None], (1, N)))
        assert len(set(D[:, 0, 2, 0].tolist())) == B


# ---- 2. line search: N = 33, lane 0 owns stages 0 and 32, lane 1 the terminal stage; three
# robots fill one and a half 64-thread blocks ----
@pytest.mark.parametrize("with_plan", [False, True])
def test_linesearch_with_robots_matches_the_host(pkg, with_plan):
    sm = pkg.srbd_model
    B, N = 3, 33
    p = sm.SrbdParams()
    params = BH.draw(p, B, 102)
    plan = random_plan(sm, p, B, N, 12) if with_plan else None
    check_linesearch(pkg, B, N, 515, params, device_robots(pkg.capi, params), plan)


# ---- 3. one field at a time: the other five fall back to the model's constants ----
@pytest.mark.parametrize("field", BH.MODEL_FIELDS)
def test_one_field_at_a_time(pkg, field):
    sm = pkg.srbd_model
    p = sm.SrbdParams()
    params = BH.only(p, BH.draw(p, 7, 103), (field,))
    check_linearize(pkg, 7, 20, 4242, "cone", params, device_robots(pkg.capi, params, (field,)))
    if field in ("mass", "Qf"):
        params = BH.only(p, BH.draw(p, 3, 104), (field,))
        check_linesearch(pkg, 3, 33, 515, params, device_robots(pkg.capi, params, (field,)))


# ---- 4. robots that repeat the model's constants, and a cleared role, are the handle with
# nothing set, bit for bit: the same VALU operations on the same operands, whether an operand
# comes from an SGPR (a kernel argument) or from a VGPR (a load) ----
def test_constant_and_cleared_robots_are_the_plain_handle_bit_for_bit(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N = 5, 20
    p = sm.SrbdParams()
    xs, us, dx0 = sm.sample_trajectories(B, N, 31, p)
    rng = np.random.default_rng(32)
    dx = rng.normal(size=xs.shape) * 0.05
    du = rng.normal(size=us.shape) * 2.0
    const_t = device_robots(capi, [p] * B)
    other_t = device_robots(capi, BH.draw(p, B, 105))

    def variants(h, run):
        """run() on the plain handle, with constant robots, and after a role was set and cleared."""
        outs = {"plain": run()}
        h.set_robots(model=const_t, plant=capi.Robots(mass=const_t.mass, Lbody=const_t.Lbody))
        outs["constant"] = run()
        h.set_robots(model=other_t, plant=capi.Robots(mass=other_t.mass))
        h.set_robots()
        outs["cleared"] = run()
        h.set_robots(model=capi.Robots(), plant=capi.Robots())  # all fields NULL: clear as well
        outs["empty"] = run()
        return outs

    def same(outs, what):
        for name in ("constant", "cleared", "empty"):
            for i, (a, b) in enumerate(zip(outs["plain"], outs[name])):
                assert torch.equal(a, b), (what, name, i)

    # linearise, every mode
    for constraints in ("none", "box_u", "cone"):
        h = handle(capi, N, B, constraints)
        xs_t, us_t = _dev(xs), _dev(us)

        def lin():
            t, _ = capi.srbd_linearize(h, xs_t, us_t, constraints)
            torch.cuda.synchronize()
            return [t[k] for k in sorted(t)]
        same(variants(h, lin), ("linearize", constraints))
    # line search
    h = handle(capi, N, B, "none")

    def ls():
        xs_t, us_t, al_t = _dev(xs), _dev(us), _dev(np.ones(B))
        merit, conv = capi.srbd_linesearch(h, xs_t, us_t, _dev(dx), _dev(du), al_t)
        h.synchronize()
        return xs_t, us_t, al_t, merit, conv
    same(variants(h, ls), "linesearch")
    # the NMPC step
    x0 = xs[:, 0] + dx0
    for constraints in ("none", "box_u"):
        h = handle(capi, N, B, constraints)

        def step():
            xs_t, us_t, al_t = _dev(xs), _dev(us), _dev(np.ones(B))
            it, conv = capi.srbd_nmpc(h, xs_t, us_t, _dev(x0), al_t, constraints, NMPC, SQP_MAX_LOOP)
            return xs_t, us_t, al_t, it, conv
        same(variants(h, step), ("nmpc", constraints))
    # advance
    h = handle(capi, N, B, "none")
    wrench_t = _dev(np.random.default_rng(33).uniform(-20.0, 20.0, size=(B, 6)))

    def adv():
        xs_t, us_t, x_t = _dev(xs), _dev(us), _dev(x0)
        u0 = capi.srbd_advance(h, xs_t, us_t, x=x_t, wrench=wrench_t, substeps=2)
        h.synchronize()
        return xs_t, us_t, x_t, u0
    same(variants(h, adv), "advance")


def test_a_role_persists_across_calls_until_it_is_cleared(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N = 5, 20
    p = sm.SrbdParams()
    xs, us, _ = sm.sample_trajectories(B, N, 31, p)
    h = handle(capi, N, B, "none")
    xs_t, us_t = _dev(xs), _dev(us)

    def lin():
        t, _ = capi.srbd_linearize(h, xs_t, us_t, "none")
        torch.cuda.synchronize()
        return t
    plain = lin()
    h.set_robots(model=device_robots(capi, BH.draw(p, B, 106)))
    first, second = lin(), lin()
    for k in plain:
        assert torch.equal(first[k], second[k]), k
    for k in ("A", "B", "b", "Q", "R", "q", "r"):
        assert not torch.equal(first[k], plain[k]), k
    # rows are read up to the batch: robots with fewer rows are refused before the launch
    h.set_robots(model=device_robots(capi, BH.draw(p, B - 1, 106)))
    with pytest.raises(ValueError, match="robots have 4 rows"):
        lin()
    # the library's own checks
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*role"):  # SRBD_QP_EINVAL
        capi.check(capi.lib().srbd_qp_srbd_set_robots_f64(h.ptr, 2, None), "set_robots")
    import ctypes as C
    rs = capi.RobotsStruct(mu=xs_t.data_ptr())
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*PLANT"):
        capi.check(capi.lib().srbd_qp_srbd_set_robots_f64(h.ptr, 1, C.byref(rs)), "set_robots")
    h4 = capi.Handle(N, 4, 4, capacity=B)
    with pytest.raises(capi.SrbdQpError, match=r"\(-2\)"):  # SRBD_QP_EDIM
        h4.set_robots(model=device_robots(capi, BH.draw(p, B, 106)))
    h.set_robots()
    again = lin()
    for k in plain:
        assert torch.equal(again[k], plain[k]), k


# ---- 5. the NMPC step ----
ROBOTS_SEED = 126  # with NMPC_SEED, on the CPU: margins 1.16e-5 (none), 1.59e-5 (box_u)


@pytest.mark.parametrize("constraints", ["none", "box_u"])
def test_nmpc_step_with_robots_matches_the_host_loop(pkg, oracle, constraints):
    sm = pkg.srbd_model
    B, N = 8, 20
    p = sm.SrbdParams()
    batch = walking_batch(sm, p, B, N, NMPC_SEED)
    xs, us, x0, alpha, plan = batch
    params = BH.draw(p, B, ROBOTS_SEED)
    host = RH.sqp_loops(sm, oracle, params, plan, xs, us, x0, alpha, NMPC, SQP_MAX_LOOP, constraints)
    nominal = host_nmpc(sm, oracle, p, batch, constraints)
    print("host iterations", [r[3] for r in host], "nominal", [r[3] for r in nominal],
          "margin", min(r[5] for r in host))
    # conditions on the inputs: no host decision on a boundary, robots that stop at different
    # iterations, and parameters that change the course of the loop
    assert min(r[5] for r in host) >= 1e-6, [r[5] for r in host]
    assert len({r[3] for r in host}) >= 2, [r[3] for r in host]
    assert [r[3] for r in host] != [r[3] for r in nominal]
    h = handle(pkg.capi, N, B, constraints)
    h.set_robots(model=device_robots(pkg.capi, params))
    xs_t, us_t, al_t = _dev(xs), _dev(us), _dev(alpha)
    it_t, cv_t = pkg.capi.srbd_nmpc(h, xs_t, us_t, _dev(x0), al_t, constraints, NMPC, SQP_MAX_LOOP,
                                    plan=device_plan(pkg.capi, plan))
    it, cv, al = it_t.cpu().numpy(), cv_t.cpu().numpy(), al_t.cpu().numpy()
    dxs, dus = xs_t.cpu().numpy(), us_t.cpu().numpy()
    for i, (hx, hu, ha, hit, hcv, _) in enumerate(host):  # as test_gpu_plan.py's step test
        assert it[i] == hit, (i, it[i], hit)
        assert bool(cv[i]) == hcv, i
        assert al[i] == ha, (i, al[i], ha)
        np.testing.assert_allclose(dxs[i], hx, rtol=1e-7, atol=1e-9, err_msg=str(i))
        np.testing.assert_allclose(dus[i], hu, rtol=1e-7, atol=1e-6, err_msg=str(i))


# ---- 6. advance: lane 0 integrates the true robot, lane 1 the believed one ----
def test_advance_moves_the_plant_with_the_plant_role_and_the_guess_with_the_model_role(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N, substeps = 5, 33, 3
    p = sm.SrbdParams()
    xs, us, x = start(sm, p, B, N, 733)
    plan = feet_plan(sm, p, B, N, 21)
    plan_t = device_plan(capi, plan)
    wrench = np.random.default_rng(22).uniform(-20.0, 20.0, size=(B, 6))
    model = BH.draw(p, B, 140)
    plant = BH.draw_plant(model, 141)
    model_t, plant_t = device_robots(capi, model), device_robots(capi, plant, BH.PLANT_FIELDS)
    h = handle(capi, N, B, "none")

    def advance(w):
        xs_t, us_t, x_t = _dev(xs), _dev(us), _dev(x)
        u0 = capi.srbd_advance(h, xs_t, us_t, x=x_t, plan=plan_t, wrench=None if w is None else _dev(w),
                               substeps=substeps)
        h.synchronize()
        # bit copies
        assert torch.equal(u0, _dev(us[:, 0]))
        assert torch.equal(xs_t[:, :N], _dev(xs[:, 1:]))
        assert torch.equal(us_t[:, :N - 1], _dev(us[:, 1:]))
        assert torch.equal(us_t[:, N - 1], _dev(us[:, N - 1]))
        return xs_t, x_t

    want_xs, _ = RH.shift_guess(sm, model, xs, us, plan)
    # the plant's parameters: the PLANT role, or the MODEL role where the PLANT role has none
    mixed = [dataclasses.replace(m, mass=q.mass) for m, q in zip(model, plant)]
    for what, roles, truth in (("both roles", dict(model=model_t, plant=plant_t), plant),
                               ("model only", dict(model=model_t), model),
                               ("plant mass only", dict(model=model_t, plant=capi.Robots(mass=plant_t.mass)),
                                mixed)):
        h.set_robots(**roles)
        xs_t, x_t = advance(wrench)
        close(x_t, RH.plant_step(sm, truth, x, us[:, 0], plan.foot_r[:, 0], plan.foot_l[:, 0], wrench, substeps),
              (what, "x"))
        close(xs_t[:, N], want_xs[:, N], (what, "xs[N]"))
        # a pure force moves the velocity rows by dt F / the true robot's mass
        force = np.concatenate([np.zeros((B, 3)), wrench[:, 3:]], axis=1)
        dv = (advance(force)[1][:, 9:12] - advance(None)[1][:, 9:12]).cpu().numpy()
        mass = np.array([q.mass for q in truth])
        np.testing.assert_allclose(dv, p.dt * force[:, 3:] / mass[:, None], rtol=1e-12, atol=0.0, err_msg=what)
    # the PLANT role alone: the guess moves with the model's constants
    h.set_robots(plant=plant_t)
    xs_t, x_t = advance(wrench)
    nominal = [p] * B
    truth = [dataclasses.replace(p, mass=q.mass, Lbody=q.Lbody) for q in plant]
    close(x_t, RH.plant_step(sm, truth, x, us[:, 0], plan.foot_r[:, 0], plan.foot_l[:, 0], wrench, substeps),
          "plant only, x")
    close(xs_t[:, N], RH.shift_guess(sm, nominal, xs, us, plan)[0][:, N], "plant only, xs[N]")


# ---- 7. the rollout ----
ROLLOUT_SEED = 30  # as tests/test_gpu_rollout.py; the MODEL role from the draw at 130, the PLANT role at 230
# d_t (the table there): the largest change of the host loop's x_log[t] /
# u_log[t-1] when the loop is rerun with x, xs, us perturbed by relative 1e-7, measured on the CPU
# (scripts/rollout_sensitivity.py --robots --seed 30) per case (constraints, alpha_reset),
# t = 1..4: (d_t of x, d_t of u).
D_T = {
    ("none", 0.0): ((2.8e-07, 5.1e-07, 7.5e-07, 8.7e-07), (1.6e-05, 1.1e-05, 8.3e-06, 6.3e-06)),
    ("none", 1.0): ((2.8e-07, 5.1e-07, 7.5e-07, 8.7e-07), (1.6e-05, 1.1e-05, 8.3e-06, 6.3e-06)),
    ("box_u", 0.0): ((2.9e-07, 5.3e-07, 7.7e-07, 9.0e-07), (1.6e-05, 1.1e-05, 8.4e-06, 6.3e-06)),
    ("box_u", 1.0): ((2.9e-07, 5.3e-07, 7.7e-07, 9.0e-07), (1.6e-05, 1.1e-05, 8.4e-06, 6.3e-06)),
}


@pytest.mark.parametrize("alpha_reset", [0.0, 1.0])
@pytest.mark.parametrize("constraints", ["none", "box_u"])
def test_rollout_with_robots(pkg, oracle, constraints, alpha_reset):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N, T, substeps = 4, 10, 4, 2
    p = sm.SrbdParams()
    xs, us, x, alpha, plan = RH.walking_case(sm, p, B, N, T, ROLLOUT_SEED)
    model = BH.draw(p, B, ROLLOUT_SEED + 100)
    plant = BH.draw_plant(model, ROLLOUT_SEED + 200)
    loop = lambda true: RH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, SQP_MAX_LOOP, constraints, model=model,
                                       plant=true, plan=plan, substeps=substeps, alpha_reset=alpha_reset)
    host = loop(plant)
    # conditions on the inputs: no host decision on a boundary, and a mismatch that matters
    assert host["margin"] >= 1e-6, host["margin"]
    assert np.abs(host["x_log"] - loop(model)["x_log"]).max() > 1e-3
    model_t, plant_t = device_robots(capi, model), device_robots(capi, plant, BH.PLANT_FIELDS)
    plan_t = device_plan(capi, plan)
    # (a) the rollout is the caller's loop over the two entry points on a second handle with the
    # same roles, bit for bit
    h, h2 = handle(capi, N, B, constraints), handle(capi, N, B, constraints)
    for hh in (h, h2):
        hh.set_robots(model=model_t, plant=plant_t)
    a = [_dev(v) for v in (xs, us, x, alpha)]
    logs_a = capi.srbd_rollout(h, *a, T, constraints, NMPC, SQP_MAX_LOOP, plan=plan_t, substeps=substeps,
                               alpha_reset=alpha_reset)
    b = [_dev(v) for v in (xs, us, x, alpha)]
    logs_b = caller_loop(capi, h2, B, N, T, constraints, *b, None, substeps, alpha_reset, plan_t=plan_t)
    names = ("xs", "us", "x", "alpha", "x_log", "u_log", "sqp_iter_log", "converged_log")
    for name, u, v in zip(names, a + list(logs_a), b + list(logs_b)):
        assert bool(torch.isfinite(u.double()).all()), name
        assert torch.equal(u, v), name
    # (b) against the host closed loop
    x_log, u_log, it_log, cv_log = (v.cpu().numpy() for v in logs_a)
    print("sqp_iter device", it_log.tolist(), "host", host["sqp_iter"].tolist())
    for t in range(1, T + 1):
        print(f"tick {t}: max |x_log - host| {np.abs(x_log[:, t] - host['x_log'][:, t]).max():.3e}, "
              f"max |u_log - host| {np.abs(u_log[:, t - 1] - host['u_log'][:, t - 1]).max():.3e}")
    assert np.array_equal(it_log, host["sqp_iter"])
    assert np.array_equal(cv_log, host["converged"])
    assert np.array_equal(a[3].cpu().numpy(), host["alpha"])
    assert np.array_equal(x_log[:, 0], x)
    dt_x, dt_u = D_T[(constraints, alpha_reset)]
    for t in range(1, T + 1):
        # tick 1 is one step: the step test's tolerance; later ticks compound, by at most d_t
        ax = STEP_ATOL_X if t == 1 else max(STEP_ATOL_X, 10.0 * dt_x[t - 1])
        au = STEP_ATOL_U if t == 1 else max(STEP_ATOL_U, 10.0 * dt_u[t - 1])
        np.testing.assert_allclose(x_log[:, t], host["x_log"][:, t], rtol=1e-7, atol=ax, err_msg=f"x {t}")
        np.testing.assert_allclose(u_log[:, t - 1], host["u_log"][:, t - 1], rtol=1e-7, atol=au,
                                   err_msg=f"u {t}")
    assert np.array_equal(a[2].cpu().numpy(), x_log[:, T])
