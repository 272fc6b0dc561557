"""Plans on the device (srbd_qp_srbd_{linearize,linesearch,nmpc}_plan_f64: a reference
trajectory, a footstep plan and a contact schedule per robot) against the host restatements:
srbd_model.build_qp(plan=) for the linearisation, tests/nmpc_plan_host.py for the line search
and the SQP loop.  Every robot and stage gets its own seeded plan values."""
import ctypes as C

import numpy as np
import pytest

import nmpc_plan_host as PH
from nmpc_plan_host import NMPC_SEED, constant_plan, random_plan, walking_batch
from srbd_device import NMPC, SQP_MAX_LOOP, _dev, device_plan, handle, host_nmpc, linesearch_matches_host

pytestmark = pytest.mark.gpu


def check_linearize(pkg, B, N, seed, constraints, plan):
    """srbd_linearize(plan) against build_qp(plan), at the tolerances of test_gpu_linearize.py."""
    import torch
    sm = pkg.srbd_model
    p = sm.SrbdParams()
    xs, us, _ = sm.sample_trajectories(B, N, seed, p)
    want = sm.build_qp(xs, us, p, constraints, plan=plan)[0].packed()
    h = handle(pkg.capi, N, B, constraints)
    xs_t, us_t, plan_t = _dev(xs), _dev(us), device_plan(pkg.capi, plan)
    t, _ = pkg.capi.srbd_linearize(h, xs_t, us_t, constraints, plan=plan_t)
    torch.cuda.synchronize()
    for k, v in t.items():
        got = v.cpu().numpy().reshape(want[k].shape)
        scale = max(np.abs(want[k]).max(), 1.0)
        np.testing.assert_allclose(got, want[k], rtol=1e-11, atol=1e-12 * scale, err_msg=k)


def check_linesearch(pkg, B, N, seed, plan):
    """srbd_linesearch(plan) against the host restatement, at the tolerances of
    test_gpu_linesearch.py: merit rtol 1e-9, accepted point 1e-13, alpha exact
    (srbd_device.linesearch_matches_host)."""
    sm = pkg.srbd_model
    p = sm.SrbdParams()
    xs, us, _ = sm.sample_trajectories(B, N, seed, p)
    rng = np.random.default_rng(seed + 1)
    dx = rng.normal(size=xs.shape) * 0.05
    du = rng.normal(size=us.shape) * 2.0
    alpha0 = np.where(np.arange(B) % 3 == 0, 0.25, 1.0)
    h = handle(pkg.capi, N, B, "none")
    xs_t, us_t, dx_t, du_t, al_t = _dev(xs), _dev(us), _dev(dx), _dev(du), _dev(alpha0)
    plan_t = device_plan(pkg.capi, plan)
    merit, conv = pkg.capi.srbd_linesearch(h, xs_t, us_t, dx_t, du_t, al_t, plan=plan_t)
    h.synchronize()
    host = [PH.line_search(sm, p, plan.robot(i), xs[i], us[i], dx[i], du[i], float(alpha0[i])) for i in range(B)]
    linesearch_matches_host(xs, us, xs_t, us_t, al_t, merit, conv, host)


# ---- 1. linearisation parity: 140 stage threads, three 64-thread blocks, the last partial ----
@pytest.mark.parametrize("constraints", ["none", "box_u", "cone"])
def test_linearize_with_a_plan_matches_the_host_model(pkg, constraints):
    sm = pkg.srbd_model
    B, N = 7, 20
    check_linearize(pkg, B, N, 4242, constraints, random_plan(sm, sm.SrbdParams(), B, N, 11))


# ---- 2. line-search parity: N = 33, lane 0 owns stages 0 and 32 ----
def test_linesearch_with_a_plan_matches_the_host(pkg):
    sm = pkg.srbd_model
    B, N = 3, 33
    check_linesearch(pkg, B, N, 515, random_plan(sm, sm.SrbdParams(), B, N, 12))


# ---- 3. a constant plan, a NULL plan and the old entry point give the same bits ----
def test_constant_and_null_plans_are_the_old_entry_points_bit_for_bit(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N = 5, 20
    p = sm.SrbdParams()
    xs, us, dx0 = sm.sample_trajectories(B, N, 31, p)
    rng = np.random.default_rng(32)
    dx = rng.normal(size=xs.shape) * 0.05
    du = rng.normal(size=us.shape) * 2.0
    const_t = device_plan(capi, constant_plan(sm, p, B, N))
    plans = {"old": None, "null": capi.Plan(), "constant": const_t}
    # linearise, every mode
    for constraints in ("none", "box_u", "cone"):
        h = handle(capi, N, B, constraints)
        xs_t, us_t = _dev(xs), _dev(us)
        outs = {}
        for name, pl in plans.items():
            outs[name], _ = capi.srbd_linearize(h, xs_t, us_t, constraints, plan=pl)
        torch.cuda.synchronize()
        # plan == NULL through the _plan_ entry point itself
        raw = {k: torch.empty_like(v) for k, v in outs["old"].items()}
        data = capi.Data(**{k: (raw[k].data_ptr() if k in raw else None) for k in capi.DATA_FIELDS})
        mp = capi.default_model_params()
        torch.cuda.synchronize()
        capi.check(capi.lib().srbd_qp_srbd_linearize_plan_f64(
            h.ptr, B, C.byref(mp), None, capi.SRBD_CONSTRAINTS[constraints], C.c_void_p(xs_t.data_ptr()),
            C.c_void_p(us_t.data_ptr()), C.byref(data), None), "srbd_qp_srbd_linearize_plan_f64")
        h.synchronize()
        outs["null pointer"] = raw
        for name in ("null", "null pointer", "constant"):
            assert outs[name].keys() == outs["old"].keys()
            for k, v in outs["old"].items():
                assert torch.equal(v, outs[name][k]), (constraints, name, k)
    # line search
    h = handle(capi, N, B, "none")
    outs = {}
    for name, pl in plans.items():
        xs_t, us_t, al_t = _dev(xs), _dev(us), _dev(np.ones(B))
        merit, conv = capi.srbd_linesearch(h, xs_t, us_t, _dev(dx), _dev(du), al_t, plan=pl)
        h.synchronize()
        outs[name] = (xs_t, us_t, al_t, merit, conv)
    for name in ("null", "constant"):
        for a, b in zip(outs["old"], outs[name]):
            assert torch.equal(a, b), name
    # the NMPC step
    x0 = xs[:, 0] + dx0
    for constraints in ("none", "box_u"):
        h = handle(capi, N, B, constraints)
        outs = {}
        for name, pl in plans.items():
            xs_t, us_t, al_t = _dev(xs), _dev(us), _dev(np.ones(B))
            it, conv = capi.srbd_nmpc(h, xs_t, us_t, _dev(x0), al_t, constraints, NMPC, SQP_MAX_LOOP,
                                      plan=pl)
            outs[name] = (xs_t, us_t, al_t, it, conv)
        for name in ("null", "constant"):
            for a, b in zip(outs["old"], outs[name]):
                assert torch.equal(a, b), (constraints, name)


# ---- 4. partial plans: the other fields fall back to the model's constants ----
@pytest.mark.parametrize("field", ["x_ref", "fz_max"])
def test_partial_plans(pkg, field):
    sm = pkg.srbd_model
    p = sm.SrbdParams()
    for constraints in ("none", "box_u", "cone"):
        check_linearize(pkg, 7, 20, 4242, constraints, random_plan(sm, p, 7, 20, 13, fields=(field,)))
    check_linesearch(pkg, 3, 33, 515, random_plan(sm, p, 3, 33, 14, fields=(field,)))


# ---- 5. the NMPC step ----
@pytest.mark.parametrize("constraints", ["none", "box_u"])
def test_nmpc_step_with_a_plan_matches_the_host_loop(pkg, oracle, constraints):
    sm = pkg.srbd_model
    B, N = 8, 20
    p = sm.SrbdParams()
    batch = walking_batch(sm, p, B, N, NMPC_SEED)
    xs, us, x0, alpha, plan = batch
    host = host_nmpc(sm, oracle, p, batch, constraints)
    # a condition on the inputs: the host loop takes no decision on a boundary
    assert min(r[5] for r in host) >= 1e-6, [r[5] for r in host]
    assert len({r[3] for r in host}) >= 2, [r[3] for r in host]
    h = handle(pkg.capi, N, B, constraints)
    xs_t, us_t, al_t = _dev(xs), _dev(us), _dev(alpha)
    it_t, cv_t = pkg.capi.srbd_nmpc(h, xs_t, us_t, _dev(x0), al_t, constraints, NMPC, SQP_MAX_LOOP,
                                    plan=device_plan(pkg.capi, plan))
    it, cv, al = it_t.cpu().numpy(), cv_t.cpu().numpy(), al_t.cpu().numpy()
    dxs, dus = xs_t.cpu().numpy(), us_t.cpu().numpy()
    for i, (hx, hu, ha, hit, hcv, _) in enumerate(host):  # as test_gpu_nmpc.py::check
        assert it[i] == hit, (i, it[i], hit)
        assert bool(cv[i]) == hcv, i
        assert al[i] == ha, (i, al[i], ha)
        np.testing.assert_allclose(dxs[i], hx, rtol=1e-7, atol=1e-9, err_msg=str(i))
        np.testing.assert_allclose(dus[i], hu, rtol=1e-7, atol=1e-6, err_msg=str(i))


# ---- 6. the contact schedule does what it says ----
def test_contact_schedule_caps_the_swing_foot(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N = 4, 20
    p = sm.SrbdParams()
    xs, us, x0 = sm.sample_trajectories(B, N, 606, p)
    fz = np.full((B, N, 2), float(p.fmax))
    swing = slice(6, 12)
    fz[:, swing, 1] = 1.0
    plan_t = capi.Plan(fz_max=_dev(fz))
    # the cone's settings in tests/test_gpu_lq.py
    st = dict(iter_max=40, mode="Speed", ric_alg=1, tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8,
              tol_comp=1e-8, lq_fact=2)
    s = capi.settings_struct(st)
    h = handle(capi, N, B, "cone")
    xs_t, us_t, x0_t = _dev(xs), _dev(us), _dev(x0)

    def left_fz_after_one_qp(pl):
        t, data = capi.srbd_linearize(h, xs_t, us_t, "cone", plan=pl)
        data.x0 = x0_t.data_ptr()
        f64 = dict(dtype=torch.float64, device="cuda")
        sol = {"x": torch.zeros(B, N + 1, 12, **f64), "u": torch.zeros(B, N, 12, **f64),
               "pi": torch.zeros(B, N + 1, 12, **f64),
               "status": torch.full((B,), -1, dtype=torch.int32, device="cuda")}
        S = capi.Solution(**{k: (sol[k].data_ptr() if k in sol else None) for k in capi.SOL_FIELDS})
        h.solve_device(B, s, data, S)
        h.synchronize()
        return sol["status"].cpu().numpy() == 0, (us_t + sol["u"])[:, swing, 8].cpu().numpy()

    ok, left = left_fz_after_one_qp(plan_t)
    assert ok.any(), "no QP reached Success with the schedule"
    assert np.all(left[ok] <= 1.0 + s.tol_ineq), left[ok].max()
    ok0, left0 = left_fz_after_one_qp(None)
    assert ok0.any()
    assert not np.all(left0[ok0] <= 1.0 + s.tol_ineq)  # without the plan the foot keeps pushing
