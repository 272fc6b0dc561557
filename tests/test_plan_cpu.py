"""Plans (srbd_plan_f64: per-robot, per-stage reference, feet and force limits) without a GPU:
the C-ABI's three _plan_ entry points exist and validate, the numpy model with a plan that
repeats SrbdParams' constants is the model without one, the host restatement of the line search
with a plan (tests/nmpc_plan_host.py) is the oracle's when the plan is constant, and a plan
that changes one stage changes that stage's blocks only."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import nmpc_plan_host as PH
import nmpc_linesearch as LS  # oracle/ (test infrastructure)

PLAN_SYMBOLS = ("srbd_qp_srbd_linearize_plan_f64", "srbd_qp_srbd_linesearch_plan_f64",
                "srbd_qp_srbd_nmpc_plan_f64")
EINVAL = -1  # SRBD_QP_EINVAL


def constant_plan(sm, p, B, N):
    """Every robot and stage gets SrbdParams' own values."""
    return sm.SrbdPlan(x_ref=np.tile(np.array(p.x_ref, dtype=np.float64), (B, N + 1, 1)),
                       foot_r=np.tile(np.array(p.foot_r, dtype=np.float64), (B, N, 1)),
                       foot_l=np.tile(np.array(p.foot_l, dtype=np.float64), (B, N, 1)),
                       fz_max=np.full((B, N, 2), float(p.fmax)))


def test_plan_entry_points_are_exported_and_reject_a_null_handle(pkg):
    capi = pkg.capi
    assert set(PLAN_SYMBOLS) <= set(capi.exported_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(PLAN_SYMBOLS) <= exported
    L = capi.lib()
    p, ls, st = capi.default_model_params(), capi.default_linesearch(), capi.settings_struct()
    plan, data = capi.PlanStruct(), capi.Data()
    assert L.srbd_qp_srbd_linearize_plan_f64(None, 1, C.byref(p), C.byref(plan), 0, None, None,
                                             C.byref(data), None) == EINVAL
    assert L.srbd_qp_srbd_linesearch_plan_f64(None, 1, C.byref(p), C.byref(plan), C.byref(ls),
                                              *([None] * 8)) == EINVAL
    assert L.srbd_qp_srbd_nmpc_plan_f64(None, 1, C.byref(p), C.byref(plan), C.byref(ls), C.byref(st),
                                        0, 1, *([None] * 6)) == EINVAL
    assert L.srbd_qp_abi_version() == 12  # additive to ABI 12


def test_plan_holder_checks_its_tensors(pkg):
    import torch
    capi = pkg.capi
    B, N = 3, 5
    ok = capi.Plan(x_ref=torch.zeros(B, N + 1, 12, dtype=torch.float64),
                   fz_max=torch.ones(B, N, 2, dtype=torch.float64))
    ps = ok.struct(B, N)
    assert ps.x_ref and ps.fz_max and not ps.foot_r and not ps.foot_l
    empty = capi.Plan().struct(B, N)
    assert not (empty.x_ref or empty.foot_r or empty.foot_l or empty.fz_max)
    with pytest.raises(ValueError, match="x_ref has shape"):
        ok.struct(B, N + 1)
    with pytest.raises(ValueError, match="foot_r must be a torch.float64"):
        capi.Plan(foot_r=torch.zeros(B, N, 3, dtype=torch.float32)).struct(B, N)
    with pytest.raises(ValueError, match="foot_l must be contiguous"):
        capi.Plan(foot_l=torch.zeros(B, 3, N, dtype=torch.float64).transpose(1, 2)).struct(B, N)
    with pytest.raises(ValueError, match="fz_max has shape"):
        capi.Plan(fz_max=torch.ones(B, N, 3, dtype=torch.float64)).struct(B, N)


@pytest.mark.parametrize("constraints", ["none", "box_u", "cone"])
def test_constant_plan_is_no_plan_bit_for_bit(pkg, constraints):
    sm = pkg.srbd_model
    B, N = 5, 20
    p = sm.SrbdParams()
    xs, us, _ = sm.sample_trajectories(B, N, 4242, p)
    want, fc0 = sm.build_qp(xs, us, p, constraints)
    got, fc1 = sm.build_qp(xs, us, p, constraints, plan=constant_plan(sm, p, B, N))
    assert np.array_equal(fc0, fc1)
    w, g = want.packed(), got.packed()
    assert w.keys() == g.keys()
    for k in w:
        assert (w[k] is None) == (g[k] is None), k
        if w[k] is not None:
            assert np.array_equal(w[k], g[k]), k


def test_host_line_search_with_a_constant_plan_is_the_oracles(pkg):
    sm = pkg.srbd_model
    B, N, seed = 6, 20, 515
    p = sm.SrbdParams()
    xs, us, _ = sm.sample_trajectories(B, N, seed, p)
    rng = np.random.default_rng(3)
    dx = rng.normal(size=xs.shape) * 0.05
    du = rng.normal(size=us.shape) * 2.0
    alpha0 = np.where(np.arange(B) % 3 == 0, 0.25, 1.0)
    plan = constant_plan(sm, p, B, N)
    Ac, bc = sm.friction_cone(p)
    for i in range(B):
        a = LS._merit(sm, p, xs[i], us[i], N, Ac, bc, True)
        b = PH.merit(sm, p, plan.robot(i), xs[i], us[i], N, Ac, bc)
        assert a[0] == b[0] and a[1] == b[1]
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        want = LS.line_search(sm, p, xs[i], us[i], dx[i], du[i], float(alpha0[i]))
        for pl in (plan.robot(i), None):
            got = PH.line_search(sm, p, pl, xs[i], us[i], dx[i], du[i], float(alpha0[i]))
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])  # accepted point
            assert want[2:7] == got[2:7]  # alpha, phi, theta, dphi, converged
            assert got[7] > 0.0


def _blocks(qp):
    d = qp.packed()
    return {k: v for k, v in d.items() if v is not None}


def test_a_plan_changes_only_its_stages(pkg):
    """One stage's x_ref, another stage's right foot and a third stage's left fz_max: q changes
    on the first, b and B on the second (A = I + dt jfx holds no foot: jfx reads the forces, jfu
    the lever arms), R / r / lg on the third, and nothing else anywhere."""
    sm = pkg.srbd_model
    B, N = 3, 20
    p = sm.SrbdParams()
    xs, us, _ = sm.sample_trajectories(B, N, 99, p)
    base = constant_plan(sm, p, B, N)
    x_ref, foot_r, fz = base.x_ref.copy(), base.foot_r.copy(), base.fz_max.copy()
    kq, kf, kz, rb = 4, 9, 13, 1  # stages, and the robot that gets the changes
    x_ref[rb, kq] += 0.1
    x_ref[rb, N, 6] += 0.2  # the terminal stage's reference too
    foot_r[rb, kf] += [0.1, -0.05, 0.02]
    fz[rb, kz, 1] = 120.0
    plan = sm.SrbdPlan(x_ref=x_ref, foot_r=foot_r, foot_l=base.foot_l, fz_max=fz)
    w = _blocks(sm.build_qp(xs, us, p, "cone")[0])
    g = _blocks(sm.build_qp(xs, us, p, "cone", plan=plan)[0])
    changed = {}
    for k in w:
        diff = w[k].reshape(B, w[k].shape[1], -1) != g[k].reshape(B, g[k].shape[1], -1)
        changed[k] = {(int(r), int(s)) for r, s in zip(*np.nonzero(diff.any(axis=2)))}
    expect = {"q": {(rb, kq), (rb, N)}, "b": {(rb, kf)}, "B": {(rb, kf)},
              "R": {(rb, kz)}, "r": {(rb, kz)}, "lg": {(rb, kz)}}
    for k in w:
        assert changed[k] == expect.get(k, set()), (k, changed[k])
    # A reads the feet through nothing but the force sum: the foot enters B ([p]x) and b only
    assert changed["A"] == set()
    # the box mode caps that foot's fz at min(u_hi, fz_max)
    wb = _blocks(sm.build_qp(xs, us, p, "box_u")[0])
    gb = _blocks(sm.build_qp(xs, us, p, "box_u", plan=plan)[0])
    d = wb["ubu"] != gb["ubu"]
    assert {tuple(int(v) for v in ix) for ix in zip(*np.nonzero(d))} == {(rb, kz, 8)}
    assert gb["ubu"][rb, kz, 8] == 120.0 - us[rb, kz, 8]
    assert np.array_equal(wb["lbu"], gb["lbu"])
