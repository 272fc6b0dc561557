"""srbd_qp_srbd_linearize_backward_f64 on the device against its numpy statement
tests/linearize_vjp_host.py (itself held to finite differences on the CPU), the call's contract
(outputs, NULL arguments, determinism, scratch reuse), and the chain robots / plan -> linearise ->
solve -> loss through autograd.  Inputs: tests/linearize_backward_cases.py (margins asserted)."""
import numpy as np
import pytest

import adjoint_rows_host as arh
import linearize_backward_cases as LC
import linearize_vjp_host as VH
import robots_host as BH
from srbd_device import _dev, device_plan, device_robots, handle

pytestmark = pytest.mark.gpu

KERNEL_BOUND = 1e-9  # per output array: |kernel - statement| <= KERNEL_BOUND max|statement|
ALL_ROBOT, ALL_PLAN = BH.MODEL_FIELDS, LC.PLAN_FIELDS
CONFIGS = {"robots+plan": (ALL_ROBOT, ALL_PLAN), "robots": (ALL_ROBOT, ()), "plan": ((), ALL_PLAN), "neither": ((), ())}
SENTINEL = -777.25
_statement = {}


def statement(sm, B, N, constraints, robots, plan, only=None):
    """(case, cotangents, the numpy statement's ten gradients), computed once per case."""
    key = (B, N, constraints, tuple(robots), tuple(plan), None if only is None else tuple(only))
    if key not in _statement:
        case = LC.make_case(sm, B, N, robots=robots, plan=plan)
        p, params, pl, xs, us = case
        cot = LC.cotangents(B, N, constraints, 5, only)
        _statement[key] = (case, cot, VH.linearize_vjp(sm, params, xs, us, constraints, cot, pl))
    return _statement[key]


def device_call(pkg, case, cot, constraints, robots, want=VH.OUTPUTS, h=None, batch=None, out=None):
    """The device call on the first `batch` robots of the case; returns (outputs, handle)."""
    capi = pkg.capi
    p, params, pl, xs, us = case
    n = xs.shape[0] if batch is None else batch
    h = h or handle(capi, us.shape[1], n, constraints)
    h.set_robots(model=device_robots(capi, params[:n], robots) if robots else None)
    plan_t = None
    if pl is not None:
        plan_t = device_plan(capi, pkg.srbd_model.SrbdPlan(**{k: (None if getattr(pl, k) is None else getattr(pl, k)[:n])
                                                              for k in ALL_PLAN}))
    got = capi.srbd_linearize_backward(h, _dev(xs[:n]), _dev(us[:n]), {k: _dev(v[:n]) for k, v in cot.items()},
                                       constraints, params=capi.model_params(p), plan=plan_t, want=want, out=out)
    h.synchronize()
    return got, h


def compare(got, want, what, rows=None):
    worst = 0.0
    for name, g in got.items():
        w = want[name] if rows is None else want[name][:rows]
        scale = np.abs(w).max()
        err = np.abs(g.cpu().numpy() - w).max()
        print(f"[linearize backward] {what} {name}: max|statement| {scale:.3g}, error {err:.2e}")
        assert err <= KERNEL_BOUND * scale, (what, name, err, scale)
        worst = max(worst, err / scale if scale > 0 else 0.0)
    return worst


def check(pkg, B, N, constraints, robots, plan, what, want=VH.OUTPUTS, only=None):
    case, cot, ref = statement(pkg.srbd_model, B, N, constraints, robots, plan, only)
    got, h = device_call(pkg, case, cot, constraints, robots, want)
    assert set(got) == set(want)
    worst = compare(got, ref, what)
    h.close()
    return worst


# ---- 1. (3, 2): one partly filled wave; every mode, with and without robots and plan ----
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("constraints", ["none", "box_u", "cone"])
def test_kernel_matches_the_statement(pkg, constraints, config):
    """Seen over the twelve cases: worst |kernel - statement| / max|statement| 5e-15 (8e-15 over
    every kernel test of this file, on Lbody at (4, 1))."""
    robots, plan = CONFIGS[config]
    check(pkg, 3, 2, constraints, robots, plan, f"(3, 2) {constraints} {config}")


# ---- 2. the stage shapes: (5, 13) robot 4 straddles the 64-stage workgroup boundary; (2, 33) more
# stages than a 32-lane group; (4, 1) N = 1; (70, 1) more robots than one workgroup's stages ----
@pytest.mark.parametrize("B,N", [(5, 13), (2, 33), (4, 1), (70, 1)])
def test_stage_shapes(pkg, B, N):
    check(pkg, B, N, "cone", ALL_ROBOT, ALL_PLAN, f"({B}, {N}) cone")


# ---- 3. partial requests on (3, 2) cone ----
@pytest.mark.parametrize("name", VH.OUTPUTS)
def test_each_output_alone(pkg, name):
    check(pkg, 3, 2, "cone", ALL_ROBOT, ALL_PLAN, f"only {name}", want=(name,))


@pytest.mark.parametrize("only", [("b",), ("D", "lg")])
def test_partial_cotangents(pkg, only):
    check(pkg, 3, 2, "cone", ALL_ROBOT, ALL_PLAN, f"cot {only}", only=only)


def test_partial_plan_and_partial_robots(pkg):
    """NULL fields of the plan and of the robots fall back to params."""
    check(pkg, 3, 2, "cone", ("mass", "Q"), ("x_ref", "fz_max"), "partial")
    check(pkg, 3, 2, "box_u", ("Lbody", "mu", "R"), ("foot_l",), "partial")


# ---- 4. what is not asked for is not written ----
def test_only_requested_outputs_are_written(pkg):
    import torch
    B, N = 3, 2
    case, cot, ref = statement(pkg.srbd_model, B, N, "cone", ALL_ROBOT, ALL_PLAN)
    want = ("mass", "Lbody", "x_ref", "foot_r")
    shapes = {n: (B,) + pkg.capi._lin_grad_shape(n, N) for n in VH.OUTPUTS}
    guard = 32
    total = sum(int(np.prod(s)) + guard for s in shapes.values()) + guard
    buf = torch.full((total,), SENTINEL, dtype=torch.float64, device="cuda")
    views, at = {}, guard
    for n, s in shapes.items():
        views[n] = buf[at:at + int(np.prod(s))].view(s)
        at += int(np.prod(s)) + guard
    got, h = device_call(pkg, case, cot, "cone", ALL_ROBOT, want, out={n: views[n] for n in want})
    compare(got, ref, "guarded")
    written = torch.zeros(total, dtype=torch.bool, device="cuda")
    for n in want:
        written[views[n].data_ptr() // 8 - buf.data_ptr() // 8:][:views[n].numel()] = True
    assert torch.all(buf[~written] == SENTINEL), "something outside the requested outputs was written"
    h.close()


# ---- 5. the same inputs give the same bits ----
def test_two_calls_give_equal_outputs(pkg):
    import torch
    case, cot, _ = statement(pkg.srbd_model, 5, 13, "cone", ALL_ROBOT, ALL_PLAN)
    first, h = device_call(pkg, case, cot, "cone", ALL_ROBOT)
    again, _ = device_call(pkg, case, cot, "cone", ALL_ROBOT, h=h)
    for n in VH.OUTPUTS:
        assert torch.equal(first[n], again[n]), n
    h.close()


# ---- 6. batch < capacity, and two batch sizes alternating on one handle (the scratch is reused) ----
def test_batch_below_capacity_and_alternating_batches(pkg):
    import torch
    case, cot, ref = statement(pkg.srbd_model, 5, 13, "box_u", ALL_ROBOT, ALL_PLAN)
    h = handle(pkg.capi, 13, 9, "box_u")
    # a robot's gradients do not depend on the others: the first n rows of the statement
    five, _ = device_call(pkg, case, cot, "box_u", ALL_ROBOT, h=h)
    compare(five, ref, "batch 5 of capacity 9")
    two, _ = device_call(pkg, case, cot, "box_u", ALL_ROBOT, h=h, batch=2)
    compare(two, ref, "batch 2 of capacity 9", rows=2)
    again, _ = device_call(pkg, case, cot, "box_u", ALL_ROBOT, h=h)
    for n in VH.OUTPUTS:
        assert torch.equal(five[n], again[n]), n
    assert h.memory_bytes() >= 9 * 13 * 6 * 8  # the scratch belongs to the handle and is counted
    h.close()


# ---- 7. the forward call is unaffected ----
def test_forward_is_unaffected(pkg):
    import torch
    capi = pkg.capi
    case, cot, _ = statement(pkg.srbd_model, 3, 2, "cone", ALL_ROBOT, ALL_PLAN)
    p, params, pl, xs, us = case
    h = handle(capi, 2, 3, "cone")
    h.set_robots(model=device_robots(capi, params, ALL_ROBOT))
    xs_t, us_t, plan_t, mp = _dev(xs), _dev(us), device_plan(capi, pl), capi.model_params(p)
    before, _ = capi.srbd_linearize(h, xs_t, us_t, "cone", params=mp, plan=plan_t)
    h.synchronize()
    device_call(pkg, case, cot, "cone", ALL_ROBOT, h=h)
    after, _ = capi.srbd_linearize(h, xs_t, us_t, "cone", params=mp, plan=plan_t)
    h.synchronize()
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k], after[k]), k
    h.close()


# ---- 8-10. end to end through autograd ----
E2E_B, E2E_N = 3, 4
# the backward pass's settings for SRBD data (tests/test_gpu_backward_rows.py): tight tolerances so
# that the active sets are beyond doubt, no regularisation (the statements have none), ric_alg = 0
E2E_ST = dict(mode="Speed", iter_max=100, alpha_min=1e-8, mu0=1e2, tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8,
              tol_comp=1e-8, reg_prim=0.0, warm_start=0, pred_corr=1, ric_alg=0, split_step=1)
ACT_TOL, RANK_TOL = 1e-4, 1e-8


class Chain:
    """robots / plan -> diff.srbd_linearize -> diff.solve_qp -> loss = sum u^2 + x^2 on the device."""

    def __init__(self, pkg, constraints, grad=True):
        import torch
        self.pkg, self.constraints = pkg, constraints
        capi, sm = pkg.capi, pkg.srbd_model
        self.case = LC.make_case(sm, E2E_B, E2E_N)
        p, params, pl, xs, us = self.case
        _, _, x0 = sm.sample_trajectories(E2E_B, E2E_N, 4321, p)
        self.h = handle(capi, E2E_N, E2E_B, constraints)
        self.robots, self.plan = device_robots(capi, params), device_plan(capi, pl)
        self.leaves = {n: getattr(self.robots, n) for n in ALL_ROBOT}
        self.leaves.update({n: getattr(self.plan, n) for n in ALL_PLAN})
        for t in self.leaves.values():
            t.requires_grad_(grad)
        self.h.set_robots(model=self.robots)
        self.xs, self.us, self.x0, self.mp = _dev(xs), _dev(us), _dev(x0), capi.model_params(p)
        self.st = capi.settings_struct(E2E_ST)
        self.torch = torch

    def forward(self):
        diff = self.pkg.diff
        qp = diff.srbd_linearize(self.h, self.xs, self.us, self.constraints, params=self.mp, plan=self.plan)
        extra = {k: qp[k] for k in ("lbu", "ubu", "D", "lg", "ug", "lg_mask", "ug_mask") if k in qp}
        x, u, pi = diff.solve_qp(self.h, qp["A"], qp["B"], qp["b"], qp["Q"], qp["S"], qp["R"], qp["q"], qp["r"],
                                 self.x0, settings=self.st, act_tol=ACT_TOL, rank_tol=RANK_TOL, **extra)
        return qp, x, u, pi, (u * u).sum() + (x * x).sum()


def test_end_to_end_none_against_differences_of_the_device_chain(pkg):
    """mass, Lbody, Q, R, foot_r, x_ref gradients of the loss through both backward passes against
    central differences of the same device forward chain, one parameter of one robot at a time.
    Step: relative 1e-4 (absolute at a zero): the loss is smooth here, so the truncation error is a
    relative 1e-8 while the loss's rounding error, 1e-16 / 1e-4, stays below it.
    Bound: 1e-6 of the array's largest gradient.  Seen: 5.8e-8 (worst, on Q[1][3]; the others 1e-8 or less)."""
    import torch
    ch = Chain(pkg, "none")
    *_, loss = ch.forward()
    loss.backward()
    ch.h.synchronize()
    probes = {"mass": [(0,), (2,)], "Lbody": [(0, 0), (1, 2), (2, 1)], "Q": [(0, 11), (1, 3), (2, 11)],
              "R": [(1,), (2,)], "foot_r": [(0, 0, 2), (1, 3, 0), (2, 1, 1)], "x_ref": [(0, 1, 11), (1, 4, 8), (2, 0, 6)]}
    worst = 0.0
    with torch.no_grad():
        for name, entries in probes.items():
            leaf = ch.leaves[name]
            grad = leaf.grad.cpu().numpy()
            scale = np.abs(grad).max()
            assert scale > 0.0, name
            for idx in entries:
                v0 = float(leaf[idx])
                hstep = 1e-4 * abs(v0) if v0 != 0.0 else 1e-4
                vals = []
                for sgn in (1.0, -1.0):
                    leaf[idx] = v0 + sgn * hstep
                    vals.append(float(ch.forward()[-1]))
                leaf[idx] = v0
                fd = (vals[0] - vals[1]) / (2.0 * hstep)
                err = abs(grad[idx] - fd)
                print(f"[linearize backward] end to end none {name}{idx}: autograd {grad[idx]:.6e}, differences {fd:.6e}, "
                      f"error / max|grad| {err / scale:.2e}")
                assert err <= 1e-6 * scale, (name, idx, grad[idx], fd, scale)
                worst = max(worst, err / scale)
    ch.h.close()


@pytest.mark.parametrize("constraints", ["box_u", "cone"])
def test_end_to_end_constrained_against_the_two_statements(pkg, OcpQpBatch, constraints):
    """The autograd result against adjoint_rows_host (the QP's statement, at the device's forward
    solution) followed by linearize_vjp_host.  Bound: 1e-8 relative, two 1e-9 comparisons
    composed through a solve.  Seen: 1.6e-14 (box_u, x_ref), 1.1e-14 (cone, x_ref).  The swing feet's fz_max = 1
    puts their rows and bounds on the active set, so mu.grad (cone) and fz_max.grad are nonzero."""
    ch = Chain(pkg, constraints)
    qp_t, x, u, pi, loss = ch.forward()
    loss.backward()
    ch.h.synchronize()
    N, B = E2E_N, E2E_B
    mat = lambda n, rows: np.swapaxes(qp_t[n].detach().cpu().numpy().reshape(B, -1, 12, rows), -1, -2)
    vec = lambda n: qp_t[n].detach().cpu().numpy()
    kw = dict(N=N, nx=12, nu=12, A=mat("A", 12), B=mat("B", 12), b=vec("b"), Q=mat("Q", 12), S=mat("S", 12),
              R=mat("R", 12), q=vec("q"), r=vec("r"))
    if constraints == "box_u":
        kw.update(lbu=vec("lbu"), ubu=vec("ubu"))
    else:
        kw.update(ng=24, D=mat("D", 24), lg=vec("lg"), ug=vec("ug"), lg_mask=vec("lg_mask"), ug_mask=vec("ug_mask"))
    qp = OcpQpBatch(**kw)
    xh, uh, pih = (t.detach().cpu().numpy() for t in (x, u, pi))
    cot = {k: [] for k in VH.COTANGENTS[constraints]}
    active = 0
    for i in range(B):
        g, counts = arh.adjoint_rows_host(qp, xh[i], uh[i], pih[i], 2.0 * xh[i], 2.0 * uh[i], i, ACT_TOL, RANK_TOL)
        active += counts[0] + counts[1]
        for k in cot:  # math orientation -> the packed column-major blocks
            cot[k].append(np.swapaxes(g[k], -1, -2) if g[k].ndim == 3 else g[k])
    assert active > 0, "no bound or row is active: the constrained path is not exercised"
    cot = {k: np.ascontiguousarray(np.array(v)) for k, v in cot.items()}
    p, params, pl, xs, us = ch.case
    want = VH.linearize_vjp(pkg.srbd_model, params, xs, us, constraints, cot, pl)
    for name in VH.OUTPUTS:
        got = ch.leaves[name].grad.cpu().numpy()
        scale = np.abs(want[name]).max()
        err = np.abs(got - want[name]).max()
        print(f"[linearize backward] end to end {constraints} {name}: max|statement| {scale:.3g}, error / max {err / scale:.2e}")
        assert err <= 1e-8 * scale, (name, err, scale)
    assert np.abs(ch.leaves["fz_max"].grad.cpu().numpy()).max() > 0.0
    if constraints == "cone":
        assert np.abs(ch.leaves["mu"].grad.cpu().numpy()).max() > 0.0
    ch.h.close()


def test_backward_raises_after_the_robots_were_replaced(pkg):
    ch = Chain(pkg, "none")
    qp = ch.pkg.diff.srbd_linearize(ch.h, ch.xs, ch.us, "none", params=ch.mp, plan=ch.plan)
    p, params, *_ = ch.case
    ch.h.set_robots(model=device_robots(pkg.capi, params))
    with pytest.raises(RuntimeError, match="robots were replaced"):
        (qp["A"].sum() + qp["R"].sum()).backward()
    ch.h.close()
