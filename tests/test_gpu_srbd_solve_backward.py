"""srbd_qp_srbd_solve_backward_f64 on the device: the fused backward pass against
the two chained device calls it replaces (same handle, same forward solution), against its numpy
statement tests/srbd_solve_vjp_host.py, the call's contract (single outputs, writes, determinism,
handle reuse, the compact buffer, alignment, side effects, argument checks) and diff.srbd_solve
through autograd.  The forward solve is the handle's own at the tight settings of
tests/test_gpu_linearize_backward.py.  Inputs: tests/linearize_backward_cases.py."""
import ctypes as C

import numpy as np
import pytest

import linearize_backward_cases as LC
import robots_host as BH
import srbd_solve_vjp_host as SH
import test_gpu_linearize_backward as LB
from srbd_device import _dev, device_plan, device_robots, handle

pytestmark = pytest.mark.gpu

CHAIN_BOUND = 1e-9      # per output: |fused - chain| <= CHAIN_BOUND max|chain|
STATEMENT_BOUND = 1e-8  # per output: |fused - statement| <= STATEMENT_BOUND max|statement|
E2E_ST, ACT_TOL, RANK_TOL = LB.E2E_ST, LB.ACT_TOL, LB.RANK_TOL
CONFIGS, ALL_ROBOT, ALL_PLAN = LB.CONFIGS, LB.ALL_ROBOT, LB.ALL_PLAN
OUTPUTS = SH.OUTPUTS
SENTINEL = -777.25
MODES = ["none", "box_u", "cone"]
NINE = ("A", "B", "b", "Q", "S", "R", "q", "r", "x0")
ROWS = {"none": (), "box_u": ("lbu", "ubu"), "cone": ("D", "lg", "ug")}


def make_case(sm, B, N, robots, plan):
    """linearize_backward_cases.make_case; a shape it has no seed for (257 robots: some row of some
    stage is always within the margin of the barrier's switch) is drawn the same way without the
    margins, which matter to finite differences only: both device paths take the same branch."""
    if (B, N) in LC.SEEDS:
        return LC.make_case(sm, B, N, robots=robots, plan=plan)
    p = sm.SrbdParams()
    xs, us, _ = sm.sample_trajectories(B, N, 7000, p)
    params = BH.only(p, BH.draw(p, B, 8000), robots)
    return p, params, (LC.case_plan(sm, p, B, N, 9000, plan) if plan else None), xs, us


class Setup:
    """A case on the device: its linearisation, the handle's forward solve of it, the cotangents of
    loss = sum x^2 + sum u^2, and the two backward paths on that one handle."""

    def __init__(self, pkg, B, N, constraints, config="robots+plan", capacity=None, batch=None):
        import torch
        self.torch, self.pkg, self.capi, self.constraints = torch, pkg, pkg.capi, constraints
        capi, sm = pkg.capi, pkg.srbd_model
        robots, plan = CONFIGS[config]
        self.robot_fields = robots
        self.case = make_case(sm, B, N, robots, plan)
        p, params, pl, xs, us = self.case
        n = B if batch is None else batch
        self.B, self.N = n, N
        _, _, x0 = sm.sample_trajectories(B, N, 4321, p)
        self.h = handle(capi, N, capacity or B, constraints)
        self.h.set_robots(model=device_robots(capi, params[:n], robots) if robots else None)
        self.plan = None
        if pl is not None:
            self.plan = device_plan(capi, sm.SrbdPlan(**{k: (None if getattr(pl, k) is None else getattr(pl, k)[:n])
                                                         for k in ALL_PLAN}))
        self.xs, self.us, self.x0, self.mp = _dev(xs[:n]), _dev(us[:n]), _dev(x0[:n]), capi.model_params(p)
        self.st = capi.settings_struct(E2E_ST)
        self.qp, self.data = capi.srbd_linearize(self.h, self.xs, self.us, constraints, params=self.mp, plan=self.plan)
        self.data.x0 = self.x0.data_ptr()
        new = lambda rows: torch.zeros(n, rows, 12, dtype=torch.float64, device="cuda")
        self.x, self.u, self.pi = new(N + 1), new(N), new(N + 1)
        self.status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.sol = capi.Solution(x=self.x.data_ptr(), u=self.u.data_ptr(), pi=self.pi.data_ptr(),
                                 status=self.status.data_ptr())
        self.h.solve_device(n, self.st, self.data, self.sol)
        self.h.synchronize()
        assert bool((self.status == 0).all()), self.status
        self.gx, self.gu = 2.0 * self.x, 2.0 * self.u

    def chain(self, want=OUTPUTS, gx="own", gu="own"):
        """srbd_qp_solve_backward_rows_f64 (all nine and the rows' gradients), then
        srbd_qp_srbd_linearize_backward_f64: (the outputs and x0, the counts)."""
        torch, capi, n, N = self.torch, self.capi, self.B, self.N
        gx, gu = (self.gx if gx == "own" else gx), (self.gu if gu == "own" else gu)
        like = dict(self.qp, x0=self.x0)
        g = {k: torch.empty_like(like[k]) for k in NINE}
        shapes = {"D": (N, 288), "lg": (N + 1, 24), "ug": (N + 1, 24), "lbu": (N, 12), "ubu": (N, 12)}
        r = {k: torch.empty(n, *shapes[k], dtype=torch.float64, device="cuda") for k in ROWS[self.constraints]}
        self.h.solve_backward_rows_device(n, self.st, self.data, self.sol, gx, gu, capi.Grad(**{k: v.data_ptr() for k, v in g.items()}),
                                          capi.GradRows(**{k: v.data_ptr() for k, v in r.items()}) if r else None,
                                          act_tol=ACT_TOL, rank_tol=RANK_TOL)
        counts = self.h.backward_active(n)
        out = capi.srbd_linearize_backward(self.h, self.xs, self.us, {**g, **r}, self.constraints, params=self.mp,
                                           plan=self.plan, want=want)
        self.h.synchronize()
        out["x0"] = g["x0"]
        return out, counts

    def fused(self, want=OUTPUTS, want_x0=True, gx="own", gu="own", out=None, sol=None, xs=None, us=None):
        gx, gu = (self.gx if gx == "own" else gx), (self.gu if gu == "own" else gu)
        got = self.capi.srbd_solve_backward(self.h, self.xs if xs is None else xs, self.us if us is None else us,
                                            self.data, sol or self.sol, gx, gu, self.constraints, params=self.mp,
                                            plan=self.plan, act_tol=ACT_TOL, rank_tol=RANK_TOL, want=want,
                                            settings=self.st, want_x0=want_x0, out=out)
        counts = self.h.backward_active(self.B)
        self.h.synchronize()
        return got, counts

    def close(self):
        self.h.close()


def compare(got, want, what, bound=CHAIN_BOUND):
    worst = 0.0
    for name, g in got.items():
        w = want[name]
        w = w.cpu().numpy() if hasattr(w, "cpu") else w
        scale = np.abs(w).max()
        err = np.abs(g.cpu().numpy() - w).max()
        print(f"[srbd solve backward] {what} {name}: max|reference| {scale:.3g}, error {err:.2e}")
        assert err <= bound * scale, (what, name, err, scale)
        worst = max(worst, err / scale if scale > 0 else 0.0)
    print(f"[srbd solve backward] {what}: worst relative error {worst:.2e}")
    return worst


def fused_matches_chain(pkg, B, N, constraints, config="robots+plan"):
    import torch
    s = Setup(pkg, B, N, constraints, config)
    want, counts_c = s.chain()
    got, counts_f = s.fused()
    assert set(got) == set(OUTPUTS) | {"x0"}
    assert torch.equal(counts_c, counts_f), (counts_c, counts_f)
    if constraints != "none" and "plan" in config:  # the swing feet's fz_max = 1 is on the active set
        assert int(counts_f[:, :2].sum()) > 0, "no bound or row is active: the constrained path is not exercised"
    compare(got, want, f"({B}, {N}) {constraints} {config}")
    s.close()


# ---- 1. fused against the chained device calls ----
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("constraints", MODES)
def test_fused_matches_the_chained_calls(pkg, constraints, config):
    fused_matches_chain(pkg, 3, 2, constraints, config)


# (5, 13): robot 4 straddles the 64-stage workgroup boundary and QP boundaries fall inside a staged
# chunk; (2, 33): a QP longer than a chunk; (4, 1), (70, 1): N = 1, every stage its own QP
@pytest.mark.parametrize("B,N", [(5, 13), (2, 33), (4, 1), (70, 1)])
@pytest.mark.parametrize("constraints", MODES)
def test_stage_shapes(pkg, constraints, B, N):
    fused_matches_chain(pkg, B, N, constraints)


@pytest.mark.parametrize("constraints", ["none", "cone"])
def test_batch_on_the_streaming_adjoint(pkg, constraints):
    fused_matches_chain(pkg, 257, 2, constraints)


# ---- 2. fused against the statement ----
@pytest.mark.parametrize("constraints", MODES)
def test_fused_matches_the_statement(pkg, OcpQpBatch, constraints):
    B, N = 3, 4
    s = Setup(pkg, B, N, constraints)
    got, counts = s.fused()
    mat = lambda n, rows: np.swapaxes(s.qp[n].cpu().numpy().reshape(B, -1, 12, rows), -1, -2)
    vec = lambda n: s.qp[n].cpu().numpy()
    kw = dict(N=N, nx=12, nu=12, A=mat("A", 12), B=mat("B", 12), b=vec("b"), Q=mat("Q", 12), S=mat("S", 12),
              R=mat("R", 12), q=vec("q"), r=vec("r"))
    if constraints == "box_u":
        kw.update(lbu=vec("lbu"), ubu=vec("ubu"))
    elif constraints == "cone":
        kw.update(ng=24, D=mat("D", 24), lg=vec("lg"), ug=vec("ug"), lg_mask=vec("lg_mask"), ug_mask=vec("ug_mask"))
    qp = OcpQpBatch(**kw)
    x, u, pi, gx, gu = (t.cpu().numpy() for t in (s.x, s.u, s.pi, s.gx, s.gu))
    per = [SH.adjoint_vectors(qp, x[i], u[i], pi[i], gx[i], gu[i], i, ACT_TOL, RANK_TOL) for i in range(B)]
    for i in range(B):
        assert tuple(counts[i].tolist()) == per[i]["counts"], (i, counts[i], per[i]["counts"])
    if constraints != "none":
        assert int(counts[:, :2].sum()) > 0
    vecs = {k: np.array([v[k] for v in per]) for k in ("dx", "du", "dpi", "nu", "dnu", "gubu")}
    vecs.update(x=x, u=u, pi=pi)
    p, params, pl, xs, us = s.case
    want = SH.solve_vjp(pkg.srbd_model, params, xs, us, constraints, vecs, pl)
    compare(got, want, f"statement {constraints}", STATEMENT_BOUND)
    if constraints == "cone":
        assert got["mu"].abs().max() > 0 and got["fz_max"].abs().max() > 0
    s.close()


# ---- 3. each output alone, one cotangent alone, and what is not asked for is not written ----
@pytest.fixture(scope="module")
def cone32(pkg):
    s = Setup(pkg, 3, 2, "cone")
    s.want, _ = s.chain()
    yield s
    s.close()


@pytest.mark.parametrize("name", OUTPUTS + ("x0",))
def test_each_output_alone(cone32, name):
    got, _ = cone32.fused(want=() if name == "x0" else (name,), want_x0=name == "x0")
    assert set(got) == {name}
    compare(got, cone32.want, f"only {name}")


@pytest.mark.parametrize("which", ["gx", "gu"])
def test_one_cotangent_alone(cone32, which):
    kw = dict(gx=None) if which == "gu" else dict(gu=None)
    want, _ = cone32.chain(**kw)
    got, _ = cone32.fused(**kw)
    compare(got, want, f"{which} only")


def test_only_requested_outputs_are_written(cone32):
    import torch
    s, B, N = cone32, 3, 2
    want = ("mass", "Lbody", "x_ref", "foot_r", "x0")
    shapes = {n: (B,) + s.capi._lin_grad_shape(n, N) for n in OUTPUTS}
    shapes["x0"] = (B, 12)
    guard = 32
    total = sum(int(np.prod(sh)) + guard for sh in shapes.values()) + guard
    buf = torch.full((total,), SENTINEL, dtype=torch.float64, device="cuda")
    views, at = {}, guard
    for n, sh in shapes.items():
        views[n] = buf[at:at + int(np.prod(sh))].view(sh)
        at += int(np.prod(sh)) + guard
    got, _ = s.fused(want=want[:-1], want_x0=True, out={n: views[n] for n in want})
    compare(got, s.want, "guarded")
    written = torch.zeros(total, dtype=torch.bool, device="cuda")
    for n in want:
        written[views[n].data_ptr() // 8 - buf.data_ptr() // 8:][:views[n].numel()] = True
    assert torch.all(buf[~written] == SENTINEL), "something outside the requested outputs was written"


# ---- 4. determinism, handle reuse, the compact buffer ----
def test_two_calls_give_equal_outputs(pkg):
    import torch
    s = Setup(pkg, 5, 13, "cone")
    first, _ = s.fused()
    again, _ = s.fused()
    for n in first:
        assert torch.equal(first[n], again[n]), n
    s.close()


@pytest.mark.parametrize("constraints", MODES)
def test_handle_reuse_and_the_compact_buffer(pkg, constraints):
    """Capacity 9, batches 5 and 2 alternating, the chained entry points in between; the handle's
    memory grows on the first fused call by the compact buffer alone, and then no more."""
    import torch
    N, cap = 13, 9
    five = Setup(pkg, 5, N, constraints, capacity=cap)
    want5, _ = five.chain()
    before = five.h.memory_bytes()
    got5, _ = five.fused()
    grown = five.h.memory_bytes() - before
    ng, box = (24 if constraints == "cone" else 0), (12 if constraints == "box_u" else 0)
    assert grown == 8 * cap * N * (2 * ng + box), (grown, constraints)
    compare(got5, want5, f"batch 5 of capacity {cap} {constraints}")
    # the same handle at batch 2 (a robot's gradients do not depend on the others), then the chain, then 5 again
    two = Setup(pkg, 5, N, constraints, batch=2)
    two.h.close()
    two.h = five.h
    two.h.set_robots(model=device_robots(pkg.capi, two.case[1][:2], two.robot_fields))
    got2, _ = two.fused()
    compare(got2, {k: v[:2] for k, v in want5.items()}, f"batch 2 of capacity {cap} {constraints}")
    five.h.set_robots(model=device_robots(pkg.capi, five.case[1], five.robot_fields))
    want_again, _ = five.chain()
    again, _ = five.fused()
    for n in got5:
        assert torch.equal(got5[n], again[n]), n
        assert torch.equal(want5[n], want_again[n]), n
    assert five.h.memory_bytes() - before == grown
    five.close()


# ---- 5. the caller's arrays need only be 8-byte aligned ----
@pytest.mark.parametrize("constraints", ["none", "cone"])
def test_arrays_offset_by_one_double(pkg, constraints):
    import torch
    s = Setup(pkg, 5, 13, constraints)
    want, _ = s.fused()

    def shifted(t):
        flat = torch.empty(t.numel() + 1, dtype=torch.float64, device="cuda")
        view = flat[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 8 and view.is_contiguous()
        return view

    x, u, pi, xs, us = (shifted(t) for t in (s.x, s.u, s.pi, s.xs, s.us))
    sol = s.capi.Solution(x=x.data_ptr(), u=u.data_ptr(), pi=pi.data_ptr())
    got, _ = s.fused(sol=sol, xs=xs, us=us)
    compare(got, want, f"offset views {constraints}")
    s.close()


# ---- 6. no side effects on the calls around it ----
def test_other_calls_are_unaffected(pkg):
    import torch
    s = Setup(pkg, 3, 2, "cone")
    lin_before, _ = s.capi.srbd_linearize(s.h, s.xs, s.us, "cone", params=s.mp, plan=s.plan)
    chain_before, counts_before = s.chain()
    x, u, pi = s.x.clone(), s.u.clone(), s.pi.clone()
    s.fused()
    lin_after, _ = s.capi.srbd_linearize(s.h, s.xs, s.us, "cone", params=s.mp, plan=s.plan)
    chain_after, counts_after = s.chain()
    for k in lin_before:
        assert torch.equal(lin_before[k], lin_after[k]) and torch.equal(lin_before[k], s.qp[k]), k
    for k in chain_before:
        assert torch.equal(chain_before[k], chain_after[k]), k
    assert torch.equal(counts_before, counts_after)
    assert torch.equal(x, s.x) and torch.equal(u, s.u) and torch.equal(pi, s.pi)
    s.close()


# ---- 7. diff.srbd_solve ----
class FusedChain(LB.Chain):
    """robots / plan -> diff.srbd_solve -> loss = sum u^2 + x^2 on the device."""

    def __init__(self, pkg, constraints, grad=True):
        super().__init__(pkg, constraints, grad)
        self.x0.requires_grad_(grad)
        self.leaves["x0"] = self.x0

    def forward(self):
        x, u, pi = self.pkg.diff.srbd_solve(self.h, self.xs, self.us, self.x0, self.constraints, params=self.mp,
                                            plan=self.plan, settings=self.st, act_tol=ACT_TOL, rank_tol=RANK_TOL)
        return x, u, pi, (u * u).sum() + (x * x).sum()


@pytest.mark.parametrize("constraints", MODES)
def test_autograd_matches_the_two_functions(pkg, constraints):
    twin = LB.Chain(pkg, constraints)
    twin.x0.requires_grad_(True)
    twin.leaves["x0"] = twin.x0
    twin.forward()[-1].backward()
    twin.h.synchronize()
    ch = FusedChain(pkg, constraints)
    x, u, pi, loss = ch.forward()
    assert not pi.requires_grad
    loss.backward()
    ch.h.synchronize()
    worst = 0.0
    for name, leaf in ch.leaves.items():
        want = twin.leaves[name].grad.cpu().numpy()
        scale = np.abs(want).max()
        err = np.abs(leaf.grad.cpu().numpy() - want).max()
        print(f"[srbd solve backward] autograd {constraints} {name}: max|chain| {scale:.3g}, error / max "
              f"{err / scale if scale > 0 else 0.0:.2e}")
        assert err <= CHAIN_BOUND * scale, (name, err, scale)
        worst = max(worst, err / scale if scale > 0 else 0.0)
    print(f"[srbd solve backward] autograd {constraints}: worst {worst:.2e}")
    twin.h.close()
    ch.h.close()


def test_autograd_none_against_differences_of_the_device_chain(pkg):
    """The probes, the step (relative 1e-4, absolute at a zero) and the bound (1e-6 of the array's
    largest gradient) of test_end_to_end_none_against_differences_of_the_device_chain."""
    import torch
    ch = FusedChain(pkg, "none")
    ch.forward()[-1].backward()
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
                print(f"[srbd solve backward] differences none {name}{idx}: autograd {grad[idx]:.6e}, differences "
                      f"{fd:.6e}, error / max|grad| {err / scale:.2e}")
                assert err <= 1e-6 * scale, (name, idx, grad[idx], fd, scale)
                worst = max(worst, err / scale)
    print(f"[srbd solve backward] differences none: worst {worst:.2e}")
    ch.h.close()


def test_backward_raises_after_the_robots_were_replaced(pkg):
    ch = FusedChain(pkg, "none")
    *_, loss = ch.forward()
    ch.h.set_robots(model=device_robots(pkg.capi, ch.case[1]))
    with pytest.raises(RuntimeError, match="robots were replaced"):
        loss.backward()
    ch.h.close()


# ---- 8. argument checks: the header's order, one case per code, nothing written ----
def test_argument_checks_write_nothing(pkg):
    import torch
    capi = pkg.capi
    L = capi.lib()
    s = Setup(pkg, 3, 2, "cone")
    mass = torch.full((3,), SENTINEL, dtype=torch.float64, device="cuda")
    gx0 = torch.full((3, 12), SENTINEL, dtype=torch.float64, device="cuda")
    grad, none = capi.LinGrad(mass=mass.data_ptr()), capi.LinGrad()
    plan_ref = capi._plan_ref(s.plan, 3, 2, s.xs.device)
    last = lambda: L.srbd_qp_last_error().decode()

    def call(h=s.h.ptr, batch=3, st=s.st, params=s.mp, constraints=2, xs=s.xs.data_ptr(), data=s.data, gx=s.gx.data_ptr(),
             act_tol=ACT_TOL, rank_tol=RANK_TOL, grad=grad, gx0=gx0.data_ptr()):
        ref = lambda v: None if v is None else C.byref(v)
        return L.srbd_qp_srbd_solve_backward_f64(h, batch, ref(st), ref(params), plan_ref, constraints, C.c_void_p(xs),
                                                 C.c_void_p(s.us.data_ptr()), ref(data), C.byref(s.sol), C.c_void_p(gx),
                                                 C.c_void_p(s.gu.data_ptr()), C.c_double(act_tol), C.c_double(rank_tol),
                                                 C.byref(grad), C.c_void_p(gx0), None)

    # 1. the linearisation's: NULL (before everything), EDIM, ECAPACITY, the mode
    assert call(xs=None, batch=99, st=None) == -1 and "NULL argument" in last()
    h13 = capi.Handle(2, 12, 11, 0, False, False, capacity=3)
    assert call(h=h13.ptr, batch=99, st=None) == -2
    h13.close()
    assert call(batch=4, st=None) == -5
    assert call(constraints=3, st=None) == -1 and "constraints" in last()
    plain = handle(capi, 2, 3, "none")
    assert call(h=plain.ptr, st=None) == -1 and "ng = 24" in last()
    plain.close()
    # 2. the solve's: a NULL struct, the tolerances, the settings, the data
    assert call(st=None, act_tol=-1.0) == -1 and "settings is NULL" in last()
    assert call(act_tol=-1.0, rank_tol=2.0) == -1 and "act_tol" in last()
    assert call(rank_tol=2.0) == -1 and "rank_tol" in last()
    assert call(st=capi.settings_struct(dict(E2E_ST, reg_prim=-1.0))) == -6
    no_d = capi.Data.from_buffer_copy(s.data)
    no_d.D = None
    assert call(data=no_d, grad=none, gx0=None) == -1 and "D, lg and ug" in last()
    # 3. no output at all, before 4. batch == 0
    assert call(batch=0, grad=none, gx0=None) == -1 and "grad" in last()
    assert call(batch=0) == 0
    s.h.synchronize()
    assert bool((mass == SENTINEL).all()) and bool((gx0 == SENTINEL).all())
    # and the call they guard works
    assert call() == 0
    s.h.synchronize()
    want, _ = s.chain(want=("mass",))
    compare({"mass": mass, "x0": gx0}, want, "after the checks")
    s.close()
