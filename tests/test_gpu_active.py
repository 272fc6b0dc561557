"""Active sets on the device (srbd_qp_srbd_set_active_f64, srbd_qp_srbd_step_work): a mask, skipping
fallen robots, and compaction of every SQP iteration to the robots that still iterate.

What is compared is device against device, bit for bit: a masked step against the plain step, the
compacted step against the masked one, a rollout with skip_fallen against the caller's own loop and
against the rollout without an active set.  The starts are chosen on the CPU with the host loop
(tests/active_host.py) so that the robots of a batch stop at different SQP iterations, one of them
at SQP_MAX_LOOP, and every test asserts that spread: a batch in which everybody stops together
would pass without showing anything.  step_work shows that compaction happens: with compact its
qp_solves is the sum of the robots' iteration counts."""
import ctypes

import numpy as np
import pytest

import active_host as AH
import contact_host as CH
import gait_host as GH
import robots_host as BH
import rollout_host as RH
from srbd_device import (NMPC, SQP_MAX_LOOP, STEP_ATOL_U, STEP_ATOL_X, _dev, _dev_i32, caller_loop, device_contact,
                         device_gait, device_plan, device_robots, handle)

pytestmark = pytest.mark.gpu

N = 10          # as tests/test_gpu_rollout.py
BASE_SEED = 53  # active_host.base_starts: host counts 8, 13, 1, 5, 7 or 8, 15, 1, 5
MASK7 = (1, 0, 1, 1, 0, 0, 1)
STEP = ("xs", "us", "alpha", "sqp_iter", "converged")

_BASE, _PLAIN = {}, {}


def batch_of(pkg, oracle, constraints, B):
    """(xs, us, x0, alpha) of B robots tiled from the base robots, and the host's iteration count of
    each; the host loops run once per constraints mode."""
    sm = pkg.srbd_model
    if constraints not in _BASE:
        _BASE[constraints] = AH.base_starts(sm, oracle, sm.SrbdParams(), N, BASE_SEED, NMPC, SQP_MAX_LOOP, constraints)
    xs, us, x0, alpha, host = _BASE[constraints]
    base, xs, us, x0, alpha = AH.tiled(B, xs, us, x0, alpha)
    counts = host["sqp_iter"][base]
    assert len(set(counts.tolist())) >= 3 and counts.max() == SQP_MAX_LOOP, counts  # the spread, on the CPU
    return (xs, us, x0, alpha), counts


def run_step(capi, h, start, constraints, active=None, plan=None, settings=NMPC):
    """One srbd_nmpc from `start` on fresh tensors with `active` on the handle: (the tensors,
    step_work)."""
    xs, us, x0, alpha = (_dev(a) for a in start)
    h.set_active(active)
    it, cv = capi.srbd_nmpc(h, xs, us, x0, alpha, constraints, settings, SQP_MAX_LOOP, plan=plan)
    return dict(xs=xs, us=us, alpha=alpha, sqp_iter=it, converged=cv), h.step_work()


def plain(pkg, oracle, constraints, B):
    """The step of a handle that never had an active set, once per (constraints, B)."""
    key = (constraints, B)
    if key not in _PLAIN:
        start, counts = batch_of(pkg, oracle, constraints, B)
        _PLAIN[key] = (start, counts) + run_step(pkg.capi, handle(pkg.capi, N, B, constraints), start, constraints)
    return _PLAIN[key]


def same(got, want, what, rows=None, keys=STEP):
    import torch
    for k in keys:
        u, v = (got[k], want[k]) if rows is None else (got[k][rows], want[k][rows])
        assert bool(torch.isfinite(u.double()).all()), (what, k)
        assert torch.equal(u, v), (what, k)


def spread(it, what, to_the_limit=True):
    """At least three iteration counts on the device, one of them the limit."""
    counts = sorted(set(it.cpu().numpy().tolist()) - {0})
    assert len(counts) >= 3 and (not to_the_limit or counts[-1] == SQP_MAX_LOOP), (what, counts)


def a_mask(B):
    if B == 7:
        return np.array(MASK7, dtype=np.int32)
    return (np.random.default_rng(B).uniform(size=B) < 0.7).astype(np.int32) * 5  # (any non-zero value)


# ---- 1. a mask, full-batch launches ----
@pytest.mark.parametrize("constraints", ["none", "box_u", "cone"])
def test_a_masked_step_steps_the_masked_robots_only(pkg, oracle, constraints):
    import torch
    capi, B = pkg.capi, 7
    start, counts, want, work0 = plain(pkg, oracle, constraints, B)
    spread(want["sqp_iter"], constraints)
    assert work0 == (int(want["sqp_iter"].max()) * B, int(want["sqp_iter"].max()))
    on = torch.tensor(MASK7, device="cuda") != 0
    got, work = run_step(capi, handle(capi, N, B, constraints), start, constraints,
                         capi.Active(mask=_dev_i32(np.array(MASK7))))
    same(got, want, constraints, rows=on)  # active: the bits of the plain step
    for k, a in zip(("xs", "us", "alpha"), (start[0], start[1], start[3])):  # the others: untouched
        assert torch.equal(got[k][~on], _dev(a)[~on]), (constraints, k)
    assert not bool(got["sqp_iter"][~on].any()) and not bool(got["converged"][~on].any())
    its = int(got["sqp_iter"].max())
    assert len(set(got["sqp_iter"][on].cpu().numpy().tolist())) >= 3 and work == (its * B, its), (work, its)


# ---- 2. compaction is the masked step, bit for bit ----
# B = 7: a wave row of the Riccati kernel partly filled, n_it falling through 4 .. 1; B = 130: the
# selection across waves; B = 1030: across its 1024-robot tiles.
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("constraints,B", [("none", 7), ("box_u", 7), ("none", 130), ("box_u", 130), ("none", 1030)])
def test_compaction_is_the_masked_step_bit_for_bit(pkg, oracle, constraints, B, masked):
    capi = pkg.capi
    start, counts = batch_of(pkg, oracle, constraints, B)
    mask = _dev_i32(a_mask(B)) if masked else None
    h = handle(capi, N, B, constraints)
    full, work_full = run_step(capi, h, start, constraints, capi.Active(mask=mask))
    comp, work = run_step(capi, h, start, constraints, capi.Active(mask=mask, compact=True))
    same(comp, full, (constraints, B, masked))
    it = comp["sqp_iter"]
    spread(it, (constraints, B, masked), to_the_limit=not (masked and B == 7))
    print(f"{constraints} B={B} masked={masked}: qp_solves {work[0]} compacted, {work_full[0]} full-batch")
    assert work == (int(it.sum()), int(it.max())), (work, int(it.sum()), int(it.max()))
    assert work_full == (int(it.max()) * B, int(it.max())), work_full
    if masked:
        assert not bool(it[mask == 0].any()) and bool((it[mask != 0] >= 1).all())


# ---- 3. rows follow their robot ----
# ROWS_SEED was chosen on the CPU (seeds 70..81 tried): the host loops' smallest comparison margin
# is 2.0e-6 (none) and 3.7e-6 (box_u), and the robots stop after 5, 6 and 13 iterations.
ROWS_SEED = 77


@pytest.mark.parametrize("constraints", ["none", "box_u"])
def test_rows_follow_their_robot(pkg, oracle, constraints):
    capi, sm = pkg.capi, pkg.srbd_model
    B = 9
    p = sm.SrbdParams()
    xs, us, x0, alpha, plan = RH.walking_case(sm, p, B, N, 1, ROWS_SEED)  # feet and fz_max differ per robot
    params = BH.draw(p, B, ROWS_SEED + 100)                              # mass, Lbody, mu, Q, Qf, R too
    host = AH.step(sm, oracle, params, plan, xs, us, x0, alpha, NMPC, SQP_MAX_LOOP, constraints)
    assert host["margin"] >= 1e-6 and len(set(host["sqp_iter"].tolist())) >= 3, (host["margin"], host["sqp_iter"])
    h = handle(capi, N, B, constraints)
    h.set_robots(model=device_robots(capi, params))
    plan_t = device_plan(capi, plan)
    start = (xs, us, x0, alpha)
    full, _ = run_step(capi, h, start, constraints, None, plan=plan_t)
    comp, work = run_step(capi, h, start, constraints, capi.Active(compact=True), plan=plan_t)
    same(comp, full, constraints)
    assert work == (int(comp["sqp_iter"].sum()), int(comp["sqp_iter"].max()))
    # and the host loop, as the step tests (tests/test_gpu_plan.py test 5)
    assert np.array_equal(comp["sqp_iter"].cpu().numpy(), host["sqp_iter"])
    assert np.array_equal(comp["converged"].cpu().numpy(), host["converged"])
    assert np.array_equal(comp["alpha"].cpu().numpy(), host["alpha"])
    np.testing.assert_allclose(comp["xs"].cpu().numpy(), host["xs"], rtol=1e-7, atol=STEP_ATOL_X)
    np.testing.assert_allclose(comp["us"].cpu().numpy(), host["us"], rtol=1e-7, atol=STEP_ATOL_U)


# ---- 4. edges ----
def test_edges_nobody_one_robot_everybody_and_cleared(pkg, oracle):
    import torch
    capi, B, c = pkg.capi, 7, "none"
    start, counts, want, work0 = plain(pkg, oracle, c, B)
    h = handle(capi, N, B, c)
    for compact in (False, True):
        # nobody: no robot is touched, nothing is solved
        got, work = run_step(capi, h, start, c, capi.Active(mask=_dev_i32(np.zeros(B)), compact=compact))
        for k, a in zip(("xs", "us", "alpha"), (start[0], start[1], start[3])):
            assert torch.equal(got[k], _dev(a)), (compact, k)
        assert not bool(got["sqp_iter"].any()) and not bool(got["converged"].any()) and work == (0, 0)
        # one robot of seven (the one that runs to the limit)
        k = int(np.argmax(counts))
        one = np.zeros(B)
        one[k] = 1
        got, work = run_step(capi, h, start, c, capi.Active(mask=_dev_i32(one), compact=compact))
        rows = torch.tensor(one, device="cuda") != 0
        same(got, want, (compact, "one"), rows=rows)
        assert torch.equal(got["xs"][~rows], _dev(start[0])[~rows]) and not bool(got["sqp_iter"][~rows].any())
        assert work == ((1 if compact else B) * SQP_MAX_LOOP, SQP_MAX_LOOP), work
    # compact with everybody active is the plain step
    got, work = run_step(capi, h, start, c, capi.Active(compact=True))
    same(got, want, "everybody")
    assert work == (int(want["sqp_iter"].sum()), int(want["sqp_iter"].max()))
    # and cleared again: the plain step's bits and work
    for clear in (None, capi.Active()):
        got, work = run_step(capi, h, start, c, clear)
        same(got, want, "cleared")
        assert work == work0


# ---- 5. across the latency IPM's limit (512 QPs) ----
@pytest.mark.parametrize("constraints", ["none", "box_u"])
def test_compaction_across_the_latency_limit(pkg, oracle, constraints):
    capi, B = pkg.capi, 520
    start, counts = batch_of(pkg, oracle, constraints, B)
    # on the CPU: everybody iterates at first, fewer than 512 after the first iteration
    assert (counts >= 1).all() and 0 < int((counts > 1).sum()) < 512 < B, int((counts > 1).sum())
    h = handle(capi, N, B, constraints)
    full, _ = run_step(capi, h, start, constraints, None)
    comp, work = run_step(capi, h, start, constraints, capi.Active(compact=True))
    spread(comp["sqp_iter"], constraints)
    assert work == (int(comp["sqp_iter"].sum()), int(comp["sqp_iter"].max()))
    if constraints == "none":
        same(comp, full, constraints)
        return
    # box_u: the stragglers are solved by another kernel -- the solver's tolerance, not bits
    it_c, it_f = comp["sqp_iter"].cpu().numpy(), full["sqp_iter"].cpu().numpy()
    cv_c, cv_f = comp["converged"].cpu().numpy(), full["converged"].cpu().numpy()
    keep = (it_c == it_f) & (cv_c == cv_f)
    dx = np.abs(comp["xs"].cpu().numpy() - full["xs"].cpu().numpy()).max(axis=(1, 2))
    du = np.abs(comp["us"].cpu().numpy() - full["us"].cpu().numpy()).max(axis=(1, 2))
    print(f"box_u B={B}: robots whose count differs {np.flatnonzero(~keep).tolist()}, "
          f"max |x - x_full| {dx[keep].max():.3e}, max |u - u_full| {du[keep].max():.3e}")
    assert int((~keep).sum()) <= 1, (np.flatnonzero(~keep), it_c[~keep], it_f[~keep])
    assert dx[keep].max() <= STEP_ATOL_X and du[keep].max() <= STEP_ATOL_U, (dx[keep].max(), du[keep].max())


# ---- 6. rollouts with skip_fallen ----
# Chosen on the CPU (the asserts below hold them): with these pushes and this z_min robots 3 and 4
# are below the threshold after tick 0, robots 1 and 6 after tick 1, robots 0, 2, 5, 7 never; every
# height is at least 6e-4 from the threshold.
GAIT_SEED, GAIT_PUSH, GAIT_Z_MIN = 61, 3000.0, 0.97
ROLL_NAMES = ("xs", "us", "x", "alpha", "ref_pose", "foot_now", "x_log", "u_log", "sqp_iter_log", "converged_log",
              "foot_log", "fz_log")


def gait_case(sm):
    B, T = 8, 6
    p = sm.SrbdParams()
    xs, us, x, alpha, gait, cmd, ref_pose, foot_now = GH.walking_case(sm, p, B, N, T, GAIT_SEED)
    wrench = np.zeros((B, T, 6))
    wrench[1, 0, 5] = -GAIT_PUSH
    wrench[4, 0:2, 5] = -0.6 * GAIT_PUSH
    wrench[6, 1:3, 5] = -0.5 * GAIT_PUSH
    contact = sm.SrbdContact(mu=0.5, Lt=(0.0, 0.05, 0.05), fz_hi=400.0, fz_contact=0.5 * (gait.fz_swing + gait.fz_stance),
                             ground_z=gait.ground_z, z_min=GAIT_Z_MIN, cos_tilt_min=0.5)
    return B, T, p, (xs, us, x, alpha, ref_pose, foot_now), gait, cmd, wrench, contact


def state_of(st):
    return {k: v.cpu().numpy() for k, v in st.items()}


def test_gait_rollout_with_skip_fallen(pkg, oracle):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    c = "box_u"
    B, T, p, start, gait, cmd, wrench, contact = gait_case(sm)
    host = AH.closed_loop(sm, oracle, *start[:4], T, NMPC, SQP_MAX_LOOP, c, skip_fallen=True, p=p, gait=gait, cmd=cmd,
                          ref_pose=start[4], foot_now=start[5], wrench=wrench, contact=contact)
    fell = np.where(host["fallen_log"].any(axis=1), host["fallen_log"].argmax(axis=1), T)  # the tick of the fall
    assert (fell < 3).sum() >= 2 and (fell == T).sum() >= 2, fell
    above = np.array([v[0] for v in host["values"]])
    assert np.abs(above - contact.z_min).min() >= 1e-6
    h = handle(capi, N, B, c)
    gait_t, cmd_t, wrench_t = device_gait(capi, gait), _dev(cmd), _dev(wrench)

    def run(active, ticks=T, loop=False):
        ct, st = device_contact(capi, contact, CH.zero_state(B))
        h.set_contact(ct)
        h.set_active(active)
        v = [_dev(w) for w in start]
        if loop:
            logs = caller_loop(capi, h, B, N, ticks, c, *v[:4], wrench_t[:, :ticks].contiguous(), 1, 0.0, gait_t=gait_t,
                               cmd_t=cmd_t, pose=v[4], feet=v[5])
            work = None
        else:
            logs = capi.srbd_rollout_gait(h, gait_t, cmd_t[:, :ticks].contiguous(), *v, ticks, 0, c, NMPC, SQP_MAX_LOOP,
                                          wrench=wrench_t[:, :ticks].contiguous())
            work = h.step_work()
        return dict(zip(ROLL_NAMES, v + list(logs))), state_of(st), work

    skip, st_skip, work_skip = run(capi.Active(skip_fallen=True))
    it_log = skip["sqp_iter_log"].cpu().numpy()
    assert np.array_equal(st_skip["fallen"] != 0, fell < T) and np.array_equal(st_skip["alive"], fell), (st_skip, fell)
    # (a) the caller's own loop on the same handle
    loop, st_loop, _ = run(capi.Active(skip_fallen=True), loop=True)
    same(skip, loop, "caller's loop", keys=ROLL_NAMES)
    assert all(np.array_equal(st_skip[k], st_loop[k]) for k in st_skip)
    # (b) the rollout without an active set
    none, st_none, work_none = run(None)
    stands = torch.from_numpy(fell == T).cuda()
    same(skip, none, "never fallen", rows=stands, keys=ROLL_NAMES)
    assert all(np.array_equal(st_skip[k], st_none[k]) for k in st_skip)
    for i in range(B):
        assert (it_log[i, :fell[i] + 1] >= 1).all() and not it_log[i, fell[i] + 1:].any(), (i, it_log[i])
        assert not skip["converged_log"][i, fell[i] + 1:].any()
    # (full-batch launches: a tick still costs its slowest active robot's iterations x B)
    assert work_skip[0] <= work_none[0] and work_none[0] == work_none[1] * B
    # a fallen robot's guess is only shifted from then on: robots fallen by tick 2, against the
    # same rollout stopped after tick 2 (k more shifts move stage k + m to stage k)
    m = T - 3
    short, _, _ = run(capi.Active(skip_fallen=True), ticks=3)
    down = torch.from_numpy(fell < 3).cuda()
    assert torch.equal(skip["xs"][down][:, :N + 1 - m], short["xs"][down][:, m:])
    assert torch.equal(skip["us"][down][:, :N - m], short["us"][down][:, m:])
    assert torch.equal(skip["alpha"][down], short["alpha"][down])
    # (c) with compaction
    comp, st_comp, work = run(capi.Active(skip_fallen=True, compact=True))
    same(comp, skip, "compact", keys=ROLL_NAMES)
    assert all(np.array_equal(st_comp[k], st_skip[k]) for k in st_skip)
    assert work[0] == int(it_log.sum()) and work[1] == int(it_log.max(axis=0).sum()) == work_skip[1], (work, work_skip)
    assert work_skip[0] == work_skip[1] * B and work[0] < work_skip[0]


# The plan rollout: tests/test_gpu_contact.py's case (robot 4 is below the threshold after the first
# tick, robot 3 after the second, the others stand).
def test_plan_rollout_with_skip_fallen(pkg, oracle):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, n, T, c = 5, 5, 3, "none"
    p = sm.SrbdParams()
    xs, us, x, alpha, plan = RH.walking_case(sm, p, B, n, T, 39)
    contact = sm.SrbdContact(mu=0.05, Lt=(0.0, 0.05, 0.05), fz_hi=400.0, fz_contact=5.0, z_min=1.0032, cos_tilt_min=0.5)
    host = AH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, SQP_MAX_LOOP, c, skip_fallen=True, p=p, plan=plan,
                          contact=contact, alpha_reset=1.0)
    fell = np.where(host["fallen_log"].any(axis=1), host["fallen_log"].argmax(axis=1), T)
    assert (fell < T - 1).any() and (fell == T).sum() >= 2, fell
    h = handle(capi, n, B, c)
    plan_t = device_plan(capi, plan)
    names = ("xs", "us", "x", "alpha", "x_log", "u_log", "sqp_iter_log", "converged_log")

    def run(active, loop=False):
        ct, st = device_contact(capi, contact, CH.zero_state(B))
        h.set_contact(ct)
        h.set_active(active)
        v = [_dev(w) for w in (xs, us, x, alpha)]
        if loop:
            logs = caller_loop(capi, h, B, n, T, c, *v, None, 1, 1.0, plan_t=plan_t)
        else:
            logs = capi.srbd_rollout(h, *v, T, c, NMPC, SQP_MAX_LOOP, plan=plan_t, alpha_reset=1.0)
        return dict(zip(names, v + list(logs))), state_of(st), h.step_work()

    skip, st_skip, work_skip = run(capi.Active(skip_fallen=True))
    it_log = skip["sqp_iter_log"].cpu().numpy()
    assert np.array_equal(st_skip["alive"], fell), (st_skip, fell)
    assert np.array_equal(it_log, host["sqp_iter"]), (it_log, host["sqp_iter"])
    loop, st_loop, _ = run(capi.Active(skip_fallen=True), loop=True)
    same(skip, loop, "caller's loop", keys=names)
    none, st_none, _ = run(None)
    same(skip, none, "never fallen", rows=torch.from_numpy(fell == T).cuda(), keys=names)
    assert all(np.array_equal(st_skip[k], st_none[k]) and np.array_equal(st_skip[k], st_loop[k]) for k in st_skip)
    for i in range(B):
        assert (it_log[i, :fell[i] + 1] >= 1).all() and not it_log[i, fell[i] + 1:].any(), (i, it_log[i])
    comp, st_comp, work = run(capi.Active(skip_fallen=True, compact=True))
    same(comp, skip, "compact", keys=names)
    assert work == (int(it_log.sum()), int(it_log.max(axis=0).sum())) and work_skip == (work[1] * B, work[1])


# ---- 7. checks ----
def test_active_errors_leave_the_arrays_alone(pkg, oracle):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, c = 7, "none"
    L = capi.lib()
    start, _ = batch_of(pkg, oracle, c, B)
    h = handle(capi, N, B, c)
    # at set time
    assert L.srbd_qp_srbd_set_active_f64(None, None) == -1
    assert L.srbd_qp_srbd_step_work(None, None, None) == -1
    for bad in (capi.ActiveStruct(None, 2, 0), capi.ActiveStruct(None, -1, 0), capi.ActiveStruct(None, 0, 2),
                capi.ActiveStruct(None, 1, -1)):
        assert L.srbd_qp_srbd_set_active_f64(h.ptr, ctypes.byref(bad)) == -1
    with pytest.raises(capi.SrbdQpError, match=r"\(-2\)"):  # SRBD_QP_EDIM
        capi.Handle(N, 4, 4, capacity=B).set_active(capi.Active(compact=True))
    with pytest.raises(ValueError, match="torch.int32"):
        h.set_active(capi.Active(mask=torch.zeros(B, dtype=torch.int64, device="cuda")))
    with pytest.raises(ValueError, match="is on cpu"):
        h.set_active(capi.Active(mask=torch.zeros(B, dtype=torch.int32)))
    assert h.step_work() == (0, 0)

    def refused(call, word):
        """The call fails with SRBD_QP_EINVAL and leaves xs, us, x0 / x and alpha as they were."""
        v = [_dev(a) for a in start]
        with pytest.raises(capi.SrbdQpError, match=rf"\(-1\).*{word}"):
            call(*v)
        torch.cuda.synchronize()
        for u, a in zip(v, start):
            assert torch.equal(u, _dev(a)), word

    step = lambda settings=NMPC: (lambda xs, us, x0, al: capi.srbd_nmpc(h, xs, us, x0, al, c, settings, SQP_MAX_LOOP))
    roll = lambda settings=NMPC: (lambda xs, us, x, al: capi.srbd_rollout(h, xs, us, x, al, 2, c, settings, SQP_MAX_LOOP))
    # skip_fallen without a contact, and with a contact that has no fallen
    h.set_active(capi.Active(skip_fallen=True))
    for call in (step(), roll()):
        refused(call, "skip_fallen")
    h.set_contact(capi.Contact())
    for call in (step(), roll()):
        refused(call, "skip_fallen")
    h.set_contact(capi.Contact(fallen=torch.zeros(B, dtype=torch.int32, device="cuda")))
    got, _ = run_step(capi, h, start, c, capi.Active(skip_fallen=True))  # and with one it runs
    assert int(got["sqp_iter"].min()) >= 1
    # compact with an IPM warm start
    h.set_active(capi.Active(compact=True))
    for call in (step(dict(NMPC, warm_start=1)), roll(dict(NMPC, warm_start=1))):
        refused(call, "warm_start")
    # a mask shorter than the batch is the binding's ValueError
    h.set_active(capi.Active(mask=_dev_i32(np.ones(B - 1))))
    with pytest.raises(ValueError, match="6 rows"):
        step()(*[_dev(a) for a in start])
