"""Terrain under the gait planner on the device (srbd_qp_srbd_set_terrain_f64,
srbd_qp_srbd_terrain_height_f64): the sampler and the planner against the host statement
srbd_model.terrain_height / gait_plan(terrain=...), flat ground and a cleared terrain against the
planner without (bit for bit), a plane against its closed form, the replanning rollout against
the caller's own loop (bit for bit) and against the host closed loop of tests/rollout_host.py
with a gait and the terrain."""
import ctypes as C

import numpy as np
import pytest

import gait_host as GH
import rollout_host as RH
import terrain_host as TH
from srbd_device import (FIELDS, NMPC, SQP_MAX_LOOP, STEP_ATOL_U, STEP_ATOL_X, _dev, caller_loop, close, device_gait,
                         device_terrain, handle)

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-11, 1e-12  # `close`'s: rtol, and atol per max(|want|, 1)
# the two map shapes, neither square: (ny, nx, x0, y0, cell) around the robots' start
GRIDS = ((7, 12, 0.1, -0.25, 0.08), (9, 5, 0.3, -0.4, 0.1))


def tol(want):
    """The tolerance `close` applies to each entry of `want`."""
    return RTOL * np.abs(want) + ATOL * max(np.abs(want).max(), 1.0)


def close_z(got, want, slack, what):
    """`close` plus `slack` per entry (G (dx + dy): the height follows the xy it is sampled at)."""
    err = np.abs(got.cpu().numpy() - want)
    bound = tol(want) + slack
    assert (err <= bound).all(), (what, float((err - bound).max()))


def terrains(sm, B, search):
    """The planner test's two terrains: two rough maps of 7 x 12 with a per-robot map index, and
    stairs of 9 x 5 (treads of two samples, 5 cm risers)."""
    ny, nx, x0, y0, cell = GRIDS[0]
    two = sm.SrbdTerrain(height=np.stack([TH.rough(ny, nx, 71), TH.rough(ny, nx, 72, 0.05)]), x0=x0, y0=y0, cell=cell,
                         map_r=np.arange(B) % 2, search=search, w_rough=100.0)
    ny, nx, x0, y0, cell = GRIDS[1]
    st = sm.SrbdTerrain(height=TH.stairs(ny, nx, 2, 0.05, 1), x0=x0, y0=y0, cell=cell, search=search, w_rough=40.0)
    return (("rough", two), ("stairs", st))


def planner_cases(sm, B, N):
    """Every case of the planner test at one shape: (name, gait, terrain, tick, inputs)."""
    p = sm.SrbdParams()
    inputs = GH.random_inputs(sm, p, B, 100 + N)
    for tick in (0, 10**12 + 3):
        period, swing, offset = GH.special_gaits(max(B, 5), N, tick, 200 + N)
        for search in (0, 1, 3):
            for name, ter in terrains(sm, B, search):
                for anchor in (0, 1):
                    g = sm.SrbdGait(period=period[:B], swing=swing[:B], offset=offset[:B],
                                    hip=((0.02, -0.11), (0.01, 0.12)), ground_z=0.03, k_raibert=0.07,
                                    fz_stance=250.0, fz_swing=1.5, anchor=anchor)
                    yield (name, search, tick, anchor), g, ter, tick, inputs


# the largest N at which the poses and the foothold tables of four robots fit a block's 64 KiB
# (56 N + 80 bytes a robot) is 291; 600 is one robot per block
SHAPES = [(5, 1), (5, 2), (5, 33), (3, 70), (5, 291), (2, 600)]
MIN_MARGIN = 1e-6  # of cell^2: no selection of any case is closer to a tie than this


# ---- 1. the sampler ----
def test_sampler_matches_the_host_statement(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    h = handle(capi, 4, 4, "none")
    rng = np.random.default_rng(5)
    for ny, nx, x0, y0, cell in ((2, 2, -0.3, 0.2, 0.25),) + GRIDS:
        H = np.stack([TH.rough(ny, nx, 31 + m) for m in range(3)])
        ter = sm.SrbdTerrain(height=H, x0=x0, y0=y0, cell=cell)
        h.set_terrain(device_terrain(capi, ter))
        xb, yb = x0 + cell * (nx - 1), y0 + cell * (ny - 1)
        ii, jj = np.meshgrid(np.arange(nx), np.arange(ny))
        nodes = np.stack([x0 + cell * ii, y0 + cell * jj], axis=-1).reshape(-1, 2)
        inside = np.stack([rng.uniform(x0, xb, 40), rng.uniform(y0, yb, 40)], axis=1)
        last = np.concatenate([np.stack([np.full(6, xb), rng.uniform(y0, yb, 6)], axis=1),
                               np.stack([rng.uniform(x0, xb, 6), np.full(6, yb)], axis=1),
                               np.stack([np.full(6, xb - 1e-9 * cell), rng.uniform(y0, yb, 6)], axis=1)])
        out = np.array([(x0 - 0.3, y0 + 0.4 * cell), (xb + 0.3, y0 + 0.4 * cell), (x0 + 0.4 * cell, y0 - 0.3),
                        (x0 + 0.4 * cell, yb + 0.3), (x0 - 1, y0 - 1), (xb + 1, y0 - 1), (x0 - 1, yb + 1),
                        (xb + 1, yb + 1), (x0 - 1e9, yb + 1e9)])
        pts = np.concatenate([nodes, inside, last, out])
        maps = rng.integers(0, 3, size=len(pts))
        got = capi.srbd_terrain_height(h, _dev(pts), torch.from_numpy(maps.astype(np.int32)).cuda())
        close(got, sm.terrain_height(ter, pts, maps), (ny, nx, "per-point maps"))
        got0 = capi.srbd_terrain_height(h, _dev(pts))
        close(got0, sm.terrain_height(ter, pts), (ny, nx, "map 0"))
        # on the nodes the sample itself, outside the grid the edge's
        got_nodes = capi.srbd_terrain_height(h, _dev(nodes))
        np.testing.assert_allclose(got_nodes.cpu().numpy(), H[0].ravel(), rtol=0, atol=2e-16)
        corners = got0[-5:-1].cpu().numpy()
        assert np.array_equal(corners, H[0][[0, 0, -1, -1], [0, -1, 0, -1]])
    assert capi.srbd_terrain_height(h, _dev(np.zeros((0, 2)))).shape == (0,)


# ---- 2. the planner against the host statement ----
@pytest.mark.parametrize("B,N", SHAPES)
def test_planner_with_terrain_matches_the_host_statement(pkg, B, N):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    p = sm.SrbdParams()
    h = handle(capi, N, B, "none")
    smallest, moved = np.inf, 0
    for case, g, ter, tick, (cmd, x, ref_pose, foot_now) in planner_cases(sm, B, N):
        S, cell, G = ter.search, ter.cell, TH.lipschitz(ter.height, ter.cell)
        want, want_pose, want_feet = sm.gait_plan(p, g, cmd, x, tick, ref_pose, foot_now, N, terrain=ter)
        q, margin, n, down = TH.selection(sm, p, g, ter, cmd, x, tick, ref_pose, foot_now, N)
        smallest = min(smallest, margin / cell ** 2)
        moved += int(((q >= 0) & (q != (2 * S + 1) ** 2 // 2)).sum())
        assert margin >= MIN_MARGIN * cell ** 2, (case, margin / cell ** 2)  # every touchdown, none skipped
        h.set_terrain(device_terrain(capi, ter))
        pose_t, feet_t = _dev(ref_pose), _dev(foot_now)
        got = capi.srbd_gait_plan(h, device_gait(capi, g), _dev(cmd), _dev(x), tick, pose_t, feet_t)
        h.synchronize()
        assert np.array_equal(got.fz_max.cpu().numpy(), want.fz_max), case
        keep = [i for i in range(12) if i != 8]
        close(got.x_ref[:, :, keep], want.x_ref[:, :, keep], (case, "x_ref"))
        txy = tol(want.x_ref[:, :, keep])
        close_z(got.x_ref[:, :, 8], want.x_ref[:, :, 8], G * (txy[:, :, 6] + txy[:, :, 7]), (case, "x_ref z"))
        for f, name in enumerate(("foot_r", "foot_l")):
            gf, wf = getattr(got, name), getattr(want, name)
            close(gf[:, :, 0:2], wf[:, :, 0:2], (case, name))
            t = tol(wf[:, :, 0:2])
            close_z(gf[:, :, 2], wf[:, :, 2], G * (t[:, :, 0] + t[:, :, 1]), (case, name, "z"))
            # the chosen candidate, exactly: the margin above is far beyond the devices' rounding
            d = np.rint((gf[:, :, 0:2].cpu().numpy() - n[:, :, f]) / cell).astype(np.int64)
            got_q = (d[:, :, 1] + S) * (2 * S + 1) + (d[:, :, 0] + S)
            assert np.array_equal(got_q[~down[:, :, f]], q[:, :, f][~down[:, :, f]]), (case, name)
        close(pose_t, want_pose, case)
        close(feet_t[:, :, 0:2], want_feet[:, :, 0:2], case)
        t = tol(want_feet[:, :, 0:2])
        close_z(feet_t[:, :, 2], want_feet[:, :, 2], G * (t[:, :, 0] + t[:, :, 1]), (case, "foot_now z"))
        # bit identities on the device's own outputs
        assert torch.equal(feet_t[:, 0], got.foot_r[:, 0]) and torch.equal(feet_t[:, 1], got.foot_l[:, 0])
        assert torch.equal(pose_t, got.x_ref[:, 1, [6, 7, 2]]), case
        stance = torch.from_numpy(~GH.schedule(g.period, g.swing, g.offset, tick, N)[0][:, 0]).cuda()
        assert bool(stance.any()), case
        assert torch.equal(feet_t[stance], _dev(foot_now)[stance]), case
        if S == 0:  # nothing is evaluated: the nominal foothold's bits
            h.set_terrain(None)
            flat = capi.srbd_gait_plan(h, device_gait(capi, g), _dev(cmd), _dev(x), tick, _dev(ref_pose),
                                       _dev(foot_now))
            assert torch.equal(flat.foot_r[:, :, 0:2], got.foot_r[:, :, 0:2]), case
            assert torch.equal(flat.foot_l[:, :, 0:2], got.foot_l[:, :, 0:2]), case
    print(f"(B, N) = ({B}, {N}): smallest selection margin {smallest:.3e} cell^2")
    assert moved > 0  # the selection moved footholds: the cases are not the nominal plan
    # the per-robot gaits hold what the cases need (right foot of robots 0..4 at the last tick)
    swinging, j, down = GH.schedule(g.period, g.swing, g.offset, tick, N)
    if B >= 5:
        assert down[0].all()                                  # a standing robot
        assert swinging[1, 0, 0]                              # in swing at stage 0
        assert not swinging[2, 0, 0] and j[2, 0, 0] == 0      # a touchdown exactly at stage 0
        assert swinging[4, :, 0].all() and j[4, 0, 0] > N     # a period above N: the clamp j' = N
        if N >= 6:  # a period below N: two touchdowns of one foot in the window
            assert len(set(j[3, :, 0][swinging[3, :, 0]].tolist())) >= 2


# ---- 3. flat ground at zero, and a cleared terrain, are the planner without terrain ----
@pytest.mark.parametrize("B,N", [(5, 33), (6, 10)])
def test_flat_ground_and_a_cleared_terrain_give_the_bits_without_terrain(pkg, B, N):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    p = sm.SrbdParams()
    h = handle(capi, N, B, "none")
    tick = 10**12 + 3
    cmd, x, ref_pose, foot_now = GH.random_inputs(sm, p, B, 100 + N)
    period, swing, offset = GH.special_gaits(max(B, 5), N, tick, 200 + N)
    g = device_gait(capi, sm.SrbdGait(period=period[:B], swing=swing[:B], offset=offset[:B], ground_z=0.03,
                                      k_raibert=0.07, fz_stance=250.0, fz_swing=1.5))

    def run():
        state = [_dev(ref_pose), _dev(foot_now)]
        w = capi.srbd_gait_plan(h, g, _dev(cmd), _dev(x), tick, *state)
        h.synchronize()
        return [getattr(w, k) for k in FIELDS] + state

    base = run()
    ny, nx, x0, y0, cell = GRIDS[0]
    h.set_terrain(capi.Terrain(_dev(TH.flat0(ny, nx)), x0, y0, cell, search=3, w_rough=4.0))
    for u, v in zip(run(), base):
        assert torch.equal(u, v)
    rough = capi.Terrain(_dev(TH.rough(ny, nx, 71)), x0, y0, cell, search=3, w_rough=4.0)
    h.set_terrain(rough)
    assert not torch.equal(run()[1], base[1])  # a terrain is felt ...
    h.set_terrain(None)  # ... and cleared again
    for u, v in zip(run(), base):
        assert torch.equal(u, v)


# ---- 4. a plane against its closed form ----
def test_a_plane_on_the_device_has_its_closed_form_heights(pkg):
    capi, sm = pkg.capi, pkg.srbd_model
    B, N, tick = 5, 33, 7
    p = sm.SrbdParams()
    h = handle(capi, N, B, "none")
    cmd, x, ref_pose, foot_now = GH.random_inputs(sm, p, B, 100 + N)
    period, swing, offset = GH.special_gaits(B, N, tick, 200 + N)
    g = sm.SrbdGait(period=period, swing=swing, offset=offset, ground_z=0.03, k_raibert=0.07, fz_stance=250.0)
    al, be, ga = 0.2, -0.1, 0.05
    ny, nx, x0, y0, cell = 31, 41, -1.5, -1.5, 0.1  # wide enough that no sample is clamped
    ter = sm.SrbdTerrain(height=TH.plane(ny, nx, x0, y0, cell, al, be, ga), x0=x0, y0=y0, cell=cell, search=1,
                         w_rough=3.0)
    G = TH.lipschitz(ter.height, cell)
    base = sm.gait_plan(p, g, cmd, x, tick, ref_pose, foot_now, N)[0]
    down = GH.schedule(period, swing, offset, tick, N)[2]
    h.set_terrain(device_terrain(capi, ter))
    got = capi.srbd_gait_plan(h, device_gait(capi, g), _dev(cmd), _dev(x), tick, _dev(ref_pose), _dev(foot_now))
    h.synchronize()
    for f, name in enumerate(("foot_r", "foot_l")):
        gf, bf = getattr(got, name), getattr(base, name)
        close(gf[:, :, 0:2], bf[:, :, 0:2], name)  # rho is the same everywhere: the nominal foothold
        want = np.where(down[:, :, f], bf[:, :, 2], g.ground_z + (al * bf[:, :, 0] + be * bf[:, :, 1] + ga))
        t = tol(bf[:, :, 0:2])
        close_z(gf[:, :, 2], want, G * (t[:, :, 0] + t[:, :, 1]), (name, "z"))
    want = cmd[:, 3, None] + (al * base.x_ref[:, :, 6] + be * base.x_ref[:, :, 7] + ga)
    t = tol(base.x_ref)
    close_z(got.x_ref[:, :, 8], want, G * (t[:, :, 6] + t[:, :, 7]), "x_ref z")


# ---- 5. the replanning rollout with terrain is the caller's loop, bit for bit ----
@pytest.mark.parametrize("constraints", ["none", "box_u"])
def test_terrain_rollout_is_the_callers_loop_bit_for_bit(pkg, constraints):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N, T, tick0 = 6, 10, 3, 10**12 + 3
    p = sm.SrbdParams()
    h = handle(capi, N, B, constraints)
    xs, us, x, alpha, gait, cmd, ref_pose, foot_now = TH.stairs_case(sm, p, B, N, T, 41)
    h.set_terrain(device_terrain(capi, TH.stairs_terrain(sm, search=1)))
    gait_t, cmd_t = device_gait(capi, gait), _dev(cmd)
    wrench_t = _dev(np.zeros((B, T, 6)))
    a = [_dev(v) for v in (xs, us, x, alpha, ref_pose, foot_now)]
    logs_a = capi.srbd_rollout_gait(h, gait_t, cmd_t, *a, T, tick0, constraints, NMPC, SQP_MAX_LOOP, wrench=wrench_t)
    b = [_dev(v) for v in (xs, us, x, alpha, ref_pose, foot_now)]
    logs_b = caller_loop(capi, h, B, N, T, constraints, *b[:4], wrench_t, 1, 0.0, gait_t=gait_t, cmd_t=cmd_t,
                         pose=b[4], feet=b[5], tick0=tick0)
    names = ("xs", "us", "x", "alpha", "ref_pose", "foot_now", "x_log", "u_log", "sqp_iter_log", "converged_log",
             "foot_log", "fz_log")
    for name, u, v in zip(names, a + list(logs_a), b + list(logs_b)):
        assert bool(torch.isfinite(u.double()).all()), name
        assert torch.equal(u, v), name
    assert int(logs_a[2].min()) >= 1  # the steps ran
    assert float(logs_a[4][:, :, :, 2].max()) >= TH.STAIRS["rise"]  # ... on the stairs
    # and without the terrain the rollout is another one
    h.set_terrain(None)
    c = [_dev(v) for v in (xs, us, x, alpha, ref_pose, foot_now)]
    logs_c = capi.srbd_rollout_gait(h, gait_t, cmd_t, *c, T, tick0, constraints, NMPC, SQP_MAX_LOOP, wrench=wrench_t)
    assert not torch.equal(logs_c[4], logs_a[4])


# ---- 6. the replanning rollout with terrain against the host closed loop ----
# STAIRS_SEED was chosen on the CPU (scripts/rollout_sensitivity.py --gait --terrain --search 20 44):
# the host loop's smallest comparison margin is >= 1e-6, no foothold selection is closer to a tie
# than 1e-6 cell^2, the iteration counts and the chosen candidates do not change under the
# perturbation of relative 1e-7, and a foot lands on a higher tread (all asserted below).
STAIRS_SEED = 21
# d_t: the largest change of the host loop's x_log[t] / u_log[t-1] / foot_log[t-1]
# under that perturbation, t = 1..4 (scripts/rollout_sensitivity.py --gait --terrain --seed 21).
D_T = {  # (d_t of x, d_t of u, d_t of the feet)
    "none": ((3.3e-07, 5.3e-07, 7.1e-07, 7.7e-07), (2.8e-05, 2.3e-05, 1.9e-05, 1.2e-05),
             (5.3e-08, 5.3e-08, 5.3e-08, 5.3e-08)),
    "box_u": ((3.4e-07, 5.4e-07, 7.3e-07, 7.9e-07), (2.9e-05, 2.4e-05, 2.0e-05, 1.2e-05),
              (5.3e-08, 5.3e-08, 5.3e-08, 5.3e-08)),
}


@pytest.mark.parametrize("constraints", ["none", "box_u"])
def test_terrain_rollout_matches_the_host_terrain_loop(pkg, oracle, constraints):
    capi, sm = pkg.capi, pkg.srbd_model
    B, N, T = 4, 10, 4
    p = sm.SrbdParams()
    xs, us, x, alpha, gait, cmd, ref_pose, foot_now = TH.stairs_case(sm, p, B, N, T, STAIRS_SEED)
    ter = TH.stairs_terrain(sm, search=1)
    cell, rise = ter.cell, TH.STAIRS["rise"]
    host = RH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, SQP_MAX_LOOP, constraints, p=p, gait=gait, cmd=cmd,
                          ref_pose=ref_pose, foot_now=foot_now, terrain=ter)
    assert host["margin"] >= 1e-6, host["margin"]
    assert host["select_margin"] >= MIN_MARGIN * cell ** 2, host["select_margin"] / cell ** 2
    assert len(set(host["sqp_iter"].ravel().tolist())) >= 2, host["sqp_iter"]
    assert (host["q_log"] >= 0).any() and ((host["q_log"] >= 0) & (host["q_log"] != 4)).any()  # a foothold moved
    h = handle(capi, N, B, constraints)
    h.set_terrain(device_terrain(capi, ter))
    a = [_dev(v) for v in (xs, us, x, alpha, ref_pose, foot_now)]
    x_log, u_log, it_log, cv_log, foot_log, fz_log = capi.srbd_rollout_gait(
        h, device_gait(capi, gait), _dev(cmd), *a, T, 0, constraints, NMPC, SQP_MAX_LOOP)
    x_log, u_log, foot_log = x_log.cpu().numpy(), u_log.cpu().numpy(), foot_log.cpu().numpy()
    print("sqp_iter device", it_log.cpu().numpy().tolist(), "host", host["sqp_iter"].tolist())
    for t in range(1, T + 1):
        print(f"tick {t}: max |x_log - host| {np.abs(x_log[:, t] - host['x_log'][:, t]).max():.3e}, "
              f"max |u_log - host| {np.abs(u_log[:, t - 1] - host['u_log'][:, t - 1]).max():.3e}, "
              f"max |foot_log - host| {np.abs(foot_log[:, t - 1] - host['foot_log'][:, t - 1]).max():.3e}")
    assert np.array_equal(it_log.cpu().numpy(), host["sqp_iter"])
    assert np.array_equal(cv_log.cpu().numpy(), host["converged"])
    assert np.array_equal(a[3].cpu().numpy(), host["alpha"])
    assert np.array_equal(fz_log.cpu().numpy(), host["fz_log"])
    assert np.array_equal(x_log[:, 0], x)
    # the chosen candidates: the device's foothold minus the host's nominal one, in cells
    swing = host["fz_log"] == gait.fz_swing
    for t in range(T):
        xt = host["x_log"][:, t]
        pose, feet = (ref_pose, foot_now) if t == 0 else (host["poses"][t - 1], host["feet"][t - 1])
        n = TH.nominal(sm, p, gait, cmd[:, t], xt, t, pose, feet, N)[0][:, 0]  # row 0: [B][2][2]
        d = np.rint((foot_log[:, t, :, 0:2] - n) / cell).astype(np.int64)
        got_q = np.where(swing[:, t], (d[:, :, 1] + 1) * 3 + (d[:, :, 0] + 1), -1)
        assert np.array_equal(got_q, host["q_log"][:, t]), t
    close(_dev(foot_log[:, 0]), host["foot_log"][:, 0], "tick 0's feet")  # planned from the same x
    dt_x, dt_u, dt_f = D_T[constraints]
    for t in range(1, T + 1):
        # tick 1 is one step: the step test's tolerance; later ticks compound, by at most d_t
        ax = STEP_ATOL_X if t == 1 else max(STEP_ATOL_X, 10.0 * dt_x[t - 1])
        au = STEP_ATOL_U if t == 1 else max(STEP_ATOL_U, 10.0 * dt_u[t - 1])
        np.testing.assert_allclose(x_log[:, t], host["x_log"][:, t], rtol=1e-7, atol=ax, err_msg=f"x {t}")
        np.testing.assert_allclose(u_log[:, t - 1], host["u_log"][:, t - 1], rtol=1e-7, atol=au, err_msg=f"u {t}")
        af = max(STEP_ATOL_X, 10.0 * dt_f[t - 1])  # tick t - 1's feet are planned from x_log[t - 1]
        np.testing.assert_allclose(foot_log[:, t - 1], host["foot_log"][:, t - 1], rtol=1e-7, atol=af,
                                   err_msg=f"feet {t - 1}")
    assert np.array_equal(a[2].cpu().numpy(), x_log[:, T])
    # physically: a foot that lands on a higher tread than it started from rises by the treads' height
    land = swing[:, :-1] & ~swing[:, 1:]  # [B][T-1][2]: down at tick t + 1
    higher = 0
    for i, t, f in zip(*np.nonzero(land)):
        before, after = TH.stairs_level(foot_now[i, f, 0]), TH.stairs_level(foot_log[i, t + 1, f, 0])
        if before >= 0 and after > before:
            rose = foot_log[i, t + 1, f, 2] - (gait.ground_z + rise * before)
            assert abs(rose - rise * (after - before)) <= 1e-12, (i, t, f, rose)
            higher += 1
    assert higher >= 1


# ---- 7. errors ----
def test_terrain_errors(pkg):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    B, N = 4, 6
    h = handle(capi, N, B, "none")
    H = _dev(TH.rough(7, 12, 1))
    good = dict(x0=0.0, y0=0.0, cell=0.1, search=1, w_rough=1.0)
    xy = _dev(np.zeros((3, 2)))
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*no terrain"):
        capi.srbd_terrain_height(h, xy)
    bad = [(dict(good, cell=0.0), "cell"), (dict(good, cell=-1.0), "cell"), (dict(good, cell=float("nan")), "cell"),
           (dict(good, search=-1), "search"), (dict(good, search=4), "search"), (dict(good, w_rough=-1.0), "w_rough"),
           (dict(good, w_rough=float("inf")), "w_rough"), (dict(good, x0=float("inf")), "x0"),
           (dict(good, y0=float("nan")), "y0")]
    for kw, word in bad:
        with pytest.raises(capi.SrbdQpError, match=rf"\(-1\).*{word}"):
            h.set_terrain(capi.Terrain(H, **kw))
    for shape, word in (((1, 12), "nx and ny"), ((7, 1), "nx and ny")):
        with pytest.raises(capi.SrbdQpError, match=rf"\(-1\).*{word}"):
            h.set_terrain(capi.Terrain(torch.zeros(*shape, dtype=torch.float64, device="cuda"), **good))
    ts = capi.Terrain(H, **good).struct()
    ts.maps = 0
    assert capi.lib().srbd_qp_srbd_set_terrain_f64(h.ptr, C.byref(ts)) == -1  # maps < 1
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*no terrain"):  # a rejected terrain is not set
        capi.srbd_terrain_height(h, xy)
    with pytest.raises(capi.SrbdQpError, match=r"\(-2\)"):  # SRBD_QP_EDIM
        capi.Handle(N, 4, 4, capacity=B).set_terrain(capi.Terrain(H, **good))
    with pytest.raises(ValueError, match="torch.float64"):
        h.set_terrain(capi.Terrain(H.float(), **good))
    with pytest.raises(ValueError, match="is on cpu"):
        h.set_terrain(capi.Terrain(H.cpu(), **good))
    with pytest.raises(ValueError, match="map_r must be a torch.int32"):
        h.set_terrain(capi.Terrain(H, map_r=torch.zeros(B, dtype=torch.int64, device="cuda"), **good))
    h.set_terrain(capi.Terrain(H, map_r=torch.zeros(B - 1, dtype=torch.int32, device="cuda"), **good))
    p = sm.SrbdParams()
    cmd, x, ref_pose, foot_now = GH.random_inputs(sm, p, B, 3)
    with pytest.raises(ValueError, match="map_r of 3 rows"):
        capi.srbd_gait_plan(h, capi.Gait(period=6, swing=(3, 3), offset=(0, 3), fz_stance=250.0), _dev(cmd), _dev(x), 0,
                            _dev(ref_pose), _dev(foot_now))
    # NULL pointers of the sampler, n < 0, n == 0
    h.set_terrain(capi.Terrain(H, **good))
    L, out = capi.lib(), torch.zeros(3, dtype=torch.float64, device="cuda")
    assert L.srbd_qp_srbd_terrain_height_f64(h.ptr, 3, None, None, out.data_ptr(), None) == -1
    assert L.srbd_qp_srbd_terrain_height_f64(h.ptr, 3, xy.data_ptr(), None, None, None) == -1
    assert L.srbd_qp_srbd_terrain_height_f64(h.ptr, -1, xy.data_ptr(), None, out.data_ptr(), None) == -1
    assert L.srbd_qp_srbd_terrain_height_f64(h.ptr, 0, xy.data_ptr(), None, out.data_ptr(), None) == 0
    assert capi.srbd_terrain_height(h, xy).shape == (3,)
    h.set_terrain(None)
    with pytest.raises(capi.SrbdQpError, match=r"\(-1\).*no terrain"):
        capi.srbd_terrain_height(h, xy)
