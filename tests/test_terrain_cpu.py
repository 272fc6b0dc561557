"""Terrain under the gait planner (srbd_qp_srbd_set_terrain_f64) without a GPU: the host
statement srbd_model.terrain_height / foothold_select / gait_plan(terrain=...) has the
properties include/srbd_qp.h states.  No terrain and flat ground are the planner as it was; a
plane is sampled exactly and moves no foothold; the sampler is exact on nodes, extends its edges
and is continuous; on stairs the selection leaves the risers, never for a worse cost, and breaks
ties towards the smallest candidate index; a stance foot keeps its bits; and one tick of
tests/rollout_host.py's loop with the terrain is gait_plan(terrain=...) followed by the host SQP
loop."""
import subprocess

import numpy as np
import pytest

import gait_host as GH
import nmpc_plan_host as PH
import rollout_host as RH
import terrain_host as TH
from gait_host import rot
from srbd_device import FIELDS, NMPC

TERRAIN_SYMBOLS = ("srbd_qp_srbd_set_terrain_f64", "srbd_qp_srbd_terrain_height_f64")
# the two map shapes of the tests, neither square: (ny, nx, x0, y0, cell) around the robots' start
GRIDS = ((7, 12, 0.1, -0.25, 0.08), (9, 5, 0.3, -0.4, 0.1))


def planner_case(sm, B, N, tick, seed):
    p = sm.SrbdParams()
    period, swing, offset = GH.special_gaits(B, N, tick, seed)
    gait = sm.SrbdGait(period=period, swing=swing, offset=offset, hip=((0.02, -0.11), (0.01, 0.12)), ground_z=0.03,
                       k_raibert=0.05, fz_stance=250.0, fz_swing=1.5)
    return (p, gait) + GH.random_inputs(sm, p, B, seed + 1)


def same_plan(a, b):
    return all(np.array_equal(getattr(a[0], k), getattr(b[0], k)) for k in FIELDS) and \
        np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- 1. the entry points exist ----
def test_terrain_entry_points_are_exported(pkg):
    capi = pkg.capi
    assert set(TERRAIN_SYMBOLS) <= set(capi.exported_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    assert set(TERRAIN_SYMBOLS) <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = capi.lib()
    assert L.srbd_qp_srbd_set_terrain_f64(None, None) == -1
    assert L.srbd_qp_srbd_terrain_height_f64(None, 0, None, None, None, None) == -1
    assert L.srbd_qp_abi_version() == 12  # additive to ABI 12
    import torch
    with pytest.raises(ValueError, match="torch.float64"):
        capi.Terrain(torch.zeros(3, 4, dtype=torch.float32), 0.0, 0.0, 1.0).struct()
    with pytest.raises(ValueError, match="is on cpu"):
        capi.Terrain(torch.zeros(3, 4, dtype=torch.float64), 0.0, 0.0, 1.0).struct()


# ---- 2. no terrain, and flat ground at zero, are the planner as it was ----
def test_no_terrain_and_flat_ground_are_the_planner_without(pkg):
    sm = pkg.srbd_model
    B, N, tick = 8, 9, 77
    p, gait, cmd, x, ref_pose, foot_now = planner_case(sm, B, N, tick, 10)
    base = sm.gait_plan(p, gait, cmd, x, tick, ref_pose, foot_now, N)
    assert same_plan(sm.gait_plan(p, gait, cmd, x, tick, ref_pose, foot_now, N, terrain=None), base)
    ny, nx, x0, y0, cell = GRIDS[0]
    for search in (0, 1, 2, 3):
        flat = sm.SrbdTerrain(height=TH.flat0(ny, nx), x0=x0, y0=y0, cell=cell, search=search, w_rough=50.0)
        assert same_plan(sm.gait_plan(p, gait, cmd, x, tick, ref_pose, foot_now, N, terrain=flat), base), search


# ---- 3. a plane: exact heights in closed form, no foothold moves ----
@pytest.mark.parametrize("search", [0, 2])
def test_a_plane_is_sampled_exactly_and_moves_no_foothold(pkg, search):
    sm = pkg.srbd_model
    B, N, tick = 8, 9, 77
    p, gait, cmd, x, ref_pose, foot_now = planner_case(sm, B, N, tick, 20)
    al, be, ga = 0.2, -0.1, 0.05
    # a grid wide enough that no sample is clamped: the closed form holds only inside
    ny, nx, x0, y0, cell = 21, 33, -1.0, -1.0, 0.1
    ter = sm.SrbdTerrain(height=TH.plane(ny, nx, x0, y0, cell, al, be, ga), x0=x0, y0=y0, cell=cell, search=search,
                         w_rough=3.0)
    base = sm.gait_plan(p, gait, cmd, x, tick, ref_pose, foot_now, N)[0]
    got = sm.gait_plan(p, gait, cmd, x, tick, ref_pose, foot_now, N, terrain=ter)[0]
    down = GH.schedule(gait.period, gait.swing, gait.offset, tick, N)[2]
    assert (~down).any() and np.array_equal(got.fz_max, base.fz_max)
    for f, name in enumerate(("foot_r", "foot_l")):
        g, b = getattr(got, name), getattr(base, name)
        assert np.array_equal(g[down[:, :, f]], b[down[:, :, f]])  # foot_now, untouched
        t = ~down[:, :, f]
        assert np.array_equal(g[t][:, 0:2], b[t][:, 0:2])  # rho is the same everywhere: d* = 0
        want = gait.ground_z + (al * g[t][:, 0] + be * g[t][:, 1] + ga)
        np.testing.assert_allclose(g[t][:, 2], want, rtol=0, atol=8 * np.finfo(float).eps)
    keep = [i for i in range(12) if i != 8]
    assert np.array_equal(got.x_ref[:, :, keep], base.x_ref[:, :, keep])
    want = cmd[:, 3, None] + (al * got.x_ref[:, :, 6] + be * got.x_ref[:, :, 7] + ga)
    np.testing.assert_allclose(got.x_ref[:, :, 8], want, rtol=0, atol=8 * np.finfo(float).eps)


# ---- 4. the sampler ----
@pytest.mark.parametrize("grid", [(2, 2, -0.3, 0.2, 0.25)] + list(GRIDS))
def test_the_sampler_is_exact_on_nodes_extends_edges_and_is_continuous(pkg, grid):
    sm = pkg.srbd_model
    ny, nx, x0, y0, cell = grid
    H = np.stack([TH.rough(ny, nx, 31), TH.rough(ny, nx, 32)])
    ter = sm.SrbdTerrain(height=H, x0=x0, y0=y0, cell=cell)
    ii, jj = np.meshgrid(np.arange(nx), np.arange(ny))
    nodes = np.stack([x0 + cell * ii, y0 + cell * jj], axis=-1)
    for m in range(2):
        np.testing.assert_allclose(sm.terrain_height(ter, nodes, m), H[m], rtol=0, atol=2e-16)
    xa, xb, ya, yb = x0, x0 + cell * (nx - 1), y0, y0 + cell * (ny - 1)
    ys, xs = np.linspace(ya, yb, 7), np.linspace(xa, xb, 7)
    on = lambda pts: sm.terrain_height(ter, np.array(pts), 1)
    # outside each side the edge value extends: the same bits however far out, and the value on
    # the edge (xb, yb are the last nodes up to their own rounding, hence the ulps)
    edge = dict(rtol=0, atol=4 * np.finfo(float).eps)
    for far in (0.01, 3.0, 1e6):
        for side, out, out1 in (([(xa, y) for y in ys], [(xa - far, y) for y in ys], [(xa - 1.0, y) for y in ys]),
                                ([(xb, y) for y in ys], [(xb + far, y) for y in ys], [(xb + 1.0, y) for y in ys]),
                                ([(x, ya) for x in xs], [(x, ya - far) for x in xs], [(x, ya - 1.0) for x in xs]),
                                ([(x, yb) for x in xs], [(x, yb + far) for x in xs], [(x, yb + 1.0) for x in xs])):
            assert np.array_equal(on(out), on(out1))
            np.testing.assert_allclose(on(out), on(side), **edge)
        corners = on([(xa - far, ya - far), (xb + far, ya - far), (xa - far, yb + far), (xb + far, yb + far)])
        assert np.array_equal(corners, H[1][[0, 0, -1, -1], [0, -1, 0, -1]])
    # continuous across a cell boundary (the first interior one, or the far edge of a 2 x 2 map)
    G, eps = TH.lipschitz(H, cell), 1e-9
    bx, by = x0 + cell * min(1, nx - 1), y0 + cell * min(1, ny - 1)
    for y in ys:
        assert abs(on([(bx + eps, y)])[0] - on([(bx - eps, y)])[0]) <= 2 * G * eps + 1e-15
    for xq in xs:
        assert abs(on([(xq, by + eps)])[0] - on([(xq, by - eps)])[0]) <= 2 * G * eps + 1e-15
    # the map argument defaults to map 0 and broadcasts
    pts = np.random.default_rng(33).uniform(-1, 1, size=(5, 2))
    assert np.array_equal(sm.terrain_height(ter, pts), sm.terrain_height(ter, pts, np.zeros(5, dtype=int)))


# ---- 5. stairs: the selection leaves the risers and never pays more than staying ----
def cost(sm, ter, n, d, maps=None):
    """J of candidate d = (di, dj) around n, restated."""
    c = n + ter.cell * np.array(d, dtype=np.float64)
    h = lambda q: sm.terrain_height(ter, q, maps)
    rho = np.max([np.abs(h(c + ter.cell * np.array(e)) - h(c)) for e in ((1, 0), (-1, 0), (0, 1), (0, -1))], axis=0)
    return ter.cell ** 2 * (d[0] ** 2 + d[1] ** 2) + ter.w_rough * rho ** 2


def test_on_stairs_the_selection_leaves_the_risers(pkg):
    sm = pkg.srbd_model
    B, N, tick, S = 8, 9, 77, 2
    p, gait, cmd, x, ref_pose, foot_now = planner_case(sm, B, N, tick, 40)
    ter = TH.stairs_terrain(sm, search=S, w_rough=100.0)
    q, margin, n, down = TH.selection(sm, p, gait, ter, cmd, x, tick, ref_pose, foot_now, N)
    got = sm.gait_plan(p, gait, cmd, x, tick, ref_pose, foot_now, N, terrain=ter)[0]
    feet = np.stack([got.foot_r, got.foot_l], axis=2)
    moved_off = 0
    for i, k, f in zip(*np.nonzero(~down)):
        d = (int(q[i, k, f]) % (2 * S + 1) - S, int(q[i, k, f]) // (2 * S + 1) - S)
        np.testing.assert_array_equal(feet[i, k, f, 0:2], n[i, k, f] + ter.cell * np.array(d, dtype=np.float64))
        assert cost(sm, ter, n[i, k, f], d) <= cost(sm, ter, n[i, k, f], (0, 0))
        if TH.stairs_level(n[i, k, f, 0]) < 0 and d != (0, 0):
            assert TH.stairs_level(feet[i, k, f, 0]) >= 0  # from a riser onto a tread
            assert feet[i, k, f, 2] == gait.ground_z + TH.STAIRS["rise"] * TH.stairs_level(feet[i, k, f, 0])
            moved_off += 1
    assert moved_off >= 1


# ---- 6. ties go to the smallest q ----
def test_ties_go_to_the_smallest_candidate_index(pkg):
    sm = pkg.srbd_model
    H = np.zeros((5, 5))
    H[2, 2] = 1.0  # a spike under the nominal foothold: the four diagonal neighbours tie
    ter = sm.SrbdTerrain(height=H, x0=-1.0, y0=-1.0, cell=0.5, search=1, w_rough=100.0)
    n = np.array([[0.0, 0.0]])
    xy, z, q, margin = sm.foothold_select(ter, n)
    assert q[0] == 0 and margin[0] == 0.0 and np.array_equal(xy[0], [-0.5, -0.5]) and z[0] == 0.0
    H2 = H.copy()
    H2[1, 0] = 1.0  # roughen candidate 0: the next of the tied ones is q = 2, (di, dj) = (+1, -1)
    xy, z, q, margin = sm.foothold_select(sm.SrbdTerrain(height=H2, x0=-1.0, y0=-1.0, cell=0.5, search=1,
                                                         w_rough=100.0), n)
    assert q[0] == 2 and margin[0] == 0.0 and np.array_equal(xy[0], [0.5, -0.5])


# ---- 7. a stance foot keeps its bits while the robot crosses cells ----
def test_a_stance_foot_keeps_its_bits_z_included(pkg):
    sm = pkg.srbd_model
    B, N, tick0 = 10, 12, 1000
    p = sm.SrbdParams()
    period, swing, offset = GH.special_gaits(B, N, tick0, 60)
    gait = sm.SrbdGait(period=period, swing=swing, offset=offset, k_raibert=0.05, fz_stance=250.0)
    cmd, x, ref_pose, foot_now = GH.random_inputs(sm, p, B, 61)
    cmd[:, 0] = np.where(np.abs(cmd[:, 0]) < 0.2, 0.4, cmd[:, 0])
    ny, nx, x0, y0, cell = 9, 12, 0.0, -0.4, 0.01  # a centimetre a cell: every robot crosses several
    ter = sm.SrbdTerrain(height=TH.rough(ny, nx, 62), x0=x0, y0=y0, cell=cell, search=1, w_rough=5.0)
    start = ref_pose.copy()
    landings, was_swinging = 0, None
    for t in range(int(period.max()) + 2):
        xa = x.copy()
        xa[:, 6:8], xa[:, 9:11] = ref_pose[:, 0:2], rot(ref_pose[:, 2], cmd[:, 0:2])
        plan, pose1, feet1 = sm.gait_plan(p, gait, cmd, xa, tick0 + t, ref_pose, foot_now, N, terrain=ter)
        swinging = GH.schedule(period, swing, offset, tick0 + t, N)[0][:, 0]
        assert np.array_equal(feet1[~swinging], foot_now[~swinging])  # x, y and z: the bits it landed on
        if was_swinging is not None:
            land = was_swinging & ~swinging  # latched at the last swing tick's target
            landings += int(land.sum())
            maps = np.zeros((B, 2), dtype=int)
            assert np.array_equal(feet1[land][:, 2], sm.terrain_height(ter, feet1[:, :, 0:2], maps)[land])
        was_swinging = swinging
        ref_pose, foot_now = pose1, feet1
    assert (np.abs(ref_pose[:, 0:2] - start[:, 0:2]).max(axis=1) > 3 * cell).all()
    assert landings >= B  # and the feet that landed were held through their stances above


# ---- 8. one tick of the host loop with terrain ----
def test_one_tick_of_the_host_terrain_loop_is_gait_plan_then_the_host_sqp_loop(pkg, oracle):
    sm = pkg.srbd_model
    B, N, T = 2, 6, 1
    p = sm.SrbdParams()
    xs, us, x, alpha, gait, cmd, ref_pose, foot_now = TH.stairs_case(sm, p, B, N, T, 5)
    ter = TH.stairs_terrain(sm)
    out = RH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, 15, "none", p=p, gait=gait, cmd=cmd,
                         ref_pose=ref_pose, foot_now=foot_now, tick0=4, terrain=ter)
    w, pose, feet = sm.gait_plan(p, gait, cmd[:, 0], x, 4, ref_pose, foot_now, N, terrain=ter)
    flat = sm.gait_plan(p, gait, cmd[:, 0], x, 4, ref_pose, foot_now, N)[0]
    assert not np.array_equal(w.foot_r, flat.foot_r) or not np.array_equal(w.foot_l, flat.foot_l)
    for k in FIELDS:
        assert np.array_equal(getattr(out["windows"][0], k), getattr(w, k)), k
    assert np.array_equal(out["ref_pose"], pose) and np.array_equal(out["foot_now"], feet)
    assert np.array_equal(out["foot_log"][:, 0], feet) and np.array_equal(out["fz_log"][:, 0], w.fz_max[:, 0])
    assert np.array_equal(out["q_log"][:, 0], TH.selection(sm, p, gait, ter, cmd[:, 0], x, 4, ref_pose, foot_now, N)[0][:, 0])
    for i in range(B):
        hx, hu, ha, hit, hcv, hm = PH.sqp_loop(sm, oracle, p, w.robot(i), xs[i], us[i], x[i], float(alpha[i]), NMPC,
                                               15, "none")
        sx, su, sa, sit, scv, smg = out["steps"][0][i]
        assert np.array_equal(sx, hx) and np.array_equal(su, hu)
        assert (sa, sit, scv, smg) == (ha, hit, hcv, hm)
        assert np.array_equal(out["u_log"][i, 0], hu[0])
    hxs = np.stack([r[0] for r in out["steps"][0]])
    hus = np.stack([r[1] for r in out["steps"][0]])
    assert np.array_equal(out["x_log"][:, 1], sm.plant_step(x, hus[:, 0], p, w.foot_r[:, 0], w.foot_l[:, 0]))
    sx, su = sm.shift_guess(hxs, hus, p, w)
    assert np.array_equal(out["xs"], sx) and np.array_equal(out["us"], su)
