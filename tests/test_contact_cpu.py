"""The plant's contact model (srbd_qp_srbd_set_contact_f64) without a GPU: the entry point is
exported and checks its arguments' holders, and the host statement srbd_model.contact_project /
plant_step(contact=...) has the properties include/srbd_qp.h states.  Without a contact the plant
step is the function it was; the projection is idempotent, its output satisfies every limit,
generous limits change nothing, a swing foot transmits nothing, and the sat bits are what a
brute-force recomputation finds; a lateral force far above mu fz moves the velocity by the
projected force's dt F / m; and the fall detector freezes, counts and flags as stated."""
import dataclasses
import subprocess

import numpy as np
import pytest

import contact_host as CH
import rollout_host as RH

CONTACT_SYMBOLS = ("srbd_qp_srbd_set_contact_f64",)


def commanded(B, seed):
    """Inputs that break every limit somewhere: negative and huge fz, lateral forces and torques
    on both sides of their bounds."""
    rng = np.random.default_rng(seed)
    u = np.empty((B, 2, 6))
    u[..., 0:2] = rng.uniform(-60.0, 60.0, size=(B, 2, 2))
    u[..., 2] = rng.uniform(-40.0, 260.0, size=(B, 2))
    u[..., 3:6] = rng.uniform(-6.0, 6.0, size=(B, 2, 3))
    return u.reshape(B, 12)


def a_contact(sm, B, seed, **kw):
    rng = np.random.default_rng(seed)
    return sm.SrbdContact(mu=0.4, mu_r=rng.uniform(0.0, 0.9, size=B), Lt=(0.0, 0.04, 0.07), fz_hi=180.0,
                          fz_contact=5.0, **kw)


# ---- 1. the entry point exists ----
def test_contact_entry_point_is_exported(pkg):
    capi = pkg.capi
    assert set(CONTACT_SYMBOLS) <= set(capi.exported_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    assert set(CONTACT_SYMBOLS) <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = capi.lib()
    assert L.srbd_qp_srbd_set_contact_f64(None, None) == -1
    assert L.srbd_qp_abi_version() == 12  # additive to ABI 12
    import torch
    with pytest.raises(ValueError, match="torch.float64"):
        capi.Contact(mu_r=torch.zeros(3, dtype=torch.float32)).struct()
    with pytest.raises(ValueError, match="is on cpu"):
        capi.Contact(mu_r=torch.zeros(3, dtype=torch.float64)).struct()
    with pytest.raises(ValueError, match="torch.int32"):
        capi.Contact(fallen=torch.zeros(3, dtype=torch.float32)).struct()
    with pytest.raises(ValueError, match="is on cpu"):
        capi.Contact(fallen=torch.zeros(3, dtype=torch.int32)).struct()
    with pytest.raises(ValueError, match="torch.float64"):
        capi.Contact(ground=capi.Terrain(torch.zeros(3, 4, dtype=torch.float32), 0.0, 0.0, 1.0)).struct()
    with pytest.raises(ValueError, match="is on cpu"):
        capi.Contact(ground=capi.Terrain(torch.zeros(3, 4, dtype=torch.float64), 0.0, 0.0, 1.0)).struct()
    # the struct's layout is the header's: 8 doubles / pointers, the terrain, 2 doubles, 3 pointers
    assert C_sizeof(capi.ContactStruct) == 8 * 8 + C_sizeof(capi.TerrainStruct) + 2 * 8 + 3 * 8


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


# ---- 2. without a contact the plant step is the function it was ----
def test_plant_step_without_a_contact_has_the_old_bits(pkg):
    sm = pkg.srbd_model
    B, N = 6, 4
    p = sm.SrbdParams()
    xs, us, dx0 = sm.sample_trajectories(B, N, 11, p)
    x, u = xs[:, 0] + dx0, us[:, 0]
    rng = np.random.default_rng(12)
    fr = np.array(p.foot_r) + rng.uniform(-0.1, 0.1, size=(B, 3))
    fl = np.array(p.foot_l) + rng.uniform(-0.1, 0.1, size=(B, 3))
    w = rng.uniform(-20.0, 20.0, size=(B, 6))
    for substeps in (1, 3):
        # the old call, restated: `substeps` RK4 steps of the model with the input as it is
        want = x
        for _ in range(substeps):
            want = sm._rk4_step(want, u, p, p.dt / substeps, sm.SrbdPlan(foot_r=fr, foot_l=fl), w)
        assert np.array_equal(sm.plant_step(x, u, p, fr, fl, w, substeps), want)
        got = sm.plant_step(x, u, p, fr, fl, w, substeps, contact=None, in_contact=None, state=None)
        assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    assert np.array_equal(sm.plant_step(x, u, p), sm._rk4_step(x, u, p, p.dt, None))


# ---- 3. the projection ----
def test_projection_is_idempotent_and_satisfies_every_limit(pkg):
    sm = pkg.srbd_model
    B = 64
    u = commanded(B, 21)
    c = a_contact(sm, B, 22)
    on = np.random.default_rng(23).uniform(size=(B, 2)) < 0.7
    up, sat = sm.contact_project(u, c, on, c.mu_r)
    up2, sat2 = sm.contact_project(up, c, on, c.mu_r)
    assert np.array_equal(up2, up) and not sat2.any()
    for f in range(2):
        o = 6 * f
        fz = up[:, o + 2]
        assert (fz >= 0.0).all() and (fz <= c.fz_hi).all()
        assert (fz[~on[:, f]] == 0.0).all()
        assert (np.abs(up[:, o]) <= c.mu_r * fz).all() and (np.abs(up[:, o + 1]) <= c.mu_r * fz).all()
        for a in range(3):
            assert (np.abs(up[:, o + 3 + a]) <= c.Lt[a] * fz).all()
        # a swing foot's six entries are zero
        assert (up[~on[:, f], o:o + 6] == 0.0).all() and (~on[:, f]).any()
    assert sat.dtype == np.uint32 and np.bitwise_or.reduce(sat) == 0xFF  # every limit bit somewhere


def test_generous_limits_return_the_input_bit_for_bit(pkg):
    sm = pkg.srbd_model
    B = 32
    u = commanded(B, 31)
    u[:, [2, 8]] = np.abs(u[:, [2, 8]])  # fz >= 0
    c = sm.SrbdContact(mu=1e6, Lt=(1e6, 1e6, 1e6), fz_hi=np.inf)
    up, sat = sm.contact_project(u, c, np.ones((B, 2), dtype=bool), c.mu)
    assert up.tobytes() == u.tobytes() and not sat.any()


def test_sat_bits_match_a_brute_force_recomputation(pkg):
    sm = pkg.srbd_model
    B = 64
    u = commanded(B, 41)
    c = a_contact(sm, B, 42)
    on = np.random.default_rng(43).uniform(size=(B, 2)) < 0.6
    up, sat = sm.contact_project(u, c, on, c.mu_r)
    for i in range(B):
        bits = 0
        for f in range(2):
            o = 6 * f
            fz, mu = float(u[i, o + 2]), float(c.mu_r[i])
            fzp = min(max(fz, 0.0), c.fz_hi) if on[i, f] else 0.0
            assert up[i, o + 2] == fzp
            if fzp != fz:
                bits |= (1 if (not on[i, f] or fzp > fz) else 2) << (4 * f)
            lat = [min(max(float(u[i, o + j]), -(mu * fzp)), mu * fzp) for j in range(2)]
            assert list(up[i, o:o + 2]) == lat
            if lat != [float(u[i, o]), float(u[i, o + 1])]:
                bits |= 4 << (4 * f)
            tq = [min(max(float(u[i, o + 3 + a]), -(c.Lt[a] * fzp)), c.Lt[a] * fzp) for a in range(3)]
            assert list(up[i, o + 3:o + 6]) == tq
            if tq != [float(v) for v in u[i, o + 3:o + 6]]:
                bits |= 8 << (4 * f)
        assert int(sat[i]) == bits, (i, hex(int(sat[i])), hex(bits))


# ---- 4. friction limits the lateral force: dv = dt F' / m + dt g, in closed form ----
def test_a_lateral_force_above_mu_fz_moves_the_velocity_by_the_projected_force(pkg):
    sm = pkg.srbd_model
    B = 5
    p = sm.SrbdParams()
    rng = np.random.default_rng(51)
    x = np.zeros((B, 12))  # zero rotation and momentum
    x[:, 6:9] = np.array([0.5, 0.0, 1.0]) + rng.uniform(-0.05, 0.05, size=(B, 3))
    u = np.zeros((B, 12))
    fz = rng.uniform(60.0, 90.0, size=(B, 2))
    u[:, 2], u[:, 8] = fz[:, 0], fz[:, 1]
    sign = np.where(rng.uniform(size=(B, 2)) < 0.5, -1.0, 1.0)  # per axis, both feet alike
    lat = sign[:, None, :] * rng.uniform(500.0, 900.0, size=(B, 2, 2))  # far above mu fz
    u[:, 0:2], u[:, 6:8] = lat[:, 0], lat[:, 1]
    mu = rng.uniform(0.05, 0.6, size=B)
    c = sm.SrbdContact(mu_r=mu, Lt=(1.0, 1.0, 1.0))
    x1, ua, st = sm.plant_step(x, u, p, contact=c, state=CH.zero_state(B))
    F = np.empty((B, 3))
    F[:, 0:2] = sign * (mu * fz[:, 0])[:, None] + sign * (mu * fz[:, 1])[:, None]
    F[:, 2] = fz[:, 0] + fz[:, 1]
    assert np.array_equal(ua[:, 0:2], sign * (mu * fz[:, 0])[:, None])
    assert np.array_equal(ua[:, 6:8], sign * (mu * fz[:, 1])[:, None])
    assert (st["sat"] == ((4 << 4) | 4)).all() and not st["fallen"].any() and (st["alive"] == 1).all()
    want = p.dt * (F / p.mass + np.array([0.0, 0.0, -9.8]))
    np.testing.assert_allclose(x1[:, 9:12] - x[:, 9:12], want, rtol=1e-12, atol=0.0)
    # the unprojected plant would have moved it by the commanded force
    free = sm.plant_step(x, u, p)
    assert (np.abs(free[:, 9:11]) > 2.0 * np.abs(x1[:, 9:11])).all()


# ---- 5. the fall detector ----
def test_fall_detection_freezes_counts_and_flags(pkg):
    sm = pkg.srbd_model
    B, N = 6, 4
    p = sm.SrbdParams()
    xs, us, dx0 = sm.sample_trajectories(B, N, 61, p)
    x, u = xs[:, 0] + dx0, us[:, 0].copy()
    x[1, 8] = 0.2           # below z_min
    x[2, 0] = 1.4           # tilted: cos(1.4) < 0.5
    u[3, 4] = np.nan        # a non-finite input
    u[4, 8] = np.inf
    c = sm.SrbdContact(mu=0.5, Lt=(0.0, 0.05, 0.05), fz_hi=500.0, z_min=0.5, cos_tilt_min=0.5)
    state = CH.zero_state(B)
    state["fallen"][5] = 1  # fallen on entry
    state["alive"][:] = 7
    state["sat"][5] = 0x80
    x1, ua, st = sm.plant_step(x, u, p, contact=c, state=state)
    assert list(st["fallen"]) == [0, 1, 1, 1, 1, 1]
    assert list(st["alive"]) == [8, 7, 7, 7, 7, 7]
    assert st["sat"][5] == 0x80 and state["alive"][0] == 7  # the inputs are left alone
    for i in (3, 4, 5):  # frozen: x keeps its bits, nothing is applied
        assert x1[i].tobytes() == x[i].tobytes() and not ua[i].any()
    for i in (0, 1, 2):  # stepped (a robot that falls on a finite state keeps that state)
        one = sm.plant_step(x[i:i + 1], u[i:i + 1], p, contact=c)
        assert np.array_equal(x1[i], one[0][0]) and np.array_equal(ua[i], one[1][0])
        assert not np.array_equal(x1[i], x[i])
    above, r33 = sm.fall_values(x1, c)
    assert above[1] < c.z_min < above[0] and r33[2] < c.cos_tilt_min < r33[0]
    # without `fallen` nothing is tested or counted
    x2, ua2, st2 = sm.plant_step(x[:3], u[:3], p, contact=c, state={"sat": np.zeros(3, dtype=np.uint32)})
    assert set(st2) == {"sat"} and np.array_equal(x2, x1[:3])
    with pytest.raises(ValueError, match="alive needs fallen"):
        sm.plant_step(x, u, p, contact=c, state={"alive": np.zeros(B, dtype=np.int32)})


# ---- 6. the true ground moves the feet in contact, and only those ----
def test_true_ground_moves_the_feet_in_contact(pkg):
    sm = pkg.srbd_model
    B = 4
    p = sm.SrbdParams()
    xs, us, dx0 = sm.sample_trajectories(B, 3, 71, p)
    x, u = xs[:, 0] + dx0, us[:, 0]
    rng = np.random.default_rng(72)
    H = rng.uniform(-0.05, 0.05, size=(2, 5, 6))
    g = sm.SrbdTerrain(height=H, x0=0.2, y0=-0.4, cell=0.2, map_r=np.arange(B) % 2)
    fr = np.array(p.foot_r) + np.array([0.5, 0.0, 0.0]) + rng.uniform(-0.1, 0.1, size=(B, 3))
    fl = np.array(p.foot_l) + np.array([0.5, 0.0, 0.0]) + rng.uniform(-0.1, 0.1, size=(B, 3))
    on = np.array([[True, True], [True, False], [False, True], [True, True]])
    c = sm.SrbdContact(mu=0.5, Lt=(1.0, 1.0, 1.0), ground_z=0.02, ground=g)
    x1, ua, _ = sm.plant_step(x, u, p, fr, fl, contact=c, in_contact=on)
    fr2, fl2 = fr.copy(), fl.copy()
    fr2[:, 2] = np.where(on[:, 0], 0.02 + sm.terrain_height(g, fr[:, 0:2], g.map_r), fr[:, 2])
    fl2[:, 2] = np.where(on[:, 1], 0.02 + sm.terrain_height(g, fl[:, 0:2], g.map_r), fl[:, 2])
    flat = dataclasses.replace(c, ground=None)
    want = sm.plant_step(x, u, p, fr2, fl2, contact=flat, in_contact=on)
    assert np.array_equal(x1, want[0]) and np.array_equal(ua, want[1])
    assert not np.array_equal(x1, sm.plant_step(x, u, p, fr, fl, contact=flat, in_contact=on)[0])
    # per-robot slices (tests/contact_host.py) are the batch
    per = RH.plant_step(sm, [p] * B, x, u, fr, fl, contact=c, in_contact=on, state=CH.zero_state(B))
    whole = sm.plant_step(x, u, p, fr, fl, contact=c, in_contact=on, state=CH.zero_state(B))
    assert np.array_equal(per[0], whole[0]) and np.array_equal(per[1], whole[1])
    assert all(np.array_equal(per[2][k], whole[2][k]) for k in whole[2])
