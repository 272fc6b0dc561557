"""Per-robot model and plant parameters (srbd_qp_srbd_set_robots_f64) without a GPU: the entry
point exists and validates, the binding checks its tensors before the library sees them, and
tests/rollout_host.py's closed loop with per-robot lists is the loop with one SrbdParams when
every robot has the same parameters."""
import ctypes as C
import dataclasses
import subprocess

import numpy as np
import pytest

import robots_host as BH
import rollout_host as RH
from srbd_device import NMPC

EINVAL = -1  # SRBD_QP_EINVAL


def test_set_robots_is_exported_and_rejects_a_null_handle(pkg):
    capi = pkg.capi
    name = "srbd_qp_srbd_set_robots_f64"
    assert name in capi.exported_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    assert name in {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = capi.lib()
    rs = capi.RobotsStruct()
    for role in (0, 1, 2):
        assert L.srbd_qp_srbd_set_robots_f64(None, role, C.byref(rs)) == EINVAL
        assert L.srbd_qp_srbd_set_robots_f64(None, role, None) == EINVAL
    assert L.srbd_qp_abi_version() == 12  # additive to ABI 12


def test_robots_binding_checks_its_tensors(pkg):
    import torch
    capi = pkg.capi
    B = 4
    f = dict(dtype=torch.float64)
    with pytest.raises(ValueError, match="mass has shape"):
        capi.Robots(mass=torch.ones(B, 1, **f)).struct("model")
    with pytest.raises(ValueError, match="Lbody has shape"):
        capi.Robots(Lbody=torch.ones(B, 4, **f)).struct("model")
    with pytest.raises(ValueError, match="Q has shape"):
        capi.Robots(Q=torch.ones(B, **f)).struct("model")
    with pytest.raises(ValueError, match="Qf has shape"):
        capi.Robots(Qf=torch.ones(12, B, **f)).struct("model")
    with pytest.raises(ValueError, match="mu must be a torch.float64"):
        capi.Robots(mu=torch.ones(B, dtype=torch.float32)).struct("model")
    with pytest.raises(ValueError, match="R must be a torch.float64"):
        capi.Robots(R=np.ones(B)).struct("model")
    with pytest.raises(ValueError, match="Lbody must be contiguous"):
        capi.Robots(Lbody=torch.ones(3, B, **f).t()).struct("plant")
    # a host tensor is on the wrong device, whatever the handle's
    with pytest.raises(ValueError, match="mass is on cpu"):
        capi.Robots(mass=torch.ones(B, **f)).struct("model")
    with pytest.raises(ValueError, match="unknown robots role"):
        capi.Robots().struct("robot")
    # the plant role takes mass and Lbody only
    for name, shape in (("mu", (B,)), ("Q", (B, 12)), ("Qf", (B, 12)), ("R", (B,))):
        with pytest.raises(ValueError, match=f"{name}: the plant role"):
            capi.Robots(**{name: torch.ones(*shape, **f)}).struct("plant")
    # nothing set is a valid, empty struct for either role
    for role in ("model", "plant"):
        rs = capi.Robots().struct(role)
        assert all(getattr(rs, n) is None for n in ("mass", "Lbody", "mu", "Q", "Qf", "R"))


def test_the_draw_changes_all_six_fields_and_nothing_else(pkg):
    sm = pkg.srbd_model
    p = sm.SrbdParams()
    model = BH.draw(p, 5, 126)
    assert model == BH.draw(p, 5, 126) and model[:3] == BH.draw(p, 3, 126)
    for q in model:
        assert 10.0 <= q.mass <= 20.0 and 0.3 <= q.mu <= 0.8 and 0.5 * p.R <= q.R <= 2.0 * p.R
        assert all(getattr(q, f) != getattr(p, f) for f in BH.MODEL_FIELDS)
        assert dataclasses.replace(q, **{f: getattr(p, f) for f in BH.MODEL_FIELDS}) == p
    plant = BH.draw_plant(model, 141)
    for q, m in zip(plant, model):
        assert 0.8 * m.mass <= q.mass <= 1.25 * m.mass and q.Lbody != m.Lbody
        assert dataclasses.replace(q, mass=m.mass, Lbody=m.Lbody) == m
    a = BH.arrays(model)
    assert [a[f].shape for f in BH.MODEL_FIELDS] == [(5,), (5, 3), (5,), (5, 12), (5, 12), (5,)]
    one = BH.only(p, model, ("mu",))
    assert all(q.mu == m.mu and dataclasses.replace(q, mu=p.mu) == p for q, m in zip(one, model))


@pytest.mark.parametrize("alpha_reset", [0.0, 1.0])
def test_identical_robots_give_the_bits_of_the_shared_closed_loop(pkg, oracle, alpha_reset):
    sm = pkg.srbd_model
    B, N, T = 2, 6, 2
    p = dataclasses.replace(sm.SrbdParams(), mass=13.0, mu=0.6)
    xs, us, x, alpha, plan = RH.walking_case(sm, p, B, N, T, 5)
    wrench = np.random.default_rng(6).uniform(-15.0, 15.0, size=(B, T, 6))
    loop = lambda **params: RH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, 15, "none", plan=plan, wrench=wrench,
                                           substeps=2, alpha_reset=alpha_reset, **params)
    want = loop(p=p)
    got = loop(model=[p] * B, plant=[p] * B)
    for k in ("x_log", "u_log", "sqp_iter", "converged", "xs", "us", "x", "alpha"):
        assert np.array_equal(got[k], want[k]), k
    assert got["margin"] == want["margin"]
    # and the plant list is what moves the plant: a heavier true robot ends elsewhere
    heavy = [dataclasses.replace(p, mass=1.2 * p.mass)] * B
    other = loop(model=[p] * B, plant=heavy)
    assert np.array_equal(other["u_log"][:, 0], want["u_log"][:, 0])  # the first step saw the same x
    assert not np.array_equal(other["x_log"][:, 1], want["x_log"][:, 1])
