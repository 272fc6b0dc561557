"""Soft box constraints, CPU side: the OcpQpBatch fields and the lift (tests/soft_lift.py)
that turns a soft QP into a hard one for the CPU oracle."""
import numpy as np
import pytest

import helpers
import soft_lift

TIGHT = dict(iter_max=50)


def _family(OcpQpBatch, nx=4, nu=2, N=5, batch=16, seed=3):
    qp, x0 = helpers.random_constrained(batch, N, nx, nu, 0, seed, OcpQpBatch)
    return soft_lift.tighten(qp), x0


def test_soft_fields_shape_checks(OcpQpBatch):
    qp, _ = _family(OcpQpBatch)
    assert not qp.has_soft
    soft_lift.soften_x(qp, (1, 3), 1.0, 1.0)
    assert qp.has_soft
    qp.check()
    for name in ("soft_x", "Zl_x", "zu_x"):
        good = getattr(qp, name)
        setattr(qp, name, good[:, :-1])
        with pytest.raises(ValueError, match=name):
            qp.check()
        setattr(qp, name, good)
    qp.lls_x = np.zeros((qp.batch, qp.N + 1, qp.nx + 1))
    with pytest.raises(ValueError, match="lls_x"):
        qp.check()
    qp.lls_x = None
    qp.soft_u = np.zeros((qp.batch, qp.N + 1, qp.nu))
    with pytest.raises(ValueError, match="soft_u"):
        qp.check()
    qp.soft_u = None
    qp.Zl_u = np.zeros((qp.batch, qp.N, qp.nu))
    with pytest.raises(ValueError, match="requires soft_u"):
        qp.check()


def test_soft_x_needs_box_x(OcpQpBatch):
    qp, _ = helpers.random_unconstrained(2, 3, 4, 2, 1, OcpQpBatch)
    qp.soft_x = np.ones((2, 4, 4))
    with pytest.raises(ValueError, match="soft_x requires lbx"):
        qp.check()
    qp.soft_x = None
    qp.soft_u = np.ones((2, 3, 2))
    with pytest.raises(ValueError, match="soft_u requires lbu"):
        qp.check()


def test_packed_and_subset_carry_soft_fields(OcpQpBatch):
    qp, _ = _family(OcpQpBatch)
    soft_lift.soften_x(qp, (1, 3), 2.0, 3.0)
    qp.lls_x = np.full(qp.soft_x.shape, -0.5)
    p = qp.packed()
    for name in ("soft_x", "Zl_x", "Zu_x", "zl_x", "zu_x", "lls_x"):
        assert p[name].dtype == np.float64 and p[name].flags.c_contiguous
        assert np.array_equal(p[name], getattr(qp, name))
    assert p["lus_x"] is None  # NULL = 0
    assert "soft_u" not in p  # no soft u family
    sub = qp.subset(np.array([3, 1]))
    assert sub.has_soft and sub.batch == 2
    assert np.array_equal(sub.soft_x, qp.soft_x[[3, 1]])
    assert np.array_equal(sub.lls_x, qp.lls_x[[3, 1]])
    assert sub.soft_u is None
    # a hard batch packs exactly what it packed before
    hard, _ = _family(OcpQpBatch)
    assert not any(k.startswith(("soft_", "Zl_", "Zu_", "zl_", "zu_", "lls_", "lus_")) for k in hard.packed())


@pytest.mark.parametrize("ric_alg", [0, 1])
def test_fixture_hard_fails_lifted_succeeds(OcpQpBatch, oracle, ric_alg):
    """Pins the fixture: the tightened boxes are infeasible as hard constraints for most
    QPs, and every QP solves once they are soft."""
    qp, x0 = _family(OcpQpBatch)
    st = dict(TIGHT, ric_alg=ric_alg)
    hard = oracle.solve(qp, st, x0=x0, riccati=False)
    assert int(np.sum(hard["status"] != 0)) >= 12, hard["status"]
    soft_lift.soften_x(qp, (1, 3), 1.0, 1.0)
    lifted, split = soft_lift.lift(qp, OcpQpBatch)
    assert lifted.nu == qp.nu + 4 and lifted.ng == 4 and lifted.N == qp.N + 1  # (soft x_N: dummy stage)
    sol = split(oracle.solve(lifted, st, x0=x0, riccati=False))
    assert np.all(sol["status"] == 0), sol["status"]
    assert sol["iter"].min() >= 5 and sol["iter"].max() <= 20, sol["iter"]
    # the slacks take up exactly the violation of the +-0.02 box
    x = sol["x"]
    for i in (1, 3):
        viol_l = np.maximum(-0.02 - x[:, 1:, i], 0.0)
        viol_u = np.maximum(x[:, 1:, i] - 0.02, 0.0)
        assert np.all(sol["sl_x"][:, 1:, i] >= viol_l - 1e-6)
        assert np.all(sol["su_x"][:, 1:, i] >= viol_u - 1e-6)
    assert np.all(sol["sl_x"] >= -1e-9) and np.all(sol["su_x"] >= -1e-9)
    assert np.all(sol["sl_x"][:, 0] == 0) and np.all(sol["sl_u"] == 0)


def test_split_round_trips(OcpQpBatch):
    qp, x0 = _family(OcpQpBatch, nx=4, nu=3, N=3, batch=2)
    soft_lift.soften_x(qp, (1,), 1.0, 1.0)
    qp.soft_u = np.zeros((2, 3, 3)); qp.soft_u[:, :, 2] = 1.0
    for n in ("Zl_u", "Zu_u", "zl_u", "zu_u"):
        setattr(qp, n, np.ones((2, 3, 3)))
    lifted, split = soft_lift.lift(qp, OcpQpBatch)
    # slots: (u, 2), (x, 1); the dummy stage carries x_N's slacks
    assert (lifted.N, lifted.nu, lifted.ng) == (4, 3 + 4, 4)
    rng = np.random.default_rng(0)
    fake = {"x": rng.normal(size=(2, 5, 4)), "pi": rng.normal(size=(2, 5, 4)),
            "u": rng.normal(size=(2, 4, 7)), "status": np.zeros(2, dtype=np.int32)}
    s = split(fake)
    assert s["x"].shape == (2, 4, 4) and s["u"].shape == (2, 3, 3)
    assert np.array_equal(s["u"], fake["u"][:, :3, :3])
    assert np.array_equal(s["sl_u"][:, :, 2], fake["u"][:, :3, 3])
    assert np.array_equal(s["su_u"][:, :, 2], fake["u"][:, :3, 4])
    assert np.array_equal(s["sl_x"][:, :, 1], fake["u"][:, :, 5])
    assert np.array_equal(s["su_x"][:, :, 1], fake["u"][:, :, 6])
    assert not s["sl_x"][:, :, [0, 2, 3]].any() and not s["sl_u"][:, :, :2].any()
    # the lifted rows: lb <= x_1 + sl, x_1 - su <= ub at stage 2 of QP 0
    assert lifted.C[0, 2, 2, 1] == 1 and lifted.D[0, 2, 2, 5] == 1 and lifted.ug_mask[0, 2, 2] == 0
    assert lifted.C[0, 2, 3, 1] == 1 and lifted.D[0, 2, 3, 6] == -1 and lifted.lg_mask[0, 2, 3] == 0
    assert lifted.lg[0, 2, 2] == qp.lbx[0, 2, 1] and lifted.ug[0, 2, 3] == qp.ubx[0, 2, 1]
    assert lifted.lbx_mask[0, 2, 1] == 0 and lifted.lbx_mask[0, 2, 3] == 1  # soft box leaves the hard set


@pytest.mark.parametrize("N", [1, 2])
def test_dummy_stage_lift_with_soft_terminal_bounds(OcpQpBatch, oracle, N):
    qp, x0 = _family(OcpQpBatch, N=N, batch=4)
    soft_lift.soften_x(qp, (1, 3), 10.0, 0.1)
    lifted, split = soft_lift.lift(qp, OcpQpBatch)
    assert lifted.N == N + 1
    sol = split(oracle.solve(lifted, TIGHT, x0=x0, riccati=False))
    assert np.all(sol["status"] == 0), sol["status"]
    assert sol["x"].shape == (4, N + 1, 4) and sol["sl_x"].shape == (4, N + 1, 4)
    # the dummy stage costs nothing: the objective is the soft QP's own
    x, u = sol["x"], sol["u"]
    obj = np.zeros(4)
    for k in range(N + 1):
        obj += 0.5 * np.einsum("bi,bij,bj->b", x[:, k], qp.Q[:, k], x[:, k]) + np.einsum("bi,bi->b", qp.q[:, k], x[:, k])
        if k < N:
            obj += 0.5 * np.einsum("bi,bij,bj->b", u[:, k], qp.R[:, k], u[:, k]) + np.einsum("bi,bi->b", qp.r[:, k], u[:, k])
            obj += np.einsum("bi,bij,bj->b", u[:, k], qp.S[:, k], x[:, k])
    for s in ("sl_x", "su_x"):
        obj += np.sum(0.5 * 0.1 * sol[s] ** 2 + 10.0 * sol[s], axis=(1, 2))
    # (the oracle's objective leaves out the x0 terms it embeds; compare without stage 0's)
    obj0 = 0.5 * np.einsum("bi,bij,bj->b", x[:, 0], qp.Q[:, 0], x[:, 0]) + np.einsum("bi,bi->b", qp.q[:, 0], x[:, 0])
    assert np.allclose(sol["obj"], obj - obj0, rtol=1e-6, atol=1e-6)
