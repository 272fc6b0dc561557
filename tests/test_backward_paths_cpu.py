"""The designed active sets of tests/backward_designs.py on the CPU: every design that
tests/test_gpu_backward_paths.py runs on the GPU has exactly the active set it was designed to
have by the rule the device uses (adjoint_rows_host.active_rows), no bound near enough to be in
doubt, and on two of them the numpy statement the GPU is held to agrees with central differences
of the equality-held forward solve (step and tolerance of tests/test_backward_rows_cpu.py).

Seen: the largest FD error over the fourteen gradients is 2.6e-8 (upper_lower, QP 0) and 1.2e-8
(saturated, QP 1), against abs 1e-7 asked.
"""
import numpy as np
import pytest

import adjoint_rows_host as arh
import backward_designs as bd
from test_backward_rows_cpu import _fd

CASES = [(name, True) for name in bd.DESIGNS] + [("partial", False), ("all_pinned", False)]


@pytest.mark.parametrize("name,rows", CASES)
def test_design_has_its_active_set(OcpQpBatch, name, rows):
    qp, x0, point = bd.build(name, OcpQpBatch, rows)
    want = bd.counts(name, rows)
    (batch, N, nx, nu, ng, box), _, stages = bd.DESIGNS[name]
    assert (qp.batch, qp.N, qp.nx, qp.nu, qp.ng, qp.has_box_u) == (batch, N, nx, nu, ng if rows else 0, box)
    for i in range(batch):
        x, u, pi = (point[k][i] for k in ("x", "u", "pi"))
        found, cnt, dropped = arh.active_rows(qp, u, bd.ACT_TOL, bd.RANK_TOL, i)
        assert cnt == tuple(want[i]), (name, i, cnt, want[i])
        # the accepted rows, their order and their sides; the dropped rows and their sides
        assert [[a[:3] for a in acc] for acc in found] == bd.held(name, i, rows), (name, i)
        designed = [(k, j, up) for (q, k), s in sorted(stages.items()) if q == i
                    for j, up, kind in s["rows"] if kind != bd.LIVE] if rows else []
        assert dropped == designed, (name, i, dropped, designed)
        # beyond doubt: on the bound or at least 1 away (the GPU tests' rule asks for less)
        dist = bd.distances(qp, u, i)
        assert not np.any((dist > 1e-6) & (dist < 1e-2)), (name, i)
        assert np.all((np.abs(dist) < 1e-9) | (dist >= 1.0)), (name, i, dist[(np.abs(dist) >= 1e-9) & (dist < 1.0)])
        assert int(np.sum(np.abs(dist) < 1e-9)) == cnt[0] + cnt[1] + cnt[2]
        # the point is the equality-held QP's: dynamics and x0 hold
        assert np.allclose(x[0], x0[i], atol=1e-12)
        step = np.einsum("kij,kj->ki", qp.A[i], x[:-1]) + np.einsum("kij,kj->ki", qp.B[i], u) + qp.b[i]
        assert np.allclose(step, x[1:], atol=1e-10)
    assert want.sum() > 0


def test_masked_bounds_sit_on_the_point(OcpQpBatch):
    """The masked design's masked-off bounds would be active: with the masks set again, the rule
    finds them (so the GPU test fails if a kernel forgets a mask)."""
    qp, x0, point = bd.build("masked", OcpQpBatch)
    for m in ("lbu_mask", "ubu_mask", "lg_mask", "ug_mask"):
        setattr(qp, m, np.ones_like(getattr(qp, m)))
    _, _, stages = bd.DESIGNS["masked"]
    extra = np.zeros(3, dtype=int)
    for (i, _), s in stages.items():
        extra[i] += len(s["off_pins"]) + len(s["off_rows"])
    assert np.all(extra > 0)
    want = bd.counts("masked")
    for i in range(qp.batch):
        _, cnt, _ = arh.active_rows(qp, point["u"][i], bd.ACT_TOL, bd.RANK_TOL, i)
        assert sum(cnt) == want[i].sum() + extra[i], (i, cnt)


@pytest.mark.parametrize("name,i", [("upper_lower", 0), ("saturated", 1)])
def test_statement_matches_finite_differences(OcpQpBatch, name, i):
    """All fourteen gradients of one QP of a 12 x 12 design and of the small saturated one (a pin,
    two accepted and three dropped rows in one stage) to abs 1e-7."""
    qp, x0, point = bd.build(name, OcpQpBatch)
    rng = np.random.default_rng(5)
    gx, gu = rng.uniform(-1, 1, (qp.N + 1, qp.nx)), rng.uniform(-1, 1, (qp.N, qp.nu))
    got, cnt = arh.adjoint_rows_host(qp, point["x"][i], point["u"][i], point["pi"][i], gx, gu, i, bd.ACT_TOL,
                                     bd.RANK_TOL)
    assert cnt == tuple(bd.counts(name)[i])
    one = qp.subset([i])
    stages, _, _ = arh.active_rows(one, point["u"][i], bd.ACT_TOL, bd.RANK_TOL, 0)
    want = _fd(one, x0[i].copy(), gx, gu, stages)
    worst = 0.0
    for n in arh.ALL_NAMES:
        err = float(np.max(np.abs(got[n] - want[n])))
        worst = max(worst, err)
        assert err <= 1e-7, (name, n, err)
    print(f"[backward designs fd] {name} QP {i}: worst {worst:.2e}")
