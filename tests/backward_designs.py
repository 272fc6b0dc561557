"""Batches whose active set is designed, not drawn, for the tests of the backward pass.

tests/test_gpu_backward*.py draw bounds, solve with the IPM and leave out the QPs whose active set
is unclear, which cannot aim at an edge of the kernels.  Here a design says per stage which inputs
are pinned at which side and which rows of D are active at which side, and build() returns a batch
and a point (x, u, pi) at which exactly that holds:

1. the QP is helpers.random_constrained's, without C and the state boxes;
2. the designed pins and the designed independent rows get small random bounds and are held as
   equalities: (x, u, pi) = adjoint_rows_host.forward_rows_host.  It is the KKT point of that
   equality-held QP; the sign of a multiplier is not looked at, since the backward pass reads the
   active set from the distances to the bounds alone;
3. every other bound is put 1 to 2 away from u (or D u) at that point;
4. a designed row that cannot be accepted (a copy of an earlier active row, a row of a stage
   whose inputs are all pinned, a row beyond nu accepted ones) is active too: its bound is its own
   value D_j u at the point;
5. a masked design entry has its bound on the point and its mask cleared.

So no QP has a distance to an unmasked bound in (1e-6, 1e-2), and none is left out of a comparison.
tests/test_backward_paths_cpu.py holds every design to that and to its counts.
"""
import numpy as np

import adjoint_rows_host as arh
import helpers

ACT_TOL, RANK_TOL = 1e-4, 1e-8
LO, HI = False, True  # the side of a bound: `upper` of adjoint_rows_host.active_rows
LIVE, DROP = "live", "drop"  # a designed row is accepted / is not; an int j0: a copy of row j0 (< j)


def stage(pins=None, rows=(), off_pins=None, off_rows=None):
    """pins {input: side}; rows [(row, side, LIVE | DROP | j0)], ascending; off_pins {input: side}
    and off_rows {row: side}: bounds on the point that are masked off."""
    return dict(pins=dict(pins or {}), rows=list(rows), off_pins=dict(off_pins or {}), off_rows=dict(off_rows or {}))


MIXED = {c: (c * 5) % 3 == 0 for c in range(12)}  # twelve pins, HI on 0, 3, 6, 9

# name -> ((batch, N, nx, nu, ng, boxes), seed, {(qp, k): stage}).  The rows kernels give eight
# stages qp N + k to a workgroup (qp_backward_rows.hip: kStages).
DESIGNS = {
    # 15 stages: workgroup 0 ends inside QP 2 (stages 6, 7 | 8), whose counts are therefore summed
    # by atomics of two workgroups, and workgroup 1 is partial (seven stages, the last ones 13, 14)
    "partial": ((5, 3, 12, 12, 4, True), 41, {
        (0, 1): stage(rows=[(1, LO, LIVE)]),
        (2, 0): stage({3: LO}, [(0, HI, LIVE)]),
        (2, 1): stage({0: HI}, [(2, LO, LIVE), (3, HI, LIVE)]),
        (2, 2): stage({5: LO, 7: HI}, [(1, LO, LIVE)]),
        (4, 1): stage({2: HI}, [(0, LO, LIVE), (3, LO, 0)]),
        (4, 2): stage({11: LO}, [(1, HI, LIVE), (2, LO, LIVE)]),
    }),
    "n1": ((3, 1, 12, 12, 3, True), 42, {
        (0, 0): stage({0: LO}, [(0, LO, LIVE), (2, HI, LIVE)]),
        (1, 0): stage(rows=[(1, HI, LIVE)]),
        (2, 0): stage({4: HI, 9: LO}),
    }),
    "ng1": ((3, 2, 12, 12, 1, False), 43, {
        (0, 0): stage(rows=[(0, LO, LIVE)]),
        (1, 1): stage(rows=[(0, HI, LIVE)]),
        (2, 0): stage(rows=[(0, LO, LIVE)]),
        (2, 1): stage(rows=[(0, HI, LIVE)]),
    }),
    "odd": ((5, 3, 12, 12, 5, True), 44, {
        (0, 0): stage(rows=[(0, LO, LIVE), (4, HI, LIVE)]),
        (1, 2): stage({1: LO}, [(2, HI, LIVE), (3, HI, 2)]),
        (2, 1): stage(rows=[(4, LO, LIVE)]),
        (3, 0): stage({6: HI}),
        (4, 2): stage(rows=[(1, HI, LIVE), (3, LO, LIVE), (4, HI, LIVE)]),
    }),
    "wide_u": ((5, 3, 3, 5, 2, True), 45, {
        (0, 0): stage(rows=[(0, LO, LIVE)]),
        (1, 1): stage({4: HI}, [(1, LO, LIVE)]),
        (2, 2): stage({0: LO, 3: HI}, [(0, HI, LIVE), (1, LO, LIVE)]),
        (3, 0): stage(rows=[(0, LO, LIVE), (1, HI, LIVE)]),
        (4, 1): stage({2: LO}),
    }),
    "tall_x": ((5, 3, 12, 4, 3, True), 46, {
        (0, 1): stage(rows=[(0, LO, LIVE), (2, HI, LIVE)]),
        (1, 0): stage({3: HI}, [(1, LO, LIVE)]),
        (2, 2): stage({0: LO, 1: HI}),
        (3, 1): stage(rows=[(0, HI, LIVE), (1, HI, LIVE), (2, LO, LIVE)]),
        (4, 2): stage({2: LO}, [(2, HI, LIVE)]),
    }),
    # stage (1, 1): no coordinate is free, so both active rows are dropped
    "all_pinned": ((3, 3, 12, 12, 4, True), 47, {
        (0, 0): stage({1: LO}, [(1, HI, LIVE)]),
        (1, 1): stage(MIXED, [(0, LO, DROP), (2, HI, DROP)]),
        (2, 2): stage(rows=[(3, LO, LIVE)]),
    }),
    # stage (1, 0): a pin and two rows fill nu = 3, the other three rows meet nacc >= nu;
    # stage (0, 1): three rows alone fill it
    "saturated": ((4, 2, 5, 3, 5, True), 48, {
        (0, 1): stage(rows=[(0, HI, LIVE), (3, LO, LIVE), (4, HI, LIVE)]),
        (1, 0): stage({1: LO}, [(0, LO, LIVE), (1, HI, LIVE), (2, LO, DROP), (3, HI, DROP), (4, LO, DROP)]),
        (3, 1): stage({0: HI}, [(2, LO, LIVE)]),
    }),
    "masked": ((3, 3, 12, 12, 4, True), 49, {
        (0, 0): stage({2: LO}, [(1, LO, LIVE)], off_pins={5: LO, 6: HI}, off_rows={3: HI}),
        (1, 1): stage(rows=[(1, HI, LIVE)], off_pins={0: HI}, off_rows={0: LO, 2: HI}),
        (2, 2): stage({7: HI}, off_rows={1: LO}),
    }),
    # the same input and the same rows at one side in one stage and at the other in the next
    "upper_lower": ((3, 3, 12, 12, 4, True), 50, {
        **{(i, 0): stage({3: HI, 8: LO}, [(1, HI, LIVE), (2, LO, LIVE)]) for i in range(3)},
        **{(i, 1): stage({3: LO, 8: HI}, [(1, LO, LIVE), (2, HI, LIVE)]) for i in range(3)},
        **{(i, 2): stage({3: HI}, [(0, LO if i % 2 else HI, LIVE)]) for i in range(3)},
    }),
}


def counts(name, rows=True):
    """[batch][3] designed (inputs pinned, rows accepted, rows dropped); rows = False: the design
    without its rows (a box-only handle)."""
    dims, _, stages = DESIGNS[name]
    out = np.zeros((dims[0], 3), dtype=int)
    for (i, _), s in stages.items():
        out[i, 0] += len(s["pins"])
        if rows:
            out[i, 1] += sum(kind == LIVE for _, _, kind in s["rows"])
            out[i, 2] += sum(kind != LIVE for _, _, kind in s["rows"])
    return out


def held(name, i, rows=True):
    """The designed accepted rows of QP i in the order active_rows takes them, as its stages
    without the E rows and bounds: per stage [(kind, index, upper)]."""
    dims, _, stages = DESIGNS[name]
    out = []
    for k in range(dims[1]):
        s = stages.get((i, k), stage())
        acc = [("pin", c, up) for c, up in sorted(s["pins"].items())]
        if rows:
            acc += [("row", j, up) for j, up, kind in s["rows"] if kind == LIVE]
        out.append(acc)
    return out


def build(name, OcpQpBatch, rows=True):
    """(qp, x0, {"x", "u", "pi"}) of a design; rows = False: ng = 0 and the design's pins alone."""
    (batch, N, nx, nu, ng, box), seed, stages = DESIGNS[name]
    ng = ng if rows else 0
    qp, x0 = helpers.random_constrained(batch, N, nx, nu, ng, seed, OcpQpBatch)
    qp.C = None
    qp.lbx = qp.ubx = qp.lbx_mask = qp.ubx_mask = None
    rng = np.random.default_rng(seed + 1000)
    small = lambda: rng.uniform(-0.3, 0.3)
    if box:
        qp.lbu, qp.ubu = np.zeros((batch, N, nu)), np.zeros((batch, N, nu))
        qp.lbu_mask, qp.ubu_mask = np.ones((batch, N, nu)), np.ones((batch, N, nu))
    else:
        qp.lbu = qp.ubu = qp.lbu_mask = qp.ubu_mask = None
    if ng:
        qp.lg, qp.ug = np.zeros((batch, N + 1, ng)), np.zeros((batch, N + 1, ng))
        qp.lg_mask, qp.ug_mask = np.ones((batch, N + 1, ng)), np.ones((batch, N + 1, ng))
    for (i, k), s in stages.items():
        assert box or not (s["pins"] or s["off_pins"]), name
        for c, up in s["pins"].items():
            (qp.ubu if up else qp.lbu)[i, k, c] = small()
        for j, up, kind in s["rows"] if ng else ():
            if kind == LIVE:
                (qp.ug if up else qp.lg)[i, k, j] = small()
            elif kind != DROP:
                assert kind < j, (name, i, k, j)
                qp.D[i, k, j] = qp.D[i, k, kind]
    point = {"x": np.zeros((batch, N + 1, nx)), "u": np.zeros((batch, N, nu)), "pi": np.zeros((batch, N + 1, nx))}
    for i in range(batch):
        acc = [[(kind, idx, up, None, None) for kind, idx, up in st] for st in held(name, i, rows)]
        point["x"][i], point["u"][i], point["pi"][i] = arh.forward_rows_host(qp, x0[i], acc, i)
    away = lambda shape: 1.0 + rng.uniform(0.0, 1.0, shape)
    u = point["u"]
    if box:
        on_l, on_u = np.zeros((batch, N, nu), dtype=bool), np.zeros((batch, N, nu), dtype=bool)
        for (i, k), s in stages.items():
            for c, up in s["pins"].items():
                (on_u if up else on_l)[i, k, c] = True
            for c, up in s["off_pins"].items():
                (qp.ubu if up else qp.lbu)[i, k, c] = u[i, k, c]
                (qp.ubu_mask if up else qp.lbu_mask)[i, k, c] = 0.0
                (on_u if up else on_l)[i, k, c] = True
        qp.lbu = np.where(on_l, qp.lbu, u - away(u.shape))
        qp.ubu = np.where(on_u, qp.ubu, u + away(u.shape))
    if ng:
        g = np.einsum("bkgj,bkj->bkg", qp.D, u)
        on_l, on_u = np.zeros((batch, N, ng), dtype=bool), np.zeros((batch, N, ng), dtype=bool)
        for (i, k), s in stages.items():
            for j, up, kind in s["rows"]:
                if kind != LIVE:
                    (qp.ug if up else qp.lg)[i, k, j] = g[i, k, j]
                (on_u if up else on_l)[i, k, j] = True
            for j, up in s["off_rows"].items():
                (qp.ug if up else qp.lg)[i, k, j] = g[i, k, j]
                (qp.ug_mask if up else qp.lg_mask)[i, k, j] = 0.0
                (on_u if up else on_l)[i, k, j] = True
        qp.lg[:, :N] = np.where(on_l, qp.lg[:, :N], g - away(g.shape))
        qp.ug[:, :N] = np.where(on_u, qp.ug[:, :N], g + away(g.shape))
        qp.lg[:, N], qp.ug[:, N] = -1.0, 1.0
    return qp, x0, point


def distances(qp, u, i):
    """The distances of QP i at u to every unmasked bound on the inputs and the rows."""
    N = qp.N
    out = []
    if qp.lbu is not None:
        out += [(u - qp.lbu[i])[qp.lbu_mask[i] != 0], (qp.ubu[i] - u)[qp.ubu_mask[i] != 0]]
    if qp.ng > 0:
        g = np.einsum("kgj,kj->kg", qp.D[i], u)
        out += [(g - qp.lg[i][:N])[qp.lg_mask[i][:N] != 0], (qp.ug[i][:N] - g)[qp.ug_mask[i][:N] != 0]]
    return np.concatenate([d.ravel() for d in out])
