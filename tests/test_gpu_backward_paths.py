"""The backward pass on every kernel path it can take, against the numpy statement of its math
(tests/adjoint_host.py, tests/adjoint_rows_host.py: one dense KKT solve per QP) at Eigen's isApprox
1e-9 per QP and array, counts exactly, reg_prim = 0 (the statement has no regularisation).

tests/test_gpu_backward.py and tests/test_gpu_backward_rows.py run at batch <= 67 and N <= 20 on
fresh, aligned tensors and a handle whose capacity is the batch.  Which kernels that reaches is
decided by three constants of the adjoint Riccati solve's dispatch (ric_f64::launch_alg,
csrc/riccati_unconstr_impl.h:957-985):

  256  kLdsBatchMax, riccati_unconstr_impl.h:918: a larger batch takes the streaming kernel;
  26   the largest N whose image fits kLdsBytesMax (riccati_unconstr_impl.h:919, use_lds_kernel
       :922-924): a longer horizon takes the streaming kernel;
  20   the largest N of lat_fits (riccati_latency_impl.h:486, and the static_assert at :268): with
       ric_alg = 0, up to it the matrix-core latency kernel, from 21 to 26 the LDS kernel.

ric_alg = 1 (the square-root recursion) never takes the latency kernel.  srbd_qp_default_settings
has ric_alg = 1, so the tests that pass no settings run the LDS kernel's square-root variant and
only the SRBD test (ric_alg = 0) the latency kernel; the shapes of PATHS below sit on every class
and on both sides of 256.  If the dispatch changes, move them.

A. test_designed_active_sets: the designs of tests/backward_designs.py (no forward solve: the
   point is given, no QP is left out).  B. test_adjoint_kernel_paths: a real forward solve, then
   the backward pass on each Riccati kernel.  C. the generic (unaligned) gradient, mask, project
   and lift kernels at 12 x 12.  D. one handle across batch sizes, entry points and a forward solve.

Seen on an MI355X: worst relative error per QP and array 7.6e-15 ... 1.7e-13 in A (every QP, none
left out; pinned / accepted / dropped as designed), at most 2.6e-12 in B (the figures are in its
docstring), 0 between the aligned and the misaligned calls of C, and every call of D bit for bit
that of a handle of its own (its batch 7 of capacity 64: 1.1e-14 and 2.5e-14 from the statement).
"""
import ctypes as C

import numpy as np
import pytest

import adjoint_host
import adjoint_rows_host as arh
import backward_designs as bd
import helpers
import test_gpu_backward as plain
import test_gpu_backward_rows as rows

pytestmark = pytest.mark.gpu

NAMES, ALL = adjoint_host.NAMES, arh.ALL_NAMES
ACT_TOL, RANK_TOL, POISON = rows.ACT_TOL, rows.RANK_TOL, rows.POISON
ST = dict(rows.ROWS_ST, reg_prim=0.0, ric_alg=0)
EINVAL, EDIM = -1, -2
assert (ACT_TOL, RANK_TOL) == (bd.ACT_TOL, bd.RANK_TOL) and plain.ACT_TOL == ACT_TOL


def shapes(qp, batch):
    """The fourteen gradient arrays in the C-ABI layout (column-major blocks as [cols][rows])."""
    N, nx, nu, ng = qp.N, qp.nx, qp.nu, qp.ng
    return {"A": (batch, N, nx, nx), "B": (batch, N, nu, nx), "b": (batch, N, nx), "Q": (batch, N + 1, nx, nx),
            "S": (batch, N, nx, nu), "R": (batch, N, nu, nu), "q": (batch, N + 1, nx), "r": (batch, N, nu),
            "x0": (batch, nx), "D": (batch, N, nu, ng), "lg": (batch, N + 1, ng), "ug": (batch, N + 1, ng),
            "lbu": (batch, N, nu), "ubu": (batch, N, nu)}


def inside(torch, a, misaligned):
    """`a` on the device as a view into a poisoned tensor: 16 bytes in, or 8 (data_ptr() % 16 == 8)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    off = 1 if misaligned else 2
    whole = torch.full((a.size + 4,), POISON, dtype=torch.float64, device="cuda:0")
    view = whole[off:off + a.size]
    view.copy_(torch.from_numpy(a.ravel()))
    assert view.data_ptr() % 16 == (8 if misaligned else 0)
    return whole, view


def backward(run, entry, gx, gu, names=None, handle=None, batch=None, misaligned=False, gu_misaligned=False):
    """One backward call through `entry` ("plain": srbd_qp_solve_backward_f64, "rows":
    srbd_qp_solve_backward_rows_f64) on `handle` (default: the run's).  Every output is a view
    into a poisoned tensor, whose rim must come back untouched.  Returns (name -> numpy in the
    C-ABI layout, counts: [batch][3], or [batch] pinned / None from the plain entry point)."""
    torch, capi, qp = run.torch, run.capi, run.qp
    h = handle or run.h
    batch = qp.batch if batch is None else batch
    names = names or (ALL if entry == "rows" else NAMES)
    off = 1 if misaligned else 2
    shp = {n: s for n, s in shapes(qp, batch).items() if n in names and int(np.prod(s)) > 0}
    whole = {n: torch.full((int(np.prod(s)) + 4,), POISON, dtype=torch.float64, device="cuda:0") for n, s in shp.items()}
    ptr = {n: whole[n][off:].data_ptr() for n in shp}
    assert all(p % 16 == (8 if misaligned else 0) for p in ptr.values())
    gx_t = torch.from_numpy(np.ascontiguousarray(gx[:batch])).to("cuda:0")
    gu_whole, gu_t = inside(torch, gu[:batch], gu_misaligned)
    grad = capi.Grad(**{n: p for n, p in ptr.items() if n in NAMES})
    if entry == "rows":
        five = {n: p for n, p in ptr.items() if n in arh.ROW_NAMES}
        h.solve_backward_rows_device(batch, run.st, run.data, run.sol, gx_t, gu_t, grad,
                                     capi.GradRows(**five) if five else None, act_tol=ACT_TOL, rank_tol=RANK_TOL)
        counts = h.backward_active(batch).cpu().numpy()
    else:
        h.solve_backward_device(batch, run.st, run.data, run.sol, gx_t, gu_t, grad, act_tol=ACT_TOL)
        counts = h.backward_pinned(batch).cpu().numpy() if qp.has_box_u else None
    h.synchronize()
    out = {}
    for n, s in shp.items():
        a = whole[n].cpu().numpy()
        size = a.size - 4
        assert np.all(a[:off] == POISON) and np.all(a[off + size:] == POISON), ("written outside", n)
        out[n] = a[off:off + size].reshape(s)
        assert not np.any(out[n] == POISON), ("not written", n)
    g = gu_whole.cpu().numpy()
    assert np.array_equal(g[1 if gu_misaligned else 2:][:gu_t.numel()], np.ravel(gu[:batch])), "gu was written"
    for n in names:  # (ng = 0: D, lg, ug are empty)
        out.setdefault(n, np.zeros(shapes(qp, batch)[n]))
    return out, counts


class Given:
    """What a backward call needs of a Run, with the forward solution given instead of solved."""

    def __init__(self, pkg, qp, x0, point, st=ST):
        import torch
        self.torch, self.capi, self.qp, self.fwd = torch, pkg.capi, qp, point
        self.h = pkg.capi.Handle(qp.N, qp.nx, qp.nu, qp.ng, qp.has_box_u, False, capacity=qp.batch)
        self.st = pkg.capi.settings_struct(st)
        self.dt, self.sol_t, self.data, self.sol = pkg.capi.device_buffers(qp, x0)
        for k in ("x", "u", "pi"):
            self.sol_t[k].copy_(torch.from_numpy(np.ascontiguousarray(point[k])))


def held_to_statement(run, entry, got, counts, gx, gu, keep, what):
    """Every QP's counts against the statement's, and the gradients of the QPs in `keep` at 1e-9.
    Returns the worst relative error."""
    qp, worst = run.qp, 0.0
    for i in range(len(gx)):
        if entry == "rows":
            want, cnt = rows.reference(qp, run.fwd, gx, gu, i)
            assert tuple(counts[i]) == cnt, (what, i, counts[i], cnt)
            if i in keep:
                worst = max(worst, rows.compare_qp(got, want, i, what=what))
        else:
            want, npin = plain.reference(qp, run.fwd, gx, gu, i, ACT_TOL if qp.has_box_u else None)
            assert counts is None or counts[i] == npin, (what, i, counts[i], npin)
            if i in keep:
                worst = max(worst, plain.compare_qp(got, want, i, what=what))
    return worst


# ---------------------------------------------------------------------------
# A. designed active sets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bd.DESIGNS))
def test_designed_active_sets(pkg, OcpQpBatch, name):
    """The rows entry point on every design of tests/backward_designs.py: all fourteen arrays and
    the three counts of every QP (none is left out), and each designed pin's and row's gradient
    on the designed side, the other side exactly zero."""
    qp, x0, point = bd.build(name, OcpQpBatch)
    gx, gu = rows.cotangents(qp, 23)
    run = Given(pkg, qp, x0, point)
    got, counts = backward(run, "rows", gx, gu)
    assert np.array_equal(counts, bd.counts(name)), (name, counts)
    worst = held_to_statement(run, "rows", got, counts, gx, gu, range(qp.batch), name)
    for (i, k), s in bd.DESIGNS[name][2].items():
        for c, up in s["pins"].items():
            assert got["ubu" if up else "lbu"][i, k, c] != 0.0 and got["lbu" if up else "ubu"][i, k, c] == 0.0, (i, k, c)
        for c in s["off_pins"]:
            assert got["lbu"][i, k, c] == 0.0 and got["ubu"][i, k, c] == 0.0, (i, k, c)
        for j, up, kind in s["rows"]:
            on, other = got["ug" if up else "lg"][i, k, j], got["lg" if up else "ug"][i, k, j]
            assert (on != 0.0) == (kind == bd.LIVE) and other == 0.0, (i, k, j)
            assert got["D"][i, k, :, j].any() == (kind == bd.LIVE), (i, k, j)
        for j in s["off_rows"]:
            assert got["lg"][i, k, j] == 0.0 and got["ug"][i, k, j] == 0.0 and not got["D"][i, k, :, j].any()
    print(f"[backward paths] design {name}: pinned / accepted / dropped {counts.sum(axis=0)}; "
          f"worst relative error {worst:.2e}")
    run.h.close()


@pytest.mark.parametrize("name", ["partial", "all_pinned"])
def test_designed_pins_through_the_entry_point_without_rows(pkg, OcpQpBatch, name):
    """The design's pins alone on a box-only handle through srbd_qp_solve_backward_f64: nine
    gradients and the pinned counts; the rows entry point on the same handle gives the same bits."""
    qp, x0, point = bd.build(name, OcpQpBatch, rows=False)
    gx, gu = rows.cotangents(qp, 23)
    run = Given(pkg, qp, x0, point)
    got, pins = backward(run, "plain", gx, gu)
    assert np.array_equal(pins, bd.counts(name, rows=False)[:, 0]), (name, pins)
    worst = held_to_statement(run, "plain", got, pins, gx, gu, range(qp.batch), name)
    again, counts = backward(run, "rows", gx, gu)
    assert np.array_equal(counts[:, 0], pins) and not counts[:, 1:].any()
    for n in NAMES:
        assert np.array_equal(again[n], got[n]), n
    held_to_statement(run, "rows", again, counts, gx, gu, range(qp.batch), name)
    print(f"[backward paths] design {name} without rows: pinned {pins.sum()}; worst relative error {worst:.2e}")
    run.h.close()


# ---------------------------------------------------------------------------
# B. the adjoint solve on each Riccati kernel
# ---------------------------------------------------------------------------
# (batch, N, ric_alg, handle kind, seed).  Kernel of the adjoint solve, by the constants above:
PATHS = [
    (300, 2, 0, "none", 3), (300, 2, 0, "box_u", 5), (300, 2, 0, "rows", 11),  # streaming: batch > 256
    (3, 21, 0, "none", 3), (3, 26, 0, "box_u", 2),                            # LDS, classical
    (3, 27, 0, "none", 3), (3, 27, 0, "box_u", 1),                            # streaming: N > 26
    (5, 3, 1, "none", 3), (5, 3, 1, "box_u", 7),                              # LDS, square root
    (300, 2, 1, "none", 3),                                                   # streaming, square root
    (257, 2, 0, "none", 3), (256, 2, 0, "none", 3),                           # streaming | latency
    (5, 3, 0, "none", 3), (5, 3, 0, "box_u", 7), (5, 3, 0, "rows", 11),       # latency
    (3, 20, 0, "none", 3),                                                    # latency, its longest horizon
]


def path_batch(OcpQpBatch, batch, N, kind, seed):
    if kind == "none":
        return helpers.random_unconstrained(batch, N, 12, 12, seed, OcpQpBatch)
    if kind == "rows":
        return rows.make_rows_batch(OcpQpBatch, (batch, N, 12, 12, 4, True, seed), 1.0)
    qp, x0 = helpers.random_constrained(batch, N, 12, 12, 0, seed, OcpQpBatch)
    qp.lbx = qp.ubx = qp.lbx_mask = qp.ubx_mask = None
    return qp, x0


def kept_of(qp, kind, u):
    """The QPs whose active set is beyond doubt, by the rule of the two existing modules."""
    if kind == "none":
        return np.arange(qp.batch)
    return rows.classify(qp, u)[0] if kind == "rows" else rows.classify_boxes(qp, u)[0]


@pytest.mark.parametrize("batch,N,ric_alg,kind,seed", PATHS)
def test_adjoint_kernel_paths(pkg, OcpQpBatch, batch, N, ric_alg, kind, seed):
    """A GPU forward solve, then the backward pass, all gradients of every kept QP against the
    statement on the GPU's own forward solution.  "none": the plain entry point, and the rows
    entry point bit for bit; "box_u": the plain entry point (nine, pinned), and the rows one with
    the same nine bit for bit and lbu, ubu against the statement; "rows": ng = 4 and boxes.

    Seeds of the box and rows cases: checked with the CPU oracle, which keeps 286 of 300 (198 of
    them with a pinned input, 306 pinned), 265 of 300 (261 with an active bound; 220 pinned, 674
    rows accepted), 3 of 3 at N = 26 (seed 2: 11 pinned) and at N = 27 (seed 1: 13 pinned; each
    the first seed from 1 up at which all three QPs are beyond doubt), 5 of 5 at (5, 3) (seed 7:
    4 with a pin, 7 pinned; rows seed 11: 5 with an active bound, 7 pinned, 18 rows).  The GPU's
    forward solve gives the same counts.

    "none" is helpers.random_unconstrained, whose A has a spectral radius near 2.  At N >= 16 the
    classical recursion (ric_alg 0) missed 1e-9 on it before this test: relative error 1.5e-8 at
    N = 16, 4.9e-6 at N = 20 (latency kernel), 1.1e-5 at N = 21 (LDS kernel), 5.7e-2 at N = 27
    (streaming kernel), each on grad A, with the square root at 4e-14.  The statement was not
    off: a numpy Riccati recursion that keeps P symmetric agrees with its dense solve to 1e-14,
    and one that carries F - Y'Y unsymmetrised reproduces the kernels' figures (the antisymmetric
    rounding grows by rho(A)^2 per stage).  Fixed in the kernels (riccati_unconstr_impl.h
    solve_qp, riccati_latency_impl.h); (3, 20), (3, 21) and (3, 27) are its regression cases and
    1e-9 holds as stated, so no wider allowance was needed.

    Seen on an MI355X: worst relative error per QP and array 1.7e-14 ... 9.7e-14 on the small
    batches (3.4e-14, 4.3e-14, 4.1e-14 at (3, 20), (3, 21), (3, 27) without bounds), 5.2e-14,
    5.3e-13 and 1.8e-12 ... 2.6e-12 (two runs) on the 300 QPs without bounds, with boxes and
    with rows."""
    qp, x0 = path_batch(OcpQpBatch, batch, N, kind, seed)
    gx, gu = rows.cotangents(qp, seed + 1)
    run = rows.Run(pkg, qp, x0, dict(ST, ric_alg=ric_alg))
    keep = kept_of(qp, kind, run.fwd["u"])
    assert len(keep) >= 0.75 * batch, len(keep)
    assert np.all(run.fwd["status"][keep] == 0), run.fwd["status"]
    what = (batch, N, ric_alg, kind)
    got, counts = backward(run, "rows", gx, gu)
    worst = held_to_statement(run, "rows", got, counts, gx, gu, keep, what)
    if kind != "none":
        bound = int(np.sum(counts[keep].sum(axis=1) > 0))
        assert bound >= 0.5 * len(keep), (bound, len(keep))
    if kind != "rows":
        old, pins = backward(run, "plain", gx, gu)
        assert pins is None or np.array_equal(pins, counts[:, 0])
        for n in NAMES:
            assert np.array_equal(old[n], got[n]), n
        worst = max(worst, held_to_statement(run, "plain", old, pins, gx, gu, keep, what))
    print(f"[backward paths] {what}: kept {len(keep)} of {batch}, pinned / accepted / dropped "
          f"{counts[keep].sum(axis=0)}; worst relative error {worst:.2e}")
    run.h.close()


# ---------------------------------------------------------------------------
# C. the alignment fallback
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,seed", [("none", 3), ("box_u", 7), ("rows", 11)])
def test_misaligned_pointers_take_the_generic_kernels(pkg, OcpQpBatch, kind, seed):
    """12 x 12 with every gradient output 8 bytes off a 16-byte boundary (the generic gradient
    kernel, the scalar lift kernel) and, with boxes or rows, gu too (the generic mask and project
    kernels; the Riccati kernel then reads the masked rm, capi_backward.hip:148-151, 176-179, not
    gu).  What the Riccati kernel and the forward solve read stays aligned.  Against the
    statement at 1e-9 and against the aligned call at 1e-12 (the generic kernels sum in another
    order); the rim of every view is checked in backward()."""
    qp, x0 = path_batch(OcpQpBatch, 5, 3, kind, seed)
    gx, gu = rows.cotangents(qp, seed + 1)
    run = rows.Run(pkg, qp, x0, ST)
    keep = kept_of(qp, kind, run.fwd["u"])
    assert len(keep) >= 0.75 * qp.batch
    worst = 0.0
    for entry in ("rows",) if kind == "rows" else ("plain", "rows"):
        want, wcnt = backward(run, entry, gx, gu)
        for outs, g in ((True, False), (False, True), (True, True)) if kind != "none" else ((True, False),):
            got, cnt = backward(run, entry, gx, gu, misaligned=outs, gu_misaligned=g)
            assert np.array_equal(cnt, wcnt)
            for n in want:
                diff, size = np.linalg.norm(got[n] - want[n]), np.linalg.norm(want[n])
                assert diff <= 1e-12 * size, (entry, outs, g, n, diff, size)
                worst = max(worst, diff / size if size else 0.0)
            held_to_statement(run, entry, got, cnt, gx, gu, keep, (kind, entry, outs, g))
    print(f"[backward paths] misaligned {kind}: worst relative difference to the aligned call {worst:.2e}")
    run.h.close()


# ---------------------------------------------------------------------------
# D. handle state
# ---------------------------------------------------------------------------
def fresh(pkg, run, entry, gx, gu, batch):
    """The call on a handle of its own with capacity = batch."""
    qp = run.qp
    h = pkg.capi.Handle(qp.N, qp.nx, qp.nu, qp.ng, qp.has_box_u, False, capacity=batch)
    out = backward(run, entry, gx, gu, handle=h, batch=batch)
    h.close()
    return out


def same(a, b):
    assert np.array_equal(a[1], b[1]), (a[1], b[1])
    for n in b[0]:
        assert np.array_equal(a[0][n], b[0][n]), n


@pytest.mark.parametrize("kind,seed", [("box_u", 5), ("rows", 13)])
def test_handle_reuse(pkg, OcpQpBatch, kind, seed):
    """One handle of capacity 64: a backward at batch 64, one at batch 7 (batch < capacity: the
    layout of the handle's buffer is the capacity's), a forward solve, batch 64 again; every
    result bit for bit that of a handle of its own with capacity = batch.  The box handle then
    changes entry points, plain -> rows -> plain: the rows layout is larger, so the buffer is
    allocated again and its zero run (the adjoint's b and x0) written again.  A handle with rows
    cannot make that change: the plain entry point refuses ng > 0 (SRBD_QP_EDIM), which is
    asserted before its first rows call, and leaves the handle as it was."""
    import torch
    capi, L = pkg.capi, pkg.capi.lib()
    qp, x0 = path_batch(OcpQpBatch, 64, 3, kind, seed)
    gx, gu = rows.cotangents(qp, seed + 1)
    big = rows.Run(pkg, qp, x0, ST)
    small = rows.Run(pkg, qp.subset(slice(0, 7)), x0[:7], ST)
    keep7 = kept_of(small.qp, kind, small.fwd["u"])
    assert len(keep7) >= 0.75 * 7, keep7
    entry = "rows" if kind == "rows" else "plain"
    want64, want7 = fresh(pkg, big, entry, gx, gu, 64), fresh(pkg, small, entry, gx, gu, 7)
    h = capi.Handle(3, 12, 12, qp.ng, True, False, capacity=64)
    some = torch.zeros(64 * 3, dtype=torch.int32, device="cuda:0")
    pinned = lambda n: L.srbd_qp_backward_pinned_f64(h.ptr, n, C.c_void_p(some.data_ptr()), None)
    active = lambda n: L.srbd_qp_backward_active_f64(h.ptr, n, C.c_void_p(some.data_ptr()), None)
    if kind == "rows":
        grad = capi.Grad(q=some.data_ptr())
        assert L.srbd_qp_solve_backward_f64(h.ptr, 64, C.byref(big.st), C.byref(big.data), C.byref(big.sol),
                                            C.c_void_p(some.data_ptr()), None, ACT_TOL, C.byref(grad), None) == EDIM
        assert pinned(1) == EINVAL and active(1) == EINVAL
    same(backward(big, entry, gx, gu, handle=h), want64)                    # 1
    got7 = backward(small, entry, gx, gu, handle=h, batch=7)                # 2
    same(got7, want7)
    worst = held_to_statement(small, entry, *got7, gx[:7], gu[:7], keep7, (kind, 7))
    assert (active if kind == "rows" else pinned)(8) == EINVAL  # eight counts after a call of seven
    assert (active if kind == "rows" else pinned)(7) == 0
    assert (pinned if kind == "rows" else active)(1) == EINVAL  # the other entry point's counts
    _, sol_t, _, sol = capi.device_buffers(qp, x0)                          # 3
    h.solve_device(64, big.st, big.data, sol)
    h.synchronize()
    assert np.all(sol_t["status"].cpu().numpy()[kept_of(qp, kind, big.fwd["u"])] == 0)
    same(backward(big, entry, gx, gu, handle=h), want64)                    # 4
    if kind == "box_u":
        before = h.memory_bytes()
        same(backward(big, "rows", gx, gu, handle=h), fresh(pkg, big, "rows", gx, gu, 64))
        assert h.memory_bytes() > before  # the rows layout: allocated again
        assert pinned(1) == EINVAL and active(64) == 0
        same(backward(small, "plain", gx, gu, handle=h, batch=7), want7)
        assert active(1) == EINVAL and pinned(7) == 0 and pinned(8) == EINVAL
        same(backward(small, "rows", gx, gu, handle=h, batch=7), fresh(pkg, small, "rows", gx, gu, 7))
    h.synchronize()
    print(f"[backward paths] handle reuse {kind}: batch 7 of capacity 64 worst relative error {worst:.2e}")
    for r in (big, small):
        r.h.close()
    h.close()
