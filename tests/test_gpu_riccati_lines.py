"""The fp64 streaming Riccati kernel moves the forward sweep's 96-byte rows as whole lines.

The rows of x, u and pi go through the wave's LDS image in chunks of four stages (aligned to
stage indices that are multiples of 4) and leave as 16-byte pieces in lane order; b comes in
the same way, one chunk ahead of its use (riccati_unconstr_impl.h, fwd_sweep).  Only the way
the data moves differs from the plain row stores and loads, so every output is the value the
single-QP kernels compute: bit-identical where they run the same instructions (ric_alg = 1 at
any N, ric_alg = 0 at N >= 21), 1e-11 against the matrix-core kernel (ric_alg = 0, N <= 20)
and 1e-9 against the oracle there, as in test_gpu_riccati_turnaround.py.

Every QP is a distinct SRBD QP, so a row stored to or read from the wrong QP, stage or chunk
shows.
"""
import functools

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

KEYS = ("x", "u", "pi", "P", "p", "K", "k", "status", "iter")


@functools.lru_cache(maxsize=None)
def _batch(pkg, N, seed=5151, batch=300):
    """300 distinct SRBD QPs of horizon N (shared between the tests: never modified)."""
    return pkg.srbd_model.generate_batch(batch, N=N, seed=seed, constraints="none")


@functools.lru_cache(maxsize=None)
def _solve300(pkg, N, ric_alg):
    qp, x0 = _batch(pkg, N)
    return pkg.capi.solve(qp, x0, dict(ric_alg=ric_alg), riccati=True)


def _head(pkg, N, b):
    qp, x0 = _batch(pkg, N)
    return qp.subset(slice(0, b)), x0[:b]


def _assert_equal(got, want, what):
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), (key, what)


@pytest.mark.parametrize("ric_alg", [0, 1])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 7, 8, 9, 20, 21])
def test_chunk_edges(pkg, oracle, N, ric_alg):
    """Batch 260 (streaming) against slices of it solved as small batches (single-QP kernels).
    The last chunk of x and pi holds (N mod 4) + 1 rows and that of u N mod 4: N = 3, 7 fill
    it, N = 4, 8, 20 leave one row of x and pi and none of u, N = 1, 2 never fill a chunk, and
    b has one chunk (N <= 4), two, three (N = 9) or six (N = 21: a last chunk of one stage)."""
    qp, x0 = _head(pkg, N, 260)
    st = dict(ric_alg=ric_alg)
    mfma = ric_alg == 0 and N <= 20
    big = pkg.capi.solve(qp, x0, st, riccati=True)
    assert np.all(big["status"] == 0) and np.all(big["iter"] == 0)
    for idx in (slice(0, 1), slice(100, 164), slice(4, 260)):
        small = pkg.capi.solve(qp.subset(idx), x0[idx], st, riccati=True)
        for key in KEYS:
            if mfma and key not in ("status", "iter"):
                for i in range(small[key].shape[0]):
                    assert helpers.is_approx(small[key][i], big[key][idx][i], 1e-11), (key, idx, i)
            else:
                assert np.array_equal(small[key], big[key][idx]), (key, idx)
    if mfma:
        ref = oracle.solve(qp, st, x0=x0)
        for key in ("x", "u", "pi", "P", "p", "K", "k"):
            for i in range(qp.batch):
                assert helpers.is_approx(big[key][i], ref[key][i], 1e-9), (key, i)


@pytest.mark.parametrize("b", [257, 258, 259, 260, 272])
def test_partial_last_wave(pkg, b):
    """1-4 live groups in the last wave (257-260) and a full last workgroup row (272) at
    N = 5 (one full chunk, one partial): each QP's outputs are those of the same QP in the
    batch of 300."""
    N, ric_alg = 5, 1
    full = _solve300(pkg, N, ric_alg)
    qp, x0 = _head(pkg, N, b)
    out = pkg.capi.solve(qp, x0, dict(ric_alg=ric_alg), riccati=True)
    _assert_equal(out, {k: full[k][:b] for k in KEYS}, b)


def _solve_at(pkg, qp, x0, settings, layout=0, place=None):
    """Solve through a handle with device buffers of the test's own.  layout = 1: the QP data
    handed over as [stage][batch][block].  place(name, tensor) -> tensor may move a buffer
    (inputs b, q, r and outputs x, u, pi) to an address of its choosing before the solve.
    Returns the outputs as numpy arrays and the placed tensors by name."""
    capi = pkg.capi
    h = capi.Handle(qp.N, 12, 12, 0, False, False, capacity=qp.batch, layout=layout)
    placed = {}
    try:
        dt, st, data, sol = capi.device_buffers(qp, x0, want_riccati=True)
        if layout == 1:
            for k in ("A", "B", "b", "Q", "S", "R", "q", "r"):
                dt[k] = dt[k].transpose(0, 1).contiguous()
                setattr(data, k, dt[k].data_ptr())
        if place is not None:
            for k in ("b", "q", "r"):
                placed[k] = dt[k] = place(k, dt[k])
                setattr(data, k, dt[k].data_ptr())
            for k in ("x", "u", "pi"):
                placed[k] = st[k] = place(k, st[k])
                setattr(sol, k, st[k].data_ptr())
        h.solve_device(qp.batch, capi.settings_struct(settings), data, sol)
        h.synchronize()
        out = {k: v.cpu().numpy() for k, v in st.items()}
    finally:
        h.close()
    out["P"] = np.swapaxes(out["P"], -1, -2)
    out["K"] = np.swapaxes(out["K"], -1, -2)
    return out, placed


@pytest.mark.parametrize("N", [5, 20])
@pytest.mark.parametrize("b", [3, 20])
def test_stage_major_small_batches(pkg, b, N):
    """layout = 1 runs the streaming kernel on 3 and 20 QPs (one partial wave; one workgroup
    and a partial second), where a chunk of b is four separate rows per QP: bit-identical to
    the same QPs in the QP-major batch of 300."""
    ric_alg = 1
    full = _solve300(pkg, N, ric_alg)
    qp, x0 = _head(pkg, N, b)
    out, _ = _solve_at(pkg, qp, x0, dict(ric_alg=ric_alg), layout=1)
    _assert_equal(out, {k: full[k][:b] for k in KEYS}, (b, N))


GUARD = 64  # doubles of NaN before, between and after the arrays (four 128-byte lines)


def _arena(sizes):
    """One NaN-filled device tensor with room for the named arrays (sizes in doubles), each
    base 16 bytes past a 128-byte boundary and GUARD doubles or more from its neighbours.
    Returns the tensor and {name: offset in doubles}."""
    import torch
    offs, o = {}, 0
    for name, n in sizes.items():
        o += GUARD
        o += (2 - o) % 16
        offs[name] = o
        o += n
    buf = torch.full((o + GUARD,), float("nan"), dtype=torch.float64, device="cuda:0")
    assert buf.data_ptr() % 128 == 0
    return buf, offs


@pytest.mark.parametrize("b", [259, 260])
def test_guard_zones(pkg, b):
    """x, u, pi as views inside one NaN-filled tensor and b, q, r inside another, every base
    16 bytes past a 128-byte boundary (the C-ABI promises 16-byte alignment and no more): the
    outputs are the aligned run's bit for bit and every guard element is still NaN.  Batch 259
    ends with a wave of three live groups, whose flush is partial."""
    import torch
    N, ric_alg = 5, 1
    full = _solve300(pkg, N, ric_alg)
    qp, x0 = _head(pkg, N, b)
    out_buf, out_off = _arena({"x": b * (N + 1) * 12, "u": b * N * 12, "pi": b * (N + 1) * 12})
    in_buf, in_off = _arena({"b": b * N * 12, "q": b * (N + 1) * 12, "r": b * N * 12})

    def place(name, t):
        buf, offs = (in_buf, in_off) if name in in_off else (out_buf, out_off)
        view = buf[offs[name]:offs[name] + t.numel()].view(t.shape)
        assert view.data_ptr() % 128 == 16
        if name in in_off:
            view.copy_(t)  # (the outputs stay NaN: an element the solve leaves out shows)
        return view

    out, placed = _solve_at(pkg, qp, x0, dict(ric_alg=ric_alg), place=place)
    _assert_equal(out, {k: full[k][:b] for k in KEYS}, b)
    guard = torch.ones(out_buf.numel(), dtype=torch.bool, device=out_buf.device)
    for n in ("x", "u", "pi"):
        guard[out_off[n]:out_off[n] + placed[n].numel()] = False
    assert int(guard.sum()) >= 4 * GUARD
    assert bool(torch.isnan(out_buf[guard]).all()), "a guard element was written"
    assert not bool(torch.isnan(out_buf[~guard]).any())


@pytest.mark.parametrize("ric_alg", [0, 1])
@pytest.mark.parametrize("stage", [2, 5, 8])
def test_fault_isolation(pkg, stage, ric_alg):
    """A NaN in one QP's b at a stage that the forward sweep reads from a staged chunk
    (N = 9: chunks 0, 1 and the one-stage chunk 2): that QP ends NaNDetected (3); the three
    other QPs of its wave (128..131) and all the rest are those of the clean run."""
    N, b, bad = 9, 260, 130
    st = dict(ric_alg=ric_alg)
    qp, x0 = _head(pkg, N, b)
    clean = pkg.capi.solve(qp, x0, st, riccati=True)
    assert np.all(clean["status"] == 0)
    qp.b = qp.b.copy()  # (the shared batch stays as it is)
    qp.b[bad, stage, 4] = np.nan
    out = pkg.capi.solve(qp, x0, st, riccati=True)
    assert out["status"][bad] == 3, out["status"][128:132]
    ok = np.arange(b) != bad
    for key in KEYS:
        assert np.array_equal(out[key][ok], clean[key][ok]), key
