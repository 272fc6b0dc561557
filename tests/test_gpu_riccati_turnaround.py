"""The fp64 streaming Riccati kernel keeps the records of stages 0 and 1 in LDS.

The backward sweep writes stage 1's and then stage 0's record last and the forward sweep
reads them first, so the large-batch kernel (riccati_unconstr_kernel, HbmSrc) leaves them
in the wave's LDS image and never sends them to the HBM workspace.  The terminal record
(stage N) always goes to the workspace, so N = 1 keeps stage 0 only.

Every QP is a distinct SRBD QP, so a record read from the wrong group of a wave shows.
The bit-exact reference is the single-QP LDS kernel, which small QP-major batches (<= 256)
take for ric_alg = 1 at any N and for ric_alg = 0 at N = 21..26: same instructions on the
same values.  At fp64, ric_alg = 0, N <= 20 the small batch takes the matrix-core kernel
(MFMA summation order): 1e-11 as in test_gpu_riccati.py::test_latency_kernel_bit_identical,
and the oracle at 1e-9.
"""
import functools

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

KEYS = ("x", "u", "pi", "P", "p", "K", "k", "status", "iter")


@functools.lru_cache(maxsize=None)
def _batch(pkg, N, seed=4242, batch=300):
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
@pytest.mark.parametrize("N", [1, 2, 3, 21])
def test_horizon_edges(pkg, oracle, N, ric_alg):
    """Batch 260 (streaming) against slices of it solved as small batches (single-QP
    kernels): N = 1 keeps stage 0 only, N = 2 keeps both and streams the terminal record
    alone, N = 3 streams one stage, N = 21 is past the matrix-core kernel's horizons."""
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
    """1-4 live groups in the last wave (257-260) and a full last workgroup row (272):
    each QP's outputs are those of the same QP in the batch of 300."""
    N, ric_alg = 3, 1
    full = _solve300(pkg, N, ric_alg)
    qp, x0 = _head(pkg, N, b)
    out = pkg.capi.solve(qp, x0, dict(ric_alg=ric_alg), riccati=True)
    _assert_equal(out, {k: full[k][:b] for k in KEYS}, b)


def _solve_stage_major(pkg, qp, x0, settings):
    """The same QPs handed over as [stage][batch][block]: the streaming kernel at any batch."""
    capi = pkg.capi
    h = capi.Handle(qp.N, 12, 12, 0, False, False, capacity=qp.batch, layout=1)
    try:
        dt, st, data, sol = capi.device_buffers(qp, x0, want_riccati=True)
        keep = {}
        for k in ("A", "B", "b", "Q", "S", "R", "q", "r"):
            keep[k] = dt[k].transpose(0, 1).contiguous()
            setattr(data, k, keep[k].data_ptr())
        h.solve_device(qp.batch, capi.settings_struct(settings), data, sol)
        h.synchronize()
        out = {k: v.cpu().numpy() for k, v in st.items()}
    finally:
        h.close()
    out["P"] = np.swapaxes(out["P"], -1, -2)
    out["K"] = np.swapaxes(out["K"], -1, -2)
    return out


@pytest.mark.parametrize("N", [2, 20])
@pytest.mark.parametrize("b", [3, 20])
def test_stage_major_small_batches(pkg, b, N):
    """layout = 1 runs the streaming kernel on 3 and 20 QPs (one partial wave; one
    workgroup and a partial second): bit-identical to the QP-major solve of the same QPs,
    which is the streaming kernel's too (the batch of 300)."""
    ric_alg = 1
    full = _solve300(pkg, N, ric_alg)
    qp, x0 = _head(pkg, N, b)
    out = _solve_stage_major(pkg, qp, x0, dict(ric_alg=ric_alg))
    _assert_equal(out, {k: full[k][:b] for k in KEYS}, (b, N))
    small = pkg.capi.solve(qp, x0, dict(ric_alg=ric_alg), riccati=True)  # QP-major, the same QPs
    _assert_equal(out, small, (b, N, "qp-major"))


def test_no_state_between_calls(pkg):
    """One handle solves batch A, then a different batch B of the same shape: B's outputs are
    those of B on a fresh handle (nothing of A's kept records is seen by B)."""
    N, b = 3, 260
    st = dict(ric_alg=1)
    qp, x0 = _batch(pkg, N)
    qa, xa = qp.subset(slice(0, b)), x0[:b]
    qb, xb = qp.subset(slice(40, 40 + b)), x0[40:40 + b]
    h = pkg.capi.Handle(N, 12, 12, capacity=b)
    try:
        first = pkg.capi.solve(qa, xa, st, riccati=True, handle=h)
        second = pkg.capi.solve(qb, xb, st, riccati=True, handle=h)
    finally:
        h.close()
    fresh = pkg.capi.solve(qb, xb, st, riccati=True)
    _assert_equal(second, fresh, "B after A")
    assert not np.array_equal(first["u"], second["u"])


@pytest.mark.parametrize("ric_alg", [0, 1])
@pytest.mark.parametrize("stage", [0, 1])
def test_fault_isolation(pkg, stage, ric_alg):
    """A NaN in one QP's R at a kept stage: that QP ends NaNDetected (3); the three other QPs
    of its wave (128..131) and all the rest are those of the clean run."""
    N, b, bad = 3, 260, 130
    st = dict(ric_alg=ric_alg)
    qp, x0 = _head(pkg, N, b)
    clean = pkg.capi.solve(qp, x0, st, riccati=True)
    assert np.all(clean["status"] == 0)
    qp.R = qp.R.copy()  # (the shared batch stays as it is)
    qp.R[bad, stage, 4, 4] = np.nan
    out = pkg.capi.solve(qp, x0, st, riccati=True)
    assert out["status"][bad] == 3, out["status"][128:132]
    ok = np.arange(b) != bad
    for key in KEYS:
        assert np.array_equal(out[key][ok], clean[key][ok]), key
