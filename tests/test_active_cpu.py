"""Active sets (srbd_qp_srbd_set_active_f64, srbd_qp_srbd_step_work) without a GPU: the entry points
are exported, declared and checked by the binding, and the host statement of tests/active_host.py
agrees with itself on a tiny case: with everybody active it is tests/rollout_host.py's loop, a robot
that is not active keeps its bits, and an active robot does not notice who else is."""
import ctypes
import subprocess

import numpy as np
import pytest

import active_host as AH
import rollout_host as RH
from srbd_device import NMPC, SQP_MAX_LOOP

ACTIVE_SYMBOLS = ("srbd_qp_srbd_set_active_f64", "srbd_qp_srbd_step_work")


# ---- 1. the entry points exist ----
def test_active_entry_points_are_exported(pkg):
    capi = pkg.capi
    assert set(ACTIVE_SYMBOLS) <= set(capi.exported_symbols())
    assert set(ACTIVE_SYMBOLS) <= set(capi.PROTOTYPES)
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    assert set(ACTIVE_SYMBOLS) <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = capi.lib()
    assert L.srbd_qp_srbd_set_active_f64(None, None) == -1
    assert L.srbd_qp_srbd_step_work(None, None, None) == -1
    assert L.srbd_qp_abi_version() == 12  # additive to ABI 12
    # the struct's layout is the header's: a pointer and two ints
    assert ctypes.sizeof(capi.ActiveStruct) == 16
    a = capi.Active(skip_fallen=True, compact=True).struct()
    assert (a.mask, a.skip_fallen, a.compact) == (None, 1, 1)
    import torch
    with pytest.raises(ValueError, match="torch.int32"):
        capi.Active(mask=torch.zeros(3, dtype=torch.float64)).struct()
    with pytest.raises(ValueError, match="is on cpu"):
        capi.Active(mask=torch.zeros(3, dtype=torch.int32)).struct()
    with pytest.raises(ValueError, match="expected"):
        capi.Active(mask=torch.zeros(3, 1, dtype=torch.int32)).struct()


# ---- 2. the host statement against itself ----
def tiny(sm):
    B, N = 3, 3
    p = sm.SrbdParams()
    xs, us, x, alpha, plan = RH.walking_case(sm, p, B, N, 2, 7)
    return B, N, p, xs, us, x, alpha, plan


def test_host_step_over_a_mask(pkg, oracle):
    sm = pkg.srbd_model
    B, N, p, xs, us, x, alpha, plan = tiny(sm)
    w = RH.window(sm, plan, 0, N)
    full = AH.step(sm, oracle, p, w, xs, us, x, alpha, NMPC, SQP_MAX_LOOP, "none")
    loops = RH.sqp_loops(sm, oracle, p, w, xs, us, x, alpha, NMPC, SQP_MAX_LOOP, "none")
    assert np.array_equal(full["xs"], np.stack([r[0] for r in loops])) and full["sqp_iter"].tolist() == [r[3] for r in loops]
    on = np.array([True, False, True])
    got = AH.step(sm, oracle, p, w, xs, us, x, alpha, NMPC, SQP_MAX_LOOP, "none", active=on)
    for k in ("xs", "us", "alpha", "sqp_iter", "converged"):
        assert np.array_equal(got[k][on], full[k][on]), k
    assert np.array_equal(got["xs"][1], xs[1]) and np.array_equal(got["us"][1], us[1]) and got["alpha"][1] == alpha[1]
    assert got["sqp_iter"][1] == 0 and got["converged"][1] == 0 and (got["sqp_iter"][on] >= 1).all()


def test_host_closed_loop_with_skip_fallen(pkg, oracle):
    sm = pkg.srbd_model
    B, N, p, xs, us, x, alpha, plan = tiny(sm)
    T = 2
    # robot 1 starts below the threshold: it falls in tick 0's plant step
    x = x.copy()
    x[1, 8] = 0.5
    contact = sm.SrbdContact(mu=0.5, Lt=(0.0, 0.05, 0.05), fz_hi=400.0, fz_contact=5.0, z_min=0.8, cos_tilt_min=0.5)
    kw = dict(p=p, plan=plan, contact=contact)
    want = RH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, SQP_MAX_LOOP, "none", **kw)
    plain = AH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, SQP_MAX_LOOP, "none", **kw)
    for k in ("x_log", "u_log", "sqp_iter", "converged", "xs", "us", "x", "alpha", "fallen_log"):
        assert np.array_equal(plain[k], want[k]), k  # tick by tick is the loop
    assert want["fallen_log"].tolist() == [[0, 0], [1, 1], [0, 0]]
    skip = AH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, SQP_MAX_LOOP, "none", skip_fallen=True, **kw)
    stands = np.array([True, False, True])
    for k in ("x_log", "u_log", "sqp_iter", "converged", "xs", "us", "x", "alpha", "fallen_log"):
        assert np.array_equal(skip[k][stands], want[k][stands]), k
    assert all(np.array_equal(skip["state"][k], want["state"][k]) for k in want["state"])
    # the fallen robot: stepped in tick 0, then only shifted
    assert skip["sqp_iter"][1].tolist() == [int(want["sqp_iter"][1, 0]), 0] and skip["converged"][1, 1] == 0
    one = AH.closed_loop(sm, oracle, xs, us, x, alpha, 1, NMPC, SQP_MAX_LOOP, "none", skip_fallen=True, **kw)
    assert np.array_equal(skip["xs"][1, :N], one["xs"][1, 1:]) and np.array_equal(skip["us"][1, :N - 1], one["us"][1, 1:])
    assert skip["alpha"][1] == one["alpha"][1] and not np.array_equal(skip["xs"][1], want["xs"][1])
    # a mask on top: robot 2 is never stepped
    masked = AH.closed_loop(sm, oracle, xs, us, x, alpha, T, NMPC, SQP_MAX_LOOP, "none", mask=np.array([1, 1, 0]),
                            skip_fallen=True, **kw)
    assert not masked["sqp_iter"][2].any() and np.array_equal(masked["x_log"][0], skip["x_log"][0])
