"""The device filter line search (srbd_linesearch_kernel) on the designed case table of
tests/linesearch_cases.py: every branch of the filter (theta, Armijo, mixed) with accepts and
rejects, every way a search stops (accept, exhaustion, alpha at the floor on entry), both values
of `converged` with each clause failing alone, and the relaxed barrier on both sides of theta_b
at the trial points -- under the default parameters and with every field of
srbd_linesearch_params and the model's mu_b, theta_b, dt, R changed, at the horizons where the
32-lane group's stage ownership changes (N = 1, 31, 32; 20 in between), with a plan (the PLAN
kernels), with per-robot parameters (the ROBOT kernels) and for a batch of one.

tests/test_linesearch_cases_cpu.py shows on the host that each batch reaches what it claims,
that no decision sits within 1e-8 of a boundary, and which case catches a kernel that ignores
a parameter.  Here the kernel is held to the host on all of it
(srbd_device.linesearch_matches_host)."""
import pytest

import linesearch_cases as LC
from srbd_device import _dev, device_plan, device_robots, handle, linesearch_matches_host

pytestmark = pytest.mark.gpu

HOST_FIELDS = ("xs", "us", "alpha", "phi", "theta", "dphi", "converged", "margin")


@pytest.mark.parametrize("batch_name", list(LC.BATCHES))
def test_linesearch_takes_the_hosts_path(pkg, batch_name):
    capi, sm = pkg.capi, pkg.srbd_model
    b = LC.batch(sm, batch_name)
    B, N = len(b["names"]), b["N"]
    assert B >= 1 and not b["left_out"], b["left_out"]
    h = handle(capi, N, B, "none")
    if b["variant"] == "robots":
        h.set_robots(model=device_robots(capi, b["params"]))
    plan_t = None if b["plan"] is None else device_plan(capi, b["plan"])
    # the default set goes through the binding's defaults, the changed one through both structs
    changed = b["set"] != "default"
    mp = capi.model_params(LC.model_of(sm, b["set"])) if changed else None
    lp = capi.LsParams(**b["ls"]) if changed else None
    xs_t, us_t, al_t = _dev(b["xs"]), _dev(b["us"]), _dev(b["alpha0"])
    merit, conv = capi.srbd_linesearch(h, xs_t, us_t, _dev(b["dx"]), _dev(b["du"]), al_t, params=mp, ls=lp,
                                       plan=plan_t)
    h.synchronize()
    host = [tuple(r[k] for k in HOST_FIELDS) for r in b["host"]]
    for name, r in zip(b["names"], b["host"]):
        print(f"{name:14s} host alpha {r['alpha']:.6g} accepted {r['accepted']} margin {r['margin']:.1e}")
    print("device alpha", al_t.cpu().numpy().tolist())
    linesearch_matches_host(b["xs"], b["us"], xs_t, us_t, al_t, merit, conv, host)
