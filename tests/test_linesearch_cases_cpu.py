"""The line search's case table (tests/linesearch_cases.py) without a GPU: every batch that
tests/test_gpu_linesearch_paths.py launches reaches, on the host, every branch of the filter and
every way a search stops; no host decision and no barrier row sits on a boundary; the changed
parameter set changes decisions field by field; and the kernel mutations the table is there to
catch would change what the GPU test asserts."""
import dataclasses

import numpy as np
import pytest

import linesearch_cases as LC
import nmpc_plan_host as PH

FULL = [b for b, v in LC.BATCHES.items() if v[2] != "one"]
CHANGED = [b for b in FULL if LC.BATCHES[b][0] == "changed"]


def _trials(r):
    return "".join(t.branch[0] for t in r["trace"]) + ("+" if r["accepted"] is not None else "-")


def _decisions(sm, b, ls=None, model=None):
    """Per robot what the GPU test holds the device to exactly or nearly so: (alpha out, a step
    was accepted) and the merit, under other line-search parameters or model fields."""
    out = []
    for i, q in enumerate(b["params"]):
        q = q if model is None else dataclasses.replace(q, **model)
        pl = None if b["plan"] is None else b["plan"].robot(i)
        trace = []
        r = PH.line_search(sm, q, pl, b["xs"][i], b["us"][i], b["dx"][i], b["du"][i], float(b["alpha0"][i]),
                           ls=ls or b["ls"], trace=trace)
        out.append(((r[2], bool(trace and trace[-1].accepted)), np.array(r[3:6])))
    return out


@pytest.mark.parametrize("batch_name", list(LC.BATCHES))
def test_every_batch_reaches_what_it_claims(pkg, batch_name):
    sm = pkg.srbd_model
    b = LC.batch(sm, batch_name)
    set_name = b["set"]
    assert not b["left_out"], f"no inputs with the margins for {b['left_out']}"
    assert len(b["names"]) % 2 == 1 and len(b["names"]) <= 16  # the last block's second group is empty
    reached = set()
    for name, r in zip(b["names"], b["host"]):
        print(f"{batch_name:20s} {name:14s} trials {_trials(r):19s} alpha {r['alpha']:.6g} theta {r['theta']:.2e} "
              f"dphi {r['dphi']:.2e} conv {int(r['converged'])} margin {r['margin']:.1e} "
              f"barrier {r['barrier_margin']:.1e}")
        claimed = LC.CASES[name][0 if set_name == "default" else 1]
        assert claimed <= r["outcomes"], (name, sorted(claimed - r["outcomes"]))
        assert r["margin"] >= LC.MARGIN, (name, r["margin"])
        assert r["barrier_margin"] >= LC.BARRIER_MARGIN, (name, r["barrier_margin"])
        reached |= r["outcomes"]
    if b["variant"] == "one":
        return
    assert not set(LC.OUTCOMES) - reached, sorted(set(LC.OUTCOMES) - reached)
    # neighbouring robots of the launch do different things
    for (n0, r0), (n1, r1) in zip(zip(b["names"], b["host"]), list(zip(b["names"], b["host"]))[1:]):
        assert _trials(r0) != _trials(r1), (n0, n1, _trials(r0))
    # no trial at the floor: the same arrays and the same alpha come back, merit and converged all the same
    for name in ("floor_at", "floor_below"):
        i = b["names"].index(name)
        r = b["host"][i]
        assert r["trace"] == [] and r["alpha"] == b["alpha0"][i] <= b["ls"]["alpha_min"]
        assert np.array_equal(r["xs"], b["xs"][i]) and np.array_equal(r["us"], b["us"][i])
        assert np.isfinite([r["phi"], r["theta"], r["dphi"]]).all()
    assert b["alpha0"][b["names"].index("floor_at")] == b["ls"]["alpha_min"]
    # a step that moves a cone row across theta_b and one that ends outside the cone were accepted
    assert any({"barrier:crossing", "barrier:negative"} <= r["outcomes"] and r["accepted"] for r in b["host"])


def test_the_table_covers_the_32_lane_groups_edges():
    horizons = {v[1] for v in LC.BATCHES.values()}
    assert {1, 31, 32} <= horizons  # two lanes; every lane one stage; lane 0 two stages
    assert {v[2] for v in LC.BATCHES.values()} == {None, "plan", "robots", "one"}
    for s in ("default", "changed"):
        assert {1, 20, 31, 32} <= {v[1] for v in LC.BATCHES.values() if v[0] == s and v[2] is None}


def test_the_changed_set_changes_every_field():
    d, c = LC.ls_of("default"), LC.ls_of("changed")
    assert all(c[f] != d[f] for f in LC.LS_FIELDS) and set(c) == set(LC.LS_FIELDS)
    assert c["beta_phi"] != c["beta_theta"] and c["beta_alpha"] != 0.5
    assert set(LC.PARAM_SETS["changed"]["model"]) == set(LC.MODEL_FIELDS)


# what a kernel with a parameter hard-wired, or a formula mistyped, would compute: the host search
# under other parameters.  eta -> -eta is the Armijo test with the wrong sign (phi - eta alpha dphi).
def _mutants(ls):
    d = PH.LS_DEFAULTS
    m = {f"{f} = its default": dict(ls, **{f: d[f]}) for f in LC.LS_FIELDS}
    m["the Armijo sign flipped"] = dict(ls, eta=-ls["eta"])
    m["beta_phi and beta_theta swapped"] = dict(ls, beta_phi=ls["beta_theta"], beta_theta=ls["beta_phi"])
    m["every field its default"] = dict(d)
    return m


@pytest.mark.parametrize("batch_name", CHANGED)
def test_a_kernel_that_ignores_a_parameter_fails_on_the_changed_set(pkg, batch_name):
    """Each mutant changes the returned alpha or whether a step is taken for at least one robot:
    the GPU test's `alpha ==` and its xs, us comparisons would fail.  For the model's fields the
    merit moves far beyond the GPU test's rtol = 1e-9."""
    sm = pkg.srbd_model
    b = LC.batch(sm, batch_name)
    real = _decisions(sm, b)
    missed = []
    for what, ls in _mutants(b["ls"]).items():
        seen = [n for n, (dr, _), (dm, _) in zip(b["names"], real, _decisions(sm, b, ls=ls)) if dr != dm]
        print(f"{batch_name}: {what}: caught by {seen}")
        if not seen:
            missed.append(what)
    assert not missed, missed
    default = sm.SrbdParams()
    for f in LC.MODEL_FIELDS:
        other = _decisions(sm, b, model={f: getattr(default, f)})
        rel = max(float(np.max(np.abs(mr - mm) / np.maximum(np.abs(mr), 1e-300))) for (_, mr), (_, mm) in zip(real, other))
        print(f"{batch_name}: {f} = its default: the merit moves by a relative {rel:.1e}")
        assert rel > 1e-6, f
