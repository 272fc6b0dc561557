#!/usr/bin/env python3
"""Chooses the numbers of tests/linesearch_cases.py's table on the CPU and writes them to
tests/golden/linesearch_cases.json.

For every batch (parameter set, horizon, variant) and every named case, the recipe's candidates
(seed, scale, ...) are tried in a fixed order through the host line search; the first one that
reaches the outcomes the case stands for, with the smallest comparison margin and the barrier's
distance from theta_b ten times above the bounds the tests assert, is kept.  A case with no such
candidate is left out of the file and reported; tests/test_linesearch_cases_cpu.py then fails on
the outcome that went missing.

usage: scripts/linesearch_case_search.py [--only=case,...] [batch ...]
(no batch: every batch; the batches, and with --only the cases, that are not named are kept)"""
import itertools
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "oracle"))

import helpers  # noqa: E402
import linesearch_cases as LC  # noqa: E402

SEEDS = range(6)


def grid(kind, **lists):
    keys = list(lists)
    return [(kind, dict(zip(keys, vals))) for vals in itertools.product(*lists.values())]


SMALL = (1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 3e-6)
CANDIDATES = {
    "theta_first": grid("restore", c=(0.9, 0.97, 0.99), push=(True,), scale=(0.5, 0.2, 0.05)),
    "armijo_first": grid("descent", scale=SMALL),
    "theta_rejects": grid("restore", c=(6.0, 4.0, 12.0), scale=(0.1, 0.01)),
    "armijo_reject": grid("overshoot", stages=(1, 2, 3), frac=(0.3, 0.1, 0.03, 0.01), at=(0.35, 0.3, 0.25, 0.2, 0.15)),
    "theta_exhaust": grid("random"),
    "mixed_phi": grid("descent", sigma=(0.0, 1e-4, 1e-5, 3e-4, 1e-3), scale=(1e-2, 3e-3, 3e-2, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0) + SMALL),
    "floor_at": grid("descent", scale=(1e-3,)),
    "switch": grid("descent", kink=(1e-3, 1e-2, 1e-4, 0.1, 0.3), scale=(0.1, 1.0, 0.01, 10.0, 1e-3)),
    "mixed_theta": grid("restore_ascent", sigma=(1e-5, 1e-4, 1e-6), scale=(1e-2, 1e-3, 1e-1, 1e-4)),
    "mixed_exhaust": grid("ascent", sigma=(1e-5, 3e-6, 1e-6, 3e-5, 3e-4, 1e-3), scale=(1e-2, 0.1, 1.0, 10.0, 1e-3, 1e-4)),
    "conv_no_dphi": grid("descent", dphi=(-1.1e-3,)),
    "not_descent": grid("ascent", scale=(0.1, 1e-2) + SMALL),
    "floor_below": grid("random"),
    "conv_no_theta": grid("descent", dphi=(-1e-5,), sigma=(1e-4, 3e-4, 5e-5, 1e-3)),
    "theta_slow": grid("restore", c=(0.02,), scale=(0.01,)),
}
# under the changed set the Armijo reject also tells theta_min = 1e-7 from the default 5e-10: theta lies
# between them and the rejected trial lowers phi, so the mixed branch would have accepted it
CANDIDATES_CHANGED = {
    "conv_no_theta": grid("descent", dphi=(-1e-5, -1e-6, -1e-4), sigma=(1e-4, 3e-4, 5e-5, 1e-3, 3e-3, 5e-4, 2e-4, 2e-3)),
    "armijo_reject": grid("overshoot", stages=(1, 2, 3), frac=(0.3, 0.1, 0.03), sigma=(1e-5, 4e-5, 3e-6, 1e-4),
                          at=(0.6, 0.55, 0.65)),
}
ALPHA0 = {"floor_at": "floor", "floor_below": "below", "mixed_phi": 0.25, "switch": 0.5}


def search(sm, batch_name, only=(), kept=()):
    set_name, N, variant = LC.BATCHES[batch_name]
    ls = LC.ls_of(set_name)
    params, plan = LC.batch_models(sm, batch_name)
    rows = []
    for i, name in enumerate(LC.batch_names(batch_name)):
        want = LC.CASES[name][0 if set_name == "default" else 1]
        pl = None if plan is None else plan.robot(i)
        alpha0 = ALPHA0.get(name, 1.0)
        found = None
        if only and name not in only:
            rows += [r for r in kept if r["name"] == name]
            continue
        cands = CANDIDATES_CHANGED.get(name, CANDIDATES[name]) if set_name == "changed" else CANDIDATES[name]
        for (kind, args), s in itertools.product(cands, SEEDS):
            seed = 100 * i + s
            case = LC.build_case(sm, params[i], pl, N, kind, seed, **args) + (LC.start_alpha(alpha0, ls),)
            r = LC.run_host(sm, params[i], pl, case, ls)
            extra = True
            if name == "mixed_exhaust":
                extra = r["theta"] >= ls["theta_min"]  # the nearly feasible one; not_descent is the feasible one
            if name == "mixed_phi":
                extra = len(r["trace"]) == 1  # at once; switch is the one that comes through the theta branch
            if name == "switch":
                extra = r["accepted"] is not None
            if name == "conv_no_theta" and set_name == "changed" and want <= r["outcomes"]:
                # beta_phi = 0.5 from the default 1e-6 and from beta_theta = 0.05: phi falls by less than half of
                # theta and by more than a twentieth of it
                other = LC.run_host(sm, params[i], pl, case, dict(ls, beta_phi=LC.ls_of("default")["beta_phi"]))
                swapped = LC.run_host(sm, params[i], pl, case, dict(ls, beta_phi=ls["beta_theta"], beta_theta=ls["beta_phi"]))
                extra = other["alpha"] != r["alpha"] and swapped["alpha"] != r["alpha"]
            if name == "armijo_reject" and set_name == "changed" and want <= r["outcomes"]:
                other = LC.run_host(sm, params[i], pl, case, dict(ls, theta_min=LC.ls_of("default")["theta_min"]))
                extra = other["alpha"] != r["alpha"]
            if (want <= r["outcomes"] and extra and r["margin"] >= 10.0 * LC.MARGIN
                    and r["barrier_margin"] >= 10.0 * LC.BARRIER_MARGIN):
                found = dict(name=name, kind=kind, seed=seed, args=args, alpha0=alpha0)
                print(f"  {name:14s} {kind:14s} seed {seed:4d} {args}  trials "
                      f"{''.join(t.branch[0] for t in r['trace']) or '-'}  accepted {r['accepted']}  "
                      f"margin {r['margin']:.1e}  barrier {r['barrier_margin']:.1e}", flush=True)
                break
        if found is None:
            print(f"  {name:14s} NOT FOUND", flush=True)
        else:
            rows.append(found)
    return rows


def main():
    sm = helpers.load_package().srbd_model
    table = json.loads(LC.TABLE_PATH.read_text()) if LC.TABLE_PATH.exists() else {}
    args = [a for a in sys.argv[1:] if not a.startswith("--only=")]
    only = [n for a in sys.argv[1:] if a.startswith("--only=") for n in a[7:].split(",")]
    for batch_name in args or [b for b, v in LC.BATCHES.items() if v[2] != "one"]:
        print(batch_name, flush=True)
        table[batch_name] = search(sm, batch_name, only, table.get(batch_name, ()))
    LC.TABLE_PATH.write_text(json.dumps(table, indent=1) + "\n")


if __name__ == "__main__":
    main()
