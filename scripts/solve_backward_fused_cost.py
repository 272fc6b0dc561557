#!/usr/bin/env python3
"""Cost of the fused backward pass robots / plan <- solve against the two chained
calls it replaces, in the setup of scripts/linearize_backward_cost.py: 65536 robots at
generate_batch's linearisation points, N = 20, each of none / box_u / cone, robots (every robot its
own mass, Lbody, mu, Q, Qf, R) and a plan (its own x_ref, feet and fz_max per stage) attached, all
ten outputs and grad x0.

In one run on one handle, after the handle's forward solve of the linearised QPs, alternating, by
device events, the smallest of --runs after a warm-up:
  chain_ms   srbd_qp_solve_backward_rows_f64 (all nine and the rows' gradients, into arrays that
             are allocated once outside the timing) + srbd_qp_srbd_linearize_backward_f64
  fused_ms   srbd_qp_srbd_solve_backward_f64
with torch.cuda.max_memory_allocated over each path above what the forward pass holds (the
chain's includes its gradient arrays), the handle's own memory, and the largest difference of an
output between the two relative to the output's largest entry.
Kernel times come from a kernel trace taken in a run of its own, per mode:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- \
      python3 scripts/solve_backward_fused_cost.py --constraints cone --runs 2
  python3 scripts/solve_backward_fused_cost.py --out FILE --kernel-trace cone=DIR/.../run_kernel_trace.csv
The second command needs no GPU: it adds the median time of the backward kernels to FILE.
A measurement, not a pass / fail line.

Usage: python scripts/solve_backward_fused_cost.py [--batch 65536] [--N 20] [--runs 5]
                                                   [--constraints none box_u cone] [--out FILE]
"""
import argparse
import csv
import json
import re
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import bench  # noqa: E402  (import_pkg)

# the forward solve whose solution the backward passes start from (tests/srbd_device.py's NMPC
# settings at tight tolerances, so that the active sets are beyond doubt)
FORWARD = dict(mode="Speed", iter_max=100, alpha_min=1e-8, mu0=1e2, tol_stat=1e-8, tol_eq=1e-8, tol_ineq=1e-8,
               tol_comp=1e-8, reg_prim=0.0, warm_start=0, pred_corr=1, ric_alg=0, split_step=1)
ACT_TOL, RANK_TOL = 1e-4, 1e-8
NINE = ("A", "B", "b", "Q", "S", "R", "q", "r", "x0")
ROWS = {"none": {}, "box_u": {"lbu": 12, "ubu": 12}, "cone": {"D": 288, "lg": 24, "ug": 24}}
KERNELS = ("srbd_solve_bwd_stage_kernel", "srbd_solve_bwd_cost_kernel", "srbd_lin_bwd_stage_kernel",
           "srbd_lin_bwd_reduce_kernel", "srbd_lin_bwd_cost_kernel", "backward_project_kernel", "backward_lift_kernel",
           "backward_grad_kernel", "backward_rows_kernel", "riccati")


def measure(pkg, constraints, B, N, runs, seed, xs, us, x0):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    dev = torch.device("cuda", 0)
    p = sm.SrbdParams()
    xs_t, us_t, x0_t = (torch.from_numpy(a).to(dev) for a in (xs, us, x0))
    g = torch.Generator(device=dev).manual_seed(seed)
    rand = lambda *shape: torch.rand(*shape, dtype=torch.float64, device=dev, generator=g)
    around = lambda v, spread, *shape: torch.tensor(v, dtype=torch.float64, device=dev) * (1.0 + spread * (2 * rand(*shape) - 1))
    robots = capi.Robots(mass=around(p.mass, 0.3, B), Lbody=around(p.Lbody, 0.3, B, 3), mu=around(p.mu, 0.3, B),
                         Q=around(p.Q, 0.5, B, 12), Qf=around(p.Qf, 0.5, B, 12), R=around(p.R, 0.5, B))
    shift = lambda v, width, *shape: torch.tensor(v, dtype=torch.float64, device=dev) + width * (2 * rand(*shape) - 1)
    plan = capi.Plan(x_ref=shift(p.x_ref, 0.3, B, N + 1, 12), foot_r=shift(p.foot_r, 0.15, B, N, 3),
                     foot_l=shift(p.foot_l, 0.15, B, N, 3), fz_max=150.0 + 450.0 * rand(B, N, 2))
    h = capi.Handle(N, 12, 12, 24 if constraints == "cone" else 0, constraints == "box_u", False, capacity=B)
    h.set_robots(model=robots)
    mp, st = capi.model_params(p), capi.settings_struct(FORWARD)
    qp, data = capi.srbd_linearize(h, xs_t, us_t, constraints, params=mp, plan=plan)
    data.x0 = x0_t.data_ptr()
    new = lambda rows: torch.zeros(B, rows, 12, dtype=torch.float64, device=dev)
    x, u, pi = new(N + 1), new(N), new(N + 1)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    sol = capi.Solution(x=x.data_ptr(), u=u.data_ptr(), pi=pi.data_ptr(), status=status.data_ptr())
    h.solve_device(B, st, data, sol)
    h.synchronize()
    gx, gu = 2.0 * x, 2.0 * u  # loss = sum x^2 + sum u^2
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()

    # the chain: its gradient arrays are the caller's
    torch.cuda.reset_peak_memory_stats()
    like = dict(qp, x0=x0_t)
    grads = {k: torch.empty_like(like[k]) for k in NINE}
    rows = {k: torch.empty(B, N + (k in ("lg", "ug")), w, dtype=torch.float64, device=dev) for k, w in ROWS[constraints].items()}
    grad = capi.Grad(**{k: v.data_ptr() for k, v in grads.items()})
    grad_rows = capi.GradRows(**{k: v.data_ptr() for k, v in rows.items()}) if rows else None
    cot = {**grads, **rows}

    def chain(out=None):
        h.solve_backward_rows_device(B, st, data, sol, gx, gu, grad, grad_rows, act_tol=ACT_TOL, rank_tol=RANK_TOL)
        return capi.srbd_linearize_backward(h, xs_t, us_t, cot, constraints, params=mp, plan=plan, out=out)

    out_c = chain()
    counts = h.backward_active(B).sum(dim=0).tolist()
    torch.cuda.synchronize()
    chain_peak = torch.cuda.max_memory_allocated() - held

    def fused(out=None):
        return capi.srbd_solve_backward(h, xs_t, us_t, data, sol, gx, gu, constraints, params=mp, plan=plan,
                                        act_tol=ACT_TOL, rank_tol=RANK_TOL, settings=st, want_x0=True, out=out)

    handle_before = h.memory_bytes()
    out_f = fused()
    torch.cuda.synchronize()

    def once(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    ms = {"chain": [], "fused": []}
    for _ in range(1 + runs):  # the first round warms up
        ms["chain"].append(once(lambda: chain(out_c)))
        ms["fused"].append(once(lambda: fused(out_f)))
    res = {"chain_ms": round(min(ms["chain"][1:]), 3), "fused_ms": round(min(ms["fused"][1:]), 3)}
    res["fused_over_chain"] = round(res["fused_ms"] / res["chain_ms"], 3)
    worst = 0.0
    for k, v in out_c.items():
        scale = float(v.abs().max())
        worst = max(worst, float((out_f[k] - v).abs().max()) / scale if scale > 0 else 0.0)
    worst = max(worst, float((out_f["x0"] - grads["x0"]).abs().max()) / float(grads["x0"].abs().max()))
    res["fused_minus_chain_rel"] = worst
    res["finite"] = bool(all(torch.isfinite(t).all() for t in out_f.values()))
    res["forward_solved"] = int((status == 0).sum())
    res["active"] = dict(zip(("pinned", "rows_accepted", "rows_dropped"), counts))
    res["handle_gb"] = round(h.memory_bytes() / 1e9, 3)
    res["compact_buffer_gb"] = round((h.memory_bytes() - handle_before) / 1e9, 3)
    res["chain_torch_peak_gb"] = round(chain_peak / 1e9, 3)
    # the fused path without the chain's arrays
    del grads, rows, cot, grad, grad_rows, out_c
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fused()
    torch.cuda.synchronize()
    res["fused_torch_peak_gb"] = round((torch.cuda.max_memory_allocated() - base) / 1e9, 3)
    h.close()
    return res


def kernel_times(path):
    """Median kernel times (ms) of the backward kernels out of a rocprofv3 kernel trace of one run."""
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            for part in KERNELS:
                if part in name:
                    m = re.search(r"(\w*" + part + r"\w*)", name)
                    groups.setdefault(m.group(1), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
                    break
    out = {k: round(statistics.median(v), 4) for k, v in sorted(groups.items())}
    out["launches"] = {k: len(v) for k, v in sorted(groups.items())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--constraints", nargs="+", default=["none", "box_u", "cone"], choices=["none", "box_u", "cone"])
    ap.add_argument("--kernel-trace", nargs="+", default=[], metavar="MODE=CSV",
                    help="rocprofv3 kernel traces (csv) of one run of this script per mode: add their kernel times")
    ap.add_argument("--out", help="a JSON file to write (an existing one is added to)")
    args = ap.parse_args()
    out = {}
    if args.out and Path(args.out).exists():
        out = json.loads(Path(args.out).read_text())
    out.update({"script": "solve_backward_fused_cost", "batch": args.batch, "N": args.N})
    if args.kernel_trace:
        for item in args.kernel_trace:
            mode, path = item.split("=", 1)
            out.setdefault("kernels", {})[mode] = kernel_times(path)
    else:
        pkg = bench.import_pkg()
        sm = pkg.srbd_model
        xs, us, x0 = sm.sample_trajectories(args.batch, args.N, args.seed, sm.SrbdParams())
        for c in args.constraints:
            out[c] = measure(pkg, c, args.batch, args.N, args.runs, args.seed, xs, us, x0)
    text = json.dumps(out, indent=1)
    if args.out:
        Path(args.out).write_text(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
