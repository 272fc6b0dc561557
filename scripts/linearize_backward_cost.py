#!/usr/bin/env python3
"""Cost of the backward pass of the SRBD linearisation:
srbd_qp_srbd_linearize_backward_f64 for 65536 robots at generate_batch's linearisation points,
N = 20, each of none / box_u / cone, every output requested, with robots (every robot its own
mass, Lbody, mu, Q, Qf, R) and a plan (its own x_ref, feet and fz_max per stage) attached.

Call times, by device events around the call (the smallest of --runs after a warm-up):
  backward_ms   srbd_qp_srbd_linearize_backward_f64, all ten outputs
  forward_ms    srbd_qp_srbd_linearize_plan_f64 on the same handle, robots and plan, in the same run
beside the time the cotangents' bytes would take at the 6.3 TB/s this project measured as
achievable (README): derived from the byte count, not measured.
Kernel times come from a kernel trace taken in a run of its own:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- \
      python3 scripts/linearize_backward_cost.py --constraints cone --runs 2
  python3 scripts/linearize_backward_cost.py --kernel-trace DIR/.../run_kernel_trace.csv
The second command needs no GPU: it prints the median time of the stage, reduce and cost kernels of
the backward pass and of the forward's two.  A measurement, not a pass / fail line.

Usage: python scripts/linearize_backward_cost.py [--batch 65536] [--N 20] [--runs 5]
                                                 [--constraints none box_u cone]
"""
import argparse
import csv
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import bench  # noqa: E402  (import_pkg)

ACHIEVABLE_TBS = 6.3


def cotangent_bytes(batch, N, constraints):
    """Bytes of the cotangents the call reads: A, B, R, b, r per stage, Q, q per stage and the
    terminal one; ubu with box_u; D, lg with cone."""
    per = N * (3 * 144 + 2 * 12) + (N + 1) * (144 + 12)
    if constraints == "box_u":
        per += N * 12
    elif constraints == "cone":
        per += N * 288 + (N + 1) * 24
    return 8 * batch * per


def measure(pkg, constraints, B, N, runs, seed, xs, us):
    import torch
    capi, sm = pkg.capi, pkg.srbd_model
    dev = torch.device("cuda", 0)
    p = sm.SrbdParams()
    xs_t, us_t = torch.from_numpy(xs).to(dev), torch.from_numpy(us).to(dev)
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
    mp = capi.model_params(p)
    cot = {k: torch.randn(B, *shape, dtype=torch.float64, device=dev, generator=g)
           for k, shape in capi._lin_cot_shapes(N, constraints).items()}
    fwd, _ = capi.srbd_linearize(h, xs_t, us_t, constraints, params=mp, plan=plan)
    out = capi.srbd_linearize_backward(h, xs_t, us_t, cot, constraints, params=mp, plan=plan)

    def timed(fn):
        ms = []
        for _ in range(1 + runs):  # the first run warms up
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        return round(min(ms[1:]), 3)

    res = {"backward_ms": timed(lambda: capi.srbd_linearize_backward(h, xs_t, us_t, cot, constraints, params=mp,
                                                                     plan=plan, out=out)),
           "forward_ms": timed(lambda: capi.srbd_linearize(h, xs_t, us_t, constraints, params=mp, plan=plan, out=fwd))}
    nbytes = cotangent_bytes(B, N, constraints)
    res["cotangent_gb"] = round(nbytes / 1e9, 3)
    res["cotangent_ms_at_achievable"] = round(nbytes / (ACHIEVABLE_TBS * 1e12) * 1e3, 3)
    res["cotangent_tbs"] = round(nbytes / res["backward_ms"] / 1e9, 3)
    res["finite"] = bool(all(torch.isfinite(t).all() for t in out.values()))
    res["handle_gb"] = round(h.memory_bytes() / 1e9, 3)
    h.close()
    return res


def kernel_times(path):
    """Median kernel times (ms) out of a rocprofv3 kernel trace of one run of this script."""
    names = {"srbd_lin_bwd_stage_kernel": "backward_stage_kernel_ms", "srbd_lin_bwd_reduce_kernel": "backward_reduce_kernel_ms",
             "srbd_lin_bwd_cost_kernel": "backward_cost_kernel_ms", "srbd_lin_stage_kernel": "forward_stage_kernel_ms",
             "srbd_lin_cost_kernel": "forward_cost_kernel_ms"}
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for part, key in names.items():
                if part in row["Kernel_Name"]:
                    groups.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
                    break
    out = {k: round(statistics.median(v), 4) for k, v in groups.items()}
    out["launches"] = {k: len(v) for k, v in groups.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--constraints", nargs="+", default=["none", "box_u", "cone"], choices=["none", "box_u", "cone"])
    ap.add_argument("--kernel-trace", help="a rocprofv3 kernel trace (csv) of one run of this script: print its kernel times")
    args = ap.parse_args()
    out = {"script": "linearize_backward_cost", "batch": args.batch, "N": args.N}
    if args.kernel_trace:
        out["kernels"] = kernel_times(args.kernel_trace)
    else:
        pkg = bench.import_pkg()
        out["achievable_tbs"] = ACHIEVABLE_TBS
        sm = pkg.srbd_model
        xs, us, _ = sm.sample_trajectories(args.batch, args.N, args.seed, sm.SrbdParams())
        for c in args.constraints:
            out[c] = measure(pkg, c, args.batch, args.N, args.runs, args.seed, xs, us)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
