#!/usr/bin/env python3
"""Cost of the backward pass of the batched QP solve: srbd_qp_solve_backward_f64
for 65536 SRBD QPs (generate_batch's, linearised on the device), N = 20, nx = nu = 12, once without
constraints and once with input boxes (BOX_U, the NMPC's configuration); with --constraints cone
srbd_qp_solve_backward_rows_f64 on the SRBD CONE QPs (ng = 24: the friction cone as rows on the
inputs), all fourteen gradients.

Call times, by device events around the call (the smallest of --runs after a warm-up):
  forward_ms             srbd_qp_solve_f64 with the NMPC settings
  backward_all_ms        the whole backward call with all nine gradients
  backward_vectors_ms    the same with q, r, b, x0 only
  backward_x0_ms         the same with x0 only: the mask kernel and the adjoint solve, plus a
                         gradient kernel that writes 96 bytes per QP
Kernel times come from a kernel trace taken in a run of its own:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- \
      python3 scripts/backward_cost.py --constraints box_u --runs 2
  python3 scripts/backward_cost.py --kernel-trace DIR/.../run_kernel_trace.csv
The second command needs no GPU.  It prints the median time of the mask kernel, of the adjoint's
Riccati kernel, of the gradient kernel of the five matrices and of the kernel of the vector
gradients with four outputs and with one (told apart by the grid's y size); all nine gradients
are the two kernels together.  With cone: the projection and the lift kernel, the bytes each
moves at least (every input and output once) and that over its time.  Beside them, the written bytes over the time and the 6.3 TB/s
this project measured as achievable (README).  A measurement, not a pass / fail line.

Usage: python scripts/backward_cost.py [--batch 65536] [--N 20] [--runs 5] [--constraints none box_u cone]
"""
import argparse
import csv
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import bench  # noqa: E402  (import_pkg, NMPC_SETTINGS, device_shard, shard_buffers)

ACHIEVABLE_TBS = 6.3
VECTORS = ("q", "r", "b", "x0")


def written_bytes(batch, N, names, nx=12, nu=12):
    """Bytes the gradient kernel writes for the outputs `names`."""
    per = {"A": N * nx * nx, "B": N * nx * nu, "Q": (N + 1) * nx * nx, "S": N * nu * nx, "R": N * nu * nu,
           "q": (N + 1) * nx, "r": N * nu, "b": N * nx, "x0": nx}
    return 8 * batch * sum(per[n] for n in names)


def rows_bytes(batch, N, ng, nx=12, nu=12):
    """Bytes the projection and the lift kernel move at least: every input and output once."""
    stage = nx * nu + nu * nx + nu * nu  # B, S, R
    active = ng * nu + 2 * ng + nu       # D, lg, ug (ug masked: its mask instead), u
    project = (2 * stage + 2 * nu + active) * N
    lift = (stage + active + 2 * nu + 6 * nx) * N + ng * nu * N + 2 * ng * (N + 1) + 2 * nu * N
    return 8 * batch * project, 8 * batch * lift


def measure(pkg, constraints, B, N, runs, seed):
    import torch
    capi = pkg.capi
    device = torch.device("cuda", 0)
    ng = 24 if constraints == "cone" else 0
    h = capi.Handle(N, 12, 12, ng, constraints == "box_u", False, capacity=B)
    dt, _, _, _ = bench.device_shard(pkg, h, N, constraints, B, 0, seed, device)
    sol_t, data, sol = bench.shard_buffers(capi, dt, B, N, "f64", device)
    st = capi.settings_struct(bench.NMPC_SETTINGS)
    g = torch.Generator(device=device).manual_seed(seed)
    gx = torch.rand(B, N + 1, 12, dtype=torch.float64, device=device, generator=g) * 2 - 1
    gu = torch.rand(B, N, 12, dtype=torch.float64, device=device, generator=g) * 2 - 1
    grads = {n: torch.empty_like(dt[n]) for n in capi.GRAD_FIELDS}
    act_tol = float(np.sqrt(st.tol_comp))

    def timed(fn):
        ms = []
        for _ in range(1 + runs):  # the first run allocates the buffers and warms up
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        return round(min(ms[1:]), 3)

    def backward(names):
        grad = capi.Grad(**{n: grads[n].data_ptr() for n in names})
        return lambda: h.solve_backward_device(B, st, data, sol, gx, gu, grad, act_tol=act_tol)

    out = {"forward_ms": timed(lambda: h.solve_device(B, st, data, sol))}
    out["status_ok"] = int((sol_t["status"] == 0).sum())
    if constraints == "cone":
        shapes = {"D": (B, N, ng * 12), "lg": (B, N + 1, ng), "ug": (B, N + 1, ng)}
        grows = {n: torch.empty(*s, dtype=torch.float64, device=device) for n, s in shapes.items()}
        grad = capi.Grad(**{n: grads[n].data_ptr() for n in capi.GRAD_FIELDS})
        rows = capi.GradRows(**{n: t.data_ptr() for n, t in grows.items()})
        call = lambda g, r: (lambda: h.solve_backward_rows_device(B, st, data, sol, gx, gu, g, r, act_tol=act_tol))
        out["backward_all_ms"] = timed(call(grad, rows))   # all fourteen (no boxes: lbu, ubu do not exist)
        out["backward_nine_ms"] = timed(call(grad, None))  # no lift kernel
        out["backward_rows_ms"] = timed(call(None, rows))  # no gradient kernel
        counts = h.backward_active(B).double().mean(dim=0)
        out["accepted_per_qp"], out["dropped_per_qp"] = round(float(counts[1]), 2), round(float(counts[2]), 2)
        out["active_per_qp"] = round(float(counts[1] + counts[2]), 2)
        out["finite"] = bool(all(torch.isfinite(t).all() for t in list(grads.values()) + list(grows.values())))
        out["project_gb"], out["lift_gb"] = (round(b / 1e9, 3) for b in rows_bytes(B, N, ng))
        out["handle_gb"] = round(h.memory_bytes() / 1e9, 2)
        h.close()
        return out
    out["backward_all_ms"] = timed(backward(capi.GRAD_FIELDS))
    out["backward_vectors_ms"] = timed(backward(VECTORS))
    out["backward_x0_ms"] = timed(backward(("x0",)))
    if constraints == "box_u":
        pins = h.backward_pinned(B)
        out["pinned_per_qp"] = round(float(pins.double().mean()), 2)
    out["finite"] = bool(all(torch.isfinite(t).all() for t in grads.values()))
    out["written_gb_all"] = round(written_bytes(B, N, capi.GRAD_FIELDS) / 1e9, 3)
    out["handle_gb"] = round(h.memory_bytes() / 1e9, 2)
    h.close()
    return out


def kernel_times(path, batch, N):
    """Median kernel times (ms) out of a rocprofv3 kernel trace of one run of this script."""
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            ms = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
            if "backward_mask_kernel" in name:
                key = "mask_kernel_ms"
            elif "backward_project_kernel" in name:
                key = "project_kernel_ms"
            elif "backward_lift_kernel" in name:
                key = "lift_kernel_ms"
            elif "backward_grad_kernel" in name:  # the five matrices (launched with all nine only)
                key = "grad_kernel_matrices_ms"
            elif "backward_rows_kernel" in name:
                key = {4: "grad_kernel_vectors_ms", 1: "grad_kernel_x0_ms"}.get(int(row["Grid_Size_Y"]),
                                                                                "grad_kernel_other_ms")
            elif "riccati_unconstr_kernel" in name:
                key = "riccati_kernel_ms"
            else:
                continue
            groups.setdefault(key, []).append(ms)
    out = {k: round(statistics.median(v), 4) for k, v in groups.items()}
    out["launches"] = {k: len(v) for k, v in groups.items()}
    if "grad_kernel_matrices_ms" in out and "grad_kernel_vectors_ms" in out:  # all nine: both kernels
        out["grad_kernel_all_ms"] = round(out["grad_kernel_matrices_ms"] + out["grad_kernel_vectors_ms"], 4)
    for key, names in (("grad_kernel_all_ms", ("A", "B", "b", "Q", "S", "R", "q", "r", "x0")),
                       ("grad_kernel_matrices_ms", ("A", "B", "Q", "S", "R")),
                       ("grad_kernel_vectors_ms", VECTORS)):
        if key in out:
            out[key.replace("_ms", "_written_tbs")] = round(written_bytes(batch, N, names) / out[key] / 1e9, 3)
    for key, nbytes in zip(("project_kernel_ms", "lift_kernel_ms"), rows_bytes(batch, N, 24)):
        if key in out:
            out[key.replace("_ms", "_tbs")] = round(nbytes / out[key] / 1e9, 3)
    out["achievable_tbs"] = ACHIEVABLE_TBS
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--constraints", nargs="+", default=["none", "box_u"],
                    choices=["none", "box_u", "cone"])
    ap.add_argument("--kernel-trace", help="a rocprofv3 kernel trace (csv) of one run of this script: print its kernel times")
    args = ap.parse_args()
    out = {"script": "backward_cost", "batch": args.batch, "N": args.N}
    if args.kernel_trace:
        out["kernels"] = kernel_times(args.kernel_trace, args.batch, args.N)
    else:
        pkg = bench.import_pkg()
        for c in args.constraints:
            out[c] = measure(pkg, c, args.batch, args.N, args.runs, args.seed)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
