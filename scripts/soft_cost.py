#!/usr/bin/env python3
"""Cost of softness: 65536 SRBD QPs (N = 20, nx = nu = 12, box u + box x) solved once with
hard boxes and once with the same boxes soft, on the batched fp64 kernels.

Same data, settings (bench.py's NMPC_SETTINGS: ric_alg 0 as box_u_n20) and timing (HIP
events on the handle's stream) as bench.py's IPM lines.  Prints one JSON line: ms per solve,
mean iterations, status counts and the bytes one iteration moves per QP, soft arrays and
soft state included.  A first measurement, not a pass / fail line.

Usage: python scripts/soft_cost.py [--batch 65536] [--steps 3] [--warmup 1] [--box-x 1.0]
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import bench  # noqa: E402  (device_shard, NMPC_SETTINGS, alg_bytes_per_qp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--box-x", type=float, default=1.0, help="half width of the state box")
    ap.add_argument("--z", type=float, default=10.0)
    ap.add_argument("--Z", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    os.environ["SRBD_IPM_LATENCY_MAX"] = "0"  # the batched kernels for the hard solve too
    pkg = bench.import_pkg()
    capi = pkg.capi
    device = torch.device("cuda", 0)
    batch, N = args.batch, args.N
    h = capi.Handle(N, 12, 12, 0, True, True, capacity=batch)
    dt, _, _, _ = bench.device_shard(pkg, h, N, "box_u", batch, 0, args.seed, device)
    f = dict(dtype=torch.float64, device=device)
    dt["lbx"] = torch.full((batch, N + 1, 12), -args.box_x, **f)
    dt["ubx"] = torch.full((batch, N + 1, 12), args.box_x, **f)
    soft_t = {"soft_u": torch.ones(batch, N, 12, **f), "soft_x": torch.ones(batch, N + 1, 12, **f)}
    for fam, n in (("u", N), ("x", N + 1)):
        soft_t["Zl_" + fam] = soft_t["Zu_" + fam] = torch.full((batch, n, 12), args.Z, **f)
        soft_t["zl_" + fam] = soft_t["zu_" + fam] = torch.full((batch, n, 12), args.z, **f)
    sol_t = {"x": torch.zeros(batch, N + 1, 12, **f), "u": torch.zeros(batch, N, 12, **f),
             "pi": torch.zeros(batch, N + 1, 12, **f),
             "status": torch.zeros(batch, dtype=torch.int32, device=device),
             "iter": torch.zeros(batch, dtype=torch.int32, device=device)}
    data = capi.Data(**{k: (None if dt.get(k) is None else dt[k].data_ptr()) for k in capi.DATA_FIELDS})
    sol = capi.Solution(**{k: (sol_t[k].data_ptr() if k in sol_t else None) for k in capi.SOL_FIELDS})
    soft = capi.Soft(**{k: (soft_t[k].data_ptr() if k in soft_t else None) for k in capi.SOFT_FIELDS})
    settings = capi.settings_struct(bench.NMPC_SETTINGS)
    ext = torch.cuda.ExternalStream(h.stream(), device=device)

    def timed(run):
        for _ in range(args.warmup):
            run()
        h.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(ext)
        for _ in range(args.steps):
            run()
        ev1.record(ext)
        h.synchronize()
        st = sol_t["status"].cpu().numpy()
        return {"ms": round(ev0.elapsed_time(ev1) / args.steps, 3),
                "mean_iter": round(float(sol_t["iter"].float().mean()), 3),
                "status_counts": {int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}}

    hard = timed(lambda: h.solve_device(batch, settings, data, sol))
    softr = timed(lambda: h.solve_soft_device(batch, settings, data, soft, sol))
    # bytes one iteration streams per QP: the QP data and both boxes, read once by RB; soft: + the
    # 5 soft arrays per family (RB, F1, B2, F2 each read them) and the soft state rows
    # (RB 12 read + 6 written, F1 6 + 6, B2 12, F2 12 + 6 = 60 rows of 12 per family and stage)
    qp_bytes = bench.alg_bytes_per_qp(N, constraints="box_u") + 8 * 2 * (N + 1) * 12
    rows = (2 * N + 1) * 12
    soft_bytes = 8 * rows * (4 * 5 + 60)
    out = {"script": "soft_cost", "batch": batch, "N": N, "box_x": args.box_x, "z": args.z, "Z": args.Z,
           "ric_alg": bench.NMPC_SETTINGS["ric_alg"], "hard": hard, "soft": softr,
           "qp_bytes_per_iter": qp_bytes, "soft_extra_bytes_per_iter": soft_bytes,
           "soft_over_hard_ms": round(softr["ms"] / hard["ms"], 3)}
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()
