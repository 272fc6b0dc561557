#!/usr/bin/env python3
"""Cost of the plant's contact model, for 65536 robots and N = 20:
srbd_qp_srbd_advance_f64 alone, hip events around each launch on the handle's stream, after a
warm-up, the median (and the smallest) of --repeats launches, with a plan, a wrench and
--substeps plant steps:

  * "plain":      no contact on the handle (the kernels of before);
  * "contact":    a contact on flat ground with fallen / alive / sat;
  * "ground":     the same with a true ground of 16 maps of 256 x 256 and a map per robot;
  * "cleared":    the contact cleared again (the kernels of before).

Every launch starts from the same xs, us, x and state (copied back outside the events).  On a
library built from an older commit (SRBD_QP_LIB=...) only "plain" runs, for A/B runs.

Prints one JSON line.  A measurement, not a pass / fail line.

Usage: python scripts/contact_cost.py [--batch 65536] [--N 20] [--substeps 1] [--repeats 50]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import bench  # noqa: E402  (import_pkg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--substeps", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    pkg = bench.import_pkg()
    capi, sm = pkg.capi, pkg.srbd_model
    device = torch.device("cuda", 0)
    batch, N = args.batch, args.N
    p = sm.SrbdParams()
    rng = np.random.default_rng(args.seed)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    xr = np.array(p.x_ref, dtype=np.float64)
    xs0 = dev(xr + 0.05 * rng.normal(size=(batch, N + 1, 12)))
    u = np.empty((batch, N, 2, 6))
    u[..., 0:2] = rng.uniform(-60.0, 60.0, size=(batch, N, 2, 2))
    u[..., 2] = rng.uniform(-20.0, 200.0, size=(batch, N, 2))
    u[..., 3:6] = rng.uniform(-6.0, 6.0, size=(batch, N, 2, 3))
    us0 = dev(u.reshape(batch, N, 12))
    x0 = dev(xr + 0.05 * rng.normal(size=(batch, 12)))
    fz = rng.uniform(150.0, 300.0, size=(batch, N, 2))
    fz[rng.uniform(size=fz.shape) < 0.3] = 1.0  # swing stages
    plan = capi.Plan(foot_r=dev(np.array(p.foot_r) + rng.uniform(-0.1, 0.1, size=(batch, N, 3))),
                     foot_l=dev(np.array(p.foot_l) + rng.uniform(-0.1, 0.1, size=(batch, N, 3))), fz_max=dev(fz))
    wrench = dev(rng.uniform(-20.0, 20.0, size=(batch, 6)))
    h = capi.Handle(N, 12, 12, capacity=batch)
    ext = h.torch_stream()
    xs, us, x = xs0.clone(), us0.clone(), x0.clone()
    ints = lambda: torch.zeros(batch, dtype=torch.int32, device=device)
    state = [ints(), ints(), ints()]

    def advance_us():
        times = []
        with torch.cuda.stream(ext):
            for _ in range(5 + args.repeats):
                xs.copy_(xs0), us.copy_(us0), x.copy_(x0)
                for s in state:
                    s.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                capi.srbd_advance(h, xs, us, x=x, plan=plan, wrench=wrench, substeps=args.substeps, stream=h.stream())
                e1.record()
                times.append((e0, e1))
        torch.cuda.synchronize()
        t = [a.elapsed_time(b) * 1e3 for a, b in times[5:]]
        return [round(statistics.median(t), 1), round(min(t), 1)]

    out = {"script": "contact_cost", "batch": batch, "N": N, "substeps": args.substeps, "lib": str(capi.LIB_PATH),
           "advance_us": {"plain": advance_us()}}
    if hasattr(capi.lib(), "srbd_qp_srbd_set_contact_f64"):
        kw = dict(mu=0.4, Lt=(0.0, 0.05, 0.05), fz_hi=180.0, fz_contact=5.0, z_min=0.5, cos_tilt_min=0.5,
                  fallen=state[0], alive=state[1], sat=state[2])
        h.set_contact(capi.Contact(**kw))
        out["advance_us"]["contact"] = advance_us()
        out["fallen"], out["saturated"] = int(state[0].sum()), int((state[2] != 0).sum())
        maps = 16
        height = dev(rng.uniform(0.0, 0.05, size=(maps, 256, 256)))
        map_r = dev(rng.integers(0, maps, size=batch).astype(np.int32))
        h.set_contact(capi.Contact(ground=capi.Terrain(height, xr[6] - 6.4, xr[7] - 6.4, 0.05, map_r=map_r), **kw))
        out["advance_us"]["ground"] = advance_us()
        h.set_contact(None)
        out["advance_us"]["cleared"] = advance_us()
    print(json.dumps(out))
    h.close()


if __name__ == "__main__":
    main()
