#!/usr/bin/env python3
"""A/B of the rounding stage: the device kernels (`rounding.round_anchor`,
what `get_trajectory_in_global_frame(device=True)` runs) against the
host loop (`PGOAgent._round_trajectory`: X copied to the host, one
np.linalg.svd per pose), on sphere2500, city10000 and the synthetic
1M-pose grid. The iterate is the odometry dead-reckoning trajectory
lifted to r = 5 with a small perturbation: rounding time does not depend
on how good the iterate is. Writes profiles/rounding.json.

python scripts/round_ab.py [--device cuda:0] [--side 100] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--side", type=int, default=100,
                    help="synthetic grid: side^3 poses")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps-below", type=int, default=20000,
                    help="repeat the host loop 3 times below this many "
                         "poses; once above (it is CPU-only and slow)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "rounding.json"))
    return ap


def lifted_iterate(T, d, r, seed=0):
    """(n (d+1), r) lifted iterate from a trajectory T (d, n (d+1))."""
    import numpy as np
    import torch
    from dpo_amd.manifold import lifting_matrix
    rng = np.random.default_rng(seed)
    X = (lifting_matrix(d, r) @ T).T
    X = X + 0.01 * rng.standard_normal(X.shape)
    return torch.from_numpy(np.ascontiguousarray(X))


def cases(side):
    from dpo_amd.io_g2o import load_dataset
    from dpo_amd.measurements import (as_measurement_array,
                                      odometry_initialization_array)
    from dpo_amd.synthetic import grid3d_soa
    for name in ("sphere2500", "city10000"):
        meas, n = load_dataset(name)
        ma = as_measurement_array(meas)
        T = odometry_initialization_array(ma.d, n,
                                          ma.select(ma.p1 + 1 == ma.p2))
        yield name, ma.d, n, T
    ma, n = grid3d_soa(side=side, seed=7)
    yield f"grid3d_side{side}", 3, n, ma.ground_truth


def main():
    args = build_parser().parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("round_ab.py measures on a GPU", file=sys.stderr)
        return 1
    from dpo_amd.agent import PGOAgent
    from dpo_amd.rounding import round_anchor
    r = 5
    rows = []
    for name, d, n, T in cases(args.side):
        dh = d + 1
        Xc = lifted_iterate(T, d, r)
        Xd = Xc.to(args.device)
        anchor = Xc[:dh].numpy().T.copy()

        def device_stage():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            traj, _ = round_anchor(Xd, d, anchor)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = traj.cpu().numpy()
            return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3, out

        for _ in range(args.warmup):
            device_stage()
        runs = [device_stage() for _ in range(args.reps)]
        dev_T = runs[-1][2]

        def host_loop():
            t0 = time.perf_counter()
            X = Xd.cpu().numpy().T
            out = PGOAgent._round_trajectory(
                SimpleNamespace(d=d, dh=dh, n=n), X, anchor[:, :d],
                anchor[:, d])
            return (time.perf_counter() - t0) * 1e3, out

        host = [host_loop()
                for _ in range(3 if n < args.host_reps_below else 1)]
        err = float(np.abs(dev_T - host[-1][1]).max())
        row = {
            "case": name, "poses": n, "d": d, "r": r,
            "device": args.device, "reps": args.reps,
            "device_ms_median": statistics.median(x[0] for x in runs),
            "device_ms_min": min(x[0] for x in runs),
            "device_ms_max": max(x[0] for x in runs),
            "device_to_numpy_ms_median":
                statistics.median(x[1] for x in runs),
            "host_loop_ms_median": statistics.median(x[0] for x in host),
            "host_loop_runs": len(host),
            "max_abs_difference": err,
        }
        row["speedup"] = row["host_loop_ms_median"] / \
            row["device_to_numpy_ms_median"]
        print(json.dumps(row))
        rows.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
