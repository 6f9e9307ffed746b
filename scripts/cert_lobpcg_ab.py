#!/usr/bin/env python3
"""A/B: the optimality certificate by thick-restart Lanczos
(basis_size=64, max_iters=4000) against LOBPCG (docs/DESIGN.md §20) on one
GPU, on a refined iterate: the chordal initialisation lifted to rank r and
refined to the certificate's gate by `refine_to_critical`. Case `ring8` is
the twisted 8-ring after one escape and a refinement at r = 3.

Runs alternate; times are medians of --reps repetitions after one warm-up
of each side. Nothing here is a pass/fail gate. Results are merged into
the JSON file under the case's name:

python scripts/cert_lobpcg_ab.py --case sphere2500 --out profiles/certify_lobpcg.json
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ring8():
    import numpy as np
    import torch
    from dpo_amd.types import RelativeSEMeasurement
    n = 8
    meas = [RelativeSEMeasurement(0, 0, k, (k + 1) % n, np.eye(2),
                                  np.zeros(2), 1.0, 1.0) for k in range(n)]
    X = torch.zeros(3 * n, 2, dtype=torch.float64)
    for k in range(n):
        a = 2 * math.pi * k / n
        X[3 * k, 0], X[3 * k, 1] = math.cos(a), math.sin(a)
        X[3 * k + 1, 0], X[3 * k + 1, 1] = -math.sin(a), math.cos(a)
    return meas, n, X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="sphere2500",
                    help="a dataset name, or ring8")
    ap.add_argument("--r", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block", type=int, default=None)
    ap.add_argument("--precond", default="auto")
    ap.add_argument("--lob-max-iters", type=int, default=512)
    ap.add_argument("--lmax-iters", type=int, default=64,
                    help="Lanczos steps of LOBPCG's lambda_max phase")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from dpo_amd.certify import certify_solution, escape_direction
    from dpo_amd.quadratic import assemble_connection_laplacian
    from dpo_amd.refine import build_preconditioner, refine_to_critical

    dev = torch.device(args.device)
    if args.case == "ring8":
        meas, n, X = ring8()
        d = 2
        Q = assemble_connection_laplacian(meas, n, d).to(dev)
        first = certify_solution(meas, n, d, X.to(dev))
        X0 = escape_direction(Q, X.to(dev), first.direction)
    else:
        from dpo_amd.chordal import chordal_initialization
        from dpo_amd.io_g2o import load_dataset
        from dpo_amd.manifold import lifting_matrix
        meas, n = load_dataset(args.case)
        d = meas[0].d
        T = chordal_initialization(d, n, meas)
        X0 = torch.from_numpy(np.ascontiguousarray(
            (lifting_matrix(d, args.r) @ T).T)).to(dev)
        Q = assemble_connection_laplacian(meas, n, d).to(dev)
    pre = build_preconditioner(Q, X0.shape[1], args.precond)
    ref = refine_to_critical(Q, X0, precond=pre)
    Xt = ref.Xt

    def run(**kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = certify_solution(meas, n, d, Xt, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t, res

    sides = {
        "lanczos": dict(basis_size=64, max_iters=4000),
        "lobpcg": dict(method="lobpcg", block_size=args.block, problem=pre,
                       max_iters=args.lob_max_iters,
                       lmax_iters=args.lmax_iters),
    }
    if Q.N < 65:       # a window of 64 vectors needs N > 64
        sides["lanczos"] = dict()
    times = {k: [] for k in sides}
    last = {}
    for rep in range(args.reps + 1):            # rep 0 is the warm-up
        for name, kw in sides.items():
            t, res = run(**kw)
            if rep:
                times[name].append(t)
            last[name] = res
    out = {"case": args.case, "lmax_iters": args.lmax_iters, "poses": n,
           "N": Q.N, "rank": Xt.shape[1], "reps": args.reps,
           "refine": ref.as_dict()}
    for name, res in last.items():
        rec = res.as_dict()
        rec["seconds"] = times[name]
        rec["median_s"] = statistics.median(times[name])
        rec["applications"] = (res.applications if name == "lobpcg"
                               else res.iterations)
        rec["basis_drops"] = res.basis_drops
        out[name] = rec
    print(json.dumps(out))
    if args.out:
        allr = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                allr = json.load(f)
        allr[f"{args.case}_lmax{args.lmax_iters}"] = out
        with open(args.out, "w") as f:
            json.dump(allr, f, indent=1)


if __name__ == "__main__":
    main()
