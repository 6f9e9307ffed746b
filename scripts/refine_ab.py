#!/usr/bin/env python3
"""A/B: global refinement to the certificate's gate on one GPU, on-device
(`refine_to_critical`) against the host trust-region loop
(`QuadraticOptimizer` batch mode on the same GPU tensors, three host
syncs per tCG iteration). Same start (chordal initialisation lifted to
rank r), tolerance, radius and budgets; runs alternate, medians reported.

python scripts/refine_ab.py --dataset sphere2500 [--reps 5] [--out F.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="sphere2500")
    ap.add_argument("--r", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precond", default="auto")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from dpo_amd.chordal import chordal_initialization
    from dpo_amd.io_g2o import load_dataset
    from dpo_amd.manifold import lifting_matrix
    from dpo_amd.quadratic import (QuadraticProblem,
                                   assemble_connection_laplacian)
    from dpo_amd.refine import (build_preconditioner, default_grad_tol,
                                refine_to_critical)
    from dpo_amd.solver import QuadraticOptimizer, TRParams
    from dpo_amd.types import OptAlgorithm

    meas, n = load_dataset(args.dataset)
    d, r = meas[0].d, args.r
    dev = torch.device(args.device)
    T = chordal_initialization(d, n, meas)
    X0 = torch.from_numpy(np.ascontiguousarray(
        (lifting_matrix(d, r) @ T).T)).to(dev)
    Q = assemble_connection_laplacian(meas, n, d).to(dev)
    tol = default_grad_tol(Q, X0)
    problem = QuadraticProblem(n, d, r, precond=args.precond)
    problem.set_q(Q)
    # both sides start from a built preconditioner
    pre = build_preconditioner(Q, r, args.precond)

    def device_run():
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = refine_to_critical(Q, X0, grad_tol=tol, precond=pre)
        torch.cuda.synchronize()
        return time.perf_counter() - t, res.grad_norm_final, res.f_final, \
            {"status": res.status, "outer": res.outer_steps,
             "inner": res.inner_iterations, "precond": res.precond}

    def host_run():
        opt = QuadraticOptimizer(
            problem, OptAlgorithm.RTR,
            TRParams(tolerance=tol, initial_radius=10.0, max_iterations=100,
                     max_inner_iterations=1000, time_bound_s=1e9))
        torch.cuda.synchronize()
        t = time.perf_counter()
        opt.optimize(X0.clone())
        torch.cuda.synchronize()
        # optimize() evaluates f and the gradient norm before and after
        return time.perf_counter() - t, opt.result.grad_norm_opt, \
            opt.result.f_opt, {}

    device_run(); host_run()                      # warm-up, both paths
    td, th = [], []
    for _ in range(args.reps):
        a = device_run(); b = host_run()
        td.append(a[0]); th.append(b[0])
    out = {"dataset": args.dataset, "r": r, "poses": n, "grad_tol": tol,
           "reps": args.reps, "device_s": td, "host_s": th,
           "device_median_s": statistics.median(td),
           "host_median_s": statistics.median(th),
           "host_over_device": statistics.median(th) / statistics.median(td),
           "device_grad_norm": a[1], "host_grad_norm": b[1],
           "device_f": a[2], "host_f": b[2], **a[3]}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
