#!/usr/bin/env python3
"""Headline parity runs: iterations-to-convergence (centralized
||grad_R|| < 0.1) and wall-clock on the shipped datasets, matching the
reference driver configuration (5 robots, r=5, greedy RBCD).

Usage: python scripts/headline.py --dataset sphere2500 --robots 5 \
          [--device cuda:0] [--partition contiguous|multilevel] \
          [--selection greedy|colored] [--accel] [--max-iters 1000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--robots", type=int, default=5)
    ap.add_argument("--r", type=int, default=5)
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--partition", default="contiguous")
    ap.add_argument("--selection", default="greedy")
    ap.add_argument("--accel", action="store_true")
    ap.add_argument("--tr-iters", type=int, default=1,
                    help="trust-region steps per RBCD round (reference: 1)")
    ap.add_argument("--max-iters", type=int, default=1000)
    ap.add_argument("--tol", type=float, default=0.1)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--dump-trajectory", default=None,
                    help="write the final rounded global trajectory as "
                         "CSV (reference PartitionInitial.cpp:329-335)")
    ap.add_argument("--driver", default="dist", choices=["dist", "local"])
    ap.add_argument("--certify", action="store_true",
                    help="after the run, certify global optimality of the "
                         "lifted iterate (min eigenvalue of Q - Lambda) and "
                         "add the verdict to the JSON line")
    ap.add_argument("--cert-basis", type=int, default=None, metavar="B",
                    help="with --certify: thick-restart Lanczos in a window "
                         "of B vectors (basis memory N (B + 1) doubles)")
    ap.add_argument("--cert-max-iters", type=int, default=None, metavar="M",
                    help="with --certify: Lanczos step budget (default 512)")
    ap.add_argument("--cert-method", default=None,
                    choices=["lanczos", "lobpcg"],
                    help="with --certify or --refine: the certificate's "
                         "eigensolver (default lanczos)")
    ap.add_argument("--cert-block", type=int, default=None, metavar="M",
                    help="with --cert-method lobpcg: block size (default "
                         "rank + 1)")
    ap.add_argument("--refine", action="store_true",
                    help="certified solve: refine the gathered iterate to "
                         "criticality on the device, certify, and climb the "
                         "rank staircase on a not-optimal verdict")
    ap.add_argument("--round", action="store_true",
                    help="round the lifted iterate to SE(d) on the device "
                         "and add the rounded cost, the relaxation cost and "
                         "the suboptimality gap to the JSON line (with "
                         "--refine: of the certified solve's final level)")
    return ap


def rounding_fields(args, rounding, seconds=None):
    """JSON fields of a `RoundingResult` under --round; nothing without
    the flag, so the default output line is unchanged."""
    if not args.round or rounding is None:
        return {}
    out = rounding.as_dict()
    if seconds is not None:
        out["round_s"] = seconds
    return out


def round_gathered(args, meas, n, d, Xt):
    """--round without --refine: round the iterate as it stands."""
    import torch
    from dpo_amd.quadratic import assemble_connection_laplacian
    from dpo_amd.rounding import round_solution
    dev = torch.device(args.device)
    Q = assemble_connection_laplacian(meas, n, d)
    if dev.type != "cpu":
        Q = Q.to(dev)
    t0 = time.perf_counter()
    res = round_solution(Q, Xt.detach().to(dev), d, mode="svd")
    return rounding_fields(args, res, time.perf_counter() - t0)


def main():
    args = build_parser().parse_args()

    from dpo_amd.io_g2o import load_dataset
    from dpo_amd.comm import init_from_env

    meas, n = load_dataset(args.dataset)
    t_setup = time.perf_counter()
    if args.driver == "dist":
        from dpo_amd.dist_driver import DistributedRBCDDriver
        comm = init_from_env(args.device)
        drv = DistributedRBCDDriver(
            meas, n, args.robots, comm, r=args.r,
            partition=args.partition, acceleration=args.accel,
            device=args.device, selection=args.selection,
            tr_max_iterations=args.tr_iters)
    else:
        from dpo_amd.driver import MultiRobotDriver
        drv = MultiRobotDriver(
            meas, n, args.robots, r=args.r, partition=args.partition,
            acceleration=args.accel, device=args.device,
            selection=args.selection,
            tr_max_iterations=args.tr_iters)
    setup_s = time.perf_counter() - t_setup
    res = drv.run(max_iters=args.max_iters, gradnorm_tol=args.tol,
                  trace_file=args.trace)
    out = {
        "dataset": args.dataset, "robots": args.robots, "r": args.r,
        "poses": n, "edges": len(meas),
        "partition": args.partition, "selection": args.selection,
        "accel": args.accel, "device": args.device,
        "iterations": res.iterations, "converged": res.converged,
        "final_cost": res.final_cost, "final_gradnorm": res.final_gradnorm,
        "wall_s": res.elapsed_s, "setup_s": setup_s,
        "ms_per_iter": res.elapsed_s / max(res.iterations, 1) * 1e3,
    }
    rank = int(os.environ.get("RANK", "0"))
    if args.dump_trajectory:
        from dpo_amd.logger import PGOLogger
        T = (drv.final_trajectory() if args.driver == "local"
             else drv.gather_final_trajectory())
        if T is not None and rank == 0:
            lg = PGOLogger(os.path.dirname(args.dump_trajectory) or ".")
            lg.log_trajectory(meas[0].d, n, T,
                              os.path.basename(args.dump_trajectory))
    if args.refine:
        import torch
        Xt = (drv.gather_lifted_iterate() if args.driver == "dist"
              else drv._gather_global_x().reshape(-1, args.r))
        if Xt is not None and rank == 0:
            from dpo_amd.refine import certified_solve
            kw = {}
            if args.cert_basis is not None:
                kw["basis_size"] = args.cert_basis
            if args.cert_max_iters is not None:
                kw["max_iters"] = args.cert_max_iters
            if args.cert_method is not None:
                kw["method"] = args.cert_method
            if args.cert_block is not None:
                kw["block_size"] = args.cert_block
            t_cert = time.perf_counter()
            stair = certified_solve(
                meas, n, meas[0].d,
                Xt.detach().to(torch.device(args.device)), certify_kw=kw,
                round=args.round)
            out.update(stair.as_dict())
            out["certified_solve_s"] = time.perf_counter() - t_cert
    elif args.certify:
        import torch
        Xt = (drv.gather_lifted_iterate() if args.driver == "dist"
              else drv._gather_global_x().reshape(-1, args.r))
        if Xt is not None and rank == 0:
            from dpo_amd.certify import certify_solution
            kw = {}
            if args.cert_basis is not None:
                kw["basis_size"] = args.cert_basis
            if args.cert_max_iters is not None:
                kw["max_iters"] = args.cert_max_iters
            if args.cert_method is not None:
                kw["method"] = args.cert_method
            if args.cert_block is not None:
                kw["block_size"] = args.cert_block
            t_cert = time.perf_counter()
            cert = certify_solution(
                meas, n, meas[0].d,
                Xt.detach().to(torch.device(args.device)), **kw)
            out.update(cert.as_dict())
            out["certificate_s"] = time.perf_counter() - t_cert
    if args.round and not args.refine:
        Xt = (drv.gather_lifted_iterate() if args.driver == "dist"
              else drv._gather_global_x().reshape(-1, args.r))
        if Xt is not None and rank == 0:
            out.update(round_gathered(args, meas, n, meas[0].d, Xt))
    if rank == 0:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
