#!/usr/bin/env python3
"""Single-robot full-batch pose-graph optimization (the reference's
examples/SingleRobotExample.cpp): chordal init + RTR at r = d (no rank
relaxation) with the batch knob set {tol 1e-1, 10 outer, 50 inner,
Delta0 10}.

python scripts/single_robot.py --dataset sphere2500 [--device cuda:0]
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
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--dump-trajectory", default=None)
    ap.add_argument("--certify", action="store_true",
                    help="certify global optimality of the result (min "
                         "eigenvalue of Q - Lambda) and add the verdict to "
                         "the JSON line")
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
                    help="certified solve: refine the result to criticality "
                         "on the device, certify, and climb the rank "
                         "staircase on a not-optimal verdict")
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

    from dpo_amd.agent import PGOAgent
    from dpo_amd.io_g2o import load_dataset
    from dpo_amd.types import PGOAgentParams

    meas, n = load_dataset(args.dataset)
    d = meas[0].d
    for m in meas:
        m.r1 = m.r2 = 0
    odometry = [m for m in meas if m.p1 + 1 == m.p2]
    loop_closures = [m for m in meas if m.p1 + 1 != m.p2]

    a = PGOAgent(0, PGOAgentParams(d=d, r=d, device=args.device))
    a.set_pose_graph(odometry, loop_closures, [])
    t0 = time.perf_counter()
    Topt = a.local_pose_graph_optimization()
    wall = time.perf_counter() - t0
    res = a.last_opt_result
    out = {
        "dataset": args.dataset, "poses": n, "edges": len(meas),
        "device": args.device,
        "f_init": res.f_init, "f_opt": res.f_opt,
        "grad_norm_init": res.grad_norm_init,
        "grad_norm_opt": res.grad_norm_opt,
        "wall_s": wall,
    }
    if args.certify or args.refine or args.round:
        import numpy as np
        import torch
        # r = d: the lifted iterate is the trajectory itself, transposed
        Xt = torch.from_numpy(np.ascontiguousarray(Topt.T)).to(
            torch.device(args.device))
        kw = {}
        if args.cert_basis is not None:
            kw["basis_size"] = args.cert_basis
        if args.cert_max_iters is not None:
            kw["max_iters"] = args.cert_max_iters
        if args.cert_method is not None:
            kw["method"] = args.cert_method
        if args.cert_block is not None:
            kw["block_size"] = args.cert_block
        if args.refine:
            from dpo_amd.refine import certified_solve
            t_cert = time.perf_counter()
            stair = certified_solve(meas, n, d, Xt, certify_kw=kw,
                                    round=args.round)
            out.update(stair.as_dict())
            out["certified_solve_s"] = time.perf_counter() - t_cert
        elif args.certify:
            from dpo_amd.certify import certify_solution
            cert = certify_solution(meas, n, d, Xt, **kw)
            out.update(cert.as_dict())
        if args.round and not args.refine:
            out.update(round_gathered(args, meas, n, d, Xt))
    print(json.dumps(out))
    if args.dump_trajectory:
        from dpo_amd.logger import PGOLogger
        lg = PGOLogger(os.path.dirname(args.dump_trajectory) or ".")
        lg.log_trajectory(d, n, Topt,
                          os.path.basename(args.dump_trajectory))


if __name__ == "__main__":
    main()
