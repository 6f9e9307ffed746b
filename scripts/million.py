#!/usr/bin/env python3
"""BASELINE.json config #5: synthetic 1M-pose grid3D, 8 agents, robust
(GNC_TLS) loop-closure rejection, on MI355X.

python scripts/million.py [--side 100] [--agents 8] [--rounds 300]
                          [--device cuda:0] [--outliers 0.1]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)  # side^3 poses
    ap.add_argument("--agents", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--outliers", type=float, default=0.1)
    ap.add_argument("--selection", default="colored")
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--mu-step", type=float, default=2.0)
    ap.add_argument("--init", default="gt-noisy",
                    choices=["odometry", "gt-noisy", "chordal"],
                    help="gt-noisy = warm start from perturbed ground "
                         "truth (a prior map); odometry = dead reckoning "
                         "(drifts over a 1M-pose chain)")
    ap.add_argument("--init-noise", type=float, default=0.05)
    ap.add_argument("--round", action="store_true",
                    help="after the run, round the iterate to SE(3) on the "
                         "device: adds round_ms and rounded_cost")
    return ap


def rounding_fields(args, drv, ma=None, n=0):
    """--round: round every agent's iterate on the device against the
    global anchor (round_ms, gather included) and evaluate f = 0.5 <Q X,
    X> of the rounded trajectory on the device, Q with the measurements'
    stored weights. Nothing without the flag."""
    if not args.round or drv is None:
        return {}
    import numpy as np
    import torch
    from dpo_amd import ops
    from dpo_amd.quadratic import assemble_connection_laplacian
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    T = drv.gather_final_trajectory(device=True)
    torch.cuda.synchronize()
    out = {"round_ms": (time.perf_counter() - t0) * 1e3}
    if T is not None:
        dev = torch.device(args.device)
        Xr = torch.from_numpy(np.ascontiguousarray(T.T)).to(dev)
        Q = assemble_connection_laplacian(ma, n, 3).to(dev)
        out["rounded_cost"] = float(ops.backend_for(Xr).round_cost(Q, Xr))
    return out


def main():
    args = build_parser().parse_args()

    import torch
    if args.device.startswith("cuda") and not torch.cuda.is_available():
        print("million.py requires a GPU (packed robust path)",
              file=sys.stderr)
        return
    from dpo_amd.comm import init_from_env
    from dpo_amd.dist_driver import DistributedRBCDDriver
    from dpo_amd.synthetic import grid3d_soa
    from dpo_amd.types import RobustCostType

    t0 = time.perf_counter()
    ma, n = grid3d_soa(side=args.side, outlier_prob=args.outliers, seed=7)
    t_gen = time.perf_counter() - t0
    print(f"# generated n={n} poses, {len(ma)} edges in {t_gen:.1f}s",
          file=sys.stderr)

    if args.init == "gt-noisy":
        # warm start from perturbed ground truth: rotations composed
        # with small random rotations, translations jittered
        import numpy as np
        from dpo_amd.synthetic import _random_rotations_batch
        from dpo_amd.liegroups import project_to_rotation_group
        rng = np.random.default_rng(11)
        T = ma.ground_truth.copy()
        Tv = T.reshape(3, n, 4).transpose(1, 0, 2)
        Rn = _random_rotations_batch(n, rng, args.init_noise)
        Tv[:, :, :3] = Tv[:, :, :3] @ Rn
        Tv[:, :, 3] += rng.standard_normal((n, 3)) * args.init_noise
        ma.warm_start = T
    elif args.init == "chordal":
        # 1M-pose chordal init on the GPU (SoA assembly + BSR-kernel
        # PCG). Outlier edges are included — in a
        # production robust run you would gate on is_known_inlier; here
        # the point is the solver's scale.
        from dpo_amd.chordal import chordal_initialization_soa
        t0c = time.perf_counter()
        ma.warm_start = chordal_initialization_soa(
            ma, n, device=args.device, tol=1e-6, max_iters=4000)
        print(f"# chordal init (SoA/GPU): "
              f"{time.perf_counter() - t0c:.2f}s", file=sys.stderr)
    comm = init_from_env(args.device)
    t0 = time.perf_counter()
    drv = DistributedRBCDDriver(
        ma, n, args.agents, comm, r=5, partition="contiguous",
        robust=RobustCostType.GNC_TLS, device=args.device,
        selection=args.selection)
    for a in drv.local_agents.values():
        a.params.robust_opt_inner_iters = args.inner
        a.robust_cost.params.gnc_mu_step = args.mu_step
        a.robust_cost.reset()
    t_setup = time.perf_counter() - t0
    print(f"# setup {t_setup:.1f}s", file=sys.stderr)

    t0 = time.perf_counter()
    res = drv.run(max_iters=args.rounds, gradnorm_tol=0.0)
    t_run = time.perf_counter() - t0

    # weight saturation / rejection statistics
    import numpy as np
    n_rej = n_kept = n_undecided = 0
    for a in drv.local_agents.values():
        if not hasattr(a, "_all_weights_dev"):
            continue
        w = a._all_weights_dev.cpu().numpy()
        lcw = w[len(a._odo_ma):]
        n_rej += int((lcw < 0.1).sum())
        n_kept += int((lcw > 0.9).sum())
        n_undecided += int(((lcw >= 0.1) & (lcw <= 0.9)).sum())

    out = {
        "config": "synthetic grid3D, robust GNC_TLS",
        "init": args.init,
        "poses": n, "edges": len(ma), "agents": args.agents,
        "outlier_fraction": args.outliers,
        "device": args.device, "selection": args.selection,
        "rounds": res.iterations,
        "cost_initial": res.trace[0][0], "cost_final": res.final_cost,
        "gradnorm_final": res.final_gradnorm,
        "lc_rejected": n_rej, "lc_kept": n_kept,
        "lc_undecided": n_undecided,
        "gen_s": t_gen, "setup_s": t_setup, "run_s": t_run,
        "ms_per_round": t_run / max(res.iterations, 1) * 1e3,
    }
    out.update(rounding_fields(args, drv, ma, n))
    if int(os.environ.get("RANK", "0")) == 0:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
