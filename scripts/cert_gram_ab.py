#!/usr/bin/env python3
"""A/B study: the two Gram kernels of the certificate's Lanczos step
(docs/DESIGN.md §14).

Contenders, on the same operator and the same stored basis:
  * column — k_cert_gram, one workgroup per stored vector (the
             unrestarted path's kernel)
  * split  — k_cert_gram_split + k_cert_gram_finish, rows of N divided
             over the grid (the thick-restart window's kernel)

Timed: one whole Lanczos step (operator, CGS2 against 64 stored vectors,
normalisation) through hip_backend.cert_lanczos_window, on random unit
vectors over a synthetic SE(3) grid (no solve). The two are alternated
inside every round; each sample is a host clock around `reps` steps that
ends in a device synchronise. Prints one JSON line per (N, kernel) and
writes profiles/cert_gram_ab.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STORED = 64


def bench_case(side, device, rounds, target_s):
    import torch
    from dpo_amd.ops import hip_backend as hb
    from dpo_amd.ops.cpu_ref import CERT_HDR
    from dpo_amd.quadratic import assemble_connection_laplacian
    from dpo_amd.synthetic import grid3d_soa

    ma, n = grid3d_soa(side=side, seed=1)
    Q = assemble_connection_laplacian(ma, n, 3).to(device)
    N = 4 * n
    g = torch.Generator().manual_seed(0)
    lam = torch.randn(n, 3, 3, dtype=torch.float64, generator=g)
    lam = (0.5 * (lam + lam.transpose(1, 2))).contiguous().to(device)
    V = torch.empty(STORED + 1, N, dtype=torch.float64, device=device)
    for j in range(STORED):
        v = torch.randn(N, dtype=torch.float64, generator=g)
        V[j] = (v / torch.linalg.norm(v)).to(device)
    ctl0 = torch.zeros(CERT_HDR + 2 * STORED, dtype=torch.float64,
                       device=device)
    ctl = ctl0.clone()
    j = STORED - 1          # the step that orthogonalises against 64

    def step(mode):
        hb.cert_lanczos_window(Q, lam, V, ctl, j, 1, gram=mode)

    def sample(mode, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            step(mode)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    # numerics on the same inputs, and warm-up of both code paths
    outs = {}
    for mode in ("column", "split"):
        ctl.copy_(ctl0)
        step(mode)
        step(mode)
        h = ctl.cpu()
        outs[mode] = (float(h[CERT_HDR + j]),
                      float(h[CERT_HDR + STORED + j]))
    reps = max(3, int(target_s / max(sample("column", 3), 1e-6)))
    times = {"column": [], "split": []}
    for _ in range(rounds):
        for mode in ("column", "split"):
            times[mode].append(sample(mode, reps))
    # bytes a step must move through the stored vectors: CGS2 reads the
    # 64 columns four times (2 Gram, 2 subtract)
    basis_bytes = 4.0 * STORED * N * 8
    recs = []
    for mode in ("column", "split"):
        med = statistics.median(times[mode])
        recs.append({
            "N": N, "poses": n, "stored_vectors": STORED, "gram": mode,
            "launches_per_step": 6 if mode == "column" else 8,
            "step_us_median": med * 1e6,
            "step_us_min": min(times[mode]) * 1e6,
            "step_us_max": max(times[mode]) * 1e6,
            "rounds": rounds, "reps_per_sample": reps,
            "basis_GBps_over_step": basis_bytes / med / 1e9,
            "alpha": outs[mode][0], "beta": outs[mode][1],
        })
        print(json.dumps(recs[-1]), flush=True)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default="profiles/cert_gram_ab.json")
    ap.add_argument("--sides", nargs="*", type=int,
                    default=[6, 14, 22, 100],
                    help="grid sides, N = 4 side^3: 864, 10 976, 42 592, 4e6")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--target-s", type=float, default=0.5,
                    help="seconds of work per timed sample")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "cert_gram_ab.py needs a GPU"
    allr = []
    for s in args.sides:
        allr += bench_case(s, args.device, args.rounds, args.target_s)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(allr, f, indent=1)


if __name__ == "__main__":
    main()
