#!/usr/bin/env python3
"""Stand-alone timing of the dense preconditioner apply (no solver loop).

Calls only hip_backend.precond_dense on random symmetric fp32 matrices at
N = 1252, 5000 and 20000, r = 5, and prints one JSON object: per N the
median time of one call (the stand-alone entry: its zeroing launch plus the
apply), over at least 0.5 s of samples taken in 5 rounds that alternate
between the sizes.

    python scripts/precond_dense_ab.py [--out FILE] [--label NAME]
    python scripts/precond_dense_ab.py --calls 20     # for a counter run

It times the build it imports; to compare two revisions run it from each
checkout in turn (alternate the two commands) and keep both outputs.
--calls K skips the timing and issues exactly K calls per size, for a
profiler run that collects counters.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpo_amd.ops import hip_backend as hb  # noqa: E402

SIZES = (1252, 5000, 20000)
R = 5
ROUNDS = 5
ROUND_SECONDS = 0.12   # per size and round: 5 rounds >= 0.5 s of samples


def make(N, dev):
    g = torch.Generator().manual_seed(N)
    A = torch.randn(N, N, dtype=torch.float32, generator=g).to(dev)
    M = ((A + A.T) / (2.0 * N ** 0.5)).contiguous()
    V = torch.randn(N, R, dtype=torch.float64, generator=g).to(dev)
    return M, V, torch.empty_like(V)


def sample(M, V, out, reps):
    """Seconds per call over `reps` back-to-back calls (device events)."""
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        hb.precond_dense(M, V, out=out)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="build")
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("precond_dense_ab: needs a GPU")
    dev = "cuda:0"
    data = {N: make(N, dev) for N in args.sizes}
    if args.calls:
        for N, (M, V, out) in data.items():
            for _ in range(args.calls):
                hb.precond_dense(M, V, out=out)
        torch.cuda.synchronize()
        print(json.dumps({"label": args.label, "calls": args.calls,
                          "sizes": args.sizes}))
        return
    reps, samples = {}, {N: [] for N in args.sizes}
    for N, (M, V, out) in data.items():   # warm up, size the batches
        sample(M, V, out, 10)
        t = sample(M, V, out, 10)
        reps[N] = max(4, int(2e-3 / t))   # about 2 ms per sample
    for _ in range(ROUNDS):
        for N, (M, V, out) in data.items():
            spent = 0.0
            while spent < ROUND_SECONDS:
                t = sample(M, V, out, reps[N])
                samples[N].append(t)
                spent += t * reps[N]
    res = {"label": args.label, "r": R, "rounds": ROUNDS, "sizes": {}}
    for N in args.sizes:
        s = sorted(samples[N])
        med = statistics.median(s)
        res["sizes"][str(N)] = {
            "median_us": med * 1e6, "min_us": s[0] * 1e6,
            "p90_us": s[int(0.9 * (len(s) - 1))] * 1e6,
            "samples": len(s), "sampled_seconds": sum(s) * reps[N],
            "matrix_GBps": 4.0 * N * N / med * 1e-9}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
