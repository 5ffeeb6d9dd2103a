#!/usr/bin/env python3
"""The statement side of an aggregate alone: the root over G leaf statements on the host (api.aggregate_root, up to 16
threads) against the device (api.AggregateVerifier.root: vp_lwe_chain, ag_leaf, ag_fold), random statements, no proofs.  One JSON line.

usage: tools/aggregate_root_speed.py [--n8] [--leaves 64,256,1024] [--runs 5]
  the level circuits give the verifier its shape only and are located as data (tools/export_circuits.py --aggregate ... levels makes them)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (the HIP runtime the library shares with it)

import vpbs_amd  # noqa: E402
from vpbs_amd import api, circuit_file  # noqa: E402

K, ELL, LOGB = 2, 4, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n8", action="store_true")
    ap.add_argument("--leaves", default="64,256,1024")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    N, n_lwe, log_n = (8, 6, 13) if args.n8 else (1024, 728, 16)
    leaves = [int(x) for x in args.leaves.split(",")]
    levels = api.aggregate_depth(max(leaves))
    circuits = [circuit_file.load(p) for p in circuit_file.find_aggregate_circuits(N, K, ELL, LOGB, n_lwe, log_n, levels)]
    rng = np.random.default_rng(1)
    f = lambda *shape: rng.integers(0, api.P, size=shape, dtype=np.uint64)
    vks = f(levels + 1, 68)
    ctx = vpbs_amd.Context(0, log_n_max=16)
    av = api.AggregateVerifier(ctx, api.AggregateShape(N, K, n_lwe, vks, circuits), max_leaves=max(leaves))
    rows = []
    for count in leaves:
        st = (f(4, N), f(count, n_lwe + 1), f(count, K * N), f(8, 4), rng.integers(0, 8, size=count), rng.integers(0, 4, size=count))
        want = api.aggregate_root(N, K, n_lwe, vks[0], *st)
        assert (av.root(*st) == want).all()          # and the warm-up of both
        host, device = [], []
        for _ in range(args.runs):                   # alternating, each call ends with its result on the host
            t = time.perf_counter()
            api.aggregate_root(N, K, n_lwe, vks[0], *st)
            host.append(1e3 * (time.perf_counter() - t))
            t = time.perf_counter()
            av.root(*st)
            device.append(1e3 * (time.perf_counter() - t))
        rows.append({"leaves": count, "host_ms": sorted(host), "device_ms": sorted(device)})
    av.close()
    ctx.close()
    print(json.dumps({"what": "root of an aggregate's statement, host (up to 16 threads) against device, N=%d n=%d, %d public inputs per leaf" %
                              (N, n_lwe, 2 * K * N + 77), "runs": args.runs, "rows": rows,
                      "host": {"cpus": len(os.sched_getaffinity(0)), "loadavg": os.getloadavg()[0]}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
