#!/usr/bin/env python3
"""The statement side of an aggregate alone: the root over G leaf statements on the host (api.aggregate_root, up to 16
threads) against the device (api.AggregateVerifier.root: ag_leaf_pair, ag_fold_many), random statements, no proofs.  One JSON line.

usage: tools/aggregate_root_speed.py [--n8] [--leaves 64,256,1024] [--runs 5]
       tools/aggregate_root_speed.py --many 1,8,64 [--tree-leaves 8,64] [--runs 5] [--n8] [--shape-circuits-n8]
  the level circuits give the verifier its shape only and are located as data (tools/export_circuits.py --aggregate ... levels makes them)
  --many T[,T2,..]: MANY trees in one run.  For every T and every L of --tree-leaves: T trees of L leaves, random statements;
    api.AggregateVerifier.roots_many (one run) against T calls of AggregateVerifier.root (the same stages with one tree per call: what T
    runs cost, and with T = 1 what the single entry's wrapper costs) and against api.aggregate_root per tree on up to 16 host threads -- the
    three legs in turn, median and range of --runs after a warm-up -- and, from the library's HIP-event timers, the leaf-pair kernel of
    the one run (--runs runs with timing on).
  --shape-circuits-n8: size the proof verifiers by the level circuits of the N = 8, n = 6 set (no proof is read by this tool; a level beyond
    the exported ones reuses the last one's shape) while the statement keeps the paper's parameters."""
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


def many(args, N, n_lwe, log_n):
    """--many: see the module text"""
    from concurrent.futures import ThreadPoolExecutor
    trees, sizes = [int(x) for x in args.many.split(",")], [int(x) for x in args.tree_leaves.split(",")]
    levels = api.aggregate_depth(max(sizes))
    if args.shape_circuits_n8:
        have = [circuit_file.load(p) for p in circuit_file.find_aggregate_circuits(8, K, ELL, LOGB, 6, 13, 3)]
        circuits = (have + [have[-1]] * levels)[:levels]
    else:
        circuits = [circuit_file.load(p) for p in circuit_file.find_aggregate_circuits(N, K, ELL, LOGB, n_lwe, log_n, levels)]
    rng = np.random.default_rng(1)
    f = lambda *shape: rng.integers(0, api.P, size=shape, dtype=np.uint64)
    vks = f(levels + 1, 68)
    ctx = vpbs_amd.Context(0, log_n_max=16)
    av = api.AggregateVerifier(ctx, api.AggregateShape(N, K, n_lwe, vks, circuits), max_leaves=max(trees) * max(sizes), max_aggregates=max(trees))
    spread = lambda ms: {"median": sorted(ms)[len(ms) // 2], "min": min(ms), "max": max(ms)}
    rows = []
    with ThreadPoolExecutor(max_workers=16) as pool:
        for L in sizes:
            for T in trees:
                total = T * L
                st = (f(4, N), f(total, n_lwe + 1), f(total, K * N), f(8, 4), rng.integers(0, 8, size=total), rng.integers(0, 4, size=total))
                one = lambda a: (st[0], st[1][a * L:(a + 1) * L], st[2][a * L:(a + 1) * L], st[3], st[4][a * L:(a + 1) * L], st[5][a * L:(a + 1) * L])
                host_root = lambda a: api.aggregate_root(N, K, n_lwe, vks[0], *one(a))
                want = np.stack(list(pool.map(host_root, range(T))))
                roots, bad = av.roots_many([L] * T, *st)          # and the warm-up of all three legs
                assert not bad.any() and (roots == want).all() and all((av.root(*one(a)) == want[a]).all() for a in range(T))
                ms = {"many": [], "single": [], "host": []}
                for _ in range(args.runs):
                    t = time.perf_counter()
                    av.roots_many([L] * T, *st)
                    ms["many"].append(1e3 * (time.perf_counter() - t))
                    t = time.perf_counter()
                    for a in range(T):
                        av.root(*one(a))
                    ms["single"].append(1e3 * (time.perf_counter() - t))
                    t = time.perf_counter()
                    list(pool.map(host_root, range(T)))
                    ms["host"].append(1e3 * (time.perf_counter() - t))
                # the leaf kernel, by the library's HIP-event timers: `runs` runs with timing on
                ctx.timing_enable(1)
                pair = []
                for _ in range(args.runs):
                    ctx.timing_report()
                    av.roots_many([L] * T, *st)
                    pair.append(ctx.timing_report().get("ag_leaf_pair", {}).get("ms", 0.0))
                ctx.timing_enable(0)
                rows.append({"trees": T, "leaves_per_tree": L, "roots_many_ms": spread(ms["many"]), "single_runs_ms": spread(ms["single"]),
                             "host_16_threads_ms": spread(ms["host"]), "ag_leaf_pair_event_ms": spread(pair)})
    av.close()
    ctx.close()
    print(json.dumps({"what": "roots of T trees of L leaves: one many-run against T single device runs and against the host on up to 16 threads, "
                              "N=%d n=%d, %d public inputs per leaf" % (N, n_lwe, 2 * K * N + 77), "runs": args.runs, "rows": rows,
                      "shape_circuits_n8": bool(args.shape_circuits_n8),
                      "host": {"cpus": len(os.sched_getaffinity(0)), "loadavg": os.getloadavg()[0]}}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n8", action="store_true")
    ap.add_argument("--leaves", default="64,256,1024")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--many")
    ap.add_argument("--tree-leaves", default="8,64")
    ap.add_argument("--shape-circuits-n8", action="store_true")
    args = ap.parse_args()
    N, n_lwe, log_n = (8, 6, 13) if args.n8 else (1024, 728, 16)
    if args.many:
        return many(args, N, n_lwe, log_n)
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
