#!/usr/bin/env python3
"""The aggregator's host path against its device witness: the same leaves folded by api.Aggregator with the node witnesses
on the host (the default) and in device batches (Aggregator.set_device_witness).  One JSON line.

usage: tools/aggregate_speed.py [--n8] [--leaves 8] [--replicate 64] [--trees 8] [--runs 5] [--device-nodes 32] [--legs host,device]
                                [--leaves-file FILE.npz] [--chains C] [--witness-batch W] [--out FILE.json]
  The leaves are `--leaves` vPBS proofs under one key set, proven once (a RingProver; seeded keys and inputs) and kept in memory; with
  --leaves-file they are saved there, and a later process -- of this build or of another one -- loads them instead of proving again.
  Timed, each after a warm-up, --runs times: `aggregate` of the leaves; `aggregate` of the leaves replicated to --replicate (the aggregator
  dedups by position, not by content, so these are --replicate - 1 distinct nodes); --trees trees of the leaves each.  For every case: median
  and range of the wall time, the process's CPU seconds (os.times: user + system, all threads) per run, Aggregator.last_run and -- on the
  device leg -- Aggregator.device_stats of the last run.
  The HOST leg uses only api.Aggregator, Aggregator.aggregate and Aggregator.last_run (the trees are a loop over aggregate), so this file
  runs unchanged on a build without the device witness: there `--legs host` is the only leg, and the line says so.  The device leg takes the
  trees as ONE Aggregator.aggregate_many.  Every device-leg aggregate is compared with the host leg's, byte for byte, when both legs run.
  The level circuits are located as data (tools/export_circuits.py --aggregate N K ELL LOGB n_lwe log_n levels makes them)."""
import argparse
import hashlib
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
SEED, SIGMA_GLWE, SIGMA_LWE = 7, 4.99027217501041e-8, 1.17021618159313e-5


def cpu_seconds():
    t = os.times()
    return t.user + t.system


def make_leaves(args, ctx, cyc, dum, N, n_lwe):
    """-> (proofs, vk0): from --leaves-file when it exists, else proven here (and saved there)"""
    if args.leaves_file and os.path.exists(args.leaves_file):
        z = np.load(args.leaves_file)
        proofs = [z["bytes"][z["offsets"][i]:z["offsets"][i + 1]].tobytes() for i in range(z["offsets"].size - 1)]
        if len(proofs) != args.leaves:
            raise SystemExit("%s holds %d leaves, not --leaves %d" % (args.leaves_file, len(proofs), args.leaves))
        return proofs, z["vk0"], 0.0
    key = ctx.keygen(N, K, ELL, LOGB, n_lwe, SEED, SIGMA_GLWE, SIGMA_LWE)
    testv, delta = api.testv(N, 2)
    cts = np.stack([api.lwe_encrypt(key["params"], key["s_lwe"], delta * (i % 2) % api.P, nonce=i) for i in range(args.leaves)])
    rp = api.RingProver(0, cyc, dum, K, ELL, LOGB, N, n_lwe, max_keys=1, chains=args.chains or (2 if args.n8 else 8),
                        witness_batch=args.witness_batch or (3 if args.n8 else 64))
    assert rp.add(key["bsk"], key["ksk"]) == 0
    t = time.perf_counter()
    proofs, _, _ = rp.prove(cts, [0] * args.leaves, testv)
    seconds = time.perf_counter() - t
    vk0 = rp.verifier_data()[0]
    rp.close()
    if args.leaves_file:
        buf, offs = api.pack_proofs(proofs)
        np.savez(args.leaves_file, bytes=buf, offsets=offs, vk0=vk0)
    return proofs, vk0, seconds


def timed(agg, run, runs, device):
    """warm-up, then `runs` runs of run() -> (its last result, the figures)"""
    out = run()
    wall, cpu = [], []
    for _ in range(runs):
        c, t = cpu_seconds(), time.perf_counter()
        out = run()
        wall.append(time.perf_counter() - t)
        cpu.append(cpu_seconds() - c)
    fig = {"wall_seconds": {"median": sorted(wall)[len(wall) // 2], "min": min(wall), "max": max(wall)},
           "cpu_seconds": {"median": sorted(cpu)[len(cpu) // 2], "min": min(cpu), "max": max(cpu)}, "last_run": agg.last_run()}
    if device:
        fig["device_stats"] = agg.device_stats()
    return out, fig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n8", action="store_true")
    ap.add_argument("--leaves", type=int, default=8)
    ap.add_argument("--replicate", type=int, default=64)
    ap.add_argument("--trees", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device-nodes", type=int, default=32)
    ap.add_argument("--legs", default="host,device")
    ap.add_argument("--leaves-file")
    ap.add_argument("--chains", type=int, default=0)
    ap.add_argument("--witness-batch", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()
    N, n_lwe, log_n = (8, 6, 13) if args.n8 else (1024, 728, 16)
    has_device = hasattr(api.Aggregator, "set_device_witness")
    legs = [leg for leg in args.legs.split(",") if leg == "host" or (leg == "device" and has_device)]
    depth = api.aggregate_depth(max(args.leaves, args.replicate))
    cyc_path, dum_path = circuit_file.find_cyclic_circuit(N, K, ELL, LOGB, n_lwe, log_n)
    cyc, dum = circuit_file.load(cyc_path), circuit_file.load(dum_path)
    levels = [circuit_file.load(p) for p in circuit_file.find_aggregate_circuits(N, K, ELL, LOGB, n_lwe, log_n, depth)]
    ctx = vpbs_amd.Context(0, log_n_max=max(16, log_n))
    leaves, vk0, leaves_seconds = make_leaves(args, ctx, cyc, dum, N, n_lwe)
    many = (leaves * ((args.replicate + len(leaves) - 1) // len(leaves)))[:args.replicate]
    forest = [leaves] * args.trees
    t = time.perf_counter()
    agg = api.Aggregator(ctx, cyc, vk0, levels)
    create_seconds = time.perf_counter() - t
    sha = lambda blobs: hashlib.sha256(b"".join(blobs)).hexdigest()
    cases = (("aggregate_%d" % len(leaves), lambda: [agg.aggregate(leaves)]), ("aggregate_%d" % len(many), lambda: [agg.aggregate(many)]),
             ("trees_%dx%d" % (args.trees, len(leaves)), None))
    out = {"what": "api.Aggregator on %d vPBS proofs at N=%d, n=%d (degree 2^%d): node witnesses on the host against device batches" %
                   (len(leaves), N, n_lwe, log_n), "runs": args.runs, "legs": legs, "build_has_device_witness": has_device,
           "leaves_seconds": leaves_seconds, "create_seconds": create_seconds, "level_degree_bits": [d.log_n for d in levels], "cases": {}}
    for leg in legs:
        device = leg == "device"
        if device:
            t = time.perf_counter()
            agg.set_device_witness(args.device_nodes)
            out["set_device_witness_seconds"], out["device_nodes"] = time.perf_counter() - t, args.device_nodes
        for name, run in cases:
            if run is None:
                run = (lambda: agg.aggregate_many(forest)) if device else (lambda: [agg.aggregate(tree) for tree in forest])
            blobs, fig = timed(agg, run, args.runs, device)
            fig["sha256"] = sha(blobs)
            out["cases"].setdefault(name, {})[leg] = fig
    for name, by_leg in out["cases"].items():
        if len(by_leg) == 2:
            by_leg["bytes_equal"] = by_leg["host"]["sha256"] == by_leg["device"]["sha256"]
    agg.close()
    ctx.close()
    out["host"] = {"cpus": len(os.sched_getaffinity(0)), "loadavg": os.getloadavg()[0]}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if all(v.get("bytes_equal", True) for v in out["cases"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
