#!/usr/bin/env python3
"""A batch of verifiable bootstraps under one key set: seeded keys, M seeded ciphertexts, ONE api.PbsProver.prove (the outputs of all of
them from the Bootstrapper, then their IVC chains on C worker threads with the chains' public inputs produced once, on the device), then
ALL proofs through api.PbsVerifier built from the prover's key_hash() and all lwe_out decrypted (api.lwe_decrypt, rounded as the
reference's main.rs:59-64).  One JSON line.

usage: tools/prove_batch.py [--count M] [--chains C] [--witness-batch B] [--steps K] [--n2048 | --n8] [--keys-on-device] [--baseline]
                            [--keys M [--baseline]] [--checkpoint DIR:every] [--resume DIR] [--aggregate [--aggregate-device [MAX_NODES]]]
  --steps K < n + 2 proves a prefix of every chain (tests); the proofs are then checked by api.verify_pbs_prefix on the host (verify_pbs
    insists on counter = n + 2); the outputs are those of the whole bootstrap either way.
  --n8: the N = 8, n = 6 miniature (degree 2^13); --n2048: N = 2048 (degree 2^17); default: the paper's N = 1024, n = 728 (degree 2^16).
  --keys-on-device: the keys are generated into device memory and never exist on the host (not with --baseline, whose entry points want
    host arrays).
  --baseline: the same batch the way it was done before PbsProver existed, using only api of that time -- C threads, each with its own
    Context + Ivc.set_device_witness(ELL, LOGB, B) + Ivc.prove_pbs on host keys, outputs from each chain's proof -- so that this file can be
    copied into a build of an older commit and run there.
  --keys M: the batch spread over M seeded key sets (ciphertext i under key set i mod M) on ONE api.RingProver: all proofs are verified in
    one run of ONE api.RingVerifier whose slot k holds RingProver.key_hash(k), every output decrypted under its own key.  --keys M
    --baseline: the same with M api.PbsProver objects, one after the other, each proving the ciphertexts of its key set, and M
    api.PbsVerifier objects (it needs nothing newer than api.PbsProver, so this file can be copied into a build of an older commit).
    Both print one JSON line with the wall time (seconds), proofs, device_bytes_held_by_the_provers (hipMemGetInfo before the first
    create and after the last), seconds_until_out_ct_complete and prepare_chain_ms.
  --checkpoint DIR:every: every `every` steps of every chain its proof so far goes to DIR/ct<i>_step<k>.bin (on_checkpoint; written under a
    temporary name and renamed, so a crash never leaves a torn file).  --resume DIR: every ciphertext that has a file there goes on from
    its highest-numbered one (PbsProver.resume / RingProver.resume); the JSON line reports resumed_from per row (0: from step 0) and, for
    a checkpoint the prover refused, its message under checkpoints_refused.  Both work with --keys M; neither with --baseline.  Every
    line carries proofs_sha256, so that a resumed run can be compared with an uninterrupted one.
  --aggregate: after the proofs and their verification, ONE api.Aggregator folds all proofs into one proof (the level circuits are located
    as data: tools/export_circuits.py --aggregate N K ELL LOGB n_lwe log_n levels makes them), which api.verify_aggregate (host) and
    api.AggregateVerifier (device) check against the statement of the whole batch; the JSON line gains "aggregate": bytes, depth, nodes and
    the times.  With --keys M too; not with --steps or --baseline, and only when every proof exists.
    --aggregate-device [MAX_NODES] (default 32): the aggregator's device witness -- the node witnesses of a tree level in
    device batches of at most MAX_NODES; the same bytes.  "aggregate" shows the aggregator's "device_stats" beside its "last_run" either way."""
import hashlib
import argparse
import json
import os
import resource
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (the HIP runtime the library shares with it)

import vpbs_amd  # noqa: E402
from vpbs_amd import api, circuit_file  # noqa: E402

K, ELL, LOGB = 2, 4, 5
P = api.P
SIGMA_GLWE, SIGMA_LWE = 4.99027217501041e-8, 1.17021618159313e-5
SEED = 0x5EED0728


def rounded(m, delta, p=2):
    """main.rs:59-64: round(m_bar / delta) mod 2 p"""
    return int(round(int(m) / delta)) % (2 * p)


def cpu_seconds():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def checkpoint_writer(directory):
    """on_checkpoint's fn for --checkpoint: directory/ct<i>_step<k>.bin, written under a temporary name and renamed into place"""
    os.makedirs(directory, exist_ok=True)
    written = []

    def write(index, done, blob):
        path = os.path.join(directory, "ct%d_step%d.bin" % (index, done))
        tmp = path + ".tmp.%d" % os.getpid()
        with open(tmp, "wb") as f:
            f.write(blob)
        os.replace(tmp, path)
        written.append(path)
    return write, written


def checkpoints_of(directory, count):
    """--resume: the highest-numbered ct<i>_step<k>.bin of every ciphertext -> (list of bytes or None, list of k or 0)"""
    best = {}
    for name in os.listdir(directory):
        if name.startswith("ct") and name.endswith(".bin") and "_step" in name:
            i, k = name[2:-4].split("_step")
            if i.isdigit() and k.isdigit() and int(i) < count and int(k) > best.get(int(i), (0, ""))[0]:
                best[int(i)] = (int(k), os.path.join(directory, name))
    blobs = [open(best[i][1], "rb").read() if i in best else None for i in range(count)]
    return blobs, [best[i][0] if i in best else 0 for i in range(count)]


def run_prover(args, prover, prove, resume):
    """prove(...) or, with --resume, resume(checkpoints, ...) under --checkpoint's writer -> (proofs, out_ct, lwe_out, resume figures)"""
    written = None
    if args.checkpoint:
        directory, every = args.checkpoint.rsplit(":", 1)
        write, written = checkpoint_writer(directory)
        prover.on_checkpoint(int(every), write)
    if args.resume:
        blobs, ks = checkpoints_of(args.resume, args.count)
        proofs, out_ct, lwe_out, errors = resume(blobs)
        refused = {i: e for i, e in enumerate(errors) if e is not None}
        figures = {"resumed_from": [0 if i in refused else k for i, k in enumerate(ks)], "checkpoints_refused": refused}
    else:
        proofs, out_ct, lwe_out = prove()
        figures = {"resumed_from": [0] * args.count, "checkpoints_refused": {}}
    figures["checkpoints_written"] = len(written) if written is not None else None
    return proofs, out_ct, lwe_out, figures


def proof_hashes(proofs):
    return [hashlib.sha256(b).hexdigest() if b is not None else None for b in proofs]


def prove_new(args, N, n_lwe, cyc, dum, ctx, keys, cts, testv):
    """-> (proofs, out_ct, lwe_out, key_hash, verifier data, seconds, seconds until out_ct was complete, extra); called inside the CPU clock"""
    t_make = time.perf_counter()
    if args.keys_on_device:
        prover = api.PbsProver(0, cyc, dum, keys["d_bsk"], keys["d_ksk"], K, ELL, LOGB, chains=args.chains, witness_batch=args.witness_batch,
                               keys_on_device=True, N=N, n_lwe=n_lwe)
    else:
        prover = api.PbsProver(0, cyc, dum, keys["bsk"], keys["ksk"], K, ELL, LOGB, chains=args.chains, witness_batch=args.witness_batch)
    t_make = time.perf_counter() - t_make
    first = []
    t0, c0 = time.perf_counter(), cpu_seconds()
    on_proof = lambda i, b: first.append(time.perf_counter() - t0)
    proofs, out_ct, lwe_out, figures = run_prover(args, prover, lambda: prover.prove(cts, testv, steps=args.steps, on_proof=on_proof),
                                                  lambda blobs: prover.resume(cts, testv, blobs, steps=args.steps, on_proof=on_proof))
    seconds, cpu = time.perf_counter() - t0, cpu_seconds() - c0
    kh, (vk, _) = prover.key_hash(), prover.verifier_data()
    run = prover.last_run()   # the library's own clock: when out_ct / lwe_out were complete, the chains' vpbs_ivc_timing
    prover.close()
    return proofs, out_ct, lwe_out, kh, vk, seconds, run["outputs_seconds"], {
        "cpu_seconds_proving": cpu, "prover_create_s": t_make, "first_proof_after_s": min(first) if first else None, "prepare_chain_ms": run["prepare_chain_ms"],
        "chain_timing_mean": run["chain"], "early_witness_ms_per_step": run["chain"]["early_witness_ms"], **figures}


def prove_baseline(args, N, n_lwe, log_n, cyc_path, dum_path, keys, cts, testv):
    """the parent's way: C threads, each with a Context and an Ivc of its own on HOST keys; a chain's output is its proof's accumulator"""
    kn = K * N
    todo, lock = list(range(len(cts))), threading.Lock()
    proofs, out_ct, done_at, errors, timings = [None] * len(cts), np.zeros((len(cts), K, N), np.uint64), [0.0] * len(cts), [], []
    chains = []
    for _ in range(args.chains):
        c = vpbs_amd.Context(0, log_n_max=max(16, log_n))
        if args.chains > 1 and "VPBS_WIDE_THRESHOLD" not in os.environ:
            c.set_option("wide_threshold", 2048)
        ivc = api.Ivc(c, circuit_file.load(cyc_path), circuit_file.load(dum_path), N, K, K * ELL * K * N)
        if args.witness_batch:
            ivc.set_device_witness(ELL, LOGB, args.witness_batch)
        chains.append((c, ivc))
    start = threading.Barrier(args.chains + 1)

    def work(ci):
        c, ivc = chains[ci]
        try:
            start.wait()
            while True:
                with lock:
                    if not todo:
                        return
                    i = todo.pop(0)
                blob, t = ivc.prove_pbs(testv, cts[i], keys["bsk"], keys["ksk"], args.steps)
                timings.append(t)
                proofs[i] = blob
                done_at[i] = time.perf_counter()
        except BaseException as e:   # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(ci,)) for ci in range(args.chains)]
    for th in threads:
        th.start()
    start.wait()
    t0, c0 = time.perf_counter(), cpu_seconds()
    for th in threads:
        th.join()
    seconds, cpu = time.perf_counter() - t0, cpu_seconds() - c0
    if errors:
        raise errors[0]
    vk, _ = chains[0][1].verifier_data()
    cyc = circuit_file.load(cyc_path)
    ncols = [cyc.n_constants + 80, 135, 20, 16]
    whole = args.steps in (0, n_lwe + 2)
    for i, blob in enumerate(proofs):   # the only place the parent's batch gets its outputs from: the last proof's accumulator
        if whole:
            out_ct[i] = api.step_proof_from_bytes(blob, ncols, log_n, cyc.n_constants)[1][kn + 1:2 * kn + 1].reshape(K, N)
    lwe_out = chains[0][0].lwe_extract(out_ct, n_lwe) if whole else None
    t_key = time.perf_counter()
    kh = api.pbs_key_hash(keys["bsk"], keys["ksk"])
    t_key = time.perf_counter() - t_key
    for c, ivc in chains:
        ivc.free()
        c.close()
    mean = {f: sum(t[f] for t in timings) / len(timings) for f in timings[0]}
    return proofs, out_ct, lwe_out, kh, vk, seconds, max(done_at) - t0, {"cpu_seconds_proving": cpu, "key_hash_on_the_host_s": t_key, "chain_timing_mean": mean,
                                                                        "early_witness_ms_per_step": mean["early_witness_ms"]}


def aggregate_section(ctx, N, n_lwe, log_n, cyc, vk, proofs, testv, cts, out_ct, key_hashes, key_of, leaves_seconds, device_nodes=None):
    """--aggregate: fold `proofs` into one proof and verify it on the host and on the device -> the "aggregate" entry of the JSON line;
    device_nodes (--aggregate-device): the node witnesses of a level in device batches of at most that many (Aggregator.set_device_witness)"""
    count = len(proofs)
    depth = api.aggregate_depth(count)
    levels = [circuit_file.load(p) for p in circuit_file.find_aggregate_circuits(N, K, ELL, LOGB, n_lwe, log_n, depth)]
    t = time.perf_counter()
    agg = api.Aggregator(ctx, cyc, vk, levels)
    if device_nodes:
        agg.set_device_witness(device_nodes)
    t_create = time.perf_counter() - t
    t = time.perf_counter()
    blob = agg.aggregate(proofs)
    t_run = time.perf_counter() - t
    run, vks, device_stats = agg.last_run(), agg.verifier_data(), agg.device_stats()
    agg.close()
    shape = api.AggregateShape(N, K, n_lwe, vks, levels)
    statement = (np.asarray(testv, np.uint64).reshape(1, N), cts, np.asarray(out_ct, np.uint64).reshape(count, K * N), np.stack(key_hashes), key_of)
    t = time.perf_counter()
    host = api.verify_aggregate(shape, blob, count, *statement)
    t_host = time.perf_counter() - t
    av = api.AggregateVerifier(ctx, shape, max_leaves=count)
    device = av.verify(blob, count, *statement)     # the first run pays for the staging buffers
    t = time.perf_counter()
    device = av.verify(blob, count, *statement)
    t_device = time.perf_counter() - t
    av.close()
    leaf_bytes = sum(len(b) for b in proofs)
    return {"count": count, "depth": depth, "nodes": run["nodes"], "last_run": run, "device_stats": device_stats,
            "level_degree_bits": [d.log_n for d in levels], "bytes": len(blob),
            "leaf_bytes_total": leaf_bytes, "bytes_ratio": len(blob) / leaf_bytes, "sha256": hashlib.sha256(blob).hexdigest(),
            "create_seconds": t_create, "aggregate_seconds": t_run, "check_leaves_ms_16_host_threads": run["check_leaves_ms"],
            "node_witness_ms": run["witness_ms"] / max(run["nodes"], 1), "node_prove_ms": run["prove_ms"] / max(run["nodes"], 1),
            "aggregate_seconds_over_leaves_seconds": t_run / leaves_seconds if leaves_seconds else None,
            "verify_host_ms": 1e3 * t_host, "verify_device_ms": 1e3 * t_device, "host": [bool(host[0]), api.aggregate_reason_text(host[1])],
            "device": [bool(device[0]), api.aggregate_reason_text(device[1])], "accepted": bool(host[0] and device[0])}


def device_bytes_free():
    free, _ = torch.cuda.mem_get_info(0)   # hipMemGetInfo
    return int(free)


def main_keys(args, N, n_lwe, log_n):
    """--keys M [--baseline]: see the module text"""
    M, count = args.keys, args.count
    cyc_path, dum_path = circuit_file.find_cyclic_circuit(N, K, ELL, LOGB, n_lwe, log_n)
    cyc, dum = circuit_file.load(cyc_path), circuit_file.load(dum_path)
    ctx = vpbs_amd.Context(0, log_n_max=max(16, log_n))
    keys = [ctx.keygen(N, K, ELL, LOGB, n_lwe, SEED + k, SIGMA_GLWE, SIGMA_LWE) for k in range(M)]
    testv, delta = api.testv(N, 2)
    key_of = [i % M for i in range(count)]
    msgs = [(3 * i + i // 2) % 2 for i in range(count)]
    cts = np.stack([api.lwe_encrypt(keys[k]["params"], keys[k]["s_lwe"], delta * m % P, nonce=i) for i, (m, k) in enumerate(zip(msgs, key_of))])
    mine = [[i for i in range(count) if key_of[i] == k] for k in range(M)]
    proofs, out_ct, lwe_out = [None] * count, np.zeros((count, K, N), np.uint64), np.zeros((count, n_lwe + 1), np.uint64)
    figures = {}
    ctx.synchronize()
    load0, free0 = os.getloadavg()[0], device_bytes_free()
    t0 = time.perf_counter()
    if args.baseline:
        provers = [api.PbsProver(0, cyc, dum, keys[k]["bsk"], keys[k]["ksk"], K, ELL, LOGB, chains=args.chains, witness_batch=args.witness_batch)
                   for k in range(M)]
        held, t_made = free0 - device_bytes_free(), time.perf_counter()
        t_out, prepare, n_proofs = 0.0, [], 0
        for k, p in enumerate(provers):           # one after the other: the outputs of the last key set wait for the proofs of all before
            if not mine[k]:
                continue
            t_k = time.perf_counter()
            got, o, l = p.prove(cts[mine[k]], testv, steps=args.steps)
            run = p.last_run()
            for j, i in enumerate(mine[k]):
                proofs[i], out_ct[i], lwe_out[i] = got[j], o[j], l[j]
            t_out = t_k - t_made + run["outputs_seconds"]
            prepare.append(run["prepare_chain_ms"] * run["proofs"])
            n_proofs += run["proofs"]
        hashes, vk = [p.key_hash() for p in provers], provers[0].verifier_data()[0]
        for p in provers:
            p.close()
        prepare_ms = sum(prepare) / max(n_proofs, 1)
    else:
        rp = api.RingProver(0, cyc, dum, K, ELL, LOGB, N, n_lwe, max_keys=M, chains=args.chains, witness_batch=args.witness_batch)
        for k in range(M):
            assert rp.add(keys[k]["bsk"], keys[k]["ksk"]) == k
        held, t_made = free0 - device_bytes_free(), time.perf_counter()
        proofs, out_ct, lwe_out, figures = run_prover(args, rp, lambda: rp.prove(cts, key_of, testv, steps=args.steps),
                                                      lambda blobs: rp.resume(cts, key_of, testv, blobs, steps=args.steps))
        run = rp.last_run()
        t_out, prepare_ms, n_proofs = run["outputs_seconds"], run["prepare_chain_ms"], run["proofs"]
        hashes, vk = [rp.key_hash(k) for k in range(M)], rp.verifier_data()[0]
        rp.close()
    t_end = time.perf_counter()
    # ---- after the clock: every proof under the key hash of its own slot, every output under its own key ----
    total = n_lwe + 2
    whole = args.steps in (0, total)
    ncols, cap = [cyc.n_constants + 80, 135, 20, 16], vk[4:].reshape(-1, 4)
    accepted, why = 0, set()
    live = [i for i in range(count) if proofs[i] is not None]   # a refused checkpoint leaves no proof: not accepted, the exit status is 1
    mine = [[i for i in m if proofs[i] is not None] for m in mine]
    if whole and not args.baseline and live:   # ONE RingVerifier for all key sets: slot k holds the key hash of the prover's slot k
        rv = api.RingVerifier(ctx, cap, ncols, vk[:4], log_n, cyc.n_constants, 80, cyc.gates, N, K, n_lwe, K * ELL * K * N, max_keys=M, max_batch=count)
        for k in range(M):
            rv.set_key(k, hashes[k])
        t_rv = time.perf_counter()
        verdicts, reasons, _ = rv.verify([proofs[i] for i in live], [key_of[i] for i in live], testv, cts[live], out_ct[live])
        figures["ring_verifier_ms"] = 1e3 * (time.perf_counter() - t_rv)
        rv.close()
        accepted = int(verdicts.sum())
        why = {api.pbs_reason_text(int(r)) for v, r in zip(verdicts, reasons) if not v}
    for k in range(M if args.baseline or not whole else 0):
        if not mine[k]:
            continue
        sel = [proofs[i] for i in mine[k]]
        if whole:
            pv = api.PbsVerifier(ctx, cap, ncols, vk[:4], log_n, cyc.n_constants, 80, cyc.gates, N, K, n_lwe, K * ELL * K * N, hashes[k], max_batch=len(sel))
            verdicts, reasons, _ = pv.verify(sel, testv, cts[mine[k]], out_ct[mine[k]].reshape(len(sel), -1))
            pv.close()
            accepted += int(verdicts.sum())
            why |= {api.pbs_reason_text(int(r)) for v, r in zip(verdicts, reasons) if not v}
        else:
            res = [api.verify_pbs_prefix(b, cap, ncols, vk[:4], log_n, cyc.n_constants, 80, cyc.gates, N, K, testv, cts[i], keys[k]["bsk"], keys[k]["ksk"])
                   for i, b in zip(mine[k], sel)]
            accepted += sum(1 for r in res if r[0] and r[1] == args.steps)
            why |= {str(r[-1]) for r in res if not r[0]}
    decrypted = sum(1 for i in range(count) if rounded(api.lwe_decrypt(keys[key_of[i]]["s_lwe"], lwe_out[i]), delta) == msgs[i])
    aggregated = True
    if args.aggregate and len(live) == count:
        figures["aggregate"] = aggregate_section(ctx, N, n_lwe, log_n, cyc, vk, proofs, testv, cts, out_ct, hashes, key_of, t_end - t_made,
                                               args.aggregate_device)
        aggregated = figures["aggregate"]["accepted"]
    ctx.close()
    print(json.dumps(dict({
        "what": "%d verifiable bootstraps under %d key sets at N=%d, n=%d (degree 2^%d), %s" % (
            count, M, N, n_lwe, log_n, "one PbsProver per key set, one after the other" if args.baseline else "one RingProver.prove"),
        "count": count, "keys": M, "chains": args.chains, "witness_batch": args.witness_batch, "steps": args.steps or total, "baseline": args.baseline,
        "seconds": t_end - t_made, "seconds_with_create_and_close": t_end - t0, "create_seconds": t_made - t0, "proofs": n_proofs,
        "seconds_per_proof": (t_end - t_made) / max(n_proofs, 1), "device_bytes_held_by_the_provers": held,
        "seconds_until_out_ct_complete": t_out, "prepare_chain_ms": prepare_ms, "accepted": accepted, "rejected_because": sorted(why),
        "decrypted_correct": decrypted, "proofs_sha256": proof_hashes(proofs),
        "host": {"cpus": len(os.sched_getaffinity(0)), "loadavg_before": load0, "loadavg_after": os.getloadavg()[0]}}, **figures)))
    return 0 if accepted == count and decrypted == count and n_proofs == count and aggregated else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=16)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--witness-batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--n2048", action="store_true")
    ap.add_argument("--n8", action="store_true")
    ap.add_argument("--keys-on-device", action="store_true")
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--keys", type=int, default=0)
    ap.add_argument("--checkpoint", default="", metavar="DIR:every")
    ap.add_argument("--resume", default="", metavar="DIR")
    ap.add_argument("--aggregate", action="store_true")
    ap.add_argument("--aggregate-device", type=int, nargs="?", const=32, default=None, metavar="MAX_NODES")
    args = ap.parse_args()
    if args.aggregate_device is not None and (not args.aggregate or args.aggregate_device < 1):
        raise SystemExit("--aggregate-device [max_nodes] (at least 1; default 32) is a switch of --aggregate")
    if args.aggregate and (args.baseline or args.steps):
        raise SystemExit("--aggregate folds whole vPBS proofs of the batch provers: it cannot run with --baseline or --steps")
    if args.baseline and (args.checkpoint or args.resume):
        raise SystemExit("--checkpoint and --resume belong to the batch provers: they cannot run with --baseline")
    if args.checkpoint and not args.checkpoint.rsplit(":", 1)[-1].isdigit():
        raise SystemExit("--checkpoint wants DIR:every")
    if args.baseline and args.keys_on_device:
        raise SystemExit("--baseline proves under host keys: it cannot run with --keys-on-device")
    N, n_lwe, log_n = (8, 6, 13) if args.n8 else ((2048, 728, 17) if args.n2048 else (1024, 728, 16))
    total = n_lwe + 2
    if args.steps < 0 or args.steps > total:
        raise SystemExit("--steps must be 0 .. %d" % total)
    whole = args.steps in (0, total)
    api.host_set_late_threads(api.late_threads_for(args.chains, api.host_cpu_budget()))
    api.host_set_early_threads(api.early_threads_for(args.chains))
    if args.keys:
        if args.keys < 0 or args.keys_on_device:
            raise SystemExit("--keys M proves under M >= 1 host key sets: it cannot run with --keys-on-device")
        return main_keys(args, N, n_lwe, log_n)
    cyc_path, dum_path = circuit_file.find_cyclic_circuit(N, K, ELL, LOGB, n_lwe, log_n)
    cyc, dum = circuit_file.load(cyc_path), circuit_file.load(dum_path)
    ctx = vpbs_amd.Context(0, log_n_max=max(16, log_n))
    keygen = ctx.keygen_device if args.keys_on_device else ctx.keygen
    keys = keygen(N, K, ELL, LOGB, n_lwe, SEED, SIGMA_GLWE, SIGMA_LWE)
    testv, delta = api.testv(N, 2)
    msgs = [(3 * i + i // 2) % 2 for i in range(args.count)]
    cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * m % P, nonce=i) for i, m in enumerate(msgs)])
    load0, cpu0 = os.getloadavg()[0], cpu_seconds()
    if args.baseline:
        proofs, out_ct, lwe_out, kh, vk, seconds, t_out, extra = prove_baseline(args, N, n_lwe, log_n, cyc_path, dum_path, keys, cts, testv)
    else:
        proofs, out_ct, lwe_out, kh, vk, seconds, t_out, extra = prove_new(args, N, n_lwe, cyc, dum, ctx, keys, cts, testv)
    cpu = cpu_seconds() - cpu0
    # ---- after the clock: every proof verified, every output decrypted ----
    ncols = [cyc.n_constants + 80, 135, 20, 16]
    cap = vk[4:].reshape(-1, 4)
    t = time.perf_counter()
    live = [i for i, b in enumerate(proofs) if b is not None]   # a refused checkpoint leaves no proof: not accepted, the exit status is 1
    if whole and live:
        pv = api.PbsVerifier(ctx, cap, ncols, vk[:4], log_n, cyc.n_constants, 80, cyc.gates, N, K, n_lwe, K * ELL * K * N, kh,
                             max_batch=len(live))
        verdicts, reasons, _ = pv.verify([proofs[i] for i in live], testv, cts[live], out_ct[live].reshape(len(live), -1))
        pv.close()
        accepted = int(verdicts.sum())
        why = sorted({api.pbs_reason_text(int(r)) for v, r in zip(verdicts, reasons) if not v})
    elif whole:
        accepted, why = 0, []
    else:   # prefixes: the host's prefix form, which wants host keys
        hk = keys if not args.keys_on_device else ctx.keygen(N, K, ELL, LOGB, n_lwe, SEED, SIGMA_GLWE, SIGMA_LWE)
        res = [api.verify_pbs_prefix(proofs[i], cap, ncols, vk[:4], log_n, cyc.n_constants, 80, cyc.gates, N, K, testv, cts[i], hk["bsk"], hk["ksk"])
               for i in live]
        accepted = sum(1 for r in res if r[0] and r[1] == args.steps)
        why = sorted({str(r[-1]) for r in res if not r[0]})
    t_verify = time.perf_counter() - t
    decrypted = None
    if lwe_out is not None:
        decrypted = sum(1 for m, want in zip(api.lwe_decrypt(keys["s_lwe"], lwe_out), msgs) if rounded(m, delta) == want)
    aggregated = True
    if args.aggregate and len(live) == args.count:
        extra["aggregate"] = aggregate_section(ctx, N, n_lwe, log_n, cyc, vk, proofs, testv, cts, out_ct, [kh], None, seconds, args.aggregate_device)
        aggregated = extra["aggregate"]["accepted"]
    if args.keys_on_device:
        ctx.device_free(keys["d_bsk"])
        ctx.device_free(keys["d_ksk"])
    ctx.close()
    print(json.dumps(dict({
        "what": "%d verifiable bootstraps under one key set at N=%d, n=%d (degree 2^%d), %s" % (
            args.count, N, n_lwe, log_n, "the parent's way: one Ivc per thread on host keys" if args.baseline else "one PbsProver.prove"),
        "count": args.count, "chains": args.chains, "witness_batch": args.witness_batch, "steps": args.steps or total,
        "keys_on_device": args.keys_on_device, "baseline": args.baseline, "seconds": seconds,
        "proofs_per_s": args.count / seconds if whole else None, "ms_per_step": 1e3 * seconds * args.chains / (args.count * (args.steps or total)),
        "seconds_until_out_ct_complete": t_out, "accepted": accepted, "rejected_because": why, "decrypted_correct": decrypted,
        "cpu_seconds_setup_and_proving": cpu, "cpu_seconds_per_proof": extra["cpu_seconds_proving"] / args.count, "verify_s": t_verify,
        "proofs_sha256": proof_hashes(proofs),
        "host": {"cpus": len(os.sched_getaffinity(0)), "loadavg_before": load0, "loadavg_after": os.getloadavg()[0]}}, **extra)))
    return 0 if accepted == args.count and (decrypted in (None, args.count)) and aggregated else 1


if __name__ == "__main__":
    sys.exit(main())
