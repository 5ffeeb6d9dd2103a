#!/usr/bin/env python3
"""A program of lookup gates on one resident key set: seeded keys, seeded input ciphertexts, a seeded layered random netlist (or a program
file), evaluated twice -- by ONE api.Program.run (the resident leg: gate inputs formed on the device, one wait at the end) and the way a
user had to before api.Program existed (the baseline leg: Bootstrapper.run per level, combinations formed on the host with numpy) -- and
compared wire by wire.  One JSON line.

usage: tools/run_program.py [--levels L] [--width W] [--fan-in F] [--program FILE.json] [--n8] [--prove] [--baseline] [--runs R] [--seed S]
                            [--instances B --keys M [--verify-per-instance]] [--multi THETA [--margins]] [--aggregate [--aggregate-device [MAX_NODES]]]
  --aggregate (with --prove, alone or with --instances B --keys M): ONE proof per program instance.  The gate proofs of
    every instance are folded by an api.Aggregator (api.Program.prove_aggregate / prove_aggregate_batch; the level circuits are located as
    data: tools/export_circuits.py --aggregate N K ELL LOGB n_lwe log_n levels makes them, and the program may have at most 2^levels gates);
    every aggregate is verified on the host (api.program_verify_aggregate, the client's check) and all of them in one device run
    (api.Program.verify_aggregate_batch); the JSON line gains "aggregate": bytes, depth, both verdict lists and the bytes a client receives.
    --aggregate-device [MAX_NODES] (default 32): the aggregator's device witness -- with --instances, the level-l nodes of ALL
    instances in the same device batches of at most MAX_NODES, in ONE run of the aggregator; the same bytes.  "aggregate" shows the aggregator's
    "device_stats" beside its "last_run" either way.
  --multi THETA: multi-output lookup gates.  W inputs, L layers of W lookups of 2^THETA tables over {0, 1} each; a later
    lookup reads every output of the one before it.  The multi leg makes ONE gate of each lookup (api.Program 5-tuples, api.lut_testv_multi);
    the single leg makes one gate per table of the same functions on the same inputs -- a plain program that runs unchanged on a build
    without multi-output gates.  Every wire of the multi leg is compared with the composition snap -> Bootstrapper.run -> extract_at in
    numpy; every output of both legs is decrypted under its key (api lwe_decode_batch) against the tables and the failures are reported,
    not judged: they are the price of the snap.  Prints gates, proofs and evaluation seconds of both legs, and with --prove the proving
    and verifying seconds and the total proof bytes.  Works alone (Program.run / prove / verify) and with --instances B --keys M
    (run_batch / prove_batch / verify_batch).  --margins (with --multi): api.Program.margins of each leg's gate inputs against the message
    every gate reads, per level -- count, failures, the deviation in positions and NoiseStats.tail_log2 at N / (2p) - 2^THETA -- in
    "margins", beside the decryption failures.
  netlist: W inputs, L layers of W gates; a gate reads F wires of the layer before it with coefficients in {1, p - 1}; gate 0 of every layer
    is the identity of gate 0 of the layer before it (fan-in 1, coefficient 1), so that one output has a known message whatever F is.
  --program: {"n_inputs", "n_luts", "gates": [{"terms": [[src, coef], ..], "const", "lut"}, ..]} instead; lut 0 is the test vector of the
    identity on {0, 1}, lut 1 its negation, further luts are seeded random words.
  --n8: the N = 8, n = 6 miniature of tools/prove_batch.py --n8; default: the paper's N = 1024, n = 728.
  --prove (without --instances): api.Program.prove on an api.PbsProver, api.Program.verify on an api.PbsVerifier made from the prover's key_hash(), and the
    output wires with a known message decrypted.
  --baseline: the baseline leg ALONE.  It needs nothing newer than api.Bootstrapper, so this file can be copied into a build of an older
    commit and time that.
  --instances B --keys M: the same program for B input sets under M seeded key sets left on the device, instance b under key set b mod M.
    The batched leg is ONE api.Program.run_batch on an api.KeyRing (level l of all instances in launches of --max-batch rows); the baseline
    leg is api.Program.run per instance on the api.Bootstrapper of that instance's key set, which is all --baseline runs here -- it uses
    nothing newer than api.Program.run.  Every wire of both legs is compared; every program output (a wire of the last level) is decrypted
    under its own key, and those with a known message are checked.  Prints wall seconds, the HIP-event time of the bootstrap launches and
    the launches queued per leg, and the bytes of the combine and delivery kernels computed from the shapes.
    With --prove the batched leg is followed by ONE api.Program.prove_batch on an api.RingProver that holds the M key sets (host copies
    from the same seeds): its wires must be the batched leg's, ALL instances are verified by one api.Program.verify_batch on an
    api.RingVerifier whose slot k holds the ring prover's key_hash(k) (verify_seconds), and the decrypted outputs are the proven ones.
    --verify-per-instance: the proofs are checked a second time by api.Program.verify per instance on the api.PbsVerifier of its key set
    (verify_per_instance_seconds, verify_per_instance_equal).  With --runs R > 1 both forms are called R more times after that first call
    (verify_again, verify_per_instance_again: seconds per call, event time and launches of their combine kernel).
  Time: wall seconds per run of a leg (after one warm-up run), per level = / levels; HIP-event milliseconds of the bootstrap launches per
  level (the library's own timers).  Bytes: what each leg moves between host and device per run, computed from the shapes."""
import argparse
import hashlib
import json
import os
import statistics
import sys
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


def layered(rng, levels, width, fan_in):
    """-> (n_inputs, gates as (terms, const, lut)): see the module text"""
    gates = []
    for lv in range(levels):
        base = 0 if lv == 0 else width + (lv - 1) * width       # first wire of the layer before
        for g in range(width):
            if g == 0:
                gates.append(([(base, 1)], 0, 0))
                continue
            srcs = rng.integers(0, width, size=fan_in)
            coefs = rng.integers(0, 2, size=fan_in)
            gates.append(([(base + int(s), 1 if c else P - 1) for s, c in zip(srcs, coefs)], 0, 0))
    return width, gates


def load_program(path):
    d = json.load(open(path))
    return d["n_inputs"], [([(int(s), int(c)) for s, c in g["terms"]], int(g.get("const", 0)), int(g.get("lut", 0))) for g in d["gates"]], d.get("n_luts", 1)


def gate_levels(n_inputs, gates):
    lv = []
    for terms, _, _ in gates:
        lv.append(1 + max([0] + [lv[s - n_inputs] for s, _ in terms if s >= n_inputs]))
    return lv


def known_messages(n_inputs, gates, msgs):
    """the message of every wire that is an identity (one term, coefficient 1, no constant, lut 0) of a wire with a known message"""
    known = list(msgs)
    for terms, const, lut in gates:
        ok = len(terms) == 1 and terms[0][1] == 1 and const == 0 and lut == 0
        known.append(known[terms[0][0]] if ok else None)
    return known


def mulmod(a, c):
    """a [rows][words] uint64 (canonical) times the field element c, word by word: c is 1 or p - 1 in the seeded netlists (exact in numpy);
    anything else goes through Python integers"""
    if c == 1:
        return a
    if c == P - 1:
        return np.where(a == 0, a, np.uint64(P) - a)
    return np.array([[int(v) * c % P for v in row] for row in a], np.uint64)


def addmod(a, b):
    s = a + b                                   # wraps at 2^64
    wrapped = s < a
    s = np.where(wrapped, s + np.uint64(0xFFFFFFFF), s)      # 2^64 = 2^32 - 1 mod p; cannot wrap again: a, b < p
    return np.where(s >= np.uint64(P), s - np.uint64(P), s)


def run_baseline(ctx, bs, n_inputs, gates, lv, inputs, testvs):
    """Bootstrapper.run per level (in chunks of max_batch) on host combinations -> (wires, event ms of every level)"""
    n_levels = max([0] + lv)
    words = inputs.shape[1]
    wires = np.zeros((n_inputs + len(gates), words), np.uint64)
    wires[:n_inputs] = inputs % np.uint64(P)
    event_ms = []
    for level in range(1, n_levels + 1):
        todo = [g for g in range(len(gates)) if lv[g] == level]
        cts = np.zeros((len(todo), words), np.uint64)
        cts[:, words - 1] = np.array([gates[g][1] for g in todo], np.uint64)
        fan = max(len(gates[g][0]) for g in todo)
        for t in range(fan):                    # term t of every gate of the level at once
            rows = [k for k, g in enumerate(todo) if len(gates[g][0]) > t]
            for c in sorted({gates[todo[k]][0][t][1] for k in rows}):
                sel = [k for k in rows if gates[todo[k]][0][t][1] == c]
                cts[sel] = addmod(cts[sel], mulmod(wires[[gates[todo[k]][0][t][0] for k in sel]], c))
        tvs = testvs[[gates[g][2] for g in todo]]
        for lo in range(0, len(todo), bs.max_batch):
            _, lwe = bs.run(cts[lo:lo + bs.max_batch], tvs[lo:lo + bs.max_batch])
            wires[[n_inputs + g for g in todo[lo:lo + bs.max_batch]]] = lwe
        event_ms.append(ctx.timing_report().get("pbs_batch", {}).get("ms", 0.0))
    wires[:n_inputs] = inputs                   # as given
    return wires, event_ms


def aggregate_setup(ctx, prog, N, n_lwe, log_n, cyc, vk, max_aggregates, device_nodes=None):
    """--aggregate: the Aggregator over the level circuits the program's gate count needs (located as data: tools/export_circuits.py
    --aggregate makes them), the verifiers' shape and the device verifier -> (aggregator, shape, device verifier); device_nodes
    (--aggregate-device): its node witnesses in device batches of at most that many (Aggregator.set_device_witness)"""
    depth = api.aggregate_depth(max(prog.n_gates, 1))
    levels = [circuit_file.load(p) for p in circuit_file.find_aggregate_circuits(N, K, ELL, LOGB, n_lwe, log_n, depth)]
    agg = api.Aggregator(ctx, cyc, vk, levels)
    if device_nodes:
        agg.set_device_witness(device_nodes)
    shape = api.AggregateShape(N, K, n_lwe, agg.verifier_data(), levels)
    return agg, shape, api.AggregateVerifier(ctx, shape, max_leaves=max_aggregates * prog.n_gates, max_aggregates=max_aggregates)


def aggregate_report(prog, shape, av, blobs, inputs, key_of, hashes, testvs, out_cts, proof_bytes, seconds):
    """every instance's aggregate on the host (api.program_verify_aggregate, the client's check) and all of them in one device run
    (Program.verify_aggregate_batch) -> the "aggregate" entry of the JSON line; bytes a client receives either way"""
    t = time.perf_counter()
    host = [api.program_verify_aggregate(prog, shape, blobs[b], inputs[b], testvs, out_cts[b], hashes[key_of[b]]) for b in range(len(blobs))]
    t_host = time.perf_counter() - t
    t = time.perf_counter()
    verdicts, reasons = prog.verify_aggregate_batch(av, inputs, key_of, np.stack(hashes), testvs, out_cts, blobs)
    t_device = time.perf_counter() - t
    device = [(bool(v), int(r)) for v, r in zip(verdicts, reasons)]
    outputs = out_cts[0].nbytes
    return {"instances": len(blobs), "gates": prog.n_gates, "depth": api.aggregate_depth(prog.n_gates), "bytes": [len(b) for b in blobs],
            "prove_and_aggregate_seconds": seconds, "verify_host_ms": 1e3 * t_host, "verify_device_ms": 1e3 * t_device,
            "host": [[ok, api.aggregate_reason_text(r)] for ok, r in host], "device": [[ok, api.aggregate_reason_text(r)] for ok, r in device],
            "client_bytes_aggregate": len(blobs[0]) + outputs, "client_bytes_per_gate_proofs": proof_bytes + outputs,
            "accepted": bool(all(ok for ok, _ in host) and device == [(ok, r) for ok, r in host])}


def prove_batch(args, ctx, prog, N, n_lwe, log_n, M, inputs, key_of, testvs, batch_wires, out):
    """--instances B --keys M --prove: Program.prove_batch on a RingProver, Program.verify_batch on a RingVerifier -> (the proven wires, all
    accepted)"""
    cyc_path, dum_path = circuit_file.find_cyclic_circuit(N, K, ELL, LOGB, n_lwe, log_n)
    cyc, dum = circuit_file.load(cyc_path), circuit_file.load(dum_path)
    chains = args.chains or (2 if args.n8 else 8)
    api.host_set_late_threads(api.late_threads_for(chains, api.host_cpu_budget()))
    api.host_set_early_threads(api.early_threads_for(chains))
    rp = api.RingProver(0, cyc, dum, K, ELL, LOGB, N, n_lwe, max_keys=M, chains=chains, witness_batch=args.witness_batch or (3 if args.n8 else 64))
    for k in range(M):
        hk = ctx.keygen(N, K, ELL, LOGB, n_lwe, SEED + k, SIGMA_GLWE, SIGMA_LWE)
        assert rp.add(hk["bsk"], hk["ksk"]) == k
    t = time.perf_counter()
    proofs, wires, out_cts = prog.prove_batch(rp, inputs, key_of, testvs)
    out["prove_seconds"] = time.perf_counter() - t
    out["proofs_sha256"] = hashlib.sha256(b"".join(blob for row in proofs for blob in row)).hexdigest()   # to compare two builds on one seed
    hashes, (vk, _) = [rp.key_hash(k) for k in range(M)], rp.verifier_data()
    aggregated = True
    if args.aggregate:   # one aggregate per instance: proven again, now folded, and checked on the host and on the device
        agg, ashape, av = aggregate_setup(ctx, prog, N, n_lwe, log_n, cyc, vk, max(1, min(len(key_of), 64)), args.aggregate_device)
        t = time.perf_counter()
        blobs, _, agg_out = prog.prove_aggregate_batch(rp, agg, inputs, key_of, testvs)
        out["aggregate"] = aggregate_report(prog, ashape, av, blobs, inputs, key_of, hashes, testvs, agg_out, sum(len(p) for p in proofs[0]),
                                            time.perf_counter() - t)
        out["aggregate"]["out_cts_equal"] = bool((agg_out == out_cts).all())
        out["aggregate"].update(last_run=agg.last_run(), device_stats=agg.device_stats())
        aggregated = out["aggregate"]["accepted"] and out["aggregate"]["out_cts_equal"]
        av.close()
        agg.close()
    rp.close()
    n_gates = prog.n_gates
    shape = (ctx, vk[4:].reshape(-1, 4), [cyc.n_constants + 80, 135, 20, 16], vk[:4], log_n, cyc.n_constants, 80, cyc.gates, N, K, n_lwe, K * ELL * K * N)
    # ONE RingVerifier, slot k = the ring prover's slot k; all rows (instance, gate) in chunks of its max_batch
    rv = api.RingVerifier(*shape, max_keys=M, max_batch=max(1, min(len(key_of) * n_gates, 512)))
    for k in range(M):
        rv.set_key(k, hashes[k])
    t = time.perf_counter()
    verdicts, reasons, _ = prog.verify_batch(rv, inputs, key_of, testvs, out_cts, proofs)
    out["verify_seconds"] = time.perf_counter() - t

    def again(call):   # --runs R > 1: R more calls after that first one -> (seconds of each, event ms and launches of their combine kernel)
        secs = []
        ctx.timing_report()
        for _ in range(args.runs if args.runs > 1 else 0):
            t0 = time.perf_counter()
            call()
            secs.append(time.perf_counter() - t0)
        rep = ctx.timing_report().get("lwe_combine", {})
        return {"seconds": secs, "combine_event_ms": rep.get("ms", 0.0), "combine_launches": rep.get("count", 0)}
    out["verify_again"] = again(lambda: prog.verify_batch(rv, inputs, key_of, testvs, out_cts, proofs))
    rv.close()
    verified = int(verdicts.sum())
    why = {api.pbs_reason_text(int(r)) for v, r in zip(verdicts.reshape(-1), reasons.reshape(-1)) if not v}
    if args.verify_per_instance:   # the form before verify_batch: Program.verify per instance on the PbsVerifier of its key set
        pvs = [api.PbsVerifier(*shape, hashes[k], max_batch=max(1, min(n_gates, 64))) for k in range(M)]
        t = time.perf_counter()
        each = [prog.verify(pvs[key_of[b]], inputs[b], testvs, out_cts[b], proofs[b]) for b in range(len(key_of))]
        out["verify_per_instance_seconds"] = time.perf_counter() - t
        out["verify_per_instance_again"] = again(lambda: [prog.verify(pvs[key_of[b]], inputs[b], testvs, out_cts[b], proofs[b]) for b in range(len(key_of))])
        for pv in pvs:
            pv.close()
        out["verify_per_instance_equal"] = bool(all((e[0] == verdicts[b]).all() and (e[1] == reasons[b]).all() for b, e in enumerate(each)))
    out["verified"], out["rejected_because"] = verified, sorted(why)
    out["proven"] = verified == len(key_of) * n_gates and aggregated
    out["proven_wires_equal"] = bool((wires == batch_wires).all())
    return wires, out["proven"] and out["proven_wires_equal"]


def main_batch(args):
    """--instances B --keys M: see the module text"""
    B, M = args.instances, max(1, args.keys)
    N, n_lwe, log_n = (8, 6, 13) if args.n8 else (1024, 728, 16)
    rng = np.random.default_rng(args.seed)
    if args.program:
        n_inputs, gates, n_luts = load_program(args.program)
    else:
        (n_inputs, gates), n_luts = layered(rng, args.levels, args.width, args.fan_in), 1
    n_gates, lv = len(gates), gate_levels(n_inputs, gates)
    n_levels = max([0] + lv)
    ctx = vpbs_amd.Context(0, log_n_max=max(16, log_n))
    keys = [ctx.keygen_device(N, K, ELL, LOGB, n_lwe, SEED + k, SIGMA_GLWE, SIGMA_LWE) for k in range(M)]
    testv, delta = api.testv(N, 2)
    testvs = np.stack([testv, np.where(testv == 0, testv, np.uint64(P) - testv)] + [rng.integers(0, P, size=N, dtype=np.uint64) for _ in range(2, n_luts)])
    testvs = np.ascontiguousarray(testvs[:max(n_luts, 1)])
    key_of = np.array([b % M for b in range(B)], np.uint32)
    msgs = rng.integers(0, 2, size=(B, n_inputs))
    words, kn = n_lwe + 1, K * N
    inputs = np.zeros((B, n_inputs, words), np.uint64)
    for b in range(B):
        k = keys[key_of[b]]
        for i in range(n_inputs):
            inputs[b, i] = api.lwe_encrypt(k["params"], k["s_lwe"], delta * int(msgs[b, i]) % P, nonce=b * n_inputs + i)
    max_batch = max(1, args.max_batch)
    out = {"what": "a program of %d gates on %d levels over %d inputs at N=%d, n=%d, for %d instances under %d key sets" %
                   (n_gates, n_levels, n_inputs, N, n_lwe, B, M), "gates": n_gates, "levels": n_levels, "inputs": n_inputs, "instances": B, "keys": M,
           "fan_in": None if args.program else args.fan_in, "max_batch": max_batch, "runs": args.runs}
    ctx.timing_enable(1)
    prog = api.Program(ctx, n_inputs, gates, testvs.shape[0])

    def leg(run, timer):
        run()                                                            # warm-up
        secs, launches, ms, wires, rep = [], [], [], None, {}
        for _ in range(args.runs):
            ctx.timing_report()
            t = time.perf_counter()
            wires = run()
            secs.append(time.perf_counter() - t)
            rep = ctx.timing_report()
            launches.append(rep.get(timer, {}).get("count", 0))
            ms.append(rep.get(timer, {}).get("ms", 0.0))
        # every figure per run, in the order of "seconds"
        return wires, rep, {"seconds": secs, "pbs_launches": launches[-1] if launches else 0, "pbs_launches_per_run": launches, "pbs_event_ms": ms,
                            "pbs_event_ms_per_launch": [m / max(c, 1) for m, c in zip(ms, launches)],
                            "wall_minus_launch_seconds": [s - m / 1e3 for s, m in zip(secs, ms)]}

    # ---- the baseline leg: Program.run per instance on the Bootstrapper of its key set ----
    bss = [api.Bootstrapper(ctx, k["d_bsk"], k["d_ksk"], K, ELL, LOGB, max_batch=max(1, min(max_batch, max(n_gates, 1))), N=N, n_lwe=n_lwe,
                            keys_on_device=True) for k in keys]
    per_instance = lambda: np.stack([prog.run(bss[key_of[b]], inputs[b], testvs, gate_cts=False, out_cts=False)[0] for b in range(B)]) \
        if B else np.zeros((0, n_inputs + n_gates, words), np.uint64)
    base_wires, base_rep, out["baseline"] = leg(per_instance, "pbs_batch")
    out["baseline"].update({"combine_event_ms": base_rep.get("lwe_combine", {}).get("ms", 0.0),   # of the last run, as the batched leg's
                            "combine_launches": base_rep.get("lwe_combine", {}).get("count", 0)})
    for bs in bss:
        bs.close()
    wires, ok = base_wires, True
    if not args.baseline:
        # ---- the batched leg: ONE Program.run_batch on a ring ----
        ring = api.KeyRing(ctx, K, ELL, LOGB, N, n_lwe, max_keys=M, max_batch=max_batch)
        for k in keys:
            ring.add(k["d_bsk"], k["d_ksk"], keys_on_device=True)
        wires, rep, out["batch"] = leg(lambda: prog.run_batch(ring, inputs, key_of, testvs, gate_cts=False, out_cts=False)[0], "pbs_keyring")
        ring.close()
        if args.prove:
            out["all_batch_equal"] = bool(wires.shape == base_wires.shape and (wires == base_wires).all())
            wires, proven = prove_batch(args, ctx, prog, N, n_lwe, log_n, M, inputs, key_of, testvs, wires, out)
        terms = sum(len(g[0]) for g in gates)
        out["batch"].update({"combine_event_ms": rep.get("lwe_combine", {}).get("ms", 0.0), "combine_launches": rep.get("lwe_combine", {}).get("count", 0),
                             "combine_bytes": 8 * words * B * (terms + n_gates),               # a read per term, a write per gate
                             "deliver_event_ms": rep.get("program_deliver", {}).get("ms", 0.0),
                             "deliver_bytes": 2 * 8 * words * B * (n_inputs + n_gates),        # every wire read and written once
                             # inputs, test vectors, and the index array: identity | slot and lut of every gate row | input rows | wire rows
                             "h2d_bytes": 8 * (B * n_inputs * words + testvs.shape[0] * N) +
                                          4 * (max(1, min(max_batch, B * max([0] + [sum(1 for x in lv if x == level) for level in range(1, n_levels + 1)]))) + B * (2 * n_gates + n_inputs) + B * (n_inputs + n_gates)),
                             "d2h_bytes": 8 * B * (n_inputs + n_gates) * words})
        out["batch_over_baseline"] = statistics.median(out["batch"]["seconds"]) / statistics.median(out["baseline"]["seconds"])
        out["all_equal"] = bool(wires.shape == base_wires.shape and (wires == base_wires).all())
        out["wires_sha256"] = hashlib.sha256(np.ascontiguousarray(wires).tobytes()).hexdigest()
        ok = out["all_equal"] and (not args.prove or proven)
    prog.close()
    # ---- every program output (the wires of the last level), under its own key ----
    outputs = [n_inputs + g for g in range(n_gates) if lv[g] == n_levels]
    checked = correct = decrypted = 0
    for b in range(B):
        known = known_messages(n_inputs, gates, [int(m) for m in msgs[b]])
        for w in outputs:
            m = rounded(api.lwe_decrypt(keys[key_of[b]]["s_lwe"], wires[b, w]), delta)
            decrypted += 1
            if known[w] is not None:
                checked += 1
                correct += m == known[w]
    out["decrypted"], out["decrypted_checked"], out["decrypted_correct"] = decrypted, checked, int(correct)
    ok = ok and correct == checked
    for k in keys:
        ctx.device_free(k["d_bsk"])
        ctx.device_free(k["d_ksk"])
    ctx.close()
    print(json.dumps(out))
    return 0 if ok else 1


TABLES = [[0, 1], [1, 0], [1, 1], [0, 0]]      # over {0, 1}: the identity, its complement, the constants; slot j holds TABLES[j % 4]


def multi_netlist(levels, width, s):
    """-> (gates of the multi-output form, gates of the single-output form, the table behind every wire's message).  W inputs, L layers of W
    gates with s outputs each; gate g of layer l reads EVERY output of gate g of the layer before it: output (g + l) % s with coefficient 1,
    every other output once with 1 and once with p - 1 (they cancel word for word), so its message is that one output's.  The single-output
    form has one gate per (gate, j) with table j alone; both forms number the wire of (gate, j) width + gate * s + j."""
    multi, single, main = [], [], []
    theta = s.bit_length() - 1
    for lv in range(levels):
        for g in range(width):
            if lv == 0:
                terms, j_main = [(g, 1)], None
            else:
                first = width + ((lv - 1) * width + g) * s
                j_main = (g + lv) % s
                terms = [(first + j_main, 1)] + [(first + j, c) for j in range(s) if j != j_main for c in (1, P - 1)]
            multi.append((terms, 0, 0, theta, s))
            single += [(terms, 0, j) for j in range(s)]
            main.append(j_main)
    return multi, single, main


def multi_messages(levels, width, s, main, msgs):
    """the message of every wire of one instance: inputs, then TABLES[j % 4][message of the gate's input] for every (gate, j)"""
    known = [int(m) for m in msgs]
    for lv in range(levels):
        for g in range(width):
            gate = lv * width + g
            m_in = known[g] if lv == 0 else known[width + ((lv - 1) * width + g) * s + main[gate]]
            known += [TABLES[j % 4][m_in] for j in range(s)]
    return known


def snap_np(a, log_n, theta):
    """vpbs_lwe_snap on canonical words, in numpy"""
    if theta == 0:
        return a
    t = np.uint64(64 - (log_n + 1) + theta)
    r = (a >> t) + ((a >> (t - np.uint64(1))) & np.uint64(1))
    return np.where((r >> (np.uint64(64) - t)) != 0, np.uint64(0), r << t)


def extract_at_np(glwe, n_lwe, j):
    """vpbs_lwe_extract_at of one GLWE [K][N], in numpy"""
    neg = lambda a: np.where(a == 0, a, np.uint64(P) - a)
    full = np.concatenate([np.concatenate([a[j::-1], neg(a[:j:-1])]) for a in glwe[:-1]])
    return np.concatenate([full[:n_lwe], glwe[-1][j:j + 1]])


def compose_multi(bs, n_inputs, gates, levels, width, s, inputs, testvs):
    """the multi-output program as the composition combine -> snap -> Bootstrapper.run -> extract_at, layer by layer, in numpy -> wires"""
    words, log_n, theta = inputs.shape[1], bs.N.bit_length() - 1, s.bit_length() - 1
    wires = np.zeros((n_inputs + len(gates) * s, words), np.uint64)
    wires[:n_inputs] = inputs % np.uint64(P)
    for lv in range(levels):
        todo = list(range(lv * width, (lv + 1) * width))
        cts = np.zeros((width, words), np.uint64)
        for t in range(max(len(gates[g][0]) for g in todo)):
            rows = [k for k, g in enumerate(todo) if len(gates[g][0]) > t]
            for c in sorted({gates[todo[k]][0][t][1] for k in rows}):
                sel = [k for k in rows if gates[todo[k]][0][t][1] == c]
                cts[sel] = addmod(cts[sel], mulmod(wires[[gates[todo[k]][0][t][0] for k in sel]], c))
        cts = snap_np(cts, log_n, theta)
        for lo in range(0, width, bs.max_batch):
            out, _ = bs.run(cts[lo:lo + bs.max_batch], testvs[[gates[g][2] for g in todo[lo:lo + bs.max_batch]]])
            for k, g in enumerate(todo[lo:lo + bs.max_batch]):
                for j in range(s):
                    wires[n_inputs + g * s + j] = extract_at_np(out[k].reshape(bs.K, bs.N), bs.n_lwe, j)
    wires[:n_inputs] = inputs
    return wires


def main_multi(args):
    """--multi THETA: gates with 2^THETA tables each against the same functions as single-output gates, on the same inputs; see the module text"""
    theta, s, p = args.multi, 1 << args.multi, 2
    N, n_lwe, log_n = (8, 6, 13) if args.n8 else (1024, 728, 16)
    if s * 2 * p > N:
        raise SystemExit("--multi %d: 2^theta * 2 p = %d exceeds N = %d" % (theta, s * 2 * p, N))
    batched = args.instances is not None
    B, M = (args.instances, max(1, args.keys)) if batched else (1, 1)
    L, W = args.levels, args.width
    rng = np.random.default_rng(args.seed)
    multi, single, main_out = multi_netlist(L, W, s)
    ctx = vpbs_amd.Context(0, log_n_max=max(16, log_n))
    host = [ctx.keygen(N, K, ELL, LOGB, n_lwe, SEED + k, SIGMA_GLWE, SIGMA_LWE) for k in range(M)]
    delta = api.testv(N, p)[1]
    tables = np.array([TABLES[j % 4] for j in range(s)], np.uint64)
    tv_multi = api.lut_testv_multi(N, p, tables, delta)[0].reshape(1, N)
    tv_single = np.stack([api.lut_testv(N, p, t, delta)[0] for t in tables])
    key_of = np.array([b % M for b in range(B)], np.uint32)
    msgs = rng.integers(0, 2, size=(B, W))
    inputs = np.stack([np.stack([api.lwe_encrypt(host[key_of[b]]["params"], host[key_of[b]]["s_lwe"], delta * int(m) % P, nonce=b * W + i)
                                 for i, m in enumerate(msgs[b])]) for b in range(B)])
    expected = np.array([multi_messages(L, W, s, main_out, msgs[b]) for b in range(B)], np.uint64)
    words = n_lwe + 1
    out = {"what": "%d layers of %d lookups of %d tables each at N=%d, n=%d, %d instance(s) under %d key set(s): one gate per lookup (multi, "
                   "theta=%d) against one gate per table (single)" % (L, W, s, N, n_lwe, B, M, theta),
           "theta": theta, "slots": s, "levels": L, "width": W, "instances": B, "keys": M, "runs": args.runs, "outputs": B * L * W * s}
    max_batch = max(1, args.max_batch)
    bss = [api.Bootstrapper(ctx, k["bsk"], k["ksk"], K, ELL, LOGB, max_batch=max(1, min(max_batch, L * W * s))) for k in host]
    ring = None
    if batched:
        ring = api.KeyRing(ctx, K, ELL, LOGB, N, n_lwe, max_keys=M, max_batch=max_batch)
        for k in host:
            ring.add(k["bsk"], k["ksk"])
    ok = True
    prover = shape = hashes = None
    if args.prove:
        cyc_path, dum_path = circuit_file.find_cyclic_circuit(N, K, ELL, LOGB, n_lwe, log_n)
        cyc, dum = circuit_file.load(cyc_path), circuit_file.load(dum_path)
        chains = args.chains or (2 if args.n8 else 8)
        api.host_set_late_threads(api.late_threads_for(chains, api.host_cpu_budget()))
        api.host_set_early_threads(api.early_threads_for(chains))
        wb = args.witness_batch or (3 if args.n8 else 64)
        if batched:
            prover = api.RingProver(0, cyc, dum, K, ELL, LOGB, N, n_lwe, max_keys=M, chains=chains, witness_batch=wb)
            for k in range(M):
                assert prover.add(host[k]["bsk"], host[k]["ksk"]) == k
        else:
            prover = api.PbsProver(0, cyc, dum, host[0]["bsk"], host[0]["ksk"], K, ELL, LOGB, chains=chains, witness_batch=wb)
    for name, gates, testvs in (("multi", multi, tv_multi), ("single", single, tv_single)):
        prog = api.Program(ctx, W, gates, testvs.shape[0])
        if batched:
            run = lambda: prog.run_batch(ring, inputs, key_of, testvs, gate_cts=False, out_cts=False)[0]
        else:
            run = lambda: prog.run(bss[0], inputs[0], testvs, gate_cts=False, out_cts=False)[0][None]
        run()                                                            # warm-up
        secs, wires = [], None
        for _ in range(args.runs):
            t = time.perf_counter()
            wires = run()
            secs.append(time.perf_counter() - t)
        leg = out[name] = {"gates": len(gates), "proofs": len(gates) * B, "wires": int(wires.shape[1]), "eval_seconds": secs}
        if name == "multi":   # every wire against the composition snap -> Bootstrapper.run -> extract_at in numpy
            want = np.stack([compose_multi(bss[key_of[b]], W, gates, L, W, s, inputs[b], testvs) for b in range(B)])
            leg["mismatches"] = int((wires != want).any(axis=2).sum())
            ok = ok and leg["mismatches"] == 0
        if args.prove:
            n_gates, rows = len(gates), len(gates) * B
            t = time.perf_counter()
            if batched:
                proofs, p_wires, out_cts = prog.prove_batch(prover, inputs, key_of, testvs)
            else:
                proofs, p_wires, out_cts = prog.prove(prover, inputs[0], testvs)
                proofs, p_wires, out_cts = [proofs], p_wires[None], out_cts[None]
            leg["prove_seconds"] = time.perf_counter() - t
            leg["proof_bytes"] = sum(len(blob) for row in proofs for blob in row)
            if shape is None:
                hashes = [prover.key_hash(k) for k in range(M)] if batched else [prover.key_hash()]
                vk = prover.verifier_data()[0]
                shape = (ctx, vk[4:].reshape(-1, 4), [cyc.n_constants + 80, 135, 20, 16], vk[:4], log_n, cyc.n_constants, 80, cyc.gates, N, K,
                         n_lwe, K * ELL * K * N)
            t = time.perf_counter()
            if batched:
                rv = api.RingVerifier(*shape, max_keys=M, max_batch=max(1, min(rows, 512)))
                for k in range(M):
                    rv.set_key(k, hashes[k])
                verdicts = prog.verify_batch(rv, inputs, key_of, testvs, out_cts, proofs)[0]
                rv.close()
            else:
                pv = api.PbsVerifier(*shape, hashes[0], max_batch=max(1, min(n_gates, 64)))
                verdicts = prog.verify(pv, inputs[0], testvs, out_cts[0], proofs[0])[0]
                pv.close()
            leg["verify_seconds"] = time.perf_counter() - t
            leg["verified"] = int(verdicts.sum())
            leg["proven_wires_equal"] = bool((p_wires == wires).all())
            ok = ok and leg["verified"] == rows and leg["proven_wires_equal"]
        if args.margins:   # what every gate's bootstrap looks up (Program.margins), per level, beside the decryption failures below
            slots = s if name == "multi" else 1
            bound = N // (2 * p) - slots
            per_level = None
            for b in range(B):
                known = expected[b]
                m_in = [int(known[g]) if lv == 0 else int(known[W + ((lv - 1) * W + g) * s + main_out[lv * W + g]])
                        for lv in range(L) for g in range(W) for _ in range(s // slots)]
                if batched:
                    cts = prog.run_batch(ring, inputs[b:b + 1], key_of[b:b + 1], testvs, out_cts=False)[1][0]
                else:
                    cts = prog.run(bss[0], inputs[0], testvs, out_cts=False)[1]
                per_level = prog.margins(ctx, host[key_of[b]]["s_lwe"], cts, [p] * testvs.shape[0], expected=m_in, N=N, stats=per_level)[3]
            leg["margins"] = [{"level": lv + 1, "count": st.count, "failures": st.failures, "std_positions": st.std(),
                               "mean_positions": st.mean(), "max_abs_positions": st.max_abs, "margin_positions": bound,
                               "tail_log2_at_margin": st.tail_log2(bound)} for lv, st in enumerate(per_level)]
        prog.close()
        # every output wire under its own key, through lwe_decode_batch: failures = decoded message != the table's entry
        stats = api.NoiseStats()
        for b in range(B):
            ctx.lwe_decode_batch(host[key_of[b]]["s_lwe"], np.ascontiguousarray(wires[b, W:]), delta, 2 * p, expected=expected[b, W:], stats=stats)
        leg["decrypted"], leg["decrypt_failures"] = stats.count, stats.failures
        leg["noise_std_over_delta"] = stats.std() / delta
        leg["noise_max_over_delta"] = stats.max_abs / delta
    out["all_equal"] = out["multi"]["mismatches"] == 0
    if args.prove:
        prover.close()
    if ring is not None:
        ring.close()
    for bs in bss:
        bs.close()
    ctx.close()
    print(json.dumps(out))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--fan-in", type=int, default=2)
    ap.add_argument("--program")
    ap.add_argument("--n8", action="store_true")
    ap.add_argument("--prove", action="store_true")
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--chains", type=int, default=0)
    ap.add_argument("--witness-batch", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--instances", type=int)
    ap.add_argument("--keys", type=int, default=1)
    ap.add_argument("--verify-per-instance", action="store_true")
    ap.add_argument("--multi", type=int)
    ap.add_argument("--margins", action="store_true")
    ap.add_argument("--aggregate", action="store_true")
    ap.add_argument("--aggregate-device", type=int, nargs="?", const=32, default=None, metavar="MAX_NODES")
    args = ap.parse_args()
    if args.aggregate_device is not None and (not args.aggregate or args.aggregate_device < 1):
        raise SystemExit("--aggregate-device [max_nodes] (at least 1; default 32) is a switch of --prove --aggregate")
    if args.aggregate and (not args.prove or args.multi is not None):
        raise SystemExit("--aggregate folds the gate proofs of --prove into one proof per instance: it needs --prove and cannot run with --multi")
    if args.margins and args.multi is None:
        raise SystemExit("--margins reports the rotation margins of the --multi legs: it needs --multi THETA")
    if args.multi is not None:
        if args.baseline or args.program:
            raise SystemExit("--multi builds its own netlist and both legs: it cannot run with --baseline or --program")
        return main_multi(args)
    if args.baseline and args.prove:
        raise SystemExit("--baseline evaluates only: it cannot run with --prove")
    if args.instances is not None:
        return main_batch(args)
    N, n_lwe, log_n = (8, 6, 13) if args.n8 else (1024, 728, 16)
    rng = np.random.default_rng(args.seed)
    if args.program:
        n_inputs, gates, n_luts = load_program(args.program)
    else:
        (n_inputs, gates), n_luts = layered(rng, args.levels, args.width, args.fan_in), 1
    n_gates, lv = len(gates), gate_levels(n_inputs, gates)
    n_levels = max([0] + lv)
    ctx = vpbs_amd.Context(0, log_n_max=max(16, log_n))
    keys = ctx.keygen(N, K, ELL, LOGB, n_lwe, SEED, SIGMA_GLWE, SIGMA_LWE)
    testv, delta = api.testv(N, 2)
    testvs = np.stack([testv, np.where(testv == 0, testv, np.uint64(P) - testv)] + [rng.integers(0, P, size=N, dtype=np.uint64) for _ in range(2, n_luts)])
    testvs = np.ascontiguousarray(testvs[:max(n_luts, 1)])
    msgs = [int(m) for m in rng.integers(0, 2, size=n_inputs)]
    inputs = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * m % P, nonce=i) for i, m in enumerate(msgs)])
    known = known_messages(n_inputs, gates, msgs)
    bs = api.Bootstrapper(ctx, keys["bsk"], keys["ksk"], K, ELL, LOGB, max_batch=max(1, min(args.max_batch, max(n_gates, 1))))
    words, kn = n_lwe + 1, K * N
    per_level = [sum(1 for x in lv if x == level) for level in range(1, n_levels + 1)]
    out = {"what": "a program of %d gates on %d levels over %d inputs at N=%d, n=%d" % (n_gates, n_levels, n_inputs, N, n_lwe), "gates": n_gates,
           "levels": n_levels, "inputs": n_inputs, "fan_in": None if args.program else args.fan_in, "max_batch": bs.max_batch, "runs": args.runs}
    ctx.timing_enable(1)

    # ---- the baseline leg ----
    run_baseline(ctx, bs, n_inputs, gates, lv, inputs, testvs)       # warm-up
    base_s, base_wires, base_events = [], None, None
    for _ in range(args.runs):
        ctx.timing_report()
        t = time.perf_counter()
        base_wires, base_events = run_baseline(ctx, bs, n_inputs, gates, lv, inputs, testvs)
        base_s.append(time.perf_counter() - t)
    out["baseline"] = {"seconds": base_s, "seconds_per_level": statistics.median(base_s) / max(n_levels, 1), "pbs_event_ms_per_level": base_events,
                       "h2d_bytes": 8 * sum(c * (words + N) for c in per_level), "d2h_bytes": 8 * sum(c * (kn + words) for c in per_level)}
    ok = True
    if not args.baseline:
        # ---- the resident leg: wires only ----
        prog = api.Program(ctx, n_inputs, gates, testvs.shape[0])
        assert prog.levels()[0].tolist() == lv
        prog.run(bs, inputs, testvs, gate_cts=False, out_cts=False)      # warm-up
        res_s, wires, rep = [], None, {}
        for _ in range(args.runs):
            ctx.timing_report()
            t = time.perf_counter()
            wires = prog.run(bs, inputs, testvs, gate_cts=False, out_cts=False)[0]
            res_s.append(time.perf_counter() - t)
            rep = ctx.timing_report()
        launches = max(rep.get("pbs_batch", {}).get("count", 0), 1)
        out["resident"] = {"seconds": res_s, "seconds_per_level": statistics.median(res_s) / max(n_levels, 1),
                           "pbs_event_ms_per_level": rep.get("pbs_batch", {}).get("ms", 0.0) / max(n_levels, 1),
                           "pbs_launches": launches, "combine_event_ms_total": rep.get("lwe_combine", {}).get("ms", 0.0),
                           "h2d_bytes": 8 * (n_inputs * words + testvs.shape[0] * N), "d2h_bytes": 8 * (n_inputs + n_gates) * words}
        out["resident_over_baseline"] = statistics.median(res_s) / statistics.median(base_s)
        out["all_equal"] = bool((wires == base_wires).all())
        ok = out["all_equal"]
        if args.prove:
            cyc_path, dum_path = circuit_file.find_cyclic_circuit(N, K, ELL, LOGB, n_lwe, log_n)
            cyc, dum = circuit_file.load(cyc_path), circuit_file.load(dum_path)
            chains = args.chains or (2 if args.n8 else 8)
            api.host_set_late_threads(api.late_threads_for(chains, api.host_cpu_budget()))
            api.host_set_early_threads(api.early_threads_for(chains))
            prover = api.PbsProver(0, cyc, dum, keys["bsk"], keys["ksk"], K, ELL, LOGB, chains=chains,
                                   witness_batch=args.witness_batch or (3 if args.n8 else 64))
            t = time.perf_counter()
            proofs, p_wires, out_cts = prog.prove(prover, inputs, testvs)
            out["prove_seconds"] = time.perf_counter() - t
            kh, (vk, _) = prover.key_hash(), prover.verifier_data()
            aggregated = True
            if args.aggregate:
                agg, ashape, av = aggregate_setup(ctx, prog, N, n_lwe, log_n, cyc, vk, 1, args.aggregate_device)
                t = time.perf_counter()
                blob, _, agg_out = prog.prove_aggregate(prover, agg, inputs, testvs)
                out["aggregate"] = aggregate_report(prog, ashape, av, [blob], inputs[None], [0], [kh], testvs, agg_out[None], sum(len(p) for p in proofs),
                                                    time.perf_counter() - t)
                out["aggregate"]["out_cts_equal"] = bool((agg_out == out_cts).all())
                out["aggregate"].update(last_run=agg.last_run(), device_stats=agg.device_stats())
                aggregated = out["aggregate"]["accepted"] and out["aggregate"]["out_cts_equal"]
                av.close()
                agg.close()
            prover.close()
            pv = api.PbsVerifier(ctx, vk[4:].reshape(-1, 4), [cyc.n_constants + 80, 135, 20, 16], vk[:4], log_n, cyc.n_constants, 80, cyc.gates, N, K,
                                 n_lwe, K * ELL * K * N, kh, max_batch=max(1, min(n_gates, 64)))
            t = time.perf_counter()
            verdicts, reasons, _ = prog.verify(pv, inputs, testvs, out_cts, proofs)
            out["verify_seconds"] = time.perf_counter() - t
            pv.close()
            out["verified"] = int(verdicts.sum())
            out["proven"] = out["verified"] == n_gates and aggregated
            out["rejected_because"] = sorted({api.pbs_reason_text(int(r)) for v, r in zip(verdicts, reasons) if not v})
            out["all_equal"] = bool(out["all_equal"] and (p_wires == base_wires).all())
            ok = out["all_equal"] and out["proven"]
        prog.close()
    # ---- the output wires (the last level) whose message is known ----
    outputs = [n_inputs + g for g in range(n_gates) if lv[g] == n_levels and known[n_inputs + g] is not None]
    got = [rounded(api.lwe_decrypt(keys["s_lwe"], base_wires[w]), delta) for w in outputs]
    out["decrypted_checked"] = len(outputs)
    out["decrypted_correct"] = sum(1 for w, m in zip(outputs, got) if m == known[w])
    ok = ok and out["decrypted_correct"] == out["decrypted_checked"]
    bs.close()
    ctx.close()
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
