#!/usr/bin/env python3
"""Bootstraps per second of the batched bootstrap (api.Bootstrapper, csrc/pbs_batch.hip) at the paper's parameters (N = 1024, K = 2,
ELL = 4, LOGB = 5, n = 728, the paper's noise; --n2048 for the other ring): keys generated on the device and adopted, LWE encryptions of
alternating messages, every output checked by decryption of the extracted LWE ciphertext.  Per batch size: HIP-event time of the launch
and wall time of the whole call (upload of the ciphertexts, launch, download of both outputs), `--runs` timed runs after a warm-up.

--baseline times Context.pbs_accumulator_chain one ciphertext at a time (event time of its 1 460 launches, wall time of the call with its
key upload), checked by Glwe::decrypt; it uses nothing older builds lack, so it can be pointed at one:  --package DIR  imports vpbs_amd
from DIR instead of this tree.

--keys M spreads every batch over M seeded key sets (Context.keygen_device; ciphertext i under key set i mod M) and bootstraps it in ONE
api.KeyRing launch (csrc/pbs_keyring.hip); every output is decrypted under its own key.  --keys M --baseline does the same with M
Bootstrappers run one after the other, which needs nothing older builds lack.  --shape N,K,ELL,LOGB,n replaces the paper's shape.

usage: tools/pbs_speed.py [--batch 1,8,64,256,1024] [--runs 3] [--n2048] [--shape N,K,ELL,LOGB,n] [--keys M] [--baseline [--calls 5]]
       [--package DIR]
One JSON line."""
import json
import os
import sys
import time

args = sys.argv[1:]


def opt(name, default):
    return args[args.index(name) + 1] if name in args else default


sys.path.insert(0, opt("--package", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import vpbs_amd
from vpbs_amd import api

P = api.P
N = 2048 if "--n2048" in args else 1024
K, ELL, LOGB, N_LWE, PMOD = 2, 4, 5, 728, 2
if "--shape" in args:
    N, K, ELL, LOGB, N_LWE = (int(v) for v in opt("--shape", "").split(","))
M_KEYS = int(opt("--keys", "0"))
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)      # main.rs:29-30
SEED = 0x5EED
runs = int(opt("--runs", "3"))
ctx = vpbs_amd.Context(0, log_n_max=16)
testv, delta = api.testv(N, PMOD)
rounded = lambda m_bar: round(int(m_bar) / delta) % (2 * PMOD)
med = lambda x: sorted(x)[len(x) // 2]
result = {"tool": "pbs_speed", "N": N, "K": K, "ELL": ELL, "LOGB": LOGB, "n_lwe": N_LWE, "runs": runs}


def event_ms(name):
    rep = ctx.timing_report()
    return rep[name]["ms"] if name in rep else None


if M_KEYS:
    # key set m = SEED + m; ciphertext i of a batch belongs to key set i mod M, so the batch arrives in mixed order
    batches = [int(b) for b in opt("--batch", "256").split(",")]
    baseline = "--baseline" in args
    keys = [ctx.keygen_device(N, K, ELL, LOGB, N_LWE, SEED + m, *SIGMAS) for m in range(M_KEYS)]
    top = max(batches)
    all_cts = np.stack([api.lwe_encrypt(keys[i % M_KEYS]["params"], keys[i % M_KEYS]["s_lwe"], delta * (i % 2) % P, nonce=i) for i in range(top)])
    key_of = np.arange(top, dtype=np.uint32) % M_KEYS
    if baseline:
        per_key = -(-top // M_KEYS)
        boots = [api.Bootstrapper(ctx, k["d_bsk"], k["d_ksk"], K, ELL, LOGB, max_batch=per_key, N=N, n_lwe=N_LWE, keys_on_device=True) for k in keys]
        timer = "pbs_batch"
    else:
        ring = api.KeyRing(ctx, K, ELL, LOGB, N, N_LWE, max_keys=M_KEYS, max_batch=top)
        for k in keys:
            ring.add(k["d_bsk"], k["d_ksk"], keys_on_device=True)
        timer = "pbs_keyring"

    def bootstrap(cts, ko):
        if not baseline:
            return ring.run(cts, ko, testv)[1]
        lwe_out = np.zeros_like(cts)
        for m in range(M_KEYS):
            rows = np.flatnonzero(ko == m)
            if rows.size:
                lwe_out[rows] = boots[m].run(cts[rows], testv)[1]
        return lwe_out
    rows_out = []
    for b in batches:
        cts, ko = all_cts[:b], key_of[:b]
        bootstrap(cts, ko)   # warm-up
        ctx.timing_enable(1)
        wall, ev = [], []
        for r in range(runs):
            t = time.perf_counter()
            lwe_out = bootstrap(cts, ko)
            wall.append((time.perf_counter() - t) * 1e3)
            ev.append(event_ms(timer))   # the sum over the launches of the call
            for m in range(M_KEYS):
                sel = np.flatnonzero(ko == m)
                got = [rounded(v) for v in api.lwe_decrypt(keys[m]["s_lwe"], lwe_out[sel])] if sel.size else []
                assert got == [int(i) % 2 for i in sel], "batch %d: an output of key set %d decrypts to the wrong message" % (b, m)
        ctx.timing_enable(0)
        rows_out.append({"batch": b, "launches": min(b, M_KEYS) if baseline else 1, "event_ms": [round(e, 3) for e in ev],
                         "wall_ms": [round(w, 3) for w in wall], "bootstraps_per_s": round(b / (med(ev) * 1e-3), 1), "all_decrypted": True})
    # bytes of key material one launch has to read when nothing is shared between key sets: (n + 1) GGSWs of K ELL K N words per key set in use
    result.update(mode="keyring_baseline" if baseline else "keyring", keys=M_KEYS, threads=os.environ.get("VPBS_PBS_BATCH_THREADS", "auto"),
                  key_set_bytes=(N_LWE + 1) * K * ELL * K * N * 8, rows=rows_out)
    for o in (boots if baseline else [ring]):
        o.close()
    for k in keys:
        ctx.device_free(k["d_bsk"])
        ctx.device_free(k["d_ksk"])
elif "--baseline" in args:
    calls = int(opt("--calls", "5"))
    keys = ctx.keygen(N, K, ELL, LOGB, N_LWE, SEED, *SIGMAS)
    acc_init = np.concatenate([np.zeros((K - 1, N), np.uint64), testv.reshape(1, N)])
    cts = [api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * (i % 2) % P, nonce=i) for i in range(calls)]
    ctx.pbs_accumulator_chain(acc_init, cts[0], keys["bsk"], keys["ksk"], K, ELL, LOGB)   # warm-up
    ctx.timing_enable(1)
    out = []
    for r in range(runs):
        wall, ev = [], []
        for i, ct in enumerate(cts):
            t = time.perf_counter()
            accs = ctx.pbs_accumulator_chain(acc_init, ct, keys["bsk"], keys["ksk"], K, ELL, LOGB)
            wall.append((time.perf_counter() - t) * 1e3)
            ev.append(event_ms("pbs_accumulator_chain"))
            assert rounded(ctx.glwe_decrypt(keys["s_to"], accs[-1])[0]) == i % 2, "baseline bootstrap %d decrypts to the wrong message" % i
        out.append({"wall_ms_per_call": med(wall), "event_ms_per_call": med(ev), "wall_ms_all": [round(w, 3) for w in wall]})
    result.update(mode="baseline", calls=calls, runs_detail=out,
                  wall_ms_per_bootstrap=[o["wall_ms_per_call"] for o in out], event_ms_per_bootstrap=[o["event_ms_per_call"] for o in out])
else:
    batches = [int(b) for b in opt("--batch", "1,8,64,256,1024").split(",")]
    keys = ctx.keygen_device(N, K, ELL, LOGB, N_LWE, SEED, *SIGMAS)
    bs = api.Bootstrapper(ctx, keys["d_bsk"], keys["d_ksk"], K, ELL, LOGB, max_batch=max(batches), N=N, n_lwe=N_LWE, keys_on_device=True)
    all_cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * (i % 2) % P, nonce=i) for i in range(max(batches))])
    rows = []
    for b in batches:
        cts = all_cts[:b]
        bs.run(cts, testv)   # warm-up
        ctx.timing_enable(1)
        wall, ev = [], []
        for r in range(runs):
            t = time.perf_counter()
            out_ct, lwe_out = bs.run(cts, testv)
            wall.append((time.perf_counter() - t) * 1e3)
            ev.append(event_ms("pbs_batch"))
            got = [rounded(m) for m in api.lwe_decrypt(keys["s_lwe"], lwe_out)]
            assert got == [i % 2 for i in range(b)], "batch %d: an extracted output decrypts to the wrong message" % b
        ctx.timing_enable(0)
        rows.append({"batch": b, "event_ms": [round(e, 3) for e in ev], "wall_ms": [round(w, 3) for w in wall],
                     "event_ms_per_bootstrap": [round(e / b, 4) for e in ev], "wall_ms_per_bootstrap": [round(w / b, 4) for w in wall],
                     "bootstraps_per_s": round(b / (med(ev) * 1e-3), 1), "all_decrypted": True})
    # threads per ciphertext: the library's choice (1024, or 512 above one ciphertext per CU) unless the environment fixes it
    result.update(mode="batch", threads=os.environ.get("VPBS_PBS_BATCH_THREADS", "auto"), rows=rows)
    bs.close()
    ctx.device_free(keys["d_bsk"])
    ctx.device_free(keys["d_ksk"])
ctx.close()
print(json.dumps(result))
