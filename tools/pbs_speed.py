#!/usr/bin/env python3
"""Bootstraps per second of the batched bootstrap (api.Bootstrapper, csrc/pbs_batch.hip) at the paper's parameters (N = 1024, K = 2,
ELL = 4, LOGB = 5, n = 728, the paper's noise; --n2048 for the other ring): keys generated on the device and adopted, LWE encryptions of
alternating messages, every output checked by decryption of the extracted LWE ciphertext.  Per batch size: HIP-event time of the launch
and wall time of the whole call (upload of the ciphertexts, launch, download of both outputs), `--runs` timed runs after a warm-up.

--baseline times Context.pbs_accumulator_chain one ciphertext at a time (event time of its 1 460 launches, wall time of the call with its
key upload), checked by Glwe::decrypt; it uses nothing older builds lack, so it can be pointed at one:  --package DIR  imports vpbs_amd
from DIR instead of this tree.

usage: tools/pbs_speed.py [--batch 1,8,64,256,1024] [--runs 3] [--n2048] [--baseline [--calls 5]] [--package DIR]
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


if "--baseline" in args:
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
