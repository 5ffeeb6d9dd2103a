#!/usr/bin/env python3
"""What do seeded keys and ciphertexts save a client of a key ring, and what does expanding them cost the server?  A key set with the
client's own secrets under the split generator (Context.keygen_seeded: the mask streams from a public mask_seed), at the paper's
parameters or --n8.  Prints the bytes a client sends each way (derived from the shapes, not measured), then measures, alternating in ONE
process with a warm-up and --runs runs each (median and range of the wall time of the call; the slot is removed again outside the timing):
  add         KeyRing.add of the full key set from a host array                  (the yardstick: what a client had to send and upload)
  add_seeded  KeyRing.add_seeded of the bodies from a host array                 (1 / K of the bytes over PCIe, the rest regenerated)
  add_seeded_device  KeyRing.add_seeded of bodies that are already on the device (the expansion alone, with its two allocations)
and the HIP-event time of key_expand_kernel alone with the share of the HBM roofline its bytes (1 / K of the key set read, all of it
written) give.  Then --count seeded ciphertexts (8 bytes each and a nonce) are expanded on the device, bootstrapped through the ring and
decoded with lwe_decode_batch.  One JSON line; --out FILE writes it there too.

usage: tools/seeded_keys.py [--n8] [--runs R] [--count C] [--seed S] [--mask-seed M] [--out FILE]
mix64 is not a cryptographic generator: the figures are about bytes and time, the keys are not fit for production."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (the HIP runtime the library shares with it; device buffers)

import vpbs_amd  # noqa: E402
from vpbs_amd import api  # noqa: E402

K, ELL, LOGB = 2, 4, 5
SIGMA_GLWE, SIGMA_LWE = 4.99027217501041e-8, 1.17021618159313e-5
HBM_BYTES_PER_S = 8.0e12   # MI355X: 8 TB/s peak


def figures(seconds):
    return {"median_ms": 1e3 * statistics.median(seconds), "min_ms": 1e3 * min(seconds), "max_ms": 1e3 * max(seconds), "runs": len(seconds)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n8", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--count", type=int, default=8)
    ap.add_argument("--seed", type=lambda v: int(v, 0), default=0x5EED0728)
    ap.add_argument("--mask-seed", type=lambda v: int(v, 0), default=0x9A9E2)
    ap.add_argument("--out")
    a = ap.parse_args()
    N, n = (8, 6) if a.n8 else (1024, 728)
    if a.runs < 1 or a.count < 1 or a.count > 256:
        ap.error("runs at least 1, count 1 .. 256")
    ctx = vpbs_amd.Context(0, log_n_max=16)
    rng = np.random.default_rng(a.seed)
    s_lwe, s_glwe = rng.integers(0, 2, size=n, dtype=np.uint64), rng.integers(0, 2, size=(K - 1, N), dtype=np.uint64)
    sk = ctx.keygen_seeded(N, K, ELL, LOGB, n, a.seed, a.mask_seed, SIGMA_GLWE, SIGMA_LWE, s_lwe=s_lwe, s_glwe=s_glwe)
    full = ctx.key_expand(N, K, ELL, n, a.mask_seed, sk["bsk_bodies"], sk["ksk_bodies"])
    body_words, full_words = api.seeded_key_shapes(N, K, ELL, n)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()
    d_bb, d_kb = dev(sk["bsk_bodies"]), dev(sk["ksk_bodies"])
    ring = api.KeyRing(ctx, K, ELL, LOGB, N, n, max_keys=1, max_batch=a.count)
    legs = {"add": lambda: ring.add(full["bsk"], full["ksk"]),
            "add_seeded": lambda: ring.add_seeded(a.mask_seed, sk["bsk_bodies"], sk["ksk_bodies"]),
            "add_seeded_device": lambda: ring.add_seeded(a.mask_seed, d_bb.data_ptr(), d_kb.data_ptr(), bodies_on_device=True)}
    seconds = {name: [] for name in legs}
    for run in range(a.runs + 1):          # run 0 warms up: the pool's first allocations, the first launch of the kernel
        for name, leg in legs.items():
            t0 = time.perf_counter()
            slot = leg()
            dt = time.perf_counter() - t0
            ring.remove(slot)
            if run:
                seconds[name].append(dt)
    # the kernel alone, by HIP events: one launch for bsk and one for ksk per add_seeded
    ctx.timing_enable(1)
    for _ in range(a.runs):
        ring.remove(ring.add_seeded(a.mask_seed, d_bb.data_ptr(), d_kb.data_ptr(), bodies_on_device=True))
    rep = ctx.timing_report()["key_expand"]
    ctx.timing_enable(0)
    kernel_ms = rep["ms"] / a.runs           # both launches of one key set
    moved = 8 * (body_words + full_words)
    # seeded ciphertexts through the ring
    slot = ring.add_seeded(a.mask_seed, d_bb.data_ptr(), d_kb.data_ptr(), bodies_on_device=True)
    tv, delta = api.testv(N, 2)
    msgs = [int(m) for m in rng.integers(0, 2, size=a.count)]
    bodies = api.lwe_encrypt_seeded_batch(sk["params"], a.mask_seed, s_lwe, [delta * m % api.P for m in msgs], nonce0=0)
    d_cts = torch.zeros((a.count, n + 1), dtype=torch.int64, device="cuda")
    d_lwe = torch.zeros((a.count, n + 1), dtype=torch.int64, device="cuda")
    d_tv = dev(tv)
    torch.cuda.synchronize()
    ctx.lwe_expand_batch(n, a.mask_seed, bodies, nonce0=0, out_dev_ptr=d_cts.data_ptr())
    ring.run_device(d_cts.data_ptr(), a.count, [slot] * a.count, d_tv.data_ptr(), d_lwe_out=d_lwe.data_ptr())
    st = api.NoiseStats()
    got = ctx.lwe_decode_batch(s_lwe, d_lwe.data_ptr(), delta, 4, expected=msgs, count=a.count, stats=st, want=("msg",))
    out = {"N": N, "n_lwe": n, "K": K, "ELL": ELL, "runs": a.runs,
           "bytes": {"key_set_full": 8 * full_words, "key_set_bodies": 8 * body_words, "mask_seed": 8,
                     "ciphertext_full": 8 * (n + 1), "ciphertext_seeded": 8, "nonce": "implied by nonce0 and the position"},
           "wall": {name: figures(s) for name, s in seconds.items()},
           "key_expand_kernel": {"ms_per_key_set": kernel_ms, "launches": rep["count"], "bytes_moved": moved,
                                 "hbm_roofline_share": moved / (kernel_ms * 1e-3) / HBM_BYTES_PER_S, "hbm_bytes_per_s": HBM_BYTES_PER_S},
           "ciphertexts": {"count": a.count, "failures": st.failures, "decoded_ok": got["msg"].tolist() == msgs,
                           "max_abs_over_delta": st.max_abs / delta}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    ring.close()
    ctx.close()
    return 0 if out["ciphertexts"]["decoded_ok"] and st.failures == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
