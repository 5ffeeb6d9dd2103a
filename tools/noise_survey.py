#!/usr/bin/env python3
"""How noisy are the outputs of a batch of bootstraps, and how many decode wrongly?  Seeded keys at the paper's sigmas left on the device
(Context.keygen_device), the messages and the secret key uploaded once, then per chunk of --batch ciphertexts: Context.lwe_encrypt_batch on
the device, Bootstrapper.run_device with the test vector of a lookup table (api.lut_testv), Context.lwe_decode_batch of the inputs and of
the outputs with expected = m and table[m] into two api.NoiseStats.  Between the phases only the messages' 8 bytes per ciphertext come
back (for --baseline to compare); no ciphertext visits the host.  One JSON line.

usage: tools/noise_survey.py [--count C] [--batch B] [--p P] [--n8] [--baseline] [--seed S] [--rotation [--log-slots T]]
  --rotation: the rotation margins instead (rotation_survey below): Context.lwe_rotation_batch on the inputs, snapped with
    --log-slots, and on the bootstraps' outputs fed back in -- the statistics of dev in positions, NoiseStats.tail_log2 at the margin
    N / (2 P) - 2^T and the time of every call from events on the context's stream; with --baseline the same for lwe_decode_batch on
    the same rows.
  --p: messages in [0, P), table[m] = (m + 1) mod P, delta = get_delta(2 P); P a power of two (default 2).
  --n8: the N = 8, n = 6 miniature instead of the paper's N = 1024, n = 728.
  --baseline: the same outputs judged the way it had to be done before these calls existed: download the output ciphertexts, api.lwe_decrypt
    per ciphertext, the float rounding round(phase / delta) mod 2 P.  Reports all_equal for the messages against the device decode.
  seconds: wall time per phase (encrypt, bootstrap, decode of the OUTPUTS), each ending in a synchronised call; the baseline leg's decode
    includes its download.  The decode of the inputs (for their noise) is outside the three."""
import argparse
import json
import os
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


def noise_figures(st, delta):
    return {"count": st.count, "failures": st.failures, "std_over_delta": st.std() / delta, "mean_over_delta": st.mean() / delta,
            "max_abs_over_delta": st.max_abs / delta, "hist": st.hist}


def margin_figures(st, bound, ms):
    """dev in positions; tail_log2 is NoiseStats.tail_log2's Gaussian model at the margin N / (2p) - 2^theta"""
    ms = sorted(ms)
    return {"count": st.count, "failures": st.failures, "std_positions": st.std(), "mean_positions": st.mean(), "max_abs_positions": st.max_abs,
            "margin_positions": bound, "tail_log2_at_margin": st.tail_log2(bound), "hist": st.hist[:20],
            "call_ms_median": ms[len(ms) // 2], "call_ms_min": ms[0], "call_ms_max": ms[-1], "calls": len(ms)}


def rotation_survey(a, ctx, N, n):
    """--rotation: what the bootstraps will look up (Context.lwe_rotation_batch), for the input ciphertexts -- snapped with --log-slots as a
    multi-output gate snaps them -- and for the bootstraps' outputs fed back in as inputs of a gate with the same log_slots.  dev is measured
    from the position of the message (expected = m, table[m]); every call is timed by events on the context's stream, around the whole
    call (tally memset, the launch, the 608 + 8 bytes that come back).  --baseline adds lwe_decode_batch on the same rows, timed the same way."""
    theta, p = a.log_slots, a.p
    s = 1 << theta
    if theta < 0 or p * s * 2 > N:
        raise SystemExit("noise_survey: 2^log_slots must stay below the half block N / (2p)")
    keys = ctx.keygen_device(N, K, ELL, LOGB, n, a.seed, SIGMA_GLWE, SIGMA_LWE)
    table = [(m + 1) % p for m in range(p)]
    if theta:
        testv, delta = api.lut_testv_multi(N, p, np.array([table] * s, np.uint64))
    else:
        testv, delta = api.lut_testv(N, p, table)
    bound = N // (2 * p) - s
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, p, size=a.count, dtype=np.uint64)
    want = np.array(table, np.uint64)[msgs]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()
    d_key, d_tv = dev(keys["s_lwe"]), dev(testv)
    d_plain, d_msgs, d_want = dev(msgs * np.uint64(delta)), dev(msgs), dev(want)
    batch = min(a.batch, a.count)
    d_raw, d_in, d_out = (torch.zeros((batch, n + 1), dtype=torch.int64, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    bs = api.Bootstrapper(ctx, keys["d_bsk"], keys["d_ksk"], K, ELL, LOGB, max_batch=batch, N=N, n_lwe=n, keys_on_device=True)
    stream = torch.cuda.ExternalStream(ctx.stream)
    names = ("inputs", "outputs")
    rot = {k: (api.NoiseStats(), []) for k in names}
    dec = {k: (api.NoiseStats(), []) for k in names}

    def timed(call, ms, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if keep:
            ms.append(e0.elapsed_time(e1))

    def chunk(lo, hi, keep):
        c = hi - lo
        ctx.lwe_encrypt_batch(keys["params"], d_key.data_ptr(), d_plain.data_ptr() + 8 * lo, nonce0=lo, out_dev_ptr=d_raw.data_ptr(), count=c)
        ctx.lwe_snap(N, theta, d_raw.data_ptr(), count=c * (n + 1), out_dev_ptr=d_in.data_ptr())       # theta 0: the reduced words
        bs.run_device(d_in.data_ptr(), c, d_tv.data_ptr(), d_lwe_out=d_out.data_ptr())
        for name, rows, exp, slots in (("inputs", d_in, d_msgs, 0), ("outputs", d_out, d_want, theta)):
            st, ms = rot[name]
            timed(lambda: ctx.lwe_rotation_batch(d_key.data_ptr(), rows.data_ptr(), N, p, log_slots=slots, expected=exp.data_ptr() + 8 * lo,
                                                 count=c, stats=st if keep else None, want=(), n_lwe=n), ms, keep)
            if a.baseline:
                st, ms = dec[name]
                timed(lambda: ctx.lwe_decode_batch(d_key.data_ptr(), rows.data_ptr(), delta, 2 * p, expected=exp.data_ptr() + 8 * lo, count=c,
                                                   stats=st if keep else None, want=(), n_lwe=n), ms, keep)

    chunk(0, min(batch, 64), keep=False)                   # warm-up: code objects, the pool's buffers
    for lo in range(0, a.count, batch):
        chunk(lo, min(lo + batch, a.count), keep=True)
    line = {"tool": "noise_survey", "leg": "rotation", "N": N, "n_lwe": n, "p": p, "log_slots": theta, "count": a.count, "batch": batch,
            "seed": a.seed, "sigma_glwe": SIGMA_GLWE, "sigma_lwe": SIGMA_LWE, "bytes_read_per_call": batch * (n + 1) * 8,
            "rotation": {k: margin_figures(rot[k][0], bound, rot[k][1]) for k in names}}
    if a.baseline:
        line["decode"] = {k: dict(noise_figures(dec[k][0], delta), call_ms_median=sorted(dec[k][1])[len(dec[k][1]) // 2],
                                  tail_log2_at_half_delta=dec[k][0].tail_log2(delta / 2)) for k in names}
    print(json.dumps(line))
    bs.close()
    ctx.device_free(keys["d_bsk"])
    ctx.device_free(keys["d_ksk"])
    ctx.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--p", type=int, default=2)
    ap.add_argument("--n8", action="store_true")
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--rotation", action="store_true")
    ap.add_argument("--log-slots", type=int, default=0)
    ap.add_argument("--seed", type=lambda v: int(v, 0), default=0x5EED0728)
    a = ap.parse_args()
    N, n = (8, 6) if a.n8 else (1024, 728)
    if a.count < 1 or a.count > 1 << 24 or a.batch < 1:
        ap.error("count must be 1 .. 2^24, batch at least 1")
    ctx = vpbs_amd.Context(0, log_n_max=16)
    if a.rotation:
        return rotation_survey(a, ctx, N, n)
    keys = ctx.keygen_device(N, K, ELL, LOGB, n, a.seed, SIGMA_GLWE, SIGMA_LWE)
    table = [(m + 1) % a.p for m in range(a.p)]
    testv, delta = api.lut_testv(N, a.p, table)
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, a.p, size=a.count, dtype=np.uint64)
    want = np.array(table, np.uint64)[msgs]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()
    d_key, d_tv = dev(keys["s_lwe"]), dev(testv)
    d_plain, d_msgs, d_want = dev(msgs * np.uint64(delta)), dev(msgs), dev(want)
    batch = min(a.batch, a.count)
    d_in = torch.zeros((batch, n + 1), dtype=torch.int64, device="cuda")
    d_out = torch.zeros((batch, n + 1), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bs = api.Bootstrapper(ctx, keys["d_bsk"], keys["d_ksk"], K, ELL, LOGB, max_batch=batch, N=N, n_lwe=n, keys_on_device=True)
    st_in, st_out = api.NoiseStats(), api.NoiseStats()
    seconds = {"encrypt": 0.0, "bootstrap": 0.0, "decode": 0.0}
    decoded = np.zeros(a.count, np.uint64)

    def chunk(lo, hi, timed):
        t0 = time.perf_counter()
        ctx.lwe_encrypt_batch(keys["params"], d_key.data_ptr(), d_plain.data_ptr() + 8 * lo, nonce0=lo, out_dev_ptr=d_in.data_ptr(), count=hi - lo)
        t1 = time.perf_counter()
        bs.run_device(d_in.data_ptr(), hi - lo, d_tv.data_ptr(), d_lwe_out=d_out.data_ptr())
        t2 = time.perf_counter()
        if a.baseline:
            # the parent's way: 8 (n + 1) bytes per ciphertext to the host, one ctypes call per ciphertext, the float rounding
            rows = d_out[:hi - lo].cpu().numpy().view(np.uint64)
            phases = api.lwe_decrypt(keys["s_lwe"], rows)
            got = np.array([int(round(int(ph) / delta)) % (2 * a.p) for ph in phases], np.uint64)
            t3 = time.perf_counter()
            dev_msg = ctx.lwe_decode_batch(d_key.data_ptr(), d_out.data_ptr(), delta, 2 * a.p, count=hi - lo, want=("msg",), n_lwe=n)["msg"]
            if timed:
                decoded[lo:hi] = got
                main.equal = main.equal and bool((got == dev_msg).all())
        else:
            got = ctx.lwe_decode_batch(d_key.data_ptr(), d_out.data_ptr(), delta, 2 * a.p, expected=d_want.data_ptr() + 8 * lo, count=hi - lo,
                                       stats=st_out if timed else None, want=("msg",), n_lwe=n)["msg"]
            t3 = time.perf_counter()
            ctx.lwe_decode_batch(d_key.data_ptr(), d_in.data_ptr(), delta, 2 * a.p, expected=d_msgs.data_ptr() + 8 * lo, count=hi - lo,
                                 stats=st_in if timed else None, want=(), n_lwe=n)       # the inputs' noise: outside the timed phases
            if timed:
                decoded[lo:hi] = got
        if timed:
            for k, dt in zip(("encrypt", "bootstrap", "decode"), (t1 - t0, t2 - t1, t3 - t2)):
                seconds[k] += dt

    main.equal = True
    chunk(0, min(batch, 64), timed=False)                  # warm-up: code objects, the pool's buffers
    for lo in range(0, a.count, batch):
        chunk(lo, min(lo + batch, a.count), timed=True)
    line = {"tool": "noise_survey", "leg": "baseline" if a.baseline else "device", "N": N, "n_lwe": n, "p": a.p, "count": a.count, "batch": batch,
            "seed": a.seed, "delta": delta, "seconds": seconds, "bootstraps_per_second": a.count / seconds["bootstrap"],
            "decode_bytes_read": a.count * (n + 1) * 8,
            "wrong_messages": int((decoded != want).sum())}
    if a.baseline:
        line["all_equal"] = main.equal
    else:
        line["input_noise"], line["output_noise"] = noise_figures(st_in, delta), noise_figures(st_out, delta)
        line["failures"] = st_out.failures
    print(json.dumps(line))
    bs.close()
    ctx.device_free(keys["d_bsk"])
    ctx.device_free(keys["d_ksk"])
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
