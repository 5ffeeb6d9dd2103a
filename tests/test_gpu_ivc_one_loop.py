"""GPU tests (-m gpu): the parts of the IVC driver's one chain loop (csrc/ivc.hip, ChainRun) that the byte-parity tests never reach -- its
tail (an output buffer that is too small must leave no thread, state or buffer behind in any source of staged steps) and its bookkeeping
(what every field of vpbs_ivc_timing means per pipeline; step hook before checkpoint, on the proving thread).  N = 8 circuits at degree
2^13: a chain of n = 1 is three step proofs, one of n = 6 eight."""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest

import export_circuits
import tfhe_oracle as T
import vpbs_amd
from vpbs_amd import api, circuit_file

pytestmark = pytest.mark.gpu
P = api.P
N, K, ELL, LOGB, LOG_N = 8, 2, 4, 5, 13
# (batch, late_on_device) of set_device_witness: the host pipeline, the early phases on the device, the late phase there as well
HOST, DEVICE_EARLY, DEVICE_LATE = (0, False), (2, False), (2, True)


def load(n_lwe):
    return [circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, n_lwe, LOG_N)]


def test_a_too_small_output_buffer_leaves_nothing_behind():
    """capacity = 16 bytes: VPBS_ERR_INVALID with the tail's message after the whole chain ran; the next call on the SAME object returns the
    golden bytes -- per pipeline, in the order host, device early, device late"""
    from test_cyclic_cpu import GOLDEN_CHAIN, n8_chain_inputs
    ring, (s_to, s_lwe, s_glwe, bsk, ksk), delta, testv, ct = n8_chain_inputs()
    cyc, dum = load(1)
    frozen = json.load(open(GOLDEN_CHAIN))
    c = vpbs_amd.Context(0, log_n_max=16)
    ivc = api.Ivc(c, cyc, dum, N, K, K * ELL * K * N)
    bsk_flat, ksk_flat = np.stack([T.flatten_ggsw(g) for g in bsk]), T.flatten_ggsw(ksk)
    tv, cw, bs, ks = (api._u64(a).reshape(-1) for a in (testv, ct, bsk_flat, ksk_flat))
    for batch, late in (HOST, DEVICE_EARLY, DEVICE_LATE):
        ivc.set_device_witness(ELL, LOGB, batch, late)
        buf, t, err = (C.c_uint8 * 16)(), api.IvcTimingC(), C.create_string_buffer(512)
        rc = api.lib().vpbs_ivc_prove_pbs(ivc.h, api._ptr(tv), api._ptr(cw), api._ptr(bs), api._ptr(ks), cw.size - 1, 0, buf, 16, C.byref(t),
                                          err, 512)
        assert rc == api.ERR_INVALID and err.value.decode() == "the output buffer is too small for the proof", (batch, late, rc, err.value)
        blob, _ = ivc.prove_pbs(testv, ct, bsk_flat, ksk_flat)
        assert (len(blob), hashlib.sha256(blob).hexdigest()) == (frozen["bytes"], frozen["sha256"]), (batch, late)
    ivc.free()
    c.close()


@pytest.fixture(scope="module")
def n6():
    """an n = 6 chain (8 steps), its keys and ciphertext, on one object for the tests below"""
    n_lwe = 6
    cyc, dum = load(n_lwe)
    c = vpbs_amd.Context(0, log_n_max=16)
    ivc = api.Ivc(c, cyc, dum, N, K, K * ELL * K * N)
    keys = c.keygen(N, K, ELL, LOGB, n_lwe, 77, 4.99027217501041e-8, 1.17021618159313e-5)
    testv, delta = api.testv(N, 2)
    ct = api.lwe_encrypt(keys["params"], keys["s_lwe"], delta % P)
    yield dict(ivc=ivc, cyc=cyc, testv=testv, ct=ct, keys=keys, args=(testv, ct, keys["bsk"], keys["ksk"]))
    ivc.free()
    c.close()


@pytest.mark.parametrize("pipeline", [HOST, DEVICE_EARLY, DEVICE_LATE], ids=["host", "device-early", "device-late"])
def test_timing_keeps_its_meaning(n6, pipeline):
    ivc, args = n6["ivc"], n6["args"]
    ivc.set_device_witness(ELL, LOGB, *pipeline)
    got = {}
    ivc.on_checkpoint(3, lambda done, b: got.setdefault(done, b))
    whole, t = ivc.prove_pbs(*args)
    ivc.on_checkpoint(0, None)
    print(pipeline, "prove_pbs", t)
    assert t["steps"] == 8 and t["base_proof_ms"] > 0
    assert t["late_witness_ms"] > 0 and t["prove_step_ms"] > 0 and t["early_witness_ms"] > 0
    blob, r = ivc.resume_pbs(got[3], *args)
    print(pipeline, "resume_pbs", r)
    assert blob == whole
    assert r["steps"] == 8 - 3 and r["base_proof_ms"] == 0
    assert r["late_witness_ms"] > 0 and r["prove_step_ms"] > 0 and r["early_witness_ms"] > 0
    ivc.set_device_witness(ELL, LOGB, 0)


@pytest.mark.parametrize("pipeline", [HOST, DEVICE_EARLY], ids=["host", "device-early"])
def test_callbacks_keep_their_order(n6, pipeline):
    ivc, args, cyc, keys = n6["ivc"], n6["args"], n6["cyc"], n6["keys"]
    ivc.set_device_witness(ELL, LOGB, *pipeline)
    events, blobs = [], {}
    ivc.on_step(lambda done: events.append(("step", done)))
    ivc.on_checkpoint(2, lambda done, b: (events.append(("checkpoint", done)), blobs.__setitem__(done, b)))
    ivc.prove_pbs(*args)
    ivc.on_checkpoint(0, None)
    ivc.on_step(None)
    ivc.set_device_witness(ELL, LOGB, 0)
    last = 6 + 2
    assert [d for what, d in events if what == "step"] == list(range(last + 1))
    assert [d for what, d in events if what == "checkpoint"] == [2, 4, 6]
    for done in (2, 4, 6):   # on one thread, the step hook first
        assert events.index(("checkpoint", done)) == events.index(("step", done)) + 1
    vk, _ = ivc.verifier_data()
    for done, b in blobs.items():
        assert api.verify_pbs_prefix(b, vk[4:].reshape(-1, 4), [cyc.n_constants + 80, 135, 20, 16], vk[:4], LOG_N, cyc.n_constants, 80,
                                     cyc.gates, N, K, n6["testv"], n6["ct"], keys["bsk"], keys["ksk"]) == (True, done, "")
