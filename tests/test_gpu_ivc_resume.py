"""GPU tests (-m gpu): checkpoints of a running IVC chain (vpbs_ivc_set_checkpoint) and resuming a chain from one (vpbs_ivc_resume_pbs).
A checkpoint is the serialised last proof of a prefix of the chain; a resumed chain must end in exactly the bytes of an uninterrupted one
(the proofs are deterministic), in the host pipeline and in the device-witness pipeline, and a checkpoint that does not verify against the
object's verifier data, the keys and the ciphertext never yields a proof."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import export_circuits
import tfhe_oracle as T
import vpbs_amd
from vpbs_amd import api, circuit_file

pytestmark = pytest.mark.gpu
P = api.P
K, ELL, LOGB = 2, 4, 5
NCOLS = lambda cyc: [cyc.n_constants + 80, 135, 20, 16]


def load(N, n_lwe, log_n):
    return [circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, n_lwe, log_n)]


def test_resume_ends_in_the_golden_chain():
    """the N = 8, n = 1 chain of the CPU oracle: a prefix of k = 1, 2, 3 steps, then resume_pbs -> the frozen bytes, in the host pipeline and
    with the early phases on the device (late phase on the host and on the device)"""
    from test_cyclic_cpu import GOLDEN_CHAIN, n8_chain_inputs
    N, n_lwe, log_n = 8, 1, 13
    ring, (s_to, s_lwe, s_glwe, bsk, ksk), delta, testv, ct = n8_chain_inputs()
    cyc, dum = load(N, n_lwe, log_n)
    frozen = json.load(open(GOLDEN_CHAIN))
    c = vpbs_amd.Context(0, log_n_max=16)
    ivc = api.Ivc(c, cyc, dum, N, K, K * ELL * K * N)
    bsk_flat, ksk_flat = np.stack([T.flatten_ggsw(g) for g in bsk]), T.flatten_ggsw(ksk)
    for pipeline in (None, False, True):
        ivc.set_device_witness(ELL, LOGB, 2 if pipeline is not None else 0, bool(pipeline))
        for k in (1, 2, 3):
            prefix, _ = ivc.prove_pbs(testv, ct, bsk_flat, ksk_flat, k)
            blob, t = ivc.resume_pbs(prefix, testv, ct, bsk_flat, ksk_flat)
            assert (len(blob), hashlib.sha256(blob).hexdigest()) == (frozen["bytes"], frozen["sha256"]), (pipeline, k)
            assert t["steps"] == n_lwe + 2 - k and t["base_proof_ms"] == 0
    ivc.free()
    c.close()


@pytest.fixture(scope="module")
def n6():
    """an n = 6 chain (8 steps) at N = 8, its keys and ciphertext, and verify_pbs of a whole chain's proof"""
    N, n_lwe, log_n = 8, 6, 13
    cyc, dum = load(N, n_lwe, log_n)
    c = vpbs_amd.Context(0, log_n_max=16)
    ivc = api.Ivc(c, cyc, dum, N, K, K * ELL * K * N)
    keys = c.keygen(N, K, ELL, LOGB, n_lwe, 77, 4.99027217501041e-8, 1.17021618159313e-5)
    testv, delta = api.testv(N, 2)
    ct = api.lwe_encrypt(keys["params"], keys["s_lwe"], delta % P)
    vk, _ = ivc.verifier_data()
    acc_init = np.concatenate([np.zeros((K - 1, N), np.uint64), np.asarray(testv, np.uint64).reshape(1, N)])
    out_ct = c.pbs_accumulator_chain(acc_init, ct, keys["bsk"], keys["ksk"], K, ELL, LOGB)[-1]

    def verify(blob):
        return api.verify_pbs(blob, vk[4:].reshape(-1, 4), NCOLS(cyc), vk[:4], log_n, cyc.n_constants, 80, cyc.gates, N, K, testv, ct,
                              keys["bsk"], keys["ksk"], out_ct)
    args = (testv, ct, keys["bsk"], keys["ksk"])
    whole, _ = ivc.prove_pbs(*args)
    yield dict(c=c, ivc=ivc, keys=keys, testv=testv, ct=ct, args=args, whole=whole, verify=verify, N=N, n_lwe=n_lwe, log_n=log_n,
               cyc=cyc, dum=dum, delta=delta)
    ivc.free()
    c.close()


def test_checkpoints_are_prefix_proofs_and_resume_points(n6):
    ivc, args, whole = n6["ivc"], n6["args"], n6["whole"]
    assert n6["verify"](whole) == (True, "")
    for pipeline in ((0, False, False), (3, False, False), (3, True, True)):   # host; device early phase; device late phase + witness checks
        batch, late, check = pipeline
        ivc.set_device_witness(ELL, LOGB, batch, late)
        ivc.set_check_witness(check)
        got = {}
        ivc.on_checkpoint(3, lambda done, b: got.__setitem__(done, b))
        final, _ = ivc.prove_pbs(*args)
        ivc.on_checkpoint(0, None)
        assert sorted(got) == [3, 6] and final == whole, pipeline
        for k in (3, 6):
            assert got[k] == ivc.prove_pbs(*args, steps=k)[0], (pipeline, k)
            blob, t = ivc.resume_pbs(got[k], *args)
            assert blob == whole and t["steps"] == 8 - k, (pipeline, k)
        if check:
            # the whole chain (base + 8), then per k: the prefix (base + k) and the resumed steps only (8 - k)
            assert ivc.witness_checks() == (9 + 4 + 5 + 7 + 2, 0)
        ivc.set_check_witness(False)
    ivc.set_device_witness(ELL, LOGB, 0)
    # resuming from 3 fires the checkpoint at 6 (not at the last step) and the step hook sees 4 .. 8
    cp3 = got[3]
    got2, seen = {}, []
    ivc.on_checkpoint(3, lambda done, b: got2.__setitem__(done, b))
    ivc.on_step(seen.append)
    blob, _ = ivc.resume_pbs(cp3, *args)
    ivc.on_checkpoint(0, None)
    ivc.on_step(None)
    assert blob == whole and n6["verify"](blob) == (True, "")
    assert seen == [4, 5, 6, 7, 8] and sorted(got2) == [6] and got2[6] == got[6]
    # steps == k returns the checkpoint; a shorter resume gives the prefix proof
    assert ivc.resume_pbs(got[6], *args, steps=6)[0] == got[6]
    assert ivc.resume_pbs(cp3, *args, steps=5)[0] == ivc.prove_pbs(*args, steps=5)[0]
    # an exception in the checkpoint hook is re-raised by the call
    ivc.on_checkpoint(2, lambda done, b: 1 / 0)
    with pytest.raises(ZeroDivisionError):
        ivc.prove_pbs(*args, steps=4)
    ivc.on_checkpoint(0, None)


def test_refused_checkpoints_yield_no_proof(n6):
    ivc, args, c = n6["ivc"], n6["args"], n6["c"]
    testv, ct, bsk, ksk = args
    cp3, _ = ivc.prove_pbs(*args, steps=3)
    cp6, _ = ivc.prove_pbs(*args, steps=6)
    other_ct = api.lwe_encrypt(n6["keys"]["params"], n6["keys"]["s_lwe"], 0, nonce=1)
    other = c.keygen(n6["N"], K, ELL, LOGB, n6["n_lwe"], 78, 4.99027217501041e-8, 1.17021618159313e-5)

    def refused(cp, match, testv=testv, ct=ct, bsk=bsk, ksk=ksk, steps=0):
        with pytest.raises(api.VpbsError, match=match):
            ivc.resume_pbs(cp, testv, ct, bsk, ksk, steps)
    refused(cp3, "checkpoint: the LWE hash chain does not match", ct=other_ct)
    refused(cp3, "checkpoint: the key hash chain does not match", bsk=other["bsk"], ksk=other["ksk"])
    b = bytearray(cp3)
    w = int.from_bytes(b[40:48], "little")
    b[40:48] = ((w + 1) % P).to_bytes(8, "little")               # a proof word, still a canonical field element
    refused(bytes(b), "checkpoint: the proof does not verify")
    refused(cp3[:-8], "checkpoint: the bytes are not a proof of this circuit")
    refused(cp6, r"checkpoint: its counter 6 is beyond the requested 3 steps", steps=3)
    # a checkpoint of a chain of another n_lwe (another cyclic circuit at the same N): never taken for one of this chain
    cyc1, dum1 = load(n6["N"], 1, n6["log_n"])
    c1 = vpbs_amd.Context(0, log_n_max=16)
    ivc1 = api.Ivc(c1, cyc1, dum1, n6["N"], K, K * ELL * K * n6["N"])
    keys1 = c1.keygen(n6["N"], K, ELL, LOGB, 1, 77, 4.99027217501041e-8, 1.17021618159313e-5)
    ct1 = api.lwe_encrypt(keys1["params"], keys1["s_lwe"], n6["delta"] % P)
    cp_other, _ = ivc1.prove_pbs(testv, ct1, keys1["bsk"], keys1["ksk"], 2)
    ivc1.free()
    c1.close()
    refused(cp_other, "checkpoint: ")
    # ... after which the same object resumes as before
    assert ivc.resume_pbs(cp3, *args)[0] == n6["whole"]


def test_a_sharded_chain_refuses_resume():
    from test_cyclic_cpu import n8_chain_inputs
    from vpbs_amd import sharding
    if not api.lib().vpbs_rccl_available():
        pytest.skip("librccl.so is not loadable here")
    N, n_lwe, log_n = 8, 1, 13
    ring, (s_to, s_lwe, s_glwe, bsk, ksk), delta, testv, ct = n8_chain_inputs()
    cyc, dum = load(N, n_lwe, log_n)
    c = vpbs_amd.Context(0, log_n_max=16)
    bsk_flat, ksk_flat = np.stack([T.flatten_ggsw(g) for g in bsk]), T.flatten_ggsw(ksk)
    plain = api.Ivc(c, cyc, dum, N, K, K * ELL * K * N)
    cp, _ = plain.prove_pbs(testv, ct, bsk_flat, ksk_flat, 1)
    plain.free()
    comm = sharding.make_comm_rccl(c, stage_words=2 << (log_n + 3))
    ivc = api.Ivc(c, cyc, dum, N, K, K * ELL * K * N, comm)
    with pytest.raises(api.VpbsError, match="not available for a sharded chain"):
        ivc.resume_pbs(cp, testv, ct, bsk_flat, ksk_flat)
    ivc.free()
    sharding.free_comm_rccl(comm)
    c.close()


def test_resume_at_the_papers_parameters():
    """N = 1024, n = 728, degree 2^16: a 7-step prefix resumed to 14 steps is prove_pbs(steps = 14), in the host pipeline and in the
    device-witness pipeline (batch 3, witnesses checked); a 726-step prefix resumed to the end passes the tool's checks of a whole chain
    (verify_pbs, decryption to the message)"""
    import __graft_entry__ as entry
    sys.path.insert(0, os.path.join(entry.ROOT, "tools"))
    import prove_ivc
    N, n_lwe, log_n = 1024, 728, 16
    cyc, dum = load(N, n_lwe, log_n)
    c = vpbs_amd.Context(0, log_n_max=16)
    ivc = api.Ivc(c, cyc, dum, N, K, K * ELL * K * N)
    keys = c.keygen(N, K, ELL, LOGB, n_lwe, 5, 4.99027217501041e-8, 1.17021618159313e-5)
    tv, delta = api.testv(N, 2)
    ct = api.lwe_encrypt(keys["params"], keys["s_lwe"], delta % P)
    args = (tv, ct, keys["bsk"], keys["ksk"])
    vk, _ = ivc.verifier_data()
    want = None
    for batch, check in ((0, False), (3, True)):
        ivc.set_device_witness(ELL, LOGB, batch)
        ivc.set_check_witness(check)
        cp7, _ = ivc.prove_pbs(*args, steps=7)
        blob, t = ivc.resume_pbs(cp7, *args, steps=14)
        want = want or ivc.prove_pbs(*args, steps=14)[0]
        assert blob == want and t["steps"] == 7, batch
        if check:
            assert ivc.witness_checks() == (1 + 7 + 7, 0)    # the prefix (base + 7), the resumed steps
        ivc.set_check_witness(False)
    ivc.set_device_witness(ELL, LOGB, 0)
    cp726, _ = ivc.prove_pbs(*args, steps=726)
    blob, t = ivc.resume_pbs(cp726, *args)
    assert t["steps"] == 4
    _, decrypted = prove_ivc.check_chain(c, cyc, vk, blob, keys, tv, delta, ct, N, n_lwe, log_n, n_lwe + 2, 1)
    assert decrypted == 1
    ivc.free()
    c.close()


def test_prove_ivc_tool_checkpoints_and_resumes(tmp_path):
    import __graft_entry__ as entry
    export_circuits.ensure_cyclic_circuit(8, K, ELL, LOGB, 6, 13)
    tool = [sys.executable, os.path.join(entry.ROOT, "tools", "prove_ivc.py"), "8", "6", "13"]

    def run(**env):
        r = subprocess.run(tool, capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])
    a = run(VPBS_IVC_CHECKPOINT="%s:3" % tmp_path)
    assert a["checkpoints_written"] == [2] and a["resumed_from"] is None and a["decrypted"] == a["message"] == 1
    assert sorted(os.listdir(tmp_path)) == ["chain0_step3.bin", "chain0_step6.bin"]
    b = run(VPBS_IVC_RESUME=str(tmp_path / "chain0_step3.bin"))
    assert b["resumed_from"] == 3 and b["decrypted"] == 1 and b["proof_sha256"] == a["proof_sha256"]
