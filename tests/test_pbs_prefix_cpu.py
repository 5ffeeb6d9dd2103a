"""The prefix form of verify_pbs (vpbs_verify_pbs_prefix, csrc/verifier.hip): its checks on the last proof of a chain of k = counter proofs --
a checkpoint of the chain, what vpbs_ivc_resume_pbs takes -- on every step proof of the CPU oracle's N = 8, n = 1 chain (tests/test_cyclic_cpu.py,
its helpers imported as they are; serialised with step_oracle.to_bytes as in tests/test_pbs_verify_cpu.py)."""
import numpy as np
import pytest

import cyclic_circuit as cc
import oracle as orc
import step_oracle
import tfhe_oracle as T
from test_cyclic_cpu import OracleProver, n8_chain_inputs, run_chain
from vpbs_amd import api

N, K, ELL, LOGB, n_lwe, log_n = 8, 2, 4, 5, 1, 13
KN = K * N


@pytest.fixture(scope="module")
def chain():
    cy = cc.CyclicStepCircuit(api, N, K, ELL, LOGB, n_lwe, orc.negacyclic_params(3), log_n)
    dm = cc.DummyCircuit(api, log_n, cy.shape.n_pi)
    C, D = OracleProver(cy.built), OracleProver(dm.built)
    ring, (s_to, s_lwe, s_glwe, bsk, ksk), delta, testv, ct = n8_chain_inputs()
    acc_init = [[0] * N for _ in range(K - 1)] + [testv]
    keys = (s_to, s_lwe, s_glwe, [T.flatten_ggsw(g) for g in bsk], T.flatten_ggsw(ksk))
    steps = run_chain(cy, dm, C, D, C.prove, D.prove, keys, ct, acc_init, check=False)
    blobs = [step_oracle.to_bytes(proof, proof["ncols"], C.nconst, pis, log_n) for proof, pis in steps]
    return dict(C=C, D=D, dm=dm, steps=steps, blobs=blobs, testv=testv, ct=ct, bsk=np.stack(keys[3]), ksk=keys[4])


def prefix(ch, blob, testv=None, ct=None, bsk=None, ksk=None, out_ct=None, prover=None, ncols=None):
    P_ = prover or ch["C"]
    return api.verify_pbs_prefix(blob, P_.cap, ncols or ch["steps"][-1][0]["ncols"], P_.vk[:4], log_n, P_.nconst, 80, P_.ps, N, K,
                                 ch["testv"] if testv is None else testv, ch["ct"] if ct is None else ct,
                                 ch["bsk"] if bsk is None else bsk, ch["ksk"] if ksk is None else ksk, out_ct=out_ct)


def whole(ch, blob, testv=None, ct=None, bsk=None, ksk=None, out_ct=None):
    C = ch["C"]
    return api.verify_pbs(blob, C.cap, ch["steps"][-1][0]["ncols"], C.vk[:4], log_n, C.nconst, 80, C.ps, N, K,
                          ch["testv"] if testv is None else testv, ch["ct"] if ct is None else ct,
                          ch["bsk"] if bsk is None else bsk, ch["ksk"] if ksk is None else ksk, out_ct)


def pi_word(blob, n_pi, j, value):
    b = bytearray(blob)
    at = len(blob) - 8 * n_pi + 8 * j
    b[at:at + 8] = int(value).to_bytes(8, "little")
    return bytes(b)


def flip(a, i):
    return np.array([int(v) ^ (k == i) for k, v in enumerate(np.asarray(a, np.uint64).reshape(-1))], np.uint64).reshape(np.shape(a))


def test_every_step_proof_is_a_checkpoint(chain):
    """each of the n + 2 = 3 step proofs is accepted with steps_done = its counter, with and without the output ciphertext"""
    assert len(chain["blobs"]) == n_lwe + 2
    for k, (blob, (_, pis)) in enumerate(zip(chain["blobs"], chain["steps"]), start=1):
        assert int(pis[KN]) == k
        assert prefix(chain, blob) == (True, k, "")
        assert prefix(chain, blob, out_ct=pis[KN + 1:2 * KN + 1]) == (True, k, "")


def test_the_last_proof_gets_verify_pbs_verdict_and_why(chain):
    """k = n + 2 with out_ct given: the prefix form's verdict and why are vpbs_verify_pbs's, accepted or refused"""
    blob, (_, pis) = chain["blobs"][-1], chain["steps"][-1]
    out_ct = pis[KN + 1:2 * KN + 1]
    n_pi = pis.size
    cases = [dict(), dict(ct=flip(chain["ct"], 1)), dict(ksk=flip(chain["ksk"], 7)), dict(out_ct=flip(out_ct, 5)),
             dict(testv=flip(chain["testv"], 3)), dict(blob=blob[:-8]), dict(blob=pi_word(blob, n_pi, 0, 1)),
             dict(blob=pi_word(blob, n_pi, 2 * KN + 1, int(pis[2 * KN + 1]) ^ 1))]
    for case in cases:
        args = dict(out_ct=out_ct)
        args.update(case)
        b = args.pop("blob", blob)
        ok, done, why = prefix(chain, b, **args)
        assert (ok, why) == whole(chain, b, **args), case
        assert done == (n_lwe + 2 if ok else 0)


def test_each_check_failing_in_turn(chain):
    blobs, steps = chain["blobs"], chain["steps"]
    last, (_, pis) = blobs[-1], steps[-1]
    n_pi = pis.size
    refused = lambda r: (r[0], r[2])
    counter = "the counter is not in 1 .. n + 2"
    assert refused(prefix(chain, pi_word(last, n_pi, KN, 0))) == (False, counter)
    assert refused(prefix(chain, pi_word(last, n_pi, KN, n_lwe + 3))) == (False, counter)
    assert refused(prefix(chain, pi_word(last, n_pi, 0, 1))) == (False, api.pbs_reason_text(api.PBS_TESTV_MASK))
    assert refused(prefix(chain, last, testv=flip(chain["testv"], 3))) == (False, api.pbs_reason_text(api.PBS_TESTV))
    step2_pis = steps[1][1]
    assert refused(prefix(chain, blobs[1], out_ct=flip(step2_pis[KN + 1:2 * KN + 1], 2))) == (False, api.pbs_reason_text(api.PBS_OUT_CT))
    # a tampered public input: the proof no longer verifies (the counter of another prefix, the LWE hash)
    assert refused(prefix(chain, pi_word(blobs[1], n_pi, KN, 1))) == (False, api.pbs_reason_text(api.PBS_PROOF))
    assert refused(prefix(chain, pi_word(last, n_pi, 2 * KN + 5, int(pis[2 * KN + 5]) ^ 1))) == (False, api.pbs_reason_text(api.PBS_PROOF))
    # another circuit's verifier data in a proof that verifies: the dummy circuit proves any public inputs, these carry the cyclic circuit's
    C, D, dm = chain["C"], chain["D"], chain["dm"]
    d_proof = D.prove(dm.witness(step2_pis), step2_pis)
    d_blob = step_oracle.to_bytes(d_proof, d_proof["ncols"], D.nconst, step2_pis, log_n)
    assert refused(prefix(chain, d_blob, prover=D, ncols=d_proof["ncols"])) == (False, api.pbs_reason_text(api.PBS_VERIFIER_DATA))
    # the LWE prefix: another ciphertext, on every prefix (ct[n] is the first mask)
    for blob in blobs:
        assert refused(prefix(chain, blob, ct=flip(chain["ct"], n_lwe))) == (False, api.pbs_reason_text(api.PBS_LWE_HASH))
    assert refused(prefix(chain, blobs[1], ct=flip(chain["ct"], 0))) == (False, api.pbs_reason_text(api.PBS_LWE_HASH))
    assert prefix(chain, blobs[0], ct=flip(chain["ct"], 0)) == (True, 1, "")     # ct[0] is the mask of step 1: not in a prefix of 1
    # the key prefix: ksk enters at k = n + 2 only, bsk_0 from k = 2 on
    key = api.pbs_reason_text(api.PBS_KEY_HASH)
    assert refused(prefix(chain, last, ksk=flip(chain["ksk"], 7))) == (False, key)
    assert prefix(chain, blobs[1], ksk=flip(chain["ksk"], 7)) == (True, 2, "")
    other_bsk = flip(chain["bsk"], 11)
    assert refused(prefix(chain, blobs[1], bsk=other_bsk)) == (False, key)
    assert prefix(chain, blobs[0], bsk=other_bsk) == (True, 1, "")
    # truncated bytes
    for blob in (last[:-8], last[:len(last) // 2], b""):
        assert refused(prefix(chain, blob)) == (False, api.pbs_reason_text(api.PBS_MALFORMED))


def test_malformed_arguments():
    gates = api.GateSet(cc.GATE_SPEC)
    with pytest.raises(api.VpbsError, match="malformed arguments"):
        api.verify_pbs_prefix(b"\0" * 64, np.zeros((16, 4), np.uint64), [10, 135, 20, 16], [0] * 4, log_n, 2, 80, gates, N, K,
                              np.zeros(N, np.uint64), np.zeros(n_lwe + 1, np.uint64), np.zeros((1, 10), np.uint64), np.zeros(10, np.uint64))
