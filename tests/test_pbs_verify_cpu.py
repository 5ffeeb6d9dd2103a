"""CPU side of the batch verifier of whole vPBS proofs (csrc/verify_pbs_batch.hip): the host key hash it is created with, and its reason
texts, which must be exactly the `why` vpbs_verify_pbs writes when each of its checks fails.  The proofs are the CPU oracle's N = 8 chain of
tests/test_cyclic_cpu.py (its helpers, imported as they are)."""
import numpy as np
import pytest

import cyclic_circuit as cc
import oracle as orc
import step_oracle
import tfhe_oracle as T
from cyclic_circuit import P
from test_cyclic_cpu import OracleProver, n8_chain_inputs, run_chain
from vpbs_amd import api


def test_key_hash_is_the_hash_chain_over_zero_bsk_ksk():
    rng = np.random.default_rng(3)
    for n_lwe, g in ((3, 64), (1, 8), (0, 16), (5, 128)):
        bsk = rng.integers(0, P, size=(n_lwe, g), dtype=np.uint64)
        ksk = rng.integers(0, P, size=g, dtype=np.uint64)
        want, _ = api.hash_chain(np.vstack([np.zeros((1, g), np.uint64), bsk, ksk.reshape(1, g)]))
        assert api.pbs_key_hash(bsk, ksk).tolist() == want.tolist()
    with pytest.raises(api.VpbsError):
        api.pbs_key_hash(np.zeros((1, 0), np.uint64), np.zeros(0, np.uint64))


@pytest.mark.parametrize("n_lwe", [0, 1, 6])
@pytest.mark.parametrize("ggsw_len", [64, 65])
def test_key_hash_is_the_last_link_of_the_public_walker(n_lwe, ggsw_len):
    """the key-links function the batch provers and vpbs_pbs_key_hash share (vpbs::key_hash_links) against vpbs_hash_chain_links over the
    same items from a zero prefix, at item lengths on both sides of a sponge block (64 = 8 blocks of rate 8, 65 = one element more)"""
    rng = np.random.default_rng(1000 * n_lwe + ggsw_len)
    bsk = rng.integers(0, P, size=(n_lwe, ggsw_len), dtype=np.uint64)
    ksk = rng.integers(0, P, size=ggsw_len, dtype=np.uint64)
    links = api.hash_chain_links(np.zeros(4, np.uint64), np.vstack([np.zeros((1, ggsw_len), np.uint64), bsk, ksk.reshape(1, ggsw_len)]))
    assert links.shape == (n_lwe + 2, 4)
    assert api.pbs_key_hash(bsk, ksk).tolist() == links[-1].tolist()


def test_reason_codes_and_texts():
    assert [api.PBS_OK, api.PBS_MALFORMED, api.PBS_TESTV_MASK, api.PBS_TESTV, api.PBS_COUNTER, api.PBS_OUT_CT, api.PBS_PROOF,
            api.PBS_VERIFIER_DATA, api.PBS_KEY_HASH, api.PBS_LWE_HASH] == list(range(10))
    texts = [api.pbs_reason_text(r) for r in range(10)]
    assert texts[0] == "" and len(set(texts)) == 10
    with pytest.raises(ValueError):
        api.pbs_reason_text(10)


def test_reason_texts_are_the_host_verifiers_why():
    """each check of vpbs_verify_pbs failing in turn on the last proof of the oracle's N = 8, n = 1 chain: its `why` is pbs_reason_text"""
    N, K, ELL, LOGB, n_lwe, log_n = 8, 2, 4, 5, 1, 13
    cy = cc.CyclicStepCircuit(api, N, K, ELL, LOGB, n_lwe, orc.negacyclic_params(3), log_n)
    dm = cc.DummyCircuit(api, log_n, cy.shape.n_pi)
    C, D = OracleProver(cy.built), OracleProver(dm.built)
    ring, (s_to, s_lwe, s_glwe, bsk, ksk), delta, testv, ct = n8_chain_inputs()
    acc_init = [[0] * N for _ in range(K - 1)] + [testv]
    keys = (s_to, s_lwe, s_glwe, [T.flatten_ggsw(g) for g in bsk], T.flatten_ggsw(ksk))
    proof, pis = run_chain(cy, dm, C, D, C.prove, D.prove, keys, ct, acc_init, check=False)[-1]
    kn = K * N
    blob = step_oracle.to_bytes(proof, proof["ncols"], C.nconst, pis, log_n)
    bsk_flat, ksk_flat, out_ct = np.stack(keys[3]), keys[4], pis[kn + 1:2 * kn + 1]
    assert api.pbs_key_hash(bsk_flat, ksk_flat).tolist() == [int(v) for v in pis[2 * kn + 1:2 * kn + 5]]
    pi_at = len(blob) - 8 * pis.size

    def vp(blob=blob, testv=testv, ct=ct, out_ct=out_ct, prover=C, ncols=proof["ncols"]):
        return api.verify_pbs(blob, prover.cap, ncols, prover.vk[:4], log_n, prover.nconst, 80, prover.ps, N, K, testv, ct, bsk_flat, ksk_flat,
                              out_ct=out_ct)

    def pi_word(j, value):
        b = bytearray(blob)
        b[pi_at + 8 * j:pi_at + 8 * j + 8] = int(value).to_bytes(8, "little")
        return bytes(b)
    flip = lambda a, i: np.array([int(v) ^ (k == i) for k, v in enumerate(np.asarray(a, np.uint64).reshape(-1))], np.uint64)
    assert vp() == (True, api.pbs_reason_text(api.PBS_OK))
    failing = {api.PBS_MALFORMED: vp(blob=blob[:-8]),
               api.PBS_TESTV_MASK: vp(blob=pi_word(0, 1)),
               api.PBS_TESTV: vp(testv=flip(testv, 3)),
               api.PBS_COUNTER: vp(blob=pi_word(kn, n_lwe + 1)),
               api.PBS_OUT_CT: vp(out_ct=flip(out_ct, 5)),
               api.PBS_PROOF: vp(blob=pi_word(2 * kn + 1, int(pis[2 * kn + 1]) ^ 1)),
               api.PBS_LWE_HASH: vp(ct=flip(ct, 1))}
    # the key hash: another key set's (the verifier holds the hash of the keys it is given)
    failing[api.PBS_KEY_HASH] = api.verify_pbs(blob, C.cap, proof["ncols"], C.vk[:4], log_n, C.nconst, 80, C.ps, N, K, testv, ct, bsk_flat,
                                               flip(ksk_flat, 7), out_ct=out_ct)
    # another circuit's verifier data in a proof that verifies: the dummy circuit proves any public inputs, these carry the cyclic circuit's
    d_proof = D.prove(dm.witness(pis), pis)
    failing[api.PBS_VERIFIER_DATA] = vp(blob=step_oracle.to_bytes(d_proof, d_proof["ncols"], D.nconst, pis, log_n), prover=D,
                                        ncols=d_proof["ncols"])
    for reason, (ok, why) in failing.items():
        assert not ok and why == api.pbs_reason_text(reason), (reason, why)
