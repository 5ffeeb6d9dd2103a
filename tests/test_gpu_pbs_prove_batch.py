"""GPU tests (-m gpu): api.PbsProver -- the bootstraps of a batch AND their vPBS proofs under one resident key set.  The proofs are
deterministic, so the batch prover must deliver, for every ciphertext and whatever the completion order, exactly the bytes
Ivc.prove_pbs makes of it; its outputs are the Bootstrapper's; the preset matrices its kernels assemble on the device are, word for word,
the numpy statement of tests/preset_layout.py."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import export_circuits
import preset_layout
import tfhe_oracle as T
import vpbs_amd
from vpbs_amd import api, circuit_file

pytestmark = pytest.mark.gpu
P = api.P
K, ELL, LOGB = 2, 4, 5
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)
NCOLS = lambda cyc: [cyc.n_constants + 80, 135, 20, 16]


def load(N, n_lwe, log_n):
    return [circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, n_lwe, log_n)]


def test_the_golden_chain():
    """the N = 8, n = 1 chain of the CPU oracle through the batch prover: the frozen length and sha256"""
    from test_cyclic_cpu import GOLDEN_CHAIN, n8_chain_inputs
    ring, (s_to, s_lwe, s_glwe, bsk, ksk), delta, testv, ct = n8_chain_inputs()
    cyc, dum = load(8, 1, 13)
    frozen = json.load(open(GOLDEN_CHAIN))
    bsk_flat, ksk_flat = np.stack([T.flatten_ggsw(g) for g in bsk]), T.flatten_ggsw(ksk)
    p = api.PbsProver(0, cyc, dum, bsk_flat, ksk_flat, K, ELL, LOGB, chains=1, witness_batch=2)
    proofs, out_ct, lwe_out = p.prove(np.array([ct], np.uint64), np.array(testv, np.uint64))
    p.close()
    assert [(len(b), hashlib.sha256(b).hexdigest()) for b in proofs] == [(frozen["bytes"], frozen["sha256"])]


@pytest.fixture(scope="module")
def n6():
    """N = 8, n = 6 (8 steps): seeded keys, five ciphertexts -- different messages and nonces, one with a mask word at or above p, one with a
    test vector of its own -- and, for each, what the existing paths make of it: Ivc.prove_pbs's bytes and Bootstrapper.run's outputs"""
    N, n_lwe, log_n = 8, 6, 13
    cyc, dum = load(N, n_lwe, log_n)
    c = vpbs_amd.Context(0, log_n_max=16)
    keys = c.keygen(N, K, ELL, LOGB, n_lwe, 77, *SIGMAS)
    tv, delta = api.testv(N, 2)
    msgs = [1, 0, 1, 1, 0]
    cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * m % P, nonce=10 + i) for i, m in enumerate(msgs)])
    cts[2, 3] = np.uint64(P + 5)                                    # a mask word at or above p
    testvs = np.stack([tv] * 5)
    testvs[4] = np.array([(P - int(v)) % P for v in tv], np.uint64)   # a test vector of its own
    ivc = api.Ivc(c, cyc, dum, N, K, K * ELL * K * N)
    want = [ivc.prove_pbs(testvs[i], cts[i], keys["bsk"], keys["ksk"])[0] for i in range(5)]
    vk, _ = ivc.verifier_data()
    bs = api.Bootstrapper(c, keys["bsk"], keys["ksk"], K, ELL, LOGB, max_batch=8)
    out_ct, lwe_out = bs.run(cts, testvs)
    bs.close()
    yield dict(c=c, ivc=ivc, cyc=cyc, dum=dum, keys=keys, cts=cts, testvs=testvs, tv=tv, delta=delta, msgs=msgs, want=want, vk=vk, out_ct=out_ct,
               lwe_out=lwe_out, N=N, n_lwe=n_lwe, log_n=log_n)
    ivc.free()
    c.close()


@pytest.mark.parametrize("chains", [1, 2, 3])
@pytest.mark.parametrize("witness_batch", [1, 3, 8])
def test_byte_parity_with_the_existing_path(n6, chains, witness_batch):
    S = n6
    keys, cyc, vk = S["keys"], S["cyc"], S["vk"]
    p = api.PbsProver(0, cyc, S["dum"], keys["bsk"], keys["ksk"], K, ELL, LOGB, chains=chains, witness_batch=witness_batch)
    order = []
    proofs, out_ct, lwe_out = p.prove(S["cts"], S["testvs"], on_proof=lambda i, b: order.append(i))
    kh, (pvk, _) = p.key_hash(), p.verifier_data()
    p.close()
    assert sorted(order) == [0, 1, 2, 3, 4]
    for i in range(5):
        assert proofs[i] == S["want"][i], (i, len(proofs[i]), len(S["want"][i]))
    assert (out_ct == S["out_ct"]).all() and (lwe_out == S["lwe_out"]).all()
    assert (kh == api.pbs_key_hash(keys["bsk"], keys["ksk"])).all() and (pvk == vk).all()
    cap = vk[4:].reshape(-1, 4)
    for i in range(5):
        assert api.verify_pbs(proofs[i], cap, NCOLS(cyc), vk[:4], S["log_n"], cyc.n_constants, 80, cyc.gates, S["N"], K, S["testvs"][i], S["cts"][i],
                              keys["bsk"], keys["ksk"], out_ct[i]) == (True, ""), i
    pv = api.PbsVerifier(S["c"], cap, NCOLS(cyc), vk[:4], S["log_n"], cyc.n_constants, 80, cyc.gates, S["N"], K, S["n_lwe"], K * ELL * K * S["N"], kh,
                         max_batch=5)
    verdicts, reasons, _ = pv.verify(proofs, S["testvs"], S["cts"], out_ct.reshape(5, -1))
    pv.close()
    assert verdicts.tolist() == [1] * 5, [api.pbs_reason_text(int(r)) for r in reasons]


def chain_sources(c, N, n_lwe, keys, ct, tv):
    """every source of the preset table for one chain, from the paths that existed before the batch prover"""
    acc_init = np.concatenate([np.zeros((K - 1, N), np.uint64), np.asarray(tv, np.uint64).reshape(1, N)])
    accs = c.pbs_accumulator_chain(acc_init, ct, keys["bsk"], keys["ksk"], K, ELL, LOGB).reshape(n_lwe + 2, -1)
    g = K * ELL * K * N
    key_links = api.hash_chain_links(np.zeros(4, np.uint64), np.concatenate([np.zeros((1, g), np.uint64), keys["bsk"].reshape(n_lwe, g),
                                                                            keys["ksk"].reshape(1, g)]))
    lwe_links = api.hash_chain_links(np.zeros(4, np.uint64), preset_layout.lwe_masks(ct).reshape(-1, 1))
    return dict(testv=np.asarray(tv, np.uint64), accs=accs, key_links=key_links, lwe_links=lwe_links, ct=np.asarray(ct, np.uint64),
                bsk=keys["bsk"].reshape(n_lwe, g), ksk=keys["ksk"].reshape(-1))


def check_preset_kernel(c, cyc, dum, N, n_lwe, keys, ct, tv, cases):
    ivc = api.Ivc(c, cyc, dum, N, K, K * ELL * K * N)
    cyc_vk, dum_vk = ivc.verifier_data()   # from an Ivc of its own: the verifier data is a function of the circuits
    ivc.free()
    p = api.PbsProver(0, cyc, dum, keys["bsk"], keys["ksk"], K, ELL, LOGB, chains=1, witness_batch=1)
    src = chain_sources(c, N, n_lwe, keys, ct, tv)
    pw, n_pi = cyc.meta["proof_words"], len(cyc.pi_pos)
    # the dummy proof as the prover's vpbs_ivc holds it on the host -- not read back from the matrix under test; it is a proof of the dummy
    # circuit: its first words are the wires cap, which differs from the cap of the constants in the verifier data
    dummy_proof = p.dummy_proof_for_tests()
    assert dummy_proof.size == pw and dummy_proof.any() and (dummy_proof < P).all() and len(cyc.preset_pos) == 2 * (pw + n_pi) + 2 + src["ksk"].size + 136
    for first, cnt in cases:
        got = p.preset_matrix(ct, tv, first, cnt)
        want = preset_layout.matrix(first, cnt, pw, cyc_vk=cyc_vk, dum_vk=dum_vk, dummy_proof=dummy_proof, **src)
        assert got.shape == want.shape == (len(cyc.preset_pos), cnt)
        assert (got == want).all(), (first, cnt, np.argwhere(got != want)[:5])
    p.close()
    return dummy_proof


def test_the_preset_kernel_alone_at_n8(n6):
    """steps [first, first + cnt) for cnt in {1, 2, 7} (n + 2 = 8 steps) with `first` on step 0, a middle step and the key-switch step"""
    S = n6
    check_preset_kernel(S["c"], S["cyc"], S["dum"], S["N"], S["n_lwe"], S["keys"], S["cts"][2], S["testvs"][4],
                        [(0, 1), (0, 2), (0, 7), (0, 8), (3, 1), (3, 2), (1, 7), (7, 1), (6, 2)])


@pytest.fixture(scope="module")
def paper():
    N, n_lwe, log_n = 1024, 728, 16
    cyc, dum = load(N, n_lwe, log_n)
    c = vpbs_amd.Context(0, log_n_max=16)
    keys = c.keygen(N, K, ELL, LOGB, n_lwe, 5, *SIGMAS)
    tv, delta = api.testv(N, 2)
    cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * m % P, nonce=i) for i, m in enumerate([1, 0, 1])])
    yield dict(c=c, cyc=cyc, dum=dum, keys=keys, tv=tv, delta=delta, cts=cts, N=N, n_lwe=n_lwe, log_n=log_n)
    c.close()


def test_the_preset_kernel_alone_at_the_papers_shape(paper):
    S = paper
    check_preset_kernel(S["c"], S["cyc"], S["dum"], S["N"], S["n_lwe"], S["keys"], S["cts"][0], S["tv"],
                        [(0, 1), (0, 2), (0, 7), (0, 64), (300, 1), (300, 2), (300, 7), (300, 64), (729, 1), (728, 2), (723, 7), (666, 64)])


def test_a_prefix_at_the_papers_parameters(paper):
    """N = 1024, n = 728: three ciphertexts on two chains, the first 24 steps of each: the bytes of Ivc.prove_pbs(..., steps=24); the outputs
    are those of the whole bootstrap and decrypt to the messages"""
    S = paper
    keys = S["keys"]
    ivc = api.Ivc(S["c"], S["cyc"], S["dum"], S["N"], K, K * ELL * K * S["N"])
    want = [ivc.prove_pbs(S["tv"], ct, keys["bsk"], keys["ksk"], steps=24)[0] for ct in S["cts"]]
    ivc.free()
    p = api.PbsProver(0, S["cyc"], S["dum"], keys["bsk"], keys["ksk"], K, ELL, LOGB, chains=2, witness_batch=8)
    proofs, out_ct, lwe_out = p.prove(S["cts"], S["tv"], steps=24)
    p.close()
    assert [len(b) for b in proofs] == [len(b) for b in want] and proofs == want
    decrypted = [int(round(int(m) / S["delta"])) % 4 for m in api.lwe_decrypt(keys["s_lwe"], lwe_out)]
    assert decrypted == [1, 0, 1]


def test_device_only_keys(n6):
    """keys that never exist on the host (Context.keygen_device) give the proofs of host keys from the same seed"""
    S = n6
    dk = S["c"].keygen_device(S["N"], K, ELL, LOGB, S["n_lwe"], 77, *SIGMAS)
    p = api.PbsProver(0, S["cyc"], S["dum"], dk["d_bsk"], dk["d_ksk"], K, ELL, LOGB, chains=2, witness_batch=3, keys_on_device=True, N=S["N"],
                      n_lwe=S["n_lwe"])
    proofs, out_ct, lwe_out = p.prove(S["cts"], S["testvs"])
    kh = p.key_hash()
    p.close()
    S["c"].device_free(dk["d_bsk"])
    S["c"].device_free(dk["d_ksk"])
    assert proofs == S["want"] and (out_ct == S["out_ct"]).all() and (lwe_out == S["lwe_out"]).all()
    assert (kh == api.pbs_key_hash(S["keys"]["bsk"], S["keys"]["ksk"])).all()


def test_reuse_checks_and_callbacks_that_raise(n6):
    S = n6
    keys = S["keys"]
    p = api.PbsProver(0, S["cyc"], S["dum"], keys["bsk"], keys["ksk"], K, ELL, LOGB, chains=2, witness_batch=3)
    # malformed runs are refused with a message and deliver nothing
    with pytest.raises(api.VpbsError, match="steps exceeds"):
        p.prove(S["cts"], S["testvs"], steps=S["n_lwe"] + 3)
    first = p.prove(S["cts"], S["testvs"])[0]
    run = p.last_run()
    assert run["proofs"] == 5 and 0 < run["outputs_seconds"] < run["seconds"] and run["chain"]["steps"] == 8
    assert run["chain"]["early_witness_ms"] > 0 and run["chain"]["prove_step_ms"] > 0 and run["prepare_chain_ms"] > 0
    p.set_check_witness(True)
    again = p.prove(S["cts"], S["testvs"])[0]
    assert first == again == S["want"]
    assert p.witness_checks() == (5 * (1 + 8), 0)
    p.set_check_witness(True)                                  # resets the counters
    prefix = p.prove(S["cts"][:3], S["testvs"][:3], steps=5)[0]
    assert p.witness_checks() == (3 * (1 + 5), 0)
    p.set_check_witness(False)
    assert prefix == [S["ivc"].prove_pbs(S["testvs"][i], S["cts"][i], keys["bsk"], keys["ksk"], steps=5)[0] for i in range(3)]
    # checkpoints carry the ciphertext index and are the prefix proofs of that ciphertext
    got = {}
    p.on_checkpoint(5, lambda i, done, b: got.__setitem__((i, done), b))
    assert p.prove(S["cts"][:3], S["testvs"][:3])[0] == S["want"][:3]
    p.on_checkpoint(0, None)
    assert sorted(got) == [(0, 5), (1, 5), (2, 5)] and [got[(i, 5)] for i in range(3)] == prefix
    # a proof callback that raises: re-raised after the run has drained, and the object goes on working
    seen = []

    def boom(i, b):
        seen.append(i)
        raise ZeroDivisionError("in the callback")
    with pytest.raises(ZeroDivisionError):
        p.prove(S["cts"], S["testvs"], on_proof=boom)
    assert len(seen) == 1
    assert p.prove(S["cts"], S["testvs"])[0] == S["want"]
    # an empty batch
    proofs, out_ct, lwe_out = p.prove(np.zeros((0, S["n_lwe"] + 1), np.uint64), S["tv"])
    assert proofs == [] and out_ct.shape == (0, K, S["N"])
    p.close()


def test_the_tool_proves_verifies_and_decrypts_a_batch():
    import __graft_entry__ as entry
    export_circuits.ensure_cyclic_circuit(8, K, ELL, LOGB, 6, 13)
    tool = [sys.executable, os.path.join(entry.ROOT, "tools", "prove_batch.py"), "--n8", "--count", "4", "--chains", "2", "--witness-batch", "3"]

    def run(*more):
        r = subprocess.run(tool + list(more), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])
    a = run("--steps", "6")
    assert (a["count"], a["chains"], a["steps"], a["accepted"], a["decrypted_correct"]) == (4, 2, 6, 4, 4), a
    assert 0 < a["seconds_until_out_ct_complete"] < a["seconds"] and a["early_witness_ms_per_step"] > 0
    b = run("--keys-on-device")
    assert (b["steps"], b["accepted"], b["decrypted_correct"], b["keys_on_device"]) == (8, 4, 4, True), b
    d = run("--baseline")
    assert (d["accepted"], d["decrypted_correct"], d["baseline"]) == (4, 4, True), d
