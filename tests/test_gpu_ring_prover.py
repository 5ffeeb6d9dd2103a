"""GPU tests (-m gpu): api.RingProver and api.Program.prove_batch -- ONE prover for the clients of a key ring.  Ciphertext i is bootstrapped
and proven under the key set of slot key_of[i]; the proofs are deterministic, so whatever the slot, the chain count and the completion order
they must be, byte for byte, what the one-key paths make under that key set: Ivc.prove_pbs, PbsProver, Program.prove.  The outputs are the
key ring's.  The shapes are the smallest of tests/test_gpu_pbs_prove_batch.py: N = 8, n = 6 (8 steps per chain), degree 2^13."""
import ctypes as C
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
N, N_LWE, LOG_N = 8, 6, 13
G = K * ELL * K * N
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)
KEY_OF = [0, 2, 1, 0, 2]
MARK = np.uint64(0xA5A5A5A5A5A5A5A5)
INVALID = -1   # VPBS_ERR_INVALID


def load(N, n_lwe, log_n):
    return [circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, n_lwe, log_n)]


def ring_prover(S, seeds=(0, 1, 2), **kw):
    rp = api.RingProver(0, S["cyc"], S["dum"], K, ELL, LOGB, N, N_LWE, max_keys=4, **kw)
    assert [rp.add(S["keys"][k]["bsk"], S["keys"][k]["ksk"]) for k in seeds] == list(range(len(seeds)))
    return rp


@pytest.fixture(scope="module")
def n6():
    """three key sets (seeds 77, 78, 79; a fourth, 80, for the slot that is reused), the five ciphertexts of test_gpu_pbs_prove_batch's n6 --
    one with a mask word at or above p, one with a test vector of its own -- and what the paths that existed before make of ciphertext i
    under key set KEY_OF[i]: Ivc.prove_pbs's bytes, KeyRing.run's outputs.  Computed once, read by every test, never changed."""
    assert api.lib().vpbs_ring_prover_run is not None and INVALID == -1
    cyc, dum = load(N, N_LWE, LOG_N)
    c = vpbs_amd.Context(0, log_n_max=16)
    keys = [c.keygen(N, K, ELL, LOGB, N_LWE, seed, *SIGMAS) for seed in (77, 78, 79, 80)]
    tv, delta = api.testv(N, 2)
    msgs = [1, 0, 1, 1, 0]
    cts = np.stack([api.lwe_encrypt(keys[0]["params"], keys[0]["s_lwe"], delta * m % P, nonce=10 + i) for i, m in enumerate(msgs)])
    cts[2, 3] = np.uint64(P + 5)                                    # a mask word at or above p
    testvs = np.stack([tv] * 5)
    testvs[4] = np.array([(P - int(v)) % P for v in tv], np.uint64)   # a test vector of its own
    ivc = api.Ivc(c, cyc, dum, N, K, G)
    prove = lambda i, k: ivc.prove_pbs(testvs[i], cts[i], keys[k]["bsk"], keys[k]["ksk"])[0]
    want = [prove(i, k) for i, k in enumerate(KEY_OF)]
    want_reused = {i: prove(i, 3) for i, k in enumerate(KEY_OF) if k == 1}   # slot 1 after key set 80 has taken it
    vk, _ = ivc.verifier_data()
    ivc.free()
    kr = api.KeyRing(c, K, ELL, LOGB, N, N_LWE, max_keys=4, max_batch=8)
    assert [kr.add(k["bsk"], k["ksk"]) for k in keys[:3]] == [0, 1, 2]
    out_ct, lwe_out = kr.run(cts, KEY_OF, testvs)
    kr.close()
    key_hashes = [api.pbs_key_hash(k["bsk"], k["ksk"]) for k in keys]
    assert len({h.tobytes() for h in key_hashes}) == 4 and len(set(want)) == 5
    yield dict(c=c, cyc=cyc, dum=dum, keys=keys, cts=cts, testvs=testvs, tv=tv, delta=delta, want=want, want_reused=want_reused, vk=vk,
               out_ct=out_ct, lwe_out=lwe_out, key_hashes=key_hashes)
    c.close()


@pytest.fixture(scope="module")
def shared(n6):
    """one ring prover with the three key sets, and its proofs of the batch: for the tests that change no slot"""
    rp = ring_prover(n6, chains=3, witness_batch=3)
    proofs, out_ct, lwe_out = rp.prove(n6["cts"], KEY_OF, n6["testvs"])
    yield dict(rp=rp, proofs=proofs, out_ct=out_ct, lwe_out=lwe_out)
    rp.close()


def verifier(S, key_hash, max_batch=5):
    cyc, vk = S["cyc"], S["vk"]
    return api.PbsVerifier(S["c"], vk[4:].reshape(-1, 4), [cyc.n_constants + 80, 135, 20, 16], vk[:4], LOG_N, cyc.n_constants, 80, cyc.gates, N, K,
                           N_LWE, G, key_hash, max_batch=max_batch)


@pytest.mark.parametrize("chains", [1, 3])
@pytest.mark.parametrize("witness_batch", [1, 3])
def test_byte_parity_with_the_one_key_path(n6, chains, witness_batch):
    S = n6
    rp = ring_prover(S, chains=chains, witness_batch=witness_batch)
    order = []
    proofs, out_ct, lwe_out = rp.prove(S["cts"], KEY_OF, S["testvs"], on_proof=lambda i, b: order.append(i))
    hashes, (pvk, _) = [rp.key_hash(s) for s in range(3)], rp.verifier_data()
    run = rp.last_run()
    rp.close()
    assert sorted(order) == [0, 1, 2, 3, 4]
    for i in range(5):
        assert proofs[i] == S["want"][i], (i, KEY_OF[i], len(proofs[i]), len(S["want"][i]))
    assert (out_ct == S["out_ct"]).all() and (lwe_out == S["lwe_out"]).all()
    for s in range(3):
        assert (hashes[s] == S["key_hashes"][s]).all(), s
    assert (pvk == S["vk"]).all()
    assert run["proofs"] == 5 and 0 < run["outputs_seconds"] < run["seconds"] and run["chain"]["steps"] == 8 and run["prepare_chain_ms"] > 0


def test_the_right_key_is_what_is_proven(n6, shared):
    """a proof is accepted by the verifier of its own slot's key hash and by no other slot's"""
    S, rp, proofs = n6, shared["rp"], shared["proofs"]
    assert proofs == S["want"]
    for slot in range(3):
        pv = verifier(S, rp.key_hash(slot))
        verdicts, reasons, _ = pv.verify(proofs, S["testvs"], S["cts"], shared["out_ct"].reshape(5, -1))
        pv.close()
        assert verdicts.tolist() == [int(k == slot) for k in KEY_OF], (slot, [api.pbs_reason_text(int(r)) for r in reasons])
        for i, k in enumerate(KEY_OF):
            if k != slot:
                assert int(reasons[i]) == 8 and "key hash" in api.pbs_reason_text(int(reasons[i]))   # VPBS_PBS_KEY_HASH


def test_the_golden_chain():
    """the N = 8, n = 1 chain of the CPU oracle through a one-slot ring prover: the frozen length and sha256"""
    from test_cyclic_cpu import GOLDEN_CHAIN, n8_chain_inputs
    ring, (s_to, s_lwe, s_glwe, bsk, ksk), delta, testv, ct = n8_chain_inputs()
    cyc, dum = load(8, 1, 13)
    frozen = json.load(open(GOLDEN_CHAIN))
    rp = api.RingProver(0, cyc, dum, K, ELL, LOGB, 8, 1, max_keys=1, chains=1, witness_batch=2)
    assert rp.add(np.stack([T.flatten_ggsw(g) for g in bsk]), T.flatten_ggsw(ksk)) == 0
    proofs, out_ct, lwe_out = rp.prove(np.array([ct], np.uint64), [0], np.array(testv, np.uint64))
    rp.close()
    assert [(len(b), hashlib.sha256(b).hexdigest()) for b in proofs] == [(frozen["bytes"], frozen["sha256"])]


def test_device_only_keys(n6):
    """keys that never exist on the host (Context.keygen_device), adopted: the proofs and hashes of host keys from the same seeds"""
    S = n6
    dks = [S["c"].keygen_device(N, K, ELL, LOGB, N_LWE, seed, *SIGMAS) for seed in (77, 78, 79)]
    rp = api.RingProver(0, S["cyc"], S["dum"], K, ELL, LOGB, N, N_LWE, max_keys=3, chains=2, witness_batch=3)
    assert [rp.add(d["d_bsk"], d["d_ksk"], keys_on_device=True) for d in dks] == [0, 1, 2]
    proofs, out_ct, lwe_out = rp.prove(S["cts"], KEY_OF, S["testvs"])
    hashes = [rp.key_hash(s) for s in range(3)]
    rp.close()
    for d in dks:
        S["c"].device_free(d["d_bsk"])
        S["c"].device_free(d["d_ksk"])
    assert proofs == S["want"] and (out_ct == S["out_ct"]).all() and (lwe_out == S["lwe_out"]).all()
    assert all((hashes[s] == S["key_hashes"][s]).all() for s in range(3))


def test_a_reused_slot_has_the_new_keys_links(n6):
    S = n6
    rp = ring_prover(S, chains=2, witness_batch=3)
    rp.remove(1)
    with pytest.raises(api.VpbsError):
        rp.key_hash(1)
    assert rp.add(S["keys"][3]["bsk"], S["keys"][3]["ksk"]) == 1
    proofs = rp.prove(S["cts"], KEY_OF, S["testvs"])[0]
    kh = rp.key_hash(1)
    rp.close()
    assert (kh == S["key_hashes"][3]).all() and not (kh == S["key_hashes"][1]).all()
    for i, k in enumerate(KEY_OF):
        assert proofs[i] == (S["want_reused"][i] if k == 1 else S["want"][i]), (i, k)


def raw_run(rp, cts, count, key_of, testv, steps, out_ct, lwe_out, calls):
    """vpbs_ring_prover_run as the C ABI has it -> (status, message)"""
    cb = api.PBS_PROOF_FN(lambda *a: calls.append(a[1]))
    err = C.create_string_buffer(512)
    ptr = lambda a: None if a is None else a.ctypes.data_as(api.U64P)
    ko = np.ascontiguousarray(key_of, dtype=np.uint32)
    rc = api.lib().vpbs_ring_prover_run(rp.h, ptr(cts), count, ko.ctypes.data, ptr(testv), 1, steps, ptr(out_ct), ptr(lwe_out), cb, None, err, 512)
    return rc, err.value.decode()


def test_refusals(n6, shared):
    S, rp = n6, shared["rp"]
    assert rp.add(S["keys"][3]["bsk"], S["keys"][3]["ksk"]) == 3
    rp.remove(3)                                                     # slot 3: emptied
    cts, testvs = np.ascontiguousarray(S["cts"]), np.ascontiguousarray(S["testvs"])
    out_ct, lwe_out, calls = np.full((5, K, N), MARK), np.full((5, N_LWE + 1), MARK), []
    untouched = lambda: (out_ct == MARK).all() and (lwe_out == MARK).all() and calls == []
    rc, msg = raw_run(rp, cts, 5, [0, 2, 3, 0, 2], testvs, 0, out_ct, lwe_out, calls)
    assert rc == INVALID and "key_of[2] = 3" in msg and "slot 3 is empty" in msg and "ciphertext 2" in msg and untouched(), msg
    rc, msg = raw_run(rp, cts, 5, [0, 2, 1, 4, 2], testvs, 0, out_ct, lwe_out, calls)
    assert rc == INVALID and "key_of[3] = 4" in msg and "out of range" in msg and "ciphertext 3" in msg and untouched(), msg
    rc, msg = raw_run(rp, None, 5, KEY_OF, testvs, 0, out_ct, lwe_out, calls)
    assert rc == INVALID and "null cts" in msg and untouched(), msg
    rc, msg = raw_run(rp, cts, 5, KEY_OF, testvs, N_LWE + 3, out_ct, lwe_out, calls)
    assert rc == INVALID and "steps exceeds n_lwe + 2 = 8" in msg and untouched(), msg
    rc, msg = raw_run(rp, cts, 0, [], testvs, 0, out_ct, lwe_out, calls)
    assert rc == 0 and untouched()
    # the Python form: the ring's message and status, nothing written
    with pytest.raises(api.VpbsError, match=r"key_of\[2\] = 3: slot 3 is empty; ciphertext 2 has no key set") as e:
        rp.prove(cts, [0, 2, 3, 0, 2], testvs, on_proof=lambda i, b: calls.append(i), out_ct=out_ct, lwe_out=lwe_out)
    assert e.value.status == INVALID and untouched()
    proofs, o, l = rp.prove(cts[:0], [], S["tv"])
    assert proofs == [] and o.shape == (0, K, N)
    # the key links live in the prover: the owned ring takes no key set from anybody else, and stays as it was
    for call in (lambda: rp.keyring.add(S["keys"][3]["bsk"], S["keys"][3]["ksk"]), lambda: rp.keyring.remove(0)):
        with pytest.raises(api.VpbsError, match="vpbs_ring_prover_add") as e:
            call()
        assert e.value.status == INVALID
    assert rp.keyring.count() == 3
    assert rp.prove(cts, KEY_OF, testvs)[0] == S["want"]              # and the object goes on working


def test_the_ring_is_shared_with_evaluation(n6, shared):
    """KeyRing.run through .keyring between two prove calls: the ring's own outputs, and the second prove as the first"""
    S, rp = n6, shared["rp"]
    first = rp.prove(S["cts"], KEY_OF, S["testvs"])
    out_ct, lwe_out, accs = rp.keyring.run(S["cts"], KEY_OF, S["testvs"], accumulators=True)
    assert (out_ct == S["out_ct"]).all() and (lwe_out == S["lwe_out"]).all() and (accs[:, -1] == S["out_ct"]).all()
    second = rp.prove(S["cts"], KEY_OF, S["testvs"])
    assert first[0] == second[0] == S["want"]
    for a, b in zip(first[1:], second[1:]):
        assert (a == b).all()


# 3 inputs (wires 0 1 2), 4 gates (wires 3 .. 6), 2 levels; gate 2 has fan-in 2 with the coefficients 3 and p - 2 and reads gate 0 and gate 1
FOUR = [([(0, 1)], 0, 0), ([(1, 1), (2, P - 1)], 7, 1), ([(3, 3), (4, P - 2)], 5, 0), ([(2, 1)], 0, 1)]
INSTANCE_KEYS = [1, 0, 1]


@pytest.fixture(scope="module")
def program(n6):
    """the program under two key sets: what Program.prove on a PbsProver of the instance's key set and Program.run_batch give, and prove_batch"""
    S = n6
    c, keys = S["c"], S["keys"]
    tv = S["tv"]
    testvs = np.stack([tv, np.array([(P - int(v)) % P for v in tv], np.uint64)])
    inputs = np.array([[api.lwe_encrypt(keys[k]["params"], keys[k]["s_lwe"], S["delta"] * m % P, nonce=40 + 3 * b + j)
                        for j, m in enumerate(((b + 1) % 2, b % 2, 1))] for b, k in enumerate(INSTANCE_KEYS)], np.uint64)
    prog = api.Program(c, 3, FOUR, 2)
    assert prog.levels()[1] == 2
    want = []
    for k in (0, 1):
        pp = api.PbsProver(0, S["cyc"], S["dum"], keys[k]["bsk"], keys[k]["ksk"], K, ELL, LOGB, chains=2, witness_batch=3)
        want.append({b: prog.prove(pp, inputs[b], testvs)[0] for b, kk in enumerate(INSTANCE_KEYS) if kk == k})
        pp.close()
    rp = ring_prover(S, seeds=(0, 1), chains=3, witness_batch=3)
    batch = prog.run_batch(rp.keyring, inputs, INSTANCE_KEYS, testvs)
    seen = []
    proofs, wires, out_cts = prog.prove_batch(rp, inputs, INSTANCE_KEYS, testvs, on_proof=lambda bg, blob: seen.append((bg, blob)))
    hashes = [rp.key_hash(s) for s in range(2)]
    rp.close()
    yield dict(prog=prog, inputs=inputs, testvs=testvs, want=want, batch=batch, proofs=proofs, wires=wires, out_cts=out_cts, seen=seen, hashes=hashes)
    prog.close()


def test_program_prove_batch_is_program_prove_per_instance(n6, program):
    Q = program
    for b, k in enumerate(INSTANCE_KEYS):
        assert Q["proofs"][b] == Q["want"][k][b], (b, k)
    assert (Q["wires"] == Q["batch"][0]).all() and (Q["out_cts"] == Q["batch"][2]).all()
    assert sorted(bg for bg, _ in Q["seen"]) == [(b, g) for b in range(3) for g in range(4)]
    assert all(blob == Q["proofs"][b][g] for (b, g), blob in Q["seen"])
    pvs = [verifier(n6, h, max_batch=4) for h in Q["hashes"]]
    for b, k in enumerate(INSTANCE_KEYS):
        verdicts, reasons, _ = Q["prog"].verify(pvs[k], Q["inputs"][b], Q["testvs"], Q["out_cts"][b], Q["proofs"][b])
        assert verdicts.tolist() == [1, 1, 1, 1], (b, [api.pbs_reason_text(int(r)) for r in reasons])
        verdicts, reasons, _ = Q["prog"].verify(pvs[1 - k], Q["inputs"][b], Q["testvs"], Q["out_cts"][b], Q["proofs"][b])
        assert verdicts.tolist() == [0, 0, 0, 0] and set(reasons.tolist()) == {8}     # another client's key hash: VPBS_PBS_KEY_HASH
    # one forged output: instance 1, gate 0 -- wire 3, which gate 2 reads
    forged = Q["out_cts"].copy()
    forged[1, 0, 0, 3] ^= np.uint64(1)
    for b, k in enumerate(INSTANCE_KEYS):
        verdicts, reasons, _ = Q["prog"].verify(pvs[k], Q["inputs"][b], Q["testvs"], forged[b], Q["proofs"][b])
        if b == 1:
            assert verdicts.tolist() == [0, 1, 0, 1] and reasons[0] == 5 and reasons[2] == 9     # VPBS_PBS_OUT_CT; VPBS_PBS_LWE_HASH
        else:
            assert verdicts.tolist() == [1, 1, 1, 1], b
    for pv in pvs:
        pv.close()


def test_program_prove_batch_refusals(n6, program):
    S, Q = n6, program
    rp = ring_prover(S, seeds=(0,), chains=1, witness_batch=3)
    seen = []
    with pytest.raises(api.VpbsError, match=r"key_of\[2\] = 1: slot 1 is empty; instance 2 has no key set") as e:
        Q["prog"].prove_batch(rp, Q["inputs"], [0, 0, 1], Q["testvs"], on_proof=lambda bg, b: seen.append(bg))
    assert e.value.status == INVALID and seen == []
    with pytest.raises(api.VpbsError, match="steps exceeds"):
        Q["prog"].prove_batch(rp, Q["inputs"], [0, 0, 0], Q["testvs"], steps=N_LWE + 3)
    proofs, wires, out_cts = Q["prog"].prove_batch(rp, Q["inputs"][:0], [], Q["testvs"])
    rp.close()
    assert proofs == [] and wires.shape == (0, 7, N_LWE + 1)


def test_the_tool_proves_under_two_key_sets():
    import __graft_entry__ as entry
    export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, N_LWE, LOG_N)
    r = subprocess.run([sys.executable, os.path.join(entry.ROOT, "tools", "prove_batch.py"), "--n8", "--keys", "2", "--count", "3", "--chains", "2",
                        "--witness-batch", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a = json.loads(r.stdout.strip().splitlines()[-1])
    assert (a["count"], a["keys"], a["accepted"], a["decrypted_correct"], a["baseline"]) == (3, 2, 3, 3, False), a
    assert a["proofs"] == 3 and 0 < a["seconds_until_out_ct_complete"] < a["seconds"] and a["prepare_chain_ms"] > 0
    assert a["device_bytes_held_by_the_provers"] > 0
