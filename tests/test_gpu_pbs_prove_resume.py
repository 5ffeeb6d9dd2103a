"""GPU tests (-m gpu): api.PbsProver.resume / api.RingProver.resume -- checkpointed chains of a batch taken up again under resident keys
(vpbs_pbs_prover_resume, vpbs_ring_prover_resume; csrc/pbs_prove_pool.h).  At N = 8, n = 6 (8 steps).  The proofs are deterministic: the
uninterrupted proofs are Ivc.prove_pbs's bytes, a checkpoint with counter k is Ivc.prove_pbs(.., steps=k), and a resumed chain must deliver
the uninterrupted proof byte for byte; outputs are the Bootstrapper's whatever happens to a row's checkpoint."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import export_circuits
import vpbs_amd
from vpbs_amd import api, circuit_file

pytestmark = pytest.mark.gpu
P = api.P
K, ELL, LOGB = 2, 4, 5
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)
N, N_LWE, LOG_N = 8, 6, 13
TOTAL = N_LWE + 2
KEY_HASH = "checkpoint: the key hash chain does not match"


def make_prover(S, keys=None, chains=2, witness_batch=3):
    keys = keys or S["keys"]
    return api.PbsProver(0, S["cyc"], S["dum"], keys["bsk"], keys["ksk"], K, ELL, LOGB, chains=chains, witness_batch=witness_batch)


def prove_with_checkpoints(prover, prove):
    """prove() under on_checkpoint(1, ..) -> (what prove returned, {(index, k): bytes})"""
    ck = {}

    def keep(index, done, blob):
        assert (index, done) not in ck
        ck[(index, done)] = blob
    prover.on_checkpoint(1, keep)
    got = prove()
    prover.on_checkpoint(0, None)
    return got, ck


@pytest.fixture(scope="module")
def S():
    """seeded keys A and B, five ciphertexts under A (different messages and nonces, one with a mask word at or above p, one with a test
    vector of its own) and four under B; for the ciphertexts under A what the existing paths make of them: Ivc.prove_pbs's bytes with the
    prefix proofs Ivc.on_checkpoint(1) hands out, Bootstrapper.run's outputs; every checkpoint of a PbsProver run of each key set"""
    cyc, dum = [circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, N_LWE, LOG_N)]
    c = vpbs_amd.Context(0, log_n_max=16)
    keys, other = c.keygen(N, K, ELL, LOGB, N_LWE, 77, *SIGMAS), c.keygen(N, K, ELL, LOGB, N_LWE, 78, *SIGMAS)
    tv, delta = api.testv(N, 2)
    msgs = [1, 0, 1, 1, 0]
    cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * m % P, nonce=10 + i) for i, m in enumerate(msgs)])
    cts[2, 3] = np.uint64(P + 5)                                    # a mask word at or above p
    testvs = np.stack([tv] * 5)
    testvs[4] = np.array([(P - int(v)) % P for v in tv], np.uint64)   # a test vector of its own
    cts_b = np.stack([api.lwe_encrypt(other["params"], other["s_lwe"], delta * m % P, nonce=40 + i) for i, m in enumerate([0, 1, 1, 0])])
    ivc = api.Ivc(c, cyc, dum, N, K, K * ELL * K * N)
    want, ref_ck = [], {}
    for i in range(5):
        ivc.on_checkpoint(1, lambda done, blob, i=i: ref_ck.__setitem__((i, done), blob))
        want.append(ivc.prove_pbs(testvs[i], cts[i], keys["bsk"], keys["ksk"])[0])
    ivc.on_checkpoint(0, None)
    bs = api.Bootstrapper(c, keys["bsk"], keys["ksk"], K, ELL, LOGB, max_batch=8)
    out_ct, lwe_out = bs.run(cts, testvs)
    bs.close()
    bs = api.Bootstrapper(c, other["bsk"], other["ksk"], K, ELL, LOGB, max_batch=8)
    out_b, lwe_b = bs.run(cts_b, tv)
    bs.close()
    S = dict(c=c, ivc=ivc, cyc=cyc, dum=dum, keys=keys, other=other, cts=cts, testvs=testvs, tv=tv, want=want, ref_ck=ref_ck, out_ct=out_ct,
             lwe_out=lwe_out, cts_b=cts_b, out_b=out_b, lwe_b=lwe_b)
    p = make_prover(S)
    (proofs, o, l), ck = prove_with_checkpoints(p, lambda: p.prove(cts, testvs))
    p.close()
    assert proofs == want and (o == out_ct).all() and (l == lwe_out).all()
    for i in range(5):
        ck[(i, TOTAL)] = want[i]   # the proof after all n + 2 steps: a checkpoint with counter n + 2
    # ciphertext 1 under key set B: the same ciphertext words, proven under other keys (for the key-hash refusal), and B's own rows
    p = make_prover(S, other)
    (proofs_b, _, _), ck_b = prove_with_checkpoints(p, lambda: p.prove(np.concatenate([cts_b, cts[1:2]]), tv))
    p.close()
    S.update(ck=ck, want_b=proofs_b[:4], ck_b=ck_b)
    yield S
    ivc.free()
    c.close()


def test_every_checkpoint_is_the_prefix_proof(S):
    """7 checkpoints per chain at every = 1, each the bytes Ivc hands out after the same step; the ones the tests below resume from are
    compared with Ivc.prove_pbs(.., steps=k) itself"""
    assert sorted(k for k in S["ck"]) == [(i, k) for i in range(5) for k in range(1, TOTAL + 1)]
    for (i, k), blob in S["ck"].items():
        if k < TOTAL:
            assert blob == S["ref_ck"][(i, k)], (i, k)
    for i, k in [(1, 1), (2, 4), (3, 7), (0, 3), (0, 5)]:
        assert S["ck"][(i, k)] == S["ivc"].prove_pbs(S["testvs"][i], S["cts"][i], S["keys"]["bsk"], S["keys"]["ksk"], steps=k)[0], (i, k)


ROWS = [None, 1, 4, N_LWE + 1, N_LWE + 2]   # the checkpoint's counter of ciphertext i


def five(S):
    return [None if k is None else S["ck"][(i, k)] for i, k in enumerate(ROWS)]


@pytest.mark.parametrize("chains,witness_batch", [(1, 3), (2, 1), (2, 3), (2, 8)])
def test_one_resume_of_five_rows(S, chains, witness_batch):
    """k = None, 1, 4, n + 1 and n + 2 in one call.  chains = 1: the rows are proven in order on one worker, so the chain resumed at k = 1
    follows a full chain of another ciphertext, and the one resumed at k = 4 finds that worker's accumulator slots below 3 stale"""
    p = make_prover(S, chains=chains, witness_batch=witness_batch)
    order = []
    proofs, out_ct, lwe_out, errors = p.resume(S["cts"], S["testvs"], five(S), on_proof=lambda i, b: order.append(i))
    run = p.last_run()
    p.close()
    assert errors == [None] * 5 and sorted(order) == [0, 1, 2, 3, 4]
    if chains == 1:
        assert order == [0, 1, 2, 3, 4]
    for i in range(5):
        assert proofs[i] == S["want"][i], (i, ROWS[i])
    assert (out_ct == S["out_ct"]).all() and (lwe_out == S["lwe_out"]).all()
    assert run["proofs"] == 5 and 0 < run["outputs_seconds"] < run["seconds"]


def test_steps_at_and_below_the_counter(S):
    """steps = k returns the validated checkpoint; steps < k is refused for that row only, and the other row gets its prefix proof"""
    p = make_prover(S)
    proofs, out_ct, lwe_out, errors = p.resume(S["cts"][1:3], S["testvs"][1:3], [S["ck"][(1, 1)], S["ck"][(2, 4)]], steps=4)
    assert errors == [None, None] and proofs == [S["ck"][(1, 4)], S["ck"][(2, 4)]]
    assert (out_ct == S["out_ct"][1:3]).all() and (lwe_out == S["lwe_out"][1:3]).all()
    proofs, out_ct, lwe_out, errors = p.resume(S["cts"][1:3], S["testvs"][1:3], [S["ck"][(1, 1)], S["ck"][(2, 4)]], steps=3)
    p.close()
    assert errors == [None, "checkpoint: its counter 4 is beyond the requested 3 steps"]
    assert proofs == [S["ck"][(1, 3)], None]
    assert (out_ct == S["out_ct"][1:3]).all() and (lwe_out == S["lwe_out"][1:3]).all()


def test_no_checkpoint_at_all_is_prove(S):
    p = make_prover(S)
    proofs, out_ct, lwe_out, errors = p.resume(S["cts"], S["testvs"], [None] * 5)
    p.close()
    assert errors == [None] * 5 and proofs == S["want"]
    assert (out_ct == S["out_ct"]).all() and (lwe_out == S["lwe_out"]).all()


def test_checkpoints_taken_during_a_resume(S):
    """every = 2 from k = 3: the checkpoints carry done = 5 and 7 -- chain steps, not steps of the call -- and are those of the
    uninterrupted run"""
    p = make_prover(S, chains=1)
    seen = []
    p.on_checkpoint(2, lambda index, done, blob: seen.append((index, done, blob)))
    proofs, _, _, errors = p.resume(S["cts"][:1], S["testvs"][:1], [S["ck"][(0, 3)]])
    p.close()
    assert errors == [None] and proofs == S["want"][:1]
    assert [(i, d) for i, d, _ in seen] == [(0, 5), (0, 7)]
    assert [b for _, _, b in seen] == [S["ck"][(0, 5)], S["ck"][(0, 7)]]


def flipped(blob):
    """one proof word changed by one bit (the first cap word: still a canonical field element)"""
    b = bytearray(blob)
    b[0] ^= 1
    return bytes(b)


def test_refused_checkpoints_among_valid_rows(S):
    """another ciphertext's checkpoint, truncated bytes, one flipped proof word, a checkpoint made under another key set: each refused
    with its message through exactly one call of proof_fn, its outputs the Bootstrapper's all the same, the valid rows around them
    delivered byte for byte"""
    rows = [0, 1, 2, 3, 4, 1, 0]   # ciphertexts
    cps = [S["ck"][(0, 3)],            # valid
           S["ck"][(2, 4)],            # ciphertext 2's, presented for ciphertext 1
           S["ck"][(2, 4)],            # valid
           S["ck"][(3, 7)][:-9],       # truncated
           flipped(S["ck"][(4, 2)]),   # does not verify
           S["ck_b"][(4, 4)],          # ciphertext 1 proven under key set B
           None]                       # valid: from step 0
    want_err = {1: "checkpoint: the LWE hash chain does not match",
                3: "checkpoint: the bytes are not a proof of this circuit (shape, canonical field elements, number of public inputs)",
                4: "checkpoint: the proof does not verify", 5: KEY_HASH}
    cts, testvs = np.ascontiguousarray(S["cts"][rows]), np.ascontiguousarray(S["testvs"][rows])
    p = make_prover(S)
    # through the C ABI, to count the calls
    calls = []
    cb = api.PBS_PROOF_FN(lambda _u, index, data, n, error: calls.append((int(index), C.string_at(data, n) if data else None, error)))
    ptrs, lens, alive = api._checkpoint_arrays(cps)
    out_ct, lwe_out = np.zeros((7, K, N), np.uint64), np.zeros((7, N_LWE + 1), np.uint64)
    err = C.create_string_buffer(512)
    n = api.lib().vpbs_pbs_prover_resume(p.h, api._ptr(cts), 7, api._ptr(testvs), 1, C.addressof(ptrs), C.addressof(lens), 0, api._ptr(out_ct),
                                         api._ptr(lwe_out), cb, None, err, 512)
    assert n == 3, err.value
    assert sorted(i for i, _, _ in calls) == list(range(7))   # once per row
    for i, blob, error in calls:
        if i in want_err:
            assert blob is None and error.decode() == want_err[i], (i, error)
        else:
            assert error is None and blob == S["want"][rows[i]], i
    assert (out_ct == S["out_ct"][rows]).all() and (lwe_out == S["lwe_out"][rows]).all()
    # and through Python: nothing raised, None in proofs, the messages in errors
    proofs, out_ct, lwe_out, errors = p.resume(cts, testvs, cps)
    p.close()
    assert errors == [want_err.get(i) for i in range(7)]
    assert proofs == [None if i in want_err else S["want"][rows[i]] for i in range(7)]
    assert (out_ct == S["out_ct"][rows]).all() and (lwe_out == S["lwe_out"][rows]).all()


def test_the_ring_prover_resumes_rows_of_two_slots(S):
    """slot 0 = key set A, slot 1 = key set B, rows interleaved: checkpoints of the ring prover's own run, a resume that takes rows of both
    slots up again, proofs equal to those of the per-key PbsProvers; a checkpoint presented under the other slot is refused"""
    rp = api.RingProver(0, S["cyc"], S["dum"], K, ELL, LOGB, N, N_LWE, max_keys=2, chains=2, witness_batch=3)
    assert rp.add(S["keys"]["bsk"], S["keys"]["ksk"]) == 0 and rp.add(S["other"]["bsk"], S["other"]["ksk"]) == 1
    cts = np.stack([S["cts"][0], S["cts_b"][0], S["cts"][1], S["cts_b"][1], S["cts_b"][2]])
    key_of = [0, 1, 0, 1, 1]
    want = [S["want"][0], S["want_b"][0], S["want"][1], S["want_b"][1], S["want_b"][2]]
    want_out = np.stack([S["out_ct"][0], S["out_b"][0], S["out_ct"][1], S["out_b"][1], S["out_b"][2]])
    want_lwe = np.stack([S["lwe_out"][0], S["lwe_b"][0], S["lwe_out"][1], S["lwe_b"][1], S["lwe_b"][2]])
    (proofs, _, _), ck = prove_with_checkpoints(rp, lambda: rp.prove(cts, key_of, S["tv"]))
    assert proofs == want
    assert ck[(0, 4)] == S["ck"][(0, 4)] and ck[(1, 2)] == S["ck_b"][(0, 2)]
    cps = [ck[(0, 4)], ck[(1, 2)], None, ck[(3, 7)], ck[(4, 1)]]
    proofs, out_ct, lwe_out, errors = rp.resume(cts, key_of, S["tv"], cps)
    assert errors == [None] * 5 and proofs == want
    assert (out_ct == want_out).all() and (lwe_out == want_lwe).all()
    # ciphertext 0 and its checkpoint under slot 1: everything but the key hash is that slot's too
    proofs, out_ct, lwe_out, errors = rp.resume(cts[[0, 1]], [1, 1], S["tv"], [ck[(0, 4)], ck[(1, 2)]])
    rp.close()
    assert errors == [KEY_HASH, None] and proofs[0] is None and proofs[1] == want[1]
    assert (out_ct[1] == want_out[1]).all() and (lwe_out[1] == want_lwe[1]).all()


def test_the_tool_checkpoints_and_resumes(tmp_path):
    import __graft_entry__ as entry
    tool = [sys.executable, os.path.join(entry.ROOT, "tools", "prove_batch.py"), "--n8", "--count", "3", "--chains", "2", "--witness-batch", "3"]

    def run(*more, status=0):
        r = subprocess.run(tool + list(more), capture_output=True, text=True, timeout=900)
        assert r.returncode == status, r.stdout[-2000:] + r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])
    d = str(tmp_path / "ck")
    a = run("--checkpoint", d + ":3")
    assert a["checkpoints_written"] == 6 and a["resumed_from"] == [0, 0, 0] and a["accepted"] == 3
    assert sorted(os.listdir(d)) == sorted("ct%d_step%d.bin" % (i, k) for i in range(3) for k in (3, 6))
    os.remove(os.path.join(d, "ct1_step6.bin"))
    os.remove(os.path.join(d, "ct2_step3.bin"))
    os.remove(os.path.join(d, "ct2_step6.bin"))
    b = run("--resume", d)
    assert b["resumed_from"] == [6, 3, 0] and b["checkpoints_refused"] == {} and (b["accepted"], b["decrypted_correct"]) == (3, 3)
    assert b["proofs_sha256"] == a["proofs_sha256"] and all(b["proofs_sha256"])
    # a foreign file in the directory: that row is refused and reported, the others are proven and verified, the exit status is 1
    with open(os.path.join(d, "ct0_step6.bin"), "rb") as f, open(os.path.join(d, "ct2_step6.bin"), "wb") as g:
        g.write(f.read())
    c = run("--resume", d, status=1)
    assert c["checkpoints_refused"] == {"2": "checkpoint: the LWE hash chain does not match"} and c["resumed_from"] == [6, 3, 0]
    assert (c["accepted"], c["decrypted_correct"]) == (2, 3) and c["proofs_sha256"] == a["proofs_sha256"][:2] + [None]
