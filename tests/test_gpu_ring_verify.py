"""GPU tests (-m gpu): api.RingVerifier and api.Program.verify_batch -- ONE device verifier of whole vPBS proofs for the clients of a key
ring.  Proof i is checked against the key hash of slot key_of[i] and the test vector testvs[testv_of[i]].  The yardstick throughout is the
host's api.verify_pbs under the keys of the proof's slot: the device must give every proof the host's verdict and, through pbs_reason_text,
the host's `why` -- and, byte for byte, what an api.PbsVerifier made from that slot's key hash gives.  The shapes are those of
tests/test_gpu_ring_prover.py: N = 8, n = 6 (8 steps per chain), degree 2^13, three key sets plus a fourth."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import export_circuits
import vpbs_amd
from batch_verify_layout import proof_layout
from vpbs_amd import api, circuit_file

pytestmark = pytest.mark.gpu
P = api.P
K, ELL, LOGB = 2, 4, 5
N, N_LWE, LOG_N = 8, 6, 13
KN = K * N
G = K * ELL * K * N
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_KEYS = 4
SLOT_KEYS = [0, 1, 3, 2]          # slot s holds the hash of key set SLOT_KEYS[s]: slot 2 the fourth one's, which no proof of the batch names
KEY_OF = [0, 3, 1, 0, 3]          # unsorted, with the highest slot in use; proof i was made under key set SLOT_KEYS[KEY_OF[i]]
MARK = 0xA5
INVALID = -1   # VPBS_ERR_INVALID


def with_word(a, i, value):
    a = np.array(a, np.uint64).reshape(-1).copy()
    a[i] = np.uint64(value)
    return a


def flip(a, i):
    a = np.array(a, np.uint64).reshape(-1)
    return with_word(a, i, int(a[i]) ^ 1)


def with_bytes(blob, at, word):
    b = bytearray(blob)
    b[at:at + 8] = int(word).to_bytes(8, "little")
    return bytes(b)


class Ring:
    """the circuit, four key sets and the proofs of five ciphertexts, ciphertext i under the key set of slot KEY_OF[i]: cases are
    (blob, testv, ct, out_ct)"""

    def __init__(self, ctx):
        self.ctx = ctx
        cyc, dum = (circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, N_LWE, LOG_N))
        self.cyc, self.dum = cyc, dum
        self.ivc = api.Ivc(ctx, cyc, dum, N, K, G)
        self.vk, _ = self.ivc.verifier_data()
        self.cap, self.digest, self.ncols = self.vk[4:].reshape(-1, 4), self.vk[:4], [cyc.n_constants + 80, 135, 20, 16]
        self.keys = [ctx.keygen(N, K, ELL, LOGB, N_LWE, seed, *SIGMAS) for seed in (77, 78, 79, 80)]
        self.hashes = [api.pbs_key_hash(k["bsk"], k["ksk"]) for k in self.keys]
        tv, self.delta = api.testv(N, 2)
        self.tv = np.asarray(tv, np.uint64)
        self.neg = np.array([(P - int(v)) % P for v in self.tv], np.uint64)      # a second test vector
        msgs = [1, 0, 1, 1, 0]
        cts = np.stack([np.asarray(api.lwe_encrypt(self.keys[0]["params"], self.keys[0]["s_lwe"], self.delta * m % P, nonce=10 + i), np.uint64)
                        for i, m in enumerate(msgs)])
        cts[2, 3] = np.uint64(P + 5)                                                # a mask word at or above p
        self.testvs = [self.tv, self.tv, self.tv, self.tv, self.neg]
        self.cases = [self.prove(self.testvs[i], cts[i], SLOT_KEYS[s]) for i, s in enumerate(KEY_OF)]
        self.fourth = self.prove(self.tv, cts[2], 3)                                # ciphertext 2 under the fourth key set
        self.memo = {}

    def prove(self, testv, ct, k):
        keys = self.keys[k]
        blob, _ = self.ivc.prove_pbs(testv, ct, keys["bsk"], keys["ksk"])
        acc_init = np.concatenate([np.zeros((K - 1, N), np.uint64), testv.reshape(1, N)])
        return blob, testv, ct, self.ctx.pbs_accumulator_chain(acc_init, ct, keys["bsk"], keys["ksk"], K, ELL, LOGB)[-1].reshape(-1)

    def shape(self, cap=None):
        return (self.ctx, self.cap if cap is None else cap, self.ncols, self.digest, LOG_N, self.cyc.n_constants, 80, self.cyc.gates, N, K, N_LWE, G)

    def ring_verifier(self, max_batch=5, slot_keys=SLOT_KEYS, cap=None):
        rv = api.RingVerifier(*self.shape(cap), max_keys=MAX_KEYS, max_batch=max_batch)
        for s, k in enumerate(slot_keys):
            if k is not None:
                rv.set_key(s, self.hashes[k])
        return rv

    def verifier(self, k, max_batch=5, cap=None):
        return api.PbsVerifier(*self.shape(cap), self.hashes[k], max_batch=max_batch)

    def host(self, case, k, cap=None):
        """api.verify_pbs under key set k -> (accepted, why), remembered"""
        blob, tv, ct, oc = case
        key = (bytes(blob), np.asarray(tv, np.uint64).tobytes(), np.asarray(ct, np.uint64).tobytes(), np.asarray(oc, np.uint64).tobytes(), k,
               None if cap is None else cap.tobytes())
        if key not in self.memo:
            self.memo[key] = api.verify_pbs(blob, self.cap if cap is None else cap, self.ncols, self.digest, LOG_N, self.cyc.n_constants, 80, self.cyc.gates,
                                            N, K, tv, ct, self.keys[k]["bsk"], self.keys[k]["ksk"], oc)
        return self.memo[key]

    def pi_offset(self, j):
        """byte offset of public input j in a serialised proof of this circuit"""
        return proof_layout(self.ncols, LOG_N, self.cyc.n_constants)["fixed_len"] + 8 + 8 * j


def unpack(cases):
    blobs, tvs, cts, outs = zip(*cases)
    return list(blobs), np.stack([np.asarray(t, np.uint64) for t in tvs]), np.stack(cts), np.stack([np.asarray(o, np.uint64).reshape(-1) for o in outs])


def check(S, rv, cases, key_of, slot_keys=SLOT_KEYS, cap=None, **how):
    """one ring run against the host, case by case, each under the key set of its slot -> (verdicts, reasons, proof_reasons)"""
    blobs, tvs, cts, outs = unpack(cases)
    v, r, sub = rv.verify(blobs, key_of, how.pop("testvs", tvs), cts, outs, **how)
    for i, case in enumerate(cases):
        ok, why = S.host(case, slot_keys[key_of[i]], cap)
        assert (bool(v[i]), api.pbs_reason_text(r[i])) == (ok, why), "case %d, slot %d: device (%d, %d), host (%s, %r)" % (i, key_of[i], v[i], r[i], ok, why)
        assert (sub[i] != api.VERIFY_OK) == (r[i] == api.PBS_PROOF), (i, r[i], sub[i])
    return v, r, sub


def per_slot(S, cases, key_of, slot_keys=SLOT_KEYS, cap=None):
    """the same batch through one PbsVerifier per slot, the results put back in the batch's order"""
    out = [np.zeros(len(cases), np.uint8) for _ in range(3)]
    for s in sorted(set(key_of)):
        mine = [i for i, k in enumerate(key_of) if k == s]
        blobs, tvs, cts, outs = unpack([cases[i] for i in mine])
        pv = S.verifier(slot_keys[s], max_batch=len(mine), cap=cap)
        got = pv.verify(blobs, tvs, cts, outs)
        pv.close()
        for a, g in zip(out, got):
            a[mine] = g
    return out


@pytest.fixture(scope="module")
def ring():
    """computed once, read by every test, never changed"""
    assert api.lib().vpbs_ring_verifier_run is not None
    c = vpbs_amd.Context(0, log_n_max=16)
    S = Ring(c)
    assert len({h.tobytes() for h in S.hashes}) == 4
    yield S
    S.ivc.free()
    c.close()


@pytest.fixture(scope="module")
def rv(ring):
    v = ring.ring_verifier()
    yield v
    v.close()


def test_a_mixed_batch_is_accepted_as_by_the_verifiers_of_its_slots(ring, rv):
    S = ring
    assert rv.count() == 4
    got = check(S, rv, S.cases, KEY_OF)
    assert got[0].all() and (got[1] == api.PBS_OK).all() and (got[2] == 0).all()
    for a, b in zip(got, per_slot(S, S.cases, KEY_OF)):
        assert a.tobytes() == b.tobytes()


def test_a_wrong_slot_is_a_wrong_key_hash(ring, rv):
    S = ring
    moved = KEY_OF[-2:] + KEY_OF[:-2]                      # [0, 3, 0, 3, 1]: the first two stay, the others get another client's slot
    assert [a == b for a, b in zip(moved, KEY_OF)] == [True, True, False, False, False]
    got = check(S, rv, S.cases, moved)
    assert got[0].tolist() == [1, 1, 0, 0, 0] and got[1].tolist() == [api.PBS_OK] * 2 + [api.PBS_KEY_HASH] * 3
    for a, b in zip(got, per_slot(S, S.cases, moved)):
        assert a.tobytes() == b.tobytes()
    # the slot that no proof of the batch was made under
    v, r, _ = check(S, rv, S.cases, [2] * 5)
    assert not v.any() and (r == api.PBS_KEY_HASH).all()


def forgeries(S, case):
    """one forged case per statement check, and per input the chains read -> [(name, case, the reason expected, or None: the host's)]"""
    blob, tv, ct, oc = case
    word = lambda j: int.from_bytes(blob[S.pi_offset(j):S.pi_offset(j) + 8], "little")
    other = lambda j: (word(j) ^ 1) if (word(j) ^ 1) < P else word(j) - 1      # another field element
    body = bytearray(blob)
    body[8 * 300] ^= 1
    return [("testv", (blob, flip(tv, N - 1), ct, oc), api.PBS_TESTV),
            ("mask", (with_bytes(blob, S.pi_offset(1), 1), tv, ct, oc), api.PBS_TESTV_MASK),
            ("counter", (with_bytes(blob, S.pi_offset(KN), N_LWE + 1), tv, ct, oc), api.PBS_COUNTER),
            ("out_ct", (blob, tv, ct, flip(oc, KN - 1)), api.PBS_OUT_CT),
            ("verifier data", (with_bytes(blob, S.pi_offset(2 * KN + 9), other(2 * KN + 9)), tv, ct, oc), api.PBS_PROOF),   # the proof fails first
            ("key hash", (with_bytes(blob, S.pi_offset(2 * KN + 4), other(2 * KN + 4)), tv, ct, oc), api.PBS_PROOF),
            ("ct", (blob, tv, flip(ct, N_LWE), oc), api.PBS_LWE_HASH),
            ("body", (bytes(body), tv, ct, oc), None)]


@pytest.mark.parametrize("at", [0, 2, 4])
def test_the_tables_are_read_for_the_row_itself(ring, rv, at):
    """a forged proof at the first, the middle and the last position among valid proofs of other slots: the forged row alone is rejected, with
    the host's reason, and its neighbours are accepted under their own slots"""
    S = ring
    assert KEY_OF[at] not in [KEY_OF[j] for j in (at - 1, at + 1) if 0 <= j < 5]
    for name, forged, want in forgeries(S, S.cases[at]):
        cases = list(S.cases)
        cases[at] = forged
        v, r, _ = check(S, rv, cases, KEY_OF)
        assert v.tolist() == [int(i != at) for i in range(5)], (name, v, r)
        assert want is None or r[at] == want, (name, r[at], want)


def test_verifier_data_of_another_circuit(ring):
    """a ring verifier that holds another cap: no proof is accepted -- it does not verify against that cap or, where its queries miss the
    changed entry, carries `another circuit's verifier data` -- as the host says under that cap, and as the verifiers of the slots say"""
    S = ring
    cap = S.cap.copy()
    cap[-1, 3] ^= np.uint64(1)
    other = S.ring_verifier(cap=cap)
    got = check(S, other, S.cases, KEY_OF, cap=cap)
    other.close()
    assert not got[0].any() and set(got[1].tolist()) <= {api.PBS_PROOF, api.PBS_VERIFIER_DATA}
    for a, b in zip(got, per_slot(S, S.cases, KEY_OF, cap=cap)):
        assert a.tobytes() == b.tobytes()


def test_test_vectors_through_an_index(ring, rv):
    S = ring
    table = np.stack([S.neg, S.tv])                                                   # proof 4 was made with `neg`, the others with `tv`
    v, r, _ = check(S, rv, S.cases, KEY_OF, testvs=table, testv_of=[1, 1, 1, 1, 0])
    assert v.all()
    # a wrong index is a wrong test vector for that row alone; the host is asked with the vector the index names
    wrong = [1, 0, 1, 1, 1]
    cases = [(c[0], table[t], c[2], c[3]) for c, t in zip(S.cases, wrong)]
    v, r, _ = check(S, rv, cases, KEY_OF, testvs=table, testv_of=wrong)
    assert v.tolist() == [1, 0, 1, 1, 0] and r[1] == r[4] == api.PBS_TESTV
    # no index, one vector per proof (check's default); no index, one vector for all
    assert check(S, rv, S.cases, KEY_OF)[0].all()
    cases = [(c[0], S.tv, c[2], c[3]) for c in S.cases]
    for shared in (S.tv, S.tv.reshape(1, N)):
        v, r, _ = check(S, rv, cases, KEY_OF, testvs=shared)
        assert v.tolist() == [1, 1, 1, 1, 0] and r[4] == api.PBS_TESTV
    with pytest.raises(ValueError, match="without testv_of"):
        rv.verify(*unpack(S.cases)[:1], KEY_OF, table, *unpack(S.cases)[2:])


def test_a_mask_word_at_or_above_p(ring, rv):
    """ciphertext 2 holds P + 5: the LWE chain reads its residue, as the host's does; with the residue itself in its place nothing changes"""
    S = ring
    blob, tv, ct, oc = S.cases[2]
    assert int(ct[3]) == P + 5
    cases = [S.cases[0], (blob, tv, with_word(ct, 3, 5), oc), S.cases[2], (blob, tv, with_word(ct, 3, 6), oc), (blob, tv, with_word(ct, 3, 2**64 - 1), oc)]
    v, r, _ = check(S, rv, cases, [0, 1, 1, 1, 1])
    assert v.tolist() == [1, 1, 1, 0, 0] and r[3] == r[4] == api.PBS_LWE_HASH


def test_batch_sizes(ring, rv):
    """count = max_batch (every run of `rv`), 65 proofs (above the 64 up to which the LWE chain has a stream of its own), and none"""
    S = ring
    big = S.ring_verifier(max_batch=65)
    mixed = list(S.cases)
    mixed[1] = (S.cases[1][0], S.cases[1][1], S.cases[1][2], flip(S.cases[1][3], 0))
    cases, key_of = (mixed * 13)[:65], (KEY_OF * 13)[:65]
    got = check(S, big, cases, key_of)
    assert got[0].tolist() == ([1, 0, 1, 1, 1] * 13)[:65] and int(got[0].sum()) == 52
    small = check(S, big, mixed, KEY_OF)                       # the same object below 64: the two-stream path
    assert all(np.tile(b, 13)[:65].tobytes() == a.tobytes() for a, b in zip(got, small))
    v, r, sub = big.verify([], [], S.tv, np.zeros((0, N_LWE + 1), np.uint64), np.zeros((0, K, N), np.uint64))
    assert v.size == r.size == sub.size == 0
    big.close()
    with pytest.raises(ValueError, match="exceed max_batch 5"):
        rv.verify(*[x for x in unpack(S.cases * 2)[:1]], KEY_OF * 2, *unpack(S.cases * 2)[1:])


def test_slots_change(ring):
    S = ring
    rv = S.ring_verifier(max_batch=6, slot_keys=[0, 1, None, 2])
    assert rv.count() == 3
    cases, key_of = S.cases + [S.fourth], KEY_OF + [1]                 # the sixth proof: made under the fourth key set, sent to slot 1
    try:
        v, r, _ = check(S, rv, cases, key_of, slot_keys=[0, 1, None, 2])
        assert v.tolist() == [1, 1, 1, 1, 1, 0] and r[5] == api.PBS_KEY_HASH
        rv.set_key(1, S.hashes[3])                                     # the fourth key set takes slot 1
        assert rv.count() == 3
        v, r, _ = check(S, rv, cases, key_of, slot_keys=[0, 3, None, 2])
        assert v.tolist() == [1, 1, 0, 1, 1, 1] and r[2] == api.PBS_KEY_HASH
        rv.clear_key(1)
        assert rv.count() == 2
        with pytest.raises(api.VpbsError, match=r"key_of\[2\] = 1: slot 1 is empty; proof 2 has no key hash") as e:
            rv.verify(*unpack(cases)[:1], key_of, *unpack(cases)[1:])
        assert e.value.status == INVALID
        with pytest.raises(api.VpbsError) as e:                        # an empty slot cannot be emptied
            rv.clear_key(1)
        assert e.value.status == INVALID and rv.count() == 2
        rv.set_key(1, S.hashes[1])
        assert rv.count() == 3 and check(S, rv, cases, key_of, slot_keys=[0, 1, None, 2])[0].tolist() == [1, 1, 1, 1, 1, 0]
    finally:
        rv.close()


def raw_run(rv, blobs, count, key_of, testvs, n_testv, testv_of, cts, outs, outputs, null=()):
    """vpbs_ring_verifier_run as the C ABI has it -> (status, message); `null`: the arguments passed as NULL"""
    buf, offs = api.pack_proofs(blobs)
    buf, offs = np.ascontiguousarray(buf, dtype=np.uint8), np.ascontiguousarray(offs, dtype=np.uint64)
    u8p, err = C.POINTER(C.c_uint8), C.create_string_buffer(512)
    ko = np.ascontiguousarray(key_of, dtype=np.uint32)
    to = None if testv_of is None else np.ascontiguousarray(testv_of, dtype=np.uint32)
    a = {"bytes": buf.ctypes.data_as(u8p), "offsets": offs.ctypes.data_as(C.POINTER(C.c_size_t)), "key_of": ko.ctypes.data, "testvs": api._ptr(testvs),
         "testv_of": None if to is None else to.ctypes.data, "ct": api._ptr(cts), "out_ct": api._ptr(outs), "verdicts": outputs[0].ctypes.data_as(u8p)}
    a.update({k: None for k in null})
    rc = api.lib().vpbs_ring_verifier_run(rv.h, a["bytes"], a["offsets"], count, a["key_of"], a["testvs"], n_testv, a["testv_of"], a["ct"], a["out_ct"],
                                          a["verdicts"], outputs[1].ctypes.data_as(u8p), outputs[2].ctypes.data_as(u8p), err, 512)
    return rc, err.value.decode()


def test_refusals(ring):
    S = ring
    rv = S.ring_verifier(slot_keys=[0, 1, 3, 2])
    rv.clear_key(2)                                                   # slot 2: emptied
    blobs, tvs, cts, outs = unpack(S.cases)
    tvs, cts, outs = (np.ascontiguousarray(x) for x in (tvs, cts, outs))
    outputs = [np.full(5, MARK, np.uint8) for _ in range(3)]
    untouched = lambda: all((o == MARK).all() for o in outputs)
    rc, msg = raw_run(rv, blobs, 5, [0, 3, 2, 0, 3], tvs, 5, None, cts, outs, outputs)
    assert rc == INVALID and "key_of[2] = 2" in msg and "slot 2 is empty" in msg and "proof 2" in msg and untouched(), msg
    rc, msg = raw_run(rv, blobs, 5, [0, 3, 1, 4, 3], tvs, 5, None, cts, outs, outputs)
    assert rc == INVALID and "key_of[3] = 4" in msg and "out of range (max_keys 4)" in msg and "proof 3" in msg and untouched(), msg
    rc, msg = raw_run(rv, blobs, 5, KEY_OF, tvs, 2, [0, 1, 1, 2, 0], cts, outs, outputs)
    assert rc == INVALID and "testv_of[3] = 2" in msg and "n_testv 2" in msg and "proof 3" in msg and untouched(), msg
    rc, msg = raw_run(rv, blobs, 5, KEY_OF, tvs, 3, None, cts, outs, outputs)          # NULL stands for i or for 0, and for nothing else
    assert rc == INVALID and "testv_of is null" in msg and untouched(), msg
    rc, msg = raw_run(rv, blobs + blobs[:1], 6, KEY_OF + [0], tvs, 1, None, cts, outs, outputs)
    assert rc == INVALID and "count 6 exceeds max_batch 5" in msg and untouched(), msg
    for name in ("offsets", "key_of", "testvs", "ct", "out_ct", "verdicts", "bytes"):
        rc, msg = raw_run(rv, blobs, 5, KEY_OF, tvs, 5, None, cts, outs, outputs, null=(name,))
        assert rc == INVALID and "null" in msg and untouched(), (name, msg)
    rc, msg = raw_run(rv, [], 0, [0], tvs, 1, None, cts, outs, outputs)
    assert rc == 0 and msg == "" and untouched()
    for max_keys in (0, 65536):
        with pytest.raises(api.VpbsError, match="max_keys must be 1 .. 65535"):
            api.RingVerifier(*S.shape(), max_keys=max_keys, max_batch=4)
    with pytest.raises(api.VpbsError) as e:                            # a slot the object does not have
        rv.set_key(MAX_KEYS, S.hashes[0])
    assert e.value.status == INVALID and rv.count() == 3
    # the Python form: the message and the status, and the object goes on working
    with pytest.raises(api.VpbsError, match=r"key_of\[2\] = 2: slot 2 is empty; proof 2 has no key hash, nothing was queued") as e:
        rv.verify(blobs, [0, 3, 2, 0, 3], tvs, cts, outs)
    assert e.value.status == INVALID
    assert check(S, rv, S.cases, KEY_OF)[0].all()
    rv.close()


# 3 inputs (wires 0 1 2), 4 gates (wires 3 .. 6), 2 levels, 2 lookup tables; gate 2 reads gate 0 and gate 1 with the coefficients 3 and p - 2
FOUR = [([(0, 1)], 0, 0), ([(1, 1), (2, P - 1)], 7, 1), ([(3, 3), (4, P - 2)], 5, 0), ([(2, 1)], 0, 1)]
INSTANCE_KEYS = [2, 0, 2]


@pytest.fixture(scope="module")
def program(ring):
    """the program for three instances on a ring prover of three key sets (slot k = key set k): prove_batch's proofs and outputs"""
    S = ring
    testvs = np.stack([S.tv, S.neg])
    inputs = np.array([[api.lwe_encrypt(S.keys[k]["params"], S.keys[k]["s_lwe"], S.delta * m % P, nonce=40 + 3 * b + j)
                        for j, m in enumerate(((b + 1) % 2, b % 2, 1))] for b, k in enumerate(INSTANCE_KEYS)], np.uint64)
    inputs[2, 1, 2] = np.uint64(P + 3)                                # an input word at or above p: reduced on read
    prog = api.Program(S.ctx, 3, FOUR, 2)
    assert prog.levels()[1] == 2
    rp = api.RingProver(0, S.cyc, S.dum, K, ELL, LOGB, N, N_LWE, max_keys=3, chains=3, witness_batch=3)
    assert [rp.add(S.keys[k]["bsk"], S.keys[k]["ksk"]) for k in range(3)] == [0, 1, 2]
    proofs, wires, out_cts = prog.prove_batch(rp, inputs, INSTANCE_KEYS, testvs)
    assert all((rp.key_hash(k) == S.hashes[k]).all() for k in range(3))
    rp.close()
    yield dict(prog=prog, inputs=inputs, testvs=testvs, proofs=proofs, out_cts=out_cts)
    prog.close()


def per_instance(S, Q, key_of, out_cts):
    """Program.verify of every instance with the PbsVerifier of its slot -> three [instances][n_gates] arrays"""
    pvs = {k: S.verifier(k, max_batch=4) for k in set(key_of)}
    rows = [Q["prog"].verify(pvs[k], Q["inputs"][b], Q["testvs"], out_cts[b], Q["proofs"][b]) for b, k in enumerate(key_of)]
    for pv in pvs.values():
        pv.close()
    return [np.stack([r[j] for r in rows]) for j in range(3)]


def test_program_verify_batch_is_program_verify_per_instance(ring, program):
    S, Q = ring, program
    rv = api.RingVerifier(*S.shape(), max_keys=3, max_batch=5)        # 12 rows in chunks of 5: a chunk straddles instances
    for k in range(3):
        rv.set_key(k, S.hashes[k])
    run = lambda key_of, out_cts: Q["prog"].verify_batch(rv, Q["inputs"], key_of, Q["testvs"], out_cts, Q["proofs"])
    got = run(INSTANCE_KEYS, Q["out_cts"])
    assert got[0].shape == (3, 4) and got[0].all() and (got[1] == api.PBS_OK).all()
    for a, b in zip(got, per_instance(S, Q, INSTANCE_KEYS, Q["out_cts"])):
        assert a.tobytes() == b.tobytes()
    # one forged output: instance 1, gate 0 -- wire 3, which gate 2 reads
    forged = Q["out_cts"].copy()
    forged[1, 0, 0, 3] ^= np.uint64(1)
    got = run(INSTANCE_KEYS, forged)
    assert got[0].tolist() == [[1, 1, 1, 1], [0, 1, 0, 1], [1, 1, 1, 1]]
    assert got[1][1, 0] == api.PBS_OUT_CT and got[1][1, 2] == api.PBS_LWE_HASH
    for a, b in zip(got, per_instance(S, Q, INSTANCE_KEYS, forged)):
        assert a.tobytes() == b.tobytes()
    # two instances' slots swapped: every gate of both is rejected, the third instance stays
    swapped = [0, 2, 2]
    got = run(swapped, Q["out_cts"])
    assert got[0].tolist() == [[0] * 4, [0] * 4, [1] * 4] and (got[1][:2] == api.PBS_KEY_HASH).all()
    for a, b in zip(got, per_instance(S, Q, swapped, Q["out_cts"])):
        assert a.tobytes() == b.tobytes()
    # refusals: the instance and the slot in the message, nothing run
    rv.clear_key(0)
    with pytest.raises(api.VpbsError, match=r"key_of\[1\] = 0: slot 0 is empty; instance 1 has no key hash") as e:
        run(INSTANCE_KEYS, Q["out_cts"])
    assert e.value.status == INVALID
    with pytest.raises(ValueError, match=r"key_of\[0\] = 3 is not a slot of a ring of 3"):
        run([3, 0, 2], Q["out_cts"])
    with pytest.raises(ValueError, match=r"expected inputs \[instances\]\[3\]\[7\]"):
        Q["prog"].verify_batch(rv, Q["inputs"][:, :2], INSTANCE_KEYS, Q["testvs"], Q["out_cts"], Q["proofs"])
    v, r, sub = Q["prog"].verify_batch(rv, Q["inputs"][:0], [], Q["testvs"], Q["out_cts"][:0], [])
    assert v.shape == (0, 4)
    rv.set_key(0, S.hashes[0])
    assert run(INSTANCE_KEYS, Q["out_cts"])[0].all()                   # and the objects go on working
    rv.close()


def tool(*argv):
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "tools", argv[0])] + list(argv[1:]), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_tools_verify_through_one_ring_verifier():
    export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, N_LWE, LOG_N)
    a = tool("prove_batch.py", "--n8", "--keys", "2", "--count", "3", "--chains", "2", "--witness-batch", "3")
    assert (a["count"], a["keys"], a["proofs"], a["accepted"], a["rejected_because"], a["decrypted_correct"]) == (3, 2, 3, 3, [], 3), a
    a = tool("run_program.py", "--n8", "--levels", "1", "--width", "2", "--instances", "2", "--keys", "2", "--prove", "--verify-per-instance")
    assert (a["instances"], a["keys"], a["gates"], a["verified"], a["rejected_because"], a["proven"]) == (2, 2, 2, 4, [], True), a
    assert a["verify_seconds"] > 0 and a["verify_per_instance_seconds"] > 0 and a["verify_per_instance_equal"] is True
