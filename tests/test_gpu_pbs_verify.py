"""GPU tests (-m gpu) of the batch verifier of whole vPBS proofs (vpbs_pbs_verifier_*, csrc/verify_pbs_batch.hip).  The yardstick throughout
is the host's api.verify_pbs on the same bytes, test vector, ciphertexts and keys: the device must give every proof the host's verdict and,
through pbs_reason_text, the host's `why`."""
import json
import os
import subprocess
import sys

import ctypes as C
import numpy as np
import pytest

import export_circuits
import vpbs_amd
from batch_verify_layout import proof_layout
from vpbs_amd import api, circuit_file

pytestmark = pytest.mark.gpu
P = api.P
K, ELL, LOGB = 2, 4, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)
ERR_INVALID = -1   # VPBS_ERR_INVALID


class Pbs:
    """one cyclic circuit, one key set and the vPBS proofs made with them: cases are (blob, testv, ct, out_ct)"""

    def __init__(self, ctx, N, n_lwe, log_n, seed, messages):
        self.ctx, self.N, self.n_lwe, self.log_n = ctx, N, n_lwe, log_n
        cyc, dum = (circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, n_lwe, log_n))
        self.ivc = api.Ivc(ctx, cyc, dum, N, K, K * ELL * K * N)
        vk, _ = self.ivc.verifier_data()
        self.cap, self.digest, self.n_constants, self.gates = vk[4:].reshape(-1, 4), vk[:4], cyc.n_constants, cyc.gates
        self.ncols = [cyc.n_constants + 80, 135, 20, 16]
        self.keys = ctx.keygen(N, K, ELL, LOGB, n_lwe, seed, *SIGMAS)
        self.testv, self.delta = api.testv(N, 2)
        self.testv = np.asarray(self.testv, np.uint64)
        self.acc_init = np.concatenate([np.zeros((K - 1, N), np.uint64), self.testv.reshape(1, N)])
        self.cases = [self.prove(m, nonce) for nonce, m in enumerate(messages)]

    def prove(self, message, nonce, steps=0):
        ct = np.asarray(api.lwe_encrypt(self.keys["params"], self.keys["s_lwe"], self.delta * message % P, nonce=nonce), np.uint64)
        blob, _ = self.ivc.prove_pbs(self.testv, ct, self.keys["bsk"], self.keys["ksk"], steps)
        accs = self.ctx.pbs_accumulator_chain(self.acc_init, ct, self.keys["bsk"], self.keys["ksk"], K, ELL, LOGB)
        return blob, self.testv, ct, accs[(steps or self.n_lwe + 2) - 1]

    def verifier(self, key_hash=None, max_batch=512, cap=None, digest=None):
        kh = api.pbs_key_hash(self.keys["bsk"], self.keys["ksk"]) if key_hash is None else key_hash
        return api.PbsVerifier(self.ctx, self.cap if cap is None else cap, self.ncols, self.digest if digest is None else digest, self.log_n,
                               self.n_constants, 80, self.gates, self.N, K, self.n_lwe, K * ELL * K * self.N, kh, max_batch=max_batch)

    def host(self, blob, testv, ct, out_ct, keys=None):
        keys = keys or self.keys
        return api.verify_pbs(blob, self.cap, self.ncols, self.digest, self.log_n, self.n_constants, 80, self.gates, self.N, K, testv, ct,
                              keys["bsk"], keys["ksk"], out_ct)

    def pi_offset(self, j):
        """byte offset of public input j in a serialised proof of this circuit"""
        return proof_layout(self.ncols, self.log_n, self.n_constants)["fixed_len"] + 8 + 8 * j


def check(S, pv, cases, shared_testv=False, keys=None):
    """device batch against the host, case by case -> (verdicts, reasons, proof_reasons)"""
    blobs, tvs, cts, outs = zip(*cases)
    testv = np.asarray(tvs[0], np.uint64) if shared_testv else np.stack([np.asarray(t, np.uint64) for t in tvs])
    v, r, sub = pv.verify(list(blobs), testv, np.stack(cts), np.stack([np.asarray(o, np.uint64).reshape(-1) for o in outs]))
    memo = {}
    for k, (blob, tv, ct, oc) in enumerate(cases):
        key = (bytes(blob), np.asarray(tv, np.uint64).tobytes(), np.asarray(ct, np.uint64).tobytes(), np.asarray(oc, np.uint64).tobytes())
        if key not in memo:
            memo[key] = S.host(blob, tv, ct, oc, keys)
        ok, why = memo[key]
        assert (bool(v[k]), api.pbs_reason_text(r[k])) == (ok, why), "case %d: device (%d, %d), host (%s, %r)" % (k, v[k], r[k], ok, why)
        assert (sub[k] != api.VERIFY_OK) == (r[k] == api.PBS_PROOF), (k, r[k], sub[k])
    return v, r, sub


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


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pbs(ctx):
    """six PBS at N = 8, n = 6 under one key set: different ciphertexts and messages"""
    S = Pbs(ctx, 8, 6, 13, 91, [1, 0, 1, 1, 0, 0])
    yield S
    S.ivc.free()


@pytest.fixture(scope="module")
def pv(pbs):
    v = pbs.verifier()
    yield v
    v.close()


def test_pbs_verifier_accepts_valid_proofs(pbs, pv):
    v, r, sub = check(pbs, pv, pbs.cases)
    assert v.all() and (r == api.PBS_OK).all() and (sub == 0).all()
    v, r, _ = check(pbs, pv, pbs.cases, shared_testv=True)
    assert v.all()
    assert api.pbs_key_hash(pbs.keys["bsk"], pbs.keys["ksk"]).tolist() == \
        api.hash_chain(np.vstack([np.zeros(K * ELL * K * pbs.N, np.uint64), pbs.keys["bsk"], pbs.keys["ksk"]]))[0].tolist()


def test_statement_sweeps_match_the_host(pbs, pv):
    n, kn = pbs.n_lwe, K * pbs.N
    c0, c1 = pbs.cases[0], pbs.cases[1]
    cases = [(c0[0], c0[1], c1[2], c0[3]),                     # another proof's ct
             (c0[0], c0[1], c0[2], c1[3])]                     # another proof's out_ct
    cases += [(c0[0], c0[1], flip(c0[2], i), c0[3]) for i in range(n + 1)]          # one word of ct, the body ct[n] included
    cases += [(c0[0], c0[1], c0[2], flip(c0[3], i)) for i in (0, 3, pbs.N, kn - 1)]
    cases += [(c0[0], flip(c0[1], i), c0[2], c0[3]) for i in (0, pbs.N - 1)]       # a wrong per-proof testv
    for bad in (P, 2**64 - 1):                                 # non-canonical words in each input
        for i in (0, n):
            cases.append((c0[0], c0[1], with_word(c0[2], i, bad), c0[3]))
            # ... and the same residue: the LWE chain reads it as the host's permutation does
            cases.append((c0[0], c0[1], with_word(c0[2], i, bad % P), c0[3]))
        cases.append((c0[0], c0[1], c0[2], with_word(c0[3], kn - 1, bad)))
        cases.append((c0[0], with_word(c0[1], 2, bad), c0[2], c0[3]))
    cases += pbs.cases
    v, r, _ = check(pbs, pv, cases)
    assert r[0] == api.PBS_LWE_HASH and r[1] == api.PBS_OUT_CT and v[-len(pbs.cases):].all()
    assert (r[2:2 + n + 1] == api.PBS_LWE_HASH).all()
    # a wrong SHARED test vector rejects every proof
    wrong = [(b, flip(tv, 1), ct, oc) for b, tv, ct, oc in pbs.cases]
    v, r, _ = check(pbs, pv, wrong, shared_testv=True)
    assert not v.any() and (r == api.PBS_TESTV).all()


def test_byte_sweeps_match_the_host_in_its_order(pbs, pv):
    """corrupted words in each public-input region and each proof section, cut bytes, a count that is too low or too high"""
    blob, tv, ct, oc = pbs.cases[2]
    kn, N = K * pbs.N, pbs.N
    regions = {"mask": [0, kn - N - 1], "testv": [kn - N, kn - 1], "counter": [kn], "accumulator": [kn + 1, 2 * kn], "key hash": [2 * kn + 1, 2 * kn + 4],
               "lwe hash": [2 * kn + 5, 2 * kn + 8], "digest": [2 * kn + 9, 2 * kn + 12], "cap": [2 * kn + 13, 2 * kn + 13 + 63]}
    want = {"mask": api.PBS_TESTV_MASK, "testv": api.PBS_TESTV, "counter": api.PBS_COUNTER, "accumulator": api.PBS_OUT_CT}
    cases, expect = [], []
    for name, idx in regions.items():
        for j in idx:
            at = pbs.pi_offset(j)
            w = int.from_bytes(blob[at:at + 8], "little")
            cases.append((with_bytes(blob, at, (w ^ 1) if (w ^ 1) < P else w - 1), tv, ct, oc))
            expect.append(want.get(name, api.PBS_PROOF))   # the public-input hash changes: the proof fails before the later checks
            cases.append((with_bytes(blob, at, P), tv, ct, oc))   # not a field element: malformed
            expect.append(api.PBS_MALFORMED)
    lay = proof_layout(pbs.ncols, pbs.log_n, pbs.n_constants)
    sections = {}
    for sec, at in lay["words"]:
        sections.setdefault(sec, []).append(at)
    for sec, offs in sections.items():
        for at in (offs[0], offs[len(offs) // 2], offs[-1]):
            w = int.from_bytes(blob[at:at + 8], "little")
            cases.append((with_bytes(blob, at, (w ^ 1) if (w ^ 1) < P else w - 1), tv, ct, oc))
            expect.append(None)
    for at in (lay["len_bytes"][0], lay["len_bytes"][-1]):
        b = bytearray(blob)
        b[at] ^= 1
        cases.append((bytes(b), tv, ct, oc))
        expect.append(api.PBS_MALFORMED)
    cases.append((with_bytes(blob, lay["pow"], int.from_bytes(blob[lay["pow"]:lay["pow"] + 8], "little") ^ 1), tv, ct, oc))
    expect.append(None)
    n_pi = 2 * kn + 13 + 64
    count_at = lay["fixed_len"]
    cases += [(blob[:-8], tv, ct, oc), (blob[:-1], tv, ct, oc), (blob[:count_at], tv, ct, oc), (b"", tv, ct, oc),
              (with_bytes(blob, count_at, n_pi + 1) + (5).to_bytes(8, "little"), tv, ct, oc),   # one public input appended
              (with_bytes(blob, count_at, n_pi - 1)[:-8], tv, ct, oc),                           # one too few (from_bytes must return n_pi)
              (blob + b"\0" * 8, tv, ct, oc)]
    expect += [api.PBS_MALFORMED] * 7
    cases.append((blob, tv, ct, oc))
    expect.append(api.PBS_OK)
    v, r, _ = check(pbs, pv, cases)
    for k, e in enumerate(expect):
        if e is not None:
            assert r[k] == e, (k, r[k], e)
        else:
            assert r[k] in (api.PBS_PROOF, api.PBS_MALFORMED), (k, r[k])


def test_counter_of_a_prefix_proof(pbs, pv):
    prefix = pbs.prove(1, 40, steps=pbs.n_lwe)
    v, r, _ = check(pbs, pv, [prefix, pbs.cases[0]])
    assert list(r) == [api.PBS_COUNTER, api.PBS_OK]


def test_other_keys_and_another_circuit(ctx, pbs, pv):
    other = ctx.keygen(pbs.N, K, ELL, LOGB, pbs.n_lwe, 92, *SIGMAS)
    pv2 = pbs.verifier(key_hash=api.pbs_key_hash(other["bsk"], other["ksk"]))
    v, r, _ = check(pbs, pv2, pbs.cases, keys=other)
    assert not v.any() and (r == api.PBS_KEY_HASH).all()
    pv2.close()
    # a proof of another cyclic circuit (n = 1): its ciphertext padded to this verifier's n + 1 words
    S1 = Pbs(ctx, 8, 1, 13, 93, [1])
    blob1, tv1, ct1, oc1 = S1.cases[0]
    ct_pad = np.concatenate([ct1[:1], np.zeros(pbs.n_lwe - 1, np.uint64), ct1[1:]])
    v, r, _ = check(pbs, pv, [(blob1, tv1, ct_pad, oc1), pbs.cases[0]])
    assert not v[0] and v[1]
    # ... and this circuit's proofs under a verifier that holds the other circuit's verifier data
    pv3 = pbs.verifier(cap=S1.cap, digest=S1.digest)
    S1.ivc.free()
    blobs, tvs, cts, ocs = zip(*pbs.cases[:2])
    v3, r3, _ = pv3.verify(list(blobs), pbs.testv, np.stack(cts), np.stack(ocs))
    for k in range(2):
        ok, why = api.verify_pbs(blobs[k], S1.cap, pbs.ncols, S1.digest, pbs.log_n, pbs.n_constants, 80, pbs.gates, pbs.N, K, pbs.testv, cts[k],
                                 pbs.keys["bsk"], pbs.keys["ksk"], ocs[k])
        assert (bool(v3[k]), api.pbs_reason_text(r3[k])) == (ok, why)
    pv3.close()


def test_batch_shapes_and_errors(ctx, pbs):
    pv = pbs.verifier(max_batch=4)
    blobs, tvs, cts, ocs = zip(*pbs.cases)
    v, r, sub = pv.verify([], pbs.testv, np.zeros((0, pbs.n_lwe + 1), np.uint64), np.zeros((0, K, pbs.N), np.uint64))
    assert v.size == 0
    check(pbs, pv, pbs.cases[:1])
    mixed = [pbs.cases[0], (blobs[1], tvs[1], cts[2], ocs[1]), pbs.cases[3], (blobs[4][:-3], tvs[4], cts[4], ocs[4])]   # exactly max_batch
    first = check(pbs, pv, mixed)
    assert list(first[0]) == [1, 0, 1, 0]
    for _ in range(2):   # repeated runs on one object
        again = pv.verify([c[0] for c in mixed], np.stack([c[1] for c in mixed]), np.stack([c[2] for c in mixed]), np.stack([c[3] for c in mixed]))
        assert all((a == b).all() for a, b in zip(first, again))
    # above 64 proofs the LWE chain runs on the context's stream, up to 64 on a stream of its own beside the proof's stages: the same verdicts
    big = pbs.verifier(max_batch=200)
    v_big, r_big, _ = check(pbs, big, (mixed * 40)[:130])
    assert (v_big == np.tile(first[0], 40)[:130]).all() and (r_big == np.tile(first[1], 40)[:130]).all()
    big.close()
    with pytest.raises(api.VpbsError):   # above max_batch
        pv.verify(list(blobs[:5]), pbs.testv, np.stack(cts[:5]), np.stack(ocs[:5]))
    # NULL ct or out_ct through the C ABI
    buf, offs = api.pack_proofs(list(blobs[:2]))
    out = np.zeros(2, np.uint8)
    u8p = C.POINTER(C.c_uint8)
    tv = np.ascontiguousarray(pbs.testv)
    c2, o2 = np.ascontiguousarray(np.stack(cts[:2])), np.ascontiguousarray(np.stack(ocs[:2]))
    run = lambda ct_p, oc_p: api.lib().vpbs_pbs_verifier_run(pv.h, buf.ctypes.data_as(u8p), offs.ctypes.data_as(C.POINTER(C.c_size_t)), 2,
                                                              api._ptr(tv), 0, ct_p, oc_p, out.ctypes.data_as(u8p), None, None)
    assert run(None, api._ptr(o2)) == ERR_INVALID and run(api._ptr(c2), None) == ERR_INVALID
    assert run(api._ptr(c2), api._ptr(o2)) == 2 and out.all()
    pv.close()
    with pytest.raises(api.VpbsError):   # max_batch 0
        pbs.verifier(max_batch=0)


def test_paper_size_batch_of_64(ctx):
    """two vPBS at N = 1024, n = 728 (the paper's parameters), replicated to a batch of 64 with some corrupted: the host's verdicts"""
    S = Pbs(ctx, 1024, 728, 16, 0x5EED, [1, 0])
    pv = S.verifier(max_batch=64)
    kn = K * S.N
    (b0, tv, c0, o0), (b1, _, c1, o1) = S.cases
    cases = [S.cases[k % 2] for k in range(64)]
    cases[5] = (b0, tv, flip(c0, 728), o0)              # the body of ct
    cases[9] = (b1, tv, flip(c1, 17), o1)
    cases[13] = (b0, tv, c0, flip(o0, kn - 1))
    cases[21] = (b1, flip(tv, 3), c1, o1)
    cases[34] = (with_bytes(b0, S.pi_offset(kn), 5), tv, c0, o0)   # the counter
    cases[55] = (b1[:-8], tv, c1, o1)
    bb = bytearray(b0)
    bb[8 * 300] ^= 1
    cases[60] = (bytes(bb), tv, c0, o0)
    v, r, _ = check(S, pv, cases)
    assert int(v.sum()) == 57 and r[5] == api.PBS_LWE_HASH and r[34] == api.PBS_COUNTER
    pv.close()
    S.ivc.free()


def test_prove_ivc_tool_with_the_device_pbs_verifier():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "prove_ivc.py"), "8", "6", "13"], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, VPBS_IVC_VERIFY="device", VPBS_IVC_CHAINS="3"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    dv = line["device_pbs_verify"]
    assert dv["verdicts"] == [1, 1, 1] and dv["reasons"] == [""] * 3 and dv["ms"] > 0
