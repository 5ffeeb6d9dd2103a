"""GPU tests (-m gpu): one proof per program instance and many aggregates in one device run.
  many-run   AggregateVerifier.roots_many on random statements against api.aggregate_root and the single-run AggregateVerifier.root, tree by
             tree, at shapes chosen for where the LWE hash falls in its sponge blocks and for which half of the leaf-pair kernel finishes
             first; AggregateVerifier.verify_many on real aggregates (the world of tests/test_gpu_aggregate.py, rebuilt here) against
             api.verify_aggregate and AggregateVerifier.verify on every slice.
  programs   Program.prove_aggregate / prove_aggregate_batch against the composition Aggregator.aggregate(Program.prove(..)), the host's
             api.program_verify_aggregate against Program.verify_aggregate_batch, forgeries of every part of the statement, the refusal of
             a program with more gates than leaves, and tools/run_program.py --prove --aggregate.
Exact field arithmetic: word for word, byte for byte."""
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
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, ELL, LOGB = 2, 4, 5
N, LOG_N, LEVELS = 8, 13, 3
KN = K * N
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    yield c
    c.close()


# ================= many aggregates in one run: N = 8, n = 1 =================
N_LWE = 1
KEY_OF = [0, 1, 1]          # leaf i was proven under the key set of slot KEY_OF[i]
TESTV_OF = [0, 0, 1]


class World:
    """three vPBS proofs under two key sets from one RingProver, the Aggregator over the exported level circuits, the aggregates of
    proofs[:2], proofs[:3] and proofs[:1], and a verifier of up to 8 aggregates over 32 leaves; computed once, read by every test"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.cyc, self.dum = (circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, N_LWE, LOG_N))
        self.levels = [circuit_file.load(p) for p in export_circuits.ensure_aggregate_circuits(N, K, ELL, LOGB, N_LWE, LOG_N, LEVELS)]
        rp = api.RingProver(0, self.cyc, self.dum, K, ELL, LOGB, N, N_LWE, max_keys=2, chains=2, witness_batch=3)
        keys = [ctx.keygen(N, K, ELL, LOGB, N_LWE, seed, *SIGMAS) for seed in (31, 32)]
        assert [rp.add(k["bsk"], k["ksk"]) for k in keys] == [0, 1]
        tv, delta = api.testv(N, 2)
        tv = np.asarray(tv, np.uint64)
        self.testvs = np.stack([tv, np.array([(P - int(v)) % P for v in tv], np.uint64)])
        self.cts = np.stack([np.asarray(api.lwe_encrypt(keys[k]["params"], keys[k]["s_lwe"], delta * (i % 2) % P, nonce=20 + i), np.uint64)
                             for i, k in enumerate(KEY_OF)])
        self.proofs, out_ct, _ = rp.prove(self.cts, KEY_OF, self.testvs[TESTV_OF])
        self.out_cts = out_ct.reshape(3, KN)
        self.key_hashes = np.stack([rp.key_hash(0), rp.key_hash(1)])
        self.vk0 = rp.verifier_data()[0]
        rp.close()
        self.agg = api.Aggregator(ctx, self.cyc, self.vk0, self.levels)
        self.vks = self.agg.verifier_data()
        self.shape = api.AggregateShape(N, K, N_LWE, self.vks, self.levels)
        self.av = api.AggregateVerifier(ctx, self.shape, max_leaves=32, max_aggregates=8)
        self.counts = [2, 3, 1]
        self.blobs = [self.agg.aggregate(self.proofs[:c]) for c in self.counts]

    def slices(self, counts):
        """the statement of trees over proofs[:c] for c in counts, leaf arrays concatenated"""
        idx = [i for c in counts for i in range(c)]
        return (self.testvs, self.cts[idx], self.out_cts[idx], self.key_hashes, [KEY_OF[i] for i in idx], [TESTV_OF[i] for i in idx])

    def one_by_one(self, blobs, counts, st):
        """(verdicts, reasons) of api.verify_aggregate and of the single-run AggregateVerifier.verify on every slice, which must agree"""
        tvs, cts, ocs, khs, ko, to = st
        out, at = [], 0
        for blob, c in zip(blobs, counts):
            sl = (tvs, cts[at:at + c], ocs[at:at + c], khs, ko[at:at + c], to[at:at + c])
            host = api.verify_aggregate(self.shape, blob, c, *sl)
            assert self.av.verify(blob, c, *sl) == host
            out.append(host)
            at += c
        return [int(ok) for ok, _ in out], [r for _, r in out]

    def close(self):
        self.av.close()
        self.agg.close()


@pytest.fixture(scope="module")
def world(ctx):
    w = World(ctx)
    yield w
    w.close()


TREES = [1, 2, 3, 5, 8, 4]   # depths 1 1 2 3 3 2: one-leaf and exact-power-of-two trees included; 23 leaves


# (N, K, n_lwe): F = (2 K N + 5) div 8 full blocks before the LWE hash, n_lwe + 2 chain links
#   (8, 2, 1)   F 4, 3 links: the sponge half is longer          (8, 2, 6)  F 4, 8 links and (8, 2, 40): the chain half is longer
#   (4, 3, 5)   2 K N + 5 = 29: the hash straddles blocks 3 and 4 at offset 5       (2, 3, 2)  17: the hash inside block 2
#   (1, 1, 1)   F 0: every block follows the chain
@pytest.mark.parametrize("n_,k_,lwe", [(8, 2, 1), (8, 2, 6), (8, 2, 40), (4, 3, 5), (2, 3, 2), (1, 1, 1)])
def test_roots_many_on_random_statements(world, n_, k_, lwe):
    """six trees in ONE run against api.aggregate_root and the single-run root per tree: key_of / testv_of repeated and out of order, ct
    words p - 1, p and 2^64 - 1, host arrays and device pointers; one out_ct word = p flags its own tree only"""
    W = world
    shape = api.AggregateShape(n_, k_, lwe, W.vks, W.levels)    # the level circuits only size the proof verifiers: no proof is read
    av = api.AggregateVerifier(W.ctx, shape, max_leaves=32, max_aggregates=8)
    rng = np.random.default_rng(1000 * n_ + 10 * k_ + lwe)
    f = lambda *s: rng.integers(0, P, size=s, dtype=np.uint64)
    total = sum(TREES)
    testvs, cts, out_cts, key_hashes = f(3, n_), f(total, lwe + 1), f(total, k_ * n_), f(4, 4)
    cts[0, 0], cts[1, lwe], cts[7, 0] = np.uint64(P - 1), np.uint64(P), np.uint64(2 ** 64 - 1)
    key_of = rng.integers(0, 4, size=total).astype(np.uint32)
    testv_of = rng.integers(0, 3, size=total).astype(np.uint32)
    key_of[:4], testv_of[:4] = [3, 0, 3, 1], [2, 2, 0, 2]
    first = np.concatenate([[0], np.cumsum(TREES)])
    want = []
    for a, c in enumerate(TREES):
        sl = slice(first[a], first[a + 1])
        st = (testvs, cts[sl], out_cts[sl], key_hashes, key_of[sl], testv_of[sl])
        want.append(api.aggregate_root(n_, k_, lwe, W.vk0, *st))
        assert (av.root(*st) == want[-1]).all(), a
    want = np.stack(want)
    roots, bad = av.roots_many(TREES, testvs, cts, out_cts, key_hashes, key_of, testv_of)
    assert bad.tolist() == [0] * 6 and (roots == want).all(), np.argwhere(roots != want)[:4].tolist()
    d = [W.ctx.device_upload_new(a) for a in (testvs, cts, out_cts, key_hashes)]
    try:
        roots, bad = av.roots_many(TREES, d[0], d[1], d[2], d[3], key_of, testv_of, on_device=True, n_testv=3, n_keys=4)
    finally:
        for p in d:
            W.ctx.device_free(p)
    assert bad.tolist() == [0] * 6 and (roots == want).all()
    # a raw word = p in the third tree: that tree alone is flagged, every other root is right
    forged = out_cts.copy()
    forged[first[2] + 1, k_ * n_ - 1] = np.uint64(P)
    roots, bad = av.roots_many(TREES, testvs, cts, forged, key_hashes, key_of, testv_of)
    assert bad.tolist() == [0, 0, 1, 0, 0, 0]
    keep = [0, 1, 3, 4, 5]
    assert (roots[keep] == want[keep]).all()
    with pytest.raises(api.VpbsError, match="not a field element"):
        api.aggregate_root(n_, k_, lwe, W.vk0, testvs, cts[first[2]:first[3]], forged[first[2]:first[3]], key_hashes, key_of[first[2]:first[3]],
                           testv_of[first[2]:first[3]])
    av.close()


def test_many_run_refusals_by_name(world):
    W = world
    f = lambda *s: np.zeros(s, np.uint64)
    st = lambda total: (f(1, N), f(total, N_LWE + 1), f(total, KN), f(1, 4))
    with pytest.raises(ValueError, match="tree 1 is empty"):
        W.av.roots_many([2, 0], *st(2))
    with pytest.raises(ValueError, match=r"tree 0: 9 leaves exceed 2\^levels = 8"):
        W.av.roots_many([9], *st(9))
    with pytest.raises(ValueError, match="exceed max_leaves 32"):
        W.av.roots_many([8, 8, 8, 8, 1], *st(33))
    with pytest.raises(ValueError, match="exceed max_aggregates 8"):
        W.av.roots_many([1] * 9, *st(9))
    # the same from the C ABI, which a caller may reach without the Python checks
    L, err = api.lib(), api.C.create_string_buffer(256)
    szp = lambda a: np.array(a, np.uint64).ctypes.data_as(api.C.POINTER(api.C.c_size_t))
    out, bad = np.zeros(4 * 9, np.uint64), np.zeros(9, np.uint8)
    bp = bad.ctypes.data_as(api.C.POINTER(api.C.c_uint8))

    def refused(first, key_of=None, total=None):
        tv, c, o, kh = st(total if total is not None else first[-1])
        ko = np.array([0] if key_of is None else key_of, np.uint32)
        rc = L.vpbs_aggregate_verifier_roots_many(W.av.h, len(first) - 1, szp(first), tv.ctypes.data, 1, None, c.ctypes.data, o.ctypes.data, kh.ctypes.data,
                                                  1, None if key_of is None else ko.ctypes.data, 0, api._ptr(out), bp, err, 256)
        assert rc == api.ERR_INVALID
        return err.value.decode()
    assert "tree 1 is empty" in refused([0, 2, 2], total=2)
    assert "tree 0: 9 leaves exceed 2^levels = 8" in refused([0, 9])
    assert "exceeds max_leaves 32" in refused([0, 8, 16, 24, 32, 33])
    assert "n_agg 9 exceeds max_aggregates 8" in refused(list(range(10)))
    assert "key_of[1] = 1 is not below n_keys 1" in refused([0, 2], key_of=[0, 1])
    # decreasing offsets of the blobs
    tv, c, o, kh = st(2)
    v = np.zeros(2, np.uint8)
    vp = v.ctypes.data_as(api.C.POINTER(api.C.c_uint8))
    rc = L.vpbs_aggregate_verifier_run_many(W.av.h, (api.C.c_uint8 * 8)(), szp([0, 8, 4]), 2, szp([0, 1, 2]), tv.ctypes.data, 1, None, c.ctypes.data,
                                            o.ctypes.data, kh.ctypes.data, 1, None, 0, vp, vp, err, 256)
    assert rc == api.ERR_INVALID and "offsets decrease at aggregate 1" in err.value.decode()


def with_word(a, at, value):
    a = np.array(a, np.uint64).copy()
    a[at] = np.uint64(value)
    return a


def test_verify_many_on_real_aggregates(world):
    """the aggregates of proofs[:2], proofs[:3] and proofs[:1] in one run (depths 1, 2, 1: two depth classes), then forgeries that reach
    ROOT, PROOF, MALFORMED and VERIFIER_DATA; every verdict and reason is api.verify_aggregate's and the single run's on that slice"""
    W = world
    st = W.slices(W.counts)
    verdicts, reasons = W.av.verify_many(W.blobs, W.counts, *st)
    assert verdicts.tolist() == [1, 1, 1] and reasons.tolist() == [api.AGG_OK] * 3
    assert W.one_by_one(W.blobs, W.counts, st) == ([1, 1, 1], [api.AGG_OK] * 3)
    # one further run: a flipped out_ct word in tree 0, a flipped opening byte in blob 1, a truncated blob 2
    tvs, cts, ocs, khs, ko, to = st
    forged = (tvs, cts, with_word(ocs, (1, 3), int(ocs[1, 3]) ^ 1), khs, ko, to)
    opening = bytearray(W.blobs[1])
    opening[8 * 300] ^= 1
    blobs = [W.blobs[0], bytes(opening), W.blobs[2][:-8]]
    verdicts, reasons = W.av.verify_many(blobs, W.counts, *forged)
    assert verdicts.tolist() == [0, 0, 0] and reasons.tolist() == [api.AGG_ROOT, api.AGG_PROOF, api.AGG_MALFORMED]
    assert W.one_by_one(blobs, W.counts, forged) == (verdicts.tolist(), reasons.tolist())
    # a forged vk_0 word in the public inputs of blob 0, beside two honest aggregates in another order (depth classes 2, 1, 1)
    lv = W.levels[0]
    at = proof_layout([lv.n_constants + 80, 135, 20, 16], lv.log_n, lv.n_constants)["fixed_len"] + 8 + 8 * 4
    word = int.from_bytes(W.blobs[0][at:at + 8], "little")
    assert word == int(W.vk0[0])
    vk_forged = bytearray(W.blobs[0])
    vk_forged[at:at + 8] = ((word ^ 1) if (word ^ 1) < P else word - 1).to_bytes(8, "little")
    counts = [3, 2, 1]
    blobs = [W.blobs[1], bytes(vk_forged), W.blobs[2]]
    st = W.slices(counts)
    verdicts, reasons = W.av.verify_many(blobs, counts, *st)
    assert verdicts.tolist() == [1, 0, 1] and reasons.tolist() == [api.AGG_OK, api.AGG_VERIFIER_DATA, api.AGG_OK]
    assert W.one_by_one(blobs, counts, st) == (verdicts.tolist(), reasons.tolist())
    # a blob under the slice of another tree of the same depth: ROOT; of another depth: MALFORMED
    blobs = [W.blobs[2], W.blobs[0], W.blobs[0]]
    counts = [2, 1, 3]
    st = W.slices(counts)
    verdicts, reasons = W.av.verify_many(blobs, counts, *st)
    assert reasons.tolist() == [api.AGG_ROOT, api.AGG_ROOT, api.AGG_MALFORMED] and not verdicts.any()
    assert W.one_by_one(blobs, counts, st) == (verdicts.tolist(), reasons.tolist())


# ================= programs: N = 8, n = 6 (8 steps per chain), the program of tests/test_gpu_multi_lut.py =================
n6 = 6
# 2 inputs (wires 0 1), 4 gates, 2 levels: gate 0 (1, 2) -> wires 2 3; gate 1 (2, 3) -> wires 4 5 6; gate 2 reads wires 3 and 6; gate 3 (snapped,
# one output) reads wires 2 and 4
FOUR = [([(0, 1)], 0, 0, 1, 2), ([(1, 1), (0, P - 1)], 7, 1, 2, 3), ([(3, 1), (6, P - 1)], 0, 0), ([(2, 1), (4, 3)], 0, 1, 1, 1)]
C1 = 0x123456789ABCDEF
NINE = [([(0, 1)], 0, 0, 1, 2), ([], C1, 1), ([(1, 1), (2, P - 1)], 0, 0, 2, 3), ([(4, P - 1), (1, 1 << 32)], 0, 1, 2, 4), ([(2, 1)], 7, 0, 1, 1),
        ([(13, 3), (8, 1)], 0, 1), ([(12, 1), (7, 2), (0, 5)], 0, 0, 1, 2), ([(16, 1), (4, P - 2)], P - 1, 1, 2, 3), ([(5, 1)], 0, 0)]


@pytest.fixture(scope="module")
def proven(ctx):
    cyc, dum = [circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, n6, LOG_N)]
    levels = [circuit_file.load(p) for p in export_circuits.ensure_aggregate_circuits(N, K, ELL, LOGB, n6, LOG_N, LEVELS)]
    keys = [ctx.keygen(N, K, ELL, LOGB, n6, seed, *SIGMAS) for seed in (77, 78)]
    delta = api.testv(N, 2)[1]
    testvs = np.stack([api.lut_testv_multi(N, 2, np.array([[0, 1], [1, 0]], np.uint64), delta)[0],
                       np.random.default_rng(3).integers(0, P, size=N, dtype=np.uint64)])
    inputs = np.stack([api.lwe_encrypt(keys[0]["params"], keys[0]["s_lwe"], delta * m % P, nonce=30 + i) for i, m in enumerate([1, 0])])
    prover = api.PbsProver(0, cyc, dum, keys[0]["bsk"], keys[0]["ksk"], K, ELL, LOGB, chains=2, witness_batch=3)
    prog = api.Program(ctx, 2, FOUR, 2)
    kh, (vk0, _) = prover.key_hash(), prover.verifier_data()
    agg = api.Aggregator(ctx, cyc, vk0, levels)
    shape = api.AggregateShape(N, K, n6, agg.verifier_data(), levels)
    seen = []
    blob, wires, out_cts = prog.prove_aggregate(prover, agg, inputs, testvs, on_proof=lambda g, b: seen.append(g))
    S = dict(ctx=ctx, cyc=cyc, dum=dum, keys=keys, testvs=testvs, inputs=inputs, prover=prover, prog=prog, kh=kh, vk0=vk0, agg=agg, shape=shape,
             blob=blob, wires=wires, out_cts=out_cts, seen=seen, av=api.AggregateVerifier(ctx, shape, max_leaves=8, max_aggregates=2))
    yield S
    S["av"].close()
    agg.close()
    prog.close()
    prover.close()


def both_paths(S, prog, blob, inputs, testvs, out_cts, kh=None):
    """(accepted, reason) of the host's program_verify_aggregate and of verify_aggregate_batch with one instance, which must be equal"""
    kh = S["kh"] if kh is None else kh
    host = api.program_verify_aggregate(prog, S["shape"], blob, inputs, testvs, out_cts, kh)
    verdicts, reasons = prog.verify_aggregate_batch(S["av"], inputs[None], [0], kh, testvs, np.asarray(out_cts)[None], [blob])
    assert (bool(verdicts[0]), int(reasons[0])) == host
    return host


def test_one_instance_is_the_composition_and_both_verifiers_accept_it(proven):
    S = proven
    proofs, wires, out_cts = S["prog"].prove(S["prover"], S["inputs"], S["testvs"])
    assert sorted(S["seen"]) == [0, 1, 2, 3] and (wires == S["wires"]).all() and (out_cts == S["out_cts"]).all()
    assert S["blob"] == S["agg"].aggregate(proofs)
    assert both_paths(S, S["prog"], S["blob"], S["inputs"], S["testvs"], S["out_cts"]) == (True, api.AGG_OK)
    # the statement is the one a verifier of gate proofs recomputes: its root is in the aggregate's public inputs
    lv = S["shape"]._keep[1]                              # four gates: depth 2
    _, pis = api.step_proof_from_bytes(S["blob"], [lv.n_constants + 80, 135, 20, 16], lv.log_n, lv.n_constants)
    root = api.program_aggregate_root(S["prog"], N, K, n6, S["vk0"], S["inputs"], S["testvs"], S["out_cts"], S["kh"])
    assert pis.size == 4 + 68 * 2 and (pis[:4] == root).all()
    cts = api.program_gate_inputs(S["prog"], N, K, n6, S["inputs"], S["out_cts"])
    lut = [g[2] for g in FOUR]
    assert (S["av"].root(S["testvs"], cts, S["out_cts"].reshape(4, KN), S["kh"], testv_of=lut) == root).all()


def test_forgeries_of_every_part_are_rejected_on_both_paths(proven):
    S = proven
    forged = S["out_cts"].copy()
    forged[0, K - 1, 1] ^= np.uint64(1)                   # body coefficient 1 of gate 0: its own leaf, and wire 3 that gate 2 reads
    assert both_paths(S, S["prog"], S["blob"], S["inputs"], S["testvs"], forged) == (False, api.AGG_ROOT)
    gates = list(FOUR)
    gates[3] = FOUR[3][:3] + (2, 1)                       # the prover snapped gate 3 with theta 1
    other = api.Program(S["ctx"], 2, gates, 2)
    assert (api.program_gate_inputs(other, N, K, n6, S["inputs"], S["out_cts"])[3] !=
            api.program_gate_inputs(S["prog"], N, K, n6, S["inputs"], S["out_cts"])[3]).any()
    assert both_paths(S, other, S["blob"], S["inputs"], S["testvs"], S["out_cts"]) == (False, api.AGG_ROOT)
    other.close()
    testvs = S["testvs"].copy()
    testvs[1, 5] ^= np.uint64(1)
    assert both_paths(S, S["prog"], S["blob"], S["inputs"], testvs, S["out_cts"]) == (False, api.AGG_ROOT)
    # input 1 is read by gate 1 alone, which snaps with theta 2 (to multiples of 2^62): half the range moves the rounded quotient by two
    inputs = S["inputs"].copy()
    inputs[1, n6] = np.uint64((int(inputs[1, n6]) + (1 << 63)) % P)
    assert (api.program_gate_inputs(S["prog"], N, K, n6, inputs, S["out_cts"])[1] !=
            api.program_gate_inputs(S["prog"], N, K, n6, S["inputs"], S["out_cts"])[1]).any()
    assert both_paths(S, S["prog"], S["blob"], inputs, S["testvs"], S["out_cts"]) == (False, api.AGG_ROOT)
    kh = S["kh"].copy()
    kh[2] ^= np.uint64(1)
    assert both_paths(S, S["prog"], S["blob"], S["inputs"], S["testvs"], S["out_cts"], kh) == (False, api.AGG_ROOT)
    flipped = bytearray(S["blob"])
    flipped[8 * 300] ^= 1
    assert both_paths(S, S["prog"], bytes(flipped), S["inputs"], S["testvs"], S["out_cts"]) == (False, api.AGG_PROOF)
    assert both_paths(S, S["prog"], S["blob"], S["inputs"], S["testvs"], S["out_cts"]) == (True, api.AGG_OK)


def test_two_instances_under_two_key_sets(proven):
    S = proven
    key_of = [1, 0]
    delta = api.testv(N, 2)[1]
    second = np.stack([api.lwe_encrypt(S["keys"][1]["params"], S["keys"][1]["s_lwe"], delta * m % P, nonce=50 + i) for i, m in enumerate([0, 1])])
    inputs = np.stack([second, S["inputs"]])              # instance 1 is the fixture's, under key set 0
    rp = api.RingProver(0, S["cyc"], S["dum"], K, ELL, LOGB, N, n6, max_keys=2, chains=2, witness_batch=3)
    assert [rp.add(k["bsk"], k["ksk"]) for k in S["keys"]] == [0, 1]
    order = []
    blobs, wires, out_cts = S["prog"].prove_aggregate_batch(rp, S["agg"], inputs, key_of, S["testvs"], on_aggregate=lambda b, _: order.append(b))
    hashes = np.stack([rp.key_hash(k) for k in range(2)])
    rp.close()
    assert order == [0, 1] and blobs[1] == S["blob"] and (wires[1] == S["wires"]).all() and (out_cts[1] == S["out_cts"]).all()
    assert (hashes[0] == S["kh"]).all()
    host = lambda claimed, ko: [api.program_verify_aggregate(S["prog"], S["shape"], blobs[b], inputs[b], S["testvs"], claimed[b], hashes[ko[b]])
                                for b in range(2)]
    forged = out_cts.copy()
    forged[0, 0, K - 1, 1] ^= np.uint64(1)
    for claimed, ko, want in ((out_cts, key_of, [(True, api.AGG_OK)] * 2), (forged, key_of, [(False, api.AGG_ROOT), (True, api.AGG_OK)]),
                              (out_cts, [0, 1], [(False, api.AGG_ROOT)] * 2)):
        verdicts, reasons = S["prog"].verify_aggregate_batch(S["av"], inputs, ko, hashes, S["testvs"], claimed, blobs)
        assert [(bool(v), int(r)) for v, r in zip(verdicts, reasons)] == want == host(claimed, ko)
    # a verifier of one aggregate per run takes the same instances in two chunks
    one = api.AggregateVerifier(S["ctx"], S["shape"], max_leaves=4)
    verdicts, reasons = S["prog"].verify_aggregate_batch(one, inputs, key_of, hashes, S["testvs"], forged, blobs)
    assert verdicts.tolist() == [0, 1] and reasons.tolist() == [api.AGG_ROOT, api.AGG_OK]
    one.close()


def test_a_nine_gate_program_is_refused_before_any_proof(proven):
    S = proven
    nine = api.Program(S["ctx"], 3, NINE, 2)
    before = S["prover"].last_run()
    called = []
    inputs = np.zeros((3, n6 + 1), np.uint64)
    with pytest.raises(api.VpbsError, match=r"n_gates 9 exceeds 2\^levels = 8"):
        nine.prove_aggregate(S["prover"], S["agg"], inputs, S["testvs"], on_proof=lambda g, b: called.append(g))
    assert not called and S["prover"].last_run() == before
    rp = api.RingProver(0, S["cyc"], S["dum"], K, ELL, LOGB, N, n6, max_keys=1, chains=1, witness_batch=3)
    assert rp.add(S["keys"][0]["bsk"], S["keys"][0]["ksk"]) == 0
    ring_before = rp.last_run()
    with pytest.raises(api.VpbsError, match=r"n_gates 9 exceeds 2\^levels = 8"):
        nine.prove_aggregate_batch(rp, S["agg"], inputs[None], [0], S["testvs"], on_aggregate=lambda b, _: called.append(b))
    assert not called and rp.last_run() == ring_before
    rp.close()
    with pytest.raises(api.VpbsError, match=r"n_gates 9 exceeds 2\^levels = 8"):
        nine.verify_aggregate_batch(S["av"], inputs[None], [0], S["kh"], S["testvs"], np.zeros((1, 9, K, N), np.uint64), [b"\0" * 8])
    nine.close()


def test_the_tool_proves_aggregates_and_verifies_both_ways():
    """tools/run_program.py --prove --aggregate at the N = 8, n = 6 set: 2 layers of 2 gates for two instances under two key sets, one
    aggregate of depth 2 per instance, accepted by the host and the device"""
    export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, n6, LOG_N)
    export_circuits.ensure_aggregate_circuits(N, K, ELL, LOGB, n6, LOG_N, LEVELS)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "tools", "run_program.py"), "--n8", "--levels", "2", "--width", "2",
                        "--prove", "--aggregate", "--instances", "2", "--keys", "2", "--chains", "2", "--witness-batch", "3"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    g = line["aggregate"]
    assert (g["instances"], g["gates"], g["depth"], g["accepted"], g["out_cts_equal"]) == (2, 4, 2, True, True), line
    assert g["host"] == g["device"] == [[True, ""], [True, ""]]
    assert g["client_bytes_aggregate"] < g["client_bytes_per_gate_proofs"] and line["proven"] is True and line["all_equal"] is True
