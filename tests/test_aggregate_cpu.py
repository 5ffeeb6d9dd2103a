"""Aggregation of vPBS proofs on the CPU: the level circuits of circuitgen/aggregate_circuit.py proven by the CPU oracle
over small leaves, the in-circuit soundness of their witness plans, and the host's statement root (api.aggregate_root) against a Python
model over pymodel.hash_no_pad.  The GPU twin is tests/test_gpu_aggregate.py."""
import random

import numpy as np
import pytest

import aggregate_circuit as ag
import cyclic_circuit as cc
import pymodel
from test_cyclic_cpu import OracleProver
from vpbs_amd import api

P = api.P


# ================= levels 1 and 2 over DummyCircuit leaves =================
class Tree:
    """three leaves (DummyCircuit(api, 5, 72) proofs whose last 68 public inputs are the circuit's own vk_words), A_1 and A_2, one level-1
    node (leaf 0, leaf 1) proven by the CPU oracle; everything the tests below share, computed once"""

    def __init__(self):
        rnd = random.Random(11)
        self.dm = cc.DummyCircuit(api, 5, 72)
        self.D = OracleProver(self.dm.built)
        self.vk0 = self.D.vk
        self.leaves = []
        for _ in range(3):
            pis = np.array([rnd.randrange(P) for _ in range(4)] + [int(v) for v in self.vk0], np.uint64)
            self.leaves.append((self.D.prove(self.dm.witness(pis), pis), pis))
        self.S0 = cc.Shape(api, 5, 72)
        self.A1 = ag.AggregateCircuit(api, self.S0, 1)
        self.P1 = OracleProver(self.A1.built)
        self.plan1 = self.A1.built.circuit.witness_plan(self.A1.positions)
        self.values1 = self.node1_values(0, 1)
        self.wires1 = self.plan1.run(self.values1)
        self.pis1 = np.array(self.A1.public_inputs(self.wires1), np.uint64)
        self.node1 = self.P1.prove(self.wires1, self.pis1)

    def node1_values(self, i, j, vk0=None):
        (pa, ia), (pb, ib) = self.leaves[i], self.leaves[j]
        return self.A1.values(self.S0.flat_proof(pa), ia, self.S0.flat_proof(pb), ib, [self.vk0 if vk0 is None else vk0])

    def statement(self, i):
        return [int(x) for x in api.hash_no_pad(self.leaves[i][1])]


@pytest.fixture(scope="module")
def tree():
    t = Tree()
    yield t
    t.plan1.free()


def test_level_1_and_2_on_the_cpu(tree):
    """A_1 over two leaf proofs and A_2 over two level-1 proofs: the witnesses satisfy the circuits, the root public inputs are the Python
    tree over api.hash_no_pad, the verifier data of the levels below ride in the public inputs, each root proof is accepted by verify_step"""
    t = tree
    A1 = t.A1
    assert A1.shape.n_pi == 72 and len(A1.positions) == 2 * (t.S0.proof_words + 72) + 68
    ok, msg = A1.built.circuit.check_witness(t.wires1, api.hash_no_pad(t.pis1))
    assert ok, msg
    hnp = lambda x: api.hash_no_pad(np.array(x, np.uint64))
    root1 = ag.tree_root([t.statement(0), t.statement(1)], hnp)
    assert [int(v) for v in t.pis1[:4]] == root1 and (t.pis1[4:] == t.vk0).all()
    assert t.P1.verify(t.node1, t.pis1)
    wrong = t.pis1.copy()
    wrong[1] ^= np.uint64(1)
    assert not t.P1.verify(t.node1, wrong)
    # level 2: both children are the level-1 node (what the padding of a three-leaf tree does to its right half)
    A2 = ag.AggregateCircuit(api, A1.shape, 2)
    assert A2.shape.n_pi == 140 and A2.built.log_n == A2.shape.log_n
    P2 = OracleProver(A2.built)
    flat1 = A1.shape.flat_proof(t.node1)
    plan2 = A2.built.circuit.witness_plan(A2.positions)
    wires2 = plan2.run(A2.values(flat1, t.pis1, flat1, t.pis1, [t.vk0, t.P1.vk]))
    pis2 = np.array(A2.public_inputs(wires2), np.uint64)
    ok, msg = A2.built.circuit.check_witness(wires2, api.hash_no_pad(pis2))
    assert ok, msg
    assert [int(v) for v in pis2[:4]] == [int(v) for v in hnp(root1 + root1)]
    assert (pis2[4:72] == t.vk0).all() and (pis2[72:] == t.P1.vk).all()
    assert [int(v) for v in pis2[:4]] == ag.tree_root([t.statement(0), t.statement(1)] * 2, hnp)
    assert P2.verify(P2.prove(wires2, pis2), pis2)
    # in-circuit soundness at level 2: a child whose vk list differs from the node's, and a child verified under another vk_1
    other = t.vk0.copy()
    other[5] ^= np.uint64(1)
    bad_child = t.pis1.copy()
    bad_child[4 + 5] ^= np.uint64(1)
    for vals in (A2.values(flat1, t.pis1, flat1, t.pis1, [other, t.P1.vk]), A2.values(flat1, t.pis1, flat1, bad_child, [t.vk0, t.P1.vk]),
                 A2.values(flat1, t.pis1, flat1, t.pis1, [t.vk0, P2.vk])):
        with pytest.raises(api.VpbsError):
            plan2.run(vals)
    plan2.free()


def test_a_bad_leaf_makes_the_level_1_witness_plan_fail(tree):
    """every word of both leaf proofs is bound (a random sweep of single flipped words, as for the gadget itself), and so are the leaf's own
    verifier-data public inputs: they must equal the vk_0 the node is proven under"""
    t = tree
    rnd = random.Random(5)
    W, n_pi = t.S0.proof_words, 72
    assert (t.plan1.run(t.values1) == t.wires1).all()
    sweep = [(slot, rnd.randrange(W)) for slot in (0, 1) for _ in range(60)] + [(0, 3), (1, W - 1), (0, t.S0.caps_words + 10)]
    for slot, at in sweep:
        bad = t.values1.copy()
        bad[slot * (W + n_pi) + at] ^= np.uint64(1 << rnd.randrange(0, 40))
        with pytest.raises(api.VpbsError):
            t.plan1.run(bad)
    # a statement word of a leaf: the proof no longer verifies in circuit
    bad = t.values1.copy()
    bad[W + 2] ^= np.uint64(1)
    with pytest.raises(api.VpbsError):
        t.plan1.run(bad)
    # a leaf whose verifier-data public inputs differ from vk_0 (whichever side is changed: the leaf's words, or the vk_0 handed in)
    for at in (W + 4, W + n_pi - 1, W + n_pi + W + 4 + 17):
        bad = t.values1.copy()
        bad[at] ^= np.uint64(1)
        with pytest.raises(api.VpbsError, match="set twice"):
            t.plan1.run(bad)
    other = t.vk0.copy()
    other[0] ^= np.uint64(1)
    with pytest.raises(api.VpbsError, match="set twice"):
        t.plan1.run(t.node1_values(0, 1, vk0=other))
    # the padding node (a leaf with itself) is an ordinary node
    w = t.plan1.run(t.node1_values(2, 2))
    s = t.statement(2)
    assert t.A1.public_inputs(w)[:4] == [int(v) for v in api.hash_no_pad(np.array(s + s, np.uint64))]


# ================= the statement alone, N = 8 =================
N, K, N_LWE = 8, 2, 1
KN = K * N


_leaf_cache = {}


def model_leaf(*parts):
    """memoised: a single-word flip changes one leaf of a statement, the others are looked up"""
    key = tuple(tuple(int(v) for v in p) for p in parts)
    if key not in _leaf_cache:
        _leaf_cache[key] = _model_leaf(*key)
    return _leaf_cache[key]


def _model_leaf(vk0, testv, ct, out_ct, key_hash):
    """s_i by the definition: hash_no_pad of acc_init | counter | accumulator | key hash | LWE hash | vk_0, ct words reduced"""
    h = [0] * 4
    for item in [ct[N_LWE]] + list(ct[:N_LWE]) + [0]:
        h = pymodel.hash_no_pad(h + [int(item) % P])
    pis = [0] * (KN - N) + [int(v) for v in testv] + [N_LWE + 2] + [int(v) for v in out_ct] + [int(v) for v in key_hash] + h + [int(v) for v in vk0]
    assert len(pis) == 2 * KN + 77
    return pymodel.hash_no_pad(pis)


def model_root(leaves):
    return ag.tree_root(leaves, pymodel.hash_no_pad)


def statement_arrays(seed, count, n_testv=3, n_keys=2):
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.integers(0, P, size=shape, dtype=np.uint64)
    return {"vk0": f(68), "testvs": f(n_testv, N), "cts": f(count, N_LWE + 1), "out_cts": f(count, KN), "key_hashes": f(n_keys, 4),
            "key_of": rng.integers(0, n_keys, size=count).astype(np.uint32), "testv_of": rng.integers(0, n_testv, size=count).astype(np.uint32)}


def api_root(s):
    return [int(v) for v in api.aggregate_root(N, K, N_LWE, s["vk0"], s["testvs"], s["cts"], s["out_cts"], s["key_hashes"], s["key_of"], s["testv_of"])]


def model_leaves(s):
    return [model_leaf(s["vk0"], s["testvs"][s["testv_of"][i]], s["cts"][i], s["out_cts"][i], s["key_hashes"][s["key_of"][i]])
            for i in range(len(s["cts"]))]


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5])
def test_aggregate_root_against_the_python_model(count):
    """depths 1, 1, 2, 2, 3 with mixed key_of / testv_of: the padding repeats the last leaf; count = 1 folds the leaf with itself"""
    s = statement_arrays(40 + count, count)
    leaves = model_leaves(s)
    assert api_root(s) == model_root(leaves)
    assert ag.tree_depth(count) == api.aggregate_depth(count) == [1, 1, 2, 2, 3][count - 1]
    if count == 3:   # the padding is the LAST leaf, not a zero leaf and not the first
        assert model_root(leaves) == model_root(leaves + [leaves[2]]) != model_root(leaves + [leaves[0]])
    # a ct word at or above p enters as its residue; the default indices: leaf i takes testvs[i] of count, key 0
    t = dict(s, cts=s["cts"].copy())
    t["cts"][0, 0] = np.uint64(P + 5)
    u = dict(s, cts=s["cts"].copy())
    u["cts"][0, 0] = np.uint64(5)
    assert api_root(t) == api_root(u)
    d = statement_arrays(60 + count, count, n_testv=count, n_keys=1)
    want = api_root(dict(d, key_of=np.zeros(count, np.uint32), testv_of=np.arange(count, dtype=np.uint32)))
    assert [int(v) for v in api.aggregate_root(N, K, N_LWE, d["vk0"], d["testvs"], d["cts"], d["out_cts"], d["key_hashes"])] == want


def test_single_word_flips_of_the_statement_change_the_root():
    """200 random single-word flips over every part of a five-leaf statement: each changes a residue, so the model's root changes -- and the
    host's root is the model's (or the word left the field and the host refuses it): no flip can be accepted by a verifier of the root"""
    s = statement_arrays(7, 5)
    base_leaves = model_leaves(s)
    base = model_root(base_leaves)
    assert api_root(s) == base
    rnd = random.Random(2)
    parts = ["testvs", "cts", "out_cts", "key_hashes", "vk0"]
    for _ in range(200):
        part = rnd.choice(parts)
        t = dict(s)
        a = t[part] = s[part].copy()
        flat = a.reshape(-1)
        at = rnd.randrange(flat.size)
        flat[at] ^= np.uint64(1 << rnd.randrange(64))
        residue_changed = int(flat[at]) % P != int(s[part].reshape(-1)[at]) % P
        used = part != "testvs" or (at // N) in set(int(x) for x in s["testv_of"])
        used = used and (part != "key_hashes" or (at // 4) in set(int(x) for x in s["key_of"]))
        raw_bad = part != "cts" and int(flat[at]) >= P and used
        if raw_bad:
            with pytest.raises(api.VpbsError, match="not a field element"):
                api_root(t)
            continue
        got = api_root(t)
        if part == "cts" and not residue_changed:
            assert got == base
            continue
        assert got == model_root(model_leaves(t))
        assert (got != base) == used


def test_raw_words_at_or_above_p_and_argument_checks():
    s = statement_arrays(9, 3)
    for part, at in (("out_cts", (1, 5)), ("testvs", (int(s["testv_of"][0]), 0)), ("key_hashes", (int(s["key_of"][2]), 3))):
        for word in (P, 2 ** 64 - 1):
            t = dict(s)
            t[part] = s[part].copy()
            t[part][at] = np.uint64(word)
            with pytest.raises(api.VpbsError, match="not a field element"):
                api_root(t)
    # count = 0
    with pytest.raises(api.VpbsError, match="malformed"):
        api.aggregate_root(N, K, N_LWE, s["vk0"], s["testvs"], np.zeros((0, N_LWE + 1), np.uint64), np.zeros((0, KN), np.uint64), s["key_hashes"],
                           np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    # an index past its table
    with pytest.raises(api.VpbsError, match="malformed"):
        api_root(dict(s, key_of=np.array([0, 2, 0], np.uint32)))
    with pytest.raises(api.VpbsError, match="malformed"):
        api_root(dict(s, testv_of=np.array([0, 1, 3], np.uint32)))
    # verify_aggregate: count = 0 and count > 2^levels are refused before the bytes are looked at
    level = cc.DummyCircuit(api, 5, 72).built           # any circuit gives a shape; none of it is reached
    shape = api.AggregateShape(N, K, N_LWE, np.zeros((3, 68), np.uint64), [level, level])
    five = statement_arrays(10, 5)
    args = lambda a: (a["testvs"], a["cts"], a["out_cts"], a["key_hashes"], a["key_of"], a["testv_of"])
    with pytest.raises(api.VpbsError, match="exceeds 2\\^levels"):
        api.verify_aggregate(shape, b"\0" * 64, 5, *args(five))
    with pytest.raises(api.VpbsError, match="count is 0"):
        api.verify_aggregate(shape, b"\0" * 64, 0, s["testvs"], np.zeros((0, N_LWE + 1), np.uint64), np.zeros((0, KN), np.uint64), s["key_hashes"],
                             np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    with pytest.raises(ValueError, match="count = 2"):
        api.verify_aggregate(shape, b"\0" * 64, 2, *args(s))
    # bytes that are no proof at all: MALFORMED, with the reason's text
    four = statement_arrays(12, 4)
    assert api.verify_aggregate(shape, b"\0" * 64, 4, *args(four)) == (False, api.AGG_MALFORMED)
    assert api.aggregate_reason_text(api.AGG_MALFORMED).startswith("the bytes are not an aggregate proof")
    assert api.aggregate_reason_text(api.AGG_OK) == ""
    with pytest.raises(ValueError):
        api.aggregate_reason_text(9)
