"""GPU tests (-m gpu): aggregation of vPBS proofs -- api.Aggregator folds the proofs of a batch into ONE proof, and
api.verify_aggregate (host) and api.AggregateVerifier (device) check it against the statement of all the bootstraps.  The yardsticks: the
test's own composition of the tree (circuitgen/aggregate_circuit.py, the CPU oracle's prover for one node, Context.prove_step for whole
trees), api.aggregate_root (itself checked against a Python model in tests/test_aggregate_cpu.py), and the host verifier for the device
one.  N = 8, n = 1 (chains of 3 steps), degree 2^13: the exported standard set; the level circuits have degree 2^14."""
import random

import numpy as np
import pytest

import aggregate_circuit as ag
import cyclic_circuit as cc
import export_circuits
import step_oracle
import vpbs_amd
from batch_verify_layout import proof_layout
from test_cyclic_cpu import OracleProver
from vpbs_amd import api, circuit_file

pytestmark = pytest.mark.gpu
P = api.P
K, ELL, LOGB = 2, 4, 5
N, N_LWE, LOG_N = 8, 1, 13
KN = K * N
LEVELS = 3
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)
KEY_OF = [0, 1, 1, 0, 1]          # leaf i was proven under the key set of slot KEY_OF[i]
TESTV_OF = [0, 0, 1, 0, 1]


class World:
    """five vPBS proofs under two key sets from one RingProver, the Aggregator over the exported level circuits, both verifiers, and the
    level circuits on the context once more for the test's own composition; computed once, read by every test"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.cyc, self.dum = (circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, N_LWE, LOG_N))
        self.levels = [circuit_file.load(p) for p in export_circuits.ensure_aggregate_circuits(N, K, ELL, LOGB, N_LWE, LOG_N, LEVELS)]
        assert [d.meta["level"] for d in self.levels] == [1, 2, 3] and all(d.meta["kind"] == 3 for d in self.levels)
        self.ncols = [self.cyc.n_constants + 80, 135, 20, 16]
        rp = api.RingProver(0, self.cyc, self.dum, K, ELL, LOGB, N, N_LWE, max_keys=2, chains=2, witness_batch=3)
        keys = [ctx.keygen(N, K, ELL, LOGB, N_LWE, seed, *SIGMAS) for seed in (31, 32)]
        assert [rp.add(k["bsk"], k["ksk"]) for k in keys] == [0, 1]
        tv, delta = api.testv(N, 2)
        tv = np.asarray(tv, np.uint64)
        self.testvs = np.stack([tv, np.array([(P - int(v)) % P for v in tv], np.uint64)])
        self.cts = np.stack([np.asarray(api.lwe_encrypt(keys[k]["params"], keys[k]["s_lwe"], delta * (i % 2) % P, nonce=20 + i), np.uint64)
                             for i, k in enumerate(KEY_OF)])
        self.proofs, out_ct, _ = rp.prove(self.cts, KEY_OF, self.testvs[TESTV_OF])
        self.out_cts = out_ct.reshape(5, KN)
        self.key_hashes = np.stack([rp.key_hash(0), rp.key_hash(1)])
        self.vk0 = rp.verifier_data()[0]
        rp.close()
        self.agg = api.Aggregator(ctx, self.cyc, self.vk0, self.levels)
        self.vks = self.agg.verifier_data()
        assert (self.vks[0] == self.vk0).all()
        self.shape = api.AggregateShape(N, K, N_LWE, self.vks, self.levels)
        self.av = api.AggregateVerifier(ctx, self.shape, max_leaves=8)
        self.memo, self.runs = {}, {}
        self.dev = None

    def aggregate(self, count):
        """the aggregate of the first `count` proofs, made once; .runs keeps the Aggregator's figures of that run"""
        if count not in self.memo:
            self.memo[count] = self.agg.aggregate(self.proofs[:count])
            self.runs[count] = self.agg.last_run()
        return self.memo[count]

    def statement(self, count):
        return (self.testvs, self.cts[:count], self.out_cts[:count], self.key_hashes, KEY_OF[:count], TESTV_OF[:count])

    def root(self, count):
        return api.aggregate_root(N, K, N_LWE, self.vk0, *self.statement(count))

    def both(self, blob, count, statement):
        """(verdict, reason) of the host and of the device, which must be equal"""
        host = api.verify_aggregate(self.shape, blob, count, *statement)
        device = self.av.verify(blob, count, *statement)
        assert host == device, (host, device)
        return host

    def leaf(self, i):
        proof, pis = api.step_proof_from_bytes(self.proofs[i], self.ncols, LOG_N, self.cyc.n_constants)
        return np.concatenate([proof[k].reshape(-1) for k in ("caps", "openings", "fri")]), pis

    # ---- the test's own composition on the context: level circuits committed here, witnesses by the circuits' plans ----
    def compose(self, count):
        if self.dev is None:
            self.dev = []
            for d in self.levels:
                sigma = d.circuit.sigma_values()
                cs = self.ctx.commit_values(np.concatenate([d.constants, sigma]))
                vk = circuit_file.verifier_data_words(cs.cap(), d.log_n)
                self.dev.append((d, sigma, cs, vk, d.circuit.witness_plan(d.preset_pos)))
        cur = [self.leaf(min(i, count - 1)) for i in range(1 << api.aggregate_depth(count))]
        vks = [self.vk0]
        for d, sigma, cs, vk, plan in self.dev[:api.aggregate_depth(count)]:
            nxt = []
            for k in range(len(cur) // 2):
                (fa, pa), (fb, pb) = cur[2 * k], cur[2 * k + 1]
                wires = plan.run(np.concatenate([fa, pa, fb, pb] + vks))
                pis = np.array([int(wires[p]) for p in d.pi_pos], np.uint64)
                si = self.ctx.make_step_inputs(d.log_n, wires, None, None, cs, vk[:4], pis, sigmas=sigma, n_routed=80, n_constants=d.n_constants,
                                               gates=d.gates)
                proof = self.ctx.prove_step(si)
                blob = self.ctx.step_proof_to_bytes(si, d.n_constants, proof)
                nxt.append((np.concatenate([proof[k].reshape(-1) for k in ("caps", "openings", "fri")]), pis, blob))
            cur = [(f, p) for f, p, _ in nxt]
            vks.append(vk)
        return nxt[0][2], vks

    def close(self):
        for d in self.dev or []:
            d[4].free()
        self.av.close()
        self.agg.close()


@pytest.fixture(scope="module")
def world():
    c = vpbs_amd.Context(0, log_n_max=16)
    w = World(c)
    yield w
    w.close()
    c.close()


def test_one_node_is_byte_for_byte_the_cpu_oracles_proof(world):
    """two vPBS proofs: the aggregate is what the test composes itself -- AggregateCircuit built here, the product's witness generator, the
    CPU oracle's prover (one proof of degree 2^14), the Python serialiser; and the level circuit's verifier data are the oracle's"""
    W = world
    A1 = ag.AggregateCircuit(api, cc.Shape(api, LOG_N, cc.cyclic_n_pi(N, K)), 1)
    assert A1.built.log_n == W.levels[0].log_n == 14
    O = OracleProver(A1.built)
    assert (O.vk == W.vks[1]).all()
    (fa, pa), (fb, pb) = W.leaf(0), W.leaf(1)
    wires = A1.built.circuit.generate_witness(dict(zip(A1.positions, (int(v) for v in A1.values(fa, pa, fb, pb, [W.vk0])))))
    pis = np.array(A1.public_inputs(wires), np.uint64)
    proof = O.prove(wires, pis)
    want = step_oracle.to_bytes(proof, proof["ncols"], O.nconst, pis, A1.built.log_n)
    got = W.aggregate(2)
    assert got == want
    assert len(got) < 2 * len(W.proofs[0])   # one 2^14 proof of 72 public inputs, against two 2^13 proofs


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5])
def test_counts_and_depths(world, count):
    """depths 1, 1, 2, 2, 3, leaves under two key sets: accepted by the host and the device alike, the root public inputs are
    api.aggregate_root's, the bytes at depths 2 and 3 are those of a tree composed here through Context.prove_step"""
    W = world
    blob = W.aggregate(count)
    d = api.aggregate_depth(count)
    assert W.both(blob, count, W.statement(count)) == (True, api.AGG_OK)
    lv = W.levels[d - 1]
    _, pis = api.step_proof_from_bytes(blob, [lv.n_constants + 80, 135, 20, 16], lv.log_n, lv.n_constants)
    assert pis.size == 4 + 68 * d and (pis[:4] == W.root(count)).all() and (pis[4:] == W.vks[:d].reshape(-1)).all()
    if count in (3, 5):
        want, vks = W.compose(count)
        assert all((a == b).all() for a, b in zip(vks, W.vks))
        assert blob == want
    # the same blob under a statement of another count of the same depth: another root
    if count in (3, 5):
        other = count + 1 if count == 3 else 6
        st = (W.testvs, W.cts[np.arange(other) % 5], W.out_cts[np.arange(other) % 5], W.key_hashes, [KEY_OF[i % 5] for i in range(other)],
              [TESTV_OF[i % 5] for i in range(other)])
        assert W.both(blob, other, st) == (False, api.AGG_ROOT)


def test_the_node_counts_of_a_run(world):
    """padding nodes with the same two children are proven once: 5 leaves are 3 + 2 + 1 nodes, 1 leaf is one node of the leaf with itself"""
    W = world
    for count, nodes in ((1, 1), (2, 1), (3, 3), (4, 3), (5, 6)):
        W.aggregate(count)
        run = W.runs[count]
        assert (run["nodes"], run["depth"]) == (nodes, api.aggregate_depth(count)), run
        assert run["prove_ms"] > 0 and run["witness_ms"] > 0 and run["seconds"] > 0


def test_the_device_root_alone(world):
    """AggregateVerifier.root against api.aggregate_root: ct words exactly p - 1, p and 2^64 - 1, testv_of with repeats, key_of out of order,
    count = 5 under max_leaves = 8 (a padded tree of depth 3), host arrays and device pointers"""
    W = world
    rng = np.random.default_rng(3)
    f = lambda *shape: rng.integers(0, P, size=shape, dtype=np.uint64)
    testvs, cts, out_cts, key_hashes = f(3, N), f(5, N_LWE + 1), f(5, KN), f(4, 4)
    cts[0, 0], cts[1, 1], cts[4, 0] = np.uint64(P - 1), np.uint64(P), np.uint64(2 ** 64 - 1)
    key_of, testv_of = [3, 0, 2, 0, 1], [2, 2, 0, 1, 2]
    # the verifier's own vk_0 is the world's: the host root is taken under it
    for count in (1, 2, 3, 4, 5):
        st = (testvs, cts[:count], out_cts[:count], key_hashes, key_of[:count], testv_of[:count])
        want = api.aggregate_root(N, K, N_LWE, W.vk0, *st)
        assert (W.av.root(*st) == want).all(), count
    d = [W.ctx.device_upload_new(a) for a in (testvs, cts, out_cts, key_hashes)]
    try:
        got = W.av.root(d[0], d[1], d[2], d[3], key_of, testv_of, on_device=True, count=5, n_testv=3, n_keys=4)
    finally:
        for p in d:
            W.ctx.device_free(p)
    assert (got == api.aggregate_root(N, K, N_LWE, W.vk0, testvs, cts, out_cts, key_hashes, key_of, testv_of)).all()
    # a raw word at or above p: refused as the host refuses it; the defaults for missing index arrays
    bad = out_cts.copy()
    bad[4, KN - 1] = np.uint64(P)
    with pytest.raises(api.VpbsError, match="not a field element"):
        W.av.root(testvs, cts, bad, key_hashes, key_of, testv_of)
    one = (f(5, N), cts, out_cts, key_hashes[:1])
    assert (W.av.root(*one) == api.aggregate_root(N, K, N_LWE, W.vk0, *one)).all()
    with pytest.raises(api.VpbsError, match="exceeds max_leaves"):
        W.av.root(f(9, N), f(9, N_LWE + 1), f(9, KN), key_hashes[:1])
    with pytest.raises(api.VpbsError, match=r"key_of\[1\] = 4"):
        W.av.root(testvs, cts, out_cts, key_hashes, [0, 4, 0, 0, 0], testv_of)


def bound_statement(count):
    """a random statement of `count` leaves, seeded by count alone (no proofs): min(count, 3) test vectors and min(count, 4) key hashes,
    so that n_testv and n_keys fit a verifier of max_leaves = count, with repeats and out of order"""
    rng = np.random.default_rng(100 + count)
    f = lambda *shape: rng.integers(0, P, size=shape, dtype=np.uint64)
    n_tv, n_kh = min(count, 3), min(count, 4)
    return (f(n_tv, N), f(count, N_LWE + 1), f(count, KN), f(n_kh, 4), rng.integers(0, n_kh, size=count), rng.integers(0, n_tv, size=count))


@pytest.mark.parametrize("max_leaves, count", [(8, 6), (8, 7), (8, 8), (5, 5), (1, 1)])
def test_the_single_root_at_the_bounds_of_the_run_buffers(world, max_leaves, count):
    """AggregateVerifier.root runs the statement of many trees with one tree; its level buffers hold max_leaves entries and its index tables
    5 max_leaves + (4 levels + 1) max_aggregates words.  Against api.aggregate_root under the verifier's vk_0, max_aggregates = 1: counts 6
    (level 1 stands on the leaf pairs (4, 5) and (5, 5)), 7 and 8 (a full tree at exactly max_leaves) under max_leaves = 8; count 5 under
    max_leaves = 5 (no power of two: 4 level-1 nodes in a buffer of 5); count 1 under max_leaves = 1 (the leaf folded with itself, a verifier
    of one level).  And a raw out_cts word equal to p in a full tree is refused as the host refuses it."""
    W = world
    av = W.av if max_leaves == 8 else api.AggregateVerifier(W.ctx, W.shape, max_leaves=max_leaves)
    try:
        assert (av.max_leaves, av.max_aggregates) == (max_leaves, 1)
        st = bound_statement(count)
        assert (av.root(*st) == api.aggregate_root(N, K, N_LWE, W.vk0, *st)).all()
        if count == 8:
            bad = (st[0], st[1], with_word(st[2], (7, KN - 1), P), *st[3:])
            with pytest.raises(api.VpbsError, match="not a field element"):
                api.aggregate_root(N, K, N_LWE, W.vk0, *bad)
            with pytest.raises(api.VpbsError, match="not a field element"):
                av.root(*bad)
    finally:
        if av is not W.av:
            av.close()


def with_word(a, at, value):
    a = np.array(a, np.uint64).copy()
    a[at] = np.uint64(value)
    return a


def test_forgeries_get_the_same_reason_on_both_paths(world):
    W = world
    blob = W.aggregate(2)
    tvs, cts, ocs, khs, ko, to = W.statement(2)
    lv = W.levels[0]
    pi_at = lambda j: proof_layout([lv.n_constants + 80, 135, 20, 16], lv.log_n, lv.n_constants)["fixed_len"] + 8 + 8 * j
    word = int.from_bytes(blob[pi_at(4):pi_at(4) + 8], "little")
    assert word == int(W.vk0[0])
    other = (word ^ 1) if (word ^ 1) < P else word - 1
    vk_forged = bytearray(blob)
    vk_forged[pi_at(4):pi_at(4) + 8] = other.to_bytes(8, "little")
    opening = bytearray(blob)
    opening[8 * 300] ^= 1
    three = W.statement(3)
    cases = [("one flipped out_ct word", blob, 2, (tvs, cts, with_word(ocs, (1, 3), int(ocs[1, 3]) ^ 1), khs, ko, to), api.AGG_ROOT),
             ("two leaves swapped", blob, 2, (tvs, cts[::-1], ocs[::-1], khs, ko[::-1], to[::-1]), api.AGG_ROOT),
             ("another slot's key hash", blob, 2, (tvs, cts, ocs, khs, [ko[0], ko[0]], to), api.AGG_ROOT),
             ("a testv row changed", blob, 2, (with_word(tvs, (0, 2), int(tvs[0, 2]) ^ 1), cts, ocs, khs, ko, to), api.AGG_ROOT),
             ("count = 3 for a depth-1 blob", blob, 3, three, api.AGG_MALFORMED),
             ("a flipped opening byte", bytes(opening), 2, W.statement(2), api.AGG_PROOF),
             ("a flipped vk_0 word in the public inputs", bytes(vk_forged), 2, W.statement(2), api.AGG_VERIFIER_DATA),
             ("a truncated blob", blob[:-8], 2, W.statement(2), api.AGG_MALFORMED),
             ("an empty blob", b"", 2, W.statement(2), api.AGG_MALFORMED),
             ("an out_ct word at or above p", blob, 2, (tvs, cts, with_word(ocs, (0, 0), P), khs, ko, to), api.AGG_ROOT),
             ("a ct word changed", blob, 2, (tvs, with_word(cts, (1, 0), int(cts[1, 0]) ^ 1), ocs, khs, ko, to), api.AGG_ROOT)]
    assert ko[0] != ko[1]
    for name, b, count, st, want in cases:
        assert W.both(b, count, st) == (False, want), name
    # the depth-2 aggregate under the depth-1 statement, and the honest ones again
    assert W.both(W.aggregate(3), 2, W.statement(2)) == (False, api.AGG_MALFORMED)
    assert W.both(blob, 2, W.statement(2)) == (True, api.AGG_OK)
    # a ct word replaced by another representative of its residue is the same statement
    low = with_word(cts, (0, 0), int(cts[0, 0]) % (2 ** 64 - P))
    assert W.both(blob, 2, (tvs, with_word(low, (0, 0), int(low[0, 0]) + P), ocs, khs, ko, to)) == W.both(blob, 2, (tvs, low, ocs, khs, ko, to))


def test_no_single_word_flip_of_the_statement_is_accepted(world):
    """200 random single-word flips over testvs, cts, out_cts and key_hashes of a three-leaf statement (each changes a residue that a leaf
    reads, so the root changes: tests/test_aggregate_cpu.py): none is accepted, host and device agree on every reason"""
    W = world
    blob = W.aggregate(3)
    base = W.statement(3)
    assert W.both(blob, 3, base) == (True, api.AGG_OK)
    rnd = random.Random(4)
    used_tv, used_kh = sorted(set(TESTV_OF[:3])), sorted(set(KEY_OF[:3]))
    for _ in range(200):
        st = [np.array(a, np.uint64).copy() for a in base[:4]]
        part = rnd.randrange(4)
        a = st[part]
        row = rnd.choice(used_tv) if part == 0 else rnd.choice(used_kh) if part == 3 else rnd.randrange(3)
        col = rnd.randrange(a.shape[1])
        old = int(a[row, col])
        new = old ^ (1 << rnd.randrange(64))
        if part == 1 and new % P == old % P:
            new = (old + 1) % P
        a[row, col] = np.uint64(new)
        assert W.both(blob, 3, (*st, base[4], base[5])) == (False, api.AGG_ROOT), (part, row, col)


def test_a_bad_leaf_is_refused_before_anything_is_proven(world):
    W = world
    good = W.aggregate(2)
    tampered = bytearray(W.proofs[1])
    tampered[8 * 300] ^= 1
    with pytest.raises(api.VpbsError, match=r"leaf 1: the proof does not verify; nothing was proven"):
        W.agg.aggregate([W.proofs[0], bytes(tampered)])
    assert W.agg.last_run()["nodes"] == 0
    with pytest.raises(api.VpbsError, match=r"leaf 0: the bytes are not a vPBS proof"):
        W.agg.aggregate([W.proofs[0][:-8], bytes(tampered)])
    assert W.agg.last_run()["nodes"] == 0
    # a valid proof of another circuit shape in a leaf's place: an aggregate is no leaf
    with pytest.raises(api.VpbsError, match=r"leaf 2: the bytes are not a vPBS proof"):
        W.agg.aggregate([W.proofs[0], W.proofs[1], good])
    with pytest.raises(api.VpbsError, match="exceeds 2\\^levels"):
        W.agg.aggregate(W.proofs * 2)
    with pytest.raises(api.VpbsError, match="count is 0"):
        W.agg.aggregate([])
    assert W.agg.aggregate(W.proofs[:2]) == good
    assert W.agg.last_run()["nodes"] == 1


def test_the_tool_aggregates_and_verifies_both_ways():
    """tools/prove_batch.py --aggregate on the N = 8, n = 6 set: three proofs under two key sets fold into a depth-2 aggregate of three
    nodes that the host and the device accept"""
    import json
    import os
    import subprocess
    import sys
    export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, 6, LOG_N)
    export_circuits.ensure_aggregate_circuits(N, K, ELL, LOGB, 6, LOG_N, LEVELS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "tools", "prove_batch.py"), "--n8", "--keys", "2", "--count", "3",
                        "--chains", "2", "--witness-batch", "3", "--aggregate"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a = json.loads(r.stdout.strip().splitlines()[-1])
    g = a["aggregate"]
    assert (a["accepted"], g["count"], g["depth"], g["nodes"], g["accepted"], g["host"], g["device"]) == (3, 3, 2, 3, True, [True, ""], [True, ""]), a
    assert g["bytes"] < g["leaf_bytes_total"] and g["level_degree_bits"] == [14, 14]
