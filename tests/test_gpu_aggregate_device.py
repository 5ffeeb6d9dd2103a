"""GPU tests (-m gpu): the aggregator's device witness -- Aggregator.set_device_witness, the node witnesses of a tree level
in one device batch, Aggregator.aggregate_many, and Program.prove_aggregate_batch handing all instances to one run.  The yardstick is the
host path of the same Aggregator on the same leaves: every aggregate byte for byte, the preset matrix and one node's wires word for word
against the host's vector and vpbs_witness_plan_run.  The world is that of tests/test_gpu_aggregate.py (N = 8, n = 1: leaf proofs of the
2^13 cyclic circuit, level circuits 1 - 3 at 2^14), built once here.  No tolerance anywhere."""
import numpy as np
import pytest

import export_circuits
import vpbs_amd
from test_gpu_aggregate import N, K, N_LWE, LEVELS, World
from vpbs_amd import api, circuit_file

pytestmark = pytest.mark.gpu
NODES = {1: 1, 2: 1, 3: 3, 5: 6}   # distinct nodes of a tree of that many leaves (5: 3 + 2 + 1)


@pytest.fixture(scope="module")
def world():
    c = vpbs_amd.Context(0, log_n_max=16)
    w = World(c)
    for count in NODES:   # the yardstick: the host path's aggregates, made before the device witness is ever on
        w.aggregate(count)
        assert w.runs[count]["nodes"] == NODES[count] and w.agg.device_stats()["nodes"] == 0
    yield w
    w.agg.set_device_witness(0)
    w.close()
    c.close()


@pytest.mark.parametrize("count", [1, 2, 3, 5])
def test_the_device_path_makes_the_host_paths_bytes(world, count):
    """one leaf with itself (both slots read the same child row), two leaves, three (the padding node (2, 2)), five (the dedup: 3 + 2 + 1
    nodes); max_nodes = 4 holds every level, so each level is one batch"""
    W = world
    W.agg.set_device_witness(4)
    blob = W.agg.aggregate(W.proofs[:count])
    assert blob == W.memo[count]
    assert W.both(blob, count, W.statement(count)) == (True, api.AGG_OK)
    run, dev = W.agg.last_run(), W.agg.device_stats()
    d = api.aggregate_depth(count)
    assert (run["nodes"], run["depth"]) == (NODES[count], d), run
    assert (dev["nodes"], dev["batches"]) == (NODES[count], d), dev
    assert dev["witness_us"] > 0 and dev["gather_us"] > 0 and run["witness_ms"] > 0 and run["prove_ms"] > 0


@pytest.mark.parametrize("max_nodes,batches", [(1, 3 + 2 + 1), (2, 2 + 1 + 1)])
def test_a_level_wider_than_max_nodes_goes_in_chunks(world, max_nodes, batches):
    """five leaves: level 1's three nodes in chunks of 1 + 1 + 1 and 2 + 1, level 2's two in 1 + 1 and 2: the same bytes"""
    W = world
    W.agg.set_device_witness(max_nodes)
    assert W.agg.aggregate(W.proofs) == W.memo[5]
    dev = W.agg.device_stats()
    assert (dev["nodes"], dev["batches"]) == (6, batches), dev


def test_one_level_1_node_word_for_word(world):
    """the preset matrix of ag_presets_kernel is the host's PartialWitness vector, instances innermost -- for one node, for a chunk whose
    nodes share rows and read one row in both slots, and for 37 nodes of level 2 (two tiles of instances, the second partial; a row length
    that is no multiple of the tile's 64 words); the wires the device plan makes of it are vpbs_witness_plan_run's, unset wires included"""
    import torch
    W = world
    W.agg.set_device_witness(40)
    (fa, pa), (fb, pb), (fc, pc) = W.leaf(0), W.leaf(1), W.leaf(2)
    rows = np.stack([np.concatenate([fa, pa]), np.concatenate([fb, pb]), np.concatenate([fc, pc])])
    vals = lambda a, b: np.concatenate([rows[a], rows[b], W.vk0])
    one = W.agg.test_preset_matrix(1, rows[:2], [[0, 1]])
    assert one.shape == (len(W.levels[0].preset_flat), 1) and (one[:, 0] == vals(0, 1)).all()
    pairs = [[0, 1], [2, 2], [1, 0]]
    three = W.agg.test_preset_matrix(1, rows, pairs)
    assert (three == np.stack([vals(a, b) for a, b in pairs], axis=1)).all()
    # level 2 at a shape of its own: the words are arbitrary, only where they land is checked
    rng = np.random.default_rng(5)
    lv = W.levels[1]
    row_words = lv.meta["proof_words"] + 4 + 68
    assert row_words % 64 != 0 and 2 * row_words + 2 * 68 == len(lv.preset_flat)
    rows2 = rng.integers(0, api.P, size=(7, row_words), dtype=np.uint64)
    pairs2 = rng.integers(0, 7, size=(37, 2))
    want = np.stack([np.concatenate([rows2[a], rows2[b], W.vks[:2].reshape(-1)]) for a, b in pairs2], axis=1)
    got = W.agg.test_preset_matrix(2, rows2, pairs2)
    assert got.shape == want.shape and (got == want).all(), np.argwhere(got != want)[:4].tolist()
    # the wires of the node (leaf 0, leaf 1): the level's full plan on the device over the kernel's matrix against the host plan
    d = W.levels[0]
    plan = d.circuit.witness_plan(d.preset_pos)
    dev = api.WitnessDevice(W.ctx, plan, max_batch=1)
    try:
        dev.run(np.ascontiguousarray(one))
        d_w = torch.zeros((135, 1 << d.log_n), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()   # the fill runs on torch's stream, the gather on the context's own
        dev.wires(0, d_w.data_ptr())
        host = plan.run(vals(0, 1))
        assert (d_w.cpu().numpy().view(np.uint64).reshape(-1) == np.asarray(host).reshape(-1)).all()
    finally:
        dev.free()
        plan.free()
    with pytest.raises(api.VpbsError, match="status"):
        W.agg.test_preset_matrix(1, rows, [[0, 3]])        # a row the chunk does not have
    with pytest.raises(api.VpbsError, match="status"):
        W.agg.test_preset_matrix(4, rows, [[0, 1]])        # a level the aggregator does not have


@pytest.mark.parametrize("counts", [[1, 3, 2], [5, 1]])
def test_many_trees_in_one_run(world, counts):
    """the level-l nodes of all trees in the same batches: every aggregate is its single aggregate, one batch per level of the deepest tree
    (max_nodes = 4 holds the four level-1 nodes of either forest), callbacks in tree order although a shallow tree is through first"""
    W = world
    W.agg.set_device_witness(4)
    order = []
    blobs = W.agg.aggregate_many([W.proofs[:c] for c in counts], on_aggregate=lambda t, b: order.append(t))
    assert order == list(range(len(counts)))
    assert blobs == [W.memo[c] for c in counts]
    run, dev = W.agg.last_run(), W.agg.device_stats()
    deepest = max(api.aggregate_depth(c) for c in counts)
    assert (run["nodes"], run["depth"]) == (sum(NODES[c] for c in counts), deepest), run
    assert (dev["nodes"], dev["batches"]) == (run["nodes"], deepest), dev


def test_a_bad_leaf_of_the_second_tree_is_refused_before_anything_runs(world):
    W = world
    W.agg.set_device_witness(4)
    tampered = bytearray(W.proofs[1])
    tampered[8 * 300] ^= 1
    called = []
    with pytest.raises(api.VpbsError, match=r"tree 1, leaf 1: the proof does not verify; nothing was proven"):
        W.agg.aggregate_many([W.proofs[:2], [W.proofs[0], bytes(tampered), W.proofs[2]]], on_aggregate=lambda t, b: called.append(t))
    assert not called and W.agg.last_run()["nodes"] == 0
    assert (W.agg.device_stats()["nodes"], W.agg.device_stats()["batches"]) == (0, 0)
    # the single run refuses its bad leaf by its own index, as on the host path, without a device witness run
    with pytest.raises(api.VpbsError, match=r"leaf 1: the proof does not verify; nothing was proven"):
        W.agg.aggregate([W.proofs[0], bytes(tampered)])
    assert W.agg.last_run()["nodes"] == 0 and W.agg.device_stats()["batches"] == 0
    # what the Python checks refuse, from the C ABI: decreasing offsets, an empty tree, a tree above 2^levels -- before anything is queued
    C = api.C
    L, err = api.lib(), C.create_string_buffer(256)
    szp = lambda a: np.array(a, np.uint64).ctypes.data_as(C.POINTER(C.c_size_t))
    cb = api.AGGREGATE_TREE_FN(lambda *a: called.append(a))

    def refused(offsets, counts):
        assert L.vpbs_aggregator_run_many(W.agg.h, (C.c_uint8 * 8)(), szp(offsets), szp(counts), len(counts), cb, None, err, 256) == api.ERR_INVALID
        return err.value.decode()
    assert "offsets decrease at leaf 1" in refused([0, 8, 4], [1, 1])
    assert "tree 1 is empty" in refused([0, 8], [1, 0])
    assert "tree 0: count 9 exceeds 2^levels = 8" in refused([0] * 10, [9])
    assert "n_trees is 0" in refused([0], [])
    assert not called
    with pytest.raises(ValueError, match="tree 1 is empty"):
        W.agg.aggregate_many([W.proofs[:1], []])


def test_back_on_the_host_path(world):
    W = world
    W.agg.set_device_witness(4)
    assert W.agg.aggregate(W.proofs[:2]) == W.memo[2] and W.agg.device_stats()["nodes"] == 1
    W.agg.set_device_witness(0)
    assert W.agg.aggregate(W.proofs[:3]) == W.memo[3]
    assert W.agg.last_run()["nodes"] == 3 and W.agg.device_stats() == dict(nodes=0, batches=0, witness_us=0, gather_us=0)
    # a many-run on the host path is a loop over the single run
    order = []
    assert W.agg.aggregate_many([W.proofs[:1], W.proofs[:2]], on_aggregate=lambda t, b: order.append(t)) == [W.memo[1], W.memo[2]]
    assert order == [0, 1] and W.agg.last_run()["nodes"] == 2 and W.agg.device_stats()["nodes"] == 0


def test_a_program_batch_is_one_run_over_all_instances():
    """Program.prove_aggregate_batch of the four-gate program of tests/test_gpu_program_aggregate.py for two instances under two key sets:
    with the device witness on, the aggregates are those of the host path, and the aggregator ran ONCE -- its last run holds the nodes of
    both instances and as many device batches as one tree has levels"""
    from test_gpu_program_aggregate import ELL, FOUR, LOGB, LOG_N, SIGMAS, n6
    P = api.P
    ctx = vpbs_amd.Context(0, log_n_max=16)
    cyc, dum = [circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, n6, LOG_N)]
    levels = [circuit_file.load(p) for p in export_circuits.ensure_aggregate_circuits(N, K, ELL, LOGB, n6, LOG_N, LEVELS)]
    keys = [ctx.keygen(N, K, ELL, LOGB, n6, seed, *SIGMAS) for seed in (77, 78)]
    delta = api.testv(N, 2)[1]
    testvs = np.stack([api.lut_testv_multi(N, 2, np.array([[0, 1], [1, 0]], np.uint64), delta)[0],
                       np.random.default_rng(3).integers(0, P, size=N, dtype=np.uint64)])
    key_of = [1, 0]
    inputs = np.stack([np.stack([api.lwe_encrypt(keys[k]["params"], keys[k]["s_lwe"], delta * m % P, nonce=30 + 10 * k + i) for i, m in enumerate([1, 0])])
                       for k in key_of])
    rp = api.RingProver(0, cyc, dum, K, ELL, LOGB, N, n6, max_keys=2, chains=2, witness_batch=3)
    prog = api.Program(ctx, 2, FOUR, 2)
    agg = None
    try:
        assert [rp.add(k["bsk"], k["ksk"]) for k in keys] == [0, 1]
        agg = api.Aggregator(ctx, cyc, rp.verifier_data()[0], levels)
        want, wires, out_cts = prog.prove_aggregate_batch(rp, agg, inputs, key_of, testvs)
        assert agg.last_run()["nodes"] == 3 and agg.device_stats()["nodes"] == 0          # the last of two runs: one instance's 2 + 1 nodes
        agg.set_device_witness(4)
        order = []
        got, wires2, out_cts2 = prog.prove_aggregate_batch(rp, agg, inputs, key_of, testvs, on_aggregate=lambda b, _: order.append(b))
        assert order == [0, 1] and got == want and (wires2 == wires).all() and (out_cts2 == out_cts).all()
        run, dev = agg.last_run(), agg.device_stats()
        assert (run["nodes"], run["depth"]) == (6, 2), run                                   # ONE run over both instances
        assert (dev["nodes"], dev["batches"]) == (6, 2), dev                                 # level 1: 2 + 2 nodes in one batch; level 2: 1 + 1
    finally:
        if agg is not None:
            agg.close()
        prog.close()
        rp.close()
        ctx.close()
