"""GPU tests (-m gpu) of the batched evaluation of a program on a key ring (vpbs_program_run_batch, csrc/program.hip; api.Program.run_batch):
one program, many input sets, instance b under the key set of ring slot key_of[b], level l of all instances in one key-ring launch per
max_batch rows.  The yardstick is existing code, word for word: tests/program_oracle.py's evaluate (and api.Program.run) on a one-key
Bootstrapper per key set.  Exact field arithmetic: every comparison is word for word."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pbs_batch_oracle as B
import program_oracle as O
import tfhe_oracle as T
import vpbs_amd
from vpbs_amd import api

pytestmark = pytest.mark.gpu
P = api.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)       # main.rs:29-30
MARK = np.uint64(0xA5A5A5A5A5A5A5A5)

# the program of tests/test_gpu_program.py: 3 inputs, 9 gates, levels 1 1 2 1 3 1 2 3 1 (the caller's order interleaves them), fan-in 0 to
# 5, coefficients p - 1 and 2^32, non-zero constants, two luts
NINE = [([(0, 1)], 0, 0),
        ([], 0x123456789ABCDEF, 1),
        ([(3, P - 1), (1, 1 << 32)], 0, 0),
        ([(2, 1), (0, 5)], 0, 1),
        ([(5, 1), (3, 1), (4, 7), (0, 3), (6, 2)], 0, 1),
        ([(1, 1)], 0, 0),
        ([(8, 1), (4, P - 2)], 0, 0),
        ([(5, 3)], P - 1, 1),
        ([(2, 1)], 0, 0)]


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    yield c
    c.close()


def oracle_keys(log_n, K, ELL, LOGB, n, seed):
    ring = T.Ring(log_n)
    rng = np.random.default_rng(seed)
    s_to, s_lwe, s_glwe, bsk, ksk = T.pbs_setup(ring, rng, n, K, ELL, LOGB)
    return dict(ring=ring, rng=rng, s_to=s_to, s_lwe=s_lwe, bsk_flat=np.stack([T.flatten_ggsw(g) for g in bsk]), ksk_flat=T.flatten_ggsw(ksk))


def ring_of(ctx, keys, K, ELL, LOGB, N, n, max_keys, max_batch):
    kr = api.KeyRing(ctx, K, ELL, LOGB, N, n, max_keys=max_keys, max_batch=max_batch)
    assert [kr.add(k["bsk_flat"], k["ksk_flat"]) for k in keys] == list(range(len(keys)))
    return kr


def per_instance(ctx, keys, K, ELL, LOGB, key_of, run):
    """run(Bootstrapper of instance b's key set, b) for every instance, stacked output by output: the yardstick of a batch"""
    bss = {k: api.Bootstrapper(ctx, keys[k]["bsk_flat"], keys[k]["ksk_flat"], K, ELL, LOGB, max_batch=3) for k in sorted(set(key_of))}
    rows = [run(bss[k], b) for b, k in enumerate(key_of)]
    for bs in bss.values():
        bs.close()
    return tuple(np.stack([r[i] for r in rows]) for i in range(3))


def same(got, want):
    for name, g, w in zip(("wires", "gate_cts", "out_cts"), got, want):
        assert g.shape == w.shape and (g == w).all(), (name, np.argwhere(g != w)[:4].tolist())


@pytest.fixture(scope="module")
def small(ctx):
    """shape (3,2,4,5,6): three key sets of tfhe_oracle.pbs_setup, made once and read by several tests"""
    log_n, K, ELL, LOGB, n = 3, 2, 4, 5, 6
    return dict(log_n=log_n, K=K, ELL=ELL, LOGB=LOGB, n=n, N=1 << log_n, keys=[oracle_keys(log_n, K, ELL, LOGB, n, 811 + 10 * k) for k in range(3)])


@pytest.mark.parametrize("log_n,K,ELL,LOGB,n", [(6, 2, 8, 8, 5), (3, 2, 4, 5, 6), (6, 3, 3, 7, 40), (5, 2, 4, 5, 9)])
def test_every_instance_is_the_composition_under_its_own_key(ctx, log_n, K, ELL, LOGB, n):
    """5 instances with key_of = [2, 0, 1, 0, 2] on a ring of max_batch 4: level 1 is 25 rows in 7 chunks, the last partial, boundaries
    inside instances, chunks that mix key sets; all three outputs of every instance are the oracle's under that instance's key, for the
    list and the CSR form of the program"""
    keys = [oracle_keys(log_n, K, ELL, LOGB, n, 277 + 10 * k + log_n + K) for k in range(3)]
    N, key_of = 1 << log_n, [2, 0, 1, 0, 2]
    delta = T.get_delta(4)
    rng = keys[0]["rng"]
    inputs = np.array([[T.lwe_encrypt(keys[k]["rng"], keys[k]["s_lwe"], delta * m % P) for m in ((b + 1) % 2, b % 2, 1)]
                       for b, k in enumerate(key_of)], np.uint64)
    testvs = np.stack([np.array(T.get_testv(keys[0]["ring"], 2, delta), np.uint64), rng.integers(0, P, size=N, dtype=np.uint64)])
    want = per_instance(ctx, keys, K, ELL, LOGB, key_of, lambda bs, b: O.evaluate(bs, 3, NINE, inputs[b], testvs))
    kr = ring_of(ctx, keys, K, ELL, LOGB, N, n, 4, 4)
    for form in (NINE, O.csr(NINE)):
        prog = api.Program(ctx, 3, form, 2)
        same(prog.run_batch(kr, inputs, key_of, testvs), want)
        wires, cts, out = prog.run_batch(kr, inputs, np.array(key_of, np.int64), testvs, gate_cts=False, out_cts=False)
        assert cts is None and out is None and (wires == want[0]).all()
        prog.close()
    kr.close()


def test_device_pointers(ctx, small):
    """inputs and test vectors in HBM; all three outputs, and only d_wires asked for: what the host form gives"""
    import torch
    S = small
    K, N, n, keys = S["K"], S["N"], S["n"], S["keys"]
    key_of = [1, 2, 0, 1]
    rng = np.random.default_rng(31)
    inputs = rng.integers(0, P, size=(4, 3, n + 1), dtype=np.uint64)
    testvs = rng.integers(0, P, size=(2, N), dtype=np.uint64)
    kr = ring_of(ctx, keys, K, S["ELL"], S["LOGB"], N, n, 3, 5)
    prog = api.Program(ctx, 3, NINE, 2)
    want = prog.run_batch(kr, inputs, key_of, testvs)
    same(want, per_instance(ctx, keys, K, S["ELL"], S["LOGB"], key_of, lambda bs, b: prog.run(bs, inputs[b], testvs)))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    back = lambda d: d.cpu().numpy().view(np.uint64)
    d_in, d_tv = t(inputs), t(testvs)
    d_w = torch.zeros((4, 12, n + 1), dtype=torch.int64, device="cuda")
    d_c = torch.zeros((4, 9, n + 1), dtype=torch.int64, device="cuda")
    d_o = torch.zeros((4, 9, K, N), dtype=torch.int64, device="cuda")
    d_w2 = torch.zeros_like(d_w)
    torch.cuda.synchronize()         # torch fills on its stream, the run is on the context's own
    assert prog.run_batch_device(kr, d_in.data_ptr(), 4, key_of, d_tv.data_ptr(), d_w.data_ptr(), d_c.data_ptr(), d_o.data_ptr()) == 3
    same((back(d_w), back(d_c), back(d_o)), want)
    assert prog.run_batch_device(kr, d_in.data_ptr(), 4, key_of, d_tv.data_ptr(), d_w2.data_ptr()) == 3
    assert (back(d_w2) == want[0]).all()
    prog.close()
    kr.close()


def test_degenerate_sizes(ctx, small):
    """one instance under a one-key ring is Program.run on that key's Bootstrapper; no instances and a program without gates return
    without a bootstrap launch and with the right shapes"""
    S = small
    K, ELL, LOGB, N, n, keys = S["K"], S["ELL"], S["LOGB"], S["N"], S["n"], S["keys"]
    rng = np.random.default_rng(32)
    inputs = rng.integers(0, P, size=(1, 3, n + 1), dtype=np.uint64)
    testvs = rng.integers(0, P, size=(2, N), dtype=np.uint64)
    kr = ring_of(ctx, keys[:1], K, ELL, LOGB, N, n, 1, 2)
    prog = api.Program(ctx, 3, NINE, 2)
    bs = api.Bootstrapper(ctx, keys[0]["bsk_flat"], keys[0]["ksk_flat"], K, ELL, LOGB, max_batch=2)
    want = prog.run(bs, inputs[0], testvs)
    bs.close()
    same(prog.run_batch(kr, inputs, [0], testvs), tuple(w[None] for w in want))
    ctx.timing_enable(1)
    ctx.timing_report()
    wires, cts, out = prog.run_batch(kr, inputs[:0], [], testvs)
    assert wires.shape == (0, 12, n + 1) and cts.shape == (0, 9, n + 1) and out.shape == (0, 9, K, N)
    L = api.lib()
    assert L.vpbs_program_run_batch(prog.h, kr.h, None, 0, None, None, None, None, None, 0) == 3      # nothing to read: the levels
    empty = api.Program(ctx, 3, [], 1)
    three = rng.integers(0, P, size=(3, 3, n + 1), dtype=np.uint64)
    wires, cts, out = empty.run_batch(kr, three, [0, 0, 0], testvs[:1])
    assert (wires == three).all() and cts.shape == (3, 0, n + 1) and out.shape == (3, 0, K, N)
    assert L.vpbs_program_run_batch(empty.h, kr.h, three.ctypes.data, 3, np.zeros(3, np.uint32).ctypes.data, None, None, None, None, 0) == 0
    rep = ctx.timing_report()
    ctx.timing_enable(0)
    assert "pbs_keyring" not in rep and "lwe_combine" not in rep, rep
    empty.close()
    prog.close()
    kr.close()


def test_edge_words(ctx, small):
    """the edge-word program of tests/test_gpu_program.py for two instances under two keys: input words 0, p - 1, 2^63 and words at or
    above p are reduced by the combination; wires show the inputs as given; every gate input is canonical"""
    S = small
    K, ELL, LOGB, N, n, keys = S["K"], S["ELL"], S["LOGB"], S["N"], S["n"], S["keys"]
    rng = np.random.default_rng(4321)
    inputs = rng.integers(0, P, size=(2, 2, n + 1), dtype=np.uint64)
    for b in range(2):
        inputs[b, 0, :5] = np.array([0, P - 1, 1 << 63, P, P + 5], np.uint64)
        inputs[b, 0, n] = np.uint64((1 << 64) - 1 - b)                           # the body, at or above p
        inputs[b, 1, 0], inputs[b, 1, 1] = np.uint64(P + (1 << 31) + b), np.uint64(P - 1)
    const = 0xFFFFFFFF00000000                                                # p - 1
    gates = [([(0, 1)], 0, 0),                       # the identity: the input, reduced
             ([(1, 1), (1, P - 1)], 0, 0),           # w + (p - 1) w
             ([], const, 0),                         # a constant alone
             ([(0, P - 1), (1, 1 << 32)], 1, 0),     # edge words under edge coefficients
             ([(2, 1), (3, 1), (4, P - 1)], 0, 0)]   # level 2
    testvs = rng.integers(0, P, size=(1, N), dtype=np.uint64)
    key_of = [1, 0]
    want = per_instance(ctx, keys, K, ELL, LOGB, key_of, lambda bs, b: O.evaluate(bs, 2, gates, inputs[b], testvs))
    kr = ring_of(ctx, keys[:2], K, ELL, LOGB, N, n, 2, 3)
    prog = api.Program(ctx, 2, gates, 1)
    got = prog.run_batch(kr, inputs, key_of, testvs)
    prog.close()
    kr.close()
    same(got, want)
    wires, gate_cts, _ = got
    assert (wires[:, :2] == inputs).all()                                     # inputs are shown as given
    assert (gate_cts < np.uint64(P)).all()
    for b in range(2):
        assert gate_cts[b, 0].tolist() == [int(w) % P for w in inputs[b, 0]] and not gate_cts[b, 1].any()
        assert gate_cts[b, 2].tolist() == [0] * n + [const]


def test_slots(ctx, small):
    """after remove(1), a key_of naming slot 1 or slot max_keys is refused with the instance and the slot in the message and no output
    word written; the next legal run is right; after add reuses slot 1 with another key set its instances follow the new key"""
    S = small
    K, ELL, LOGB, N, n, keys = S["K"], S["ELL"], S["LOGB"], S["N"], S["n"], S["keys"]
    fourth = oracle_keys(S["log_n"], K, ELL, LOGB, n, 999)
    rng = np.random.default_rng(33)
    inputs = rng.integers(0, P, size=(4, 3, n + 1), dtype=np.uint64)
    testvs = rng.integers(0, P, size=(2, N), dtype=np.uint64)
    kr = ring_of(ctx, keys, K, ELL, LOGB, N, n, 3, 4)
    prog = api.Program(ctx, 3, NINE, 2)
    kr.remove(1)
    L = api.lib()
    wires, cts, out = np.full((4, 12, n + 1), MARK, np.uint64), np.full((4, 9, n + 1), MARK, np.uint64), np.full((4, 9, K, N), MARK, np.uint64)
    for key_of, index, slot, word in (([0, 2, 3, 0], 2, 3, "out of range"), ([0, 2, 2, 1], 3, 1, "empty")):
        ko = np.array(key_of, np.uint32)
        rc = L.vpbs_program_run_batch(prog.h, kr.h, inputs.ctypes.data, 4, ko.ctypes.data, testvs.ctypes.data, wires.ctypes.data, cts.ctypes.data,
                                      out.ctypes.data, 0)
        msg = L.vpbs_last_error(ctx.h).decode()
        assert rc == -1, rc                                                   # VPBS_ERR_INVALID
        assert "key_of[%d] = %d" % (index, slot) in msg and word in msg and "instance %d" % index in msg, msg
        assert (wires == MARK).all() and (cts == MARK).all() and (out == MARK).all()
    with pytest.raises(api.VpbsError, match=r"key_of\[3\] = 1.*instance 3"):
        prog.run_batch(kr, inputs, [0, 2, 2, 1], testvs)
    # null pointers with something to read, a null ring: refused, nothing written
    ko = np.array([0, 2, 2, 0], np.uint32)
    for a in ((None, 4, ko.ctypes.data, testvs.ctypes.data), (inputs.ctypes.data, 4, None, testvs.ctypes.data), (inputs.ctypes.data, 4, ko.ctypes.data, None)):
        assert L.vpbs_program_run_batch(prog.h, kr.h, *a, wires.ctypes.data, cts.ctypes.data, out.ctypes.data, 0) == -1
    assert L.vpbs_program_run_batch(prog.h, None, inputs.ctypes.data, 4, ko.ctypes.data, testvs.ctypes.data, wires.ctypes.data, None, None, 0) == -1
    assert (wires == MARK).all() and (cts == MARK).all() and (out == MARK).all()
    # the next legal run
    key_of = [0, 2, 2, 0]
    sets = {0: keys[0], 2: keys[2]}
    same(prog.run_batch(kr, inputs, key_of, testvs), per_instance(ctx, sets, K, ELL, LOGB, key_of, lambda bs, b: prog.run(bs, inputs[b], testvs)))
    # slot 1 again, with a key set the ring has not seen
    assert kr.add(fourth["bsk_flat"], fourth["ksk_flat"]) == 1
    key_of = [1, 2, 1, 0]
    sets = {0: keys[0], 1: fourth, 2: keys[2]}
    got = prog.run_batch(kr, inputs, key_of, testvs)
    same(got, per_instance(ctx, sets, K, ELL, LOGB, key_of, lambda bs, b: prog.run(bs, inputs[b], testvs)))
    old = per_instance(ctx, {1: keys[1]}, K, ELL, LOGB, [1], lambda bs, b: prog.run(bs, inputs[0], testvs))
    assert not (got[0][0] == old[0][0]).all()                                 # instance 0 is under slot 1: the new key shows
    prog.close()
    kr.close()


def test_messages_at_sigma_zero(ctx):
    """the depth-3 program of tests/test_gpu_program.py without noise for 3 instances with different messages under 2 keys: every wire
    decrypts to exactly delta * m under its own key"""
    log_n, K, ELL, LOGB, n = 6, 2, 8, 8, 5
    keys = [oracle_keys(log_n, K, ELL, LOGB, n, 4242 + k) for k in range(2)]
    ring0 = keys[0]["ring"]
    delta = T.get_delta(4)
    testvs = np.array([T.get_testv(ring0, 2, delta)], np.uint64)
    one = lambda w: ([(w, 1)], 0, 0)
    add = lambda a, b: ([(a, 1), (b, 1)], 0, 0)
    gates = [one(0), one(1), one(2), one(3),                 # wires 4 .. 7: the inputs a b c d
             add(4, 5), add(7, 6), add(4, 7), one(5),        # wires 8 .. 11: a+b, d+c, a+d, b
             one(8), add(10, 11), add(10, 4)]                # wires 12 .. 14: a+b, a+d+b, a+d+a
    # messages with every sum in {0, 1}: the identity test vector on {0, 1} returns them
    msgs = [[0, 1, 1, 0], [0, 0, 0, 1], [0, 1, 0, 0]]
    key_of = [1, 0, 1]

    def all_messages(m):
        a, b, c, d = m
        w = [a, b, c, d, a, b, c, d, a + b, d + c, a + d, b]
        return w + [w[8], w[10] + w[11], w[10] + w[4]]
    want_msgs = [all_messages(m) for m in msgs]
    assert all(0 <= v <= 1 for w in want_msgs for v in w)
    inputs = np.array([[T.lwe_encrypt(keys[k]["rng"], keys[k]["s_lwe"], delta * m % P) for m in ms] for ms, k in zip(msgs, key_of)], np.uint64)
    kr = ring_of(ctx, keys, K, ELL, LOGB, 1 << log_n, n, 2, 5)
    prog = api.Program(ctx, 4, gates, 1)
    assert prog.levels()[1] == 3
    wires, gate_cts, out_cts = prog.run_batch(kr, inputs, key_of, testvs)
    same((wires, gate_cts, out_cts), per_instance(ctx, keys, K, ELL, LOGB, key_of, lambda bs, b: O.evaluate(bs, 4, gates, inputs[b], testvs)))
    prog.close()
    kr.close()
    for b, k in enumerate(key_of):
        assert [B.lwe_decrypt(keys[k]["s_lwe"], w) for w in wires[b]] == [delta * m % P for m in want_msgs[b]], b
        assert [T.glwe_decrypt(ring0, keys[k]["s_to"][:K - 1], B.glwe_list(o), K)[0] for o in out_cts[b]] == \
            [delta * m % P for m in want_msgs[b][4:]], b


def test_the_papers_parameters_and_noise(ctx):
    """N = 1024, n = 728: three keygen_device key sets at the paper's sigmas in a ring of max_batch 5; a 2-level program of 4 gates for 4
    instances in mixed slot order (level 1: 12 rows in 3 chunks).  Every word is Program.run's on the matching Bootstrapper; the
    identity gates decrypt to their messages under their own keys"""
    N, K, ELL, LOGB, n = 1024, 2, 4, 5, 728
    keys = [ctx.keygen_device(N, K, ELL, LOGB, n, 0x5EED + k, *SIGMAS) for k in range(3)]
    testv, delta = api.testv(N, 2)
    testvs = testv.reshape(1, N)
    key_of = [2, 0, 1, 0]
    msgs = [[1, 0], [0, 1], [1, 1], [0, 0]]
    inputs = np.stack([np.stack([api.lwe_encrypt(keys[k]["params"], keys[k]["s_lwe"], delta * m % P, nonce=300 + 2 * b + i) for i, m in enumerate(ms)])
                       for b, (ms, k) in enumerate(zip(msgs, key_of))])
    gates = [([(0, 1)], 0, 0), ([(1, 1)], 0, 0), ([(0, 1), (1, P - 1)], 0, 0),      # level 1: a, b, a difference
             ([(2, 1)], 0, 0)]                                                      # level 2: a
    prog = api.Program(ctx, 2, gates, 1)
    assert prog.levels()[0].tolist() == [1, 1, 1, 2]
    kr = api.KeyRing(ctx, K, ELL, LOGB, N, n, max_keys=4, max_batch=5)
    bss = []
    for d in keys:
        kr.add(d["d_bsk"], d["d_ksk"], keys_on_device=True)
        bss.append(api.Bootstrapper(ctx, d["d_bsk"], d["d_ksk"], K, ELL, LOGB, max_batch=4, N=N, n_lwe=n, keys_on_device=True))
    got = prog.run_batch(kr, inputs, key_of, testvs)
    rows = [prog.run(bss[k], inputs[b], testvs) for b, k in enumerate(key_of)]
    prog.close()
    kr.close()
    for bs in bss:
        bs.close()
    for d in keys:
        ctx.device_free(d["d_bsk"])
        ctx.device_free(d["d_ksk"])
    same(got, tuple(np.stack([r[i] for r in rows]) for i in range(3)))
    for b, (k, (ma, mb)) in enumerate(zip(key_of, msgs)):
        for g, m in ((0, ma), (1, mb), (3, ma)):
            assert B.round_message(api.lwe_decrypt(keys[k]["s_lwe"], got[0][b, 2 + g]), delta, 2) == m, (b, g)


def test_the_tool_in_a_fresh_process():
    """tools/run_program.py --n8 --instances 3 --keys 2: both legs give the same wires, the batched leg queues fewer bootstrap launches
    than the per-instance leg, the checked outputs decrypt under their own keys"""
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "run_program.py"), "--n8", "--instances", "3",
                        "--keys", "2"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["all_equal"] is True and line["instances"] == 3 and line["keys"] == 2 and line["levels"] == 3
    assert 0 < line["batch"]["pbs_launches"] < line["baseline"]["pbs_launches"], line
    assert line["batch"]["pbs_launches"] == 3 and line["baseline"]["pbs_launches"] == 9
    assert line["decrypted"] == 3 * 8 and line["decrypted_checked"] >= 3 and line["decrypted_correct"] == line["decrypted_checked"]
