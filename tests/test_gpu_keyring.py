"""GPU tests (-m gpu) of the key ring (vpbs_keyring_*, api.KeyRing; csrc/pbs_keyring.hip): mixed batches under many resident key sets in
one launch.  Two yardsticks: the CPU restatement (tests/tfhe_oracle.py) under each ciphertext's own key on small shapes, and the one-key
Bootstrapper at the paper's parameters.  Exact field arithmetic: every comparison is word for word."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pbs_batch_oracle as B
import tfhe_oracle as T
import vpbs_amd
from vpbs_amd import api

pytestmark = pytest.mark.gpu
P = api.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)       # main.rs:29-30
PAPER = dict(N=1024, K=2, ELL=4, LOGB=5, n=728, p=2)
MARK = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    yield c
    c.close()


@pytest.fixture(scope="module")
def paper(ctx):
    """the paper's parameters and noise: three seeded key sets left on the device, six ciphertexts in mixed order with the edge words in
    one mask, and what the one-key Bootstrapper of each key set gives for its rows -- computed once, read by several tests"""
    S = dict(PAPER)
    N, K, ELL, LOGB, n = S["N"], S["K"], S["ELL"], S["LOGB"], S["n"]
    S["keys"] = [ctx.keygen_device(N, K, ELL, LOGB, n, 0x5EED + k, *SIGMAS) for k in range(3)]
    S["testv"], S["delta"] = api.testv(N, S["p"])
    S["key_of"] = np.array([2, 0, 1, 1, 0, 2], np.uint32)
    S["msgs"] = [0, 1, 1, 0, 1, 0]
    S["cts"] = np.stack([api.lwe_encrypt(S["keys"][k]["params"], S["keys"][k]["s_lwe"], S["delta"] * m % P, nonce=20 + i)
                         for i, (k, m) in enumerate(zip(S["key_of"], S["msgs"]))])
    S["cts"][3, 0], S["cts"][3, 1], S["cts"][3, 2] = 0, P - 1, 1 << 63
    S["bs"] = [api.Bootstrapper(ctx, d["d_bsk"], d["d_ksk"], K, ELL, LOGB, max_batch=300, N=N, n_lwe=n, keys_on_device=True) for d in S["keys"]]
    S["want_out"], S["want_lwe"] = np.zeros((6, K, N), np.uint64), np.zeros((6, n + 1), np.uint64)
    for k in range(3):
        rows = np.flatnonzero(S["key_of"] == k)
        S["want_out"][rows], S["want_lwe"][rows] = S["bs"][k].run(S["cts"][rows], S["testv"])
    yield S
    for b in S["bs"]:
        b.close()
    for d in S["keys"]:
        ctx.device_free(d["d_bsk"])
        ctx.device_free(d["d_ksk"])


def paper_ring(ctx, S, max_batch=8, slots=3):
    ring = api.KeyRing(ctx, S["K"], S["ELL"], S["LOGB"], S["N"], S["n"], max_keys=4, max_batch=max_batch)
    for d in S["keys"][:slots]:
        ring.add(d["d_bsk"], d["d_ksk"], keys_on_device=True)
    return ring


def oracle_keys(log_n, K, ELL, LOGB, n, seed):
    ring = T.Ring(log_n)
    rng = np.random.default_rng(seed)
    s_to, s_lwe, s_glwe, bsk, ksk = T.pbs_setup(ring, rng, n, K, ELL, LOGB)
    return dict(ring=ring, rng=rng, s_lwe=s_lwe, bsk=bsk, ksk=ksk, bsk_flat=np.stack([T.flatten_ggsw(g) for g in bsk]), ksk_flat=T.flatten_ggsw(ksk))


@pytest.mark.parametrize("log_n,K,ELL,LOGB,n", [(6, 2, 8, 8, 5), (3, 2, 4, 5, 6), (6, 3, 3, 7, 40), (5, 2, 4, 5, 9)])
def test_bit_exact_against_the_oracle_under_each_ciphertexts_key(ctx, log_n, K, ELL, LOGB, n):
    """three key sets of tfhe_oracle.pbs_setup, a batch of 7 with key_of = [2,0,1,0,2,2,0], per-ciphertext random test vectors and a shared
    one, one mask with the edge words 0, p - 1, 2^63: every accumulator of every chain is tfhe_oracle.pbs_chain's under THAT ciphertext's
    key, out_ct its last, lwe_out the restated extraction; without accumulators the same words"""
    keys = [oracle_keys(log_n, K, ELL, LOGB, n, 177 + 10 * k + log_n + K) for k in range(3)]
    ring0 = keys[0]["ring"]
    N, count = ring0.n, 7
    key_of = [2, 0, 1, 0, 2, 2, 0]
    delta = T.get_delta(4)
    cts = np.array([T.lwe_encrypt(keys[k]["rng"], keys[k]["s_lwe"], delta * (i % 2) % P) for i, k in enumerate(key_of)], np.uint64)
    cts[3, 0], cts[3, 1], cts[3, 2] = 0, P - 1, 1 << 63
    shared = np.array(T.get_testv(ring0, 2, delta), np.uint64)
    per_ct = keys[0]["rng"].integers(0, P, size=(count, N), dtype=np.uint64)
    kr = api.KeyRing(ctx, K, ELL, LOGB, N, n, max_keys=3, max_batch=count)
    assert [kr.add(k["bsk_flat"], k["ksk_flat"]) for k in keys] == [0, 1, 2] and kr.count() == 3
    for testv in (per_ct, shared):
        out_ct, lwe_out, accs = kr.run(cts, key_of, testv, accumulators=True)
        assert accs.shape == (count, n + 2, K, N)
        for i in range(count):
            k = keys[key_of[i]]
            tv = testv[i] if testv.ndim == 2 else testv
            acc0 = [[0] * N for _ in range(K - 1)] + [[int(v) for v in tv]]
            want = T.pbs_chain(k["ring"], acc0, [int(v) for v in cts[i]], k["bsk"], k["ksk"], K, ELL, LOGB)
            for s in range(n + 2):
                assert (accs[i, s] == np.array(want[s], np.uint64)).all(), (i, s)
            assert (out_ct[i] == accs[i, n + 1]).all(), i
            assert lwe_out[i].tolist() == B.extract(want[-1], n), i
        out2, lwe2 = kr.run(cts, key_of, testv)
        assert (out2 == out_ct).all() and (lwe2 == lwe_out).all()
    assert kr.run(cts[:0], [], shared)[0].shape == (0, K, N)     # count == 0 is legal
    kr.close()


@pytest.mark.parametrize("log_n,K,ELL,LOGB,n", [(6, 2, 8, 8, 5), (3, 2, 4, 5, 6), (6, 3, 3, 7, 40), (5, 2, 4, 5, 9)])
def test_a_ring_of_one_slot_is_the_bootstrapper_word_for_word(ctx, log_n, K, ELL, LOGB, n):
    """one key set, a batch of 3 (a mask with the edge words, per-ciphertext test vectors): a KeyRing with ONE slot gives every accumulator,
    out_ct and lwe_out as a Bootstrapper of that key set does, with and without accumulators, through run and through run_from with
    start = [0, 2, n + 2] and acc_in taken from the first run.  At these shapes the ring holds 8, 4, 4 and 4 key words ahead per thread and
    the Bootstrapper none: the two kernels share one chain body, and this pins its prefetching paths against the plain one."""
    k = oracle_keys(log_n, K, ELL, LOGB, n, 311 + log_n + K)
    N, count = k["ring"].n, 3
    delta = T.get_delta(4)
    cts = np.array([T.lwe_encrypt(k["rng"], k["s_lwe"], delta * (i % 2) % P) for i in range(count)], np.uint64)
    cts[1, 0], cts[1, 1], cts[1, 2] = 0, P - 1, 1 << 63
    testv = k["rng"].integers(0, P, size=(count, N), dtype=np.uint64)
    key_of = np.zeros(count, np.uint32)
    bs = api.Bootstrapper(ctx, k["bsk_flat"], k["ksk_flat"], K, ELL, LOGB, max_batch=count)
    kr = api.KeyRing(ctx, K, ELL, LOGB, N, n, max_keys=1, max_batch=count)
    assert kr.add(k["bsk_flat"], k["ksk_flat"]) == 0
    want = bs.run(cts, testv, accumulators=True)
    assert want[2].shape == (count, n + 2, K, N) and want[2][:, n + 1].any()
    for got in (kr.run(cts, key_of, testv, accumulators=True), kr.run(cts, key_of, testv)):
        assert all((g == w).all() for g, w in zip(got, want)), len(got)
    start = [0, 2, n + 2]
    acc_in = np.stack([want[2][i, max(s, 1) - 1] for i, s in enumerate(start)])     # row 0 starts at step 0: its acc_in is not read
    want_from = bs.run_from(cts, start, acc_in, testv, accumulators=True)
    assert (want_from[0] == want[0]).all() and (want_from[1] == want[1]).all()     # a resumed chain ends where the whole one does
    for got in (kr.run_from(cts, key_of, start, acc_in, testv, accumulators=True), kr.run_from(cts, key_of, start, acc_in, testv)):
        assert all((g == w).all() for g, w in zip(got, want_from)), len(got)
    kr.close()
    bs.close()


def test_word_for_word_the_one_key_bootstrapper_at_the_papers_parameters(ctx, paper, monkeypatch):
    """three noisy key sets, a batch of 6 in mixed order: every out_ct and lwe_out row is Bootstrapper(key k).run's of that row, the
    outputs decrypt under their own keys, and 256, 512 and 1024 threads per ciphertext change no word"""
    S = paper
    ring = paper_ring(ctx, S)
    out_ct, lwe_out = ring.run(S["cts"], S["key_of"], S["testv"])
    ring.close()
    assert (out_ct == S["want_out"]).all() and (lwe_out == S["want_lwe"]).all()
    got = [B.round_message(api.lwe_decrypt(S["keys"][k]["s_lwe"], lwe_out[i]), S["delta"], S["p"]) for i, k in enumerate(S["key_of"])]
    assert got == S["msgs"]
    for threads in ("256", "512", "1024"):
        monkeypatch.setenv("VPBS_PBS_BATCH_THREADS", threads)
        ring = paper_ring(ctx, S)
        o, l = ring.run(S["cts"], S["key_of"], S["testv"])
        ring.close()
        assert (o == S["want_out"]).all() and (l == S["want_lwe"]).all(), threads
    monkeypatch.setenv("VPBS_PBS_BATCH_THREADS", "384")
    with pytest.raises(api.VpbsError, match="VPBS_PBS_BATCH_THREADS"):
        api.KeyRing(ctx, S["K"], S["ELL"], S["LOGB"], S["N"], S["n"], max_keys=2, max_batch=2)


def test_more_workgroups_than_compute_units(ctx, paper):
    """300 ciphertexts under 2 keys at the paper's shape (two 512-thread workgroups per CU): every row equals the Bootstrapper's"""
    S = paper
    key_of = np.array([(i * 7 + i // 5) % 2 for i in range(300)], np.uint32)
    cts = np.stack([api.lwe_encrypt(S["keys"][k]["params"], S["keys"][k]["s_lwe"], S["delta"] * (i % 2) % P, nonce=2000 + i)
                    for i, k in enumerate(key_of)])
    ring = paper_ring(ctx, S, max_batch=300, slots=2)
    out_ct, lwe_out = ring.run(cts, key_of, S["testv"])
    ring.close()
    for k in range(2):
        rows = np.flatnonzero(key_of == k)
        o, l = S["bs"][k].run(cts[rows], S["testv"])
        assert (out_ct[rows] == o).all() and (lwe_out[rows] == l).all(), k


def test_slots_are_reused_and_host_and_device_keys_mix(ctx):
    """add 3, remove the middle one, add a different key: it gets the freed number and runs use the new key; adopted device keys and
    uploaded host keys in one ring give the same words; all of key_of equal gives Bootstrapper.run's words"""
    N, K, ELL, LOGB, n = 256, 2, 4, 5, 100
    host = [ctx.keygen(N, K, ELL, LOGB, n, 0xC0DE + k, *SIGMAS) for k in range(4)]
    dev = ctx.keygen_device(N, K, ELL, LOGB, n, 0xC0DE + 2, *SIGMAS)       # key set 2 again, left on the device
    testv, delta = api.testv(N, 2)
    key_of = np.array([1, 0, 2, 1, 2], np.uint32)
    cts = np.stack([api.lwe_encrypt(host[0]["params"], host[0]["s_lwe"], delta * (i % 2) % P, nonce=i) for i in range(5)])

    def want(sets):
        out = np.zeros((5, K, N), np.uint64), np.zeros((5, n + 1), np.uint64)
        for slot, k in enumerate(sets):
            rows = np.flatnonzero(key_of == slot)
            bs = api.Bootstrapper(ctx, host[k]["bsk"], host[k]["ksk"], K, ELL, LOGB, max_batch=5)
            out[0][rows], out[1][rows] = bs.run(cts[rows], testv)
            bs.close()
        return out
    ring = api.KeyRing(ctx, K, ELL, LOGB, N, n, max_keys=3, max_batch=5)
    assert ring.add(host[0]["bsk"], host[0]["ksk"]) == 0
    assert ring.add(host[1]["bsk"], host[1]["ksk"]) == 1
    assert ring.add(dev["d_bsk"], dev["d_ksk"], keys_on_device=True) == 2      # adopted beside uploaded
    with pytest.raises(api.VpbsError, match="max_keys"):
        ring.add(host[3]["bsk"], host[3]["ksk"])                              # past max_keys
    first = ring.run(cts, key_of, testv)
    w = want([0, 1, 2])
    assert (first[0] == w[0]).all() and (first[1] == w[1]).all()
    ring.remove(1)
    assert ring.count() == 2
    with pytest.raises(api.VpbsError, match="slot"):
        ring.remove(1)
    assert ring.add(host[3]["bsk"], host[3]["ksk"]) == 1 and ring.count() == 3
    second = ring.run(cts, key_of, testv)
    w = want([0, 3, 2])
    assert (second[0] == w[0]).all() and (second[1] == w[1]).all()
    assert not (second[0][0] == first[0][0]).all()                            # row 0 is under slot 1: the new key shows
    # one tenant: all of key_of equal
    bs = api.Bootstrapper(ctx, host[3]["bsk"], host[3]["ksk"], K, ELL, LOGB, max_batch=5)
    o, l = bs.run(cts, testv)
    bs.close()
    o2, l2 = ring.run(cts, np.ones(5, np.uint32), testv)
    assert (o == o2).all() and (l == l2).all()
    ring.close()
    ctx.device_free(dev["d_bsk"])
    ctx.device_free(dev["d_ksk"])


def test_device_pointers_and_the_loop_closes(ctx, paper):
    """run_device with inputs and outputs in HBM; lwe_out fed back as the cts of a second run under the same key_of bootstraps to the same
    messages again, each under its own key"""
    import torch
    S = paper
    N, K, n = S["N"], S["K"], S["n"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    back = lambda d: d.cpu().numpy().view(np.uint64)
    d_cts, d_tv = t(S["cts"]), t(S["testv"])
    d_out = torch.zeros((6, K, N), dtype=torch.int64, device="cuda")
    d_lwe = torch.zeros((6, n + 1), dtype=torch.int64, device="cuda")
    d_lwe2 = torch.zeros_like(d_lwe)
    torch.cuda.synchronize()         # torch fills on its stream, the run is on the context's own
    ring = paper_ring(ctx, S)
    ring.run_device(d_cts.data_ptr(), 6, S["key_of"], d_tv.data_ptr(), False, d_out.data_ptr(), d_lwe.data_ptr(), None)
    assert (back(d_out) == S["want_out"]).all() and (back(d_lwe) == S["want_lwe"]).all()
    ring.run_device(d_lwe.data_ptr(), 6, S["key_of"], d_tv.data_ptr(), False, None, d_lwe2.data_ptr(), None)
    ring.close()
    second = back(d_lwe2)
    got = [B.round_message(api.lwe_decrypt(S["keys"][k]["s_lwe"], second[i]), S["delta"], S["p"]) for i, k in enumerate(S["key_of"])]
    assert got == S["msgs"]


def test_refusals_launch_nothing(ctx):
    """key_of with a slot at or above max_keys and with a removed slot: VPBS_ERR_INVALID, a message that names the index and the slot,
    outputs pre-filled with a marker untouched; a shape above the LDS budget is refused at create with the budget in the message"""
    N, K, ELL, LOGB, n = 64, 2, 4, 5, 20
    keys = ctx.keygen(N, K, ELL, LOGB, n, 0xF00D, *SIGMAS)
    testv, delta = api.testv(N, 2)
    cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * (i % 2) % P, nonce=i) for i in range(4)])
    ring = api.KeyRing(ctx, K, ELL, LOGB, N, n, max_keys=3, max_batch=4)
    assert [ring.add(keys["bsk"], keys["ksk"]) for _ in range(3)] == [0, 1, 2]
    ring.remove(1)
    L = api.lib()
    out_ct, lwe_out = np.full((4, K, N), MARK, np.uint64), np.full((4, n + 1), MARK, np.uint64)
    for key_of, index, slot, word in (([0, 2, 7, 0], 2, 7, "out of range"), ([0, 2, 2, 1], 3, 1, "empty")):
        ko = np.array(key_of, np.uint32)
        rc = L.vpbs_keyring_run(ring.h, cts.ctypes.data, 4, ko.ctypes.data, testv.ctypes.data, 0, out_ct.ctypes.data, lwe_out.ctypes.data, None, 0)
        msg = L.vpbs_last_error(ctx.h).decode()
        assert rc == -1, rc                                                   # VPBS_ERR_INVALID
        assert "key_of[%d] = %d" % (index, slot) in msg and word in msg and "ciphertext %d" % index in msg, msg
        assert (out_ct == MARK).all() and (lwe_out == MARK).all()
    with pytest.raises(api.VpbsError, match=r"key_of\[3\] = 1"):
        ring.run(cts, [0, 2, 2, 1], testv)
    with pytest.raises(api.VpbsError):
        ring.run(np.concatenate([cts, cts[:1]]), [0, 0, 0, 0, 0], testv)      # count above max_batch, as the Bootstrapper
    good = ring.run(cts, [0, 2, 2, 0], testv)                                 # the ring is usable after the refusals
    bs = api.Bootstrapper(ctx, keys["bsk"], keys["ksk"], K, ELL, LOGB, max_batch=4)
    want = bs.run(cts, testv)
    bs.close()
    assert (good[0] == want[0]).all() and (good[1] == want[1]).all()
    ring.close()
    with pytest.raises(api.VpbsError, match="budget"):
        api.KeyRing(ctx, 4, 8, 8, 2048, 100, max_keys=1, max_batch=1)         # N = 2048, K = 4, ELL = 8: 256 KiB


def test_pbs_speed_tool_with_three_key_sets():
    """tools/pbs_speed.py --keys 3 at a small shape in a process of its own: exit 0, one JSON line, every output decrypted under its own key"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pbs_speed.py"), "--keys", "3", "--shape", "256,2,4,5,100", "--batch", "7",
                        "--runs", "1"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["mode"] == "keyring" and line["keys"] == 3 and line["N"] == 256 and [row["batch"] for row in line["rows"]] == [7]
    assert all(row["all_decrypted"] and row["event_ms"][0] > 0 for row in line["rows"])
