"""GPU tests (-m gpu) of the batched, key-resident bootstrap (vpbs_bootstrapper_*, vpbs_lwe_extract; csrc/pbs_batch.hip).  Two yardsticks:
the CPU restatement (tests/tfhe_oracle.py, tests/pbs_batch_oracle.py) on small shapes, and the per-step device path
(Context.pbs_accumulator_chain) at the paper's parameters.  Exact field arithmetic: every comparison is word for word."""
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


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    yield c
    c.close()


@pytest.fixture(scope="module")
def paper(ctx):
    """the paper's parameters and noise, seeded keys from vpbs_keygen, one Bootstrapper for batches of up to 64"""
    S = dict(PAPER)
    S["keys"] = ctx.keygen(S["N"], S["K"], S["ELL"], S["LOGB"], S["n"], 0x5EED, *SIGMAS)
    S["testv"], S["delta"] = api.testv(S["N"], S["p"])
    S["bs"] = api.Bootstrapper(ctx, S["keys"]["bsk"], S["keys"]["ksk"], S["K"], S["ELL"], S["LOGB"], max_batch=64)
    yield S
    S["bs"].close()


def rounded(m_bar, delta, p):
    return B.round_message(m_bar, delta, p)


def oracle_keys(log_n, K, ELL, LOGB, n, seed):
    ring = T.Ring(log_n)
    rng = np.random.default_rng(seed)
    s_to, s_lwe, s_glwe, bsk, ksk = T.pbs_setup(ring, rng, n, K, ELL, LOGB)
    return ring, rng, s_to, s_lwe, bsk, ksk, np.stack([T.flatten_ggsw(g) for g in bsk]), T.flatten_ggsw(ksk)


@pytest.mark.parametrize("log_n,K,ELL,LOGB,n", [(6, 2, 8, 8, 5), (3, 2, 4, 5, 6), (6, 3, 3, 7, 40), (5, 2, 4, 5, 9)])
def test_bit_exact_against_the_oracle(ctx, log_n, K, ELL, LOGB, n):
    """a batch of 7 with per-ciphertext test vectors (random words) and with one shared test vector: every accumulator of every chain is
    tfhe_oracle.pbs_chain's, out_ct its last, lwe_out the restated extraction.  (5, ..): an odd log N, whose transforms end in a lone stage."""
    ring, rng, s_to, s_lwe, bsk, ksk, bsk_flat, ksk_flat = oracle_keys(log_n, K, ELL, LOGB, n, 77 + log_n + K)
    N, count = ring.n, 7
    delta = T.get_delta(4)
    cts = np.array([T.lwe_encrypt(rng, s_lwe, delta * (i % 2) % P) for i in range(count)], np.uint64)
    cts[3, 0], cts[3, 1], cts[3, 2] = 0, P - 1, 1 << 63
    shared = np.array(T.get_testv(ring, 2, delta), np.uint64)
    per_ct = rng.integers(0, P, size=(count, N), dtype=np.uint64)
    bs = api.Bootstrapper(ctx, bsk_flat, ksk_flat, K, ELL, LOGB, max_batch=count)
    for testv in (per_ct, shared):
        out_ct, lwe_out, accs = bs.run(cts, testv, accumulators=True)
        assert accs.shape == (count, n + 2, K, N)
        for i in range(count):
            tv = testv[i] if testv.ndim == 2 else testv
            acc0 = [[0] * N for _ in range(K - 1)] + [[int(v) for v in tv]]
            want = T.pbs_chain(ring, acc0, [int(v) for v in cts[i]], bsk, ksk, K, ELL, LOGB)
            for s in range(n + 2):
                assert (accs[i, s] == np.array(want[s], np.uint64)).all(), (i, s)
            assert (out_ct[i] == accs[i, n + 1]).all(), i
            assert lwe_out[i].tolist() == B.extract(want[-1], n), i
        # the outputs alone: the same words without the accumulators
        out2, lwe2 = bs.run(cts, testv)
        assert (out2 == out_ct).all() and (lwe2 == lwe_out).all()
    bs.close()


def test_bit_exact_against_the_per_step_path_at_the_papers_parameters(ctx, paper):
    """vpbs_keygen's noisy keys, a batch of 5 (mixed messages, one ciphertext with the edge words 0, p - 1, 2^63 in its mask): every
    accumulator equals Context.pbs_accumulator_chain's on the same ciphertext"""
    S, keys = paper, paper["keys"]
    N, K, n = S["N"], S["K"], S["n"]
    cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], S["delta"] * m % P, nonce=10 + i) for i, m in enumerate([0, 1, 1, 0, 1])])
    cts[2, 0], cts[2, 1], cts[2, 2], cts[2, 727] = 0, P - 1, 1 << 63, P - 1
    out_ct, lwe_out, accs = S["bs"].run(cts, S["testv"], accumulators=True)
    acc_init = np.concatenate([np.zeros((K - 1, N), np.uint64), S["testv"].reshape(1, N)])
    for i in range(5):
        want = ctx.pbs_accumulator_chain(acc_init, cts[i], keys["bsk"], keys["ksk"], K, S["ELL"], S["LOGB"])
        assert (accs[i] == want).all(), (i, int(np.argmax((accs[i] != want).reshape(n + 2, -1).any(axis=1))))
        assert (out_ct[i] == want[-1]).all()
        assert lwe_out[i].tolist() == B.extract(B.glwe_list(want[-1]), n)


def test_bit_exact_against_the_per_step_path_at_n2048(ctx):
    """one ciphertext at N = 2048 (accumulator + outputs + limbs = 128 KiB of LDS), the paper's K, ELL, LOGB, n and noise"""
    N, K, ELL, LOGB, n = 2048, 2, 4, 5, 728
    keys = ctx.keygen(N, K, ELL, LOGB, n, 0x2048, *SIGMAS)
    testv, delta = api.testv(N, 2)
    ct = api.lwe_encrypt(keys["params"], keys["s_lwe"], delta % P, nonce=3)
    bs = api.Bootstrapper(ctx, keys["bsk"], keys["ksk"], K, ELL, LOGB, max_batch=1)
    out_ct, lwe_out, accs = bs.run(ct.reshape(1, -1), testv, accumulators=True)
    bs.close()
    acc_init = np.concatenate([np.zeros((K - 1, N), np.uint64), testv.reshape(1, N)])
    want = ctx.pbs_accumulator_chain(acc_init, ct, keys["bsk"], keys["ksk"], K, ELL, LOGB)
    assert (accs[0] == want).all() and (out_ct[0] == want[-1]).all()
    assert lwe_out[0].tolist() == B.extract(B.glwe_list(want[-1]), n)
    assert rounded(api.lwe_decrypt(keys["s_lwe"], lwe_out[0]), delta, 2) == 1


def test_words_at_or_above_p_follow_the_per_step_path(ctx):
    """the header's statement on non-canonical words: they are not reduced first and go through the operations of
    vpbs_pbs_accumulator_chain, so the two paths agree on them word for word (test vector, mask and body words in [p, 2^64))"""
    N, K, ELL, LOGB, n = 64, 2, 4, 5, 20
    keys = ctx.keygen(N, K, ELL, LOGB, n, 0xABCDE, *SIGMAS)
    testv, delta = api.testv(N, 2)
    testv = testv.copy()
    for i, w in ((0, P), (1, P + 5), (17, (1 << 64) - 1), (63, P + (1 << 31))):
        testv[i] = np.uint64(w)
    cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * m % P, nonce=i) for i, m in enumerate([1, 0, 1])])
    for i, j, w in ((0, 0, P), (0, 5, (1 << 64) - 1), (1, n, (1 << 64) - 1), (2, n, P + 1), (2, 3, P + (1 << 30))):   # j = n: the body
        cts[i, j] = np.uint64(w)
    bs = api.Bootstrapper(ctx, keys["bsk"], keys["ksk"], K, ELL, LOGB, max_batch=3)
    out_ct, lwe_out, accs = bs.run(cts, testv, accumulators=True)
    bs.close()
    acc_init = np.concatenate([np.zeros((K - 1, N), np.uint64), testv.reshape(1, N)])
    for i in range(3):
        want = ctx.pbs_accumulator_chain(acc_init, cts[i], keys["bsk"], keys["ksk"], K, ELL, LOGB)
        assert (accs[i] == want).all() and (out_ct[i] == want[-1]).all(), i
        assert (lwe_out[i] == ctx.lwe_extract(want[-1], n)).all(), i


def test_thread_count_never_changes_a_word(ctx, paper, monkeypatch):
    """256, 512 and 1024 threads per ciphertext (VPBS_PBS_BATCH_THREADS, read when the object is made) and the library's own choice give
    the same accumulators: at the paper's parameters and on a small shape with K = 3; any other value is refused"""
    S, keys = paper, paper["keys"]
    cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], S["delta"] * m % P, nonce=50 + m) for m in (0, 1)])
    want = S["bs"].run(cts, S["testv"], accumulators=True)
    small = ctx.keygen(64, 3, 3, 7, 40, 0x777, *SIGMAS)
    tv, delta = api.testv(64, 2)
    small_cts = np.stack([api.lwe_encrypt(small["params"], small["s_lwe"], delta * (i % 2) % P, nonce=i) for i in range(3)])
    fresh = api.Bootstrapper(ctx, small["bsk"], small["ksk"], 3, 3, 7, max_batch=3)
    small_want = fresh.run(small_cts, tv, accumulators=True)
    fresh.close()
    for threads in ("256", "512", "1024"):
        monkeypatch.setenv("VPBS_PBS_BATCH_THREADS", threads)
        bs = api.Bootstrapper(ctx, keys["bsk"], keys["ksk"], S["K"], S["ELL"], S["LOGB"], max_batch=2)
        got = bs.run(cts, S["testv"], accumulators=True)
        bs.close()
        assert all((g == w).all() for g, w in zip(got, want)), threads
        bs = api.Bootstrapper(ctx, small["bsk"], small["ksk"], 3, 3, 7, max_batch=3)
        got = bs.run(small_cts, tv, accumulators=True)
        bs.close()
        assert all((g == w).all() for g, w in zip(got, small_want)), threads
    monkeypatch.setenv("VPBS_PBS_BATCH_THREADS", "384")
    with pytest.raises(api.VpbsError, match="VPBS_PBS_BATCH_THREADS"):
        api.Bootstrapper(ctx, small["bsk"], small["ksk"], 3, 3, 7, max_batch=3)


def test_more_ciphertexts_than_compute_units(ctx, paper):
    """300 ciphertexts (the library then runs two 512-thread workgroups per CU): the outputs are those of the same ciphertexts in batches
    of 64, and decrypt to their messages"""
    S, keys = paper, paper["keys"]
    msgs = [(i // 5) % 2 for i in range(300)]
    cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], S["delta"] * m % P, nonce=1000 + i) for i, m in enumerate(msgs)])
    bs = api.Bootstrapper(ctx, keys["bsk"], keys["ksk"], S["K"], S["ELL"], S["LOGB"], max_batch=300)
    out_ct, lwe_out = bs.run(cts, S["testv"])
    bs.close()
    assert [rounded(m, S["delta"], S["p"]) for m in api.lwe_decrypt(keys["s_lwe"], lwe_out)] == msgs
    for lo in range(0, 300, 64):
        o, l = S["bs"].run(cts[lo:lo + 64], S["testv"])
        assert (o == out_ct[lo:lo + 64]).all() and (l == lwe_out[lo:lo + 64]).all(), lo


def test_the_loop_closes_at_the_papers_parameters(ctx, paper):
    """batch of 64, messages 0 / 1, the paper's noise: the extracted outputs decrypt under the LWE key to the messages (rounded as
    main.rs:59-64 rounds); fed back in as the ciphertexts of a second run, they bootstrap to the same messages again"""
    S, keys = paper, paper["keys"]
    msgs = [(i * 7 + i // 3) % 2 for i in range(64)]
    cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], S["delta"] * m % P, nonce=100 + i) for i, m in enumerate(msgs)])
    out_ct, lwe_out = S["bs"].run(cts, S["testv"])
    first = [rounded(m, S["delta"], S["p"]) for m in api.lwe_decrypt(keys["s_lwe"], lwe_out)]
    assert first == msgs
    assert [rounded(ctx.glwe_decrypt(keys["s_to"], out_ct[i])[0], S["delta"], S["p"]) for i in range(64)] == msgs
    out2, lwe2 = S["bs"].run(lwe_out, S["testv"])
    assert [rounded(ctx.glwe_decrypt(keys["s_to"], out2[i])[0], S["delta"], S["p"]) for i in range(64)] == msgs
    assert [rounded(m, S["delta"], S["p"]) for m in api.lwe_decrypt(keys["s_lwe"], lwe2)] == msgs


def test_the_loop_closes_without_noise_and_sums_bootstrap(ctx):
    """sigma = 0 on a small shape: two levels of bootstraps reproduce delta * m exactly, and the sum of two extracted outputs of
    messages 0 and 1, bootstrapped once more, gives 1"""
    log_n, K, ELL, LOGB, n = 6, 2, 8, 8, 5
    ring, rng, s_to, s_lwe, bsk, ksk, bsk_flat, ksk_flat = oracle_keys(log_n, K, ELL, LOGB, n, 4242)
    delta = T.get_delta(4)
    testv = np.array(T.get_testv(ring, 2, delta), np.uint64)
    msgs = [0, 1, 1, 0, 1, 0]
    cts = np.array([T.lwe_encrypt(rng, s_lwe, delta * m % P) for m in msgs], np.uint64)
    bs = api.Bootstrapper(ctx, bsk_flat, ksk_flat, K, ELL, LOGB, max_batch=8)
    out1, lwe1 = bs.run(cts, testv)
    assert [B.lwe_decrypt(s_lwe, c) for c in lwe1] == [delta * m % P for m in msgs]
    out2, lwe2 = bs.run(lwe1, testv)
    assert [T.glwe_decrypt(ring, s_to[:K - 1], B.glwe_list(o), K)[0] for o in out2] == [delta * m % P for m in msgs]
    assert [B.lwe_decrypt(s_lwe, c) for c in lwe2] == [delta * m % P for m in msgs]
    sums = np.array([[(int(a) + int(b)) % P for a, b in zip(lwe2[i], lwe2[j])] for i, j in ((0, 1), (3, 2), (0, 3))], np.uint64)
    out3, lwe3 = bs.run(sums, testv)
    assert [B.lwe_decrypt(s_lwe, c) for c in lwe3] == [delta, delta, 0]
    assert [rounded(api.lwe_decrypt(np.array(s_lwe, np.uint64), c), delta, 2) for c in lwe3] == [1, 1, 0]
    bs.close()


def test_device_pointers_adopted_keys_and_reuse(ctx):
    """on_device = 1 with the keys adopted from vpbs_keygen(.., keys_on_device = 1); two runs on one object with counts 1 and max_batch
    give what fresh objects with uploaded keys give; count > max_batch and a shape beyond the LDS budget are refused with a message and
    leave the object and the context usable"""
    import torch
    N, K, ELL, LOGB, n, max_batch = 256, 2, 4, 5, 100, 6
    host = ctx.keygen(N, K, ELL, LOGB, n, 0xD0D0, *SIGMAS)
    dev = ctx.keygen_device(N, K, ELL, LOGB, n, 0xD0D0, *SIGMAS)
    assert (dev["s_lwe"] == host["s_lwe"]).all()
    testv, delta = api.testv(N, 2)
    cts = np.stack([api.lwe_encrypt(host["params"], host["s_lwe"], delta * (i % 2) % P, nonce=i) for i in range(max_batch + 1)])
    per_ct = np.random.default_rng(5).integers(0, P, size=(max_batch, N), dtype=np.uint64)
    bs = api.Bootstrapper(ctx, dev["d_bsk"], dev["d_ksk"], K, ELL, LOGB, max_batch=max_batch, N=N, n_lwe=n, keys_on_device=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    back = lambda d: d.cpu().numpy().view(np.uint64)
    d_cts, d_tv, d_tvs = t(cts), t(testv), t(per_ct)
    for count, d_testv, tv, per in ((1, d_tv, testv, False), (max_batch, d_tvs, per_ct, True), (1, d_tv, testv, False)):
        d_out = torch.zeros((count, K, N), dtype=torch.int64, device="cuda")
        d_lwe = torch.zeros((count, n + 1), dtype=torch.int64, device="cuda")
        d_accs = torch.zeros((count, n + 2, K, N), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()         # torch fills on its stream, the run is on the context's own
        bs.run_device(d_cts.data_ptr(), count, d_testv.data_ptr(), per, d_out.data_ptr(), d_lwe.data_ptr(), d_accs.data_ptr())
        fresh = api.Bootstrapper(ctx, host["bsk"], host["ksk"], K, ELL, LOGB, max_batch=count)
        out_ct, lwe_out, accs = fresh.run(cts[:count], tv, accumulators=True)
        fresh.close()
        assert (back(d_out) == out_ct).all() and (back(d_lwe) == lwe_out).all() and (back(d_accs) == accs).all(), count
        # only lwe_out asked for
        d_lwe2 = torch.zeros_like(d_lwe)
        torch.cuda.synchronize()
        bs.run_device(d_cts.data_ptr(), count, d_testv.data_ptr(), per, None, d_lwe2.data_ptr(), None)
        assert (back(d_lwe2) == lwe_out).all()
    # refusals
    L = api.lib()
    assert L.vpbs_bootstrapper_run(bs.h, d_cts.data_ptr(), max_batch + 1, d_tv.data_ptr(), 0, d_out.data_ptr(), None, None, 1) == -1
    assert L.vpbs_bootstrapper_run(bs.h, None, 1, d_tv.data_ptr(), 0, d_out.data_ptr(), None, None, 1) == -1
    assert L.vpbs_bootstrapper_run(bs.h, d_cts.data_ptr(), 1, None, 0, d_out.data_ptr(), None, None, 1) == -1
    assert L.vpbs_bootstrapper_run(bs.h, d_cts.data_ptr(), 1, d_tv.data_ptr(), 0, None, None, None, 1) == -1
    with pytest.raises(api.VpbsError):
        bs.run(cts, testv)                      # max_batch + 1 ciphertexts
    g = 4 * 8 * 4 * 2048
    with pytest.raises(api.VpbsError, match="budget"):
        api.Bootstrapper(ctx, np.zeros((1, g), np.uint64), np.zeros(g, np.uint64), 4, 8, 8, max_batch=1)      # N = 2048, K = 4, ELL = 8: 256 KiB
    with pytest.raises(api.VpbsError, match="n_lwe"):
        api.Bootstrapper(ctx, np.zeros((N + 1, K * ELL * K * N), np.uint64), host["ksk"], K, ELL, LOGB, max_batch=1)   # n_lwe > (K - 1) N
    host_fresh = api.Bootstrapper(ctx, host["bsk"], host["ksk"], K, ELL, LOGB, max_batch=2)
    want = host_fresh.run(cts[:2], testv)
    host_fresh.close()
    got = bs.run(cts[:2], testv)                # host pointers on the object with adopted keys, after the refusals
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    bs.close()
    ctx.device_free(dev["d_bsk"])
    ctx.device_free(dev["d_ksk"])


def test_lwe_extract_on_host_and_device_pointers(ctx):
    """vpbs_lwe_extract against the restatement (n_lwe not a multiple of N, n_lwe > N with K = 3, edge words) and against the extraction
    the batch kernel does from LDS"""
    import torch
    rng = np.random.default_rng(9)
    for N, K, n_lwe, count in ((64, 3, 100, 9), (64, 3, 128, 2), (8, 2, 6, 5), (1024, 2, 728, 3), (16, 4, 33, 4)):
        g = rng.integers(0, P, size=(count, K, N), dtype=np.uint64)
        g[0, 0, 0], g[0, 0, 1], g[0, 0, N - 1], g[0, K - 1, 0] = 0, P - 1, 0, P - 1
        want = np.array([B.extract(B.glwe_list(x), n_lwe) for x in g], np.uint64)
        assert (ctx.lwe_extract(g, n_lwe) == want).all()
        assert (ctx.lwe_extract(g[1], n_lwe) == want[1]).all()
        d_g = torch.from_numpy(g.view(np.int64)).cuda()
        d_out = torch.zeros((count, n_lwe + 1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.lwe_extract(d_g.data_ptr(), n_lwe, count=count, N=N, K=K, out_dev_ptr=d_out.data_ptr())
        assert (d_out.cpu().numpy().view(np.uint64) == want).all()
    with pytest.raises(api.VpbsError, match="n_lwe"):
        ctx.lwe_extract(np.zeros((1, 2, 8), np.uint64), 9)
    # the in-kernel extraction
    N, K, ELL, LOGB, n = 64, 3, 3, 7, 100
    keys = ctx.keygen(N, K, ELL, LOGB, n, 31337, *SIGMAS)
    testv, delta = api.testv(N, 2)
    cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * (i % 2) % P, nonce=i) for i in range(4)])
    bs = api.Bootstrapper(ctx, keys["bsk"], keys["ksk"], K, ELL, LOGB, max_batch=4)
    out_ct, lwe_out = bs.run(cts, testv)
    bs.close()
    assert (ctx.lwe_extract(out_ct, n) == lwe_out).all()


def test_pbs_speed_tool_checks_every_output():
    """tools/pbs_speed.py in a process of its own, two small batches at the paper's parameters: one JSON line, every output decrypted"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pbs_speed.py"), "--batch", "1,3", "--runs", "1"], capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["mode"] == "batch" and [row["batch"] for row in line["rows"]] == [1, 3]
    assert all(row["all_decrypted"] and row["event_ms"][0] > 0 for row in line["rows"])
