"""GPU tests (-m gpu) of the start mode of the bootstrap kernels (vpbs_bootstrapper_run_from, vpbs_keyring_run_from; csrc/pbs_batch.hip,
csrc/pbs_keyring.hip).  The yardstick is the existing full run: for every row, run_from(start = k, acc_in = accs[k - 1]) must give out_ct,
lwe_out and accs[k - 1:] of Bootstrapper.run / KeyRing.run(.., accumulators=True) word for word, and must leave the slots below k - 1 of a
pre-filled accs_out buffer as they were.  Exact field arithmetic: every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import vpbs_amd
from vpbs_amd import api

pytestmark = pytest.mark.gpu
P = api.P
K, ELL, LOGB = 2, 4, 5
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)   # what the slots a resumed row must not write hold beforehand


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    yield c
    c.close()


def batch(ctx, N, n, count, seed, own_testv_rows=(), high_word=None):
    """seeded keys, `count` ciphertexts of alternating messages, per-row test vectors (all the shared one but those of own_testv_rows)"""
    keys = ctx.keygen(N, K, ELL, LOGB, n, seed, *SIGMAS)
    tv, delta = api.testv(N, 2)
    cts = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * (i % 2) % P, nonce=20 + i) for i in range(count)])
    if high_word is not None:
        cts[high_word, 2] = np.uint64(P + 7)   # a mask word at or above p: read raw by the mod switch, as in the full run
    testvs = np.stack([tv] * count)
    for i, row in enumerate(own_testv_rows):
        testvs[row] = np.array([(P - int(v)) * (i + 1) % P for v in tv], np.uint64)
    return keys, cts, testvs


def acc_in_of(accs, start):
    """acc_in [count][K][N]: accs[i][k - 1] for a row that enters at k, words that must never be read (all ones) for k = 0"""
    a = np.full((len(start),) + accs.shape[2:], np.uint64(2**64 - 1), np.uint64)
    for i, k in enumerate(start):
        if k:
            a[i] = accs[i, k - 1]
    return a


def check_rows(got, want, start):
    out_ct, lwe_out, accs = got
    w_out, w_lwe, w_accs = want
    assert (out_ct == w_out).all(), np.argwhere((out_ct != w_out).reshape(len(start), -1).any(axis=1)).ravel()
    assert (lwe_out == w_lwe).all(), np.argwhere((lwe_out != w_lwe).any(axis=1)).ravel()
    for i, k in enumerate(start):
        lo = max(k - 1, 0)
        assert (accs[i, lo:] == w_accs[i, lo:]).all(), (i, k)
        assert (accs[i, :lo] == FILL).all(), (i, k)   # slots below k - 1 are not written


# ---- N = 8, n = 6 (8 steps): k = 0, 1, n, n + 1 (the key switch alone) and n + 2 (no step) in one launch ----
N8, N_LWE8 = 8, 6
MIX8 = [1, 0, N_LWE8, N_LWE8 + 1, N_LWE8 + 2, 3]   # row 1 enters at step 0 with a test vector of its own: read by the start-mode kernel


@pytest.fixture(scope="module")
def n8(ctx):
    keys, cts, testvs = batch(ctx, N8, N_LWE8, len(MIX8), 77, own_testv_rows=(1, 4), high_word=2)
    bs = api.Bootstrapper(ctx, keys["bsk"], keys["ksk"], K, ELL, LOGB, max_batch=8)
    want = bs.run(cts, testvs, accumulators=True)
    yield dict(keys=keys, cts=cts, testvs=testvs, bs=bs, want=want)
    bs.close()


def test_a_launch_that_mixes_every_start_at_n8(n8):
    """rows at k = 1, 0, n, n + 1, n + 2 and a middle step; row 1 (k = 0, not the first workgroup) and row 4 (k = n + 2) have test vectors
    of their own, row 2 (k = n) a mask word at or above p; per-row test vectors, then the shared one on the rows that use it"""
    S = n8
    pre = np.full(S["want"][2].shape, FILL, np.uint64)
    got = S["bs"].run_from(S["cts"], MIX8, acc_in_of(S["want"][2], MIX8), S["testvs"], accumulators=pre)
    assert got[2] is pre
    check_rows(got, S["want"], MIX8)
    # k = n + 2 runs no step: out_ct is acc_in itself
    assert (got[0][4] == S["want"][2][4, N_LWE8 + 1]).all()
    # without accs_out, and with the shared test vector (rows 2, 3 and 5 use it, and so does row 0, here from step 0)
    rows, start = [2, 0, 3, 5], [MIX8[2], 0, MIX8[3], MIX8[5]]
    out_ct, lwe_out = S["bs"].run_from(S["cts"][rows], start, acc_in_of(S["want"][2][rows], start), S["testvs"][0])
    assert (out_ct == S["want"][0][rows]).all() and (lwe_out == S["want"][1][rows]).all()


def test_every_single_start_at_n8(n8):
    """one row, every k in 0 .. n + 2, on the ciphertext with the high mask word"""
    S = n8
    ct, tv = S["cts"][2:3], S["testvs"][2:3]
    want = tuple(w[2:3] for w in S["want"])
    for k in range(N_LWE8 + 3):
        pre = np.full(want[2].shape, FILL, np.uint64)
        check_rows(S["bs"].run_from(ct, [k], acc_in_of(want[2], [k]), tv, accumulators=pre), want, [k])


def test_null_start_and_all_zero_start_equal_run(n8):
    S = n8
    L = api.lib()
    count, n = len(MIX8), N_LWE8
    out_ct, lwe_out = np.zeros((count, K, N8), np.uint64), np.zeros((count, n + 1), np.uint64)
    accs = np.zeros((count, n + 2, K, N8), np.uint64)
    rc = L.vpbs_bootstrapper_run_from(S["bs"].h, S["cts"].ctypes.data, count, None, None, S["testvs"].ctypes.data, 1, out_ct.ctypes.data,
                                      lwe_out.ctypes.data, accs.ctypes.data, 0)
    assert rc == count
    assert (out_ct == S["want"][0]).all() and (lwe_out == S["want"][1]).all() and (accs == S["want"][2]).all()
    got = S["bs"].run_from(S["cts"], [0] * count, None, S["testvs"], accumulators=True)
    assert all((g == w).all() for g, w in zip(got, S["want"]))


def test_a_start_beyond_the_chain_is_refused_with_the_row_named(n8):
    S = n8
    count, n = 3, N_LWE8
    start = [1, n + 3, 0]
    acc_in = acc_in_of(S["want"][2][:count], [1, 1, 0])
    with pytest.raises(api.VpbsError, match=r"vpbs_bootstrapper_run_from: start\[1\] = %d .*ciphertext 1" % (n + 3)) as e:
        S["bs"].run_from(S["cts"][:count], start, acc_in, S["testvs"][:count])
    assert e.value.status == -1
    # the outputs are untouched
    L = api.lib()
    st = np.array(start, np.uint32)
    out_ct, lwe_out = np.full((count, K, N8), FILL, np.uint64), np.full((count, n + 1), FILL, np.uint64)
    accs = np.full((count, n + 2, K, N8), FILL, np.uint64)
    rc = L.vpbs_bootstrapper_run_from(S["bs"].h, S["cts"].ctypes.data, count, st.ctypes.data, acc_in.ctypes.data, S["testvs"].ctypes.data, 1,
                                      out_ct.ctypes.data, lwe_out.ctypes.data, accs.ctypes.data, 0)
    assert rc == -1
    assert (out_ct == FILL).all() and (lwe_out == FILL).all() and (accs == FILL).all()
    # a late start without acc_in is refused as well
    rc = L.vpbs_bootstrapper_run_from(S["bs"].h, S["cts"].ctypes.data, 1, np.array([2], np.uint32).ctypes.data, None, S["testvs"].ctypes.data, 1,
                                      out_ct.ctypes.data, None, None, 0)
    assert rc == -1 and (out_ct == FILL).all()


def test_the_key_ring_with_rows_of_two_slots_interleaved(ctx, n8):
    """the same mix through vpbs_keyring_run_from: rows alternate between two key sets; the yardsticks are KeyRing.run on the same batch and,
    for the rows of slot 0, the Bootstrapper of that key set"""
    S = n8
    other = ctx.keygen(N8, K, ELL, LOGB, N_LWE8, 78, *SIGMAS)
    ring = api.KeyRing(ctx, K, ELL, LOGB, N8, N_LWE8, max_keys=3, max_batch=8)
    assert ring.add(S["keys"]["bsk"], S["keys"]["ksk"]) == 0 and ring.add(other["bsk"], other["ksk"]) == 1
    key_of = [0, 1, 0, 1, 0, 1]
    want = ring.run(S["cts"], key_of, S["testvs"], accumulators=True)
    for i in (0, 2, 4):
        assert (want[2][i] == S["want"][2][i]).all()
    pre = np.full(want[2].shape, FILL, np.uint64)
    check_rows(ring.run_from(S["cts"], key_of, MIX8, acc_in_of(want[2], MIX8), S["testvs"], accumulators=pre), want, MIX8)
    # null start equals run; a start beyond the chain names the row and writes nothing
    got = ring.run_from(S["cts"], key_of, [0] * len(MIX8), None, S["testvs"], accumulators=True)
    assert all((g == w).all() for g, w in zip(got, want))
    with pytest.raises(api.VpbsError, match=r"vpbs_keyring_run_from: start\[3\] = %d .*ciphertext 3" % (N_LWE8 + 3)) as e:
        ring.run_from(S["cts"], key_of, [0, 0, 0, N_LWE8 + 3, 0, 0], acc_in_of(want[2], [0, 0, 0, 1, 0, 0]), S["testvs"])
    assert e.value.status == -1
    ring.close()


# ---- N = 1024 and N = 2048 (both pass structures of the transforms), n = 3: k in {0, 2, 4, 5}, once per thread count ----
@pytest.mark.parametrize("N", [1024, 2048])
def test_every_thread_count_at_both_pass_structures(ctx, N, monkeypatch):
    """n = 3 (5 steps): k = 2 (a blind-rotate step, a mask word at or above p), 0, 4 = n + 1 (the key switch alone), 5 = n + 2 (no step); 256, 512 and 1024 threads per
    ciphertext, pinned as tests/test_gpu_pbs_batch.py pins them (VPBS_PBS_BATCH_THREADS, read when the object is made), through the
    Bootstrapper and through a key ring (whose rows of 512 threads hold 8 key words ahead, of 1024 threads 4)"""
    n, start = 3, [2, 0, 4, 5]   # row 1: from step 0, with a test vector of its own
    keys, cts, testvs = batch(ctx, N, n, 4, 0x900 + N, own_testv_rows=(1,), high_word=0)
    bs = api.Bootstrapper(ctx, keys["bsk"], keys["ksk"], K, ELL, LOGB, max_batch=4)
    want = bs.run(cts, testvs, accumulators=True)
    bs.close()
    acc_in = acc_in_of(want[2], start)
    for threads in ("256", "512", "1024"):
        monkeypatch.setenv("VPBS_PBS_BATCH_THREADS", threads)
        bs = api.Bootstrapper(ctx, keys["bsk"], keys["ksk"], K, ELL, LOGB, max_batch=4)
        pre = np.full(want[2].shape, FILL, np.uint64)
        got = bs.run_from(cts, start, acc_in, testvs, accumulators=pre)
        bs.close()
        check_rows(got, want, start)
        ring = api.KeyRing(ctx, K, ELL, LOGB, N, n, max_keys=2, max_batch=4)
        assert ring.add(keys["bsk"], keys["ksk"]) == 0
        pre = np.full(want[2].shape, FILL, np.uint64)
        got = ring.run_from(cts, [0] * 4, start, acc_in, testvs, accumulators=pre)
        ring.close()
        check_rows(got, want, start)
