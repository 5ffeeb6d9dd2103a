"""CPU side of the rotation margins (csrc/rotation.h, vpbs_lwe_rotation_batch) through the null-context host path, against
the Python restatement (tests/rotation_oracle.py): mu, idx and dev on rows built from the edge words of both roundings, the statistics,
every refusal, NoiseStats.tail_log2 against math.erfc, Program.margins against per-gate calls, and the prediction contract itself against
the restated bootstrap of tests/tfhe_oracle.py at log_n 5.  Exact integers throughout."""
import math

import numpy as np
import pytest

import rotation_oracle as R
import tfhe_oracle as T
from vpbs_amd import api

P = api.P


def test_library_exports_the_entry_point_and_api_binds_it():
    L = api.lib()
    name = "vpbs_lwe_rotation_batch"
    assert name in api.SIGNATURES
    fn = getattr(L, name)
    assert fn.argtypes == api.SIGNATURES[name][1] and fn.restype == api.SIGNATURES[name][0]
    assert callable(api.lwe_rotation_batch) and hasattr(api.Context, "lwe_rotation_batch") and callable(api.lut_expect)
    assert hasattr(api.NoiseStats, "tail_log2") and hasattr(api.Program, "margins")


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 728])
@pytest.mark.parametrize("log_n", [1, 3, 7, 10, 11])
def test_host_form_equals_the_restatement(log_n, n):
    N = 1 << log_n
    for theta in range(min(3, log_n) + 1):
        cts = R.edge_rows(log_n, n, theta, 100 * log_n + n)
        count = len(cts)
        for s in R.keys(n, n + theta):
            mus = [R.rotation(s, ct, log_n, theta) for ct in cts]
            for p in sorted({1, 2, N}):
                two_p = 2 * p
                expected = [[0, p - 1, p, two_p - 1, two_p, two_p + 3, (1 << 64) - 1][i % 7] for i in range(count)]
                for exp in (None, expected):
                    st, want = api.NoiseStats(), R.Stats()
                    got = api.lwe_rotation_batch(s, cts, N, p, log_slots=theta, expected=exp, stats=st, want=("rot", "idx", "dev"))
                    ref = [R.margin(mu, log_n, p, None if exp is None else exp[i]) for i, mu in enumerate(mus)]
                    for (_, dev, failed) in ref:
                        want.add(dev, failed)
                    where = (log_n, n, theta, p, exp is not None)
                    assert got["rot"].tolist() == mus, where
                    assert got["idx"].tolist() == [r[0] for r in ref], where
                    assert got["dev"].dtype == np.int64 and got["dev"].tolist() == [r[1] for r in ref], where
                    assert st.as_dict() == want.as_dict(), where
                    if exp is None:
                        assert st.failures == 0 and st.max_abs <= (N // p + 1) // 2


def test_the_corners_by_hand():
    """log_n 3 (2N = 16, a word's top 4 bits and the rounding bit), n 1"""
    one = np.ones(1, np.uint64)
    row = lambda a, b: np.array([[a, b]], np.uint64)
    rot = lambda cts, theta=0, s=one: int(api.lwe_rotation_batch(s, cts, 8, 2, log_slots=theta, want=("rot",))["rot"][0])
    assert rot(row(0, 0)) == 0
    assert rot(row(3 << 60, 0)) == 16 - 3 and rot(row(0, 3 << 60)) == 3                # mu = phase position: body - mask
    assert rot(row(0, 3 << 60), s=np.zeros(1, np.uint64)) == 3 and rot(row(5 << 60, 3 << 60), s=np.zeros(1, np.uint64)) == 3
    assert rot(row((15 << 60) | (1 << 59), 0)) == 0                                    # ms carries to 2N = 16: a full turn
    assert rot(row(P, (1 << 64) - 1)) == 0                                             # reduced on read: 0 and 2^32 - 2
    assert rot(row((7 << 60) | (1 << 59), 0)) == 8 and rot(row((7 << 60) | ((1 << 59) - 1), 0)) == 9
    # theta 2: words rounded to multiples of 4 positions; 14.0 -> 16 wraps to 0, 13.99 -> 12
    assert rot(row(14 << 60, 0), theta=2) == 0 and rot(row((14 << 60) - 1, 0), theta=2) == 4
    assert rot(row(2 << 60, 0), theta=2) == 12 and rot(row((2 << 60) - 1, 0), theta=2) == 0
    # idx, dev: p = 2, block 4, h 2: mu 0 1 | 2 .. 5 | 6 .. 9 | 10 .. 13 | 14 15 -> idx 0 1 2 3 0
    cts = np.array([[0, mu << 60] for mu in range(16)], np.uint64)
    got = api.lwe_rotation_batch(one, cts, 8, 2, want=("idx", "dev"))
    assert got["idx"].tolist() == [0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 0, 0]
    assert got["dev"].tolist() == [0, 1, -2, -1, 0, 1, -2, -1, 0, 1, -2, -1, 0, 1, -2, -1]
    got = api.lwe_rotation_batch(one, cts, 8, 2, expected=[1] * 16, want=("dev",))
    assert got["dev"].tolist() == [-4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, -8, -7, -6, -5]      # centred into [-N, N)
    # p = N: every position is a table entry; p = 1: one block, the negated half is idx 1
    assert api.lwe_rotation_batch(one, cts, 8, 8)["idx"].tolist() == list(range(16))
    assert api.lwe_rotation_batch(one, cts, 8, 1)["idx"].tolist() == [0] * 4 + [1] * 8 + [0] * 4


def test_lut_expect_is_the_rotated_coefficient():
    tv = np.array([5, 6, 7, P + 2], np.uint64)
    assert [api.lut_expect(tv, mu) for mu in range(9)] == [5, 6, 7, 2, P - 5, P - 6, P - 7, P - 2, 5]
    assert api.lut_expect(tv, 3, j=2) == P - 6 and api.lut_expect(tv, 7, j=1) == 5
    assert api.lut_expect(tv, np.array([0, 3, 4, 7], np.uint64), 1).tolist() == [6, P - 5, P - 6, 5]
    assert all(api.lut_expect(tv, mu, j) == R.expect(tv.tolist(), mu, j) for mu in range(8) for j in range(4))


def test_statistics_accumulate_and_carry_negative_deviations():
    log_n, n, p = 7, 65, 2
    N = 1 << log_n
    rng = np.random.default_rng(9)
    s = rng.integers(0, 2, size=n, dtype=np.uint64)
    cts = rng.integers(0, 1 << 64, size=(40, n + 1), dtype=np.uint64)
    expected = rng.integers(0, 2 * p, size=40).astype(np.uint64)
    whole, halves, want = api.NoiseStats(), api.NoiseStats(), R.Stats()
    got = api.lwe_rotation_batch(s, cts, N, p, expected=expected, stats=whole, want=("dev",))
    api.lwe_rotation_batch(s, cts[:20], N, p, expected=expected[:20], stats=halves, want=())
    api.lwe_rotation_batch(s, cts[20:], N, p, expected=expected[20:], stats=halves, want=())
    _, idxs, devs = R.rotation_batch(s, cts, log_n, p, 0, expected.tolist(), want)
    assert got["dev"].tolist() == devs and min(devs) < 0 < max(devs)
    assert whole.as_dict() == halves.as_dict() == want.as_dict()
    assert whole.count == 40 and whole.failures == sum(int(i != e) for i, e in zip(idxs, expected.tolist())) > 0
    assert whole.sum_signed == sum(devs) and whole.sum_abs == sum(abs(d) for d in devs) and whole.max_abs == max(abs(d) for d in devs)
    assert whole.hist == [sum(1 for d in devs if abs(d).bit_length() == k) for k in range(65)]
    # only negative deviations: the signed sum is negative
    neg = api.NoiseStats()
    cts = np.array([[0, (mu << 56)] for mu in (2, 3, 10, 11)], np.uint64)                     # log_n 7: positions are words >> 56
    assert api.lwe_rotation_batch(np.ones(1, np.uint64), cts, N, 16, stats=neg, want=("dev",))["dev"].tolist() == [2, 3, 2, 3]
    cts = np.array([[0, (mu << 56)] for mu in (5, 6, 7, 255)], np.uint64)
    neg = api.NoiseStats()
    assert api.lwe_rotation_batch(np.ones(1, np.uint64), cts, N, 16, stats=neg, want=("dev",))["dev"].tolist() == [-3, -2, -1, -1]
    assert neg.sum_signed == -7 and neg.sum_abs == 7 and neg.sum_sq == 15 and neg.max_abs == 3 and neg.hist[1:3] == [2, 2]


def test_refusals():
    L = api.lib()
    buf = np.zeros(64, np.uint64)
    b = buf.ctypes.data

    def call(s=b, c=b, count=2, n=3, log_n=3, theta=0, p=2, where=0, key_dev=0):
        return L.vpbs_lwe_rotation_batch(None, s, key_dev, c, count, n, log_n, theta, p, None, b, b, b, None, where)
    assert call() == 0
    assert call(s=None) == -1 and call(c=None) == -1
    assert call(n=0) == -1 and call(n=1 << 24) == -1
    assert call(log_n=0) == -1 and call(log_n=17) == -1 and call(log_n=16, n=1) == 0
    assert call(theta=4) == -1 and call(theta=3) == 0
    assert call(p=0) == -1 and call(p=3) == -1 and call(p=16) == -1 and call(p=8) == 0 and call(p=1) == 0
    assert call(count=(1 << 31) + 1) == -1
    assert call(where=1) == -1 and call(where=2) == -1 and call(where=3) == -1 and call(key_dev=1) == -1
    assert call(c=None, count=0) == 0
    key = np.array([0, 1, P, P + 1, 2, 1, P + 2], np.uint64)       # reduced: 0 1 0 1 2 1 2
    assert L.vpbs_lwe_rotation_batch(None, key.ctypes.data, 0, b, 2, 7, 3, 0, 2, None, b, b, b, None, 0) == -1
    assert L.vpbs_lwe_rotation_batch(None, key.ctypes.data, 0, b, 2, 4, 3, 0, 2, None, b, b, b, None, 0) == 0
    with pytest.raises(api.VpbsError, match="key word 4 is neither 0 nor 1"):
        api.lwe_rotation_batch(key, np.zeros((2, 8), np.uint64), 8, 2)
    with pytest.raises(api.VpbsError, match="key word 5 is neither 0 nor 1"):
        api.lwe_rotation_batch(np.concatenate([key[:4], key[5:]]), np.zeros((0, 7), np.uint64), 8, 2)   # refused before the empty batch returns
    with pytest.raises(ValueError):
        api.lwe_rotation_batch(np.zeros(3, np.uint64), np.zeros((2, 5), np.uint64), 8, 2)
    with pytest.raises(ValueError):
        api.lwe_rotation_batch(np.zeros(3, np.uint64), np.zeros((2, 4), np.uint64), 8, 2, want=("msg",))
    with pytest.raises(ValueError):
        api.lwe_rotation_batch(np.zeros(3, np.uint64), np.zeros((2, 4), np.uint64), 12, 2)


def test_tail_log2_against_erfc_and_beyond_it():
    st = api.NoiseStats()
    rng = np.random.default_rng(4)
    n = 40
    cts = rng.integers(0, 1 << 64, size=(500, n + 1), dtype=np.uint64)
    api.lwe_rotation_batch(rng.integers(0, 2, size=n, dtype=np.uint64), cts, 1 << 10, 1 << 10, expected=[7] * 500, stats=st, want=())
    m, s = st.mean(), st.std()
    assert s > 100 and m != 0
    prev = 1.0
    for k in range(0, 300):
        bound = k * s / 4                                            # up to 75 sigma; erfc underflows near 27 / sqrt(2) ... 38 sigma
        got = st.tail_log2(bound)
        assert math.isfinite(got) and got < prev, k
        prev = got
        tail = 0.5 * (math.erfc((bound - m) / (s * math.sqrt(2))) + math.erfc((bound + m) / (s * math.sqrt(2))))
        if tail > 1e-300:
            assert got == pytest.approx(math.log2(tail), abs=1e-9), k
    assert st.tail_log2(0) == pytest.approx(0.0, abs=1e-12)
    assert st.tail_log2(75 * s) < -4000                              # about -(75^2 / 2) log2 e
    # the seam of the two forms of ln erfc
    assert api.NoiseStats._ln_erfc(25.0 - 1e-9) == pytest.approx(api.NoiseStats._ln_erfc(25.0), abs=1e-6)
    doc = api.NoiseStats.tail_log2.__doc__
    assert "MODEL" in doc and "LIGHTER tails than a Gaussian" in doc and "IS Gaussian" in doc
    zero = api.NoiseStats()
    api.lwe_rotation_batch(np.ones(1, np.uint64), np.zeros((3, 2), np.uint64), 8, 2, stats=zero, want=())
    assert zero.tail_log2(1) == -math.inf and zero.tail_log2(-1) == 0.0


def test_program_margins_on_a_host_only_program_are_the_per_gate_calls():
    """three levels, two test vectors with different p, gates of one level and p that are not neighbours"""
    log_n, n = 5, 9
    N = 1 << log_n
    gates = [([(0, 1)], 0, 0), ([(1, 1)], 0, 1), ([(0, 1), (1, 1)], 0, 0), ([(2, 1)], 0, 1), ([(3, 1), (5, 1)], 0, 0, 1, 2), ([(4, 1)], 3, 1)]
    prog = api.Program(None, 2, gates, 2)
    level, n_levels = prog.levels()
    assert level.tolist() == [1, 1, 1, 2, 3, 2] and n_levels == 3
    rng = np.random.default_rng(21)
    s = rng.integers(0, 2, size=n, dtype=np.uint64)
    gate_cts = rng.integers(0, P, size=(6, n + 1), dtype=np.uint64)
    p_of_lut = [2, 8]
    expected = np.array([1, 9, 3, 15, 0, 2], np.uint64)
    for exp in (None, expected):
        mu, idx, dev, stats = prog.margins(None, s, gate_cts, p_of_lut, expected=exp, N=N)
        assert len(stats) == 3 and [st.count for st in stats] == [3, 2, 1]
        want = [R.Stats() for _ in range(3)]
        for g in range(6):
            p = p_of_lut[gates[g][2]]
            one = api.lwe_rotation_batch(s, gate_cts[g:g + 1], N, p, expected=None if exp is None else exp[g:g + 1], want=("rot", "idx", "dev"))
            assert (int(mu[g]), int(idx[g]), int(dev[g])) == (int(one["rot"][0]), int(one["idx"][0]), int(one["dev"][0])), g
            i, d, failed = R.margin(R.rotation(s, gate_cts[g], log_n), log_n, p, None if exp is None else exp[g])
            assert (int(idx[g]), int(dev[g])) == (i, d)
            want[level[g] - 1].add(d, failed)
        assert [st.as_dict() for st in stats] == [w.as_dict() for w in want]
    with pytest.raises(ValueError):
        prog.margins(None, s, gate_cts, [2], N=N)
    prog.close()


def test_prediction_contract_against_the_restated_bootstrap():
    """log_n 5, K 2, ELL 8, LOGB 8 (exact decomposition), n 5, p 2, noise-free keys: for every third of the 125 rows the restated chain's
    output GLWE decrypts, at coefficients 0 .. 3, to lut_expect(testv, mu, j) -- and the rounded PHASE names another table entry on some
    rows, which is why the call exists"""
    log_n, K, ELL, LOGB, n, p = 5, 2, 8, 8, 5, 2
    N = 1 << log_n
    ring = T.Ring(log_n)
    rng = np.random.default_rng(5150)
    s_to, s_lwe, s_glwe, bsk, ksk = T.pbs_setup(ring, rng, n, K, ELL, LOGB)
    delta = T.get_delta(2 * p)
    testv = api.lut_testv(N, p, [1, 0], delta)[0]
    words, cts = R.contract_rows(rng, s_lwe, log_n, p)
    assert len(cts) == 125
    got = api.lwe_rotation_batch(np.array(s_lwe, np.uint64), cts, N, p, want=("rot", "idx"))
    msg = api.lwe_decode_batch(np.array(s_lwe, np.uint64), cts, delta, 2 * p, want=("msg",))["msg"]
    differ = np.nonzero(got["idx"] != msg)[0]
    assert len(differ) >= 1
    acc0 = [[0] * N for _ in range(K - 1)] + [[int(v) for v in testv]]
    for r in sorted(set(range(0, 125, 3)) | set(differ[:4].tolist())):
        out = T.pbs_chain(ring, acc0, [int(v) for v in cts[r]], bsk, ksk, K, ELL, LOGB)[-1]
        coeffs = T.glwe_decrypt(ring, s_to[:K - 1], out, K)
        for j in range(4):
            assert coeffs[j] == api.lut_expect(testv, int(got["rot"][r]), j), (r, j)
