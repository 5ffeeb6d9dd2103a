"""CPU side of the batched client calls (csrc/lwe_client.hip) through their null-context host path: vpbs_lwe_encrypt_batch against the seeded
restatement (tests/tfhe_oracle.py) and the one-ciphertext call, vpbs_lut_testv against vpbs_testv and a table checked by hand,
vpbs_lwe_decode_batch and vpbs_noise_stats against Python integers (tests/lwe_client_oracle.py), and every refusal that needs no device."""
import ctypes as C

import numpy as np
import pytest

import lwe_client_oracle as O
import tfhe_oracle as T
from vpbs_amd import api

P = api.P
SIGMA_LWE = 1.17021618159313e-5       # main.rs:30
NAMES = ["vpbs_lwe_encrypt_batch", "vpbs_lut_testv", "vpbs_lwe_decode_batch"]


def params(n_lwe, seed, sigma_lwe=0.0, log_n=10, K=2, ELL=4, LOGB=5):
    return api.KeygenParamsC(log_n, K, ELL, LOGB, n_lwe, seed, 0.0, sigma_lwe)


def test_library_exports_the_entry_points_and_api_binds_them():
    L = api.lib()
    for name in NAMES:
        assert name in api.SIGNATURES, name
        fn = getattr(L, name)
        assert fn.argtypes == api.SIGNATURES[name][1] and fn.restype == api.SIGNATURES[name][0]
    for name in ("lwe_encrypt_batch", "lwe_decode_batch"):
        assert callable(getattr(api, name)) and hasattr(api.Context, name)
    assert C.sizeof(api.NoiseStatsC) == 8 * 75


@pytest.mark.parametrize("sigma", [0.0, SIGMA_LWE])
@pytest.mark.parametrize("n_lwe", [1, 65, 728])
def test_encrypt_batch_is_the_single_call_row_by_row(n_lwe, sigma):
    seed = 0xC0FFEE + n_lwe
    prm = params(n_lwe, seed, sigma)
    rng = np.random.default_rng(n_lwe)
    s = rng.integers(0, 2, size=n_lwe, dtype=np.uint64)
    delta = T.get_delta(4)
    msgs = [0, 1, P - 1, delta, 3 * delta % P]
    for nonce0 in (0, (1 << 24) - len(msgs)):
        got = api.lwe_encrypt_batch(prm, s, msgs, nonce0=nonce0)
        assert got.shape == (len(msgs), n_lwe + 1)
        for i, m in enumerate(msgs):
            assert got[i].tolist() == T.seeded_lwe_encrypt(seed, [int(v) for v in s], m, sigma, nonce=nonce0 + i), (nonce0, i)
            assert (got[i] == api.lwe_encrypt(prm, s, m, nonce=nonce0 + i)).all(), (nonce0, i)
    if sigma:
        assert (api.lwe_encrypt_batch(prm, s, msgs) != api.lwe_encrypt_batch(params(n_lwe, seed), s, msgs))[:, n_lwe].all()   # noise is drawn


def test_encrypt_batch_with_a_key_that_is_not_binary():
    n_lwe, seed = 9, 5
    prm = params(n_lwe, seed, SIGMA_LWE)
    s = np.array([0, 1, 2, P - 1, P, P + 3, 1 << 63, 0, 1], np.uint64)
    got = api.lwe_encrypt_batch(prm, s, [7, 8], nonce0=100)
    for i in range(2):
        assert (got[i] == api.lwe_encrypt(prm, s, 7 + i, nonce=100 + i)).all()
        assert got[i].tolist() == T.seeded_lwe_encrypt(seed, [int(v) % P for v in s], 7 + i, SIGMA_LWE, nonce=100 + i)
    assert api.lwe_encrypt_batch(prm, s, []).shape == (0, n_lwe + 1)


def test_encrypt_batch_refusals():
    prm, s = params(6, 1), np.ones(6, np.uint64)
    with pytest.raises(api.VpbsError, match="message 2 is not below p"):
        api.lwe_encrypt_batch(prm, s, [0, P - 1, P, P + 1])
    with pytest.raises(api.VpbsError, match="2\\^24"):
        api.lwe_encrypt_batch(prm, s, [0, 1, 2], nonce0=(1 << 24) - 2)
    assert api.lwe_encrypt_batch(prm, s, [0, 1], nonce0=(1 << 24) - 2).shape == (2, 7)
    L = api.lib()
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    assert L.vpbs_lwe_encrypt_batch(None, C.byref(prm), p, 0, p, 2, 0, p, 0) == 0
    assert L.vpbs_lwe_encrypt_batch(None, None, p, 0, p, 2, 0, p, 0) == -1             # VPBS_ERR_INVALID
    assert L.vpbs_lwe_encrypt_batch(None, C.byref(prm), None, 0, p, 2, 0, p, 0) == -1
    assert L.vpbs_lwe_encrypt_batch(None, C.byref(prm), p, 0, None, 2, 0, p, 0) == -1
    assert L.vpbs_lwe_encrypt_batch(None, C.byref(prm), p, 0, p, 2, 0, None, 0) == -1
    assert L.vpbs_lwe_encrypt_batch(None, C.byref(prm), p, 1, p, 2, 0, p, 0) == -1     # device pointers without a context
    assert L.vpbs_lwe_encrypt_batch(None, C.byref(prm), p, 0, p, 2, 0, p, 1) == -1


@pytest.mark.parametrize("N", [8, 1024])
def test_lut_testv_of_the_identity_table_is_testv(N):
    for p in (1, 2, 4, N):
        want, delta = api.testv(N, p)
        got, d = api.lut_testv(N, p, list(range(p)))
        assert d == delta == T.get_delta(2 * p) and (got == want).all(), p
        assert got.tolist() == O.lut_testv(N, p, list(range(p)), delta), p
        got2, _ = api.lut_testv(N, p, list(range(p)), delta=delta)
        assert (got2 == want).all()


def test_lut_testv_of_a_permutation_checked_by_hand():
    """N = 8, p = 4: blocks of two, shifted left by one; table 2 0 3 1 -> coefficients 2 2 0 0 3 3 1 1 (times delta) -> 2 0 0 3 3 1 1 -2"""
    delta = T.get_delta(8)
    got, _ = api.lut_testv(8, 4, [2, 0, 3, 1])
    assert got.tolist() == [2 * delta, 0, 0, 3 * delta, 3 * delta, delta, delta, P - 2 * delta]
    # entries in [p, 2 p) and another delta
    got, d = api.lut_testv(8, 4, [7, 4, 0, 5], delta=12345)
    assert d == 12345 and got.tolist() == [7 * 12345, 4 * 12345, 4 * 12345, 0, 0, 5 * 12345, 5 * 12345, P - 7 * 12345]
    assert got.tolist() == O.lut_testv(8, 4, [7, 4, 0, 5], 12345)


def test_lut_testv_refusals():
    L = api.lib()
    out, tab = np.zeros(8, np.uint64), np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, 0, 0, 0, 0, 0, 0, 0], np.uint64)
    ok = lambda log_n, p, t: L.vpbs_lut_testv(log_n, p, api._ptr(t), 5, api._ptr(out))
    assert ok(3, 4, tab) == 0
    assert ok(3, 4, np.array([0, 1, 8, 3], np.uint64)) == -1     # an entry at 2 p
    assert ok(3, 3, tab) == -1                                    # p not a power of two
    assert ok(3, 16, tab) == -1                                   # p > N
    assert ok(3, 0, tab) == -1
    assert L.vpbs_lut_testv(3, 4, None, 5, api._ptr(out)) == -1 and L.vpbs_lut_testv(3, 4, api._ptr(tab), 5, None) == -1
    with pytest.raises(api.VpbsError):
        api.lut_testv(8, 4, [0, 1, 2, 8])
    with pytest.raises(ValueError):
        api.lut_testv(8, 4, [0, 1, 2])


def test_decode_phase_is_lwe_decrypt():
    rng = np.random.default_rng(3)
    for n in (1, 6, 64, 65, 728):
        s = rng.integers(0, P, size=n, dtype=np.uint64)
        cts = rng.integers(0, P, size=(7, n + 1), dtype=np.uint64)
        cts[0, 0], cts[1, n], s[0] = np.uint64(P), np.uint64((1 << 64) - 1), np.uint64(P + 1)       # words at or above p
        got = api.lwe_decode_batch(s, cts, 1 << 61, 4, want=("phase",))
        assert list(got) == ["phase"] and (got["phase"] == api.lwe_decrypt(s, cts)).all(), n
        assert got["phase"].tolist() == [O.phase(s, c) for c in cts]


def trivial(phases, n=3):
    """ciphertexts of the given phases under the zero key"""
    cts = np.zeros((len(phases), n + 1), np.uint64)
    cts[:, n] = np.array(phases, np.uint64)
    return np.zeros(n, np.uint64), cts


@pytest.mark.parametrize("delta,modulus", [(T.get_delta(4), 4), (T.get_delta(8), 8), ((1 << 61) + 1, 5), (P, 1), (1, 1 << 40)])
def test_decode_rounds_at_the_half_way_points(delta, modulus):
    half, top = delta // 2, modulus - 1
    up = 1 if delta % 2 == 0 else 0          # an even delta has an exact half-way point, and it rounds up
    phases = [half - 1, half, half + 1, top * delta + half - 1, top * delta + half, top * delta + half + 1]
    want = [0, up % modulus, 1 % modulus, top, (top + up) % modulus, 0]
    if delta == 1:                            # half = 0: the first of each triple is one below the message itself
        phases, want = [0, 1, top, top + 1], [0, 1 % modulus, top, 0]
    if delta == P:                            # one message, nothing above the half-way point is below p
        phases, want = [0, half - 1, half, P - 1], [0, 0, 0, 0]
    s, cts = trivial(phases)
    got = api.lwe_decode_batch(s, cts, delta, modulus, want=("phase", "msg", "err"))
    assert got["phase"].tolist() == phases and got["msg"].tolist() == want
    assert got["msg"].tolist() == [O.decode(ph, delta, modulus)[0] for ph in phases]
    assert got["err"].dtype == np.int64 and got["err"].tolist() == [O.decode(ph, delta, modulus)[1] for ph in phases]


def test_decode_err_sign_and_centring():
    delta, modulus = T.get_delta(4), 4
    half = delta // 2
    for m in (0, 1, 3):
        errs = [0, 1, -1, half, -half, half - 1, -(half - 1)]
        s, cts = trivial([(m * delta + e) % P for e in errs])
        got = api.lwe_decode_batch(s, cts, delta, modulus, expected=[m] * len(errs), want=("msg", "err"))
        assert got["err"].tolist() == errs, m
        # +half rounds up to the next message, -half stays: the rounding is floor((phase + half) / delta)
        assert got["msg"].tolist() == [m, m, m, (m + 1) % 4, m, m, m]
        # without expected, err is measured from the decoded message itself; 3 delta + half decodes to 4 mod 4 = 0, and p = 4 delta + 1
        own = api.lwe_decode_batch(s, cts, delta, modulus, want=("err",))["err"].tolist()
        assert own == [0, 1, -1, -half - 1 if m == 3 else -half, -half, half - 1, -(half - 1)]
    # the centring interval is (-p/2, p/2]: with delta = p every phase is its own error
    s, cts = trivial([(P - 1) // 2, (P + 1) // 2, P - 1, 0])
    assert api.lwe_decode_batch(s, cts, P, 1, want=("err",))["err"].tolist() == [(P - 1) // 2, -((P - 1) // 2), -1, 0]
    # expected is not reduced for err: ref * delta mod p
    s, cts = trivial([5])
    assert api.lwe_decode_batch(s, cts, delta, 4, expected=[6], want=("err",))["err"].tolist() == [O.decode(5, delta, 4, 6)[1]]


def seeded_set(n, count, delta, modulus, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, size=n, dtype=np.uint64)
    msgs = rng.integers(0, modulus, size=count)
    noise = rng.integers(-(delta // 8), delta // 8, size=count)
    cts = rng.integers(0, P, size=(count, n + 1), dtype=np.uint64)
    for i in range(count):
        ip = sum(int(a) for a, b in zip(cts[i, :n], s) if b) % P
        cts[i, n] = np.uint64((ip + int(msgs[i]) * delta + int(noise[i])) % P)
    return s, cts, msgs.astype(np.uint64), noise


def test_statistics_match_the_oracle_and_accumulate():
    delta, modulus, n, count = T.get_delta(8), 8, 20, 60
    s, cts, msgs, noise = seeded_set(n, count, delta, modulus, 77)
    expected = msgs.copy()
    expected[17] = (expected[17] + 3) % modulus            # one forced failure
    st, want = api.NoiseStats(), O.Stats()
    got = api.lwe_decode_batch(s, cts, delta, modulus, expected=expected, stats=st, want=("msg", "err"))
    ph, ms, er = O.decode_batch(s, cts, delta, modulus, expected, want)
    assert got["msg"].tolist() == ms == msgs.tolist() and got["err"].tolist() == er
    assert [e for i, e in enumerate(er) if i != 17] == [int(v) for i, v in enumerate(noise) if i != 17]
    assert st.as_dict() == want.as_dict() and st.failures == 1 and st.count == count
    # a second call adds to the same struct; this one has errors near p / 2, so that the sums pass 64, 128 bits
    big = [(P - 1) // 2, (P + 1) // 2, (P - 1) // 2 - 1] * 5
    s0, cts0 = trivial(big, n)
    api.lwe_decode_batch(s0, cts0, P, 1, stats=st, want=())
    O.decode_batch(s0, cts0, P, 1, None, want)
    assert st.as_dict() == want.as_dict() and st.count == count + 15 and st.sum_sq >> 128 and st.max_abs == (P - 1) // 2
    assert st.hist[63] == 15 + (abs(er[17]).bit_length() == 63) and sum(st.hist) == st.count and st.hist[64] == 0
    mean = want.sum_signed / want.count
    assert st.mean() == pytest.approx(mean, rel=1e-12)
    assert st.std() == pytest.approx((want.sum_sq / want.count - mean * mean) ** 0.5, rel=1e-9)
    assert st.mean_abs() == pytest.approx(want.sum_abs / want.count, rel=1e-12)
    # a negative total
    neg = api.NoiseStats()
    s1, cts1 = trivial([P - 5, P - 7, 1])
    api.lwe_decode_batch(s1, cts1, 1 << 62, 4, stats=neg, want=())
    assert neg.sum_signed == -11 and neg.sum_abs == 13 and neg.sum_sq == 75 and neg.max_abs == 7 and neg.hist[3] == 2 and neg.hist[1] == 1


def test_decode_refusals():
    L = api.lib()
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    call = lambda s, c, n, delta, modulus, where=0, key_dev=0, count=2: L.vpbs_lwe_decode_batch(None, s, key_dev, c, count, n, delta, modulus, None, p, p,
                                                                                               p, None, where)
    assert call(p, p, 3, 5, 2) == 0
    assert call(None, p, 3, 5, 2) == -1 and call(p, None, 3, 5, 2) == -1
    assert call(p, p, 0, 5, 2) == -1 and call(p, p, 3, 0, 2) == -1 and call(p, p, 3, 5, 0) == -1
    assert call(p, p, 3, 5, 2, where=1) == -1 and call(p, p, 3, 5, 2, where=2) == -1 and call(p, p, 3, 5, 2, key_dev=1) == -1
    assert call(p, p, 3, 5, 2, where=3) == -1
    assert call(p, None, 3, 5, 2, count=0) == 0
    with pytest.raises(ValueError):
        api.lwe_decode_batch(np.zeros(3, np.uint64), np.zeros((2, 5), np.uint64), 5, 2)
    with pytest.raises(ValueError):
        api.lwe_decode_batch(np.zeros(3, np.uint64), np.zeros((2, 4), np.uint64), 5, 2, want=("message",))
