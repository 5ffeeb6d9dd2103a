"""CPU side of the batched bootstrap (csrc/pbs_batch.hip): the exported entry points and their ctypes bindings, vpbs_lwe_decrypt against
its restatement, the argument checks that need no device, and the identity the restatement of sample extraction exists for."""
import ctypes as C

import numpy as np
import pytest

import pbs_batch_oracle as B
import tfhe_oracle as T
from vpbs_amd import api

P = api.P
NAMES = ["vpbs_bootstrapper_create", "vpbs_bootstrapper_run", "vpbs_bootstrapper_free", "vpbs_lwe_extract", "vpbs_lwe_decrypt"]


def test_library_exports_the_entry_points_and_api_binds_them():
    L = api.lib()
    for name in NAMES:
        assert name in api.SIGNATURES, name
        fn = getattr(L, name)
        assert fn.argtypes == api.SIGNATURES[name][1] and fn.restype == api.SIGNATURES[name][0]
    assert callable(api.lwe_decrypt) and hasattr(api.Context, "lwe_extract") and hasattr(api.Bootstrapper, "run")


def test_lwe_decrypt_matches_the_restatement():
    rng = np.random.default_rng(11)
    for n in (1, 2, 6, 40, 728, 1500):
        s = rng.integers(0, 2, size=n, dtype=np.uint64)
        ct = rng.integers(0, P, size=n + 1, dtype=np.uint64)
        assert api.lwe_decrypt(s, ct) == B.lwe_decrypt(s, ct), n
        # a key that is not binary: the inner product is a full field product
        s = rng.integers(0, P, size=n, dtype=np.uint64)
        assert api.lwe_decrypt(s, ct) == B.lwe_decrypt(s, ct), n
    edge = [0, 1, P - 1]
    for body in edge:
        for a in edge:
            for k in edge:
                s, ct = np.array([k, 1, P - 1], np.uint64), np.array([a, P - 1, P - 1, body], np.uint64)
                assert api.lwe_decrypt(s, ct) == B.lwe_decrypt(s, ct), (body, a, k)
    cts = rng.integers(0, P, size=(5, 9), dtype=np.uint64)
    s = rng.integers(0, 2, size=8, dtype=np.uint64)
    assert api.lwe_decrypt(s, cts).tolist() == [B.lwe_decrypt(s, c) for c in cts]


def test_null_arguments_are_refused_without_a_device():
    L = api.lib()
    buf = np.zeros(64, np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    assert L.vpbs_bootstrapper_run(None, p, 1, p, 0, p, p, None, 0) == -1          # VPBS_ERR_INVALID
    assert L.vpbs_lwe_extract(None, 3, 2, 6, p, 1, p, 0) == -1
    out = C.c_void_p()
    err = C.create_string_buffer(256)
    prm = api.TfheParamsC(3, 2, 4, 5)
    assert L.vpbs_bootstrapper_create(None, C.byref(prm), 6, p, p, 0, 4, C.byref(out), err, 256) == -1 and not out.value
    assert err.value != b""
    L.vpbs_bootstrapper_free(None)
    one = np.zeros(1, np.uint64)
    assert L.vpbs_lwe_decrypt(None, api._ptr(buf), 3, api._ptr(one)) == -1
    assert L.vpbs_lwe_decrypt(api._ptr(buf), None, 3, api._ptr(one)) == -1
    assert L.vpbs_lwe_decrypt(api._ptr(buf), api._ptr(buf), 3, None) == -1


def test_sample_extract_order():
    ct = [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]]
    assert B.sample_extract(ct) == [1, P - 4, P - 3, P - 2, 5, P - 8, P - 7, P - 6, 9]
    assert B.extract(ct, 6) == [1, P - 4, P - 3, P - 2, 5, P - 8, 9]
    assert B.extract([[0, 0], [7, 1]], 2) == [0, 0, 7]                      # the negation of 0 is 0


@pytest.mark.parametrize("log_n,K,n_lwe", [(3, 2, 6), (3, 2, 8), (3, 2, 1), (6, 2, 40), (6, 3, 40), (6, 3, 64), (6, 3, 100), (6, 3, 128),
                                           (4, 4, 37), (10, 2, 728)])
def test_extraction_commutes_with_decryption(log_n, K, n_lwe):
    """lwe::decrypt(flatten_partial_key(s_to), partial_sample_extract(ct)) == Glwe::decrypt(s_to, ct)[0] for any GLWE ct: the constant
    coefficient of a_j * s_j over X^N + 1 is a_j[0] s_j[0] - sum_{c >= 1} a_j[N - c] s_j[c], and the key has no coefficient past n_lwe
    (glwe.rs:194-214 is this identity on an encryption)"""
    ring = T.Ring(log_n)
    rng = np.random.default_rng(1000 * log_n + 10 * K + n_lwe)
    for trial in range(3):
        s_to = B.partial_key(rng, ring.n, K, n_lwe)
        assert sum(map(sum, s_to)) == sum(B.flatten_partial_key(s_to, n_lwe))
        ct = [[int(v) for v in rng.integers(0, P, size=ring.n, dtype=np.uint64)] for _ in range(K)]
        if trial == 2:                    # edge words in the mask and the body
            ct[0][0], ct[0][1], ct[0][ring.n - 1], ct[K - 1][0] = 0, P - 1, 0, P - 1
        want = T.glwe_decrypt(ring, s_to[:K - 1], ct, K)[0]
        lwe = B.extract(ct, n_lwe)
        assert len(lwe) == n_lwe + 1
        assert B.lwe_decrypt(B.flatten_partial_key(s_to, n_lwe), lwe) == want
        assert api.lwe_decrypt(np.array(B.flatten_partial_key(s_to, n_lwe), np.uint64), np.array(lwe, np.uint64)) == want
