"""CPU side of the seeded keys and ciphertexts (csrc/keygen.hip, csrc/key_seeded.hip, csrc/lwe_client.hip): the entry points in the header,
api.SIGNATURES and the Rust binding; the null-context host forms of vpbs_lwe_encrypt_seeded_batch and vpbs_lwe_expand_batch against the split
generator restated in tests/seeded_oracle.py; with mask_seed == seed, expand(encrypt_seeded) against vpbs_lwe_encrypt_batch word for word;
the refusals that need no device; the shape helpers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import seeded_oracle as SO
import tfhe_oracle as T
from vpbs_amd import api

P = api.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA_LWE = 1.17021618159313e-5       # main.rs:30
ENTRIES = ["vpbs_keygen_seeded", "vpbs_key_expand", "vpbs_lwe_encrypt_seeded_batch", "vpbs_lwe_expand_batch", "vpbs_keyring_add_seeded",
           "vpbs_ring_prover_add_seeded"]
INVALID = -1


def params(n_lwe, seed, sigma_lwe=0.0, log_n=10, K=2, ELL=4, LOGB=5):
    return api.KeygenParamsC(log_n, K, ELL, LOGB, n_lwe, seed, 0.0, sigma_lwe)


def test_header_signatures_and_rust_binding_carry_the_entries():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vpbs_prover.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "vpbs_sys.rs")).read()
    L = api.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert "pub fn %s(" % name in rust, name
        assert name in api.SIGNATURES, name
        fn = getattr(L, name)
        assert fn.argtypes == api.SIGNATURES[name][1] and fn.restype == api.SIGNATURES[name][0]
    for name in ("lwe_encrypt_seeded_batch", "lwe_expand_batch"):
        assert callable(getattr(api, name)) and hasattr(api.Context, name)
    for name in ("keygen_seeded", "key_expand"):
        assert hasattr(api.Context, name)
    assert hasattr(api.KeyRing, "add_seeded") and hasattr(api.RingProver, "add_seeded")


@pytest.mark.parametrize("sigma", [0.0, SIGMA_LWE])
@pytest.mark.parametrize("n_lwe", [1, 65, 728])
def test_host_forms_against_the_split_oracle(n_lwe, sigma):
    seed, mask_seed = 0xC0FFEE + n_lwe, 0xFACADE - n_lwe
    prm = params(n_lwe, seed, sigma)
    s = np.random.default_rng(n_lwe).integers(0, 2, size=n_lwe, dtype=np.uint64)
    delta = T.get_delta(4)
    msgs = [0, 1, P - 1, delta, 3 * delta % P]
    for nonce0 in (0, (1 << 24) - len(msgs)):
        bodies = api.lwe_encrypt_seeded_batch(prm, mask_seed, s, msgs, nonce0=nonce0)
        assert bodies.shape == (len(msgs),) and bodies.dtype == np.uint64
        rows = api.lwe_expand_batch(n_lwe, mask_seed, bodies, nonce0=nonce0)
        assert rows.shape == (len(msgs), n_lwe + 1)
        for i, m in enumerate(msgs):
            want = SO.split_lwe_encrypt(seed, mask_seed, s, m, sigma, nonce=nonce0 + i)
            assert int(bodies[i]) == want[-1], (nonce0, i)
            assert rows[i].tolist() == want, (nonce0, i)
    # the masks are the mask seed's alone, the noise the private seed's alone
    other = api.lwe_expand_batch(n_lwe, mask_seed, np.zeros(3, np.uint64))
    assert (other[:, :n_lwe] == api.lwe_encrypt_batch(params(n_lwe, mask_seed), s, [0, 0, 0])[:, :n_lwe]).all() and (other[:, n_lwe] == 0).all()
    if sigma:
        assert (api.lwe_encrypt_seeded_batch(prm, mask_seed, s, msgs) != api.lwe_encrypt_seeded_batch(params(n_lwe, seed), mask_seed, s, msgs)).all()


@pytest.mark.parametrize("count", [1, 67, 300])
@pytest.mark.parametrize("n_lwe", [6, 40, 728])
def test_with_one_seed_expand_of_encrypt_seeded_is_encrypt_batch(n_lwe, count):
    seed = 0x5EED + n_lwe + count
    prm = params(n_lwe, seed, SIGMA_LWE)
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, size=n_lwe, dtype=np.uint64)
    msgs = rng.integers(0, P, size=count, dtype=np.uint64)
    nonce0 = 1000 + count
    bodies = api.lwe_encrypt_seeded_batch(prm, seed, s, msgs, nonce0=nonce0)
    assert (api.lwe_expand_batch(n_lwe, seed, bodies, nonce0=nonce0) == api.lwe_encrypt_batch(prm, s, msgs, nonce0=nonce0)).all()


def test_a_key_that_is_not_binary_and_the_empty_batch():
    n_lwe, seed, mask_seed = 9, 5, 6
    prm = params(n_lwe, seed, SIGMA_LWE)
    s = np.array([0, 1, 2, P - 1, P, P + 3, 1 << 63, 0, 1], np.uint64)
    got = api.lwe_encrypt_seeded_batch(prm, mask_seed, s, [7, 8], nonce0=100)
    for i in range(2):
        assert int(got[i]) == SO.split_lwe_encrypt(seed, mask_seed, [int(v) % P for v in s], 7 + i, SIGMA_LWE, nonce=100 + i)[-1]
    assert api.lwe_encrypt_seeded_batch(prm, mask_seed, s, []).shape == (0,)
    assert api.lwe_expand_batch(n_lwe, mask_seed, []).shape == (0, n_lwe + 1)
    # a body at or above p is copied unchanged
    assert api.lwe_expand_batch(n_lwe, mask_seed, [P + 1, (1 << 64) - 1])[:, n_lwe].tolist() == [P + 1, (1 << 64) - 1]


def test_refusals_on_the_host():
    n_lwe = 6
    prm = params(n_lwe, 1)
    s = np.ones(n_lwe, np.uint64)
    with pytest.raises(api.VpbsError, match="message 2 is not below p"):
        api.lwe_encrypt_seeded_batch(prm, 2, s, [0, P - 1, P, P + 1])
    with pytest.raises(api.VpbsError, match="2\\^24"):
        api.lwe_encrypt_seeded_batch(prm, 2, s, [0, 1, 2], nonce0=(1 << 24) - 2)
    assert api.lwe_encrypt_seeded_batch(prm, 2, s, [0, 1], nonce0=(1 << 24) - 2).shape == (2,)
    with pytest.raises(api.VpbsError, match="2\\^24"):
        api.lwe_expand_batch(n_lwe, 2, [0, 1, 2], nonce0=(1 << 24) - 2)
    assert api.lwe_expand_batch(n_lwe, 2, [0, 1], nonce0=(1 << 24) - 2).shape == (2, n_lwe + 1)
    with pytest.raises(api.VpbsError, match="n_lwe"):
        api.lwe_expand_batch(0, 2, [0])
    L = api.lib()
    mark = np.uint64(0xA5A5A5A5A5A5A5A5)
    buf = np.full(2 * (n_lwe + 1), mark, np.uint64)
    two = np.array([3, 4], np.uint64)
    p, q = buf.ctypes.data, two.ctypes.data
    enc = lambda *a: L.vpbs_lwe_encrypt_seeded_batch(*a)
    assert enc(None, C.byref(prm), 2, s.ctypes.data, 0, q, 2, 0, p, 0) == 0 and (buf[:2] != mark).all() and (buf[2:] == mark).all()
    buf[:] = mark
    assert enc(None, None, 2, s.ctypes.data, 0, q, 2, 0, p, 0) == INVALID
    assert enc(None, C.byref(prm), 2, None, 0, q, 2, 0, p, 0) == INVALID
    assert enc(None, C.byref(prm), 2, s.ctypes.data, 0, None, 2, 0, p, 0) == INVALID
    assert enc(None, C.byref(prm), 2, s.ctypes.data, 0, q, 2, 0, None, 0) == INVALID
    assert enc(None, C.byref(prm), 2, s.ctypes.data, 1, q, 2, 0, p, 0) == INVALID     # device pointers without a context
    assert enc(None, C.byref(prm), 2, s.ctypes.data, 0, q, 2, 0, p, 1) == INVALID
    assert enc(None, C.byref(prm), 2, s.ctypes.data, 0, q, 2, (1 << 24) - 1, p, 0) == INVALID
    exp = lambda *a: L.vpbs_lwe_expand_batch(*a)
    assert exp(None, n_lwe, 2, 0, None, 2, p, 0) == INVALID
    assert exp(None, n_lwe, 2, 0, q, 2, None, 0) == INVALID
    assert exp(None, n_lwe, 2, 0, q, 2, p, 1) == INVALID                              # device pointers without a context
    assert exp(None, 0, 2, 0, q, 2, p, 0) == INVALID and exp(None, 1 << 24, 2, 0, q, 2, p, 0) == INVALID
    assert exp(None, n_lwe, 2, (1 << 24) - 1, q, 2, p, 0) == INVALID and exp(None, n_lwe, 2, (1 << 24) + 1, q, 0, p, 0) == INVALID
    assert (buf == mark).all()                                                        # no refusal wrote a word
    assert exp(None, n_lwe, 2, 0, q, 2, p, 0) == 0 and buf[n_lwe] == 3 and buf[2 * n_lwe + 1] == 4
    # the calls that need a context refuse a null one
    assert L.vpbs_key_expand(None, None, 6, 0, None, None, 0, None, None, 0) == INVALID
    assert L.vpbs_keygen_seeded(None, C.byref(prm), 0, None, None, None, None, None, None, None, 0) == INVALID
    slot = C.c_uint(77)
    assert L.vpbs_keyring_add_seeded(None, 0, p, p, 0, C.byref(slot)) == INVALID and slot.value == 77
    err = C.create_string_buffer(512)
    assert L.vpbs_ring_prover_add_seeded(None, 0, p, p, 0, C.byref(slot), err, 512) == INVALID and slot.value == 77 and err.value


def test_shape_helpers():
    # the paper's key set: 95 551 488 bytes full, half of it as bodies (K = 2)
    bodies, full = api.seeded_key_shapes(1024, 2, 4, 728)
    assert full == 729 * 2 * 4 * 2 * 1024 and bodies * 2 == full and 8 * full == 95551488 and 8 * bodies == 47775744
    assert api.seeded_key_shapes(64, 3, 3, 40) == (41 * 3 * 3 * 64, 41 * 3 * 3 * 3 * 64)
    N, K, ELL, n = 8, 2, 4, 6
    g = K * ELL * N
    b, k = api.key_expand_args(N, K, ELL, n, [[1] * g] * n, [[2] * N] * (K * ELL))
    assert b.shape == (n, g) and k.shape == (g,) and b.dtype == k.dtype == np.uint64 and b.flags["C_CONTIGUOUS"]
    assert api.key_expand_args(N, K, ELL, n, None, np.zeros(g, np.uint64))[0] is None
    assert api.key_expand_args(N, K, ELL, n, np.zeros((n, g), np.uint64), None)[1] is None
    for bad_b, bad_k in ((np.zeros((n, g + 1)), np.zeros(g)), (np.zeros((n + 1, g)), np.zeros(g)), (np.zeros((n, g)), np.zeros(g * K)),
                         (np.zeros(n * g), np.zeros(g))):
        with pytest.raises(ValueError, match="key_expand"):
            api.key_expand_args(N, K, ELL, n, bad_b, bad_k)
