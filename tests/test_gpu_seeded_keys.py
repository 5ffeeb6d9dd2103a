"""GPU tests (-m gpu) of the seeded keys and ciphertexts: vpbs_keygen_seeded, vpbs_key_expand (csrc/keygen.hip, csrc/key_seeded.hip),
vpbs_keyring_add_seeded, vpbs_ring_prover_add_seeded, vpbs_lwe_encrypt_seeded_batch and vpbs_lwe_expand_batch.  Yardsticks: vpbs_keygen
itself when mask_seed is the seed (the anchor), the split generator restated in tests/seeded_oracle.py when it is not, the null-context host
forms of the ciphertext calls, and the slots that KeyRing.add / RingProver.add fill.  Exact field arithmetic: every comparison is word for
word."""
import ctypes as C

import numpy as np
import pytest
import torch

import export_circuits
import seeded_oracle as SO
import tfhe_oracle as T
import vpbs_amd
from vpbs_amd import api, circuit_file

pytestmark = pytest.mark.gpu
P = api.P
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)       # main.rs:29-30
MARK = np.uint64(0xA5A5A5A5A5A5A5A5)
INVALID = -1   # VPBS_ERR_INVALID
# (log_N, n_lwe, K, ELL, LOGB): fewer points than lanes; two mask polynomials per GLWE; every pass of the transform at N = 1024; the extra
# pass at N = 2048
SHAPES = [(3, 6, 2, 4, 5), (6, 40, 3, 3, 7), (10, 3, 2, 4, 5), (11, 2, 2, 4, 5)]


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    yield c
    c.close()


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def dev_full(shape, value=0):
    d = torch.full(shape, int(np.uint64(value).view(np.int64)), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()         # torch fills on its stream, the calls work on the context's own
    return d


def back(d):
    return d.cpu().numpy().view(np.uint64)


def masks(ggsw_flat, K, ELL, N):
    """the K - 1 mask polynomials of every GLWE of flattened GGSWs"""
    g = np.asarray(ggsw_flat)
    return g.reshape(g.shape[:-1] + (K * ELL, K, N))[..., :K - 1, :]


def own_secrets(rng, n, K, N):
    return rng.integers(0, 2, size=n, dtype=np.uint64), rng.integers(0, 2, size=(K - 1, N), dtype=np.uint64)


@pytest.mark.parametrize("log_n,n,K,ELL,LOGB", SHAPES)
def test_anchor_with_one_seed_expand_of_keygen_seeded_is_keygen(ctx, log_n, n, K, ELL, LOGB):
    N, seed = 1 << log_n, 0xA2C402 + log_n
    keys = ctx.keygen(N, K, ELL, LOGB, n, seed, *SIGMAS)
    sk = ctx.keygen_seeded(N, K, ELL, LOGB, n, seed, seed, *SIGMAS)
    for name in ("s_lwe", "s_glwe", "s_to"):
        assert (sk[name] == keys[name]).all(), name
    assert sk["bsk_bodies"].shape == (n, K * ELL * N) and sk["ksk_bodies"].shape == (K * ELL * N,)
    assert (sk["bsk_bodies"] == SO.bodies_of(keys["bsk"], K, ELL, N)).all() and (sk["ksk_bodies"] == SO.bodies_of(keys["ksk"], K, ELL, N)).all()
    ex = ctx.key_expand(N, K, ELL, n, seed, sk["bsk_bodies"], sk["ksk_bodies"])
    assert (ex["bsk"] == keys["bsk"]).all(), np.argwhere(ex["bsk"] != keys["bsk"])[:4].tolist()
    assert (ex["ksk"] == keys["ksk"]).all(), np.argwhere(ex["ksk"] != keys["ksk"])[:4].tolist()
    # either pair alone
    only_k = ctx.key_expand(N, K, ELL, n, seed, None, sk["ksk_bodies"])
    only_b = ctx.key_expand(N, K, ELL, n, seed, sk["bsk_bodies"], None)
    assert only_k["bsk"] is None and (only_k["ksk"] == keys["ksk"]).all() and only_b["ksk"] is None and (only_b["bsk"] == keys["bsk"]).all()


@pytest.mark.parametrize("log_n,n,K,ELL,LOGB", SHAPES[:2])
def test_split_against_the_oracle(ctx, log_n, n, K, ELL, LOGB):
    N, seed, mask_seed = 1 << log_n, 0x5EC2E7 + log_n, 0x9B11C + log_n
    sk = ctx.keygen_seeded(N, K, ELL, LOGB, n, seed, mask_seed, *SIGMAS)
    ring = T.Ring(log_n)
    s_to, s_lwe, s_glwe, bsk, ksk = SO.split_pbs_keys(ring, seed, mask_seed, n, K, ELL, LOGB, *SIGMAS)
    assert (sk["s_to"] == np.array(s_to, np.uint64)).all() and (sk["s_lwe"] == np.array(s_lwe, np.uint64)).all()
    assert (sk["s_glwe"] == np.array(s_glwe, np.uint64)).all()
    want_bsk = np.stack([bsk[i] for i in range(n)])
    assert (sk["bsk_bodies"] == SO.bodies_of(want_bsk, K, ELL, N)).all() and (sk["ksk_bodies"] == SO.bodies_of(ksk, K, ELL, N)).all()
    ex = ctx.key_expand(N, K, ELL, n, mask_seed, sk["bsk_bodies"], sk["ksk_bodies"])
    assert (ex["bsk"] == want_bsk).all() and (ex["ksk"] == ksk).all()
    # the masks are those of the one-seed generator under mask_seed, the secrets are not
    pub = ctx.keygen(N, K, ELL, LOGB, n, mask_seed, *SIGMAS)
    assert (masks(ex["bsk"], K, ELL, N) == masks(pub["bsk"], K, ELL, N)).all() and (masks(ex["ksk"], K, ELL, N) == masks(pub["ksk"], K, ELL, N)).all()
    assert (SO.bodies_of(ex["bsk"], K, ELL, N) != SO.bodies_of(pub["bsk"], K, ELL, N)).any()
    assert (ctx.keygen(N, K, ELL, LOGB, n, seed, *SIGMAS)["s_lwe"] == sk["s_lwe"]).all()


@pytest.mark.parametrize("log_n,n,K,ELL,LOGB", SHAPES[:2])
def test_own_secrets(ctx, log_n, n, K, ELL, LOGB):
    N, seed, mask_seed = 1 << log_n, 0x0E5EC + log_n, 0x3A5C + log_n
    # the secrets that the seed itself yields reproduce the NULL form
    null = ctx.keygen_seeded(N, K, ELL, LOGB, n, seed, mask_seed, *SIGMAS)
    same = ctx.keygen_seeded(N, K, ELL, LOGB, n, seed, mask_seed, *SIGMAS, s_lwe=null["s_lwe"], s_glwe=null["s_glwe"])
    for name in ("s_lwe", "s_glwe", "s_to", "bsk_bodies", "ksk_bodies"):
        assert (same[name] == null[name]).all(), name
    # other secrets: the oracle's keys under them
    s_lwe, s_glwe = own_secrets(np.random.default_rng(seed), n, K, N)
    s_lwe[:2] = [1, 0]
    own = ctx.keygen_seeded(N, K, ELL, LOGB, n, seed, mask_seed, *SIGMAS, s_lwe=s_lwe, s_glwe=s_glwe)
    assert (own["s_lwe"] == s_lwe).all() and (own["s_glwe"] == s_glwe).all()
    want_to = np.zeros(K * N, np.uint64)
    want_to[:n] = s_lwe
    assert (own["s_to"] == want_to.reshape(K, N)).all()                     # s_to[x / N][x % N] = s_lwe[x], zeros elsewhere
    ring = T.Ring(log_n)
    sample = list(range(n)) if n <= 6 else [0, 1, 17, n - 1]
    _, _, _, bsk, ksk = SO.split_pbs_keys(ring, seed, mask_seed, n, K, ELL, LOGB, *SIGMAS, bsk_indices=sample, secrets=(s_lwe, s_glwe))
    ex = ctx.key_expand(N, K, ELL, n, mask_seed, own["bsk_bodies"], own["ksk_bodies"])
    assert (ex["ksk"] == ksk).all()
    for i in sample:
        assert (ex["bsk"][i] == bsk[i]).all(), i
    assert (own["bsk_bodies"] != null["bsk_bodies"]).any()
    # GLWE (p = K-1, l = ELL-1) of GGSW i decrypts under the caller's s_glwe to s_i * B^(first + ELL - 1) within 7 sigma q
    for i in (0, 1):
        g = ex["bsk"][i].reshape(K, ELL, K, N)
        ct = np.stack([np.array(ring.bw([int(v) for v in g[K - 1, ELL - 1, r]]), np.uint64) for r in range(K)])
        m = ctx.glwe_decrypt(s_glwe, ct)
        want = int(s_lwe[i]) * pow(2, LOGB * (T.num_limbs(LOGB) - 1), P) % P
        err = [min((int(v) - (want if j == 0 else 0)) % P, (-(int(v) - (want if j == 0 else 0))) % P) for j, v in enumerate(m)]
        assert 0 < max(err) < 7 * T.sigma_to_int(SIGMAS[0]), i


def test_a_secret_that_is_not_binary_is_refused_and_named(ctx):
    log_n, n, K, ELL, LOGB = SHAPES[0]
    N = 1 << log_n
    s_lwe, s_glwe = own_secrets(np.random.default_rng(4), n, K, N)
    bad_lwe, bad_glwe = s_lwe.copy(), s_glwe.copy()
    bad_lwe[3], bad_glwe[0, 5] = 2, 2
    with pytest.raises(api.VpbsError, match=r"s_lwe_in\[3\] = 2 is neither 0 nor 1"):
        ctx.keygen_seeded(N, K, ELL, LOGB, n, 1, 2, *SIGMAS, s_lwe=bad_lwe, s_glwe=s_glwe)
    with pytest.raises(api.VpbsError, match=r"s_glwe_in\[5\] = 2 is neither 0 nor 1"):
        ctx.keygen_seeded(N, K, ELL, LOGB, n, 1, 2, *SIGMAS, s_lwe=s_lwe, s_glwe=bad_glwe)
    # no output word is written, on the host or on the device
    prm = api.KeygenParamsC(log_n, K, ELL, LOGB, n, 1, *SIGMAS)
    g = K * ELL * N
    outs = [np.full(sz, MARK, np.uint64) for sz in (n, (K - 1) * N, K * N, n * g, g)]
    d_b, d_k = dev_full((n * g,), MARK), dev_full((g,), MARK)
    L = api.lib()
    for bodies, on_device in ((tuple(o.ctypes.data for o in outs[3:]), 0), ((d_b.data_ptr(), d_k.data_ptr()), 1)):
        rc = L.vpbs_keygen_seeded(ctx.h, C.byref(prm), 2, bad_lwe.ctypes.data, s_glwe.ctypes.data, api._ptr(outs[0]), api._ptr(outs[1]), api._ptr(outs[2]),
                                  bodies[0], bodies[1], on_device)
        assert rc == INVALID and b"s_lwe_in[3]" in L.vpbs_last_error(ctx.h)
        rc = L.vpbs_keygen_seeded(ctx.h, C.byref(prm), 2, s_lwe.ctypes.data, None, api._ptr(outs[0]), api._ptr(outs[1]), api._ptr(outs[2]), bodies[0],
                                  bodies[1], on_device)
        assert rc == INVALID                                                # one secret without the other
    assert all((o == MARK).all() for o in outs) and (back(d_b) == MARK).all() and (back(d_k) == MARK).all()
    # the context stays usable
    assert (ctx.keygen_seeded(N, K, ELL, LOGB, n, 1, 2, *SIGMAS, s_lwe=s_lwe, s_glwe=s_glwe)["s_lwe"] == s_lwe).all()


@pytest.mark.parametrize("log_n,n,K,ELL,LOGB", SHAPES[:2])
def test_bodies_on_the_host_and_on_the_device_give_the_same_key(ctx, log_n, n, K, ELL, LOGB):
    N, seed, mask_seed = 1 << log_n, 0xD0D + log_n, 0xB0D1E5 + log_n
    g = K * ELL * K * N
    host = ctx.keygen_seeded(N, K, ELL, LOGB, n, seed, mask_seed, *SIGMAS)
    dev = ctx.keygen_seeded(N, K, ELL, LOGB, n, seed, mask_seed, *SIGMAS, on_device=True)
    assert "bsk_bodies" not in dev and (dev["s_lwe"] == host["s_lwe"]).all()
    want = ctx.key_expand(N, K, ELL, n, mask_seed, host["bsk_bodies"], host["ksk_bodies"])
    got = ctx.key_expand(N, K, ELL, n, mask_seed, dev["d_bsk_bodies"], dev["d_ksk_bodies"])            # device bodies, host keys
    assert (got["bsk"] == want["bsk"]).all() and (got["ksk"] == want["ksk"]).all()
    for bodies in ((host["bsk_bodies"], host["ksk_bodies"]), (dev["d_bsk_bodies"], dev["d_ksk_bodies"])):   # ... and device keys
        d_b, d_k = dev_full((n, g), MARK), dev_full((g,), MARK)
        assert ctx.key_expand(N, K, ELL, n, mask_seed, *bodies, d_bsk=d_b.data_ptr(), d_ksk=d_k.data_ptr()) is None
        assert (back(d_b) == want["bsk"]).all() and (back(d_k) == want["ksk"]).all()
    fresh = ctx.key_expand(N, K, ELL, n, mask_seed, dev["d_bsk_bodies"], dev["d_ksk_bodies"], on_device=True)
    bs = api.Bootstrapper(ctx, fresh["d_bsk"], fresh["d_ksk"], K, ELL, LOGB, max_batch=2, N=N, n_lwe=n, keys_on_device=True)
    bs2 = api.Bootstrapper(ctx, want["bsk"], want["ksk"], K, ELL, LOGB, max_batch=2, N=N, n_lwe=n)
    tv, delta = api.testv(N, 2)
    cts = api.lwe_encrypt_batch(host["params"], host["s_lwe"], [0, delta])
    assert all((a == b).all() for a, b in zip(bs.run(cts, tv), bs2.run(cts, tv)))
    bs.close()
    bs2.close()
    # a misaligned device pointer is refused before anything is queued
    d_b = dev_full((n * g + 1,), MARK)
    with pytest.raises(api.VpbsError, match="16-byte aligned"):
        ctx.key_expand(N, K, ELL, n, mask_seed, host["bsk_bodies"], None, d_bsk=d_b.data_ptr() + 8)
    assert (back(d_b) == MARK).all()
    for d in (dev["d_bsk_bodies"], dev["d_ksk_bodies"], fresh["d_bsk"], fresh["d_ksk"]):
        ctx.device_free(d)


@pytest.mark.parametrize("log_n,K,ELL,LOGB,n", [(3, 2, 4, 5, 6), (6, 3, 3, 7, 40)])
def test_a_slot_from_add_seeded_is_a_slot_from_add(ctx, log_n, K, ELL, LOGB, n):
    N, count = 1 << log_n, 7
    sets = []
    for k in range(2):
        sk = ctx.keygen_seeded(N, K, ELL, LOGB, n, 0x511 + k, 0xAA00 + k, *SIGMAS, *own_secrets(np.random.default_rng(40 + k), n, K, N))
        sk.update(ctx.key_expand(N, K, ELL, n, sk["mask_seed"], sk["bsk_bodies"], sk["ksk_bodies"]))
        sets.append(sk)
    a, b = sets
    ring = api.KeyRing(ctx, K, ELL, LOGB, N, n, max_keys=2, max_batch=count)
    assert ring.add(a["bsk"], a["ksk"]) == 0 and ring.add_seeded(a["mask_seed"], a["bsk_bodies"], a["ksk_bodies"]) == 1 and ring.count() == 2
    tv, delta = api.testv(N, 2)
    rng = np.random.default_rng(log_n)
    cts = api.lwe_encrypt_batch(a["params"], a["s_lwe"], [delta * (i % 2) for i in range(count)], nonce0=3)
    cts[3, 0], cts[3, 1], cts[3, 2] = 0, P - 1, 1 << 63
    per_ct = rng.integers(0, P, size=(count, N), dtype=np.uint64)
    key_of = np.array([0, 1, 1, 0, 1, 0, 0], np.uint32)
    for testv in (tv, per_ct):
        mixed, plain, seeded = (ring.run(cts, ko, testv, accumulators=True) for ko in (key_of, [0] * count, [1] * count))
        for got, want, other in zip(mixed, plain, seeded):
            assert (got == want).all() and (other == want).all()
    # a full ring refuses, and leaves the slot number alone
    slot = C.c_uint(99)
    rc = api.lib().vpbs_keyring_add_seeded(ring.h, b["mask_seed"], b["bsk_bodies"].ctypes.data, b["ksk_bodies"].ctypes.data, 0, C.byref(slot))
    assert rc == INVALID and slot.value == 99
    with pytest.raises(api.VpbsError, match="all 2 slots of the ring are taken"):
        ring.add_seeded(b["mask_seed"], b["bsk_bodies"], b["ksk_bodies"])
    # remove, then add_seeded, reuses the number -- with another key set, from device bodies, and what was expanded before is gone
    ring.remove(0)
    d_bb, d_kb = to_dev(b["bsk_bodies"]), to_dev(b["ksk_bodies"])
    assert ring.add_seeded(b["mask_seed"], d_bb.data_ptr(), d_kb.data_ptr(), bodies_on_device=True) == 0 and ring.count() == 2
    del d_bb, d_kb                                                          # read during the call only
    ref = api.KeyRing(ctx, K, ELL, LOGB, N, n, max_keys=1, max_batch=count)
    assert ref.add(b["bsk"], b["ksk"]) == 0
    cts_b = api.lwe_encrypt_batch(b["params"], b["s_lwe"], [delta * (i % 2) for i in range(count)], nonce0=30)
    for got, want in zip(ring.run(cts_b, [0] * count, tv), ref.run(cts_b, [0] * count, tv)):
        assert (got == want).all()
    ring.remove(1)
    ring.remove(0)
    assert ring.count() == 0 and ring.add_seeded(a["mask_seed"], a["bsk_bodies"], a["ksk_bodies"]) == 0
    with pytest.raises(ValueError, match="key_expand"):
        ring.add_seeded(1, a["bsk_bodies"][:, :-1], a["ksk_bodies"])
    ref.close()
    ring.close()


def test_ring_prover_add_seeded(ctx):
    """the N = 8 world of tests/test_gpu_ring_prover.py: 8 steps per chain, degree 2^13"""
    K, ELL, LOGB, N, n, log_deg = 2, 4, 5, 8, 6, 13
    cyc, dum = [circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, n, log_deg)]
    sk = ctx.keygen_seeded(N, K, ELL, LOGB, n, 77, 0x7007, *SIGMAS, *own_secrets(np.random.default_rng(7), n, K, N))
    full = ctx.key_expand(N, K, ELL, n, sk["mask_seed"], sk["bsk_bodies"], sk["ksk_bodies"])
    tv, delta = api.testv(N, 2)
    cts = api.lwe_encrypt_batch(sk["params"], sk["s_lwe"], [delta, 0], nonce0=10)
    rp = api.RingProver(0, cyc, dum, K, ELL, LOGB, N, n, max_keys=3, chains=2, witness_batch=3)
    try:
        assert rp.add(full["bsk"], full["ksk"]) == 0
        assert rp.add_seeded(sk["mask_seed"], sk["bsk_bodies"], sk["ksk_bodies"]) == 1
        d_bb, d_kb = to_dev(sk["bsk_bodies"]), to_dev(sk["ksk_bodies"])
        assert rp.add_seeded(sk["mask_seed"], d_bb.data_ptr(), d_kb.data_ptr(), bodies_on_device=True) == 2
        want_hash = api.pbs_key_hash(full["bsk"], full["ksk"])
        for slot in range(3):
            assert (rp.key_hash(slot) == want_hash).all(), slot
        # one proof under the seeded slot is, byte for byte, the proof under the slot that add filled
        proofs, out_ct, lwe_out = rp.prove(np.stack([cts[0], cts[0], cts[1], cts[1]]), [0, 1, 0, 2], tv)
        assert proofs[0] == proofs[1] and proofs[2] == proofs[3] and proofs[0] != proofs[2] and len(proofs[0]) > 1000
        assert (out_ct[0] == out_ct[1]).all() and (lwe_out[2] == lwe_out[3]).all()
        # the ring is the prover's: add_seeded on it directly is refused with the message that names the prover's call
        with pytest.raises(api.VpbsError, match="vpbs_ring_prover_add") as e:
            rp.keyring.add_seeded(sk["mask_seed"], sk["bsk_bodies"], sk["ksk_bodies"])
        assert e.value.status == INVALID and rp.keyring.count() == 3
        with pytest.raises(api.VpbsError, match="all 3 slots"):
            rp.add_seeded(sk["mask_seed"], sk["bsk_bodies"], sk["ksk_bodies"])
        rp.remove(1)
        assert rp.add_seeded(sk["mask_seed"], sk["bsk_bodies"], sk["ksk_bodies"]) == 1 and (rp.key_hash(1) == want_hash).all()
    finally:
        rp.close()


@pytest.mark.parametrize("n_lwe", [6, 728])
def test_lwe_expand_on_the_device_is_the_host_form(ctx, n_lwe):
    mask_seed = 0xE7A + n_lwe
    rng = np.random.default_rng(n_lwe)
    for count in (1, 67, 300):
        bodies = rng.integers(0, 1 << 63, size=count, dtype=np.uint64) * np.uint64(2) + np.uint64(1)      # words up to 2^64 - 1: copied unchanged
        nonce0 = (1 << 24) - count if count == 67 else 11 * count
        want = api.lwe_expand_batch(n_lwe, mask_seed, bodies, nonce0=nonce0)
        got = ctx.lwe_expand_batch(n_lwe, mask_seed, bodies, nonce0=nonce0)                               # host bodies, host rows
        assert got.shape == want.shape and (got == want).all(), (count, np.argwhere(got != want)[:4].tolist())
        d_out = dev_full((count + 1, n_lwe + 1), MARK)
        assert ctx.lwe_expand_batch(n_lwe, mask_seed, bodies, nonce0=nonce0, out_dev_ptr=d_out.data_ptr()) is None
        assert (back(d_out)[:count] == want).all() and (back(d_out)[count] == MARK).all()                 # nothing past the last row
        d_out2, d_b = dev_full((count, n_lwe + 1), MARK), to_dev(bodies)
        ctx.lwe_expand_batch(n_lwe, mask_seed, d_b.data_ptr(), nonce0=nonce0, out_dev_ptr=d_out2.data_ptr(), count=count)
        assert (back(d_out2) == want).all()
    # the refusals write nothing
    d_out, d_b = dev_full((3, n_lwe + 1), MARK), to_dev(np.arange(3, dtype=np.uint64))
    with pytest.raises(api.VpbsError, match="ciphertext 1 is the first without a nonce"):
        ctx.lwe_expand_batch(n_lwe, mask_seed, d_b.data_ptr(), nonce0=(1 << 24) - 1, out_dev_ptr=d_out.data_ptr(), count=3)
    with pytest.raises(api.VpbsError, match="n_lwe"):
        ctx.lwe_expand_batch(1 << 24, mask_seed, d_b.data_ptr(), out_dev_ptr=d_out.data_ptr(), count=3)
    L = api.lib()
    assert L.vpbs_lwe_expand_batch(ctx.h, n_lwe, mask_seed, 0, None, 3, d_out.data_ptr(), 1) == INVALID
    assert L.vpbs_lwe_expand_batch(ctx.h, n_lwe, mask_seed, 0, d_b.data_ptr(), 3, None, 1) == INVALID and b"null pointer" in L.vpbs_last_error(ctx.h)
    assert (back(d_out) == MARK).all()
    assert (ctx.lwe_expand_batch(n_lwe, mask_seed, [5]) == api.lwe_expand_batch(n_lwe, mask_seed, [5])).all()   # the context stays usable


@pytest.mark.parametrize("n_lwe", [6, 65, 728])
def test_seeded_encryption_on_the_device_is_the_host_form(ctx, n_lwe):
    seed, mask_seed = 0xABCD00 + n_lwe, 0x1234 + n_lwe
    prm = api.KeygenParamsC(10, 2, 4, 5, n_lwe, seed, *SIGMAS)
    rng = np.random.default_rng(2000 + n_lwe)
    s = rng.integers(0, 2, size=n_lwe, dtype=np.uint64)
    s[n_lwe - 1] = np.uint64(P + 2)                                          # a key word at or above p, as the unseeded call takes it
    d_s = to_dev(s)
    delta = T.get_delta(4)
    for count in (1, 2, 257):
        msgs = rng.integers(0, 4, size=count, dtype=np.uint64) * np.uint64(delta)
        msgs[:2] = np.array([P - 1, 0], np.uint64)[:count]
        nonce0 = (1 << 24) - count if count == 2 else 7 * count
        want = api.lwe_encrypt_seeded_batch(prm, mask_seed, s, msgs, nonce0=nonce0)
        got = ctx.lwe_encrypt_seeded_batch(prm, mask_seed, s, msgs, nonce0=nonce0)                        # host key, host bodies
        assert got.shape == (count,) and (got == want).all(), (count, np.argwhere(got != want)[:4].tolist())
        assert (ctx.lwe_encrypt_seeded_batch(prm, mask_seed, d_s.data_ptr(), msgs, nonce0=nonce0) == want).all()   # device key, host bodies
        d_out = dev_full((count + 1,), MARK)
        assert ctx.lwe_encrypt_seeded_batch(prm, mask_seed, d_s.data_ptr(), msgs, nonce0=nonce0, out_dev_ptr=d_out.data_ptr()) is None
        assert (back(d_out)[:count] == want).all() and back(d_out)[count] == MARK                         # device key, device bodies
        d_out2, d_m = dev_full((count,), MARK), to_dev(msgs)
        ctx.lwe_encrypt_seeded_batch(prm, mask_seed, s, d_m.data_ptr(), nonce0=nonce0, out_dev_ptr=d_out2.data_ptr(), count=count)   # host key
        assert (back(d_out2) == want).all()
    # with one seed the expanded rows are lwe_encrypt_batch's
    msgs = rng.integers(0, P, size=67, dtype=np.uint64)
    d_rows = dev_full((67, n_lwe + 1))
    d_bodies = dev_full((67,))
    ctx.lwe_encrypt_seeded_batch(prm, seed, d_s.data_ptr(), msgs, nonce0=5, out_dev_ptr=d_bodies.data_ptr())
    ctx.lwe_expand_batch(n_lwe, seed, d_bodies.data_ptr(), nonce0=5, out_dev_ptr=d_rows.data_ptr(), count=67)
    assert (back(d_rows) == api.lwe_encrypt_batch(prm, s, msgs, nonce0=5)).all()
    # refusals, as lwe_encrypt_batch's
    bad = np.array([0, 1, 2, P, 4, P + 1], np.uint64)
    with pytest.raises(api.VpbsError, match="message 3 is not below p"):
        ctx.lwe_encrypt_seeded_batch(prm, mask_seed, s, bad)
    d_out, d_m = dev_full((6,), MARK), to_dev(bad)
    with pytest.raises(api.VpbsError, match="message 3 is not below p"):                                   # found by the kernel
        ctx.lwe_encrypt_seeded_batch(prm, mask_seed, s, d_m.data_ptr(), out_dev_ptr=d_out.data_ptr(), count=6)
    with pytest.raises(api.VpbsError, match="ciphertext 1 is the first without a nonce"):
        ctx.lwe_encrypt_seeded_batch(prm, mask_seed, s, bad[:3], nonce0=(1 << 24) - 1)


def test_end_to_end_at_the_papers_parameters(ctx):
    """own secrets, mask_seed != seed, the bodies born on the device and expanded into a ring slot; eight messages encrypted seeded (8 bytes
    each), expanded on the device, bootstrapped with KeyRing.run_device and decoded: no failure"""
    N, K, ELL, LOGB, n, p = 1024, 2, 4, 5, 728, 2
    seed, mask_seed = 0x5EED, 0x9A9E2
    s_lwe, s_glwe = own_secrets(np.random.default_rng(2024), n, K, N)
    sk = ctx.keygen_seeded(N, K, ELL, LOGB, n, seed, mask_seed, *SIGMAS, s_lwe=s_lwe, s_glwe=s_glwe, on_device=True)
    assert api.seeded_key_shapes(N, K, ELL, n) == (sk["params"].n_lwe * K * ELL * N + K * ELL * N, 729 * K * ELL * K * N)
    ring = api.KeyRing(ctx, K, ELL, LOGB, N, n, max_keys=1, max_batch=8)
    assert ring.add_seeded(mask_seed, sk["d_bsk_bodies"], sk["d_ksk_bodies"], bodies_on_device=True) == 0
    for d in (sk["d_bsk_bodies"], sk["d_ksk_bodies"]):
        ctx.device_free(d)
    tv, delta = api.testv(N, p)
    msgs = [0, 1, 1, 0, 1, 0, 0, 1]
    bodies = ctx.lwe_encrypt_seeded_batch(sk["params"], mask_seed, s_lwe, [delta * m % P for m in msgs], nonce0=100)
    assert bodies.nbytes == 8 * 8
    d_cts, d_lwe, d_tv = dev_full((8, n + 1)), dev_full((8, n + 1)), to_dev(tv)
    ctx.lwe_expand_batch(n, mask_seed, bodies, nonce0=100, out_dev_ptr=d_cts.data_ptr())
    ring.run_device(d_cts.data_ptr(), 8, [0] * 8, d_tv.data_ptr(), d_lwe_out=d_lwe.data_ptr())
    st = api.NoiseStats()
    got = ctx.lwe_decode_batch(s_lwe, d_lwe.data_ptr(), delta, 2 * p, expected=msgs, count=8, stats=st, want=("msg",))
    assert st.count == 8 and st.failures == 0 and got["msg"].tolist() == msgs and 0 < st.max_abs < delta // 2
    # the inputs decode too: the rows are honest ciphertexts under the caller's own key
    assert ctx.lwe_decode_batch(s_lwe, d_cts.data_ptr(), delta, 2 * p, count=8)["msg"].tolist() == msgs
    ring.close()
