"""The split generator of the seeded calls (csrc/keygen_streams.h), built from tfhe_oracle's primitives: the streams of kind BSK_MASK,
KSK_MASK and LWE_MASK are keyed by mask_seed, every other kind by seed.  `Split` has `Seeded`'s interface, so tfhe_oracle's
seeded_glwe_encrypt and seeded_ggsw_hat take it unchanged; split_pbs_keys is seeded_pbs_keys with it, and with given secrets."""
import numpy as np

import tfhe_oracle as T

P = T.P
MASK_KINDS = (T.BSK_MASK, T.KSK_MASK, T.LWE_MASK)


class Split:
    def __init__(self, seed, mask_seed):
        self.private, self.public = T.Seeded(seed), T.Seeded(mask_seed)

    def stream(self, kind, a=0, b=0, c=0):
        return (self.public if kind in MASK_KINDS else self.private).stream(kind, a, b, c)

    draw = staticmethod(T.Seeded.draw)

    def field(self, key, i):
        return self.private.field(key, i)     # a function of the stream key alone

    def bit(self, key, i):
        return self.private.bit(key, i)

    def noise(self, key, i, m_sigma):
        return self.private.noise(key, i, m_sigma)


def partial_key(ring, s_lwe, K):
    """Glwe::partial_key's layout of a given LWE key: s_to[x // N][x % N] = s_lwe[x], zeros elsewhere"""
    s_to = [[0] * ring.n for _ in range(K)]
    for x, v in enumerate(s_lwe):
        s_to[x // ring.n][x % ring.n] = int(v)
    return s_to


def split_pbs_keys(ring, seed, mask_seed, n_lwe, K, ELL, logb, sigma_glwe=0.0, sigma_lwe=0.0, bsk_indices=None, secrets=None):
    """tfhe_oracle.seeded_pbs_keys under the split generator; secrets = (s_lwe [n], s_glwe [K-1][N]) are the caller's own, None: the seed's
    -> s_to, s_lwe, s_glwe, {i: bsk[i]} for the requested indices (all when None), ksk"""
    g = Split(seed, mask_seed)
    if secrets is None:
        s_to, s_lwe, s_glwe = T.seeded_keys(ring, seed, n_lwe, K)
    else:
        s_lwe, s_glwe = [int(v) for v in secrets[0]], [[int(v) for v in p] for p in secrets[1]]
        s_to = partial_key(ring, s_lwe, K)
    one = [1] + [0] * (ring.n - 1)
    msgs = [list(s_glwe[p]) for p in range(K - 1)] + [one]
    idx = range(n_lwe) if bsk_indices is None else bsk_indices
    bsk = {i: T.seeded_ggsw_hat(ring, g, s_glwe, msgs, s_lwe[i], K, ELL, logb, T.BSK_MASK, T.BSK_NOISE, i, T.sigma_to_int(sigma_glwe)) for i in idx}
    ksk = T.seeded_ggsw_hat(ring, g, s_to, msgs, 1, K, ELL, logb, T.KSK_MASK, T.KSK_NOISE, 0, T.sigma_to_int(sigma_lwe))
    return s_to, s_lwe, s_glwe, bsk, ksk


def bodies_of(ggsw_flat, K, ELL, N):
    """the last polynomial of every GLWE of flattened GGSWs [..][K*ELL*K*N] -> [..][K*ELL*N]"""
    g = np.asarray(ggsw_flat, np.uint64)
    return np.ascontiguousarray(g.reshape(g.shape[:-1] + (K * ELL, K, N))[..., K - 1, :]).reshape(g.shape[:-1] + (K * ELL * N,))


def split_lwe_encrypt(seed, mask_seed, s_lwe, message, sigma_lwe, nonce=0):
    """tfhe_oracle.seeded_lwe_encrypt under the split generator -> the n + 1 words of the ciphertext"""
    g = Split(seed, mask_seed)
    km, ke = g.stream(T.LWE_MASK, nonce), g.stream(T.LWE_NOISE, nonce)
    mask = [g.field(km, i) for i in range(len(s_lwe))]
    body = (sum(a * int(b) for a, b in zip(mask, s_lwe)) + message + g.noise(ke, 0, T.sigma_to_int(sigma_lwe))) % P
    return mask + [body]
