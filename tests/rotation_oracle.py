"""Restatement of the rotation margins (TEST INFRASTRUCTURE; the checker of vpbs_lwe_rotation_batch) in Python integers, over
tests/tfhe_oracle.py (mod_switch, get_delta): the definitions of csrc/rotation.h written down a second time, with nothing shared with the
product.  The snap is restated here as well; nothing in this file calls vpbs_lwe_rotation_batch, vpbs_lwe_snap or api.lut_expect."""
import numpy as np

import lwe_client_oracle as LC
import tfhe_oracle as T

P = T.P


def snap(w, log_n, theta):
    """the reduced word, rounded to a multiple of 2^t, t = 64 - (log_n + 1) + theta; the quotient 2^(64 - t) wraps to 0"""
    w = int(w) % P
    if theta == 0:
        return w
    t = 64 - (log_n + 1) + theta
    r = (w >> t) + ((w >> (t - 1)) & 1)
    return (r << t) % (1 << 64)


def rotation(s, ct, log_n, theta=0):
    """mu = (2N - R) mod 2N, R the sum of step 0's rotation ms(-w_n) and of ms(w_i) over the key bits that are 1"""
    s = [int(v) % P for v in s]
    assert len(ct) == len(s) + 1 and all(v in (0, 1) for v in s)
    w = [snap(v, log_n, theta) for v in ct]
    two_n = 2 << log_n
    r = T.mod_switch((P - w[-1]) % P, log_n) + sum(T.mod_switch(w[i], log_n) for i in range(len(s)) if s[i])
    return (two_n - r % two_n) % two_n


def expect(testv, mu, j=0):
    """E(mu + j): testv[x] for x < N, its negation at x - N otherwise; indices mod 2N"""
    n = len(testv)
    x = (int(mu) + j) % (2 * n)
    return int(testv[x]) % P if x < n else (P - int(testv[x - n])) % P


def margin(mu, log_n, p, expected=None):
    """-> (idx, dev, failed); dev centred into [-N, N)"""
    n = 1 << log_n
    block = n // p
    idx = ((mu + block // 2) // block) % (2 * p)
    ref = idx if expected is None else int(expected) % (2 * p)
    dev = (mu - ref * block) % (2 * n)
    if dev >= n:
        dev -= 2 * n
    return idx, dev, expected is not None and idx != ref


def rotation_batch(s, cts, log_n, p, theta=0, expected=None, stats=None):
    """-> (mus, idxs, devs) as lists of Python integers; stats (an lwe_client_oracle.Stats) is added to, err := dev"""
    mus, idxs, devs = [], [], []
    for i, ct in enumerate(cts):
        mu = rotation(s, ct, log_n, theta)
        idx, dev, failed = margin(mu, log_n, p, None if expected is None else expected[i])
        mus.append(mu)
        idxs.append(idx)
        devs.append(dev)
        if stats is not None:
            stats.add(dev, failed)
    return mus, idxs, devs


Stats = LC.Stats


def edge_words(log_n, theta):
    """words that reach the corners of the definition: 0, 1, p - 1, p, 2^64 - 1 (the last two reduced on read); a word whose rounding bit
    carries ms to 2N; words that snap to r = 2^(L - theta) and wrap to 0, and the last one that does not; half-way points of both roundings"""
    L = log_n + 1
    out = [0, 1, P - 1, P, (1 << 64) - 1, 1 << 63, (1 << 63) - 1]
    out += [P - 1 - ((1 << (64 - L - 1)) - 1), (((2 << log_n) - 1) << (64 - L)) | (1 << (64 - L - 1))]      # ms = 2N below p, if any
    out += [1 << (64 - L - 1), (1 << (64 - L - 1)) - 1, 3 << (64 - L - 1)]                                     # ms half-way points
    if theta:
        t = 64 - L + theta
        top = ((1 << (64 - t)) - 1) << t                                                                      # the last multiple of 2^t
        out += [top | (1 << (t - 1)), (top | (1 << (t - 1))) - 1, top, 1 << (t - 1), (1 << (t - 1)) - 1, 3 << (t - 1)]
    return [v % (1 << 64) for v in out]


def edge_rows(log_n, n, theta, seed):
    """rows whose words walk through the edge words (every edge word meets every position class), random rows, a zero body, a zero row"""
    edge = edge_words(log_n, theta)
    rng = np.random.default_rng(seed)
    rows = np.array([[edge[(r + 3 * i) % len(edge)] for i in range(n + 1)] for r in range(len(edge))], np.uint64)
    rand = rng.integers(0, 1 << 64, size=(6, n + 1), dtype=np.uint64)
    rand[0, n] = 0                                               # a zero body
    rand[1, :] = 0
    return np.concatenate([rows, rand])


def keys(n, seed):
    rng = np.random.default_rng(seed)
    mixed = rng.integers(0, 2, size=n, dtype=np.uint64)
    mixed[0] = np.uint64(P + 1)                                  # 1 after reduction
    return [np.zeros(n, np.uint64), np.ones(n, np.uint64), mixed]


def contract_rows(rng, s_lwe, log_n, p):
    """noise-free ciphertexts whose phases step in quarter positions across every block edge: (q block - h) 2^(64 - L) + k 2^(64 - L - 2),
    q in 0 .. 2p, k in -12 .. 12"""
    L, block = log_n + 1, (1 << log_n) // p
    words = [((q * block - block // 2) * (1 << (64 - L)) + k * (1 << (64 - L - 2))) % P for q in range(2 * p + 1) for k in range(-12, 13)]
    return words, np.array([T.lwe_encrypt(rng, s_lwe, w) for w in words], np.uint64)
