"""CPU restatement of what closes the bootstrapping loop (TEST INFRASTRUCTURE): sample extraction and LWE decryption.

What it follows in the reference (/root/reference/src/vtfhe/crypto/):
  * Glwe::sample_extract / partial_sample_extract   glwe.rs:96-113
  * Glwe::partial_key / flatten_partial_key         glwe.rs:19-38, :145-147
  * lwe::decrypt                                     lwe.rs:62-69
  * the rounding of a decrypted message              /root/reference/src/main.rs:59-64
Pure Python integers; tfhe_oracle.py is imported as it is for everything else."""
import numpy as np

P = 0xFFFFFFFF00000001


def sample_extract(ct):
    """ct: K polynomials -> [a_0[0], -a_0[N-1], .., -a_0[1], a_1[0], .., body[0]]"""
    a = []
    for poly in ct[:-1]:
        a.append(int(poly[0]))
        a += [(P - int(c)) % P for c in list(poly[1:])[::-1]]
    a.append(int(ct[-1][0]))
    return a


def extract(ct, n_lwe):
    """partial_sample_extract(n_lwe): the first n_lwe mask words of the full sample, then the body"""
    full = sample_extract(ct)
    assert n_lwe <= len(full) - 1
    return full[:n_lwe] + [full[-1]]


def lwe_decrypt(s, ct):
    """body - <s, mask>"""
    s, ct = [int(v) for v in s], [int(v) for v in ct]
    assert len(ct) == len(s) + 1
    return (ct[-1] - sum(a * b for a, b in zip(s, ct[:-1]))) % P


def partial_key(rng, n, K, n_lwe):
    """K polynomials, binary, only the leading n_lwe coefficients (in flattened order) non-zero"""
    flat = [int(v) for v in rng.integers(0, 2, size=n_lwe)] + [0] * (K * n - n_lwe)
    return [flat[j * n:(j + 1) * n] for j in range(K)]


def flatten_partial_key(s_to, n_lwe):
    return [int(c) for poly in s_to for c in poly][:n_lwe]


def round_message(m_bar, delta, p):
    """main.rs:59-64, as tests/test_gpu_parity.py::test_seeded_pbs_decrypts_to_the_message rounds"""
    return round(int(m_bar) / delta) % (2 * p)


def glwe_list(a):
    """numpy [K][N] -> lists of Python integers"""
    return [[int(v) for v in poly] for poly in np.asarray(a)]
