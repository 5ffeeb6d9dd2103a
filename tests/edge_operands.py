"""Edge operands for the GPU parity tests (TEST INFRASTRUCTURE, not a conftest).

The kernels compute on u64 residues and canonicalise only where they store.  Every canonical value below 2^32 - 1 has a
second 64-bit alias in [p, 2^64), so a store that misses its canonicalisation, or a wrong wrap correction, shows up only
when a result or an intermediate lands on one of the values below -- for uniformly random operands about once in 2^32.
The helpers here put the edges where the arithmetic lands while every value handed to the ABI stays canonical
(include/vpbs_prover.h): chosen outputs with derived inputs, polynomials whose evaluations are edge values everywhere, and
chosen challenges.  Pure Python big-int arithmetic, plus the C oracle's transforms (pinned to a naive DFT in
tests/test_oracle_cpu.py).
"""
import numpy as np

import oracle as orc

P = 0xFFFFFFFF00000001
W = 7   # GF(p^2) = GF(p)[X] / (X^2 - 7)

# the edge set E
E = [0, 1, 2, P - 1, P - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, P - (1 << 32), (P - 1) // 2, (P + 1) // 2]
# the 8th roots of unity: +-1, +-2^48 (order 4), +-2^24 and +-2^72 = +-2^24 * 2^48 (order 8)
ROOTS = [1, P - 1, 1 << 48, P - (1 << 48), 1 << 24, P - (1 << 24), pow(2, 72, P), P - pow(2, 72, P)]
E_ROOTS = E + [r for r in ROOTS if r not in E]

# extension points for the openings: 1, -1, the generator X of GF(p^2), 2^32, (p-1)(1 + X)
ZETAS = [(1, 0), (P - 1, 0), (0, 1), (1 << 32, 0), (P - 1, P - 1)]


def pattern(n, offset=0, stride=1, values=E_ROOTS):
    """[n] uint64: values[(offset + stride * i) % len(values)]"""
    idx = (offset + stride * np.arange(n, dtype=np.int64)) % len(values)
    return np.array(values, dtype=np.uint64)[idx]


def patterns(ncols, n, values=E_ROOTS):
    """[ncols][n] uint64: a different walk through `values` per column (strides coprime to 13 and 17)"""
    return np.stack([pattern(n, 3 * c, (1, 5, 2, 7, 3)[c % 5], values) for c in range(ncols)])


def constant_columns(ncols, n, offset=0, values=E):
    """[ncols][n] uint64: column c is the constant values[(offset + c) % len(values)]"""
    v = np.array(values, dtype=np.uint64)[(offset + np.arange(ncols)) % len(values)]
    return np.ascontiguousarray(np.repeat(v[:, None], n, axis=1))


def values_for_coeffs(coeffs):
    """values on the subgroup H whose inverse transform is exactly `coeffs` ([ncols][n])"""
    return np.stack([orc.fft(c) for c in np.atleast_2d(coeffs)])


def root_of_unity(log_n):
    return int(orc.lib().orc_gl_root_of_unity(log_n))


def bitrev_index(log_n):
    """idx[j] = bit reversal of j on log_n bits (leaf order of an LDE: leaf[j] = natural[idx[j]])"""
    j = np.arange(1 << log_n, dtype=np.int64)
    r = np.zeros_like(j)
    for b in range(log_n):
        r |= ((j >> b) & 1) << (log_n - 1 - b)
    return r


def monomial_lde(log_n, rate_bits, shift, k):
    """natural-order coset LDE of x^k (degree < 2^log_n) in closed form: (shift * g^j)^k, g of order 2^(log_n + rate_bits)"""
    assert 0 <= k < 1 << log_n
    log_big = log_n + rate_bits
    step = pow(root_of_unity(log_big), k, P)
    out = np.zeros(1 << log_big, np.uint64)
    v = pow(shift, k, P)
    for j in range(1 << log_big):
        out[j] = v
        v = v * step % P
    return out


def monomial(n, k):
    c = np.zeros(n, np.uint64)
    c[k] = 1
    return c


# ---- GF(p^2) ----
def ext_horner(coeffs, zeta):
    """sum_i coeffs[i] zeta^i in GF(p^2), big-int Horner"""
    z0, z1 = int(zeta[0]), int(zeta[1])
    a0 = a1 = 0
    for v in reversed([int(x) for x in coeffs]):
        a0, a1 = (a0 * z0 + W * a1 * z1 + v) % P, (a0 * z1 + a1 * z0) % P
    return a0, a1


def opening_columns(n):
    """[ncols][n] coefficient columns for the openings: E walks, and columns whose value is 0 at zeta = 1 or at zeta = -1, with the
    cancelling terms on either side of every 256- and 4096-coefficient boundary of the partial sums"""
    cols = [pattern(n, 0, 1), pattern(n, 4, 7)]
    c = np.zeros(n, np.uint64)
    if n > 1:
        c[0], c[1] = 1, P - 1                           # [1, p-1, 0, ...]: 0 at zeta = 1
    cols.append(c)
    c = np.zeros(n, np.uint64)                          # a, -a around every block boundary: 0 at zeta = 1
    for b in range(256, n, 256):
        v = E[b // 256 % len(E)]
        c[b - 1], c[b] = v, (P - v) % P
    if n == 1:
        c[0] = 0
    cols.append(c)
    cols.append(np.full(n, P - 1, np.uint64))           # sum = -n
    cols.append(np.ones(n, np.uint64) if n > 1 else np.zeros(n, np.uint64))   # 0 at zeta = -1 (n even)
    return np.ascontiguousarray(np.stack(cols))


# ---- permutation argument ----
def k_is(n_routed):
    return [pow(W, j, P) for j in range(n_routed)]


def denominators_nonzero(wires, sigmas, betas, gammas):
    """True when no denominator w + beta sigma + gamma of the partial products is 0 (that case is an error test of its own)"""
    return not _bad_denominators(wires, sigmas, betas, gammas).any()


def _bad_denominators(wires, sigmas, betas, gammas):
    w, sg = wires.astype(object), sigmas.astype(object)
    bad = np.zeros(sigmas.shape, bool)
    for b, g in zip(betas, gammas):
        bad |= (w + int(b) * sg + int(g)) % P == 0
    return bad


def avoid_zero_denominators(wires, sigmas, betas, gammas, values=E):
    """replace each sigma whose denominator vanishes for some challenge by the next value of `values` that does not"""
    sig = sigmas.copy()
    for j, i in np.argwhere(_bad_denominators(wires, sig, betas, gammas)):
        t = values.index(int(sig[j, i])) if int(sig[j, i]) in values else 0
        while any((int(wires[j, i]) + int(b) * int(sig[j, i]) + int(g)) % P == 0 for b, g in zip(betas, gammas)):
            t += 1
            sig[j, i] = values[t % len(values)]
    assert denominators_nonzero(wires, sig, betas, gammas)
    return sig


def wires_for_ratio_minus_one(sigmas, beta, gamma):
    """wires that make every ratio (w + beta k_j x + gamma) / (w + beta sigma + gamma) equal p - 1: w = -(beta k_j x + beta sigma + 2 gamma) / 2"""
    n_routed, n = sigmas.shape
    log_n = n.bit_length() - 1
    g = root_of_unity(log_n)
    xs, x = [], 1
    for _ in range(n):
        xs.append(x)
        x = x * g % P
    kx = np.array(k_is(n_routed), dtype=object)[:, None] * np.array(xs, dtype=object)[None, :]
    w = (-(beta * kx + beta * sigmas.astype(object) + 2 * gamma)) * ((P + 1) // 2) % P
    return w.astype(np.uint64)


def partial_products_model(wires, sigmas, betas, gammas, max_degree=8):
    """plonk/prover.rs wires_permutation_partial_products_and_zs by big-int arithmetic: [nc * chunks][n], the Z columns first, then the
    chunks - 1 partial products of each challenge"""
    n_routed, n = sigmas.shape
    nc = len(betas)
    chunks = (n_routed + max_degree - 1) // max_degree
    g = root_of_unity(n.bit_length() - 1)
    ks = k_is(n_routed)
    out = np.zeros((nc * chunks, n), np.uint64)
    for c, (beta, gamma) in enumerate(zip(betas, gammas)):
        z = 1
        for i in range(n):
            x = pow(g, i, P)
            out[c, i] = z
            run = z
            for k in range(chunks):
                for j in range(max_degree * k, min(max_degree * k + max_degree, n_routed)):
                    w = int(wires[j, i])
                    den = (w + beta * int(sigmas[j, i]) + gamma) % P
                    assert den != 0
                    run = run * (w + beta * ks[j] * x + gamma) % P * pow(den, P - 2, P) % P
                if k < chunks - 1:
                    out[nc + c * (chunks - 1) + k, i] = run
            z = run
    return out


# ---- TFHE ----
def mask_boundaries(log_N):
    """masks on the mod-switch boundaries (tfhe.hip mod_switch: the top log_N + 1 bits, rounded with bit 62 - log_N): 0, p - 1 (shift 2N),
    and every multiple k 2^(62 - log_N) exactly and +-1 -- the rounding ties at odd k (the shift steps up between tie - 1 and tie), the
    truncation boundaries of the top bits at even k"""
    out = [0, P - 1]
    step = 1 << (62 - log_N)
    for k in range(1, P // step + 1):
        for d in (-1, 0, 1):
            v = k * step + d
            if 0 <= v < P:
                out.append(v)
    return out


def decomposition_boundaries(logb):
    """accumulator coefficients on the digit boundaries of a base-2^logb decomposition: 0, 1, p-1, 2^63 - 1, 2^63, carries that ripple through
    every digit (sum (B/2) B^l and sum (B/2 - 1) B^l over as many digits as stay below p), and p - 1 - x of each of those"""
    B = 1 << logb
    half, below = 0, 0
    for l in range(-(-64 // logb)):
        if half + (B // 2) * B ** l < P:
            half += (B // 2) * B ** l
        if below + (B // 2 - 1) * B ** l < P:
            below += (B // 2 - 1) * B ** l
    base = [0, 1, P - 1, (1 << 63) - 1, 1 << 63, half, below]
    return list(dict.fromkeys(base + [P - 1 - x for x in base]))


def acc_for_difference(target, shift):
    """the polynomial a with a X^shift - a = target modulo X^N + 1 (what a normal CMUX step decomposes), or None when X^shift = 1
    (shift 0 or 2N: the difference is 0 whatever a is); Gauss-Jordan elimination modulo p"""
    n = len(target)
    if shift % (2 * n) == 0:
        return None
    m = [[0] * n + [int(t)] for t in target]
    for i in range(n):   # column i of (rotation by shift) - identity
        j = i + shift
        m[j % n][i] = (P - 1) if (j // n) & 1 else 1
        m[i][i] = (m[i][i] - 1) % P
    for c in range(n):
        piv = next(r for r in range(c, n) if m[r][c])
        m[c], m[piv] = m[piv], m[c]
        inv = pow(m[c][c], P - 2, P)
        m[c] = [v * inv % P for v in m[c]]
        for r in range(n):
            if r != c and m[r][c]:
                f = m[r][c]
                m[r] = [(a - f * b) % P for a, b in zip(m[r], m[c])]
    return [m[r][n] for r in range(n)]


# ---- device witness ----
def legal_preset(gate, wire, v):
    """the free input `wire` of a `gate` row set to `v` where the gate's generators accept any field element, else the largest legal value
    (a BaseSum sum below B^limbs, a RandomAccess index below the vector length, the Poseidon swap and the exponent bits in {0, 1}, a non-zero
    CosetInterpolation shift)"""
    k, p0, p1 = gate.kind, gate.p0, gate.p1
    if k == "base_sum" and wire == 0:
        return min(v, min(P, p1 ** p0) - 1)
    if k == "random_access" and wire % (2 + (1 << p0)) == 0 and wire < (2 + (1 << p0)) * p1:
        return min(v, (1 << p0) - 1)
    if (k == "poseidon" and wire == 24) or (k == "exponentiation" and 1 <= wire <= p0):
        return min(v, 1)
    if k == "coset_interpolation" and wire == 0:
        return v or P - 1
    return v


# (n_routed, log_n, max_degree, num_challenges, kind): (80, 8) runs the one-kernel path with its shared inversion, any other shape the
# three-kernel path; 17 routed wires at degree 8 leave a ragged last chunk of one
PP_KINDS = ("beta0", "beta_minus1", "ratio_minus1", "edge")
PP_CASES = [(17, 3, 8, nc, kind) for kind in PP_KINDS for nc in (1, 2)] + [(80, 4, 8, 2, kind) for kind in PP_KINDS] + \
           [(10, 4, 4, 3, "edge"), (80, 16, 8, 2, "beta_minus1"), (80, 16, 8, 2, "ratio_minus1")]


def pp_case(n_routed, log_n, nc, kind):
    """-> wires, sigmas, betas, gammas of a partial-products case, every denominator non-zero (asserted)"""
    n = 1 << log_n
    wires, sig = patterns(n_routed, n), patterns(n_routed + 3, n)[3:].copy()
    if kind == "beta0":          # every ratio is 1: Z and every partial product are exactly 1
        betas, gammas = [0] * nc, [3, (1 << 32) + 2, P - 3, 5][:nc]
    elif kind == "beta_minus1":
        betas, gammas = [P - 1, 1 << 63, (P + 1) // 2, 1][:nc], [1, P - 1, 0, (1 << 32) - 1][:nc]
    elif kind == "ratio_minus1":   # every ratio is p - 1
        betas, gammas = [P - 1] * nc, [1] * nc
        g = root_of_unity(log_n)
        kx = np.array(k_is(n_routed), dtype=object)[:, None] * np.array([pow(g, i, P) for i in range(n)], dtype=object)[None, :] % P
        for j, i in np.argwhere(sig.astype(object) == kx):   # sigma = k_j x would make numerator and denominator 0
            sig[j, i] = E[(E.index(int(sig[j, i])) + 1) % len(E)] if int(sig[j, i]) in E else 2
        wires = wires_for_ratio_minus_one(sig, betas[0], gammas[0])
    else:
        betas, gammas = [E[(3 + 4 * c) % len(E)] for c in range(nc)], [E[(7 + 5 * c) % len(E)] for c in range(nc)]
    sig = avoid_zero_denominators(wires, sig, betas, gammas)
    return wires, sig, betas, gammas
