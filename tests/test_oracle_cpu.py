"""CPU tests (-m "not gpu"): pin the oracle against the golden vectors and small big-int models."""
import glob
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import fri_shapes
import oracle as orc
import pymodel
from pymodel import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
rng = np.random.default_rng(1234)


def rand_field(*shape):
    return (rng.integers(0, P, size=shape, dtype=np.uint64, endpoint=False)).astype(np.uint64)


def test_field_ops_match_bigint():
    L = orc.lib()
    edge = [0, 1, 2, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000, 1 << 63]
    vals = edge + [int(x) for x in rand_field(40)]
    for a in vals:
        for b in vals[:12]:
            assert L.orc_gl_add(a, b) == (a + b) % P
            assert L.orc_gl_sub(a, b) == (a - b) % P
            assert L.orc_gl_mul(a, b) == (a * b) % P
        if a:
            assert L.orc_gl_mul(a, L.orc_gl_inv(a)) == 1
    assert L.orc_gl_exp(7, (P - 1) >> 32) == 1753635133440165772  # POWER_OF_TWO_GENERATOR
    assert L.orc_gl_root_of_unity(3) == pow(2, 24, P) * (P - 1) % P or L.orc_gl_exp(L.orc_gl_root_of_unity(3), 8) == 1
    assert L.orc_gl_exp(2, 96) == P - 1 and L.orc_gl_exp(2, 48) ** 2 % P == P - 1


def test_ext_field():
    L = orc.lib()
    for _ in range(20):
        a, b = rand_field(2), rand_field(2)
        out = np.zeros(2, np.uint64)
        L.orc_ext_mul(orc.ptr(a), orc.ptr(b), orc.ptr(out))
        assert tuple(int(x) for x in out) == pymodel.ext_mul([int(x) for x in a], [int(x) for x in b])
        inv = np.zeros(2, np.uint64)
        L.orc_ext_inv(orc.ptr(a), orc.ptr(inv))
        L.orc_ext_mul(orc.ptr(a), orc.ptr(inv), orc.ptr(out))
        assert list(out) == [1, 0]
    # EXT_POWER_OF_TWO_GENERATOR^2 == base POWER_OF_TWO_GENERATOR (same FFT subgroups in GF(p) and GF(p^2))
    g = np.array([0, 15659105665374529263], np.uint64); out = np.zeros(2, np.uint64)
    L.orc_ext_mul(orc.ptr(g), orc.ptr(g), orc.ptr(out))
    assert list(out) == [1753635133440165772, 0]


def test_poseidon_constants_and_kats():
    kat = json.load(open(os.path.join(GOLD, "poseidon_kat.json")))
    rc = pymodel.round_constants()
    assert hashlib.sha256(struct.pack("<360Q", *rc)).hexdigest() == kat["constants_sha256"]
    for k in kat["kats"]:
        assert [int(x) for x in orc.poseidon(k["input"])] == k["output"], k["name"]
    # first output words quoted in SURVEY.md 8c (upstream plonky2 test vectors)
    assert kat["kats"][0]["output"][0] == 0x3c18a9786cb0b359
    assert kat["kats"][1]["output"][0] == 0xd64e1e3efc5b8e9e
    assert kat["kats"][2]["output"][0] == 0xbe0085cfc57a8357


def test_poseidon_random_vs_bigint_and_batch():
    states = rand_field(6, 12)
    for s in states:
        assert [int(x) for x in orc.poseidon(s)] == pymodel.poseidon(s)
    b = states.copy()
    orc.lib().orc_poseidon_batch(orc.ptr(b), 6)
    for i in range(6):
        assert list(b[i]) == list(orc.poseidon(states[i]))


@pytest.mark.parametrize("n", [0, 1, 4, 5, 8, 9, 16, 17, 135])
def test_sponge_modes(n):
    x = rand_field(n)
    if n:
        assert [int(v) for v in orc.hash_no_pad(x)] == pymodel.hash_no_pad(x)
    noop = orc.hash_or_noop(x)
    if n <= 4:  # hash_or_noop: short leaves are zero-padded, not hashed
        assert list(noop) == list(x) + [0] * (4 - n)
    else:
        assert list(noop) == list(orc.hash_no_pad(x))


def test_two_to_one_and_chain():
    l, r = rand_field(4), rand_field(4)
    s = pymodel.poseidon([int(v) for v in l] + [int(v) for v in r] + [0] * 4)
    assert [int(v) for v in orc.two_to_one(l, r)] == s[:4]
    # verify_hash_output chain (reference ivc_based_vpbs.rs:64-78)
    data = rand_field(3, 5)
    out = np.zeros(4, np.uint64)
    orc.lib().orc_hash_chain(orc.ptr(data), 3, 5, orc.ptr(out))
    h = [0] * 4
    for row in data:
        h = pymodel.hash_no_pad(h + [int(v) for v in row])
    assert [int(v) for v in out] == h


@pytest.mark.parametrize("log_n", [1, 2, 3, 5])
def test_fft_matches_naive_dft(log_n):
    n = 1 << log_n
    c = rand_field(n)
    w = pymodel.root_of_unity(log_n)
    naive = [sum(int(c[i]) * pow(w, i * k, P) for i in range(n)) % P for k in range(n)]
    assert [int(v) for v in orc.fft(c)] == naive
    assert list(orc.fft(orc.fft(c), inverse=True)) == list(c)


def test_coset_lde_semantics():
    log_n, rate = 4, 3
    n = 1 << log_n
    c = rand_field(n)
    out = orc.coset_lde(c, rate, 7)
    w = pymodel.root_of_unity(log_n + rate)
    for t in (0, 1, 5, 17, 127):
        x = 7 * pow(w, t, P) % P
        assert int(out[t]) == sum(int(c[i]) * pow(x, i, P) for i in range(n)) % P


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "ntt_params_*.json"))))
def test_negacyclic_ntt_golden(path):
    """The reference's own KAT: poly.rs:195-208 (TESTG -> TESTGHAT and back) for every params_{N}.rs."""
    g = json.load(open(path))
    roots, inv, ninv = orc.negacyclic_params(g["LOGN"])
    assert ninv == g["NINV"]
    for name, arr in (("ROOTS", roots), ("INVROOTS", inv)):
        assert hashlib.sha256(struct.pack("<%dQ" % g["N"], *[int(v) for v in arr])).hexdigest() == g[name + "_sha256"]
        if name in g:
            assert [int(v) for v in arr] == g[name]
    assert [int(v) for v in orc.negacyclic_forward(g["TESTG"], roots)] == g["TESTGHAT"]
    assert [int(v) for v in orc.negacyclic_backward(g["TESTGHAT"], inv, ninv)] == g["TESTG"]


def test_negacyclic_is_negacyclic_convolution():
    log_n = 3; n = 8
    roots, inv, ninv = orc.negacyclic_params(log_n)
    a, b = rand_field(n), rand_field(n)
    prod = (orc.negacyclic_forward(a, roots).astype(object) * orc.negacyclic_forward(b, roots).astype(object)) % P
    got = orc.negacyclic_backward(np.array(prod, dtype=np.uint64), inv, ninv)
    want = [0] * n
    for i in range(n):
        for j in range(n):
            k = i + j
            want[k % n] = (want[k % n] + (1 if k < n else -1) * int(a[i]) * int(b[j])) % P
    assert [int(v) for v in got] == want


@pytest.mark.parametrize("leaf_len", [3, 4, 7, 20])
def test_merkle_cap_and_proofs(leaf_len):
    n, cap_h = 32, 2
    leaves = rand_field(n, leaf_len)
    t = orc.Merkle(leaves, cap_h)
    cap = t.cap()
    # independent recomputation of cap[1] (leaves 8..15)
    dig = [orc.hash_or_noop(leaves[i]) for i in range(8, 16)]
    while len(dig) > 1:
        dig = [orc.two_to_one(dig[2 * i], dig[2 * i + 1]) for i in range(len(dig) // 2)]
    assert list(cap[1]) == list(dig[0])
    for idx in (0, 9, 31):
        sib = t.prove(idx)
        assert sib.shape == (3, 4)
        assert orc.merkle_verify(leaves[idx], idx, cap, cap_h, sib)
        bad = leaves[idx].copy(); bad[0] ^= np.uint64(1)
        assert not orc.merkle_verify(bad, idx, cap, cap_h, sib)


def test_polynomial_batch_layout():
    log_n, ncols, rate = 4, 5, 3
    vals = rand_field(ncols, 1 << log_n)
    b = orc.Batch(vals, rate, 2, from_values=True)
    coeffs = b.coeffs()
    for c in range(ncols):
        assert list(coeffs[c]) == list(orc.fft(vals[c], inverse=True))
    leaves = b.leaves()
    log_big = log_n + rate
    lde0 = orc.coset_lde(coeffs[0], rate)
    brev = lambda x: int(format(x, "0%db" % log_big)[::-1], 2)
    for j in (0, 1, 2, 77, 127):
        assert int(leaves[j][0]) == int(lde0[brev(j)])
        assert list(b.lde_row(brev(j))) == list(leaves[j])
    # from_coeffs(coeffs) gives the same commitment
    b2 = orc.Batch(coeffs, rate, 2, from_values=False)
    assert (b2.cap() == b.cap()).all()
    # on the subgroup the LDE reproduces the trace: lde_c at 7*w^t is not on H, so check via eval instead
    zeta = rand_field(2)
    ev = b.eval_ext(zeta)
    z = (int(zeta[0]), int(zeta[1]))
    acc, zp = (0, 0), (1, 0)
    for i in range(1 << log_n):
        acc = ((acc[0] + int(coeffs[2][i]) * zp[0]) % P, (acc[1] + int(coeffs[2][i]) * zp[1]) % P)
        zp = pymodel.ext_mul(zp, z)
    assert (int(ev[2][0]), int(ev[2][1])) == acc


def test_challenger_matches_model():
    ch, model = orc.ChallengerState(), pymodel.Challenger()
    seq = [("o", 3), ("g", 2), ("o", 8), ("o", 1), ("g", 9), ("g", 1), ("o", 17), ("g", 3)]
    for kind, k in seq:
        if kind == "o":
            xs = rand_field(k)
            ch.observe(xs); model.observe(xs)
        else:
            assert ch.get_n(k) == [model.get() for _ in range(k)]


def _fri_setup(log_n, cols=(3, 5, 2, 4), rate=3, cap_h=None, gen=None, **over):
    """rate / cap_h: the FriConfig of the commitments and of the params (cap_h None: the standard 4); gen: a generator of the case's own"""
    params = orc.fri_params(log_n, rate_bits=rate, **({} if cap_h is None else {"cap_height": cap_h}), **over)
    field = rand_field if gen is None else (lambda *shape: gen.integers(0, P, size=shape, dtype=np.uint64))
    oracles = []
    for i, nc in enumerate(cols):
        oracles.append(orc.Batch(field(nc, 1 << log_n), params.rate_bits, params.cap_height, from_values=(i != 3)))
    ch = orc.ChallengerState()
    for o in oracles:
        ch.observe(o.cap())
    zeta = ch.get_ext()
    g = pymodel.root_of_unity(log_n)
    zeta_next = np.array([int(zeta[0]) * g % P, int(zeta[1]) * g % P], np.uint64)
    all_polys = [(o, p) for o in range(len(cols)) for p in range(cols[o])]
    batches = [(zeta, all_polys), (zeta_next, [(2, 0), (2, 1)])]
    openings = [np.concatenate([oracles[o].eval_ext(zeta)[p][None] for o, p in all_polys]),
                np.concatenate([oracles[2].eval_ext(zeta_next)[p][None] for p in (0, 1)])]
    for op in openings:
        ch.observe(op)
    return params, oracles, ch, batches, openings


@pytest.mark.parametrize("log_n,over", [(6, {}), (9, {}), (7, {"mul_final_by_x": 1}), (6, {"pow_bits": 4, "num_query_rounds": 5})])
def test_fri_prove_then_verify(log_n, over):
    params, oracles, ch, batches, openings = _fri_setup(log_n, **over)
    ch_v = ch.clone()
    proof = orc.prove_openings(oracles, batches, ch, params, log_n)
    caps = [o.cap() for o in oracles]; ncols = [o.ncols for o in oracles]
    assert orc.verify_fri(caps, ncols, batches, openings, ch_v.clone(), params, log_n, proof)
    # prover and verifier leave the transcript in the same state
    ch_v2 = ch_v.clone()
    orc.verify_fri(caps, ncols, batches, openings, ch_v2, params, log_n, proof)
    assert ch_v2.state_words() == ch.state_words()
    # tampering: a proof word, an opening, the pow witness
    for pos in (0, proof.size // 2, proof.size - 1):
        bad = proof.copy(); bad[pos] = (int(bad[pos]) + 1) % P
        assert not orc.verify_fri(caps, ncols, batches, openings, ch_v.clone(), params, log_n, bad)
    bad_open = [o.copy() for o in openings]; bad_open[0][1][0] = (int(bad_open[0][1][0]) + 1) % P
    assert not orc.verify_fri(caps, ncols, batches, bad_open, ch_v.clone(), params, log_n, proof)


def test_fri_pow_is_minimal_and_forcable():
    params, oracles, ch, batches, openings = _fri_setup(6, pow_bits=6)
    ch2 = ch.clone()
    proof = orc.prove_openings(oracles, batches, ch, params, 6)
    w = int(proof[-1])
    # a different valid nonce is accepted when forced (reference: rayon find_any returns any valid nonce)
    proof2 = orc.prove_openings(oracles, batches, ch2.clone(), params, 6, forced_pow=w)
    assert (proof2 == proof).all()


def test_fri_arity_schedule():
    # 2^15 -> [4,4,4] (final 2^3), 2^12 -> [4,4] (2^4), 2^16 -> [4,4,4] (2^4)
    for d, rounds in ((15, 3), (12, 2), (16, 3)):
        p = orc.fri_params(d)
        assert p.n_rounds == rounds and list(p.arity_bits)[:rounds] == [4] * rounds


# ---- FRI off the standard configuration (fri_shapes.py): the reference side of test_gpu_fri_shapes.py, checked against itself.  The
# oracle's prover folds coefficients, its verifier checks the folds by Lagrange interpolation: two methods, one answer. ----
def _prove_verify_tamper(log_n, cols, seed, rate=3, cap_h=4, **over):
    gen = np.random.default_rng(seed)
    params, oracles, ch, batches, openings = _fri_setup(log_n, cols, rate, cap_h, gen=gen, **over)
    ch_v = ch.clone()
    proof = orc.prove_openings(oracles, batches, ch, params, log_n)
    caps = [o.cap() for o in oracles]; ncols = [o.ncols for o in oracles]
    ch_v2 = ch_v.clone()
    assert orc.verify_fri(caps, ncols, batches, openings, ch_v2, params, log_n, proof)
    assert ch_v2.state_words() == ch.state_words()   # prover and verifier leave the transcript in the same state
    for pos in [0, proof.size // 2, proof.size - 1] + [int(q) for q in gen.integers(0, proof.size, 20)]:
        bad = proof.copy(); bad[pos] = (int(bad[pos]) + 1) % P
        assert not orc.verify_fri(caps, ncols, batches, openings, ch_v.clone(), params, log_n, bad), pos
    return params, caps, ncols, batches, openings, ch_v, proof


@pytest.mark.parametrize("shape", fri_shapes.FRI_SHAPES, ids=fri_shapes.shape_id)
def test_fri_shapes_prove_then_verify(shape):
    log_n, rate, cap_h, bits = shape
    params, *_ = _prove_verify_tamper(log_n, fri_shapes.FRI_COLS, 1000 + fri_shapes.FRI_SHAPES.index(shape), rate, cap_h, arity_bits=bits)
    assert (params.rate_bits, params.cap_height, params.n_rounds, list(params.arity_bits)) == (rate, cap_h, len(bits), bits + [0] * (16 - len(bits)))


@pytest.mark.parametrize("cols", fri_shapes.POLY_COUNTS, ids=lambda c: "%d_polys" % sum(c))
def test_fri_polynomial_counts_prove_then_verify(cols):
    _prove_verify_tamper(fri_shapes.POLY_COUNT_LOG_N, cols, 2000 + sum(cols))


@pytest.mark.parametrize("nq", fri_shapes.QUERY_COUNTS)
def test_fri_query_counts_prove_then_verify(nq):
    _prove_verify_tamper(fri_shapes.QUERY_COUNT_LOG_N, fri_shapes.FRI_COLS, 3000 + nq, pow_bits=fri_shapes.QUERY_COUNT_POW_BITS, num_query_rounds=nq)


def test_fri_proof_is_bound_to_its_arity_list():
    params, caps, ncols, batches, openings, ch_v, proof = _prove_verify_tamper(8, fri_shapes.FRI_COLS, 4000, arity_bits=[3, 2])
    other = orc.fri_params(8, arity_bits=[2, 3])
    sizes = (orc.C.c_size_t * 4)(*ncols)
    words = [orc.lib().orc_fri_proof_words(orc.C.byref(p), 8, sizes, 4) for p in (params, other)]
    assert words[0] != words[1]   # the two layouts differ in length; the verifier reads only what its own layout names, inside the longer buffer
    padded = np.concatenate([proof, np.zeros(max(0, words[1] - words[0]), np.uint64)])
    assert not orc.verify_fri(caps, ncols, batches, openings, ch_v.clone(), other, 8, padded)


def test_standard_arities_restate_the_oracles_rule():
    for log_n in range(1, 22):
        assert fri_shapes.standard_arities(log_n) == list(orc.fri_params(log_n).arity_bits)[:orc.fri_params(log_n).n_rounds]
    for (log_n, rate, cap_h), rounds in fri_shapes.STEP_SHAPES:
        assert fri_shapes.standard_arities(log_n, rate, cap_h) == [4] * rounds


@pytest.mark.parametrize("shape,rounds", fri_shapes.STEP_SHAPES, ids=lambda v: "n%d-r%d-c%d" % v if isinstance(v, tuple) else None)
def test_step_oracle_proves_and_verifies_at_every_step_shape(shape, rounds):
    import step_oracle
    from vpbs_amd import synth
    log_n, rate, cap_h = shape
    inputs = synth.step_inputs(log_n, cols=fri_shapes.STEP_COLS)
    pis = synth.field_elements(0xABCD, 11)
    digest = np.array([11, 22, 33, 44], np.uint64)
    proof = step_oracle.prove_step(inputs, digest, pis, log_n, rate_bits=rate, cap_height=cap_h)
    assert proof["caps"].shape == (3, 1 << cap_h, 4) and proof["ncols"] == list(fri_shapes.STEP_COLS.values())
    assert step_oracle.verify_step(proof, proof["cs_cap"], proof["ncols"], digest, pis, log_n, rate_bits=rate, cap_height=cap_h)
    if (rate, cap_h) != (3, 4):   # ... and not under the standard configuration
        bad = dict(proof, fri=proof["fri"].copy())
        bad["fri"][-2] = (int(bad["fri"][-2]) + 1) % P
        assert not step_oracle.verify_step(bad, proof["cs_cap"], proof["ncols"], digest, pis, log_n, rate_bits=rate, cap_height=cap_h)


def test_step_oracle_defaults_are_the_standard_configuration():
    """the generalised step_oracle under its defaults: the frozen proofs of test_oracle_reproduces_frozen_step_proofs pin the words; here the
    parameters themselves"""
    import step_oracle
    for log_n in (5, 6, 10, 12, 15, 16):
        a, b = step_oracle.step_fri_params(log_n), orc.fri_params(log_n)
        assert bytes(a) == bytes(b)


def test_partial_products_match_bigint_model():
    """plonk/prover.rs wires_permutation_partial_products_and_zs restated; checked against a direct big-int evaluation
    (num/den per element, chunk products, running Z) incl. a ragged last chunk."""
    log_n, n_routed, deg = 3, 10, 4
    n = 1 << log_n
    wires, sig = rand_field(n_routed, n), rand_field(n_routed, n)
    betas, gammas = [int(x) for x in rand_field(2)], [int(x) for x in rand_field(2)]
    got = orc.partial_products(wires, sig, betas, gammas, max_degree=deg)
    w = pymodel.root_of_unity(log_n)
    chunks = (n_routed + deg - 1) // deg
    assert got.shape == (2 * chunks, n)
    for c in range(2):
        z = 1
        for i in range(n):
            x = pow(w, i, P)
            q = [(int(wires[j][i]) + betas[c] * pow(7, j, P) * x + gammas[c]) *
                 pow(int(wires[j][i]) + betas[c] * int(sig[j][i]) + gammas[c], P - 2, P) % P for j in range(n_routed)]
            assert int(got[c][i]) == z            # Z(w^i), Z(1) = 1
            run = z
            for k in range(chunks):
                for j in range(deg * k, min(deg * k + deg, n_routed)):
                    run = run * q[j] % P
                if k < chunks - 1:
                    assert int(got[2 + c * (chunks - 1) + k][i]) == run
            z = run


def test_partial_products_true_permutation_closes():
    """With sigma a genuine permutation of the (column, row) positions and wire values constant on its cycles, the grand
    product returns to 1: Z(w^n) = 1 (the property the PLONK permutation check relies on)."""
    log_n, n_routed = 4, 8
    n = 1 << log_n
    w = pymodel.root_of_unity(log_n)
    perm = rng.permutation(n_routed * n)
    # wire values: equal along each cycle of perm
    vals = np.zeros(n_routed * n, dtype=np.uint64)
    seen = np.zeros(n_routed * n, bool)
    for s0 in range(n_routed * n):
        if not seen[s0]:
            v = rand_field(1)[0]
            t = s0
            while not seen[t]:
                seen[t] = True; vals[t] = v; t = perm[t]
    wires = vals.reshape(n_routed, n)
    sig = np.zeros((n_routed, n), np.uint64)
    for pos in range(n_routed * n):
        tc, tr = divmod(int(perm[pos]), n)
        sig[pos // n][pos % n] = pow(7, tc, P) * pow(w, tr, P) % P
    betas, gammas = [int(x) for x in rand_field(1)], [int(x) for x in rand_field(1)]
    out = orc.partial_products(wires, sig, betas, gammas, max_degree=8)
    assert int(out[0][0]) == 1
    # Z(w^n) = Z(w^(n-1)) * (row n-1 product); num_prods = 0 here so recompute the last row product directly
    x = pow(w, n - 1, P)
    i = n - 1
    rowp = 1
    for j in range(n_routed):
        rowp = rowp * (int(wires[j][i]) + betas[0] * pow(7, j, P) * x + gammas[0]) % P
        rowp = rowp * pow(int(wires[j][i]) + betas[0] * int(sig[j][i]) + gammas[0], P - 2, P) % P
    assert int(out[0][n - 1]) * rowp % P == 1


def _copy_constraint_instance(log_n, n_routed):
    """wires constant on the cycles of a random permutation of the (column, row) cells + its sigma polynomials (values)"""
    n = 1 << log_n
    w = pymodel.root_of_unity(log_n)
    perm = rng.permutation(n_routed * n)
    vals = np.zeros(n_routed * n, dtype=np.uint64)
    seen = np.zeros(n_routed * n, bool)
    for s0 in range(n_routed * n):
        if not seen[s0]:
            v = rand_field(1)[0]
            t = s0
            while not seen[t]:
                seen[t] = True; vals[t] = v; t = perm[t]
    sig = np.zeros((n_routed, n), np.uint64)
    for pos in range(n_routed * n):
        tc, tr = divmod(int(perm[pos]), n)
        sig[pos // n][pos % n] = pow(7, tc, P) * pow(w, tr, P) % P
    return vals.reshape(n_routed, n), sig


@pytest.mark.parametrize("log_n,n_routed", [(4, 8), (5, 16), (4, 20)])
def test_quotient_permutation_satisfies_verifier_identity(log_n, n_routed):
    """a12 + a13 (permutation part) end to end on the CPU oracle: for a witness that satisfies its copy constraints the
    quotient chunks satisfy vanishing(zeta) = Z_H(zeta) * t(zeta) at a random extension point; a broken witness does not."""
    wires, sig = _copy_constraint_instance(log_n, n_routed)
    betas, gammas, alphas = ([int(x) for x in rand_field(2)] for _ in range(3))
    nc = 2
    n_chunks = (n_routed + 7) // 8

    def run(wv):
        zs_pp = orc.partial_products(wv, sig, betas, gammas)
        coeffs = lambda m: np.stack([orc.fft(r, inverse=True) for r in m])
        wc, sc, zc = coeffs(wv), coeffs(sig), coeffs(zs_pp)
        q = orc.quotient_permutation(wc, sc, zc, betas, gammas, alphas)
        zeta = rand_field(2)
        g = pymodel.root_of_unity(log_n)
        zeta_next = np.array([int(zeta[0]) * g % P, int(zeta[1]) * g % P], np.uint64)
        ev = orc.eval_coeffs_ext
        zs_z, zs_next = ev(zc[:nc], zeta), ev(zc[:nc], zeta_next)
        pps = ev(zc[nc:], zeta) if n_chunks > 1 else np.zeros((0, 2), np.uint64)
        return orc.check_vanishing_at_zeta(ev(wc, zeta), ev(sc, zeta), zs_z, zs_next, pps, ev(q, zeta), log_n, betas, gammas, alphas, zeta)

    assert run(wires)
    bad = wires.copy(); bad[1][3] = (int(bad[1][3]) + 1) % P   # breaks one copy constraint
    assert not run(bad)


def test_tfhe_oracle_reference_properties():
    """tests/tfhe_oracle.py restates the in-circuit TFHE step; pin it with the reference's own test properties:
    test_decompose (glwe_poly.rs:239: sum limb_i B^i == x, digits centred) and test_blind_rot_step (mod.rs:223-279)."""
    import tfhe_oracle as T
    for logb in (8, 5, 4, 7):
        for x in [0, 1, P - 1, P - 2, 1 << 63, (1 << 63) - 1, 0xFFFFFFFF] + [int(v) for v in rand_field(30)]:
            d = T.decompose(x, logb)
            assert sum(di * pow(2, logb * i, P) for i, di in enumerate(d)) % P == x % P
            assert all(-(1 << (logb - 1)) <= (di if di < P // 2 else di - P) <= (1 << (logb - 1)) for di in d)
    ring = T.Ring(3); K, ELL, LOGB = 2, 8, 8
    for bit in (0, 1):
        s = [[int(v) for v in rng.integers(0, 2, size=8)] for _ in range(K - 1)]
        m = list(range(8))
        ct = T.glwe_encrypt(ring, rng, s, m, K)
        gg = T.ggsw_encrypt_hat(ring, rng, s, [bit] + [0] * 7, K, ELL, LOGB)
        ai = int(rand_field(1)[0])
        assert T.glwe_decrypt(ring, s, T.step(ring, ct, ai, gg, K, ELL, LOGB), K) == (m if bit == 0 else T.rotate(m, T.mod_switch(ai, 3)))
        # first step: pure rotation by -mask; last step: plain external product (no CMUX add)
        assert T.glwe_decrypt(ring, s, T.step(ring, ct, ai, gg, K, ELL, LOGB, first_step=True), K) == T.rotate(m, T.mod_switch((P - ai) % P, 3))
        assert T.glwe_decrypt(ring, s, T.step(ring, ct, ai, gg, K, ELL, LOGB, last_step=True), K) == [bit * v for v in m]


def test_oracle_reproduces_frozen_step_proofs():
    """regression vectors (tests/golden/regression_step_proofs.json, produced by THIS oracle at an earlier commit -- not reference
    vectors): caps, challenges, openings, FRI proof and pow witness of four seeded step proofs must not drift."""
    import gates_oracle as go
    import regression_cases as rc
    import step_oracle
    for case in rc.cases():
        b = rc.build(case)
        if b["gates"] is None:
            p = step_oracle.prove_step(b["inputs"], rc.DIGEST, b["pis"], b["log_n"])
        else:
            p = step_oracle.prove_step(b["inputs"], rc.DIGEST, b["pis"], b["log_n"], sigmas=b["sigma"], n_routed=80,
                                       n_constants=b["n_constants"], gates=go.GateSet(b["gates"]))
        rc.check(case, p)


def test_oracle_x8_poseidon_matches_the_kat_pinned_scalar_form():
    """oracle/poseidon_x8.c (eight permutations per AVX-512 register: what the oracle's Merkle trees, its proof-of-work scan and bench.py's
    cpu_baseline use where the CPU has AVX-512) against the scalar orc_poseidon that the upstream KATs pin: the KAT vectors themselves,
    random and edge-valued states, ragged batch sizes, leaf hashing / tree levels / the PoW scan in both forms."""
    import ctypes as C
    L = orc.lib()
    L.orc_poseidon_x8_enable.restype, L.orc_poseidon_x8_enable.argtypes = C.c_int, [C.c_int]
    if not L.orc_poseidon_x8_enable(1):
        pytest.skip("no AVX-512F/DQ on this CPU: the oracle only has its scalar permutation here")
    try:
        import step_oracle
        kat = json.load(open(os.path.join(GOLD, "poseidon_kat.json")))["kats"]
        rng = np.random.default_rng(77)
        edge = np.array([0, 1, P - 1, P - 2, 0xFFFFFFFF, 1 << 32, 0xFFFFFFFF00000000, 1 << 63], np.uint64)
        for n in (8, 9, 15, 16, 23, 1000):
            st = rng.integers(0, P, size=(n, 12), dtype=np.uint64)
            st[rng.random(st.shape) < 0.2] = edge[rng.integers(0, edge.size)]
            for i, v in enumerate(kat[:min(n, len(kat))]):
                st[i] = np.array([int(x) for x in v["input"]], np.uint64)
            want = np.stack([orc.poseidon(s) for s in st])
            got = st.copy()
            L.orc_poseidon_batch(orc.ptr(got), n)          # n >= 8: the x8 path
            assert (got == want).all(), n
            for i, v in enumerate(kat[:min(n, len(kat))]):
                assert [int(x) for x in got[i]] == [int(x) for x in v["output"]]
        # trees: leaf lengths on both sides of the hash_or_noop boundary and of the sponge blocks, ragged leaf counts via the cap height
        for leaf_len, log_leaves, cap in ((3, 5, 1), (4, 4, 0), (5, 6, 2), (8, 5, 4), (9, 7, 3), (135, 6, 4), (32, 4, 4)):
            leaves = rng.integers(0, P, size=(1 << log_leaves, leaf_len), dtype=np.uint64)
            L.orc_poseidon_x8_enable(0)
            a = orc.Merkle(leaves, cap)
            cap_a, path_a = a.cap(), a.prove(3)
            L.orc_poseidon_x8_enable(1)
            b = orc.Merkle(leaves, cap)
            assert (b.cap() == cap_a).all() and (b.prove(3) == path_a).all(), (leaf_len, log_leaves, cap)
        # a whole FRI proof (trees, proof-of-work scan: the smallest nonce) in both forms
        log_n = 6
        datas = [rng.integers(0, P, size=(nc, 1 << log_n), dtype=np.uint64) for nc in (4, 6, 3, 2)]
        proofs = []
        for on in (0, 1):
            L.orc_poseidon_x8_enable(on)
            ob = [orc.Batch(d, 3, 4, from_values=(i != 3)) for i, d in enumerate(datas)]
            ch = orc.ChallengerState()
            for o in ob:
                ch.observe(o.cap())
            zeta = ch.get_ext()
            batches, zeta_next = step_oracle.step_batches([4, 6, 3, 2], 2, zeta, log_n)
            ch.observe(np.concatenate([o.eval_ext(zeta) for o in ob] + [ob[2].eval_ext(zeta_next)[:2]]))
            proofs.append(orc.prove_openings(ob, batches, ch, orc.fri_params(log_n), log_n))
        assert (proofs[0] == proofs[1]).all()
    finally:
        L.orc_poseidon_x8_enable(1)
