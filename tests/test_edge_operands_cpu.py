"""CPU checks of tests/edge_operands.py: the edge operands are canonical, and every expected value the GPU edge tests
(tests/test_gpu_edge_operands.py) derive from them agrees with the oracle."""
import numpy as np
import pytest

import edge_operands as eo
import oracle as orc
import tfhe_oracle as T

P = eo.P


def test_edge_set_is_canonical_and_distinct():
    for vals in (eo.E, eo.ROOTS, eo.E_ROOTS):
        assert all(0 <= v < P for v in vals) and len(set(vals)) == len(vals)
    assert len(eo.E) == 13
    assert all(pow(r, 8, P) == 1 for r in eo.ROOTS)
    assert sorted(pow(r, 4, P) for r in eo.ROOTS).count(P - 1) == 4      # four primitive 8th roots
    for z in eo.ZETAS:
        assert all(0 <= v < P for v in z)
    assert (eo.patterns(5, 64) < P).all()
    assert (eo.constant_columns(20, 4) < P).all()
    for n in (1, 2, 256, 4096, 8192):
        assert (eo.opening_columns(n) < P).all()


@pytest.mark.parametrize("log_n", [1, 2, 3, 6, 11, 12, 13])
def test_derived_inputs_round_trip(log_n):
    coeffs = eo.patterns(3, 1 << log_n)
    vals = eo.values_for_coeffs(coeffs)
    assert (vals < P).all()
    for c in range(3):
        assert (orc.fft(vals[c], inverse=True) == coeffs[c]).all()


@pytest.mark.parametrize("n", [1, 2, 8, 64])
def test_ext_horner_matches_oracle(n):
    cols = np.concatenate([eo.patterns(3, n), eo.opening_columns(n)])
    for zeta in eo.ZETAS:
        want = orc.eval_coeffs_ext(cols, zeta)
        assert [eo.ext_horner(c, zeta) for c in cols] == [tuple(int(x) for x in w) for w in want]
        assert (orc.Batch(cols, 3, 0, from_values=False).eval_ext(np.array(zeta, np.uint64)) == want).all()


def test_opening_columns_vanish_where_chosen():
    for n in (256, 8192):
        cols = eo.opening_columns(n)
        assert eo.ext_horner(cols[2], (1, 0)) == (0, 0)
        assert eo.ext_horner(cols[3], (1, 0)) == (0, 0)
        assert eo.ext_horner(cols[4], (1, 0)) == ((P - n) % P, 0)
        assert eo.ext_horner(cols[5], (P - 1, 0)) == (0, 0)


@pytest.mark.parametrize("log_n,rate_bits,shift", [(2, 0, 1), (3, 1, 1), (4, 2, 1), (4, 3, 1), (3, 3, 7), (5, 0, 7)])
def test_monomial_closed_forms_match_coset_lde(log_n, rate_bits, shift):
    n = 1 << log_n
    for k in (0, n // 4, n // 2, n - 1):
        want = eo.monomial_lde(log_n, rate_bits, shift, k)
        assert (orc.coset_lde(eo.monomial(n, k), rate_bits, shift) == want).all()
        if shift == 1 and k == n // 2 and rate_bits <= 2:   # +-1 at rate 0, the 4th roots of unity at rate 1, the 8th at rate 2
            assert set(int(v) for v in want) <= set(eo.ROOTS)


def test_bitrev_index():
    assert list(eo.bitrev_index(3)) == [0, 4, 2, 6, 1, 5, 3, 7]
    assert list(eo.bitrev_index(0)) == [0]


def test_partial_product_cases_have_nonzero_denominators():
    for n_routed, log_n, deg, nc, kind in eo.PP_CASES:
        if log_n > 4:
            continue   # the 2^16-row cases assert the same in pp_case itself, on the GPU box
        wires, sig, betas, gammas = eo.pp_case(n_routed, log_n, nc, kind)
        assert (wires < P).all() and (sig < P).all()
        assert eo.denominators_nonzero(wires, sig, betas, gammas)
    with pytest.raises(AssertionError):
        eo.partial_products_model(np.zeros((1, 2), np.uint64), np.zeros((1, 2), np.uint64), [1], [0], 8)


@pytest.mark.parametrize("n_routed,log_n,deg", [(17, 3, 8), (10, 3, 4), (80, 2, 8)])
def test_partial_products_model_matches_oracle(n_routed, log_n, deg):
    n = 1 << log_n
    wires, sig = eo.patterns(n_routed, n), eo.patterns(n_routed, n)[::-1].copy()
    for betas, gammas in (([0, 5], [3, 7]), ([P - 1, 2], [1, P - 2])):
        s = eo.avoid_zero_denominators(wires, sig, betas, gammas)
        assert (eo.partial_products_model(wires, s, betas, gammas, deg) == orc.partial_products(wires, s, betas, gammas, deg)).all()


def test_ratio_minus_one_wires():
    n_routed, n = 17, 8
    sig = eo.patterns(n_routed, n)
    beta, gamma = P - 1, 1
    w = eo.wires_for_ratio_minus_one(sig, beta, gamma)
    pp = eo.partial_products_model(w, sig, [beta], [gamma], 8)
    assert (orc.partial_products(w, sig, [beta], [gamma], 8) == pp).all()
    # chunks of 8, 8 and 1 ratios of -1: Z alternates 1, -1
    assert [int(v) for v in pp[0]] == [1, P - 1] * (n // 2)


def test_mask_boundaries_hold_every_tie_and_truncation_boundary():
    """mod_switch (tfhe.hip, tfhe_oracle) rounds the top log_N + 1 bits with bit 62 - log_N: the shift steps up between each tie
    (2k + 1) 2^(62 - log_N) and its -1 neighbour, and the set holds every such pair and every truncation boundary k 2^(63 - log_N)"""
    for log_N in (3, 4):
        ms = set(eo.mask_boundaries(log_N))
        assert all(0 <= m < P for m in ms) and {0, P - 1} <= ms
        assert T.mod_switch(P - 1, log_N) == 2 << log_N and T.mod_switch(0, log_N) == 0
        half = 1 << (62 - log_N)
        ties = [t for t in range(half, P, 2 * half)]
        assert len(ties) == 1 << (log_N + 1)
        for t in ties:
            assert {t - 1, t, t + 1} <= ms
            assert T.mod_switch(t, log_N) == T.mod_switch(t - 1, log_N) + 1 == T.mod_switch(t + 1, log_N)
        for b in range(2 * half, P, 2 * half):
            assert {b - 1, b, b + 1} <= ms and T.mod_switch(b - 1, log_N) == T.mod_switch(b, log_N)
        assert {T.mod_switch(m, log_N) for m in ms} == set(range((2 << log_N) + 1))


@pytest.mark.parametrize("logb", [4, 5, 7, 8])
def test_decomposition_boundaries(logb):
    """canonical, centred digits that recompose to the value, and carries that reach the top digit"""
    B, nl = 1 << logb, -(-64 // logb)
    bs = eo.decomposition_boundaries(logb)
    assert all(0 <= x < P for x in bs) and len(set(bs)) == len(bs)
    for x in bs:
        d = T.decompose(x, logb)
        assert len(d) == nl and all(min(v, P - v) <= B // 2 for v in d)
        assert sum(v * B ** l for l, v in enumerate(d)) % P == x
    half = bs[5]
    assert all(v != 0 for v in T.decompose(half, logb)[:-1])    # sum (B/2) B^l: every digit but the top one carries


@pytest.mark.parametrize("shift", [1, 3, 8, 9, 15])
def test_acc_for_difference(shift):
    t = eo.pattern(8, shift, 1, eo.decomposition_boundaries(5))
    a = eo.acc_for_difference(t, shift)
    assert all(0 <= v < P for v in a)
    assert [(x - y) % P for x, y in zip(T.rotate(a, shift), a)] == [int(v) for v in t]
    assert eo.acc_for_difference(t, 0) is None and eo.acc_for_difference(t, 16) is None


def test_legal_presets():
    import gates_oracle as go
    gs = go.GateSet(["noop", "base_sum", "poseidon", ("random_access", 4), "exponentiation", "coset_interpolation", "arithmetic"])
    g = {x.kind: x for x in gs.gates}
    bs = g["base_sum"]
    assert eo.legal_preset(bs, 0, P - 1) == min(P, bs.p1 ** bs.p0) - 1 and eo.legal_preset(bs, 0, 2) == 2
    ra = g["random_access"]
    assert eo.legal_preset(ra, 0, P - 1) == (1 << ra.p0) - 1 and eo.legal_preset(ra, 2, P - 1) == P - 1
    assert eo.legal_preset(g["poseidon"], 24, 1 << 63) == 1 and eo.legal_preset(g["poseidon"], 3, 1 << 63) == 1 << 63
    assert eo.legal_preset(g["exponentiation"], 1, P - 2) == 1 and eo.legal_preset(g["exponentiation"], 0, P - 2) == P - 2
    assert eo.legal_preset(g["coset_interpolation"], 0, 0) == P - 1
    assert eo.legal_preset(g["arithmetic"], 0, P - 1) == P - 1
