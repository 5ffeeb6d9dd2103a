"""GPU parity tests (-m gpu) on edge operands: every kernel that keeps u64 residues between its steps (the transforms, the openings'
lazy sums, the partial products' shared inversion, the quotient's lazy products, the gate evaluators, FRI, the TFHE step) fed so that its
results and intermediates land on 0, p - 1, 2^32 - 1, 2^63, the roots of unity and their neighbours -- where a missing canonicalisation
or a wrong wrap correction shows, and where uniformly random operands land about once in 2^32 (tests/edge_operands.py).  Every value
handed to the ABI is canonical; every array that comes back must be canonical and equal, word for word, big-int arithmetic or the
oracle."""
import random

import numpy as np
import pytest

import edge_operands as eo
import gates_oracle as go
import oracle as orc
import step_oracle
import vpbs_amd
from vpbs_amd import api

pytestmark = pytest.mark.gpu
P = api.P
DIGEST = np.array([11, 22, 33, 44], np.uint64)
ALL = ["noop", "constant", "public_input", "arithmetic", "base_sum", "poseidon", "poseidon_mds", "arithmetic_ext", "mul_ext", "reducing",
       "reducing_ext", ("random_access", 4), "exponentiation", "coset_interpolation"]
SMALL_VARIANTS = [("base_sum", 10, 3), ("random_access", 1), ("random_access", 2), ("random_access", 3), ("random_access", 5),
                  ("coset_interpolation", 2), ("coset_interpolation", 3), ("coset_interpolation", 5), ("constant", 1), ("reducing", 5),
                  ("reducing_ext", 1), ("exponentiation", 7), ("mul_ext", 2), ("arithmetic", 3)]   # those of tests/test_gpu_gates.py


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    yield c
    c.close()


def canonical(a, kernel):
    a = np.asarray(a)
    assert (a < P).all(), "%s stored a non-canonical word: %r" % (kernel, a[a >= P][:4])


# ---------- inverse transform and coset LDE: ntt_small_kernel below 2^12, every plan16 (NR, QL) sequence from 2^12 to 2^22 ----------
NTT_LOGS = [1, 2, 3, 6, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22]


def _kernel(log_n):
    return "ntt_small_kernel" if log_n < 12 else "radix-16 plan16(%d)" % log_n


@pytest.mark.parametrize("log_n", NTT_LOGS)
@pytest.mark.parametrize("ncols", [1, 3])
def test_intt_of_derived_values_gives_the_edge_coefficients(ctx, log_n, ncols):
    """choose the coefficients from E and the roots of unity, derive the values with the oracle's forward FFT: the device inverse
    transform must give back exactly the chosen coefficients"""
    coeffs = eo.patterns(ncols, 1 << log_n)
    got = ctx.intt(eo.values_for_coeffs(coeffs))
    canonical(got, _kernel(log_n))
    assert (got == coeffs).all(), _kernel(log_n)


@pytest.mark.parametrize("log_n", NTT_LOGS)
@pytest.mark.parametrize("shift", [7, 1])
def test_coset_lde_of_edge_polynomials(ctx, log_n, shift):
    """constant E columns (every LDE point is the constant), x^(n/2) and x^(n/4) (at shift 1: roots of unity of small order
    everywhere), E coefficient walks; the coefficient size 2^log_n picks the plan (launch_coset_lde), the rate only the number of cosets"""
    rate_bits = min(3, 22 - log_n)
    n, log_big = 1 << log_n, log_n + rate_bits
    kernel = _kernel(log_n)
    idx = eo.bitrev_index(log_big)
    consts = np.zeros((3, n), np.uint64)
    consts[:, 0] = eo.constant_columns(3, 1, offset=log_n)[:, 0]   # the constant polynomials, as coefficients
    got = ctx.coset_lde(consts, rate_bits, shift)
    canonical(got, kernel)
    assert (got == consts[:, :1]).all(), kernel
    mono = np.stack([eo.monomial(n, n // 2 if n > 1 else 0), eo.monomial(n, n // 4 if n > 2 else 0)])
    got = ctx.coset_lde(mono, rate_bits, shift)
    canonical(got, kernel)
    for c in range(2):
        k = int(np.argmax(mono[c]))
        want = eo.monomial_lde(log_n, rate_bits, shift, k) if log_big <= 16 else orc.coset_lde(mono[c], rate_bits, shift)
        assert (got[c] == want[idx]).all(), (kernel, k)
    coeffs = eo.patterns(3, n)
    got = ctx.coset_lde(coeffs, rate_bits, shift)
    canonical(got, kernel)
    for c in range(3):
        assert (got[c] == orc.coset_lde(coeffs[c], rate_bits, shift)[idx]).all(), kernel


@pytest.mark.parametrize("log_n,ncols,kind", [(1, 3, "const"), (2, 4, "walk"), (3, 1, "const"), (4, 2, "walk"), (6, 5, "mono"), (2, 9, "const"),
                                              (10, 3, "walk"), (12, 3, "const"), (13, 4, "mono"), (16, 3, "walk")])
@pytest.mark.parametrize("from_values", [True, False])
def test_commit_edge_columns(ctx, log_n, ncols, kind, from_values):
    """commit_values / commit_coeffs of constant, monomial and E-walk columns: caps, opened rows and paths, coefficients, LDE rows"""
    n = 1 << log_n
    if kind == "const":
        data = eo.constant_columns(ncols, n, offset=ncols)
    elif kind == "mono":
        data = np.stack([eo.monomial(n, (n >> (1 + c % 2)) if n > 2 else 0) for c in range(ncols)])
    else:
        data = eo.patterns(ncols, n)
    want = orc.Batch(data, 3, 4, from_values=from_values)
    got = (ctx.commit_values if from_values else ctx.commit_coeffs)(data)
    assert (got.cap() == want.cap()).all()
    co = got.coeffs()
    canonical(co, "commit: iNTT")
    assert (co == want.coeffs()).all()
    L = 1 << (log_n + 3)
    for idx in sorted({0, 1, L // 2, L // 2 + 3, L - 1}):
        leaf, sib = got.open(idx)
        canonical(leaf, "commit: coset LDE")
        wleaf, wsib = want.open(idx)
        assert (leaf == wleaf).all() and (sib == wsib).all(), idx
    rows = got.lde_rows(0, min(4, L), step=1)
    for k in range(rows.shape[0]):
        assert (rows[k] == want.lde_row(k, 1)).all()
    got.free()


# ---------- openings: eval_partial_kernel / eval_finish_kernel (Batch.eval_ext) ----------
@pytest.mark.parametrize("log_n", [1, 3, 8, 9, 12, 13, 16])   # one partial sum of <= 256 terms, 256-term blocks, 4096-term chunks
def test_openings_at_edge_points(ctx, log_n):
    """coefficient columns of E walks and of cancelling pairs across every block / chunk boundary (true value 0 at zeta = 1 or -1),
    evaluated at 1, -1, X, 2^32 and (p-1)(1 + X): big-int Horner in GF(p^2)"""
    n = 1 << log_n
    cols = eo.opening_columns(n)
    b = ctx.commit_coeffs(cols)
    ob = orc.Batch(cols, 3, 4, from_values=False) if log_n <= 12 else None
    for zeta in eo.ZETAS:
        got = b.eval_ext(np.array(zeta, np.uint64))
        canonical(got, "eval_partial_kernel / eval_finish_kernel")
        want = [eo.ext_horner(c, zeta) for c in cols]
        assert [tuple(int(x) for x in g) for g in got] == want, zeta
        if ob is not None:
            assert (ob.eval_ext(np.array(zeta, np.uint64)) == got).all()
    assert tuple(b.eval_ext(np.array((1, 0), np.uint64))[2]) == (0, 0) and tuple(b.eval_ext(np.array((P - 1, 0), np.uint64))[5]) == (0, 0)
    b.free()


# ---------- partial products: pp_rows_kernel (80 routed wires, degree 8: one kernel, shared inversion) and the three-kernel path ----------
@pytest.mark.parametrize("n_routed,log_n,deg,nc,kind", eo.PP_CASES)
def test_partial_products_on_edge_operands(ctx, n_routed, log_n, deg, nc, kind):
    """beta = 0 (every ratio 1: Z and every partial product exactly 1), beta = p - 1 with gamma = 1, ratios that all equal p - 1, E wires
    and sigmas with E challenges; against the big-int model at small n and against the oracle at 2^16 x 80"""
    path = "pp_rows_kernel (shared inversion)" if (n_routed, deg) == (80, 8) else "pp_chunk / pp_row / pp_block_prod / pp_finish kernels"
    wires, sig, betas, gammas = eo.pp_case(n_routed, log_n, nc, kind)
    got = ctx.partial_products(wires, sig, betas, gammas, deg)
    canonical(got, path)
    want = eo.partial_products_model(wires, sig, betas, gammas, deg) if log_n <= 4 else orc.partial_products(wires, sig, betas, gammas, deg)
    assert got.shape == want.shape and (got == want).all(), path
    if kind == "beta0":
        assert (got == 1).all(), path
    if kind == "ratio_minus1":
        assert set(int(v) for v in np.unique(got)) <= {1, P - 1}, path


# ---------- quotient, permutation part ----------
def _leaf_order(nat, log_big):
    return np.ascontiguousarray(nat[:, eo.bitrev_index(log_big)])


def _gate_terms_dev(values_nat, log_big):
    import torch
    d = torch.from_numpy(_leaf_order(values_nat, log_big).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("log_n,n_routed,n_constants,nc,with_gates", [(4, 8, 0, 1, False), (6, 20, 3, 2, True), (7, 80, 3, 4, True),
                                                                      (8, 80, 5, 2, False), (5, 80, 2, 1, True)])
def test_quotient_permutation_vanishes_with_beta_zero(ctx, log_n, n_routed, n_constants, nc, with_gates):
    """beta = 0 makes every ratio 1, so Z = every partial product = 1 and every permutation term vanishes identically: with alpha from E
    (and zero gate terms) every quotient word is exactly 0 -- canonical 0, not p"""
    n = 1 << log_n
    wires_v, sig_v = eo.patterns(n_routed + 4, n), eo.patterns(n_routed + 7, n)[7:].copy()
    const_v = eo.constant_columns(n_constants, n)
    betas, gammas = [0] * nc, [3, 5, (1 << 32) + 2, P - 3][:nc]
    alphas = [eo.E[(2 + 3 * c) % len(eo.E)] for c in range(nc)]
    sig_v = eo.avoid_zero_denominators(wires_v[:n_routed], sig_v, betas, gammas)
    zs_v = orc.partial_products(wires_v[:n_routed], sig_v, betas, gammas)
    assert (zs_v == 1).all()
    cs = ctx.commit_values(np.concatenate([const_v, sig_v]) if n_constants else sig_v)
    wb, zb = ctx.commit_values(wires_v), ctx.commit_values(zs_v)
    gate_dev = _gate_terms_dev(np.zeros((nc, 8 * n), np.uint64), log_n + 3) if with_gates else None
    got = ctx.quotient_permutation(cs, n_constants, wb, zb, n_routed, betas, gammas, alphas,
                                   gate_terms_dev=gate_dev.data_ptr() if with_gates else None)
    canonical(got, "quotient (permutation part)")
    assert (got == 0).all()
    for b in (cs, wb, zb):
        b.free()


@pytest.mark.parametrize("log_n,n_routed,n_constants,nc,with_gates", [(4, 8, 0, 1, False), (6, 20, 3, 2, True), (7, 80, 3, 4, True),
                                                                      (8, 80, 5, 2, False), (5, 80, 2, 1, True)])
def test_quotient_permutation_edge_challenges(ctx, log_n, n_routed, n_constants, nc, with_gates):
    """a non-vanishing case: E wires and sigmas, E-valued alpha, beta and gamma, E-valued gate terms; against the oracle"""
    n = 1 << log_n
    wires_v, sig_v = eo.patterns(n_routed + 4, n), eo.patterns(n_routed + 5, n)[5:].copy()
    const_v = eo.constant_columns(n_constants, n, offset=4)
    betas = [eo.E[(3 + 2 * c) % 13] for c in range(nc)]
    gammas = [eo.E[(6 + 5 * c) % 13] for c in range(nc)]
    alphas = [eo.E[(9 + 7 * c) % 13] for c in range(nc)]
    sig_v = eo.avoid_zero_denominators(wires_v[:n_routed], sig_v, betas, gammas)
    zs_v = orc.partial_products(wires_v[:n_routed], sig_v, betas, gammas)
    cs = ctx.commit_values(np.concatenate([const_v, sig_v]) if n_constants else sig_v)
    wb, zb = ctx.commit_values(wires_v), ctx.commit_values(zs_v)
    gate_nat = eo.patterns(nc, 8 * n) if with_gates else None
    gate_dev = _gate_terms_dev(gate_nat, log_n + 3) if with_gates else None
    got = ctx.quotient_permutation(cs, n_constants, wb, zb, n_routed, betas, gammas, alphas,
                                   gate_terms_dev=gate_dev.data_ptr() if with_gates else None)
    canonical(got, "quotient (permutation part)")
    want = orc.quotient_permutation(wb.coeffs()[:n_routed], cs.coeffs()[n_constants:], zb.coeffs(), betas, gammas, alphas, gate_terms=gate_nat)
    assert got.shape == want.shape and (got == want).all()
    for b in (cs, wb, zb):
        b.free()


# ---------- gate terms: every gate kernel arrangement ----------
# the defaults (the fused LDS-tile kernel where the gate set fits a tile plan), one launch per gate type on one stream (gates_tile = 0 and
# gates_fused = 0), and the three-stream lanes with their join sum -- which run only where the fused kernel does not, hence gates_tile = 0
ARRANGEMENTS = [{}, {"gates_tile": 0}, {"gates_fused": 0}, {"gate_lanes": 3}, {"gates_tile": 0, "gate_lanes": 3}]


def _with_options(ctx, over, fn):
    defaults = {name: ctx.get_option(name) for name in ctx.OPTIONS}
    try:
        for name, v in over.items():
            ctx.set_option(name, v)
        return fn()
    finally:
        for name, v in defaults.items():
            ctx.set_option(name, v)


@pytest.mark.parametrize("over", ARRANGEMENTS, ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()) or "defaults")
@pytest.mark.parametrize("spec", [ALL, SMALL_VARIANTS + ["noop"]], ids=["all14", "small_variants"])
def test_gate_terms_on_constant_edge_columns(ctx, over, spec):
    """wire and constant columns constant per column with values from E (so every LDE point is an edge value), the selector columns set to
    one gate's selector values at a time (every filter is hit), alpha and pi_hash from E: device == gates_oracle, bit for bit"""
    import torch
    log_n = 3
    n = 1 << log_n
    gs, ps = go.GateSet(spec), api.GateSet(spec)
    n_const = gs.num_selectors + gs.num_constants
    out = torch.zeros((2, 8 * n), dtype=torch.int64, device="cuda")

    def run():
        for gi, gate in enumerate(gs.gates):
            consts = eo.constant_columns(n_const + 3, n, offset=gi)
            consts[:gs.num_selectors] = np.array(gs.selector_values(gate), np.uint64)[:, None]
            wires = eo.constant_columns(135, n, offset=3 * gi)
            pi_hash = [eo.E[(gi + k) % 13] for k in range(4)]
            alphas = [eo.E[(5 + gi) % 13], eo.E[(11 + 2 * gi) % 13]]
            cs, wb = ctx.commit_values(consts), ctx.commit_values(wires)
            out.zero_()
            torch.cuda.synchronize()
            ctx.gate_terms(cs, wb, ps, pi_hash, alphas, out.data_ptr())
            ctx.synchronize()
            got = _leaf_order(out.cpu().numpy().view(np.uint64), log_n + 3)   # bit reversal is its own inverse
            canonical(got, "gate kernels %r (gate %s)" % (over, gate.kind))
            want = gs.terms_coset(cs.coeffs()[:n_const], wb.coeffs(), pi_hash, alphas)
            assert (got == want).all(), (over, gi, gate.kind)
            cs.free(); wb.free()
    _with_options(ctx, over, run)


# ---------- FRI ----------
def _fri_edge_case(ctx, log_n, kind):
    """four oracles as in tests/test_gpu_parity.py _fri_case, with zero / constant (every FRI codeword 0) or E-coefficient polynomials"""
    cols = (4, 6, 3, 2)
    n = 1 << log_n
    if kind == "zero":
        datas = [np.zeros((c, n), np.uint64) for c in cols]
    elif kind == "const":
        datas = [eo.constant_columns(c, n, offset=3 * i) for i, c in enumerate(cols)]
        datas[3] = np.zeros((cols[3], n), np.uint64); datas[3][:, 0] = [eo.E[5], eo.E[9]]   # coefficients of constants
    else:
        datas = [eo.patterns(c, n) for c in cols]
    o_batches = [orc.Batch(d, 3, 4, from_values=(i != 3)) for i, d in enumerate(datas)]
    g_batches = [(ctx.commit_values if i != 3 else ctx.commit_coeffs)(d) for i, d in enumerate(datas)]
    ch = orc.ChallengerState()
    for o in o_batches:
        ch.observe(o.cap())
    zeta = ch.get_ext()
    batches, zeta_next = step_oracle.step_batches(list(cols), 2, zeta, log_n)
    openings = np.concatenate([o.eval_ext(zeta) for o in o_batches] + [o_batches[2].eval_ext(zeta_next)[:2]])
    ch.observe(openings)
    gch = api.ChallengerState()
    for o in g_batches:
        gch.observe(o.cap())
    assert list(gch.get_ext()) == list(zeta)
    gch.observe(openings)
    return o_batches, g_batches, ch, gch, batches, openings


@pytest.mark.parametrize("log_n", [5, 9, 12])
@pytest.mark.parametrize("kind", ["zero", "const", "edge"])
@pytest.mark.parametrize("wide_threshold", [None, 0])
def test_fri_on_edge_polynomials(ctx, log_n, kind, wide_threshold):
    """the combine step, the division by (X - zeta), the folds and the query gathers with polynomials whose FRI codewords are 0 (zero and
    constant columns: every f - f(zeta) vanishes) or E walks: proof, verifier and final challenger state equal the oracle's"""
    ob, gb, ch, gch, batches, openings = _fri_edge_case(ctx, log_n, kind)
    ch_v = ch.clone()
    op, gp = orc.fri_params(log_n), api.fri_params(log_n)

    def run():
        return ctx.fri_prove(gb, batches, gch, gp)
    got = run() if wide_threshold is None else _with_options(ctx, {"wide_threshold": wide_threshold}, run)
    canonical(got[:-1], "FRI (combine / divide / fold / open kernels)")
    want = orc.prove_openings(ob, batches, ch, op, log_n)
    assert got.shape == want.shape and (got == want).all()
    assert gch.state_words() == ch.state_words()
    total = sum(o.ncols for o in ob)
    assert orc.verify_fri([o.cap() for o in ob], [o.ncols for o in ob], batches, [openings[:total], openings[total:]], ch_v, op, log_n, got)
    for b in gb:
        b.free()


# ---------- a whole step proof with gates on edge columns ----------
@pytest.mark.parametrize("kind", ["const", "zero_pminus1"])
def test_step_proof_with_gates_on_edge_wires(ctx, kind):
    """the circuit of test_context_options_choose_between_bit_identical_arrangements with its wires replaced by constant E columns or by
    columns of {0, p - 1} (the witness need not satisfy the circuit): every stage on the device against the oracle prover"""
    gate_spec = ["noop", "constant", "public_input", "arithmetic", "base_sum", "poseidon", "reducing", ("random_access", 4), "coset_interpolation"]
    gs, ps = go.GateSet(gate_spec), api.GateSet(gate_spec)
    rnd = random.Random(5)
    log_c = 7
    n = 1 << log_c
    cpis = [rnd.randrange(P) for _ in range(4)]
    constants, wires, sigma, _ = go.demo_circuit(rnd, gs, log_c, cpis)
    if kind == "const":
        wires = eo.constant_columns(135, n, offset=1)
    else:
        wires = np.where(eo.patterns(135, n) % np.uint64(2) == 0, np.uint64(0), np.uint64(P - 1)).astype(np.uint64)
    nconst = constants.shape[0]
    cs_values = np.concatenate([constants, sigma])
    want = step_oracle.prove_step({"constants_sigmas": cs_values, "wires": wires, "quotient": None}, DIGEST, cpis, log_c, sigmas=sigma,
                                  n_routed=80, n_constants=nconst, gates=gs)
    cs = ctx.commit_values(cs_values)
    si = ctx.make_step_inputs(log_c, wires, None, None, cs, DIGEST, cpis, sigmas=sigma, n_routed=80, n_constants=nconst, gates=ps)
    for over in ARRANGEMENTS:
        got = _with_options(ctx, over, lambda: ctx.prove_step(si))
        for key in ("caps", "challenges", "openings", "fri"):
            canonical(got[key], "step proof %r: %s" % (over, key))
            assert (got[key] == want[key]).all(), (over, key)
    cs.free()


# ---------- TFHE step: br_decompose_ntt_kernel / br_mac_intt_kernel, negacyclic_kernel ----------
@pytest.mark.parametrize("K,ELL,LOGB", [(2, 8, 8), (2, 4, 4), (2, 4, 5), (3, 3, 7)])
def test_blind_rotate_step_on_boundaries(ctx, K, ELL, LOGB):
    """N = 8: one instance per mask on a mod-switch boundary (0, p - 1 = shift 2N, every multiple of 2^59 and its neighbours: the rounding
    ties and the truncation boundaries), with the decomposition-boundary values (tb = 64 with the sign path at LOGB 4 / 8, 65 at LOGB 5, 70
    at LOGB 7) where the decomposer reads them: the last step decomposes the accumulator itself, a normal step rotate(acc) - acc, so there
    the accumulator is derived to make that difference the boundary values (except at shift 0 / 2N, where it is 0); the first step only
    rotates.  Against tfhe_oracle.step"""
    import tfhe_oracle as T
    log_N = 3
    N = 1 << log_N
    ring = T.Ring(log_N)
    masks = eo.mask_boundaries(log_N)
    bvals = eo.decomposition_boundaries(LOGB)
    B = len(masks)
    acc = np.stack([eo.pattern(K * N, 3 * b, 1, bvals).reshape(K, N) for b in range(B)])
    derived = acc.copy()
    for b in range(B):
        for p in range(K):
            a = eo.acc_for_difference(acc[b][p], T.mod_switch(masks[b], log_N))
            if a is not None:
                assert [(x - y) % P for x, y in zip(T.rotate(a, T.mod_switch(masks[b], log_N)), a)] == [int(v) for v in acc[b][p]]
                derived[b][p] = a
    ggsw = eo.pattern(K * ELL * K * N, 0, 5, eo.E_ROOTS)
    hat = [[[list(map(int, ggsw[((p * ELL + l) * K + r) * N:((p * ELL + l) * K + r + 1) * N])) for r in range(K)] for l in range(ELL)]
           for p in range(K)]
    for first, last, a_in in ((False, False, derived), (False, False, acc), (True, False, acc), (False, True, acc)):
        got = ctx.blind_rotate_step(a_in, masks, ggsw, K, ELL, LOGB, first_step=first, last_step=last)
        canonical(got, "br_decompose_ntt_kernel / br_mac_intt_kernel")
        for b in range(B):
            want = T.step(ring, [list(map(int, a_in[b][p])) for p in range(K)], masks[b], hat, K, ELL, LOGB, first, last)
            assert [[int(v) for v in got[b][p]] for p in range(K)] == want, (first, last, b, hex(masks[b]))


@pytest.mark.parametrize("log_N", [3, 4, 5, 6, 7, 8, 9, 10, 11])   # every tests/golden/ntt_params_*.json size
def test_negacyclic_ntt_to_edge_values(ctx, log_N):
    """forward and inverse negacyclic transforms whose OUTPUTS are E walks (inputs derived with the oracle's other direction)"""
    N = 1 << log_N
    roots, inv, ninv = orc.negacyclic_params(log_N)
    target = eo.patterns(3, N)
    fw_in = np.stack([orc.negacyclic_backward(t, inv, ninv) for t in target])
    got = ctx.negacyclic_ntt(fw_in)
    canonical(got, "negacyclic_kernel (forward)")
    assert (got == target).all()
    assert all((orc.negacyclic_forward(fw_in[c], roots) == target[c]).all() for c in range(3))
    bw_in = np.stack([orc.negacyclic_forward(t, roots) for t in target])
    got = ctx.negacyclic_ntt(bw_in, inverse=True)
    canonical(got, "negacyclic_kernel (inverse)")
    assert (got == target).all()


# ---------- device witness: the wd_* kernels of witness_device.hip ----------
def _edge_witness(ctx, spec, log_n):
    """the demo circuit over `spec` with every free preset taken from E (edge_operands.legal_preset) and E public inputs; the Poseidon row
    that hashes the public inputs keeps its zero padding, which is circuit structure.  Two instances with different E walks, run by the
    device witness generator -> (gate set, circuit, plan, WitnessDevice, preset columns, pi hashes)"""
    import test_gates_cpu as tg
    n = 1 << log_n
    gs, ps = go.GateSet(spec), api.GateSet(spec)
    constants, wires, _, _, desc = go.demo_circuit(random.Random(404), gs, log_n, [eo.E[k] for k in (3, 5, 9, 11)], describe=True)
    circ = api.Circuit(ps, log_n, desc["row_gate"], constants, desc["copies"])
    generated = set()
    for row in range(n):
        generated |= {(w, row) for w in tg._owned_wires(gs.gates[int(desc["row_gate"][row])])}
    fed = set()
    for cl in desc["classes"]:
        if any(tuple(x) in generated for x in cl):
            fed |= {tuple(x) for x in cl}
    positions = []
    for row in range(n):
        g = gs.gates[int(desc["row_gate"][row])]
        if g.kind != "public_input":
            positions += [(w, row) for w in tg._free_inputs(g) if (w, row) not in fed]
    columns, pi_hashes = [], []
    for off in (0, 7):
        vals = [int(wires[w, row]) if (row == 1 and w >= 4) else eo.legal_preset(gs.gates[int(desc["row_gate"][row])], w, eo.E[(off + k) % 13])
                for k, (w, row) in enumerate(positions)]
        columns.append(vals)
        pi_hashes.append(orc.hash_no_pad([vals[positions.index((i, 1))] for i in range(4)]))   # row 1 absorbs the public inputs
    plan = circ.witness_plan(positions)
    dev = api.WitnessDevice(ctx, plan, max_batch=2)
    dev.run(np.ascontiguousarray(np.array(columns, dtype=np.uint64).T))
    return gs, circ, plan, dev, columns, pi_hashes


def test_device_witness_with_edge_presets(ctx):
    """test_device_witness_for_every_gate_type (tests/test_gpu_gates.py) with every free preset taken from E instead of at random -- the
    largest legal value where a generator has a range (edge_operands.legal_preset) -- and E public inputs.  Two instances with different E
    walks in one batch: the device wires (wd_preset / wd_const / wd_arith / wd_bits / wd_rowop / wd_poseidon / wd_misc / wd_walk / wd_column
    kernels) equal the host plan's witness and satisfy every constraint"""
    import torch
    log_n = 7
    n = 1 << log_n
    gs, circ, plan, dev, columns, pi_hashes = _edge_witness(ctx, ALL, log_n)
    d_w = torch.zeros((135, n), dtype=torch.int64, device="cuda")
    for i in range(2):
        dev.wires(i, d_w.data_ptr())
        got = d_w.cpu().numpy().view(np.uint64)
        canonical(got, "wd_* kernels (instance %d)" % i)
        want = plan.run(columns[i])
        assert (got == want).all(), np.argwhere(got != want)[:5]
        ok, msg = circ.check_witness(got, pi_hashes[i])
        assert ok, msg
    dev.free(); plan.free()


WITNESS_SETS = [(ALL, 7), (SMALL_VARIANTS + ["noop", "public_input", "poseidon"], 6)]


@pytest.mark.parametrize("spec,log_n", WITNESS_SETS, ids=["all14", "small_variants"])
def test_device_checker_on_edge_witnesses(ctx, spec, log_n):
    """the device witness checker (api.WitnessChecker) on the edge-valued witnesses above: it accepts them from host arrays and as the wires
    WitnessDevice leaves in HBM; then one cell of every used row replaced by another E value: the device's (ok, message) is the host
    checker's, exactly"""
    import torch
    n = 1 << log_n
    gs, circ, plan, dev, columns, pi_hashes = _edge_witness(ctx, spec, log_n)
    chk = api.WitnessChecker(ctx, circ)
    d_w = torch.zeros((135, n), dtype=torch.int64, device="cuda")
    noop = gs.by_kind("noop").index
    changed = 0
    for i in range(2):
        host = plan.run(columns[i])
        h = pi_hashes[i]
        assert chk.check(host, h) == (True, "") == circ.check_witness(host, h)
        dev.wires(i, d_w.data_ptr())
        ctx.synchronize()
        assert chk.check(d_w.data_ptr(), h) == (True, "")
        if i == 0:
            continue
        for row in range(n):
            if int(circ.row_gate[row]) == noop:
                continue
            for k in range(2):
                col = (11 * row + 37 * k) % gs.gates[int(circ.row_gate[row])].num_wires
                w = host.copy()
                cur = int(w[col, row])
                j = eo.E.index(cur) if cur in eo.E else row % len(eo.E)
                w[col, row] = eo.E[(j + 1 + k) % len(eo.E)]
                want = circ.check_witness(w, h)
                assert chk.check(w, h) == want, (row, col, want)
                changed += 1
    assert changed >= 40, changed
    chk.free(); dev.free(); plan.free()
