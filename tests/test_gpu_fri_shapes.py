"""GPU tests (-m gpu): FRI proofs, commitments and step proofs OFF the standard configuration -- other arity lists, rates and cap heights,
many rounds, the smallest trees, many polynomials, one and 128 query rounds (fri_shapes.py) -- against the CPU oracle on identical inputs,
and the parameter sets the library refuses as a whole.  Every comparison is exact equality of uint64 words.  Nothing here exceeds
log_n = 9; besides the module's standard context at most one more context is alive at a time, closed in a `finally`."""
import contextlib
import ctypes

import numpy as np
import pytest

import fri_shapes
import oracle as orc
import step_oracle
import vpbs_amd
from vpbs_amd import api, synth

pytestmark = pytest.mark.gpu
P = api.P
DIGEST = np.array([11, 22, 33, 44], np.uint64)
# the arrangements of the tree kernels: wide_threshold = 0 selects the one-lane leaf and level kernels (the only way the multi-block narrow
# leaf kernel runs at these sizes), merkle_climb = 0 one launch per level
ARRANGEMENTS = [{}, {"wide_threshold": 0}, {"merkle_climb": 0}]


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=10)
    yield c
    c.close()


@contextlib.contextmanager
def _context(ctx, rate, cap_h):
    """the module's context for the standard configuration, otherwise a context of this shape that lives for the block"""
    if (rate, cap_h) == (3, 4):
        yield ctx
        return
    c = vpbs_amd.Context(0, log_n_max=10, rate_bits=rate, cap_height=cap_h)
    try:
        yield c
    finally:
        c.close()


def _with_options(ctx, over, fn):
    defaults = {name: ctx.get_option(name) for name in ctx.OPTIONS}
    try:
        for name, v in over.items():
            ctx.set_option(name, v)
        return fn()
    finally:
        for name, v in defaults.items():
            ctx.set_option(name, v)


def _fri_case(ctx, log_n, cols, seed, rate=3, cap_h=4, **over):
    """test_gpu_parity._fri_case with the context's rate and cap height: the fourth batch is committed from coefficients"""
    gen = np.random.default_rng(seed)
    datas = [gen.integers(0, P, size=(nc, 1 << log_n), dtype=np.uint64) for nc in cols]
    o_batches = [orc.Batch(d, rate, cap_h, from_values=(i != 3)) for i, d in enumerate(datas)]
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
    over = dict(over, rate_bits=rate, cap_height=cap_h)
    return o_batches, g_batches, ch, gch, batches, openings, orc.fri_params(log_n, **over), api.fri_params(log_n, **over)


def _assert_fri_bit_exact(ctx, log_n, cols, seed, rate=3, cap_h=4, arrangements=ARRANGEMENTS, **over):
    """the three assertions of test_fri_prove_bit_exact under every arrangement; the reference is computed once"""
    ob, gb, ch, gch, batches, openings, op, gp = _fri_case(ctx, log_n, cols, seed, rate, cap_h, **over)
    try:
        ch_v = ch.clone()
        want = orc.prove_openings(ob, batches, ch, op, log_n)
        total = sum(o.ncols for o in ob)
        caps, ncols = [o.cap() for o in ob], [o.ncols for o in ob]
        for arrangement in arrangements:
            g = gch.clone()
            got = _with_options(ctx, arrangement, lambda: ctx.fri_prove(gb, batches, g, gp))
            assert got.shape == want.shape, arrangement
            assert (got == want).all(), (arrangement, int(np.flatnonzero(got != want)[0]))
            assert g.state_words() == ch.state_words(), arrangement
            assert orc.verify_fri(caps, ncols, batches, [openings[:total], openings[total:]], ch_v.clone(), op, log_n, got), arrangement
    finally:
        for b in gb:
            b.free()


# ---------- 1. FRI, every shape ----------
@pytest.mark.parametrize("shape", fri_shapes.FRI_SHAPES, ids=fri_shapes.shape_id)
def test_fri_prove_bit_exact_at_every_shape(ctx, shape):
    log_n, rate, cap_h, bits = shape
    with _context(ctx, rate, cap_h) as c:
        _assert_fri_bit_exact(c, log_n, fri_shapes.FRI_COLS, 1000 + fri_shapes.FRI_SHAPES.index(shape), rate, cap_h, arity_bits=bits)


# ---------- 2. polynomial and query counts ----------
@pytest.mark.parametrize("cols", fri_shapes.POLY_COUNTS, ids=lambda c: "%d_polys" % sum(c))
def test_fri_prove_bit_exact_at_the_combine_group_counts(ctx, cols):
    """launch_combine: one group below 64 polynomials, 16 groups from 64 on -- 64 and 65 leave trailing groups empty, 241 a ragged last one"""
    _assert_fri_bit_exact(ctx, fri_shapes.POLY_COUNT_LOG_N, cols, 2000 + sum(cols), arrangements=[{}])


@pytest.mark.parametrize("nq", fri_shapes.QUERY_COUNTS)
def test_fri_prove_bit_exact_at_the_query_count_limits(ctx, nq):
    _assert_fri_bit_exact(ctx, fri_shapes.QUERY_COUNT_LOG_N, fri_shapes.FRI_COLS, 3000 + nq, arrangements=[{}],
                          pow_bits=fri_shapes.QUERY_COUNT_POW_BITS, num_query_rounds=nq)


# ---------- 3. commitments ----------
@pytest.mark.parametrize("rate,cap_h", fri_shapes.RATE_CAPS)
def test_commit_matches_oracle_at_every_rate_and_cap(ctx, rate, cap_h):
    """the assertions of test_commit_matches_oracle on a context of every (rate_bits, cap_height) of the two tables"""
    gen = np.random.default_rng(5000 + 16 * rate + cap_h)
    with _context(ctx, rate, cap_h) as c:
        for log_n in (5, 8):
            if log_n + rate < cap_h:
                continue
            for from_values in (True, False):
                data = gen.integers(0, P, size=(3, 1 << log_n), dtype=np.uint64)
                data[0] = P - 1
                want = orc.Batch(data, rate, cap_h, from_values=from_values)
                got = (c.commit_values if from_values else c.commit_coeffs)(data)
                try:
                    assert got.cap_at_commit.shape == (1 << cap_h, 4)
                    assert (got.cap_at_commit == want.cap()).all() and (got.cap() == want.cap()).all()
                    assert (got.coeffs() == want.coeffs()).all()
                    L = 1 << (log_n + rate)
                    for idx in (0, 1, L // 2 + 3, L - 1):
                        leaf, sib = got.open(idx)
                        wleaf, wsib = want.open(idx)
                        assert sib.shape == (log_n + rate - cap_h, 4)
                        assert (leaf == wleaf).all() and (sib == wsib).all(), (log_n, from_values, idx)
                    rows = got.lde_rows(3, 5, step=2)
                    for k in range(5):
                        assert (rows[k] == want.lde_row(3 + k, 2)).all()
                    zeta = gen.integers(0, P, size=2, dtype=np.uint64)
                    assert (got.eval_ext(zeta) == want.eval_ext(zeta)).all()
                finally:
                    got.free()


# ---------- 4. step proofs ----------
N_CONSTANTS = 2
TAMPERINGS = ("cap word", "final-polynomial word", "last sibling of the last query")


def _tampered(proof, which, log_n, rounds):
    bad = {k: np.array(proof[k], np.uint64, copy=True) for k in ("caps", "openings", "fri")}
    final_words = 2 << (log_n - 4 * rounds)
    key, pos = {"cap word": ("caps", 5), "final-polynomial word": ("fri", bad["fri"].size - 2),
                "last sibling of the last query": ("fri", bad["fri"].size - 2 - final_words)}[which]
    flat = bad[key].reshape(-1)
    flat[pos] = (int(flat[pos]) + 1) % P
    return bad


def _step_case(c, log_n, rate, cap_h, rounds):
    """-> (device proof, oracle proof, public inputs, serialised device proof, verdicts and reasons of the device verifier for the proof and its
    three tampered copies)"""
    inputs = synth.step_inputs(log_n, cols=fri_shapes.STEP_COLS)
    pis = synth.field_elements(0xABCD, 11)
    cs = c.commit_values(inputs["constants_sigmas"])
    si = c.make_step_inputs(log_n, inputs["wires"], inputs["zs_partial_products"], inputs["quotient"], cs, DIGEST, pis)
    got = c.prove_step(si)
    want = step_oracle.prove_step(inputs, DIGEST, pis, log_n, rate_bits=rate, cap_height=cap_h)
    blob = c.step_proof_to_bytes(si, N_CONSTANTS, got)
    blobs = [blob] + [step_oracle.to_bytes(_tampered(got, t, log_n, rounds), want["ncols"], N_CONSTANTS, pis, log_n, cap_height=cap_h,
                                           rate_bits=rate) for t in TAMPERINGS]
    v = api.ProofVerifier(c, want["cs_cap"], want["ncols"], DIGEST, log_n, check_permutation=False, rate_bits=rate, cap_height=cap_h,
                          max_batch=4, max_public_inputs=16)
    try:
        verdicts, reasons = v.verify(blobs)
    finally:
        v.close()
        cs.free()
    return got, want, pis, blob, [int(x) for x in verdicts], [int(x) for x in reasons]


@pytest.fixture(scope="module")
def control_reasons(ctx):
    """what a ProofVerifier on the standard context says about the (6, 3, 4) control and its three tampered copies"""
    (log_n, rate, cap_h), rounds = fri_shapes.STEP_SHAPES[0]
    assert (log_n, rate, cap_h) == (6, 3, 4)
    *_, verdicts, reasons = _step_case(ctx, log_n, rate, cap_h, rounds)
    assert verdicts == [1, 0, 0, 0] and reasons[0] == api.VERIFY_OK and all(r != api.VERIFY_OK for r in reasons[1:])
    return reasons


@pytest.mark.parametrize("shape,rounds", fri_shapes.STEP_SHAPES, ids=lambda v: "n%d-r%d-c%d" % v if isinstance(v, tuple) else None)
def test_step_proof_bit_exact_at_every_step_shape(ctx, control_reasons, shape, rounds):
    log_n, rate, cap_h = shape
    with _context(ctx, rate, cap_h) as c:
        got, want, pis, blob, verdicts, reasons = _step_case(c, log_n, rate, cap_h, rounds)
    ncols = want["ncols"]
    assert got["caps"].shape == want["caps"].shape == (3, 1 << cap_h, 4)
    for key in ("caps", "challenges", "openings", "fri"):
        assert got[key].shape == want[key].shape and (got[key] == want[key]).all(), key
    assert got["challenger"].state_words() == want["challenger"].state_words()
    assert blob == step_oracle.to_bytes(want, ncols, N_CONSTANTS, pis, log_n, cap_height=cap_h, rate_bits=rate)
    back, back_pis = api.step_proof_from_bytes(blob, ncols, log_n, N_CONSTANTS, rate_bits=rate, cap_height=cap_h)
    assert all((back[k].reshape(-1) == got[k].reshape(-1)).all() for k in ("caps", "openings", "fri")) and (back_pis == pis).all()
    assert step_oracle.verify_step(got, want["cs_cap"], ncols, DIGEST, pis, log_n, rate_bits=rate, cap_height=cap_h)
    assert api.verify_step_fri_only(got, want["cs_cap"], ncols, DIGEST, pis, log_n, rate_bits=rate, cap_height=cap_h)
    # the device verifier: the proof accepted, each tampered copy rejected for the reason the control's copy is rejected for
    assert verdicts == [1, 0, 0, 0], (verdicts, reasons)
    assert reasons == control_reasons, dict(zip(("proof",) + TAMPERINGS, zip(reasons, control_reasons)))
    # ... and the host verifier rejects the same three copies
    for t in TAMPERINGS:
        assert not api.verify_step_fri_only(_tampered(got, t, log_n, rounds), want["cs_cap"], ncols, DIGEST, pis, log_n, rate_bits=rate,
                                            cap_height=cap_h), t


# ---------- 5. refusals ----------
SENTINEL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def standard_case(ctx):
    """the standard proof of log_n = 6: committed batches, challenger states and the oracle's proof, shared by the refusal tests"""
    ob, gb, ch, gch, batches, openings, op, gp = _fri_case(ctx, 6, fri_shapes.FRI_COLS, 6000)
    want = orc.prove_openings(ob, batches, ch, op, 6)
    yield gb, gch, batches, gp, want, ch
    for b in gb:
        b.free()


def _assert_refused_untouched(ctx, case, params, gb=None):
    gb_std, gch, batches, gp, want, ch = case
    gb = gb if gb is not None else gb_std
    # a buffer sized for the nearest valid shape (the standard parameters at this degree), pre-filled: the refusal comes before any write
    sizes = (ctypes.c_size_t * 4)(*[b.ncols for b in gb])
    ok = api.fri_params(gb[0].log_n)
    buf = np.full(api.lib().vpbs_fri_proof_words(ctypes.byref(ok), gb[0].log_n, sizes, 4), SENTINEL, np.uint64)
    g = gch.clone()
    with pytest.raises(api.VpbsError) as e:
        ctx.fri_prove(gb, batches, g, params, proof_out=buf)
    assert e.value.status == api.ERR_INVALID, str(e.value)
    assert (buf == SENTINEL).all(), "a refused call wrote to the proof buffer"
    assert g.state_words() == gch.state_words(), "a refused call drew from the challenger"
    # the Python wrapper sizes the proof by vpbs_fri_proof_words and must refuse as well (a count of 0 is not a size to allocate)
    with pytest.raises(api.VpbsError) as e:
        ctx.fri_prove(gb, batches, gch.clone(), params)
    assert e.value.status == api.ERR_INVALID, str(e.value)
    # afterwards the same context still produces the bit-exact standard proof of log_n = 6
    g = gch.clone()
    got = ctx.fri_prove(gb_std, batches, g, gp)
    assert (got == want).all() and g.state_words() == ch.state_words()


@pytest.mark.parametrize("name,log_n,over", [r for r in fri_shapes.REFUSED_SHAPES if r[1] == 6],
                         ids=[r[0].replace(" ", "_") for r in fri_shapes.REFUSED_SHAPES if r[1] == 6])
def test_refused_fri_parameters_reach_no_kernel(ctx, standard_case, name, log_n, over):
    _assert_refused_untouched(ctx, standard_case, api.fri_params(log_n, **over))


def test_refused_tree_count_reaches_no_kernel(ctx, standard_case):
    """(10, 3, 4, [1] * 9): 4 + 9 = 13 trees, one more than the query kernel's argument block holds"""
    (name, log_n, over), = [r for r in fri_shapes.REFUSED_SHAPES if r[1] != 6]
    gen = np.random.default_rng(6100)
    gb = [(ctx.commit_values if i != 3 else ctx.commit_coeffs)(gen.integers(0, P, size=(nc, 1 << log_n), dtype=np.uint64))
          for i, nc in enumerate(fri_shapes.FRI_COLS)]
    try:
        _assert_refused_untouched(ctx, standard_case, api.fri_params(log_n, **over), gb)
    finally:
        for b in gb:
            b.free()


@pytest.mark.parametrize("over", [{"rate_bits": 2}, {"cap_height": 3}, {"rate_bits": 4, "cap_height": 0}], ids=lambda o: "-".join("%s=%d" % kv for kv in o.items()))
def test_params_of_another_configuration_are_refused(ctx, standard_case, over):
    """params whose rate_bits or cap_height differ from the context's have a word count of their own, so only vpbs_fri_prove can refuse"""
    gb, gch, batches, gp, want, ch = standard_case
    params = api.fri_params(6, **over)
    buf = np.full(2 * want.size, SENTINEL, np.uint64)
    g = gch.clone()
    with pytest.raises(api.VpbsError) as e:
        ctx.fri_prove(gb, batches, g, params, proof_out=buf)
    assert e.value.status == api.ERR_INVALID and (buf == SENTINEL).all() and g.state_words() == gch.state_words()
    g = gch.clone()
    assert (ctx.fri_prove(gb, batches, g, gp) == want).all() and g.state_words() == ch.state_words()
