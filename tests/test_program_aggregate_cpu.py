"""One proof per program instance, the host side: api.program_gate_inputs against the restatement of what a verifier of a
program recomputes (tests/multi_lut_oracle.py: wires_of + gate_inputs), api.program_aggregate_root against api.aggregate_root over those gate
inputs and against the Python model of tests/test_aggregate_cpu.py, single-word flips of every part of the statement, and the refusals with
their messages.  Nothing here needs a device: the programs are host-only.  The GPU twin is tests/test_gpu_program_aggregate.py."""
import random

import numpy as np
import pytest

import cyclic_circuit as cc
import multi_lut_oracle as M
import test_aggregate_cpu as TA
from vpbs_amd import api

P = api.P
NAMES = ["vpbs_program_gate_inputs", "vpbs_program_aggregate_root", "vpbs_program_verify_aggregate", "vpbs_program_prove_aggregate",
         "vpbs_program_prove_aggregate_batch", "vpbs_program_verify_aggregate_batch", "vpbs_aggregate_verifier_create_many",
         "vpbs_aggregate_verifier_run_many", "vpbs_aggregate_verifier_roots_many"]
# the program of tests/test_gpu_multi_lut.py: plain, multi-output and snapped gates, a negative coefficient, a constant; 2 inputs, 9 wires
FOUR = [([(0, 1)], 0, 0, 1, 2), ([(1, 1), (0, P - 1)], 7, 1, 2, 3), ([(3, 1), (6, P - 1)], 0, 0), ([(2, 1), (4, 3)], 0, 1, 1, 1)]
# plain gates only (lwe_extract's rows), every input read, a gate without terms
PLAIN = [([(0, 1), (1, 2)], 0, 0), ([], 5, 1), ([(2, P - 1), (3, 1)], 9, 1)]
# the last gate reads an input together with outputs of two different levels (gate 0: level 1, gate 1: level 2): plain, and with the
# outputs of multi-output gates that are not their gate's first
DEEP = [([(0, 1)], 0, 0), ([(2, 1), (1, 2)], 3, 1), ([(0, P - 1), (2, 5), (3, 1)], 1, 0)]
DEEP_MULTI = [([(0, 1)], 0, 0, 1, 2), ([(3, 1), (1, 2)], 3, 1, 2, 3), ([(1, P - 1), (3, 5), (6, 1)], 1, 0, 1, 1)]


def test_library_exports_the_entry_points_and_api_binds_them():
    L = api.lib()
    for name in NAMES:
        assert name in api.SIGNATURES, name
        fn = getattr(L, name)
        assert fn.argtypes == api.SIGNATURES[name][1] and fn.restype == api.SIGNATURES[name][0]
    for f in (api.program_gate_inputs, api.program_aggregate_root, api.program_verify_aggregate, api.Program.prove_aggregate,
              api.Program.prove_aggregate_batch, api.Program.verify_aggregate_batch, api.AggregateVerifier.verify_many,
              api.AggregateVerifier.roots_many):
        assert callable(f)


def statement(seed, gates, n_inputs, log_n, K, n, instances=None):
    """random inputs (words up to 2^64 - 1: reduced on read), claimed outputs and test vectors below p"""
    rng = np.random.default_rng(seed)
    N, lead = 1 << log_n, () if instances is None else (instances,)
    inputs = rng.integers(0, 1 << 64, size=lead + (n_inputs, n + 1), dtype=np.uint64)
    out_cts = rng.integers(0, P, size=lead + (len(gates), K, N), dtype=np.uint64)
    testvs = rng.integers(0, P, size=(2, N), dtype=np.uint64)
    return inputs, out_cts, testvs


def want_gate_inputs(gates, n_inputs, inputs, out_cts, n, log_n):
    wires = M.wires_of(inputs, gates, out_cts, n)
    return M.gate_inputs(n_inputs, gates, wires, n + 1, log_n)


@pytest.mark.parametrize("gates,log_n,K,n", [(FOUR, 3, 2, 6), (FOUR, 3, 3, 12), (PLAIN, 3, 2, 6), (PLAIN, 2, 3, 5), (DEEP, 2, 3, 5),
                                             (DEEP_MULTI, 3, 2, 6)])
def test_gate_inputs_against_the_restatement(gates, log_n, K, n):
    """(3, 3, 12) and (2, 3, 5): the extraction crosses a polynomial; input words p - 1, p and 2^64 - 1; two instances; a host-only program;
    DEEP and DEEP_MULTI: one gate reads an input and outputs of two levels"""
    N = 1 << log_n
    prog = api.Program(None, 2, gates, 2)
    inputs, out_cts, _ = statement(70 + K + n, gates, 2, log_n, K, n)
    inputs[0, 0], inputs[0, 1], inputs[1, n] = np.uint64(P - 1), np.uint64(P), np.uint64(2 ** 64 - 1)
    out_cts[0, 0, ::2] = 0                                   # the negation of 0 stays 0
    got = api.program_gate_inputs(prog, N, K, n, inputs, out_cts)
    assert got.shape == (len(gates), n + 1) and (got == want_gate_inputs(gates, 2, inputs, out_cts, n, log_n)).all()
    assert (got < np.uint64(P)).all()
    two_in, two_out, _ = statement(90 + K + n, gates, 2, log_n, K, n, instances=2)
    two_in[1], two_out[1] = inputs, out_cts
    both = api.program_gate_inputs(prog, N, K, n, two_in, two_out)
    assert both.shape == (2, len(gates), n + 1) and (both[1] == got).all()
    assert (both[0] == want_gate_inputs(gates, 2, two_in[0], two_out[0], n, log_n)).all()
    prog.close()


# ---- the root: N = 8, K = 2, n = 1, the shape of the Python model in tests/test_aggregate_cpu.py ----
N, K, N_LWE, LOG_N = TA.N, TA.K, TA.N_LWE, 3
# every input is read by a gate that does not snap (gate 3 reads both: a changed residue always shows), both test vectors are used, five
# gates: depth 3 with padding
FIVE = [([(0, 1), (1, P - 1)], 0, 0, 1, 2), ([(2, 1)], 3, 1), ([(1, 2), (3, 1)], 0, 0, 2, 3), ([(4, 1), (7, P - 2), (0, 3), (1, 1)], 1, 1), ([(0, 5)], 0, 0, 1, 1)]


def root_statement(seed):
    rng = np.random.default_rng(seed)
    inputs, out_cts, testvs = statement(seed, FIVE, 2, LOG_N, K, N_LWE)
    inputs %= np.uint64(P)
    return dict(vk0=rng.integers(0, P, size=68, dtype=np.uint64), inputs=inputs, testvs=testvs, out_cts=out_cts,
                key_hash=rng.integers(0, P, size=4, dtype=np.uint64))


def program_root(prog, s):
    return [int(v) for v in api.program_aggregate_root(prog, N, K, N_LWE, s["vk0"], s["inputs"], s["testvs"], s["out_cts"], s["key_hash"])]


def model_root(s, gates=FIVE):
    cts = want_gate_inputs(gates, 2, s["inputs"], s["out_cts"], N_LWE, LOG_N)
    leaves = [TA.model_leaf(s["vk0"], s["testvs"][g[2]], cts[i], s["out_cts"][i].reshape(-1), s["key_hash"]) for i, g in enumerate(gates)]
    return TA.model_root(leaves)


def test_the_root_is_aggregate_root_over_the_gate_inputs_and_the_models():
    prog = api.Program(None, 2, FIVE, 2)
    s = root_statement(21)
    cts = api.program_gate_inputs(prog, N, K, N_LWE, s["inputs"], s["out_cts"])
    lut = np.array([g[2] for g in FIVE], np.uint32)
    want = api.aggregate_root(N, K, N_LWE, s["vk0"], s["testvs"], cts, s["out_cts"].reshape(5, -1), s["key_hash"], testv_of=lut)
    got = program_root(prog, s)
    assert got == [int(v) for v in want] == model_root(s)
    # gate order matters: the same gates' statement with two leaves exchanged is another root
    other = api.aggregate_root(N, K, N_LWE, s["vk0"], s["testvs"], cts[[1, 0, 2, 3, 4]], s["out_cts"].reshape(5, -1)[[1, 0, 2, 3, 4]], s["key_hash"],
                               testv_of=lut[[1, 0, 2, 3, 4]])
    assert [int(v) for v in other] != got
    # one gate: the leaf folded with itself
    one = api.Program(None, 2, FIVE[:1], 2)
    t = dict(s, out_cts=s["out_cts"][:1])
    assert program_root(one, t) == model_root(t, FIVE[:1])
    one.close()
    prog.close()


def test_single_word_flips_of_the_statement_change_the_root():
    """single-word flips over inputs, out_cts, testvs and the key hash: every input is read by some gate and every flip changes the word's
    residue, so the model's root changes, and the host's root is the model's -- or the raw word left the field and the host refuses it"""
    prog = api.Program(None, 2, FIVE, 2)
    s = root_statement(22)
    base = program_root(prog, s)
    assert base == model_root(s)
    rnd = random.Random(6)
    for k in range(60):
        part = ["inputs", "out_cts", "testvs", "key_hash"][k % 4]
        t = dict(s)
        a = t[part] = s[part].copy()
        flat = a.reshape(-1)
        at = rnd.randrange(flat.size)
        old = int(flat[at])
        new = old ^ (1 << rnd.randrange(64))
        if part == "inputs" and new % P == old % P:
            new = (old + 1) % P
        flat[at] = np.uint64(new)
        if part != "inputs" and new >= P:
            with pytest.raises(api.VpbsError, match="not a field element"):
                program_root(prog, t)
            continue
        got = program_root(prog, t)
        assert got == model_root(t), (part, at)
        assert got != base, (part, at)
    prog.close()


def test_refusals_with_their_messages():
    prog = api.Program(None, 2, FIVE, 2)
    s = root_statement(23)
    # a shape without sample extraction: N no power of two, n_lwe = 0, n_lwe above (K - 1) N
    for n_, k_, lwe in ((6, 2, 1), (8, 2, 9), (8, 1, 1)):
        x, o = np.zeros((2, lwe + 1), np.uint64), np.zeros((5, k_, n_), np.uint64)
        with pytest.raises(api.VpbsError, match="no sample extraction"):
            api.program_gate_inputs(prog, n_, k_, lwe, x, o)
    with pytest.raises(api.VpbsError, match="no sample extraction"):
        api.program_aggregate_root(prog, 8, 1, 1, s["vk0"], s["inputs"], s["testvs"], np.zeros((5, 1, 8), np.uint64), s["key_hash"])
    # slots_fit: gate 0 packs 2^4 slots, the ring has N = 8
    wide = api.Program(None, 2, [([(0, 1)], 0, 0, 4, 2)], 2)
    with pytest.raises(api.VpbsError, match=r"gate 0: 2\^gate_log_slots = 2\^4 exceeds N = 8"):
        api.program_gate_inputs(wide, N, K, N_LWE, s["inputs"], s["out_cts"][:1])
    with pytest.raises(api.VpbsError, match=r"vpbs_program_aggregate_root: gate 0: .*exceeds N = 8"):
        api.program_aggregate_root(wide, N, K, N_LWE, s["vk0"], s["inputs"], s["testvs"], s["out_cts"][:1], s["key_hash"])
    wide.close()
    # too many gates for the verifier's shape: refused before the bytes are looked at, n_gates and 2^levels named
    level = cc.DummyCircuit(api, 5, 72).built           # any circuit gives a shape; none of it is reached
    shape = api.AggregateShape(N, K, N_LWE, np.zeros((3, 68), np.uint64), [level, level])
    with pytest.raises(api.VpbsError, match=r"n_gates 5 exceeds 2\^levels = 4"):
        api.program_verify_aggregate(prog, shape, b"\0" * 64, s["inputs"], s["testvs"], s["out_cts"], s["key_hash"])
    four = api.Program(None, 2, FIVE[:4], 2)
    # bytes that are no proof at all: MALFORMED, as verify_aggregate says it
    assert api.program_verify_aggregate(four, shape, b"\0" * 64, s["inputs"], s["testvs"], s["out_cts"][:4], s["key_hash"]) == (False, api.AGG_MALFORMED)
    four.close()
    # a program without gates has no aggregate
    none = api.Program(None, 2, [], 2)
    with pytest.raises(api.VpbsError, match="no gates"):
        api.program_aggregate_root(none, N, K, N_LWE, s["vk0"], s["inputs"], s["testvs"], np.zeros((0, K, N), np.uint64), s["key_hash"])
    none.close()
    # null pointers, straight at the C ABI
    L, err = api.lib(), api.C.create_string_buffer(256)
    out = np.zeros(5 * (N_LWE + 1), np.uint64)
    assert L.vpbs_program_gate_inputs(None, N, K, N_LWE, api._ptr(s["inputs"].reshape(-1)), 1, api._ptr(s["out_cts"].reshape(-1)), api._ptr(out), err,
                                      256) == api.ERR_INVALID and b"null program" in err.value
    assert L.vpbs_program_gate_inputs(prog.h, N, K, N_LWE, None, 1, api._ptr(s["out_cts"].reshape(-1)), api._ptr(out), err, 256) == api.ERR_INVALID
    assert b"null inputs, out_cts or cts_out" in err.value
    root = np.zeros(4, np.uint64)
    assert L.vpbs_program_aggregate_root(prog.h, N, K, N_LWE, None, api._ptr(s["inputs"].reshape(-1)), api._ptr(s["testvs"].reshape(-1)),
                                         api._ptr(s["out_cts"].reshape(-1)), api._ptr(s["key_hash"]), api._ptr(root), err, 256) == api.ERR_INVALID
    assert b"null vk0" in err.value
    assert L.vpbs_program_verify_aggregate(prog.h, None, None, None, None, None, None, 0, None, err, 256) == api.ERR_INVALID and b"null shape" in err.value
    # the Python argument checks need no device either
    with pytest.raises(ValueError, match=r"expected inputs \[2\]\[2\]"):
        api.program_gate_inputs(prog, N, K, N_LWE, np.zeros((3, 2), np.uint64), s["out_cts"])
    with pytest.raises(ValueError, match="expected out_cts"):
        api.program_gate_inputs(prog, N, K, N_LWE, s["inputs"], s["out_cts"][:4])
    with pytest.raises(ValueError, match="tree 1 is empty"):
        api.aggregate_many_args([2, 0, 1])
    with pytest.raises(ValueError, match=r"tree 0: 9 leaves exceed 2\^levels = 8"):
        api.aggregate_many_args([9], levels=3)
    with pytest.raises(ValueError, match="exceed max_leaves 4"):
        api.aggregate_many_args([2, 3], max_leaves=4)
    with pytest.raises(ValueError, match="exceed max_aggregates 1"):
        api.aggregate_many_args([2, 3], max_aggregates=1)
    assert api.aggregate_many_args([1, 2, 3]).tolist() == [0, 1, 3, 6]
    prog.close()
