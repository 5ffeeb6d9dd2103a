"""GPU tests (-m gpu) of programs of lookup gates on resident keys (vpbs_program_*, csrc/program.hip; api.Program).  The yardsticks are
existing code: for evaluation, Bootstrapper.run per level on combinations formed with Python integers mod p (tests/program_oracle.py); for
proofs, PbsProver.prove; for verdicts, PbsVerifier.verify on inputs the test recomputes itself.  Exact field arithmetic: every comparison
is word for word or byte for byte."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import export_circuits
import pbs_batch_oracle as B
import program_oracle as O
import tfhe_oracle as T
import vpbs_amd
from vpbs_amd import api, circuit_file

pytestmark = pytest.mark.gpu
P = api.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = (4.99027217501041e-8, 1.17021618159313e-5)       # main.rs:29-30


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    yield c
    c.close()


def oracle_keys(log_n, K, ELL, LOGB, n, seed):
    ring = T.Ring(log_n)
    rng = np.random.default_rng(seed)
    s_to, s_lwe, s_glwe, bsk, ksk = T.pbs_setup(ring, rng, n, K, ELL, LOGB)
    return ring, rng, s_to, s_lwe, np.stack([T.flatten_ggsw(g) for g in bsk]), T.flatten_ggsw(ksk)


def same(got, want):
    for name, g, w in zip(("wires", "gate_cts", "out_cts"), got, want):
        assert g.shape == w.shape and (g == w).all(), (name, np.argwhere(g != w)[:4].tolist())


# 3 inputs (wires 0 1 2), 9 gates (gate g is wire 3 + g), 3 levels: level 1 = gates 0 1 3 5 8, level 2 = gates 2 6, level 3 = gates 4 7 -- the
# caller's order interleaves the levels.  Fan-in 0 (gate 1), 1, 2 and 5 (gate 4); coefficients p - 1 and 2^32 (gate 2); non-zero constants
# (gates 1, 7); wire 3 is read on level 2 (gate 2) and on level 3 (gate 4); input 0 is read on level 3 (gate 4); two luts.
NINE = [([(0, 1)], 0, 0),
        ([], 0x123456789ABCDEF, 1),
        ([(3, P - 1), (1, 1 << 32)], 0, 0),
        ([(2, 1), (0, 5)], 0, 1),
        ([(5, 1), (3, 1), (4, 7), (0, 3), (6, 2)], 0, 1),
        ([(1, 1)], 0, 0),
        ([(8, 1), (4, P - 2)], 0, 0),
        ([(5, 3)], P - 1, 1),
        ([(2, 1)], 0, 0)]


@pytest.mark.parametrize("log_n,K,ELL,LOGB,n", [(6, 2, 8, 8, 5), (3, 2, 4, 5, 6), (6, 3, 3, 7, 40), (5, 2, 4, 5, 9)])
def test_bit_exact_evaluation_against_the_composition(ctx, log_n, K, ELL, LOGB, n):
    """max_batch = 2: level 1 (five gates) spans three chunks, the last of them partial"""
    ring, rng, s_to, s_lwe, bsk_flat, ksk_flat = oracle_keys(log_n, K, ELL, LOGB, n, 99 + log_n + K)
    assert O.levels(3, NINE) == ([1, 1, 2, 1, 3, 1, 2, 3, 1], 3)
    delta = T.get_delta(4)
    inputs = np.array([T.lwe_encrypt(rng, s_lwe, delta * m % P) for m in (1, 0, 1)], np.uint64)
    testvs = np.stack([np.array(T.get_testv(ring, 2, delta), np.uint64), rng.integers(0, P, size=ring.n, dtype=np.uint64)])
    bs = api.Bootstrapper(ctx, bsk_flat, ksk_flat, K, ELL, LOGB, max_batch=2)
    want = O.evaluate(bs, 3, NINE, inputs, testvs)
    for form in (NINE, O.csr(NINE)):
        prog = api.Program(ctx, 3, form, 2)
        assert prog.levels()[0].tolist() == [1, 1, 2, 1, 3, 1, 2, 3, 1]
        same(prog.run(bs, inputs, testvs), want)
        prog.close()
    bs.close()


def test_edge_words(ctx):
    """input words 0, p - 1, 2^63 and words at or above p (reduced by the combination, as the header says); w + (p - 1) w is the all-zero
    ciphertext; a constant-only gate is the trivial ciphertext of its constant"""
    log_n, K, ELL, LOGB, n = 3, 2, 4, 5, 6
    ring, rng, s_to, s_lwe, bsk_flat, ksk_flat = oracle_keys(log_n, K, ELL, LOGB, n, 4321)
    inputs = rng.integers(0, P, size=(2, n + 1), dtype=np.uint64)
    inputs[0, :5] = np.array([0, P - 1, 1 << 63, P, P + 5], np.uint64)
    inputs[0, n] = np.uint64((1 << 64) - 1)                                   # the body, at or above p
    inputs[1, 0], inputs[1, 1] = np.uint64(P + (1 << 31)), np.uint64(P - 1)
    const = 0xFFFFFFFF00000000                                                # p - 1
    gates = [([(0, 1)], 0, 0),                       # the identity: the input, reduced
             ([(1, 1), (1, P - 1)], 0, 0),           # w + (p - 1) w
             ([], const, 0),                         # a constant alone
             ([(0, P - 1), (1, 1 << 32)], 1, 0),     # edge words under edge coefficients
             ([(2, 1), (3, 1), (4, P - 1)], 0, 0)]   # level 2
    testvs = rng.integers(0, P, size=(1, ring.n), dtype=np.uint64)
    bs = api.Bootstrapper(ctx, bsk_flat, ksk_flat, K, ELL, LOGB, max_batch=4)
    want = O.evaluate(bs, 2, gates, inputs, testvs)
    prog = api.Program(ctx, 2, gates, 1)
    got = prog.run(bs, inputs, testvs)
    prog.close()
    bs.close()
    same(got, want)
    wires, gate_cts, _ = got
    assert (wires[:2] == inputs).all()                                        # inputs are shown as given
    assert gate_cts[0].tolist() == [int(w) % P for w in inputs[0]] and gate_cts[0, 3] == 0 and gate_cts[0, 4] == 5
    assert not gate_cts[1].any()
    assert gate_cts[2].tolist() == [0] * n + [const]
    assert (gate_cts < np.uint64(P)).all()


def test_messages_at_sigma_zero(ctx):
    """depth 3 without noise: identity gates and sums of a 0-wire and a 1-wire (and of two 0-wires) decrypt to exactly delta * m"""
    log_n, K, ELL, LOGB, n = 6, 2, 8, 8, 5
    ring, rng, s_to, s_lwe, bsk_flat, ksk_flat = oracle_keys(log_n, K, ELL, LOGB, n, 4242)
    delta = T.get_delta(4)
    testvs = np.array([T.get_testv(ring, 2, delta)], np.uint64)
    msgs = [0, 1, 1, 0]
    inputs = np.array([T.lwe_encrypt(rng, s_lwe, delta * m % P) for m in msgs], np.uint64)
    one = lambda w: ([(w, 1)], 0, 0)
    add = lambda a, b: ([(a, 1), (b, 1)], 0, 0)
    gates = [one(0), one(1), one(2), one(3),                 # wires 4 .. 7: 0 1 1 0
             add(4, 5), add(7, 6), add(4, 7), one(5),        # wires 8 .. 11: 1 1 0 1
             one(8), add(10, 11), add(10, 4)]                # wires 12 .. 14: 1 1 0 (the last reads level 2 and level 1)
    want_msgs = msgs + [0, 1, 1, 0, 1, 1, 0, 1, 1, 1, 0]
    bs = api.Bootstrapper(ctx, bsk_flat, ksk_flat, K, ELL, LOGB, max_batch=8)
    prog = api.Program(ctx, 4, gates, 1)
    assert prog.levels()[1] == 3
    wires, gate_cts, out_cts = prog.run(bs, inputs, testvs)
    prog.close()
    same((wires, gate_cts, out_cts), O.evaluate(bs, 4, gates, inputs, testvs))
    bs.close()
    assert [B.lwe_decrypt(s_lwe, w) for w in wires] == [delta * m % P for m in want_msgs]
    assert [T.glwe_decrypt(ring, s_to[:K - 1], B.glwe_list(o), K)[0] for o in out_cts] == [delta * m % P for m in want_msgs[4:]]


def test_the_papers_parameters_and_noise(ctx):
    """N = 1024, n = 728, max_batch 8; 4 inputs, 6 gates, 3 levels.  Every wire is the composition's; the fan-in-1, coefficient-1 gates
    decrypt to their messages (what test_the_loop_closes_at_the_papers_parameters establishes); the sums are held to the composition only"""
    N, K, ELL, LOGB, n = 1024, 2, 4, 5, 728
    keys = ctx.keygen(N, K, ELL, LOGB, n, 0x5EED, *SIGMAS)
    testv, delta = api.testv(N, 2)
    msgs = [1, 0, 1, 0]
    inputs = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * m % P, nonce=200 + i) for i, m in enumerate(msgs)])
    gates = [([(0, 1)], 0, 0), ([(1, 1)], 0, 0), ([(2, 1), (3, 1)], 0, 0),      # level 1: 1, 0, a sum
             ([(4, 1)], 0, 0), ([(4, 1), (5, 1)], 0, 0),                        # level 2: 1, a sum
             ([(7, 1)], 0, 0)]                                                  # level 3: 1
    bs = api.Bootstrapper(ctx, keys["bsk"], keys["ksk"], K, ELL, LOGB, max_batch=8)
    prog = api.Program(ctx, 4, gates, 1)
    assert prog.levels()[0].tolist() == [1, 1, 1, 2, 2, 3]
    got = prog.run(bs, inputs, testv.reshape(1, N))
    prog.close()
    same(got, O.evaluate(bs, 4, gates, inputs, testv.reshape(1, N)))
    bs.close()
    wires = got[0]
    for g, m in ((0, 1), (1, 0), (3, 1), (5, 1)):
        assert B.round_message(api.lwe_decrypt(keys["s_lwe"], wires[4 + g]), delta, 2) == m, g


def test_device_pointers_adopted_keys_and_reuse(ctx):
    """keys from Context.keygen_device, on_device = 1 inputs and outputs, two runs on one object with an invalid call in between: what a fresh
    object with host keys gives"""
    import torch
    N, K, ELL, LOGB, n = 256, 2, 4, 5, 100
    host = ctx.keygen(N, K, ELL, LOGB, n, 0xD0D0, *SIGMAS)
    dev = ctx.keygen_device(N, K, ELL, LOGB, n, 0xD0D0, *SIGMAS)
    testv, delta = api.testv(N, 2)
    testvs = np.stack([testv, np.random.default_rng(6).integers(0, P, size=N, dtype=np.uint64)])
    inputs = np.stack([api.lwe_encrypt(host["params"], host["s_lwe"], delta * m % P, nonce=i) for i, m in enumerate([1, 0])])
    gates = [([(0, 1)], 0, 0), ([(2, 1), (1, P - 1)], 3, 1), ([(1, 1)], 0, 1), ([(3, 1), (4, 2)], 0, 0)]      # levels 1 2 1 3
    fresh_bs = api.Bootstrapper(ctx, host["bsk"], host["ksk"], K, ELL, LOGB, max_batch=3)
    fresh = api.Program(ctx, 2, gates, 2)
    want = fresh.run(fresh_bs, inputs, testvs)
    same(want, O.evaluate(fresh_bs, 2, gates, inputs, testvs))
    fresh.close()
    fresh_bs.close()
    bs = api.Bootstrapper(ctx, dev["d_bsk"], dev["d_ksk"], K, ELL, LOGB, max_batch=1, N=N, n_lwe=n, keys_on_device=True)
    prog = api.Program(ctx, 2, gates, 2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    back = lambda d: d.cpu().numpy().view(np.uint64)
    d_in, d_tv = t(inputs), t(testvs)
    L = api.lib()
    for attempt in range(2):
        d_w = torch.zeros((6, n + 1), dtype=torch.int64, device="cuda")
        d_c = torch.zeros((4, n + 1), dtype=torch.int64, device="cuda")
        d_o = torch.zeros((4, K, N), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()         # torch fills on its stream, the run is on the context's own
        assert prog.run_device(bs, d_in.data_ptr(), d_tv.data_ptr(), d_w.data_ptr(), d_c.data_ptr(), d_o.data_ptr()) == 3
        same((back(d_w), back(d_c), back(d_o)), want)
        # only the wires asked for
        d_w2 = torch.zeros_like(d_w)
        torch.cuda.synchronize()
        assert prog.run_device(bs, d_in.data_ptr(), d_tv.data_ptr(), d_w2.data_ptr()) == 3
        assert (back(d_w2) == want[0]).all()
        # refusals leave the object usable
        assert L.vpbs_program_run(prog.h, bs.h, None, d_tv.data_ptr(), d_w.data_ptr(), None, None, 1) == -1
        assert L.vpbs_program_run(prog.h, bs.h, d_in.data_ptr(), None, d_w.data_ptr(), None, None, 1) == -1
        assert L.vpbs_program_run(prog.h, None, d_in.data_ptr(), d_tv.data_ptr(), d_w.data_ptr(), None, None, 1) == -1
    same(prog.run(bs, inputs, testvs), want)          # host pointers on the same object
    prog.close()
    bs.close()
    ctx.device_free(dev["d_bsk"])
    ctx.device_free(dev["d_ksk"])


# ---- proofs: N = 8, n = 6 (8 steps per chain), the n6 shape of tests/test_gpu_pbs_prove_batch.py ----
K6, ELL6, LOGB6, N6, n6, LOG6 = 2, 4, 5, 8, 6, 13
# 2 inputs (wires 0 1), 4 gates (wires 2 .. 5), 2 levels; wire 2 (gate 0) is read by gate 2 alone
FOUR = [([(0, 1)], 0, 0), ([(1, 1), (0, P - 1)], 7, 1), ([(2, 1), (3, P - 1)], 0, 0), ([(3, 1)], 0, 1)]


@pytest.fixture(scope="module")
def proven(ctx):
    cyc, dum = [circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N6, K6, ELL6, LOGB6, n6, LOG6)]
    keys = ctx.keygen(N6, K6, ELL6, LOGB6, n6, 77, *SIGMAS)
    tv, delta = api.testv(N6, 2)
    testvs = np.stack([tv, np.array([(P - int(v)) % P for v in tv], np.uint64)])
    inputs = np.stack([api.lwe_encrypt(keys["params"], keys["s_lwe"], delta * m % P, nonce=30 + i) for i, m in enumerate([1, 0])])
    prover = api.PbsProver(0, cyc, dum, keys["bsk"], keys["ksk"], K6, ELL6, LOGB6, chains=2, witness_batch=3)
    prog = api.Program(ctx, 2, FOUR, 2)
    seen = []
    proofs, wires, out_cts = prog.prove(prover, inputs, testvs, on_proof=lambda g, b: seen.append((g, b)))
    kh, (vk, _) = prover.key_hash(), prover.verifier_data()
    ncols = [cyc.n_constants + 80, 135, 20, 16]
    make = lambda max_batch: api.PbsVerifier(ctx, vk[4:].reshape(-1, 4), ncols, vk[:4], LOG6, cyc.n_constants, 80, cyc.gates, N6, K6, n6,
                                             K6 * ELL6 * K6 * N6, kh, max_batch=max_batch)
    S = dict(ctx=ctx, keys=keys, testvs=testvs, inputs=inputs, prover=prover, prog=prog, seen=seen, proofs=proofs, wires=wires, out_cts=out_cts,
             pv3=make(3), pv4=make(4))         # pv3: four gates span two chunks of the program's verify; pv4: the yardstick, one batch
    yield S
    S["pv3"].close()
    S["pv4"].close()
    prog.close()
    prover.close()


def recomputed(S, gates, out_cts):
    """what a verifier derives from the claimed outputs, restated: wires = inputs | extractions; the gate inputs; the per-gate test vectors"""
    wires = np.concatenate([S["inputs"], np.array([B.extract(B.glwe_list(o), n6) for o in out_cts], np.uint64)])
    return O.gate_inputs(2, gates, wires, n6 + 1), S["testvs"][[g[2] for g in gates]]


def test_proofs_are_the_batch_provers(proven):
    S = proven
    bs = api.Bootstrapper(S["ctx"], S["keys"]["bsk"], S["keys"]["ksk"], K6, ELL6, LOGB6, max_batch=4)
    wires, gate_cts, out_cts = O.evaluate(bs, 2, FOUR, S["inputs"], S["testvs"])
    bs.close()
    assert (S["wires"] == wires).all() and (S["out_cts"] == out_cts).all()
    want, _, lwe = S["prover"].prove(gate_cts, S["testvs"][[g[2] for g in FOUR]])
    assert S["proofs"] == want and (lwe == wires[2:]).all()
    assert sorted(g for g, _ in S["seen"]) == [0, 1, 2, 3] and all(b == want[g] for g, b in S["seen"])     # the caller's gate indices
    verdicts, reasons, _ = S["prog"].verify(S["pv3"], S["inputs"], S["testvs"], S["out_cts"], S["proofs"])
    assert verdicts.tolist() == [1, 1, 1, 1], [api.pbs_reason_text(int(r)) for r in reasons]
    # a prefix: steps is the batch prover's
    prefix = S["prog"].prove(S["prover"], S["inputs"], S["testvs"], steps=3)[0]
    assert prefix == S["prover"].prove(gate_cts, S["testvs"][[g[2] for g in FOUR]], steps=3)[0]
    with pytest.raises(api.VpbsError, match="steps exceeds"):
        S["prog"].prove(S["prover"], S["inputs"], S["testvs"], steps=n6 + 3)


def check_forgery(S, gates, out_cts, proofs, refused):
    cts, tvs = recomputed(S, gates, out_cts)
    want = S["pv4"].verify(proofs, tvs, cts, out_cts.reshape(4, -1))
    prog = api.Program(S["ctx"], 2, gates, 2)
    got = prog.verify(S["pv3"], S["inputs"], S["testvs"], out_cts, proofs)
    prog.close()
    for g, w in zip(got, want):
        assert g.tolist() == w.tolist()
    assert [g for g in range(4) if not got[0][g]] == refused
    return got


def test_a_forged_output_fails_its_gate_and_every_consumer(proven):
    S = proven
    out_cts = S["out_cts"].copy()
    out_cts[0, 0, 3] ^= np.uint64(1)                  # a mask word of gate 0's output: wire 2 changes, gate 2 reads it
    verdicts, reasons, _ = check_forgery(S, FOUR, out_cts, S["proofs"], [0, 2])
    assert reasons[0] == 5 and reasons[2] == 9        # VPBS_PBS_OUT_CT; VPBS_PBS_LWE_HASH


def test_a_changed_coefficient_fails_exactly_that_gate(proven):
    S = proven
    gates = list(FOUR)
    gates[2] = ([(2, 1), (3, P - 2)], 0, 0)
    check_forgery(S, gates, S["out_cts"], S["proofs"], [2])


def test_swapped_proofs_fail_both_gates(proven):
    S = proven
    proofs = list(S["proofs"])
    proofs[1], proofs[3] = proofs[3], proofs[1]
    check_forgery(S, FOUR, S["out_cts"], proofs, [1, 3])


def test_a_wrong_lut_fails_exactly_that_gate(proven):
    S = proven
    gates = list(FOUR)
    gates[1] = (FOUR[1][0], FOUR[1][1], 0)
    verdicts, reasons, _ = check_forgery(S, gates, S["out_cts"], S["proofs"], [1])
    assert reasons[1] == 3                            # VPBS_PBS_TESTV


def test_the_tool_evaluates_proves_verifies_and_decrypts():
    export_circuits.ensure_cyclic_circuit(N6, K6, ELL6, LOGB6, n6, LOG6)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_program.py"), "--n8", "--levels", "2", "--width", "2", "--prove"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["all_equal"] is True and line["gates"] == 4 and line["levels"] == 2
    assert line["verified"] == 4 and line["proven"] is True
    assert line["decrypted_checked"] >= 1 and line["decrypted_correct"] == line["decrypted_checked"]
