"""GPU tests (-m gpu) of multi-output lookup gates (csrc/multi_lut.hip, csrc/program.hip): the device forms of the snap and
of sample extraction at a coefficient against the host forms; programs whose gates have several outputs against the composition
snap -> Bootstrapper.run -> extract_at in Python integers (tests/multi_lut_oracle.py); messages through two levels without noise; the
batched evaluation against the per-key one; and, at the N = 8 circuits of tests/test_gpu_program.py, one proof per gate -- byte for byte the
batch prover's proof of the snapped gate input with the packed test vector.  Exact field arithmetic: word for word, byte for byte."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import export_circuits
import multi_lut_oracle as M
import pbs_batch_oracle as B
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
    return dict(ring=ring, rng=rng, s_to=s_to, s_lwe=s_lwe, bsk_flat=np.stack([T.flatten_ggsw(g) for g in bsk]), ksk_flat=T.flatten_ggsw(ksk))


def same(got, want):
    for name, g, w in zip(("wires", "gate_cts", "out_cts"), got, want):
        assert g.shape == w.shape and (g == w).all(), (name, np.argwhere(g != w)[:4].tolist())


@pytest.mark.parametrize("log_n,K,n", [(3, 2, 6), (3, 3, 12)])
def test_device_forms_equal_the_host_forms(ctx, log_n, K, n):
    """every theta and every j, host arrays through the device and device pointers; (3, 3, 12) crosses a polynomial"""
    import torch
    N = 1 << log_n
    rng = np.random.default_rng(40 + K)
    words = rng.integers(0, 1 << 64, size=(5, n + 1), dtype=np.uint64)
    words[0, :6] = np.array([0, 1, P - 1, P, (1 << 64) - 1, 1 << 63], np.uint64)
    glwe = rng.integers(0, P, size=(3, K, N), dtype=np.uint64)
    glwe[1, 0, ::2] = 0
    index = np.array([j for _ in range(3) for j in range(N)] + [N - 1, 0], np.uint32)
    src = np.array([c for c in range(3) for _ in range(N)] + [0, 2], np.uint32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    back = lambda d: d.cpu().numpy().view(np.uint64)
    for theta in range(log_n + 1):
        want = api.lwe_snap(N, theta, words)
        assert (ctx.lwe_snap(N, theta, words) == want).all(), theta
        d_in, d_out = t(words), torch.zeros(words.shape, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()         # torch fills on its stream, the call is on the context's own
        assert ctx.lwe_snap(N, theta, d_in.data_ptr(), count=words.size, out_dev_ptr=d_out.data_ptr()) is None
        assert (back(d_out) == want).all(), theta
    want = api.lwe_extract_at(glwe, n, index, src)
    assert (ctx.lwe_extract_at(glwe, n, index, src) == want).all()
    assert (want[index == 0] == ctx.lwe_extract(glwe, n)[src[index == 0]]).all()          # j = 0 is the existing extraction
    d_g, d_o = t(glwe), torch.zeros(want.shape, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert ctx.lwe_extract_at(d_g.data_ptr(), n, index, src, count=3, N=N, K=K, out_dev_ptr=d_o.data_ptr()) is None
    assert (back(d_o) == want).all()
    with pytest.raises(api.VpbsError, match="row 1.*index 8"):
        ctx.lwe_extract_at(glwe, n, [0, N], [0, 0])
    with pytest.raises(api.VpbsError, match="row 0.*src 3"):
        ctx.lwe_extract_at(glwe, n, [0], [3])
    with pytest.raises(api.VpbsError, match="log_slots"):
        ctx.lwe_snap(N, log_n + 1, words)


C1 = 0x123456789ABCDEF
# 3 inputs (wires 0 1 2), 9 gates that mix (0, 1), (1, 2), (2, 3), (2, 4) and a snapped single-output gate (1, 1); 21 wires; levels
# 1 1 1 2 1 2 3 4 2 (the caller's order interleaves them); level 1 has four gates and level 2 three: two chunks each at max_batch 2.
#   gate 3 reads wire 4 = output 1 of gate 0 on the next level; gate 6 reads wire 7 = output 1 of gate 2 two levels later and wire 12 =
#   output 3 of gate 3; gate 5 reads wire 13 = the output of the snapped single-output gate 4, and wire 8 = output 2 of gate 2
NINE = [([(0, 1)], 0, 0, 1, 2),                           # wires 3 4
        ([], C1, 1),                                      # wire 5
        ([(1, 1), (2, P - 1)], 0, 0, 2, 3),               # wires 6 7 8
        ([(4, P - 1), (1, 1 << 32)], 0, 1, 2, 4),         # wires 9 10 11 12
        ([(2, 1)], 7, 0, 1, 1),                           # wire 13
        ([(13, 3), (8, 1)], 0, 1),                        # wire 14
        ([(12, 1), (7, 2), (0, 5)], 0, 0, 1, 2),          # wires 15 16
        ([(16, 1), (4, P - 2)], P - 1, 1, 2, 3),          # wires 17 18 19
        ([(5, 1)], 0, 0)]                                 # wire 20
NINE_LEVELS = [1, 1, 1, 2, 1, 2, 3, 4, 2]


@pytest.mark.parametrize("log_n,K,ELL,LOGB,n", [(3, 2, 4, 5, 6), (6, 3, 3, 7, 40), (5, 2, 4, 5, 9)])
def test_bit_exact_evaluation_against_the_composition(ctx, log_n, K, ELL, LOGB, n):
    k = oracle_keys(log_n, K, ELL, LOGB, n, 199 + log_n + K)
    assert M.levels(3, NINE) == (NINE_LEVELS, 4) and M.out_first(NINE)[-1] == 18
    delta = T.get_delta(4)
    inputs = np.array([T.lwe_encrypt(k["rng"], k["s_lwe"], delta * m % P) for m in (1, 0, 1)], np.uint64)
    inputs[2, 1] = np.uint64(P + 9)                                       # a word at or above p: reduced before it is snapped
    testvs = k["rng"].integers(0, P, size=(2, 1 << log_n), dtype=np.uint64)
    bs = api.Bootstrapper(ctx, k["bsk_flat"], k["ksk_flat"], K, ELL, LOGB, max_batch=2)
    want = M.evaluate(bs, 3, NINE, inputs, testvs)
    assert want[0].shape == (21, n + 1)
    for form in (NINE, M.csr(NINE)):
        prog = api.Program(ctx, 3, form, 2)
        assert prog.levels()[0].tolist() == NINE_LEVELS and prog.wires()[1] == 21
        same(prog.run(bs, inputs, testvs), want)
        wires, cts, out = prog.run(bs, inputs, testvs, gate_cts=False, out_cts=False)     # the GLWEs are still made: the wires come from them
        assert cts is None and out is None and (wires == want[0]).all()
        prog.close()
    # the snap shows: the input of gate 4 (theta 1) is a multiple of 2^(64 - log_n), that of gate 2 (theta 2) of twice that
    assert not (want[1][4] & np.uint64((1 << (64 - log_n)) - 1)).any() and not (want[1][2] & np.uint64((1 << (65 - log_n)) - 1)).any()
    bs.close()


def test_the_all_0_1_description_through_the_new_call_is_the_plain_program(ctx):
    log_n, K, ELL, LOGB, n = 3, 2, 4, 5, 6
    k = oracle_keys(log_n, K, ELL, LOGB, n, 77)
    plain = [g[:3] for g in NINE[:3]] + [([(3, 1), (5, 2)], 1, 1), ([(6, P - 1)], 0, 0)]
    inputs = k["rng"].integers(0, P, size=(3, n + 1), dtype=np.uint64)
    testvs = k["rng"].integers(0, P, size=(2, 8), dtype=np.uint64)
    bs = api.Bootstrapper(ctx, k["bsk_flat"], k["ksk_flat"], K, ELL, LOGB, max_batch=2)
    a, b = api.Program(ctx, 3, plain, 2), api.Program(ctx, 3, [g + (0, 1) for g in plain], 2)
    same(b.run(bs, inputs, testvs), a.run(bs, inputs, testvs))
    # a gate whose slots do not fit the ring is refused at run time, with the gate named
    c = api.Program(ctx, 3, [plain[0], plain[1] + (4, 1)], 2)
    with pytest.raises(api.VpbsError, match="gate 1.*exceeds N = 8"):
        c.run(bs, inputs, testvs)
    for p in (a, b, c):
        p.close()
    bs.close()


@pytest.mark.parametrize("theta", [1, 2])
def test_messages_at_sigma_zero(ctx, theta):
    """log_n 7, K 2, n 5, p 2, no noise, the decomposition exact (ELL * LOGB = 64).  The only error is the mod switch of the snapped
    words: n + 1 roundings of at most 2^(theta - 1) positions each, and the worst case (n + 1) 2^(theta - 1) <= N / (2 p) - 2^theta
    keeps position rotation + j inside the message's half block: 6 <= 30 for theta 1, 12 <= 28 for theta 2.  So the reference arithmetic
    alone cannot fail, and every output wire and GLWE coefficient j decrypts to exactly table_j[m] * delta, through two levels."""
    log_n, K, ELL, LOGB, n, p = 7, 2, 8, 8, 5, 2
    N, s = 1 << log_n, 1 << theta
    assert (n + 1) * (1 << (theta - 1)) <= N // (2 * p) - s
    k = oracle_keys(log_n, K, ELL, LOGB, n, 5150 + theta)
    delta = T.get_delta(2 * p)
    tables = [[0, 1], [1, 0], [1, 1], [0, 0]][:s]                         # the identity, its complement, two constants
    packed = api.lut_testv_multi(N, p, np.array(tables, np.uint64), delta)[0]
    other = api.lut_testv_multi(N, p, np.array(tables[::-1], np.uint64), delta)[0]
    testvs = np.stack([packed, other])
    msgs = [1, 0]
    inputs = np.array([T.lwe_encrypt(k["rng"], k["s_lwe"], delta * m % P) for m in msgs], np.uint64)
    first = lambda g: 2 + g * s                                           # every gate has s outputs
    gates = [([(0, 1)], 0, 0, theta, s), ([(1, 1)], 0, 1, theta, s),      # level 1: all tables of both inputs
             ([(first(0) + 1, 1)], 0, 0, theta, s),                       # level 2: all tables of NOT m0 (output 1 of gate 0)
             ([(first(1) + s - 2, 1)], 0, 1, theta, s)]                   # ... and of output s - 2 of gate 1, under the reversed tables
    rev = tables[::-1]
    m2, m3 = tables[1][msgs[0]], rev[s - 2][msgs[1]]
    want_msgs = [[t[msgs[0]] for t in tables], [t[msgs[1]] for t in rev], [t[m2] for t in tables], [t[m3] for t in rev]]
    bs = api.Bootstrapper(ctx, k["bsk_flat"], k["ksk_flat"], K, ELL, LOGB, max_batch=4)
    prog = api.Program(ctx, 2, gates, 2)
    assert prog.levels()[0].tolist() == [1, 1, 2, 2]
    wires, gate_cts, out_cts = prog.run(bs, inputs, testvs)
    prog.close()
    same((wires, gate_cts, out_cts), M.evaluate(bs, 2, gates, inputs, testvs))
    bs.close()
    for g in range(4):
        coeffs = T.glwe_decrypt(k["ring"], k["s_to"][:K - 1], B.glwe_list(out_cts[g]), K)
        for j in range(s):
            assert B.lwe_decrypt(k["s_lwe"], wires[first(g) + j]) == delta * want_msgs[g][j] % P, (g, j)
            assert coeffs[j] == delta * want_msgs[g][j] % P, (g, j)


def test_run_batch_is_run_under_each_instances_key(ctx):
    """a ring of 3 key sets, 5 instances, max_batch 4: level 1 is 20 gate rows in 5 chunks whose output rows (8 per instance) start and
    end inside instances; slice b is Program.run on a Bootstrapper of key set key_of[b]"""
    log_n, K, ELL, LOGB, n = 3, 2, 4, 5, 6
    keys = [oracle_keys(log_n, K, ELL, LOGB, n, 611 + 10 * i) for i in range(3)]
    key_of = [2, 0, 1, 0, 2]
    rng = np.random.default_rng(12)
    inputs = rng.integers(0, P, size=(5, 3, n + 1), dtype=np.uint64)
    testvs = rng.integers(0, P, size=(2, 8), dtype=np.uint64)
    prog = api.Program(ctx, 3, NINE, 2)
    bss = [api.Bootstrapper(ctx, k["bsk_flat"], k["ksk_flat"], K, ELL, LOGB, max_batch=3) for k in keys]
    rows = [prog.run(bss[k], inputs[b], testvs) for b, k in enumerate(key_of)]
    want = tuple(np.stack([r[i] for r in rows]) for i in range(3))
    same(rows[1], M.evaluate(bss[0], 3, NINE, inputs[1], testvs))
    for bs in bss:
        bs.close()
    for max_batch in (4, 64):
        kr = api.KeyRing(ctx, K, ELL, LOGB, 8, n, max_keys=3, max_batch=max_batch)
        assert [kr.add(k["bsk_flat"], k["ksk_flat"]) for k in keys] == [0, 1, 2]
        got = prog.run_batch(kr, inputs, key_of, testvs)
        assert got[0].shape == (5, 21, n + 1) and got[1].shape == (5, 9, n + 1)
        same(got, want)
        wires, cts, out = prog.run_batch(kr, inputs, key_of, testvs, gate_cts=False, out_cts=False)
        assert cts is None and out is None and (wires == want[0]).all()
        kr.close()
    prog.close()


# ---- proofs: N = 8, n = 6 (8 steps per chain), the circuits tests/test_gpu_program.py exports ----
K6, ELL6, LOGB6, N6, n6, LOG6 = 2, 4, 5, 8, 6, 13
# 2 inputs (wires 0 1), 4 gates, 2 levels, 4 proofs for 7 results: gate 0 (1, 2) -> wires 2 3; gate 1 (2, 3) -> wires 4 5 6; gate 2 reads wire 3
# (output 1 of gate 0) and wire 6 (output 2 of gate 1); gate 3 (snapped, one output) reads wire 2 (output 0 of gate 0) and wire 4
FOUR = [([(0, 1)], 0, 0, 1, 2), ([(1, 1), (0, P - 1)], 7, 1, 2, 3), ([(3, 1), (6, P - 1)], 0, 0), ([(2, 1), (4, 3)], 0, 1, 1, 1)]


@pytest.fixture(scope="module")
def proven(ctx):
    cyc, dum = [circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N6, K6, ELL6, LOGB6, n6, LOG6)]
    keys = [ctx.keygen(N6, K6, ELL6, LOGB6, n6, seed, *SIGMAS) for seed in (77, 78)]
    delta = api.testv(N6, 2)[1]
    testvs = np.stack([api.lut_testv_multi(N6, 2, np.array([[0, 1], [1, 0]], np.uint64), delta)[0],
                       np.random.default_rng(3).integers(0, P, size=N6, dtype=np.uint64)])
    inputs = np.stack([api.lwe_encrypt(keys[0]["params"], keys[0]["s_lwe"], delta * m % P, nonce=30 + i) for i, m in enumerate([1, 0])])
    prover = api.PbsProver(0, cyc, dum, keys[0]["bsk"], keys[0]["ksk"], K6, ELL6, LOGB6, chains=2, witness_batch=3)
    prog = api.Program(ctx, 2, FOUR, 2)
    proofs, wires, out_cts = prog.prove(prover, inputs, testvs)
    kh, (vk, _) = prover.key_hash(), prover.verifier_data()
    shape = (ctx, vk[4:].reshape(-1, 4), [cyc.n_constants + 80, 135, 20, 16], vk[:4], LOG6, cyc.n_constants, 80, cyc.gates, N6, K6, n6,
             K6 * ELL6 * K6 * N6)
    S = dict(ctx=ctx, cyc=cyc, dum=dum, keys=keys, testvs=testvs, inputs=inputs, prover=prover, prog=prog, proofs=proofs, wires=wires,
             out_cts=out_cts, shape=shape, pv=api.PbsVerifier(*shape, kh, max_batch=3))       # four gates span two chunks
    yield S
    S["pv"].close()
    prog.close()
    prover.close()


def test_one_proof_per_gate_and_it_is_the_batch_provers(proven):
    S = proven
    bs = api.Bootstrapper(S["ctx"], S["keys"][0]["bsk"], S["keys"][0]["ksk"], K6, ELL6, LOGB6, max_batch=4)
    wires, gate_cts, out_cts = M.evaluate(bs, 2, FOUR, S["inputs"], S["testvs"])
    bs.close()
    assert S["wires"].shape == (9, n6 + 1) and (S["wires"] == wires).all() and (S["out_cts"] == out_cts).all()
    want, out, _ = S["prover"].prove(gate_cts, S["testvs"][[g[2] for g in FOUR]])
    assert len(S["proofs"]) == 4 and S["proofs"] == want and (out.reshape(out_cts.shape) == out_cts).all()
    verdicts, reasons, _ = S["prog"].verify(S["pv"], S["inputs"], S["testvs"], S["out_cts"], S["proofs"])
    assert verdicts.tolist() == [1, 1, 1, 1], [api.pbs_reason_text(int(r)) for r in reasons]
    # what the verifier recomputes, restated: the wires from the claimed outputs, the snapped gate inputs from the wires
    assert (M.wires_of(S["inputs"], FOUR, S["out_cts"], n6) == wires).all()
    assert (M.gate_inputs(2, FOUR, wires, n6 + 1, 3) == gate_cts).all()


def test_a_forged_coefficient_fails_its_gate_and_exactly_the_readers_of_that_output(proven):
    S = proven
    forged = S["out_cts"].copy()
    forged[0, K6 - 1, 1] ^= np.uint64(1)              # body coefficient 1 of gate 0: wire 3 changes, wire 2 does not; gate 2 reads wire 3
    verdicts, reasons, _ = S["prog"].verify(S["pv"], S["inputs"], S["testvs"], forged, S["proofs"])
    assert verdicts.tolist() == [0, 1, 0, 1]
    assert reasons[0] == api.PBS_OUT_CT and reasons[2] == api.PBS_LWE_HASH
    forged = S["out_cts"].copy()
    forged[1, K6 - 1, 2] ^= np.uint64(1)              # output 2 of gate 1 = wire 6 (gate 2); gate 3 reads wire 4 and stays
    verdicts, reasons, _ = S["prog"].verify(S["pv"], S["inputs"], S["testvs"], forged, S["proofs"])
    assert verdicts.tolist() == [1, 0, 0, 1] and reasons[1] == api.PBS_OUT_CT and reasons[2] == api.PBS_LWE_HASH
    forged = S["out_cts"].copy()
    forged[1, K6 - 1, 3] ^= np.uint64(1)              # a coefficient that is no output (gate 1 has three): only the output check sees it
    assert S["prog"].verify(S["pv"], S["inputs"], S["testvs"], forged, S["proofs"])[0].tolist() == [1, 0, 1, 1]


def test_another_theta_on_the_verifiers_side_fails_that_gate(proven):
    S = proven
    gates = list(FOUR)
    gates[3] = FOUR[3][:3] + (2, 1)                   # the prover snapped gate 3 with theta 1
    other = api.Program(S["ctx"], 2, gates, 2)
    verdicts, reasons, _ = other.verify(S["pv"], S["inputs"], S["testvs"], S["out_cts"], S["proofs"])
    other.close()
    cts = M.gate_inputs(2, gates, S["wires"], n6 + 1, 3)
    assert (cts[3] != M.gate_inputs(2, FOUR, S["wires"], n6 + 1, 3)[3]).any()      # the two snaps differ on this input
    assert verdicts.tolist() == [1, 1, 1, 0] and reasons[3] == api.PBS_LWE_HASH


def test_prove_batch_and_verify_batch_rows_equal_the_per_instance_calls(proven):
    S = proven
    key_of = [1, 0]
    delta = api.testv(N6, 2)[1]
    second = np.stack([api.lwe_encrypt(S["keys"][1]["params"], S["keys"][1]["s_lwe"], delta * m % P, nonce=50 + i) for i, m in enumerate([0, 1])])
    inputs = np.stack([second, S["inputs"]])          # instance 1 is the fixture's, under key set 0
    rp = api.RingProver(0, S["cyc"], S["dum"], K6, ELL6, LOGB6, N6, n6, max_keys=2, chains=2, witness_batch=3)
    assert [rp.add(k["bsk"], k["ksk"]) for k in S["keys"]] == [0, 1]
    proofs, wires, out_cts = S["prog"].prove_batch(rp, inputs, key_of, S["testvs"])
    hashes = [rp.key_hash(k) for k in range(2)]
    rp.close()
    assert wires.shape == (2, 9, n6 + 1) and len(proofs) == 2 and all(len(row) == 4 for row in proofs)
    assert proofs[1] == S["proofs"] and (wires[1] == S["wires"]).all() and (out_cts[1] == S["out_cts"]).all()
    rv = api.RingVerifier(*S["shape"], max_keys=2, max_batch=3)       # 8 rows in chunks of 3: a chunk straddles the instances
    pvs = [api.PbsVerifier(*S["shape"], h, max_batch=4) for h in hashes]
    for k in range(2):
        rv.set_key(k, hashes[k])
    forged = out_cts.copy()
    forged[0, 0, K6 - 1, 1] ^= np.uint64(1)           # instance 0: wire 3
    for claimed, want in ((out_cts, [[1, 1, 1, 1], [1, 1, 1, 1]]), (forged, [[0, 1, 0, 1], [1, 1, 1, 1]])):
        got = S["prog"].verify_batch(rv, inputs, key_of, S["testvs"], claimed, proofs)
        assert got[0].tolist() == want
        rows = [S["prog"].verify(pvs[k], inputs[b], S["testvs"], claimed[b], proofs[b]) for b, k in enumerate(key_of)]
        for a, b in zip(got, [np.stack([r[j] for r in rows]) for j in range(3)]):
            assert a.tobytes() == b.tobytes()
    for pv in pvs:
        pv.close()
    rv.close()


def test_the_tool_with_multi_output_gates():
    export_circuits.ensure_cyclic_circuit(N6, K6, ELL6, LOGB6, n6, LOG6)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "tools", "run_program.py"), "--n8", "--multi", "1", "--prove"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["multi"]["mismatches"] == 0 and line["all_equal"] is True
    assert line["multi"]["proofs"] == line["multi"]["gates"] < line["single"]["gates"] == line["single"]["proofs"]
    assert line["multi"]["verified"] == line["multi"]["gates"] and line["single"]["verified"] == line["single"]["gates"]
