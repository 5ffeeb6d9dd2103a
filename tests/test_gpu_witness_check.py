"""GPU tests (-m gpu) of the device witness checker (vpbs_witness_checker_*, csrc/witness_check.hip) and of the checked proving paths built on
it (vpbs_prove_step_checked, vpbs_ivc_set_check_witness).  The yardstick throughout is the host checker, vpbs_check_witness: the device must
return the same verdict and the same message for every witness, satisfied or not."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import export_circuits
import oracle as orc
import step_circuit as sc
import tfhe_oracle as T
import vpbs_amd
from vpbs_amd import api, circuit_file

pytestmark = pytest.mark.gpu
P = api.P
K, ELL, LOGB = 2, 4, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    yield c
    c.close()


def pi_hash(circuit, pi_pos, wires):
    return api.hash_no_pad(np.array([wires[c][r] for c, r in pi_pos], np.uint64))


def step_circuit_n8():
    """the step circuit at N = 8 (circuitgen), its plan and one satisfied witness -> (StepCircuit, built circuit, plan, preset values, wires)"""
    circ = sc.StepCircuit(api, 8, K, ELL, LOGB, 6, orc.negacyclic_params(3))
    b = circ.built
    targets = ([t for p in circ.acc_init for t in p] + [t for p in circ.acc_in for t in p] + circ.ggsw_flat + [circ.counter, circ.mask] +
               circ.bsk_hash_in + circ.lwe_hash_in)
    plan = b.circuit.witness_plan([b.pos(t) for t in targets])
    rng = np.random.default_rng(8)
    vals = rng.integers(0, P, size=len(targets), dtype=np.uint64)
    vals[len(targets) - 10] = 3   # the counter
    wires = plan.run(vals)
    return circ, b, plan, vals, wires


def step_circuit_file(N):
    d = circuit_file.load(export_circuits.ensure_step_circuit(N, K, ELL, LOGB, 728))
    plan = d.circuit.witness_plan(d.preset_pos)
    v = np.random.default_rng(N).integers(0, P, size=len(d.preset_pos), dtype=np.uint64)
    v[len(d.preset_pos) - 10] = 1
    return d, plan, plan.run(v)


def cyclic_step0(ctx, N, n_lwe, log_n):
    """a satisfied witness of the CYCLIC step circuit: its first chained step, on top of a real base proof of the dummy circuit (the previous
    proof of the step) and the dummy proof of all-zero public inputs -> (cyclic description, dummy description, cyclic wires, the base proof's
    dummy-circuit wires, its public inputs)"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prove_ivc
    paths = export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, n_lwe, log_n)
    cyc, dum = prove_ivc.Circuit(ctx, paths[0]), prove_ivc.Circuit(ctx, paths[1])
    kn = K * N
    testv, _ = api.testv(N, 2)
    base_pis = np.concatenate([np.zeros((K - 1) * N, np.uint64), testv.reshape(-1), np.zeros(1 + kn + 8, np.uint64), cyc.vk])
    flat = lambda p: np.concatenate([np.asarray(p[k], np.uint64).reshape(-1) for k in ("caps", "openings", "fri")])

    def prove_dummy(pis):
        w = dum.plan.run(pis)
        d_w = torch.from_numpy(w.view(np.int64)).cuda()
        torch.cuda.synchronize()
        proof = dum.prove(d_w.data_ptr(), pis)[0]
        return w, flat(proof)
    _, dummy_flat = prove_dummy(np.zeros(base_pis.size, np.uint64))
    base_wires, base_flat = prove_dummy(base_pis)
    mask = np.array([12345 % P], np.uint64)
    values = np.concatenate([base_flat, base_pis, np.array([0], np.uint64), np.zeros(K * ELL * K * N, np.uint64), mask, cyc.vk, dum.vk,
                             dummy_flat, np.zeros(base_pis.size, np.uint64)])
    wires = cyc.plan.run(values)
    return cyc.d, dum.d, wires, base_wires, base_pis


def both(checker, circuit, wires, h, device_ptr=None):
    """(host verdict, device verdict) on the same matrix"""
    want = circuit.check_witness(wires, h)
    got = checker.check(device_ptr if device_ptr is not None else wires, h)
    return want, got


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. acceptance

def test_device_checker_accepts_satisfied_step_circuit_witnesses(ctx):
    import torch
    circ, b, plan, _, w = step_circuit_n8()
    h = api.hash_no_pad(np.array(circ.public_inputs(w), np.uint64))
    chk = api.WitnessChecker(ctx, b.circuit)
    assert b.circuit.check_witness(w, h) == (True, "")
    assert chk.check(w, h) == (True, "")
    d_w = torch.from_numpy(w.view(np.int64)).cuda()
    torch.cuda.synchronize()
    assert chk.check(d_w.data_ptr(), h) == (True, "")
    chk.free()
    plan.free()
    d, plan, w = step_circuit_file(1024)
    h = pi_hash(d.circuit, d.pi_pos, w)
    chk = api.WitnessChecker(ctx, d.circuit)
    assert d.circuit.check_witness(w, h) == (True, "")
    assert chk.check(w, h) == (True, "")
    d_w = torch.from_numpy(w.view(np.int64)).cuda()
    torch.cuda.synchronize()
    assert chk.check(d_w.data_ptr(), h) == (True, "")
    # the same matrix under a wrong hash: both name the public-input row
    bad = h.copy()
    bad[2] ^= 1
    want, got = both(chk, d.circuit, w, bad)
    assert not want[0] and got == want
    chk.free()
    plan.free()


@pytest.mark.parametrize("N,n_lwe,log_n", [(8, 1, 13), (1024, 728, 16)])
def test_device_checker_accepts_satisfied_cyclic_circuit_witnesses(ctx, N, n_lwe, log_n):
    import torch
    cyc, dum, w, base_w, base_pis = cyclic_step0(ctx, N, n_lwe, log_n)
    h = pi_hash(cyc.circuit, cyc.pi_pos, w)
    chk = api.WitnessChecker(ctx, cyc.circuit)
    assert cyc.circuit.check_witness(w, h) == (True, "")
    assert chk.check(w, h) == (True, "")
    d_w = torch.from_numpy(w.view(np.int64)).cuda()
    torch.cuda.synchronize()
    assert chk.check(d_w.data_ptr(), h) == (True, "")
    chk.free()
    dchk = api.WitnessChecker(ctx, dum.circuit)   # the base proof's witness: the dummy circuit
    hb = api.hash_no_pad(base_pis)
    assert dum.circuit.check_witness(base_w, hb) == (True, "") and dchk.check(base_w, hb) == (True, "")
    dchk.free()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the same verdict and the same message on a seeded corpus of corrupted witnesses

def corpus(circuit, wires, h, rng, per_kind):
    """yield (label, wires, pi_hash) corruptions of a satisfied witness"""
    n = circuit.n
    gates = list(circuit.gates.arr)
    rows_of = {}
    for r, g in enumerate(circuit.row_gate):
        rows_of.setdefault(int(g), []).append(r)
    kinds = {}
    for gi, rows in rows_of.items():
        kinds.setdefault(gates[gi].kind, []).append(gi)
    copies = circuit.copies
    # copy pairs whose first cell is not read by its row's gate: changing it breaks only the copy constraint
    first_gate = circuit.row_gate[copies[:, 0] % n]
    n_constraints = np.array([g.num_constraints for g in gates])[first_gate]
    n_wires = np.array([g.num_wires for g in gates])[first_gate]
    quiet = np.nonzero((n_constraints == 0) | (copies[:, 0] // n >= n_wires))[0]

    def changed(w, col, row, value=None):
        w = w.copy()
        w[col, row] = value if value is not None else (int(w[col, row]) + 1 + int(rng.integers(0, P - 1, dtype=np.uint64))) % P
        return w
    for kind, gis in sorted(kinds.items()):
        if gates[gis[0]].num_constraints == 0:
            continue
        for _ in range(per_kind):
            gi = gis[int(rng.integers(len(gis)))]
            row = rows_of[gi][int(rng.integers(len(rows_of[gi])))]
            col = int(rng.integers(gates[gi].num_wires))
            yield "gate %s" % api.GATE_KINDS[kind], changed(wires, col, row), h
    for _ in range(per_kind):
        i = int(rng.integers(copies.shape[0]))
        a = int(copies[i][int(rng.integers(2))])
        yield "routed cell", changed(wires, a // n, a % n), h
    for _ in range(min(per_kind, len(quiet))):
        a = int(copies[quiet[int(rng.integers(len(quiet)))]][0])
        yield "copy pair", changed(wires, a // n, a % n), h
    for _ in range(4):
        bad = h.copy()
        bad[int(rng.integers(4))] = int(rng.integers(0, P, dtype=np.uint64))
        yield "pi hash", wires, bad
    constrained = [g for g in rows_of if gates[g].num_constraints]
    for _ in range(per_kind):   # a gate row AND a copy pair broken: the host reports the gate
        gi = constrained[int(rng.integers(len(constrained)))]
        row = rows_of[gi][int(rng.integers(len(rows_of[gi])))]
        w = changed(wires, int(rng.integers(gates[gi].num_wires)), row)
        if len(quiet):
            a = int(copies[quiet[int(rng.integers(len(quiet)))]][0])
            w = changed(w, a // n, a % n)
        yield "gate + copy", w, h
    for value in (P, (1 << 64) - 1):   # the non-canonical words of tests/edge_operands.py, on cells that hold 0 and on any cell
        zeros = np.argwhere(wires[:, :] == 0)
        for _ in range(per_kind):
            c, r = zeros[int(rng.integers(len(zeros)))] if len(zeros) and rng.integers(2) else (int(rng.integers(circuit.n_wires)), int(rng.integers(n)))
            yield "non-canonical %#x" % value, changed(wires, int(c), int(r), value), h


@pytest.mark.parametrize("which", ["step_n8", "cyclic_n8"])
def test_device_and_host_checkers_agree_on_corrupted_witnesses(ctx, which):
    if which == "step_n8":
        circ, b, plan, _, w = step_circuit_n8()
        circuit, h = b.circuit, api.hash_no_pad(np.array(circ.public_inputs(w), np.uint64))
        plan.free()
    else:
        d, _, w, _, _ = cyclic_step0(ctx, 8, 1, 13)
        circuit, h = d.circuit, pi_hash(d.circuit, d.pi_pos, w)
    rng = np.random.default_rng(0xC4EC + len(which))
    # every copy pair of these circuits has both cells read by their rows' gates, so a changed cell always breaks a gate first; extra pairs
    # between equal cells of routed columns on NoopGate rows give the corpus cells whose change breaks a copy constraint alone
    noop = np.nonzero(np.array([circuit.gates.arr[g].kind for g in circuit.row_gate]) == 0)[0]
    cells = [(c, int(r)) for r in noop[:32] for c in range(0, 80, 7)]
    extra = []
    for i in range(64):
        (c1, r1), (c2, r2) = cells[int(rng.integers(len(cells)))], cells[int(rng.integers(len(cells)))]
        if (c1, r1) != (c2, r2) and w[c1, r1] == w[c2, r2]:
            extra.append((c1 * circuit.n + r1, c2 * circuit.n + r2))
    assert len(extra) >= 16
    circuit = api.Circuit(circuit.gates, circuit.log_n, circuit.row_gate, circuit.constants, np.concatenate([circuit.copies, np.array(extra)]),
                          circuit.n_wires, circuit.n_routed)
    assert circuit.check_witness(w, h) == (True, "")
    chk = api.WitnessChecker(ctx, circuit)
    seen, labels, violated, copy_messages = 0, {}, 0, 0
    for label, cw, ch in corpus(circuit, w, h, rng, per_kind=24 if which == "step_n8" else 12):
        want, got = both(chk, circuit, cw, ch)
        assert got == want, (label, want, got)
        seen += 1
        labels[label.split(" 0x")[0]] = labels.get(label.split(" 0x")[0], 0) + 1
        violated += not want[0]
        copy_messages += want[1].startswith("copy constraint violated")
    assert seen >= 200, seen
    assert violated >= seen // 2, (violated, seen)   # most corruptions must actually break something
    assert labels.get("copy pair", 0) >= 12 and copy_messages >= 12, (labels, copy_messages)
    kinds = {l for l in labels if l.startswith("gate ")}
    if which == "cyclic_n8":   # the in-circuit verifier uses every gate kind with constraints, coset interpolation and Poseidon among them
        assert {"gate poseidon", "gate coset_interpolation", "gate public_input"} <= kinds, kinds
    chk.free()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. wires that never left the device

def test_device_checker_on_wires_gathered_on_the_device(ctx):
    import torch
    circ, b, plan, vals, _ = step_circuit_n8()
    rng = np.random.default_rng(3)
    cols = [vals]
    for i in range(2):
        v = rng.integers(0, P, size=vals.size, dtype=np.uint64)
        v[vals.size - 10] = 4 + i   # the counter
        cols.append(v)
    dev = api.WitnessDevice(ctx, plan, max_batch=3)
    dev.run(np.ascontiguousarray(np.stack(cols, axis=1)))
    chk = api.WitnessChecker(ctx, b.circuit)
    d_w = torch.zeros((135, b.n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    n = b.n
    for i in range(3):
        dev.wires(i, d_w.data_ptr())
        ctx.synchronize()
        host = d_w.cpu().numpy().view(np.uint64).copy()
        h = api.hash_no_pad(np.array(circ.public_inputs(host), np.uint64))
        assert chk.check(d_w.data_ptr(), h) == (True, "") == b.circuit.check_witness(host, h)
        # one word overwritten in HBM: a cell of a PoseidonGate row (every one of its wires is constrained), then a cell of a copy pair
        pos_rows = [r for r in range(n) if b.circuit.gates.arr[b.circuit.row_gate[r]].kind == api.GATE_KINDS.index("poseidon")]
        targets = [(int(rng.integers(135)), pos_rows[int(rng.integers(len(pos_rows)))])]
        a = int(b.circuit.copies[int(rng.integers(b.circuit.copies.shape[0]))][1])
        targets.append((a // n, a % n))
        for col, row in targets:
            dev.wires(i, d_w.data_ptr())
            ctx.synchronize()
            d_w[col, row] = int((int(host[col, row]) + 5) % P) - (1 << 64 if (int(host[col, row]) + 5) % P >= 1 << 63 else 0)
            torch.cuda.synchronize()
            down = d_w.cpu().numpy().view(np.uint64)
            assert int(down[col, row]) != int(host[col, row])
            want = b.circuit.check_witness(down, h)
            assert chk.check(d_w.data_ptr(), h) == want
            assert not want[0] and ("row %d:" % row in want[1] or "row %d)" % row in want[1]), (want, col, row)
    chk.free()
    dev.free()
    plan.free()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. checked step proofs

def test_checked_step_proof(ctx):
    circ, b, plan, _, w = step_circuit_n8()
    plan.free()
    sigma = b.circuit.sigma_values()
    nconst = b.constants.shape[0]
    cs = ctx.commit_values(np.concatenate([b.constants, sigma]))
    digest = [0xA, 0xB, 0xC, 0xD]
    chk = api.WitnessChecker(ctx, b.circuit)

    def si(wires):
        return ctx.make_step_inputs(b.log_n, wires, None, None, cs, digest, circ.public_inputs(w), sigmas=sigma, n_routed=80,
                                    n_constants=nconst, gates=b.gates)
    plain = ctx.prove_step(si(w))
    checked = ctx.prove_step_checked(si(w), chk)
    for k in ("caps", "openings", "fri", "challenges"):
        assert (plain[k] == checked[k]).all(), k
    h = api.hash_no_pad(np.array(circ.public_inputs(w), np.uint64))
    rng = np.random.default_rng(4)
    for _ in range(3):
        bad = w.copy()
        c, r = int(rng.integers(135)), int(rng.integers(b.n))
        bad[c, r] = (int(bad[c, r]) + 1) % P
        ok, msg = b.circuit.check_witness(bad, h)
        if ok:
            continue
        with pytest.raises(api.WitnessError) as e:
            ctx.prove_step_checked(si(bad), chk)
        assert str(e.value) == msg and e.value.status == api.ERR_WITNESS == -6
        again = ctx.prove_step(si(w))   # the context is still usable and proves as before
        for k in ("caps", "openings", "fri"):
            assert (again[k] == plain[k]).all(), k
    again = ctx.prove_step_checked(si(w), chk)
    assert (again["fri"] == plain["fri"]).all()
    chk.free()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. checked IVC chains

def test_checked_ivc_chain_matches_the_golden_chain():
    from test_cyclic_cpu import GOLDEN_CHAIN, n8_chain_inputs
    N, n_lwe, log_n = 8, 1, 13
    ring, (s_to, s_lwe, s_glwe, bsk, ksk), delta, testv, ct = n8_chain_inputs()
    cyc, dum = (circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, n_lwe, log_n))
    c = vpbs_amd.Context(0, log_n_max=16)
    ivc = api.Ivc(c, cyc, dum, N, K, K * ELL * K * N)
    frozen = json.load(open(GOLDEN_CHAIN))
    bsk_flat, ksk_flat = np.stack([T.flatten_ggsw(g) for g in bsk]), T.flatten_ggsw(ksk)
    steps = n_lwe + 2
    assert ivc.witness_checks() == (0, 0)
    for batch, late in ((0, False), (3, False), (3, True)):
        ivc.set_device_witness(ELL, LOGB, batch, late)
        ivc.set_check_witness(True)
        blob, _ = ivc.prove_pbs(testv, ct, bsk_flat, ksk_flat)
        assert (len(blob), hashlib.sha256(blob).hexdigest()) == (frozen["bytes"], frozen["sha256"]), (batch, late)
        assert ivc.witness_checks() == (steps + 1, 0), (batch, late)
    ivc.set_check_witness(False)
    ivc.set_device_witness(ELL, LOGB, 0, False)
    blob, _ = ivc.prove_pbs(testv, ct, bsk_flat, ksk_flat)
    assert hashlib.sha256(blob).hexdigest() == frozen["sha256"] and ivc.witness_checks() == (0, 0)
    ivc.free()
    # a sharded chain (a communicator, here of one rank) refuses checking
    import ctypes as C
    comm = api.CommC()
    comm.rank, comm.world = 0, 1
    comm.allgather = api.ALLGATHER_FN(lambda user, local, words, out: (C.memmove(out, local, 8 * words), 0)[1])
    comm.allreduce_sum = api.ALLREDUCE_FN(lambda user, inout, words: 0)
    ivc = api.Ivc(c, cyc, dum, N, K, K * ELL * K * N, comm)
    with pytest.raises(api.VpbsError, match="sharded"):
        ivc.set_check_witness(True)
    ivc.set_check_witness(False)
    ivc.free()
    c.close()
