"""GPU tests (-m gpu) of the device verifiers on forged proofs (tests/forged_proofs.py) that pass every check before the one under test.
Genuine proofs only ever reach the device's late stages with pseudo-random operands, and a tampered word stops a proof at the first stage
that reads it; a forgery makes vb_gates / vb_vanishing, the transcript after the openings and vb_fri compute on values the prover chose
(edge openings, a solved quotient chunk, folds that interpolate to edge values) and the device must name exactly the next check.  The
expected reason comes from the oracle (orc_check_vanishing_at_zeta, oracle/gates.c, orc_verify_fri_checks), never from the product."""
import random
import time

import numpy as np
import pytest

import forged_proofs as fp
import gates_oracle as go
import vpbs_amd
from test_gpu_batch_verify import fri_only, step_n8
from test_gpu_pbs_verify import Pbs, check
from vpbs_amd import api

pytestmark = pytest.mark.gpu
P = api.P
OK, VANISHING, POW, FRI, MERKLE = api.VERIFY_OK, api.VERIFY_VANISHING, api.VERIFY_POW, api.VERIFY_FRI, api.VERIFY_MERKLE
REASONS = (OK, VANISHING, POW, FRI, MERKLE)
BY_NAME = {"OK": OK, "VANISHING": VANISHING, "POW": POW, "FRI": FRI, "MERKLE": MERKLE}
DIGEST = np.array([11, 22, 33, 44], np.uint64)
FORGERS_PER_SHAPE = 2


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pbs(ctx):
    """cyclic_n8 (N = 8, n = 1, log_n 13) chains under one key set: the genuine proofs of that shape and their statements"""
    S = Pbs(ctx, 8, 1, 13, 91, [1, 0])
    yield S
    S.ivc.free()


def spec_of(gates):
    """the explicit gate spec of an api.GateSet (its *_from_config parameters filled in)"""
    return [(api.GATE_KINDS[g.kind], g.p0, g.p1, g.p2) for g in gates]


def api_compat(shape):
    return api.compat(**shape.compat_over) if shape.compat_over else None


def forge(shape, seed0, public_inputs=None):
    """FORGERS_PER_SHAPE forgers of a shape -> (blobs, expected reasons, kinds); the expected reason is the oracle's and must be the class's"""
    blobs, want, kinds = [], [], []
    for seed in range(seed0, seed0 + FORGERS_PER_SHAPE):
        fill, chunk = fp.forger_variants(seed)
        for kind, f in fp.Forger(shape, seed, fill, chunk, public_inputs).forge().items():
            van, checks, _ = fp.oracle_checks(f)
            r = fp.expected_reason(van, checks, REASONS)
            assert r == BY_NAME[fp.NOMINAL[kind]], (shape.name, seed, kind, van, checks)
            blobs.append(f.blob())
            want.append(r)
            kinds.append(kind)
    return blobs, want, kinds


def device(ctx, shape, blobs, gates=None, max_public_inputs=64):
    v = api.ProofVerifier(ctx, shape.cap, shape.ncols, shape.digest, shape.log_n, num_challenges=shape.nc, check_permutation=not shape.fri_only,
                          n_constants=shape.n_constants, n_routed=shape.n_routed,
                          gates=None if shape.fri_only else (gates or api.GateSet(shape.spec)), compat=api_compat(shape),
                          max_batch=len(blobs), max_public_inputs=max_public_inputs)
    got, why = v.verify(blobs)
    v.close()
    return got, why


def gate_demo(ctx):
    """the ALL gate set's demo circuit at log_n 7 (tests/test_gpu_edge_operands.py): its cap, and one genuine proof"""
    gs, ps = go.GateSet(fp.ALL), api.GateSet(fp.ALL)
    rnd = random.Random(7)
    cpis = [rnd.randrange(P) for _ in range(4)]
    constants, wires, sigma, _ = go.demo_circuit(rnd, gs, 7, cpis)
    nconst = constants.shape[0]
    cs = ctx.commit_values(np.concatenate([constants, sigma]))
    si = ctx.make_step_inputs(7, wires, None, None, cs, DIGEST, cpis, sigmas=sigma, n_routed=80, n_constants=nconst, gates=ps)
    blob = ctx.step_proof_to_bytes(si, nconst, ctx.prove_step(si))
    cap = cs.cap()
    cs.free()
    return dict(cap=cap, digest=DIGEST), nconst, ps, [blob]


def test_device_verifier_names_the_check_each_forgery_reaches(ctx, pbs):
    t0 = time.time()
    real = {"all_log7": gate_demo(ctx)}
    c = step_n8(ctx, 2)
    real["step_n8"] = dict(cap=c.cap, digest=c.digest, spec=spec_of(c.gates)), c.n_constants, c.gates, c.blobs
    real["cyclic_n8"] = (dict(cap=pbs.cap, digest=pbs.digest, spec=spec_of(pbs.gates)), pbs.n_constants, pbs.gates,
                         [b for b, _, _, _ in pbs.cases])
    fo = fri_only(ctx, 2)
    real["fri_only_log10"] = dict(cap=fo.cap, digest=fo.digest, ncols=fo.ncols), 0, None, fo.blobs
    total, seen, summary = 0, set(), {}
    for k, (name, kw) in enumerate(fp.shapes()):
        over, nconst, gates, genuine = real.get(name, ({}, None, None, []))
        shape = fp.make_shape(name, kw, **over)
        if nconst is not None:
            assert shape.n_constants == nconst, name
        if name in ("step_n8", "cyclic_n8"):
            assert shape.log_n == (c.log_n if name == "step_n8" else pbs.log_n) and shape.ncols == (c.ncols if name == "step_n8" else pbs.ncols)
        blobs, want, kinds = forge(shape, 2 * k)
        batch = list(genuine) + blobs
        got, why = device(ctx, shape, batch, gates, max_public_inputs=1024 if genuine else 64)
        ng = len(genuine)
        assert got[:ng].tolist() == [1] * ng and why[:ng].tolist() == [OK] * ng, (name, why[:ng].tolist())
        bad = [(kinds[i], int(why[ng + i]), want[i]) for i in range(len(blobs)) if why[ng + i] != want[i]]
        assert not bad and not got[ng:].any(), (name, bad[:8])
        total += len(blobs)
        seen |= set(want)
        summary[name] = sorted(set(kinds))
    assert total >= 300, total
    assert seen == {VANISHING, POW, FRI, MERKLE}, seen
    print("\nforged blobs: %d over %d shapes in %.1f s" % (total, len(summary), time.time() - t0))


def test_pbs_verifier_on_forged_chain_proofs(ctx, pbs):
    """cyclic_n8 forgeries carrying a genuine chain proof's public inputs: the vPBS verifier fails them at the proof (PBS_PROOF) with the
    step verifier's reason, genuine cases in the same batch pass"""
    name, kw = next(e for e in fp.shapes() if e[0] == "cyclic_n8")
    shape = fp.make_shape(name, kw, cap=pbs.cap, digest=pbs.digest, spec=spec_of(pbs.gates))
    cases, want = list(pbs.cases), [OK] * len(pbs.cases)
    for j, (blob, tv, ct, oc) in enumerate(pbs.cases):
        _, pis = api.step_proof_from_bytes(blob, pbs.ncols, pbs.log_n, pbs.n_constants)
        blobs, reasons, _ = forge(shape, 100 + 2 * j, public_inputs=pis)
        cases += [(b, tv, ct, oc) for b in blobs]
        want += reasons
    pv = pbs.verifier(max_batch=len(cases))
    try:
        v, r, sub = check(pbs, pv, cases)
    finally:
        pv.close()
    ng = len(pbs.cases)
    assert v[:ng].all() and (r[:ng] == api.PBS_OK).all()
    assert (r[ng:] == api.PBS_PROOF).all() and not v[ng:].any()
    assert sub.tolist() == want
    _, step_why = device(ctx, shape, [b for b, _, _, _ in cases], pbs.gates, max_public_inputs=1024)
    assert step_why.tolist() == sub.tolist()
