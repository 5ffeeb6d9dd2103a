"""CPU tests of the proof forger (tests/forged_proofs.py) against the oracle: every class and control of every shape reaches exactly the check
it is built to reach -- the vanishing identity holds where it should, the PoW response has 16 leading zeros where it was ground, and the
oracle's exhaustive FRI check (orc_verify_fri_checks) reports exactly the failures the class leaves -- and the product's host parser reads
every blob back word for word, and its host verifier rejects it.  tests/test_gpu_forged_proofs.py puts the same forgeries through the
device verifiers."""
import numpy as np
import pytest

import forged_proofs as fp
import oracle as orc
from vpbs_amd import api

SHAPES = fp.shapes()
POW_GROUND = {"F2", "F3", "fold+1", "final+1"}
FRI_CHECKS = {"F2": {"fri", "merkle"}, "F3": {"merkle"}, "fold+1": {"fri", "merkle"}, "final+1": {"fri", "merkle"}}


def api_compat(shape):
    return api.compat(**shape.compat_over) if shape.compat_over else None


def host_verify(shape, blob):
    cp = api_compat(shape)
    proof, pis = api.step_proof_from_bytes(blob, shape.ncols, shape.log_n, shape.n_constants, num_challenges=shape.nc, compat=cp)
    if shape.fri_only:
        ok = api.verify_step(proof, shape.cap, shape.ncols, shape.digest, pis, shape.log_n, num_challenges=shape.nc, check_permutation=False,
                             compat=cp)
    else:
        ok = api.verify_step(proof, shape.cap, shape.ncols, shape.digest, pis, shape.log_n, num_challenges=shape.nc, n_constants=shape.n_constants,
                             n_routed=shape.n_routed, gates=api.GateSet(shape.spec), compat=cp)
    return proof, pis, ok


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=[n for n, _ in SHAPES])
def test_forgeries_reach_exactly_their_check(k):
    name, kw = SHAPES[k]
    shape = fp.make_shape(name, kw)
    fill, chunk = fp.forger_variants(k)
    forged = fp.Forger(shape, k, fill, chunk).forge()
    assert set(forged) == set(shape.classes()) | set(shape.controls()), sorted(forged)
    reasons = {}
    for kind, f in forged.items():
        van, checks, resp = fp.oracle_checks(f)
        # the vanishing identity at zeta: the forger's big-int permutation part + oracle/gates.c against orc_check_vanishing_at_zeta
        assert van == (None if shape.fri_only else kind != "quotient+1"), (name, kind)
        # the PoW: ground for F2, F3 and the FRI controls, F1's witness elsewhere
        assert (resp >> (64 - fp.POW_BITS) == 0) == (kind in POW_GROUND), (name, kind, hex(resp))
        if kind in FRI_CHECKS:
            assert checks == FRI_CHECKS[kind], (name, kind, checks)
        else:
            assert "pow" in checks, (name, kind, checks)
        reasons[kind] = fp.expected_reason(van, checks, ("OK", "VANISHING", "POW", "FRI", "MERKLE"))
        # the host parser reads the blob back word for word; the host verifier rejects it
        proof, pis, ok = host_verify(shape, f.blob())
        for key in ("caps", "openings", "fri"):
            assert (proof[key] == f.proof()[key]).all(), (name, kind, key)
        assert (pis == f.pis).all() and not ok, (name, kind)
    assert reasons == {kind: fp.NOMINAL[kind] for kind in forged}, (name, reasons)


def test_forger_solves_and_grinds_like_an_honest_prover():
    """on an honest oracle proof of the gate demo circuit: solving quotient chunk 0 or 7 from the other openings gives back the honest chunk,
    and orc_pow_grind on the honest transcript gives the prover's witness (the smallest nonce)"""
    import random

    import gates_oracle as go
    import step_oracle
    rng = random.Random(17)
    gs = go.GateSet(fp.ALL)
    log_n = 6
    cpis = [rng.randrange(fp.P) for _ in range(4)]
    constants, wires, sigma, _ = go.demo_circuit(rng, gs, log_n, cpis)
    digest = np.array([11, 22, 33, 44], np.uint64)
    proof = step_oracle.prove_step({"constants_sigmas": np.concatenate([constants, sigma]), "wires": wires, "quotient": None}, digest, cpis,
                                   log_n, sigmas=sigma, n_routed=80, n_constants=constants.shape[0], gates=gs)
    shape = fp.Shape.of_gates("honest", gs, log_n, cap=proof["cs_cap"], digest=digest)
    f = fp.Forger(shape, 0, public_inputs=cpis)
    ch = orc.ChallengerState()
    ch.observe(digest)
    ch.observe(orc.hash_no_pad(cpis))
    ch.observe(proof["caps"][0])
    f.betas, f.gammas = ch.get_n(2), ch.get_n(2)
    ch.observe(proof["caps"][1])
    f.alphas = ch.get_n(2)
    ch.observe(proof["caps"][2])
    f.zeta = tuple(ch.get_n(2))
    assert [int(x) for x in proof["challenges"]] == f.betas + f.gammas + f.alphas + list(f.zeta)
    honest = fp.pairs(proof["openings"])
    for chunk in (0, 7):
        f.open, f.solve_chunk = list(honest), chunk
        j = f.o_quot(8 + chunk)
        f.open[j] = (0, 0)
        f.solve_quotient()
        assert f.open == honest, chunk
    ch.observe(proof["openings"])
    ch.get_n(2)
    params, fri = shape.params, proof["fri"]
    for r in range(params.n_rounds):
        ch.observe(fri[r * 64:(r + 1) * 64])
        ch.get_n(2)
    n_final = 2 << (log_n - sum(params.arity_bits[r] for r in range(params.n_rounds)))
    ch.observe(fri[-1 - n_final:-1])
    assert orc.pow_grind(ch) == int(fri[-1])
