"""GPU tests (-m gpu) of the batch verifier of serialised step proofs (vpbs_proof_verifier_*, csrc/verify_batch.hip).  The yardstick
throughout is the host: api.step_proof_from_bytes + api.verify_step on the same bytes.  The device must give every byte string the host's
verdict, and name the first failing check in the host verifier's order."""
import hashlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import export_circuits
import oracle as orc
import step_circuit as sc
import tfhe_oracle as T
import vpbs_amd
from batch_verify_layout import proof_layout
from vpbs_amd import api, circuit_file, synth

pytestmark = pytest.mark.gpu
P = api.P
K, ELL, LOGB = 2, 4, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_PI = 1 << 13
ERR_INVALID = -1   # VPBS_ERR_INVALID
OK, MALFORMED, VANISHING, POW, FRI, MERKLE = (api.VERIFY_OK, api.VERIFY_MALFORMED, api.VERIFY_VANISHING, api.VERIFY_POW, api.VERIFY_FRI,
                                             api.VERIFY_MERKLE)


class Circ:
    """what both verifiers need of one circuit, and its proofs as bytes"""

    def __init__(self, name, cap, ncols, digest, log_n, n_constants, n_routed, gates, full=True, compat=None):
        self.name, self.cap, self.ncols, self.digest, self.log_n = name, np.asarray(cap, np.uint64).reshape(-1, 4), list(ncols), digest, log_n
        self.n_constants, self.n_routed, self.gates, self.full, self.compat = n_constants, n_routed, gates, full, compat
        self.blobs = []

    def kw(self):
        return dict(check_permutation=self.full, n_constants=self.n_constants, n_routed=self.n_routed, gates=self.gates if self.full else None)

    def verifier(self, ctx, max_batch=1024, compat="own", max_public_inputs=MAX_PI):
        return api.ProofVerifier(ctx, self.cap, self.ncols, self.digest, self.log_n, max_batch=max_batch, max_public_inputs=max_public_inputs,
                                 compat=self.compat if compat == "own" else compat, **self.kw())

    def host(self, blob, compat="own", max_public_inputs=MAX_PI):
        cp = self.compat if compat == "own" else compat
        try:
            proof, pis = api.step_proof_from_bytes(blob, self.ncols, self.log_n, self.n_constants, max_public_inputs=max_public_inputs, compat=cp)
        except api.VpbsError:
            return False
        return api.verify_step(proof, self.cap, self.ncols, self.digest, pis, self.log_n, compat=cp, **self.kw())

    def layout(self):
        return proof_layout(self.ncols, self.log_n, self.n_constants)


@pytest.fixture(scope="module")
def ctx():
    c = vpbs_amd.Context(0, log_n_max=16)
    yield c
    c.close()


def _prove(ctx, c, log_n, wires, cs, sigma, pis):
    si = ctx.make_step_inputs(log_n, wires, None, None, cs, c.digest, pis, sigmas=sigma, n_routed=80, n_constants=c.n_constants, gates=c.gates)
    return ctx.step_proof_to_bytes(si, c.n_constants, ctx.prove_step(si))


def step_n8(ctx, n_proofs=3):
    circ = sc.StepCircuit(api, 8, K, ELL, LOGB, 6, orc.negacyclic_params(3))
    b = circ.built
    targets = ([t for p in circ.acc_init for t in p] + [t for p in circ.acc_in for t in p] + circ.ggsw_flat + [circ.counter, circ.mask] +
               circ.bsk_hash_in + circ.lwe_hash_in)
    plan = b.circuit.witness_plan([b.pos(t) for t in targets])
    sigma = b.circuit.sigma_values()
    cs = ctx.commit_values(np.concatenate([b.constants, sigma]))
    nconst = b.constants.shape[0]
    c = Circ("step_n8", cs.cap(), [nconst + 80, 135, 20, 16], np.array([1, 2, 3, 4], np.uint64), b.log_n, nconst, 80, b.gates)
    for seed in range(n_proofs):
        vals = np.random.default_rng(100 + seed).integers(0, P, size=len(targets), dtype=np.uint64)
        vals[len(targets) - 10] = 3
        w = plan.run(vals)
        c.blobs.append(_prove(ctx, c, b.log_n, w, cs, sigma, circ.public_inputs(w)))
    plan.free()
    return c


def step_file(ctx, N, n_proofs):
    d = circuit_file.load(export_circuits.ensure_step_circuit(N, K, ELL, LOGB, 728))
    plan = d.circuit.witness_plan(d.preset_pos)
    sigma = d.circuit.sigma_values()
    cs = ctx.commit_values(np.concatenate([d.constants, sigma]))
    c = Circ("step_%d" % N, cs.cap(), [d.n_constants + 80, 135, 20, 16], np.array([11, 22, 33, 44], np.uint64), d.log_n, d.n_constants, 80,
             d.gates)
    for seed in range(n_proofs):
        v = np.random.default_rng(N + seed).integers(0, P, size=len(d.preset_pos), dtype=np.uint64)
        v[len(d.preset_pos) - 10] = 1 + seed
        w = plan.run(v)
        pis = np.array([w[col][row] for col, row in d.pi_pos], np.uint64)
        c.blobs.append(_prove(ctx, c, d.log_n, w, cs, sigma, pis))
    plan.free()
    return c


def cyclic_n8(ctx):
    """the last proofs of Ivc.prove_pbs on the n8_chain_inputs chain (steps 1, 2 and the whole chain, whose bytes are pinned)"""
    from test_cyclic_cpu import GOLDEN_CHAIN, n8_chain_inputs
    N, n_lwe, log_n = 8, 1, 13
    ring, (s_to, s_lwe, s_glwe, bsk, ksk), delta, testv, ct = n8_chain_inputs()
    cyc, dum = (circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(N, K, ELL, LOGB, n_lwe, log_n))
    ivc = api.Ivc(ctx, cyc, dum, N, K, K * ELL * K * N)
    bsk_flat, ksk_flat = np.stack([T.flatten_ggsw(g) for g in bsk]), T.flatten_ggsw(ksk)
    vk, _ = ivc.verifier_data()
    c = Circ("cyclic_n8", vk[4:].reshape(-1, 4), [cyc.n_constants + 80, 135, 20, 16], vk[:4], log_n, cyc.n_constants, 80, cyc.gates)
    for steps in (1, 2, 0):
        blob, _ = ivc.prove_pbs(testv, ct, bsk_flat, ksk_flat, steps)
        c.blobs.append(blob)
    frozen = json.load(open(GOLDEN_CHAIN))
    assert (len(c.blobs[-1]), hashlib.sha256(c.blobs[-1]).hexdigest()) == (frozen["bytes"], frozen["sha256"])
    ivc.free()
    return c


def fri_only(ctx, n_proofs=3, compat=None):
    """synthetic columns (bench.py's kind of trace): transcript + FRI only"""
    log_n = 10
    inputs = synth.step_inputs(log_n)
    cs = ctx.commit_values(inputs["constants_sigmas"])
    ncols = [inputs["constants_sigmas"].shape[0], inputs["wires"].shape[0], inputs["zs_partial_products"].shape[0], inputs["quotient"].shape[0]]
    c = Circ("fri_only", cs.cap(), ncols, np.array([5, 6, 7, 8], np.uint64), log_n, 0, 0, None, full=False, compat=compat)
    for seed in range(n_proofs):
        pis = synth.field_elements(300 + seed, 40 + seed)
        si = ctx.make_step_inputs(log_n, inputs["wires"], inputs["zs_partial_products"], inputs["quotient"], cs, c.digest, pis)
        c.blobs.append(ctx.step_proof_to_bytes(si, 0, ctx.prove_step(si)))
    return c


@pytest.fixture(scope="module")
def circuits(ctx):
    return {"step_n8": step_n8(ctx), "cyclic_n8": cyclic_n8(ctx), "fri_only": fri_only(ctx)}


def agree(ctx, c, blobs, **kw):
    """device (verdicts, reasons) of one batch, asserted equal to the host's verdicts"""
    v = c.verifier(ctx, max_batch=max(1, len(blobs)), **kw)
    got, why = v.verify(blobs)
    v.close()
    want = np.array([c.host(b, **kw) for b in blobs], np.uint8)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (c.name, bad[:10].tolist(), got[bad[:10]].tolist(), want[bad[:10]].tolist(), why[bad[:10]].tolist())
    assert ((why == OK) == (got == 1)).all()
    return got, why


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. acceptance

def test_device_verifier_accepts_valid_proofs(ctx, circuits):
    for c in list(circuits.values()) + [step_file(ctx, 1024, 3)]:
        assert len(set(c.blobs)) == len(c.blobs) >= 3
        got, why = agree(ctx, c, c.blobs)
        assert got.tolist() == [1] * len(c.blobs) and why.tolist() == [OK] * len(c.blobs), c.name


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. tamper sweep

def put_word(blob, off, v):
    b = bytearray(blob)
    b[off:off + 8] = int(v).to_bytes(8, "little")
    return bytes(b)


def word_at(blob, off):
    return int.from_bytes(blob[off:off + 8], "little")


def tampers(c, blob, rng, n):
    """n seeded corruptions of one proof covering every section and every kind of damage"""
    lay = c.layout()
    words = lay["words"]              # [(section, byte offset)] of every word before the public inputs
    pi_start = lay["fixed_len"] + 8
    n_pi = (len(blob) - pi_start) // 8
    out = []
    sections = sorted(set(s for s, _ in words))
    for k in range(n):
        kind = k % 8
        if kind in (0, 1, 2):   # +1 mod p at a uniformly drawn position of a section (the sections in turn), the public inputs included
            sec = (sections + ["pi"])[(k // 8) % (len(sections) + 1)]
            if sec == "pi":
                off = pi_start + 8 * int(rng.integers(0, n_pi))
            else:
                cand = [o for s, o in words if s == sec]
                off = cand[int(rng.integers(0, len(cand)))]
            out.append(put_word(blob, off, (word_at(blob, off) + 1) % P))
        elif kind == 3:         # a word set to a value >= p
            s, off = words[int(rng.integers(0, len(words)))]
            out.append(put_word(blob, off, P + int(rng.integers(0, 1 << 32))))
        elif kind == 4:         # the PoW witness
            out.append(put_word(blob, lay["pow"], [P, (1 << 64) - 1, int(rng.integers(0, P, dtype=np.uint64))][(k // 8) % 3]))
        elif kind == 5:         # a path-length byte
            b = bytearray(blob)
            pos = lay["len_bytes"][int(rng.integers(0, len(lay["len_bytes"])))]
            b[pos] = (b[pos] + 1 + int(rng.integers(0, 254))) % 256
            out.append(bytes(b))
        elif kind == 6:         # truncated or extended by 1 or 8 bytes
            d = [1, 8, -1, -8][(k // 8) % 4]
            out.append(blob + bytes(d) if d > 0 else blob[:d])
        else:                   # the public-input count prefix
            d = [1, -1, 1 << 40, MAX_PI + 1 - n_pi][(k // 8) % 4]
            out.append(put_word(blob, lay["fixed_len"], (n_pi + d) % (1 << 64)))
    return out


@pytest.mark.parametrize("which", ["step_n8", "cyclic_n8", "fri_only"])
def test_tamper_sweep_matches_the_host(ctx, circuits, which):
    c = circuits[which]
    rng = np.random.default_rng(zlib.crc32(which.encode()))
    batch, originals = [], []
    for j, blob in enumerate(c.blobs):
        for t in tampers(c, blob, rng, 90):
            batch.append(t)
        originals.append(len(batch))
        batch.append(blob)
    assert len(batch) - len(originals) >= 256
    got, why = agree(ctx, c, batch)
    assert all(got[i] == 1 for i in originals)
    assert (got == 0).sum() >= 200   # a random canonical PoW witness may pass the leading-zero test: then the host accepts it as well


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. reasons of targeted tampers

@pytest.mark.parametrize("which", ["step_n8", "cyclic_n8"])
def test_reasons_of_targeted_tampers(ctx, circuits, which):
    c = circuits[which]
    blob = c.blobs[0]
    lay = c.layout()
    rng = np.random.default_rng(5)
    cases = []

    def pick(sec):
        cand = [o for s, o in lay["words"] if s == sec]
        return cand[int(rng.integers(0, len(cand)))]
    for _ in range(6):
        off = pick("sibling")
        cases.append((put_word(blob, off, (word_at(blob, off) + 1) % P), MERKLE))
        for sec in ("leaf", "fold"):
            off = pick(sec)
            cases.append((put_word(blob, off, (word_at(blob, off) + 1) % P), FRI))
        off = pick("openings_quotient")
        cases.append((put_word(blob, off, (word_at(blob, off) + 1) % P), VANISHING))
        cases.append((put_word(blob, pick("caps"), P), MALFORMED))
        cases.append((put_word(blob, pick("fold"), (1 << 64) - 1), MALFORMED))
    cases.append((put_word(blob, lay["pow"], P), POW))
    cases.append((put_word(blob, lay["pow"], (1 << 64) - 1), POW))
    cases.append((blob[:-1], MALFORMED))
    cases.append((blob + bytes(8), MALFORMED))
    got, why = agree(ctx, c, [b for b, _ in cases])
    assert why.tolist() == [r for _, r in cases]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. batch shapes and errors

def test_batch_shapes_and_errors(ctx, circuits):
    import ctypes as C
    c = circuits["step_n8"]
    rng = np.random.default_rng(9)
    pool = []
    for blob in c.blobs:
        pool += tampers(c, blob, rng, 24) + [blob]
    max_batch = 96
    pool = (pool * 2)[:max_batch]
    v = c.verifier(ctx, max_batch=max_batch)
    full, full_why = v.verify(pool)
    want = np.array([c.host(b) for b in pool], np.uint8)
    assert (full == want).all()
    for n in (1, 63, 64, 65, max_batch):
        got, why = v.verify(pool[:n])
        assert (got == full[:n]).all() and (why == full_why[:n]).all(), n
    # errors: count > max_batch, decreasing offsets
    buf, offs = api.pack_proofs(pool[:2])
    u8p = C.POINTER(C.c_uint8)
    out = np.zeros(max_batch + 1, np.uint8)
    big_buf, big_offs = api.pack_proofs(pool[:1] * (max_batch + 1))
    assert api.lib().vpbs_proof_verifier_run(v.h, big_buf.ctypes.data_as(u8p), big_offs.ctypes.data_as(C.POINTER(C.c_size_t)), max_batch + 1,
                                             out.ctypes.data_as(u8p), None) == ERR_INVALID
    bad = offs.copy()
    bad[1], bad[2] = offs[2], offs[1]
    assert api.lib().vpbs_proof_verifier_run(v.h, buf.ctypes.data_as(u8p), bad.ctypes.data_as(C.POINTER(C.c_size_t)), 2,
                                             out.ctypes.data_as(u8p), None) == ERR_INVALID
    assert v.verify([])[0].size == 0
    v.close()
    # gate_terms_zeta without gates is refused at create
    with pytest.raises(api.VpbsError):
        api.ProofVerifier(ctx, c.cap, c.ncols, c.digest, c.log_n, n_constants=c.n_constants, n_routed=80, gate_terms_zeta=np.zeros(4, np.uint64))
    # proofs of circuit A through a verifier of circuit B: the host's verdicts
    cy = circuits["cyclic_n8"]
    agree(ctx, cy, c.blobs + cy.blobs)
    agree(ctx, c, c.blobs + cy.blobs)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. compat positions

def test_compat_positions(ctx):
    for over in (dict(fri_mul_final_by_x=1), dict(bytes_pi_len_prefix=0)):
        table = api.compat(**over)
        ctx.set_compat(**over)
        try:
            c = fri_only(ctx, 2, compat=table)
        finally:
            ctx.set_compat()
        got, why = agree(ctx, c, c.blobs)
        assert got.tolist() == [1, 1], over
        agree(ctx, c, c.blobs, compat=None)   # under the default table: whatever the host says


def test_no_public_inputs_capacity(ctx):
    """max_public_inputs = 0 (a circuit without public inputs): the length and the count prefix are still checked, proof by proof"""
    c = fri_only(ctx, 1)
    log_n = c.log_n
    inputs = synth.step_inputs(log_n)
    cs = ctx.commit_values(inputs["constants_sigmas"])
    si = ctx.make_step_inputs(log_n, inputs["wires"], inputs["zs_partial_products"], inputs["quotient"], cs, c.digest, np.zeros(0, np.uint64))
    blob = ctx.step_proof_to_bytes(si, 0, ctx.prove_step(si))
    zero = Circ("fri_only_no_pi", cs.cap(), c.ncols, c.digest, log_n, 0, 0, None, full=False)
    with_pi = c.blobs[0]
    for kw in (dict(max_public_inputs=0), dict(max_public_inputs=1)):
        batch = [blob, blob + bytes(1), blob + bytes(8), blob[:-1], blob[:-8], with_pi, blob]
        got, why = agree(ctx, zero, batch, **kw)
        assert got.tolist() == [1, 0, 0, 0, 0, 0, 1], kw
        assert why.tolist()[1:6] == [MALFORMED] * 5


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. paper size

def test_paper_size_batch_of_730(ctx):
    c = step_file(ctx, 1024, 8)
    rng = np.random.default_rng(730)
    batch = list(c.blobs)
    per = (730 - len(batch)) // len(c.blobs) + 1
    for blob in c.blobs:
        batch += tampers(c, blob, rng, per)
    batch = batch[:730]
    got, why = agree(ctx, c, batch)
    assert got[:8].tolist() == [1] * 8


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. the tool

def test_prove_pbs_tool_with_the_device_verifier():
    export_circuits.ensure_step_circuit(1024, K, ELL, LOGB, 14)   # the tool loads circuit files, it does not make them
    env = dict(os.environ, VPBS_PBS_VERIFY="device")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "prove_pbs.py"), "14", "4", "2"], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["step_proofs"] == 16 and "all 16 proofs verified" in d["checks"] and "vpbs_proof_verifier" in d["checks"]
