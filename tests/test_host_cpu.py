"""CPU tests (-m "not gpu") of the product's host side: ABI surface, host Challenger/Poseidon, parameter tables,
synthetic inputs, sharding plan (incl. a world_size-2 gloo run).  No device compute is called."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fri_shapes
import oracle as orc
import step_oracle
import vpbs_amd
from vpbs_amd import api, sharding, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
P = api.P


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(api.LIB_PATH):
        api.build_library()


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "vpbs_prover.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vpbs_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 35
    L = ctypes.CDLL(api.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(L, name), "missing export: " + name
    assert declared == set(api.SIGNATURES), declared ^ set(api.SIGNATURES)


def test_rust_binding_matches_the_header():
    """The Rust side of the boundary (no rustc in the authoring image, so this test stands where the compiler would):
    bindings/rust/vpbs_sys.rs is what tools/gen_rust_ffi.py makes of the header TODAY (a stale binding fails), it declares every function
    the header does with the header's arity, and every `fn vpbs_*` declaration INTEGRATION.md shows is one of its lines -- a document that
    drifts from the header (round 3: vpbs_ivc_set_device_witness had four arguments there and five here) is a test failure."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi
    want = gen_rust_ffi.generate()
    have = open(gen_rust_ffi.OUT).read()
    assert have == want, "bindings/rust/vpbs_sys.rs is stale: run tools/gen_rust_ffi.py"
    norm = lambda line: " ".join(line.replace("pub fn", "fn").split())
    generated = {}
    for line in have.splitlines():
        m = re.match(r"\s*pub fn (vpbs_\w+)\(", line)
        if m:
            generated[m.group(1)] = norm(line)
    # arity against an independent reading of the header (comma count of every prototype)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vpbs_prover.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(vpbs_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr) if "(*" not in m.group(0)}
    assert set(protos) == set(generated) and len(generated) >= 120
    for name, args in protos.items():
        n_c = 0 if args.strip() in ("", "void") else args.count(",") + 1
        inner = generated[name][generated[name].index("(") + 1:generated[name].rindex(")")]
        n_r = 0 if not inner.strip() else inner.count(",") + 1
        assert n_c == n_r, (name, n_c, n_r)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert gen_rust_ffi.integration_excerpt() in doc, "INTEGRATION.md's excerpt is stale: run tools/gen_rust_ffi.py --integration"
    shown = []
    for block in re.findall(r"```rust\n(.*?)```", doc, flags=re.S):
        for line in block.splitlines():
            m = re.match(r"\s*(?:pub )?fn (vpbs_\w+)\(", line)
            if m:
                shown.append((m.group(1), norm(line.split("//")[0].rstrip())))
    assert len(shown) >= 50
    for name, line in shown:
        assert name in generated, "INTEGRATION.md declares a function the header does not have: " + name
        assert line == generated[name], "INTEGRATION.md and the header disagree on %s:\n  doc:    %s\n  header: %s" % (name, line, generated[name])
    for must in ("vpbs_prove_step", "vpbs_verify_step", "vpbs_step_proof_to_bytes", "vpbs_rccl_unique_id", "vpbs_comm_rccl_create",
                 "vpbs_comm_rccl_destroy", "vpbs_ivc_set_device_witness"):
        assert must in dict(shown), must
    assert "late_on_device: i32" in dict(shown)["vpbs_ivc_set_device_witness"]


def test_no_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(api.VpbsError):
        vpbs_amd.Context(0)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "verifiable-fhe-paper_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp", ".inc")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "libvpbs_oracle" not in txt and "import oracle" not in txt and "orc_" not in txt, f


def test_host_challenger_matches_oracle():
    rng = np.random.default_rng(7)
    a, b = api.ChallengerState(), orc.ChallengerState()
    for kind, k in [("o", 5), ("g", 3), ("o", 8), ("g", 1), ("o", 64), ("g", 10), ("o", 1), ("g", 2)]:
        if kind == "o":
            xs = rng.integers(0, P, size=k, dtype=np.uint64)
            a.observe(xs); b.observe(xs)
        else:
            assert a.get_n(k) == b.get_n(k)
    assert a.state_words() == b.state_words()


def test_host_poseidon_kats_via_hash():
    kat = json.load(open(os.path.join(GOLD, "poseidon_kat.json")))
    # hash_no_pad of 8 zeros = first 4 words of perm(0^12)
    assert [int(v) for v in api.hash_no_pad(np.zeros(8, np.uint64))] == kat["kats"][0]["output"][:4]
    rng = np.random.default_rng(3)
    for n in (1, 7, 8, 9, 24, 135, 4173):
        x = rng.integers(0, P, size=n, dtype=np.uint64)
        assert list(api.hash_no_pad(x)) == list(orc.hash_no_pad(x))


@pytest.mark.parametrize("log_n", [3, 4, 5, 6, 7, 8, 9, 10, 11])
def test_ntt_params_match_reference_tables(log_n):
    g = json.load(open(os.path.join(GOLD, "ntt_params_%d.json" % (1 << log_n))))
    roots, inv, ninv = api.ntt_params(log_n)
    import hashlib, struct
    assert ninv == g["NINV"]
    assert hashlib.sha256(struct.pack("<%dQ" % g["N"], *[int(v) for v in roots])).hexdigest() == g["ROOTS_sha256"]
    assert hashlib.sha256(struct.pack("<%dQ" % g["N"], *[int(v) for v in inv])).hexdigest() == g["INVROOTS_sha256"]


def test_fri_params_and_proof_size_agree_with_oracle():
    for d in (6, 12, 15, 16):
        a, b = api.fri_params(d), orc.fri_params(d)
        assert (a.n_rounds, list(a.arity_bits)) == (b.n_rounds, list(b.arity_bits))
        ncols = [85, 135, 20, 16]
        arr = (ctypes.c_size_t * 4)(*ncols)
        assert api.lib().vpbs_fri_proof_words(ctypes.byref(a), d, arr, 4) == orc.lib().orc_fri_proof_words(ctypes.byref(b), d, arr, 4)


def test_synth_inputs_are_canonical_and_seeded():
    a = synth.trace(0x5EED0000, 3, 6)
    b = synth.trace(0x5EED0000, 3, 6)
    assert (a == b).all() and a.shape == (3, 64) and int(a.max()) < P
    assert (synth.trace(0x5EED0001, 3, 6) != a).any()
    s = synth.step_inputs(5)
    assert {k: v.shape[0] for k, v in s.items()} == {"wires": 135, "zs_partial_products": 20, "quotient": 16, "constants_sigmas": 85}
    # scalar splitmix64 reference for the first element
    z = (0x5EED0000 + 0x9E3779B97F4A7C15) & (2**64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    z ^= z >> 31
    assert int(synth.splitmix64(0x5EED0000, 1)[0]) == z


def test_sharding_plan():
    # rate 8: 8 cosets; coset r fills leaf block brev3(r); 16 cap entries, 2 per coset
    for world in (1, 2, 4, 8):
        seen, caps = [], []
        for rank in range(world):
            seen += sharding.coset_assignment(3, rank, world)
            lo, hi = sharding.cap_slice(3, 4, rank, world)
            caps += list(range(lo, hi))
        assert sorted(seen) == list(range(8)) and caps == list(range(16))
    assert sharding.coset_assignment(3, 1, 2) == [1, 5, 3, 7]  # leaf blocks 4..7 <- cosets brev3(4..7)
    assert sharding.replica_assignment(10, 0, 4) == [0, 1, 2] and sharding.replica_assignment(10, 3, 4) == [8, 9]
    with pytest.raises(ValueError):
        sharding.coset_assignment(3, 0, 3)


def test_coset_sharded_commit_gloo_world2(tmp_path):
    """world_size-2 gloo run of the sharded-commit plan: each rank builds the Merkle subtrees of its cosets (oracle as
    the stand-in compute backend on CPU), one all_gather of cap hashes, result == single-process cap."""
    script = os.path.join(ROOT, "tests", "gloo_sharded_commit.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29531")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29531", script], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "SHARDED_COMMIT_OK" in r.stdout


def test_checked_allgather_reports_a_failing_rank_gloo_world2():
    """Failure semantics between ranks (include/vpbs_prover.h; the reference has none: it unwraps and dies, ivc_based_vpbs.rs:308): world-2 gloo
    run of vpbs_comm_allgather_checked -- the failing rank takes part with its status, both ranks return an error within the call, the
    communicator stays in step.  (The sharded step proof's own protocol needs the device: tests/gloo_sharded_failure_gpu.py.)"""
    script = os.path.join(ROOT, "tests", "gloo_comm_failure.py")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29537", script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "COMM_FAILURE_OK world=2" in r.stdout


def test_step_proof_byte_size_matches_paper_scale():
    """ProofWithPublicInputs::to_bytes size for the N=1024 step circuit from the restated layout:
    3 caps + 258 extension openings + FRI proof (3 caps, 28 query rounds, 8-coefficient final poly, nonce) + 4173 public
    inputs = ~180 kB, the scale the reference logs at ivc_based_vpbs.rs:488 ("proof ~200 kB" in
    the paper).  A weak but real consistency pin of the restated proof shape."""
    log_n, ncols, n_pi = 15, [85, 135, 20, 16], 4173
    p = api.fri_params(log_n)
    words = api.lib().vpbs_fri_proof_words(ctypes.byref(p), log_n, (ctypes.c_size_t * 4)(*ncols), 4)
    cap = 16 * 4
    openings = 2 * (sum(ncols) + 2)
    merkle_len_bytes = 28 * (4 + 3)                      # one u8 per Merkle proof
    total = 8 * (3 * cap + openings + words + 1 + n_pi) + merkle_len_bytes
    assert 150_000 < total < 200_000, total
    # closed form of the FRI part
    per_query = sum(ncols) + 4 * 4 * 14 + sum(32 + 4 * k for k in (10, 6, 2))
    assert words == 3 * cap + 28 * per_query + 2 * 8 + 1


def test_product_verifier_accepts_oracle_proofs_and_rejects_tampering():
    """vpbs_verify_step is host-only, so it runs here: it must agree with the oracle's verifier on oracle-made proofs."""
    import step_oracle
    log_n = 6
    cols = {"constants_sigmas": 9, "wires": 12, "zs_partial_products": 4, "quotient": 16}
    inputs = synth.step_inputs(log_n, cols=cols)
    inputs["quotient"] = None
    pis = synth.field_elements(5, 9)
    digest = np.array([9, 8, 7, 6], np.uint64)
    n_constants, n_routed = 1, 8
    sig = np.ascontiguousarray(inputs["constants_sigmas"][n_constants:n_constants + n_routed])
    # zs batch must have num_challenges * ceil(8/8) = 2 columns when computed from sigmas
    proof = step_oracle.prove_step(inputs, digest, pis, log_n, sigmas=sig, n_routed=n_routed, n_constants=n_constants)
    ncols = proof["ncols"]
    assert ncols == [9, 12, 2, 16]
    assert step_oracle.verify_step(proof, proof["cs_cap"], ncols, digest, pis, log_n)
    assert api.verify_step_fri_only(proof, proof["cs_cap"], ncols, digest, pis, log_n)
    # random sigmas are not a permutation of the wires: the FRI part verifies, the vanishing identity does not
    assert not api.verify_step(proof, proof["cs_cap"], ncols, digest, pis, log_n, check_permutation=True, n_constants=n_constants,
                               n_routed=n_routed)
    # every word of the FRI part (query leaves, Merkle siblings, fold evaluations, final polynomial, proof-of-work witness), a random sweep:
    # with the Merkle checks batched eight paths per AVX-512 register (where the CPU has it) and one after the other (VPBS_POSEIDON_X8=0)
    rnd = np.random.default_rng(17)
    sweep = [("fri", 0), ("fri", proof["fri"].size // 2), ("fri", proof["fri"].size - 1), ("openings", 3), ("caps", 5)] + \
            [("fri", int(q)) for q in rnd.integers(0, proof["fri"].size, 120)]
    for form in (True, False):
        api.host_set_poseidon_x8(form)
        try:
            assert api.verify_step_fri_only(proof, proof["cs_cap"], ncols, digest, pis, log_n)
            for key, pos in sweep:
                bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in proof.items()}
                flat = bad[key].reshape(-1)
                flat[pos] = (int(flat[pos]) + 1) % P
                assert not api.verify_step_fri_only(bad, proof["cs_cap"], ncols, digest, pis, log_n), (key, pos)
        finally:
            api.host_set_poseidon_x8(True)
    assert not api.verify_step_fri_only(proof, proof["cs_cap"], ncols, digest, pis[:-1], log_n)   # different public inputs
    # the default is the full check: without the circuit's shape it refuses instead of quietly running the FRI part alone
    with pytest.raises(ValueError):
        api.verify_step(proof, proof["cs_cap"], ncols, digest, pis, log_n)
    # FRI configurations whose caps are taller than a tree of the proof are rejected as malformed (they used to underflow the path lengths)
    for log_bad, cap_bad, rate_bad in ((3, 8, 3), (6, 8, 0), (4, 8, 3), (1, 5, 3)):
        with pytest.raises(api.VpbsError):
            api.verify_step_fri_only(proof, np.zeros((1 << cap_bad, 4), np.uint64), ncols, digest, pis, log_bad, rate_bits=rate_bad,
                                     cap_height=cap_bad)
        with pytest.raises(api.VpbsError):
            api.step_proof_from_bytes(b"\0" * 64, ncols, log_bad, 1, rate_bits=rate_bad, cap_height=cap_bad)


def test_fri_arities_follow_the_supplied_config():
    """ConstantArityBits(4, 5) depends on rate_bits and cap_height: reduce while degree_bits > 5 and degree_bits + rate_bits - 4 >= cap_height"""
    import oracle as orc
    for log_n in range(1, 18):
        p = api.fri_params(log_n)
        assert [p.arity_bits[i] for i in range(p.n_rounds)] == list(orc.fri_params(log_n).arity_bits)[:p.n_rounds]
        d, rounds = log_n, 0
        while d > 5 and d + 3 - 4 >= 4:
            d -= 4
            rounds += 1
        assert p.n_rounds == rounds
        assert fri_shapes.standard_arities(log_n) == [4] * rounds == api.standard_arity_bits(log_n)
    # ... and with the rate and cap height of the caller's configuration: the library (FriParams::standard inside make_proof_shape) agrees
    # with fri_shapes.standard_arities on every step shape -- it takes a serialised proof of exactly the oracle's length, whose layout
    # (step_oracle.to_bytes) has the rounds of standard_arities, and refuses one byte less
    for (log_n, rate, cap_h), rounds in fri_shapes.STEP_SHAPES:
        assert fri_shapes.standard_arities(log_n, rate, cap_h) == [4] * rounds == api.standard_arity_bits(log_n, rate, cap_h)
        p, pis, digest = _oracle_step_proof(log_n, rate, cap_h)
        blob = step_oracle.to_bytes(p, p["ncols"], N_CONSTANTS_STEP, pis, log_n, cap_height=cap_h, rate_bits=rate)
        back, back_pis = api.step_proof_from_bytes(blob, p["ncols"], log_n, N_CONSTANTS_STEP, rate_bits=rate, cap_height=cap_h)
        assert back["fri"].size == p["fri"].size and (back_pis == pis).all()
        with pytest.raises(api.VpbsError):
            api.step_proof_from_bytes(blob[:-1], p["ncols"], log_n, N_CONSTANTS_STEP, rate_bits=rate, cap_height=cap_h)
        if rounds != len(fri_shapes.standard_arities(log_n)):   # the standard configuration's rounds would give another length
            with pytest.raises(api.VpbsError):
                api.step_proof_from_bytes(blob, p["ncols"], log_n, N_CONSTANTS_STEP)


N_CONSTANTS_STEP = 2
_step_proofs = {}


def _oracle_step_proof(log_n, rate, cap_h):
    """the oracle's step proof of a step shape over synthetic columns (computed once per shape, never changed)"""
    key = (log_n, rate, cap_h)
    if key not in _step_proofs:
        inputs = synth.step_inputs(log_n, cols=fri_shapes.STEP_COLS)
        pis, digest = synth.field_elements(0xABCD, 11), np.array([11, 22, 33, 44], np.uint64)
        _step_proofs[key] = (step_oracle.prove_step(inputs, digest, pis, log_n, rate_bits=rate, cap_height=cap_h), pis, digest)
    return _step_proofs[key]


@pytest.mark.parametrize("shape", fri_shapes.FRI_SHAPES, ids=fri_shapes.shape_id)
def test_fri_proof_words_agree_with_the_oracle_at_every_shape(shape):
    log_n, rate, cap_h, bits = shape
    a = api.fri_params(log_n, rate_bits=rate, cap_height=cap_h, arity_bits=bits)
    b = orc.fri_params(log_n, rate_bits=rate, cap_height=cap_h, arity_bits=bits)
    assert bytes(a) == bytes(b)   # one struct layout, one meaning of arity_bits=[...]
    arr = (ctypes.c_size_t * 4)(*fri_shapes.FRI_COLS)
    words = api.lib().vpbs_fri_proof_words(ctypes.byref(a), log_n, arr, 4)
    assert words == orc.lib().orc_fri_proof_words(ctypes.byref(b), log_n, arr, 4) and words > 0
    # closed form: round caps | per query: leaves and paths of the four oracles, then per round the coset and its path | final polynomial | nonce
    per_q, lg, d = sum(fri_shapes.FRI_COLS) + 4 * 4 * (log_n + rate - cap_h), log_n + rate, log_n
    for ab in bits:
        lg, d = lg - ab, d - ab
        per_q += (2 << ab) + 4 * (lg - cap_h)
    assert words == len(bits) * (4 << cap_h) + a.num_query_rounds * per_q + (2 << d) + 1


def test_fri_proof_words_counts_and_query_rounds_agree_with_the_oracle():
    for cols in fri_shapes.POLY_COUNTS:
        a, b = api.fri_params(fri_shapes.POLY_COUNT_LOG_N), orc.fri_params(fri_shapes.POLY_COUNT_LOG_N)
        arr = (ctypes.c_size_t * 4)(*cols)
        assert api.lib().vpbs_fri_proof_words(ctypes.byref(a), 6, arr, 4) == orc.lib().orc_fri_proof_words(ctypes.byref(b), 6, arr, 4) > 0
    for nq in fri_shapes.QUERY_COUNTS:
        a, b = api.fri_params(6, pow_bits=2, num_query_rounds=nq), orc.fri_params(6, pow_bits=2, num_query_rounds=nq)
        arr = (ctypes.c_size_t * 4)(*fri_shapes.FRI_COLS)
        assert api.lib().vpbs_fri_proof_words(ctypes.byref(a), 6, arr, 4) == orc.lib().orc_fri_proof_words(ctypes.byref(b), 6, arr, 4) > 0


@pytest.mark.parametrize("name,log_n,over", fri_shapes.REFUSED_SHAPES, ids=[r[0].replace(" ", "_") for r in fri_shapes.REFUSED_SHAPES])
def test_fri_proof_words_is_zero_for_refused_parameters(name, log_n, over):
    """parameters that over-fold, outgrow a struct or put a cap above its tree have no word count (the unsigned arithmetic used to wrap into a
    garbage count, by which the caller sized the proof buffer)"""
    p = api.fri_params(log_n, **over)
    arr = (ctypes.c_size_t * 4)(*fri_shapes.FRI_COLS)
    assert api.lib().vpbs_fri_proof_words(ctypes.byref(p), log_n, arr, 4) == 0
    ok = api.fri_params(log_n)   # the nearest valid parameters still have one
    assert api.lib().vpbs_fri_proof_words(ctypes.byref(ok), log_n, arr, 4) > 0
    if name == "13 trees":       # the count is of trees, not of rounds: the same nine rounds next to three oracles are fine
        assert api.lib().vpbs_fri_proof_words(ctypes.byref(p), log_n, arr, 3) > 0
    assert api.lib().vpbs_fri_proof_words(None, log_n, arr, 4) == 0


@pytest.mark.parametrize("shape,rounds", fri_shapes.STEP_SHAPES, ids=lambda v: "n%d-r%d-c%d" % v if isinstance(v, tuple) else None)
def test_host_verifier_on_oracle_step_proofs_at_every_step_shape(shape, rounds):
    """vpbs_step_proof_from_bytes and vpbs_verify_step (host only) at every (log_n, rate_bits, cap_height): the oracle's proof parses back to
    the same words and is accepted; five tampered words are rejected"""
    log_n, rate, cap_h = shape
    p, pis, digest = _oracle_step_proof(log_n, rate, cap_h)
    ncols = p["ncols"]
    blob = step_oracle.to_bytes(p, ncols, N_CONSTANTS_STEP, pis, log_n, cap_height=cap_h, rate_bits=rate)
    back, back_pis = api.step_proof_from_bytes(blob, ncols, log_n, N_CONSTANTS_STEP, rate_bits=rate, cap_height=cap_h)
    for key in ("caps", "openings", "fri"):
        assert (back[key].reshape(-1) == np.asarray(p[key], np.uint64).reshape(-1)).all(), key
    assert (back_pis == pis).all()
    assert api.verify_step_fri_only(back, p["cs_cap"], ncols, digest, back_pis, log_n, rate_bits=rate, cap_height=cap_h)
    n_fri = p["fri"].size
    for key, pos in (("caps", 5), ("openings", 3), ("fri", 0), ("fri", n_fri // 2), ("fri", n_fri - 2)):
        bad = {k: back[k].copy() for k in ("caps", "openings", "fri")}
        flat = bad[key].reshape(-1)
        flat[pos] = (int(flat[pos]) + 1) % P
        assert not api.verify_step_fri_only(bad, p["cs_cap"], ncols, digest, back_pis, log_n, rate_bits=rate, cap_height=cap_h), (key, pos)


def test_hash_chain_matches_oracle_and_reference_semantics():
    """verify_hash_output (/root/reference/src/vtfhe/ivc_based_vpbs.rs:64-78): h <- hash_no_pad(h || item) from h = 0."""
    rng = np.random.default_rng(3)
    for n_items, item_len in [(1, 1), (3, 5), (4, 12), (2, 100), (5, 4)]:
        items = rng.integers(0, P, size=(n_items, item_len), dtype=np.uint64)
        want = np.zeros(4, np.uint64)
        orc.lib().orc_hash_chain(orc.ptr(np.ascontiguousarray(items)), n_items, item_len, orc.ptr(want))
        h = np.zeros(4, np.uint64)
        for k in range(n_items):   # the reference's loop, with the product's own hash_no_pad
            h = api.hash_no_pad(np.concatenate([h, items[k]]))
        got, ok = api.hash_chain(items, claimed=want)
        assert ok and (got == want).all() and (h == want).all()
        bad = want.copy(); bad[0] ^= np.uint64(1)
        assert not api.hash_chain(items, claimed=bad)[1]


def test_hash_chains_of_concurrent_callers_share_lanes_and_agree_with_the_oracle():
    """Nine threads walk nine different chains at once, eight links per call (vpbs_hash_chain_links; items of 200, 64 and 65 elements: long
    enough to share the lanes of the eight-lane host Poseidon where the CPU has AVX-512 and the process counts as short of CPUs; one chain
    of short items never shares, one has a different number of links): every chain ends in the oracle's value and every link equals
    hash_no_pad of the concatenation, whoever happened to run whose batch."""
    import threading
    rng = np.random.default_rng(11)
    shapes = [(16, 200)] * 5 + [(16, 64), (16, 65), (12, 200), (20, 5)]
    chains = [rng.integers(0, P, size=sh, dtype=np.uint64) for sh in shapes]
    want = []
    for items in chains:
        w = np.zeros(4, np.uint64)
        orc.lib().orc_hash_chain(orc.ptr(np.ascontiguousarray(items)), items.shape[0], items.shape[1], orc.ptr(w))
        want.append(w)
    for attempt in range(4):
        api.lib().vpbs_host_set_blocking_sync(1 if attempt < 3 else 0)   # sharing is for processes short of CPUs; the last pass: every caller alone
        got = [None] * len(chains)
        start = threading.Barrier(len(chains))

        def walk(i):
            start.wait()
            seg = 8 if chains[i].shape[0] % 8 == 0 else 4
            h, links = np.zeros(4, np.uint64), []
            for k in range(0, chains[i].shape[0], seg):
                out = api.hash_chain_links(h, chains[i][k:k + seg])
                links.append(out)
                h = out[-1].copy()
            got[i] = np.concatenate(links)
        threads = [threading.Thread(target=walk, args=(i,)) for i in range(len(chains))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for g, w, items in zip(got, want, chains):
            assert (g[-1] == w).all()
            assert (g[3] == api.hash_no_pad(np.concatenate([g[2], items[3]]))).all()
    api.lib().vpbs_host_set_blocking_sync(-1)
    assert (api.hash_chain(chains[0])[0] == want[0]).all()


def test_recorded_bench_line_keeps_the_contract():
    """profiles/r06_bench_detail_n1.json is the full result `python bench.py` wrote on the GPU box (since round 6 the DETAIL file; stdout carries the
    compact record built from it, test_bench_line_is_a_compact_record): the keys the judge reads.  The
    headline is the IVC chain (chained step proofs through vpbs_ivc_prove_pbs); since round 4 the roofline object has the contract's form
    (bound hbm: algorithmic bytes per launch / launch duration / 8 TB/s, the PMC traffic and its source named) with the integer-issue pricing
    beside it, the whole step priced against HBM, and a sustained figure (whole chains) next to the burst."""
    import json
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r06_bench_detail_n1.json")
    d = json.load(open(path))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None and d["scaling"] == "weak"
    assert "workload" in d["config"] and "model" not in d["config"] and "vpbs_ivc_prove_pbs" in d["config"]["workload"]
    chains = d["config"]["chains_per_gpu"]
    assert chains >= 1 and abs(d["value"] - chains * 1e3 / d["ms_per_step"] / 730) / d["value"] < 1e-6      # chained proofs/s / 730
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0 < r["frac"] < 0.1
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["launch_ms_avg"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    assert 0.95 < r["traffic"] / r["algorithmic_bytes_per_launch"] < 1.05 and "profiles/" in r["traffic_measured_in"] and "single_chain" in r["measured_in"]
    i = r["int_valu_issue"]
    assert i["bound"] == "int-valu-issue" and abs(i["frac"] - i["achieved"] / i["peak"]) < 1e-9 and 0 < i["frac"] <= 1.0
    assert 0.01 < r["step_hbm_frac"] < 0.2
    # round 5: the WHOLE step against the bound that holds it (wave-level VALU instructions per step by kernel / issue rate / measured time), and
    # what ran: ranks counted by the communication library, who started them, CPUs per rank, the pipeline chosen
    b = r["valu_budget"]
    assert abs(sum(b["by_kernel_G"].values()) - b["wave_instructions_per_step_G"]) < 1e-6 and "r06_pmc_sq_kernels_shared_gpu.csv" in b["counters_from"]   # several chains per GPU: the counter pass with THEIR settings
    assert "r06_pmc_sq_kernels.csv" in r["valu_budget_single_chain"]["counters_from"]
    assert b["wave_instructions_per_step_G"] < r["valu_budget_single_chain"]["wave_instructions_per_step_G"]
    assert abs(b["frac"] - b["instruction_time_ms_per_step"] / b["measured_ms_per_step_proof"]) < 1e-9 and 0.8 < b["frac"] < 1.05
    assert abs(b["measured_ms_per_step_proof"] - d["ms_per_step"] / chains) < 1e-6
    assert d["rccl"]["ranks"] == d["n_gpus"] and d["cpus_per_rank"] >= 1 and d["pipeline"]["chains_per_gpu"] == chains and d["launched_by"]
    s = d["sustained"]
    assert s["chains"] == chains and abs(s["sustained_over_burst"] - s["vpbs_proofs_per_s"] / d["value"]) < 1e-9 and 0.9 < s["sustained_over_burst"] < 1.1
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["sample"] and c["runs"] >= 5
    assert len(c["ms_per_step_runs"]) == c["runs"] and sum(c["stages_ms_median"].values()) < 1.05 * c["ms_per_step"]
    assert "cargo" in c["reference_probe"]
    assert d["parity_checked_full_size"] is True and d["step_micro"]["ms_per_step_proof"] > 0 and d["ivc_single_chain"]["ms_per_step"] > d["ms_per_step"] / chains
    assert d["ivc_chain_n2048"]["ms_per_step"] > d["ivc_single_chain"]["ms_per_step"] and d["ivc_chain"]["decrypted"] == d["ivc_chain"]["message"]


def _recorded_details():
    """full results of bench.py runs on the GPU box (bench_detail.json), kept under profiles/: one GPU, two ranks on one device, the sharded mode"""
    import glob
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [os.path.join(root, "profiles", "r05_bench_latest.json")] + sorted(glob.glob(os.path.join(root, "profiles", "r06_bench_detail*.json")))
    return [(os.path.basename(p), json.load(open(p))) for p in paths]


def test_bench_line_is_a_compact_record():
    """the line bench.py prints is a record the driver parses -- under 4 kB, finite numbers and short identifiers, the contract
    keys, BASELINE.json's metric verbatim -- built by tools/bench_record.py from the full result, which goes to bench_detail.json.  Checked on every
    recorded detail (N = 1; two ranks on one device; --mode sharded) and on a worst case: every string of the detail blown up to a paragraph."""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import bench_record
    metric = json.load(open(os.path.join(root, "BASELINE.json")))["metric"]
    details = _recorded_details()
    assert details

    def blow_up(x):
        if isinstance(x, dict):
            return {k: blow_up(v) for k, v in x.items()}
        if isinstance(x, list):
            return [blow_up(v) for v in x]
        if isinstance(x, str):
            return x + " " + "and a long explanation of why, " * 40
        return x

    for name, d in details + [("blown up " + n, blow_up(x)) for n, x in details]:
        line = bench_record.dumps(bench_record.compact_record(d))
        assert len(line) < 4096 and "\n" not in line and line.startswith('{"metric"'), name
        r = json.loads(line)
        assert r["metric"] == metric and r["higher_is_better"] is True and r["vs_baseline"] is None
        assert r["dtype"] == "u64" and r["data"] == "synthetic" and r["scaling"][:4] in ("weak", "stro")
        assert r["n_gpus"] == d["n_gpus"] and r["steps"] == d["steps"] and r["warmup"] == d["warmup"]
        assert abs(r["value"] - d["value"]) <= 1e-5 * d["value"] and abs(r["ms_per_step"] - d["ms_per_step"]) <= 1e-5 * d["ms_per_step"]
        c = r["config"]
        assert 0 < len(c["workload"]) <= 200 and "model" not in c and c["chains_per_gpu"] >= 1
        if not name.startswith("blown up"):
            assert r["unit"] == "vPBS proofs/s" and c["parallelism"] in ("replicas", "coset-sharded") and r["scaling"] in ("weak", "strong")
        f = r["roofline"]
        assert f["bound"][:3] == "hbm" and f["unit"][:4] == "GB/s" and f["peak"] == 8000.0 and f["kernel"] == "leaf_hash_kernel"
        assert abs(f["frac"] - f["achieved"] / f["peak"]) < 1e-6 and 0 < f["frac"] < 0.1
        assert abs(f["achieved"] - f["algorithmic_bytes_per_launch"] / (f["launch_ms_avg"] * 1e-3) / 1e9) < 1e-4 * f["achieved"]
        assert f["traffic"] is None or 0.9 < f["traffic"] / f["algorithmic_bytes_per_launch"] < 1.1
        if "cpu_baseline" in d:
            b = r["cpu_baseline"]
            assert b["cores"] >= 1 and b["value"] > 0 and b["runs"] >= 1 and 0 < len(b["sample"]) <= 120
        assert r["rccl"]["ranks"] == r["n_gpus"]
    # NaN / Infinity never reach the line; an oversized one is refused, not printed
    d = dict(details[0][1], value=float("nan"))
    assert json.loads(bench_record.dumps(bench_record.compact_record(d)))["value"] is None
    with pytest.raises(ValueError):
        bench_record.dumps(dict(bench_record.compact_record(details[0][1]), junk="x" * 5000))


def test_counter_files_belong_to_the_kernels_as_they_stand():
    """`roofline.traffic` and `valu_budget.by_kernel_G` are constants read from profiles/ (counter passes are their own
    rocprofv3 runs).  The newest counter set carries the fingerprint of the device sources it was measured on (tools/refresh_profiles.sh ->
    profiles/rNN_pmc_sources.json); any edit of a kernel source after that fails here until the counters are taken again."""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import kernel_sources
    src = kernel_sources.newest_profile("pmc_sources.json")
    assert src, "no profiles/rNN_pmc_sources.json: run tools/refresh_profiles.sh on the GPU box and tools/condense_profiles.py here"
    tag = os.path.basename(src)[:3]
    for suffix in ("pmc_sq_kernels.csv", "pmc_sq_kernels_shared_gpu.csv", "pmc_leaf_hash.json"):     # what bench.py will read: the same round's
        assert os.path.basename(kernel_sources.newest_profile(suffix)).startswith(tag), suffix
    was, now = json.load(open(src)), kernel_sources.fingerprint()
    changed = sorted(k for k in now["files"] if was["files"].get(k) != now["files"][k])
    assert not changed, "device sources changed since the counters of %s were measured: %s -- refresh them (tools/refresh_profiles.sh)" % (tag, changed)


def _kernel_resources(src, tmp_path):
    """hipcc -Rpass-analysis=kernel-resource-usage over one source of csrc/ (device code only, gfx950): {kernel name: {remark key: int}} and the
    path of the ISA listing"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "verifiable-fhe-paper_amd", "csrc")
    out = str(tmp_path / (src + ".s"))
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-pass-failed", "-Rpass-analysis=kernel-resource-usage",
                        "-S", "--cuda-device-only", os.path.join(csrc, src), "-o", out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: [^:]*:\d+:\d+:\s+(.*?)\s*\[-Rpass-analysis", line) or re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1)
        if text.startswith("Function Name:"):
            cur = kernels.setdefault(text.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in text:
            k, v = text.rsplit(":", 1)
            try:
                cur[k.strip()] = int(v)
            except ValueError:
                pass
    return kernels, out


def test_hash_and_gate_kernels_do_not_spill(tmp_path):
    """leaf_hash_kernel had 66 SGPR spills -- ~140 v_readlane / v_writelane per permutation in its sponge loop (the
    compiler split all 24 constants of a partial-round group on the scalar unit ahead of the S-boxes and parked the halves in VGPR lanes; the first
    round's and round 25's constants, loop-invariant, were loaded once and read back from lanes by every permutation) -- and gate_tile_kernel<2>
    spilled six VGPRs to scratch.  Now: no VGPR spill and no scratch in any of the hot kernels; what is left of the scalar spills in the sponge
    kernels are kernel arguments touched once per absorb (counted in the ISA of the loop: at most 16 lane moves per permutation of ~13.3 k
    instructions); the gate tile kernel dispatches its work units on scalar registers (s_cbranch, not exec masks)."""
    kernels, asm = _kernel_resources("hash.hip", tmp_path)

    def find(part):
        hits = [v for k, v in kernels.items() if part in k]
        assert len(hits) == 1, (part, list(kernels))
        return hits[0]
    for part, limit in (("16leaf_hash_kernelILb0EE", 16), ("20fri_leaf_hash_kernelE", 16), ("19merkle_level_kernelE", 8), ("16hash_rows_kernelE", 8)):
        k = find(part)
        assert k["VGPRs Spill"] == 0 and k["ScratchSize [bytes/lane]"] == 0 and k["SGPRs Spill"] <= limit, (part, k)
        assert k["Occupancy [waves/SIMD]"] >= 4, (part, k)
    # the sponge loop of the launched leaf kernel: lane moves between the loop header and its back edge
    text = open(asm).read()
    body = text[text.index("leaf_hash_kernelILb0EE"):]
    body = body[:body.index("s_endpgm")]
    lines = body.splitlines()
    header = next(i for i, l in enumerate(lines) if "=>This Loop Header: Depth=1" in l)
    label = lines[header].split(":")[0].strip().lstrip(".L")        # blocks of the loop carry "Header=BBn_m" / "Parent Loop BBn_m" remarks
    last = max(i for i, l in enumerate(lines) if ("Header=" + label) in l or ("Parent Loop " + label) in l)
    end = next((i for i in range(last + 1, len(lines)) if re.match(r"\.LBB\d+_\d+:", lines[i])), len(lines))
    loop = lines[header:end]
    is_move = lambda l: "v_readlane_b32" in l or "v_writelane_b32" in l
    lane_moves = sum(1 for l in loop if is_move(l))
    valu = sum(1 for l in loop if re.match(r"\s+v_", l))
    # the round loops inside (full rounds x 4, partial groups x 7, full rounds x 4: the blocks remarked "Inner Loop Header: Depth=2", each up to
    # the next label) run several times per permutation: not one lane move in them
    inner = 0
    for i, l in enumerate(loop):
        m = re.match(r"(\.LBB\d+_\d+):", l)
        if m and i + 1 < len(loop) and "Inner Loop Header: Depth=2" in loop[i + 1]:
            j = max(k for k in range(i, len(loop)) if re.search(r"s_cbranch_\w+\s+" + re.escape(m.group(1)) + r"\s*$", loop[k]))   # its back edge
            inner += sum(1 for x in loop[i:j] if is_move(x))
    assert valu > 3000 and lane_moves <= 16 and inner == 0, (lane_moves, inner, valu)
    kernels, asm = _kernel_resources("gates.hip", tmp_path)
    k = [v for name, v in kernels.items() if "gate_tile_kernelILi2EE" in name][0]
    assert k["VGPRs Spill"] == 0 and k["ScratchSize [bytes/lane]"] == 0 and k["Occupancy [waves/SIMD]"] >= 4, k
    text = open(asm).read()
    body = text[text.index("gate_tile_kernelILi2EE"):]
    body = body[:body.index("s_endpgm")]
    assert "s_cbranch_scc" in body and len(re.findall(r"v_cmp_eq_u32_e32 vcc, \d+, v\d+\n\s+s_and_saveexec", body)) == 0


def test_pmc_table_counts_one_step_proof_exactly(tmp_path):
    """tools/pmc_table.py: `valu_per_step_proof` = SQ_INSTS_VALU of the dispatches between the first and the last quotient_perm_kernel dispatch /
    the periods between them -- the setup commitment's launches (before the first step) and the tail are not in it, whatever their size"""
    import csv
    import subprocess
    d = tmp_path / "pmc" / "runc"
    d.mkdir(parents=True)
    rows, disp = [], [0]

    def launch(kernel, valu):
        disp[0] += 1
        for name, v in (("SQ_INSTS_VALU", valu), ("SQ_WAVES", 10)):
            rows.append({"Dispatch_Id": disp[0], "Kernel_Name": "vpbs::(anonymous namespace)::%s(unsigned long*)" % kernel, "Counter_Name": name,
                         "Counter_Value": v})

    launch("leaf_hash_kernel", 999)          # setup: a commitment of another shape
    launch("merkle_level_kernel", 77)
    for step in range(4):                     # four identical step proofs
        for k in range(3):
            launch("leaf_hash_kernel", 100 + k)
        launch("merkle_level_kernel", 10)
        launch("quotient_perm_kernel", 7)
        launch("gate_tile_kernel", 50)
    with open(d / "1_counter_collection.csv", "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pmc_table.py"), str(tmp_path / "pmc")], capture_output=True, text=True, check=True)
    table = {r["kernel"]: r for r in csv.DictReader(out.stdout.splitlines())}
    assert float(table["leaf_hash_kernel"]["valu_per_step_proof"]) == 100 + 101 + 102      # not (999 + 4 * 303) / (13 / 3)
    assert float(table["merkle_level_kernel"]["valu_per_step_proof"]) == 10
    assert float(table["gate_tile_kernel"]["valu_per_step_proof"]) == 50 and float(table["quotient_perm_kernel"]["valu_per_step_proof"]) == 7
    assert int(table["leaf_hash_kernel"]["launches"]) == 13 and float(table["leaf_hash_kernel"]["SQ_INSTS_VALU"]) == 999 + 4 * 303


def test_bench_parent_starts_the_ranks_without_touching_the_gpu(tmp_path):
    """`python bench.py --gpus N` outside a launcher is the PARENT of its ranks: it must import nothing that could open
    the device -- neither torch nor the prover library -- start `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a CHILD
    process (never an exec) and relay one JSON line and the exit code.  Checked with stand-ins for `torch` and `vpbs_amd` at the head of
    PYTHONPATH that record which process imported them: only the child may."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    log = tmp_path / "imports.log"
    (tmp_path / "torch" / "distributed").mkdir(parents=True)
    stamp = "import os\nopen(%r, 'a').write('%%s %%d %%d\\n' %% (__name__, os.getpid(), os.getppid()))\n" % str(log)
    (tmp_path / "torch" / "__init__.py").write_text(stamp)
    (tmp_path / "torch" / "distributed" / "__init__.py").write_text("")
    (tmp_path / "vpbs_amd.py").write_text(stamp)
    (tmp_path / "torch" / "distributed" / "run.py").write_text(
        "import json, os, sys\n"
        "print('rank chatter that is not the line')\n"
        "print(json.dumps({'metric': 'm', 'argv': sys.argv[1:], 'self': os.environ.get('VPBS_BENCH_SELF_LAUNCHED'), 'pid': os.getpid(),\n"
        "                  'ipc': os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')}))\n"
        "sys.exit(int(os.environ.get('FAKE_RC', '0')))\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    env["PYTHONPATH"] = str(tmp_path)
    p = subprocess.Popen([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--device", "0", "--steps", "3"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, env=env)
    out, err = p.communicate(timeout=120)
    assert p.returncode == 0, err[-2000:]
    lines = out.strip().splitlines()
    assert len(lines) == 1 and "rank chatter" in err
    d = json.loads(lines[0])
    a = d["argv"]
    assert a[a.index("--nproc-per-node") + 1] == "4" and a[a.index("--master-addr") + 1] == "127.0.0.1" and "--nnodes=1" in a
    assert a[-6:] == ["--gpus", "4", "--device", "0", "--steps", "3"] and a[-7] == os.path.join(root, "bench.py")
    assert d["self"] == "1" and d["ipc"] == "0" and d["pid"] != p.pid
    seen = [ln.split() for ln in log.read_text().splitlines()]
    assert seen and all(int(pid) != p.pid for _, pid, _ in seen)          # the parent imported neither stand-in
    assert all(int(ppid) == p.pid for _, _, ppid in seen)                   # ... its child did (a child process, not an exec)
    # the launcher's exit code is the parent's
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--device", "0"], capture_output=True, text=True,
                       env=dict(env, FAKE_RC="7"), timeout=120)
    assert r.returncode == 7
    # fewer devices visible than ranks asked for and no --device: refused before anything starts (fake KFD topology: one GPU node, one CPU node)
    top = tmp_path / "kfd"
    for i, simd in enumerate((0, 256)):
        (top / str(i)).mkdir(parents=True)
        (top / str(i) / "properties").write_text("cpu_cores_count %d\nsimd_count %d\n" % (16 if simd == 0 else 0, simd))
    sys.path.insert(0, root)
    try:
        import importlib
        spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(root, "bench.py"))
        bench = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bench)
    finally:
        sys.path.remove(root)
    saved = {k: os.environ.pop(k, None) for k in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES")}
    try:
        assert bench.visible_gpus(str(top)) == 1 and bench.visible_gpus(str(tmp_path / "absent")) is None
        os.environ["HIP_VISIBLE_DEVICES"] = ""                  # this container's own setting: no device
        assert bench.visible_gpus(str(top)) == 0
        os.environ["HIP_VISIBLE_DEVICES"] = "0,1"               # a mask cannot add devices
        assert bench.visible_gpus(str(top)) == 1
    finally:
        os.environ.pop("HIP_VISIBLE_DEVICES", None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    # under a launcher (RANK / WORLD_SIZE present) or at N = 1 the process is a rank, not a parent
    assert bench.launch_ranks(["--gpus", "1"]) is None
    os.environ["WORLD_SIZE"] = "2"
    try:
        assert bench.launch_ranks(["--gpus", "2"]) is None
    finally:
        del os.environ["WORLD_SIZE"]


def test_proof_bytes_round_trip_and_verify():
    """data format behind the path: an (oracle) step proof serialised with the restated ProofWithPublicInputs::to_bytes layout is parsed
    back by the product (vpbs_step_proof_from_bytes) into the very arrays it came from, public inputs included, and the parsed proof
    is accepted by vpbs_verify_step; truncated / padded / foreign-shape / non-canonical byte strings are rejected."""
    import regression_cases as rc
    import step_oracle
    case = next(c for c in rc.cases() if rc.build(c)["gates"] is None)
    b = rc.build(case)
    p = step_oracle.prove_step(b["inputs"], rc.DIGEST, b["pis"], b["log_n"])
    ncols, n_constants = p["ncols"], 3
    blob = step_oracle.to_bytes(p, ncols, n_constants, b["pis"], b["log_n"])
    proof, pis = api.step_proof_from_bytes(blob, ncols, b["log_n"], n_constants)
    for key in ("caps", "openings", "fri"):
        assert (proof[key].reshape(-1) == np.asarray(p[key], np.uint64).reshape(-1)).all(), key
    assert (pis == np.asarray(b["pis"], np.uint64)).all()
    assert api.verify_step_fri_only(proof, p["cs_cap"], ncols, rc.DIGEST, pis, b["log_n"])
    for bad in (blob[:-8], blob + b"\\0" * 8, blob[:len(blob) // 2]):
        with pytest.raises(api.VpbsError):
            api.step_proof_from_bytes(bad, ncols, b["log_n"], n_constants)
    with pytest.raises(api.VpbsError):
        api.step_proof_from_bytes(blob, [ncols[0], ncols[1] + 1, ncols[2], ncols[3]], b["log_n"], n_constants)
    with pytest.raises(api.VpbsError):
        api.step_proof_from_bytes(blob, ncols, b["log_n"] + 1, n_constants)
    tampered = bytearray(blob)
    tampered[8:16] = (0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")          # a cap element >= p
    with pytest.raises(api.VpbsError):
        api.step_proof_from_bytes(bytes(tampered), ncols, b["log_n"], n_constants)


def test_seeded_lwe_encrypt_and_testv_match_the_oracle():
    """the host-only members of the seeded generator (vpbs_lwe_encrypt, vpbs_testv) against tests/tfhe_oracle.py; the noise stand-in has
    the requested standard deviation"""
    import tfhe_oracle as T
    seed, n = 0xC0FFEE, 40
    ring = T.Ring(6)
    s_to, s_lwe, s_glwe = T.seeded_keys(ring, seed, n, 3)
    assert set(s_lwe) <= {0, 1} and 8 < sum(s_lwe) < 32 and all(v == 0 for poly in s_to[1:] for v in poly) and s_to[0][n:] == [0] * (64 - n)
    prm = api.KeygenParamsC(6, 3, 3, 7, n, seed, 1e-8, 1.17021618159313e-5)
    for p, nonce in ((2, 0), (4, 9)):
        t, delta = api.testv(64, p)
        assert delta == T.get_delta(2 * p) and (t == np.array(T.get_testv(ring, p, delta), np.uint64)).all()
        ct = api.lwe_encrypt(prm, s_lwe, delta % P, nonce)
        assert (ct == np.array(T.seeded_lwe_encrypt(seed, s_lwe, delta % P, 1.17021618159313e-5, nonce), np.uint64)).all()
    g = T.Seeded(seed)
    m_sigma = T.sigma_to_int(4.99027217501041e-8)
    xs = [g.noise(g.stream(T.BSK_NOISE, 1, 2), i, m_sigma) for i in range(4000)]
    xs = [x - P if x > P // 2 else x for x in xs]
    mean, std = sum(xs) / len(xs), (sum(x * x for x in xs) / len(xs)) ** 0.5
    assert abs(mean) < 0.1 * m_sigma and 0.9 * m_sigma < std < 1.1 * m_sigma and max(abs(x) for x in xs) <= 6 * m_sigma


def test_prover_tools_load_the_circuit_as_data():
    """Layering: the product package imports nothing from tests/, circuitgen/ or oracle/; bench.py and the prover tools get their circuits
    from exported files through the product package and never import the circuit builder (circuitgen/); bench.py touches tests/ (the
    checker) only inside its cpu_baseline leg; only the exporter tools import circuitgen/"""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in glob.glob(os.path.join(root, "verifiable-fhe-paper_amd", "*.py")):
        src = open(path).read()
        for word in ('"tests"', '"circuitgen"', '"oracle"', "import step_circuit", "import cyclic_circuit", "import pymodel", "import oracle",
                     "export_circuits.ensure", "import export_"):   # the package neither imports nor RUNS a circuit builder
            assert word not in src, (path, word)
        if path.endswith("circuit_file.py"):
            assert "subprocess" not in src and "os.system" not in src, path   # (api.py's only child process is `make` of the library itself)
    for tool in ("prove_pbs.py", "prove_ivc.py"):
        src = open(os.path.join(root, "tools", tool)).read()
        assert "import step_circuit" not in src and "import cyclic_circuit" not in src and '"tests"' not in src and '"circuitgen"' not in src, tool
        assert "export_circuits" not in src and "export_step_circuit" not in src and "ensure_" not in src, tool   # they locate circuit files (find_*)
    from vpbs_amd import circuit_file
    with pytest.raises(FileNotFoundError, match="tools/export_circuits.py --cyclic 16 2 4 5 3 13"):
        circuit_file.find_cyclic_circuit(16, 2, 4, 5, 3, 13)   # a parameter set nobody exported: located, not built
    bench = open(os.path.join(root, "bench.py")).read()
    # the harness may RUN the build step (tools/export_circuits.py, a process of its own) for a checkout that was never built; it imports no builder
    assert "import step_circuit" not in bench and "import cyclic_circuit" not in bench and "import export_circuits" not in bench
    assert bench.count('os.path.join(ROOT, "tests")') == 1 and bench.index("def cpu_baseline") < bench.index('os.path.join(ROOT, "tests")')
    exporters = {os.path.basename(p) for p in glob.glob(os.path.join(root, "tools", "*.py")) if '"circuitgen"' in open(p).read() or "'circuitgen'" in open(p).read()}
    assert {"export_step_circuit.py", "step_circuit_sizes.py"} <= exporters
    assert not {"prove_pbs.py", "prove_ivc.py", "soak.py", "verify_speed.py"} & exporters


def test_circuit_file_round_trip(tmp_path):
    """exporter -> file -> circuit_file.load: the loaded description generates the sample witness and its public inputs"""
    import subprocess
    import sys
    from vpbs_amd import circuit_file
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "step8.bin")
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "export_step_circuit.py"), path, "8", "2", "4", "5", "6"], stdout=subprocess.DEVNULL)
    d = circuit_file.load(path)
    assert d.meta == {"N": 8, "K": 2, "ELL": 4, "LOGB": 5, "n_lwe": 6, "used_rows": d.used_rows} and d.n == 1 << d.log_n
    plan = d.circuit.witness_plan(d.preset_pos)
    w = plan.run(d.sample_values)
    assert (np.array([w[c][r] for c, r in d.pi_pos], np.uint64) == d.sample_public_inputs).all()
    ok, msg = d.circuit.check_witness(w, api.hash_no_pad(d.sample_public_inputs))
    assert ok, msg
    plan.free()


def test_host_poseidon_batches_match_the_oracle():
    """vpbs_k_poseidon_host: n independent permutations on the host -- eight per AVX-512 register where the CPU has it (csrc/host/poseidon_x8.h),
    one by one otherwise -- against the oracle's permutation, edge values and a ragged tail (n not a multiple of eight) included"""
    rng = np.random.default_rng(11)
    for n in (0, 1, 7, 8, 9, 203):
        st = rng.integers(0, P, size=(n, 12), dtype=np.uint64)
        if n > 2:
            st[0], st[1], st[2] = 0, P - 1, np.arange(12)
        got = st.copy()
        rc = api.lib().vpbs_k_poseidon_host(api._ptr(got) if n else None, n)
        assert rc in (0, 1)
        assert all((got[i] == orc.poseidon(st[i])).all() for i in range(n))


COMPAT_POSITIONS = [dict(fri_mul_final_by_x=m, bytes_pi_len_prefix=b, digest_domain_separator=d) for m in (0, 1) for b in (0, 1) for d in (0, 1)]


def test_compat_defaults_and_digest_agree_with_the_oracle():
    """the switch table of include/vpbs_prover.h and its copy in oracle/vpbs_oracle.h: same fields, same defaults; hash_pad and the circuit
    digest of CircuitBuilder::build agree in both formulas, and with a third restatement in plain Python (circuitgen/cyclic_circuit.py)"""
    import cyclic_circuit as cc
    assert api.compat_dict() == orc.compat_dict() == dict(fri_mul_final_by_x=0, bytes_pi_len_prefix=1, digest_domain_separator=1, pow_smallest_nonce=1)
    for words in ([], [5], list(range(1, 7)), list(range(1, 8)), list(range(1, 9)), list(range(3, 23))):
        assert api.hash_pad(words).tolist() == orc.hash_pad(words).tolist() == [int(x) for x in cc.hash_pad(words)]
    # pad10*1: the empty message is the block 1, 0, 0, 0, 0, 0, 0, 1
    assert api.hash_pad([]).tolist() == api.hash_no_pad([1, 0, 0, 0, 0, 0, 0, 1]).tolist()
    cap = synth.field_elements(31, 64).reshape(16, 4)
    sep = api.hash_pad([])
    for ds in (0, 1):
        want = api.hash_no_pad(np.concatenate([cap.reshape(-1), sep if ds else sep[:0], np.array([13], np.uint64)]))
        assert api.circuit_digest(cap, 13, api.compat(digest_domain_separator=ds)).tolist() == want.tolist()
        assert orc.circuit_digest(cap, 13, orc.compat(digest_domain_separator=ds)).tolist() == want.tolist()
        assert cc.circuit_digest(cap, 13, bool(ds)).tolist() == want.tolist()
    assert api.circuit_digest(cap, 13).tolist() == api.circuit_digest(cap, 13, api.compat()).tolist()   # NULL = the defaults
    with pytest.raises(ValueError):
        api.compat(no_such_switch=1)


@pytest.mark.parametrize("pos", COMPAT_POSITIONS, ids=lambda p: "x%d_pi%d_ds%d" % tuple(p.values()))
def test_every_compat_position_oracle_prover_vs_product_verifier(pos):
    """Every position of the switch table, oracle prover against the product's host-side parser and verifier (the device prover against the
    oracle under every position: test_gpu_parity.py::test_every_compat_position_bit_exact): bytes made under a position parse and verify under
    the same position, and each switch that changes the proof is noticed when the two sides disagree."""
    import step_oracle
    log_n = 6
    cols = {"constants_sigmas": 9, "wires": 12, "zs_partial_products": 4, "quotient": 16}
    inputs = synth.step_inputs(log_n, cols=cols)
    pis = synth.field_elements(5, 9)
    ko, kp = orc.compat(**pos), api.compat(**pos)
    cs = orc.Batch(inputs["constants_sigmas"], 3, 4, True)
    digest = orc.circuit_digest(cs.cap(), log_n, ko)
    assert digest.tolist() == api.circuit_digest(cs.cap(), log_n, kp).tolist()
    proof = step_oracle.prove_step(inputs, digest, pis, log_n, cs_batch=cs, compat=ko)
    ncols = proof["ncols"]
    assert step_oracle.verify_step(proof, proof["cs_cap"], ncols, digest, pis, log_n, compat=ko)
    blob = step_oracle.to_bytes(proof, ncols, 1, pis, log_n, compat=ko)
    back, back_pis = api.step_proof_from_bytes(blob, ncols, log_n, 1, compat=kp)
    assert back_pis.tolist() == pis.tolist()
    for key in ("caps", "openings", "fri"):
        assert (back[key].reshape(-1) == proof[key].reshape(-1)).all()
    assert api.verify_step(back, proof["cs_cap"], ncols, digest, back_pis, log_n, check_permutation=False, compat=kp)
    # the other position of each switch
    flipped = lambda name: api.compat(**{**pos, name: 1 - pos[name]})
    assert not api.verify_step(back, proof["cs_cap"], ncols, digest, back_pis, log_n, check_permutation=False, compat=flipped("fri_mul_final_by_x"))
    assert not step_oracle.verify_step(proof, proof["cs_cap"], ncols, digest, pis, log_n, compat=orc.compat(**{**pos, "fri_mul_final_by_x": 1 - pos["fri_mul_final_by_x"]}))
    other_digest = api.circuit_digest(cs.cap(), log_n, flipped("digest_domain_separator"))
    assert other_digest.tolist() != digest.tolist()
    assert not api.verify_step(back, proof["cs_cap"], ncols, other_digest, back_pis, log_n, check_permutation=False, compat=kp)
    if pos["bytes_pi_len_prefix"]:
        # read without the prefix the length word becomes a tenth public input: another statement, which does not verify
        b2, p2 = api.step_proof_from_bytes(blob, ncols, log_n, 1, compat=flipped("bytes_pi_len_prefix"))
        assert p2.tolist() == [len(pis)] + pis.tolist()
        assert not api.verify_step(b2, proof["cs_cap"], ncols, digest, p2, log_n, check_permutation=False, compat=kp)
    else:
        # read with the prefix the first public input is taken for a length that the buffer does not have
        with pytest.raises(api.VpbsError):
            api.step_proof_from_bytes(blob, ncols, log_n, 1, compat=flipped("bytes_pi_len_prefix"))


def test_bench_dump_outputs_are_exact_and_bounded(tmp_path, monkeypatch):
    """bench.py --dump-outputs: 64-bit words go out as exact (low, high) 32-bit halves in float64; over the budget every array keeps the
    same seeded sample of its rows on every run, with the row indices beside it, and the files stay within the budget"""
    import bench
    words = np.array([0, 1, P - 1, P, (1 << 64) - 1, 0x123456789ABCDEF0], np.uint64)
    h = bench.u64_halves(words)
    assert h.dtype == np.float64 and h.shape == (6, 2)
    assert [int(lo) + (int(hi) << 32) for lo, hi in h] == [int(w) for w in words]
    small = {"a": bench.u64_halves(words), "b": np.arange(5, dtype=np.float32)}
    info = bench.dump_outputs(str(tmp_path / "small"), small)
    assert not info["sampled"] and sorted(os.listdir(tmp_path / "small")) == ["a.npy", "b.npy"]
    assert (np.load(tmp_path / "small" / "a.npy") == small["a"]).all() and np.load(tmp_path / "small" / "b.npy").dtype == np.float32
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    big = {"x": np.arange(4000, dtype=np.float32), "y": np.arange(3000, dtype=np.float64).reshape(1500, 2)}
    runs = []
    for name in ("r1", "r2"):
        info = bench.dump_outputs(str(tmp_path / name), big, rank=1, world=2)
        files = sorted(os.listdir(tmp_path / name))
        assert info["sampled"] and files == ["rank1_x.npy", "rank1_x_rows.npy", "rank1_y.npy", "rank1_y_rows.npy"]
        arrays = {f: np.load(tmp_path / name / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 4096
        assert (arrays["rank1_x.npy"] == big["x"][arrays["rank1_x_rows.npy"].astype(np.int64)]).all()
        assert (arrays["rank1_y.npy"] == big["y"][arrays["rank1_y_rows.npy"].astype(np.int64)]).all()
        runs.append(arrays)
    assert all((runs[0][f] == runs[1][f]).all() for f in runs[0])
