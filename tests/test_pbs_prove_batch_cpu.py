"""CPU side of the batch prover (csrc/pbs_prove_batch.hip): the exported entry points and their bindings, those argument checks that need
no object (a run with steps > n_lwe + 2 needs one: tests/test_gpu_pbs_prove_batch.py), and the layout of the early-phase preset matrix -- the numpy statement of tests/preset_layout.py against the matrix the
device-witness pipeline's host loop builds (vpbs_test_ivc_preset_matrix), which makes that statement the yardstick for the kernels on the GPU."""
import ctypes as C
import os

import numpy as np

import export_circuits
import preset_layout
import tfhe_oracle as T
from vpbs_amd import api, circuit_file

P = api.P
INVALID = -1
NAMES = ["vpbs_pbs_prover_create", "vpbs_pbs_prover_run", "vpbs_pbs_prover_key_hash", "vpbs_pbs_prover_verifier_data",
         "vpbs_pbs_prover_set_check_witness", "vpbs_pbs_prover_witness_checks", "vpbs_pbs_prover_set_checkpoint",
         "vpbs_pbs_prover_last_run", "vpbs_pbs_prover_free"]
TEST_ENTRIES = ["vpbs_test_ivc_preset_matrix", "vpbs_test_pbs_prover_preset_matrix", "vpbs_test_pbs_prover_preset_words",
                "vpbs_test_pbs_prover_dummy_proof"]


def test_library_exports_the_entry_points_and_api_binds_them():
    L = api.lib()
    for name in NAMES:
        assert name in api.SIGNATURES, name
        fn = getattr(L, name)
        assert fn.argtypes == api.SIGNATURES[name][1] and fn.restype == api.SIGNATURES[name][0]
    for method in ("prove", "key_hash", "verifier_data", "close", "set_check_witness", "witness_checks", "on_checkpoint", "last_run"):
        assert callable(getattr(api.PbsProver, method))
    header = open(os.path.join(export_circuits.ROOT, "include", "vpbs_prover.h")).read()
    rust = open(os.path.join(export_circuits.ROOT, "bindings", "rust", "vpbs_sys.rs")).read()
    for name in NAMES:
        assert name + "(" in header and "fn " + name + "(" in rust, name
    # the test entries are exported and bound, and stay out of the C ABI and the Rust binding
    for name in TEST_ENTRIES:
        assert name in api.INTERNAL_SIGNATURES and name not in api.SIGNATURES and getattr(L, name).argtypes == api.INTERNAL_SIGNATURES[name][1]
        assert name not in header and name not in rust, name


def test_a_failed_chain_keeps_what_the_others_delivered():
    """PbsProver.prove raises PbsProveError after the run: the failed indices with their messages, and the proofs and outputs of the rest"""
    out_ct, lwe_out = np.zeros((3, 2, 8), np.uint64), np.zeros((3, 7), np.uint64)
    e = api.PbsProveError({1: "step 4: the witness violates a constraint"}, [b"a", None, b"c"], out_ct, lwe_out)
    assert isinstance(e, api.VpbsError) and "ciphertext 1: step 4" in str(e)
    assert e.failures == {1: "step 4: the witness violates a constraint"} and e.proofs == [b"a", None, b"c"]
    assert e.out_ct is out_ct and e.lwe_out is lwe_out


def n8_circuits(n_lwe=1):
    return [circuit_file.load(p) for p in export_circuits.ensure_cyclic_circuit(8, 2, 4, 5, n_lwe, 13)]


def side(d, proof_words, keep):
    c = api.IvcCircuitC()
    pre = np.ascontiguousarray(d.preset_flat, dtype=np.uint32)
    pi = np.ascontiguousarray(d.pi_flat, dtype=np.uint32)
    keep += [pre, pi, d]
    c.circuit = C.pointer(d.circuit.c)
    c.preset_pos, c.n_preset = pre.ctypes.data_as(api.U32P), pre.size
    c.pi_pos, c.n_pi = pi.ctypes.data_as(api.U32P), pi.size
    c.proof_words = proof_words
    return c


def test_malformed_arguments_are_refused_and_launch_nothing():
    """no GPU is needed to be refused: the checks come before the first context is made"""
    L = api.lib()
    cyc, dum = n8_circuits()
    keep = []
    cy, du = side(cyc, cyc.meta["proof_words"], keep), side(dum, 0, keep)
    prm = api.TfheParamsC(3, 2, 4, 5)
    keys = np.zeros(2 * 4 * 2 * 8, np.uint64)
    pk = C.c_void_p(keys.ctypes.data)

    def create(cy_=C.byref(cy), du_=C.byref(du), prm_=C.byref(prm), bsk=pk, ksk=pk, chains=2, batch=3, want_out=True):
        out, err = C.c_void_p(), C.create_string_buffer(256)
        rc = L.vpbs_pbs_prover_create(0, cy_, du_, prm_, 1, bsk, ksk, 0, chains, batch, C.byref(out) if want_out else None, err, 256)
        assert not out.value
        return rc, err.value.decode()
    for kw, word in ((dict(chains=0), "chains"), (dict(chains=65), "chains"), (dict(batch=0), "witness_batch"), (dict(cy_=None), "null"),
                     (dict(du_=None), "null"), (dict(prm_=None), "null"), (dict(bsk=None), "null"), (dict(ksk=None), "null"),
                     (dict(want_out=False), "null")):
        rc, msg = create(**kw)
        assert rc == INVALID and word in msg, (kw, rc, msg)
    # run: no proof_fn, a count with null cts or testv, a null object
    fn = api.PBS_PROOF_FN(lambda *a: None)
    none_fn = C.cast(None, api.PBS_PROOF_FN)
    buf = np.zeros(16, np.uint64)
    err = C.create_string_buffer(256)
    for args, word in (((None, api._ptr(buf), 1, api._ptr(buf), 0, 0, None, None, none_fn, None), "proof_fn"),
                       ((None, None, 1, api._ptr(buf), 0, 0, None, None, fn, None), "null cts"),
                       ((None, api._ptr(buf), 1, None, 0, 0, None, None, fn, None), "null cts or testv"),
                       ((None, api._ptr(buf), 1, api._ptr(buf), 0, 0, None, None, fn, None), "null prover")):
        assert L.vpbs_pbs_prover_run(*args, err, 256) == INVALID and word in err.value.decode(), (word, err.value)
    four = np.zeros(4, np.uint64)
    assert L.vpbs_pbs_prover_key_hash(None, api._ptr(four)) == INVALID
    assert L.vpbs_pbs_prover_verifier_data(None, None, None) == INVALID
    assert L.vpbs_pbs_prover_set_check_witness(None, 1) == INVALID and L.vpbs_pbs_prover_witness_checks(None, api._ptr(four)) == INVALID
    assert L.vpbs_pbs_prover_set_checkpoint(None, 1, C.cast(None, api.PBS_CHECKPOINT_FN), None) == INVALID
    assert L.vpbs_pbs_prover_last_run(None, None) == INVALID
    assert L.vpbs_test_pbs_prover_preset_matrix(None, api._ptr(buf), api._ptr(buf), 0, 1, api._ptr(buf)) == INVALID
    assert L.vpbs_test_pbs_prover_preset_words(None) == 0 and L.vpbs_test_pbs_prover_dummy_proof(None, api._ptr(buf)) == INVALID
    L.vpbs_pbs_prover_free(None)
    assert L.vpbs_test_ivc_preset_matrix(4, 4, 4, 4, 1, 0, 0, *([api._ptr(buf)] * 8)) == INVALID          # count = 0
    assert L.vpbs_test_ivc_preset_matrix(4, 4, 4, 4, 1, 2, 2, *([api._ptr(buf)] * 8)) == INVALID          # beyond step n + 1
    assert L.vpbs_test_ivc_preset_matrix(4, 4, 4, 4, 1, 0, 1, None, *([api._ptr(buf)] * 7)) == INVALID


def n8_chain_sources():
    """the N = 8, n = 1 chain of test_cyclic_cpu (3 steps): every source of the table, natively"""
    from test_cyclic_cpu import n8_chain_inputs
    N, K, ELL, LOGB, n_lwe = 8, 2, 4, 5, 1
    ring, (s_to, s_lwe, s_glwe, bsk, ksk), delta, testv, ct = n8_chain_inputs()
    bsk_flat, ksk_flat = np.stack([T.flatten_ggsw(g) for g in bsk]), T.flatten_ggsw(ksk)
    acc_init = [[0] * N for _ in range(K - 1)] + [testv]
    accs = np.array([[v for p in a for v in p] for a in T.pbs_chain(ring, acc_init, ct, bsk, ksk, K, ELL, LOGB)], np.uint64)
    key_links = api.hash_chain_links(np.zeros(4, np.uint64), np.stack([np.zeros(ksk_flat.size, np.uint64)] + list(bsk_flat) + [ksk_flat]))
    lwe_links = api.hash_chain_links(np.zeros(4, np.uint64), preset_layout.lwe_masks(ct).reshape(-1, 1))
    assert key_links.shape == lwe_links.shape == (n_lwe + 2, 4)
    return dict(testv=np.array(testv, np.uint64), accs=accs, key_links=key_links, lwe_links=lwe_links, ct=np.array(ct, np.uint64), bsk=bsk_flat,
                ksk=ksk_flat)


def test_the_numpy_statement_is_the_host_loops_matrix():
    cyc, dum = n8_circuits()
    proof_words, n_pi, kn = cyc.meta["proof_words"], len(cyc.pi_pos), 16
    src = n8_chain_sources()
    rng = np.random.default_rng(3)
    cyc_vk, dum_vk = rng.integers(1, P, size=68, dtype=np.uint64), rng.integers(1, P, size=68, dtype=np.uint64)
    dummy_proof = rng.integers(1, P, size=proof_words, dtype=np.uint64)
    assert n_pi == 2 * kn + 9 + 68
    for first, cnt in ((0, 3), (0, 1), (1, 2), (2, 1), (1, 1)):
        pis = np.stack([preset_layout.predecessor_public_inputs(s, src["testv"], src["accs"], src["key_links"], src["lwe_links"], cyc_vk, kn)
                        for s in range(first, first + cnt)])
        got = api.ivc_preset_matrix_for_tests(proof_words, 1, first, pis, src["ct"], src["bsk"], src["ksk"], cyc_vk, dum_vk, dummy_proof)
        want = preset_layout.matrix(first, cnt, proof_words, cyc_vk=cyc_vk, dum_vk=dum_vk, dummy_proof=dummy_proof, **src)
        assert got.shape == want.shape == (len(cyc.preset_pos), cnt), (got.shape, want.shape, len(cyc.preset_pos))
        assert (got == want).all(), (first, cnt, np.argwhere(got != want)[:5])
    # the sections are where the statement says: condition, GGSW and mask of the CMUX step (s = 1) and of the key switch (s = 2)
    m = preset_layout.matrix(0, 3, proof_words, cyc_vk=cyc_vk, dum_vk=dum_vk, dummy_proof=dummy_proof, **src)
    r = proof_words + n_pi
    assert m[r].tolist() == [0, 1, 1]
    assert (m[r + 1:r + 1 + src["ksk"].size, 0] == 0).all() and (m[r + 1:r + 1 + src["ksk"].size, 1] == src["bsk"][0]).all()
    assert (m[r + 1:r + 1 + src["ksk"].size, 2] == src["ksk"]).all()
    assert m[r + 1 + src["ksk"].size].tolist() == [int(src["ct"][1]), int(src["ct"][0]), 0]
    assert (m[:proof_words] == 0).all() and (m[-n_pi:] == 0).all()
    assert m[proof_words + kn].tolist() == [0, 1, 2]                                   # the counter the predecessor carries
    assert (m[proof_words + kn + 1:proof_words + 2 * kn + 1, 2] == src["accs"][1]).all()
