"""CPU side of the ring prover (vpbs_ring_prover_*, csrc/pbs_prove_ring.hip; api.RingProver) and of vpbs_program_prove_batch (csrc/program.hip;
api.Program.prove_batch): the header, the generated Rust binding, the ctypes table, the argument checks of api.ring_prove_args that need
no device, and the refusals of a null ring prover, which touch no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vpbs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["vpbs_ring_prover_create", "vpbs_ring_prover_add", "vpbs_ring_prover_remove", "vpbs_ring_prover_key_hash", "vpbs_ring_prover_keyring",
           "vpbs_ring_prover_context", "vpbs_ring_prover_run", "vpbs_ring_prover_verifier_data", "vpbs_ring_prover_set_check_witness",
           "vpbs_ring_prover_witness_checks", "vpbs_ring_prover_set_checkpoint", "vpbs_ring_prover_last_run", "vpbs_ring_prover_free",
           "vpbs_program_prove_batch"]
INVALID = -1   # VPBS_ERR_INVALID


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "vpbs_prover.h")).read()
    assert "typedef struct vpbs_ring_prover vpbs_ring_prover;" in text
    for name in ENTRIES:
        assert re.search(r"^(int|long|void|vpbs_keyring\*|vpbs_ctx\*) %s\(" % name, text, re.M), name
    run = re.sub(r"/\*.*?\*/", " ", re.search(r"^long vpbs_ring_prover_run\((.*?)\);", text, re.M | re.S).group(1), flags=re.S)
    assert "const uint32_t* key_of" in run and "vpbs_pbs_proof_fn proof_fn" in run and run.count(",") == 12
    batch = re.sub(r"/\*.*?\*/", " ", re.search(r"^long vpbs_program_prove_batch\((.*?)\);", text, re.M | re.S).group(1), flags=re.S)
    assert "vpbs_ring_prover* ring_prover" in batch and "size_t instances" in batch and "const uint32_t* key_of" in batch and batch.count(",") == 12


def test_rust_binding_carries_them():
    text = open(os.path.join(ROOT, "bindings", "rust", "vpbs_sys.rs")).read()
    assert "pub struct VpbsRingProver { _private: [u8; 0] }" in text
    for name in ENTRIES:
        assert "    pub fn %s(" % name in text, name
    fn = re.search(r"    pub fn vpbs_program_prove_batch\((.*?)\) -> c_long;", text, re.S).group(1)
    assert "ring_prover: *mut VpbsRingProver" in fn and "key_of: *const u32" in fn and "instances: usize" in fn


def test_library_exports_them_with_the_tables_types():
    L = api.lib()
    for name in ENTRIES:
        assert name in api.SIGNATURES, name
        fn = getattr(L, name)
        assert fn.argtypes == api.SIGNATURES[name][1] and fn.restype == api.SIGNATURES[name][0], name
    assert api.SIGNATURES["vpbs_ring_prover_run"][0] == api.SIGNATURES["vpbs_program_prove_batch"][0] == C.c_long
    for cls, method in ((api.RingProver, "add"), (api.RingProver, "remove"), (api.RingProver, "key_hash"), (api.RingProver, "prove"),
                        (api.RingProver, "verifier_data"), (api.RingProver, "close"), (api.Program, "prove_batch")):
        assert callable(getattr(cls, method))


N, n, MAX_KEYS = 8, 6, 3


def args(cts, key_of, testv, steps=0):
    return api.ring_prove_args(N, n, MAX_KEYS, cts, key_of, testv, steps)


def test_the_legal_forms_are_accepted():
    cts, tv = np.arange(4 * (n + 1), dtype=np.uint64).reshape(4, n + 1), np.ones(N, np.uint64)
    c, ko, t = args(cts, [2, 0, 1, 0], tv)
    assert (c == cts).all() and c.flags["C_CONTIGUOUS"] and ko.dtype == np.uint32 and ko.tolist() == [2, 0, 1, 0] and t.shape == (N,)
    assert args(cts, np.array([0, 1, 2, 2], np.int64), np.zeros((4, N), np.uint64), steps=n + 2)[2].shape == (4, N)
    assert args(cts[::2], np.array([2, 9, 1, 9], np.int8)[::2], tv)[1].tolist() == [2, 1]      # strided views are made contiguous
    e = args(cts[:0], [], tv)                                                                  # an empty batch is legal
    assert e[0].shape == (0, n + 1) and e[1].shape == (0,) and e[1].dtype == np.uint32


def test_wrong_arguments_are_refused_with_a_message():
    cts, tv = np.zeros((4, n + 1), np.uint64), np.zeros(N, np.uint64)
    for bad in (np.zeros((4, n), np.uint64), np.zeros(n + 1, np.uint64), np.zeros((4, 1, n + 1), np.uint64)):
        with pytest.raises(ValueError, match=r"RingProver.prove: expected cts \[count\]\[7\]"):
            args(bad, [0] * 4, tv)
    for bad in (np.zeros(N + 1, np.uint64), np.zeros((3, N), np.uint64), np.zeros((4, N, 1), np.uint64)):
        with pytest.raises(ValueError, match=r"testv \[8\] or \[count\]\[8\]"):
            args(cts, [0] * 4, bad)
    for bad, what in (([0, 1, 2], "key_of"), ([[0, 1], [2, 0]], "key_of"), ([0.0, 1.0, 2.0, 0.0], "integers"), ([True] * 4, "integers"),
                      ([0, 1, MAX_KEYS, 0], r"key_of\[2\] = 3 is not a slot of a ring of 3"), ([0, -1, 0, 0], r"key_of\[1\] = -1"),
                      ([0, 0, 0, 1 << 32], r"key_of\[3\]")):
        with pytest.raises(ValueError, match=what):
            args(cts, bad, tv)
    for bad in (n + 3, -1, 2.5):
        with pytest.raises(ValueError, match=r"steps must be 0 \.\. n_lwe \+ 2 = 8"):
            args(cts, [0] * 4, tv, steps=bad)


def test_a_null_ring_prover_is_refused_without_a_device():
    L = api.lib()
    calls = []
    cb = api.PBS_PROOF_FN(lambda *a: calls.append(a))
    err = C.create_string_buffer(512)
    cts, tv, ko = np.zeros((2, n + 1), np.uint64), np.zeros((2, N), np.uint64), np.zeros(2, np.uint32)
    out_ct, lwe_out = np.full((2, 2, N), 7, np.uint64), np.full((2, n + 1), 7, np.uint64)
    p = lambda a: a.ctypes.data_as(api.U64P)
    assert L.vpbs_ring_prover_run(None, p(cts), 2, ko.ctypes.data, p(tv), 1, 0, p(out_ct), p(lwe_out), cb, None, err, 512) == INVALID
    assert err.value == b"null prover" and calls == [] and (out_ct == 7).all() and (lwe_out == 7).all()
    assert L.vpbs_ring_prover_run(None, p(cts), 2, ko.ctypes.data, p(tv), 1, 0, p(out_ct), p(lwe_out), C.cast(None, api.PBS_PROOF_FN), None, err,
                                  512) == INVALID and b"proof_fn" in err.value
    prog = api.Program(None, 1, [([(0, 1)], 0, 0)], 1)          # host-only: no context, no device
    x = np.zeros((2, 1, n + 1), np.uint64)
    assert L.vpbs_program_prove_batch(prog.h, None, p(x), 2, ko.ctypes.data, p(tv), 0, None, None, cb, None, err, 512) == INVALID
    assert b"null ring prover" in err.value and calls == []
    with pytest.raises(api.VpbsError, match="host-only"):
        prog.prove_batch(None, x, [0, 0], tv[:1])
    prog.close()
    for fn, a in ((L.vpbs_ring_prover_key_hash, (None, 0, p(tv))), (L.vpbs_ring_prover_remove, (None, 0, err, 512)),
                  (L.vpbs_ring_prover_add, (None, None, None, 0, None, err, 512)), (L.vpbs_ring_prover_last_run, (None, None)),
                  (L.vpbs_ring_prover_set_check_witness, (None, 1))):
        assert fn(*a) == INVALID
    assert L.vpbs_ring_prover_keyring(None) is None and L.vpbs_ring_prover_context(None) is None
    L.vpbs_ring_prover_free(None)
