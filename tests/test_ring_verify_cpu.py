"""CPU side of the ring verifier (vpbs_ring_verifier_*, csrc/verify_pbs_batch.hip; api.RingVerifier) and of vpbs_program_verify_batch
(csrc/program.hip; api.Program.verify_batch): the header, the generated Rust binding, the ctypes table, the argument checks of
api.ring_verify_args that need no device, and the refusals of a null ring verifier, which touch no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vpbs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["vpbs_ring_verifier_create", "vpbs_ring_verifier_set_key", "vpbs_ring_verifier_clear_key", "vpbs_ring_verifier_count",
           "vpbs_ring_verifier_run", "vpbs_ring_verifier_free", "vpbs_program_verify_batch"]
INVALID = -1   # VPBS_ERR_INVALID


def params(text, name, ret="long"):
    """the parameter list of a declaration of the header, comments removed"""
    return re.sub(r"/\*.*?\*/", " ", re.search(r"^%s %s\((.*?)\);" % (ret, name), text, re.M | re.S).group(1), flags=re.S)


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "vpbs_prover.h")).read()
    assert "typedef struct vpbs_ring_verifier vpbs_ring_verifier;" in text
    for name in ENTRIES:
        assert re.search(r"^(int|long|void) %s\(" % name, text, re.M), name
    create = params(text, "vpbs_ring_verifier_create", "int")
    assert "const vpbs_verify_pbs_inputs* shape" in create and "unsigned max_keys" in create and "size_t max_batch" in create and create.count(",") == 6
    assert params(text, "vpbs_ring_verifier_set_key", "int").count(",") == 2 and "const uint64_t key_hash[4]" in params(text, "vpbs_ring_verifier_set_key", "int")
    run = params(text, "vpbs_ring_verifier_run")
    assert "const uint32_t* key_of" in run and "size_t n_testv" in run and "const uint32_t* testv_of" in run and run.count(",") == 14
    assert run.index("key_of") < run.index("testvs") < run.index("n_testv") < run.index("testv_of") < run.index("out_ct") < run.index("verdicts")
    batch = params(text, "vpbs_program_verify_batch")
    assert "vpbs_ring_verifier* ring_verifier" in batch and "size_t instances" in batch and "const uint32_t* key_of" in batch and batch.count(",") == 13
    # vpbs_program_verify itself stays as it is
    assert params(text, "vpbs_program_verify").count(",") == 9 and "vpbs_pbs_verifier* pbs_verifier" in params(text, "vpbs_program_verify")


def test_rust_binding_carries_them():
    text = open(os.path.join(ROOT, "bindings", "rust", "vpbs_sys.rs")).read()
    assert "pub struct VpbsRingVerifier { _private: [u8; 0] }" in text
    for name in ENTRIES:
        assert "    pub fn %s(" % name in text, name
    fn = re.search(r"    pub fn vpbs_ring_verifier_run\((.*?)\) -> c_long;", text, re.S).group(1)
    assert "v: *mut VpbsRingVerifier" in fn and "key_of: *const u32" in fn and "n_testv: usize" in fn and "testv_of: *const u32" in fn
    assert fn.count(":") == 15
    fn = re.search(r"    pub fn vpbs_program_verify_batch\((.*?)\) -> c_long;", text, re.S).group(1)
    assert "ring_verifier: *mut VpbsRingVerifier" in fn and "key_of: *const u32" in fn and "instances: usize" in fn and fn.count(":") == 14


def test_library_exports_them_with_the_tables_types():
    L = api.lib()
    text = open(os.path.join(ROOT, "include", "vpbs_prover.h")).read()
    for name in ENTRIES:
        assert name in api.SIGNATURES, name
        fn = getattr(L, name)
        assert fn.argtypes == api.SIGNATURES[name][1] and fn.restype == api.SIGNATURES[name][0], name
        ret = re.search(r"^(int|long|void) %s\(" % name, text, re.M).group(1)
        assert api.SIGNATURES[name][0] == {"int": C.c_int, "long": C.c_long, "void": None}[ret], name
        assert len(api.SIGNATURES[name][1]) == params(text, name, ret).count(",") + 1, name     # the table has the header's arity
    for cls, method in ((api.RingVerifier, "set_key"), (api.RingVerifier, "clear_key"), (api.RingVerifier, "count"), (api.RingVerifier, "verify"),
                        (api.RingVerifier, "verify_packed"), (api.RingVerifier, "close"), (api.Program, "verify_batch")):
        assert callable(getattr(cls, method))


N, K, n, MAX_KEYS, MAX_BATCH = 8, 2, 6, 3, 6


def args(count, key_of, testvs, cts=None, out_cts=None, testv_of=None):
    cts = np.zeros((count, n + 1), np.uint64) if cts is None else cts
    out_cts = np.zeros((count, K, N), np.uint64) if out_cts is None else out_cts
    return api.ring_verify_args(N, K, n, MAX_KEYS, MAX_BATCH, count, key_of, testvs, cts, out_cts, testv_of)


def test_the_legal_forms_are_accepted():
    tv = np.arange(N, dtype=np.uint64)
    ko, t, c, o, to = args(4, [2, 0, 1, 0], tv)
    assert ko.dtype == np.uint32 and ko.tolist() == [2, 0, 1, 0] and t.shape == (1, N) and c.shape == (4, n + 1) and o.shape == (4, K * N) and to is None
    assert args(4, np.array([0, 1, 2, 2], np.int64), np.zeros((4, N), np.uint64))[1].shape == (4, N)        # one test vector per proof
    ko, t, c, o, to = args(4, [0] * 4, np.zeros((2, N), np.uint64), testv_of=np.array([1, 0, 0, 1], np.int8))  # a table and its indices
    assert t.shape == (2, N) and to.dtype == np.uint32 and to.tolist() == [1, 0, 0, 1] and to.flags["C_CONTIGUOUS"]
    assert args(2, [0, 1], np.zeros((MAX_BATCH, N), np.uint64), testv_of=[MAX_BATCH - 1, 0])[4].tolist() == [MAX_BATCH - 1, 0]
    big = np.arange(8 * K * N, dtype=np.uint64).reshape(8, K, N)
    assert (args(4, [0] * 4, tv, out_cts=big[::2])[3] == big[::2].reshape(4, -1)).all()                      # strided views are made contiguous
    e = args(0, [], tv)                                                                                      # an empty batch is legal
    assert e[0].shape == (0,) and e[0].dtype == np.uint32 and e[2].shape == (0, n + 1) and e[3].shape == (0, K * N)
    assert args(MAX_BATCH, [0] * MAX_BATCH, tv)[0].size == MAX_BATCH


def test_wrong_arguments_are_refused_with_a_message():
    tv = np.zeros(N, np.uint64)
    with pytest.raises(ValueError, match=r"7 proofs exceed max_batch 6"):
        args(MAX_BATCH + 1, [0] * (MAX_BATCH + 1), tv)
    for bad in (np.zeros(N + 1, np.uint64), np.zeros((4, N, 1), np.uint64), np.zeros((MAX_BATCH + 1, N), np.uint64)):
        with pytest.raises(ValueError, match=r"expected testvs \[8\] or \[n_testv\]\[8\]"):
            args(4, [0] * 4, bad)
    for bad in (np.zeros((4, n), np.uint64), np.zeros((3, n + 1), np.uint64), np.zeros(4 * (n + 1), np.uint64)):
        with pytest.raises(ValueError, match=r"expected cts \[4\]\[7\]"):
            args(4, [0] * 4, tv, cts=bad)
    for bad in (np.zeros((4, K, N + 1), np.uint64), np.zeros((3, K, N), np.uint64), np.zeros((2, 2 * K, N), np.uint64)):
        with pytest.raises(ValueError, match=r"out_cts \[4\]\[2\]\[8\]"):
            args(4, [0] * 4, tv, out_cts=bad)
    for bad, what in (([0, 1, 2], "key_of"), ([[0, 1], [2, 0]], "key_of"), ([0.0, 1.0, 2.0, 0.0], "integers"),
                      ([0, 1, MAX_KEYS, 0], r"key_of\[2\] = 3 is not a slot of a ring of 3"), ([0, -1, 0, 0], r"key_of\[1\] = -1")):
        with pytest.raises(ValueError, match=what):
            args(4, bad, tv)
    # without testv_of the table is one vector per proof or one for all
    for bad in (np.zeros((2, N), np.uint64), np.zeros((5, N), np.uint64)):
        with pytest.raises(ValueError, match=r"without testv_of"):
            args(4, [0] * 4, bad)
    two = np.zeros((2, N), np.uint64)
    for bad, what in (([0, 1, 2, 0], r"testv_of\[2\] = 2 is not below n_testv 2"), ([0, -1, 0, 0], r"testv_of\[1\] = -1"), ([0, 1, 0], r"testv_of \[4\]"),
                      ([0.0, 1.0, 0.0, 0.0], r"testv_of \[4\] of integers")):
        with pytest.raises(ValueError, match=what):
            args(4, [0] * 4, two, testv_of=bad)


def test_a_null_ring_verifier_is_refused_without_a_device():
    L = api.lib()
    u8p = C.POINTER(C.c_uint8)
    err = C.create_string_buffer(512)
    buf, offs = np.zeros(16, np.uint8), np.array([0, 8, 16], np.uint64)
    cts, tv, out_cts, ko = np.zeros((2, n + 1), np.uint64), np.zeros((2, N), np.uint64), np.zeros((2, K, N), np.uint64), np.zeros(2, np.uint32)
    outs = [np.full(2, 0xA5, np.uint8) for _ in range(3)]
    p = lambda a: a.ctypes.data_as(api.U64P)
    rc = L.vpbs_ring_verifier_run(None, buf.ctypes.data_as(u8p), offs.ctypes.data_as(C.POINTER(C.c_size_t)), 2, ko.ctypes.data, p(tv), 2, None, p(cts),
                                  p(out_cts), *(o.ctypes.data_as(u8p) for o in outs), err, 512)
    assert rc == INVALID and b"null ring verifier" in err.value and all((o == 0xA5).all() for o in outs)
    kh = np.zeros(4, np.uint64)
    assert L.vpbs_ring_verifier_set_key(None, 0, p(kh)) == INVALID and L.vpbs_ring_verifier_clear_key(None, 0) == INVALID
    assert L.vpbs_ring_verifier_count(None) == INVALID
    h = C.c_void_p()
    assert L.vpbs_ring_verifier_create(None, None, 2, 4, C.byref(h), err, 512) == INVALID and b"null argument" in err.value and not h.value
    L.vpbs_ring_verifier_free(None)
    prog = api.Program(None, 1, [([(0, 1)], 0, 0)], 1)          # host-only: no context, no device
    x = np.zeros((2, 1, n + 1), np.uint64)
    args = lambda pr, rv: (pr, rv, p(x), 2, ko.ctypes.data, p(tv), p(out_cts), buf.ctypes.data_as(u8p), offs.ctypes.data_as(C.POINTER(C.c_size_t)),
                           *(o.ctypes.data_as(u8p) for o in outs), err, 512)
    assert L.vpbs_program_verify_batch(*args(prog.h, None)) == INVALID and b"null ring verifier" in err.value
    assert L.vpbs_program_verify_batch(*args(None, None)) == INVALID and all((o == 0xA5).all() for o in outs)
    with pytest.raises(api.VpbsError, match="host-only"):
        prog.verify_batch(None, x, [0, 0], tv[:1], out_cts[:, None], [[b""], [b""]])
    prog.close()
