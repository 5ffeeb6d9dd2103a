"""CPU side of the batched evaluation of a program on a key ring (vpbs_program_run_batch, csrc/program.hip; api.Program.run_batch): the
header, the generated Rust binding, the ctypes table, the argument checks of api.program_batch_args that need no device, and the refusal
of a host-only program."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vpbs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vpbs_program_run_batch"


def test_header_declares_the_entry():
    text = open(os.path.join(ROOT, "include", "vpbs_prover.h")).read()
    decl = re.search(r"^long %s\((.*?)\);" % NAME, text, re.M | re.S)
    assert decl, NAME
    args = re.sub(r"/\*.*?\*/", " ", decl.group(1), flags=re.S)
    assert "const uint32_t* key_of" in args and "size_t instances" in args and "vpbs_keyring* ring" in args
    assert args.count(",") == 9 and args.split(",")[-1].strip() == "int on_device"


def test_rust_binding_carries_it_and_the_library_exports_it():
    text = open(os.path.join(ROOT, "bindings", "rust", "vpbs_sys.rs")).read()
    fn = re.search(r"    pub fn %s\((.*?)\) -> c_long;" % NAME, text, re.S)
    assert fn, NAME
    assert "key_of: *const u32" in fn.group(1) and "instances: usize" in fn.group(1) and "ring: *mut VpbsKeyring" in fn.group(1)
    assert NAME in api.SIGNATURES
    f = getattr(api.lib(), NAME)
    assert f.argtypes == api.SIGNATURES[NAME][1] and f.restype == api.SIGNATURES[NAME][0] == C.c_long
    assert len(f.argtypes) == 10 and f.argtypes[3] == C.c_size_t
    for method in ("run_batch", "run_batch_device"):
        assert callable(getattr(api.Program, method))


N, n, N_IN, N_LUTS, MAX_KEYS = 8, 6, 3, 2, 4


def args(inputs, key_of, testvs):
    return api.program_batch_args(N_IN, n, N, N_LUTS, MAX_KEYS, inputs, key_of, testvs)


def test_the_legal_forms_are_accepted():
    x, tv = np.arange(5 * N_IN * (n + 1), dtype=np.uint64).reshape(5, N_IN, n + 1), np.ones((N_LUTS, N), np.uint64)
    gx, ko, gtv = args(x, [2, 0, 1, 0, 3], tv)
    assert (gx == x).all() and gx.flags["C_CONTIGUOUS"] and (gtv == tv).all() and gtv.flags["C_CONTIGUOUS"]
    assert ko.dtype == np.uint32 and ko.tolist() == [2, 0, 1, 0, 3] and ko.flags["C_CONTIGUOUS"]
    for dtype in (np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64):
        ko = args(x, np.array([2, 0, 1, 0, 3], dtype), tv)[1]
        assert ko.dtype == np.uint32 and ko.tolist() == [2, 0, 1, 0, 3], dtype
    assert args(x[::2], np.array([3, 9, 1, 9, 0], np.int64)[::2], tv)[1].tolist() == [3, 1, 0]        # strided views are made contiguous
    ex, eko, _ = args(np.zeros((0, N_IN, n + 1), np.uint64), [], tv)                                  # an empty batch is legal
    assert ex.shape == (0, N_IN, n + 1) and eko.shape == (0,) and eko.dtype == np.uint32
    # a program without inputs: [instances][0][n + 1]
    assert api.program_batch_args(0, n, N, 1, 1, np.zeros((2, 0, n + 1), np.uint64), [0, 0], np.zeros((1, N), np.uint64))[0].shape == (2, 0, n + 1)


def test_wrong_shapes_are_refused():
    x, tv = np.zeros((4, N_IN, n + 1), np.uint64), np.zeros((N_LUTS, N), np.uint64)
    for bad in (np.zeros((N_IN, n + 1), np.uint64), np.zeros((4, N_IN, n), np.uint64), np.zeros((4, N_IN + 1, n + 1), np.uint64),
                np.zeros((4, 1, N_IN, n + 1), np.uint64)):
        with pytest.raises(ValueError, match="inputs"):
            args(bad, [0] * 4, tv)
    for bad in (np.zeros(N, np.uint64), np.zeros((N_LUTS + 1, N), np.uint64), np.zeros((N_LUTS, N + 1), np.uint64),
                np.zeros((4, N_LUTS, N), np.uint64)):
        with pytest.raises(ValueError, match="testvs"):
            args(x, [0] * 4, bad)


def test_a_wrong_key_of_is_refused_and_the_index_named():
    x, tv = np.zeros((4, N_IN, n + 1), np.uint64), np.zeros((N_LUTS, N), np.uint64)
    for bad, what in (([0, 1, 2], "key_of"), ([0] * 5, "key_of"), ([[0, 1], [2, 0]], "key_of"), ([], "key_of"),
                      ([0.0, 1.0, 2.0, 0.0], "integers"), ([True] * 4, "integers"), (["0"] * 4, "integers"),
                      ([0, -1, 0, 0], r"key_of\[1\] = -1"), (np.array([0, 0, 0, -3], np.int8), r"key_of\[3\] = -3"),
                      ([0, 1, MAX_KEYS, 0], r"key_of\[2\] = %d" % MAX_KEYS), ([1 << 32, 0, 0, 0], r"key_of\[0\] = %d" % (1 << 32))):
        with pytest.raises(ValueError, match=what):
            args(x, bad, tv)
    # the first offending index is the one named
    with pytest.raises(ValueError, match=r"key_of\[1\] = 7"):
        args(x, [0, 7, -1, 9], tv)


def test_a_host_only_program_refuses_run_batch():
    L = api.lib()
    buf = np.zeros(64, np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    ko = np.zeros(2, np.uint32)
    prog = api.Program(None, 1, [([(0, 1)], 0, 0)], 1)
    marked = np.full(64, 0xA5A5A5A5A5A5A5A5, np.uint64)
    m = C.c_void_p(marked.ctypes.data)
    assert L.vpbs_program_run_batch(prog.h, None, p, 2, ko.ctypes.data, p, m, m, m, 0) == -1
    assert L.vpbs_program_run_batch(None, None, p, 2, ko.ctypes.data, p, m, m, m, 0) == -1
    assert (marked == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
    with pytest.raises(api.VpbsError, match="host-only"):
        prog.run_batch(None, np.zeros((2, 1, 7), np.uint64), [0, 0], np.zeros((1, 8), np.uint64))
    with pytest.raises(api.VpbsError, match="host-only"):
        prog.run_batch_device(None, 0, 2, [0, 0], 0)
    assert prog.levels()[0].tolist() == [1]          # and stays usable
    prog.close()
