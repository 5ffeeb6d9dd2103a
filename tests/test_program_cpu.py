"""CPU side of programs of lookup gates (csrc/program.hip): the exported entry points and their ctypes bindings, the argument checks that
need no device, one test per validation rule (status and a message that names the gate), and the level vector of a host-only object
against the restatement in tests/program_oracle.py."""
import ctypes as C

import numpy as np
import pytest

import program_oracle as O
from vpbs_amd import api

P = api.P
NAMES = ["vpbs_program_create", "vpbs_program_run", "vpbs_program_prove", "vpbs_program_verify", "vpbs_program_free"]


def test_library_exports_the_entry_points_and_api_binds_them():
    L = api.lib()
    for name in NAMES + ["vpbs_program_levels"]:
        assert name in api.SIGNATURES, name
        fn = getattr(L, name)
        assert fn.argtypes == api.SIGNATURES[name][1] and fn.restype == api.SIGNATURES[name][0]
    for method in ("levels", "run", "prove", "verify", "close"):
        assert callable(getattr(api.Program, method))


def test_null_arguments_are_refused_without_a_device():
    L = api.lib()
    buf = np.zeros(64, np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    u8 = (C.c_uint8 * 8)()
    offs = (C.c_size_t * 2)(0, 8)
    out, err = C.c_void_p(), C.create_string_buffer(256)
    assert L.vpbs_program_create(None, None, C.byref(out), err, 256) == -1 and not out.value and err.value != b""
    d = api.ProgramDescC(1, 0, 1, 0, None, None, None, None, None)
    assert L.vpbs_program_create(None, C.byref(d), None, err, 256) == -1
    d = api.ProgramDescC(1, 1, 1, 0, None, None, None, None, None)          # a gate, no arrays
    assert L.vpbs_program_create(None, C.byref(d), C.byref(out), err, 256) == -1 and not out.value
    assert L.vpbs_program_levels(None, None) == -1
    assert L.vpbs_program_run(None, None, p, p, p, p, p, 0) == -1
    cb = api.PBS_PROOF_FN(lambda *a: None)
    assert L.vpbs_program_prove(None, None, api._ptr(buf), api._ptr(buf), 0, None, None, cb, None, err, 256) == -1 and err.value != b""
    assert L.vpbs_program_verify(None, None, api._ptr(buf), api._ptr(buf), api._ptr(buf), u8, offs, u8, None, None) == -1
    L.vpbs_program_free(None)
    # a host-only object (made without a context) is refused by everything that needs a device, and stays usable
    prog = api.Program(None, 1, [([(0, 1)], 0, 0)], 1)
    assert L.vpbs_program_run(prog.h, None, p, p, p, p, p, 0) == -1
    assert L.vpbs_program_prove(prog.h, None, api._ptr(buf), api._ptr(buf), 0, None, None, cb, None, err, 256) == -1
    assert L.vpbs_program_verify(prog.h, None, api._ptr(buf), api._ptr(buf), api._ptr(buf), u8, offs, u8, None, None) == -1
    assert prog.levels()[0].tolist() == [1]
    prog.close()
    prog.close()


DIAMOND = [([(0, 1)], 0, 0), ([(1, 1)], 0, 0), ([(1, 1)], 0, 0), ([(2, 1), (3, P - 1)], 5, 1)]     # 1 input, 4 gates


def refused(n_inputs, gates, n_luts, gate, word):
    with pytest.raises(api.VpbsError) as e:
        api.Program(None, n_inputs, gates, n_luts)
    text = str(e.value)
    assert "status -1" in text and ("gate %d" % gate) in text and word in text, text


def test_a_forward_reference_is_refused():
    gates = [list(g) for g in DIAMOND]
    gates[1][0] = [(4, 1)]             # gate 1 reads wire 4 = gate 3
    refused(1, gates, 2, 1, "topological")


def test_a_self_reference_is_refused():
    gates = [list(g) for g in DIAMOND]
    gates[2][0] = [(1, 1), (3, 1)]     # gate 2 reads wire 1 + 2 = itself
    refused(1, gates, 2, 2, "topological")


def test_a_lut_out_of_range_is_refused():
    gates = [list(g) for g in DIAMOND]
    gates[3][2] = 2
    refused(1, gates, 2, 3, "gate_lut")


def test_a_coefficient_equal_to_p_is_refused():
    gates = [list(g) for g in DIAMOND]
    gates[3][0] = [(2, 1), (3, P)]
    refused(1, gates, 2, 3, "term_coef")
    gates = [list(g) for g in DIAMOND]
    gates[0][1] = P
    refused(1, gates, 2, 0, "gate_const")


def test_a_broken_gate_first_is_refused():
    for first, gate in (([0, 1, 3, 2, 5], 2), ([0, 1, 2, 3, 4], 3), ([0, 1, 2, 3, 6], 3), ([1, 1, 2, 3, 5], 0)):
        arrays = O.csr(DIAMOND)
        arrays["gate_first"] = np.array(first, np.uint64)
        with pytest.raises(api.VpbsError) as e:
            api.Program(None, 1, arrays, 2)
        assert "status -1" in str(e.value) and ("gate %d" % gate) in str(e.value) and "gate_first" in str(e.value), (first, str(e.value))


def test_the_first_violation_in_gate_order_is_the_one_reported():
    gates = [list(g) for g in DIAMOND]
    gates[1][2], gates[3][0] = 7, [(9, 1)]
    assert O.validate(1, gates, 2) == (1, "lut")
    refused(1, gates, 2, 1, "gate_lut")
    assert O.validate(1, DIAMOND, 2) is None


def check_levels(n_inputs, gates, n_luts):
    want, n_levels = O.levels(n_inputs, gates)
    for form in (gates, O.csr(gates)):
        prog = api.Program(None, n_inputs, form, n_luts)
        got, n = prog.levels()
        prog.close()
        assert got.tolist() == want and n == n_levels
    return want, n_levels


def test_levels_of_a_diamond_a_chain_and_a_gate_without_terms():
    assert check_levels(1, DIAMOND, 2) == ([1, 2, 2, 3], 3)
    chain = [([(g, 1)], 0, 0) for g in range(6)]
    assert check_levels(1, chain, 1) == ([1, 2, 3, 4, 5, 6], 6)
    # a gate without terms is level 1 wherever it stands; its consumer is level 2; an input consumed late does not raise a level
    gates = [([(0, 1)], 0, 0), ([(2, 1)], 0, 0), ([], 9, 0), ([(4, 1), (0, 2)], 0, 0), ([], 0, 0)]
    assert check_levels(2, gates, 1) == ([1, 2, 1, 2, 1], 2)
    assert check_levels(3, [], 1) == ([], 0)
    assert check_levels(0, [([], 1, 0), ([(0, 3)], 0, 0)], 1) == ([1, 2], 2)


def test_levels_of_a_seeded_random_dag_of_200_gates():
    gates = O.random_dag(np.random.default_rng(200), 5, 200, 3)
    want, n_levels = check_levels(5, gates, 3)
    assert n_levels > 3 and len(set(want)) == n_levels      # every level is inhabited: the levels are contiguous
