"""CPU tests of the surface of resuming checkpointed chains in the batch provers (vpbs_bootstrapper_run_from, vpbs_keyring_run_from,
vpbs_pbs_prover_resume, vpbs_ring_prover_resume): the header, the generated Rust binding, the ctypes table, the argument checks of
api.resume_args and api.run_from_args that need no device, and the refusals of null objects, which touch none."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vpbs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["vpbs_bootstrapper_run_from", "vpbs_keyring_run_from", "vpbs_pbs_prover_resume", "vpbs_ring_prover_resume"]
INVALID = -1
N, n = 8, 6


def test_header_declares_the_four_entries():
    text = open(os.path.join(ROOT, "include", "vpbs_prover.h")).read()
    for name in ENTRIES:
        assert re.search(r"^long %s\(" % name, text, re.M), name
        assert name in api.SIGNATURES, name
    args = lambda name: re.sub(r"/\*.*?\*/", "", re.search(r"long %s\((.*?)\);" % name, text, re.S).group(1))
    run_from = args("vpbs_bootstrapper_run_from")
    assert "const uint32_t* start" in run_from and "const uint64_t* acc_in" in run_from and run_from.count(",") == 10
    ring_from = args("vpbs_keyring_run_from")
    assert ring_from.index("key_of") < ring_from.index("start") < ring_from.index("acc_in") and ring_from.count(",") == 11
    resume = args("vpbs_pbs_prover_resume")
    assert "const uint8_t* const* checkpoints" in resume and "const size_t* lens" in resume and resume.count(",") == 13
    ring_resume = args("vpbs_ring_prover_resume")
    assert "const uint32_t* key_of" in ring_resume and "const uint8_t* const* checkpoints" in ring_resume and ring_resume.count(",") == 14
    # the existing entry points keep their arguments
    assert args("vpbs_bootstrapper_run").count(",") == 8 and args("vpbs_keyring_run").count(",") == 9
    assert args("vpbs_pbs_prover_run").count(",") == 11 and args("vpbs_ring_prover_run").count(",") == 12


def test_rust_binding_carries_them():
    text = open(os.path.join(ROOT, "bindings", "rust", "vpbs_sys.rs")).read()
    for name in ENTRIES:
        assert "    pub fn %s(" % name in text, name
    assert "start: *const u32, acc_in: *const u64" in text
    assert text.count("checkpoints: *const *const u8, lens: *const usize") == 2


def test_library_exports_them_with_the_tables_types():
    L = api.lib()
    for name in ENTRIES:
        fn = getattr(L, name)
        assert fn.argtypes == api.SIGNATURES[name][1] and fn.restype is C.c_long, name
    assert len(api.SIGNATURES["vpbs_bootstrapper_run_from"][1]) == 11 and len(api.SIGNATURES["vpbs_keyring_run_from"][1]) == 12
    assert len(api.SIGNATURES["vpbs_pbs_prover_resume"][1]) == 14 and len(api.SIGNATURES["vpbs_ring_prover_resume"][1]) == 15


def test_resume_args_accepts_the_legal_forms():
    cts, tv = np.zeros((3, n + 1), np.uint64), np.zeros(N, np.uint64)
    c, t, cps, ko = api.resume_args(N, n, cts, tv, [b"\x01\x02", None, bytearray(b"\x03")])
    assert c.shape == (3, n + 1) and t.shape == (N,) and cps == [b"\x01\x02", None, b"\x03"] and ko is None
    assert all(b is None or type(b) is bytes for b in cps)
    c, t, cps, ko = api.resume_args(N, n, cts, np.zeros((3, N), np.uint64), (None, None, None), steps=n + 2, key_of=[2, 0, 1], max_keys=3)
    assert cps == [None] * 3 and ko.dtype == np.uint32 and ko.tolist() == [2, 0, 1] and t.shape == (3, N)
    assert api.resume_args(N, n, cts[:0], tv, [])[2] == []   # an empty batch is legal
    ptrs, lens, alive = api._checkpoint_arrays([b"abc", None])
    assert (lens[0], lens[1], ptrs[1]) == (3, 0, None) and C.string_at(ptrs[0], 3) == b"abc" and len(alive) == 2


def test_resume_args_refusals():
    cts, tv = np.zeros((3, n + 1), np.uint64), np.zeros(N, np.uint64)
    ok = [None, b"x", None]
    for bad_cts in (np.zeros((3, n), np.uint64), np.zeros(n + 1, np.uint64)):
        with pytest.raises(ValueError, match=r"PbsProver.resume: expected cts"):
            api.resume_args(N, n, bad_cts, tv, ok)
    for bad_tv in (np.zeros(N + 1, np.uint64), np.zeros((2, N), np.uint64)):
        with pytest.raises(ValueError, match="testv"):
            api.resume_args(N, n, cts, bad_tv, ok)
    for steps in (-1, n + 3, 2.5):
        with pytest.raises(ValueError, match=r"steps must be 0 \.\. n_lwe \+ 2 = 8"):
            api.resume_args(N, n, cts, tv, ok, steps=steps)
    for bad, what in (([None, None], "expected 3 checkpoints"), ([None] * 4, "expected 3 checkpoints"), (b"abc", "list of bytes or None"),
                      (None, "list of bytes or None"), ([None, "text", None], r"checkpoints\[1\] must be bytes or None, not str"),
                      ([np.zeros(4, np.uint8), None, None], r"checkpoints\[0\] must be bytes or None, not ndarray"),
                      ([None, None, b""], r"checkpoints\[2\] is empty")):
        with pytest.raises(ValueError, match=what):
            api.resume_args(N, n, cts, tv, bad)
    # the ring prover's form: key_of as the key ring checks it, and its own name in the messages
    for bad, what in (([0, 1], "key_of"), ([0, 3, 0], r"key_of\[1\] = 3"), ([0.0, 1.0, 0.0], "integers")):
        with pytest.raises(ValueError, match=what):
            api.resume_args(N, n, cts, tv, ok, key_of=bad, max_keys=3)
    with pytest.raises(ValueError, match=r"RingProver.resume: steps"):
        api.resume_args(N, n, cts, tv, ok, steps=9, key_of=[0, 0, 0], max_keys=3)


def test_run_from_args():
    K = 2
    cts, tv, acc = np.zeros((3, n + 1), np.uint64), np.zeros(N, np.uint64), np.zeros((3, K, N), np.uint64)
    c, st, a, t = api.run_from_args(N, K, n, cts, [0, 4, n + 2], acc, tv)
    assert st.dtype == np.uint32 and st.tolist() == [0, 4, 8] and a.shape == (3, K, N)
    assert api.run_from_args(N, K, n, cts, [0, 0, 0], None, tv)[2] is None
    # a start above n + 2 is the library's refusal (it names the row): not refused here
    assert api.run_from_args(N, K, n, cts, [0, n + 3, 0], acc, tv)[1].tolist() == [0, n + 3, 0]
    for bad, what in (([0, 1], r"start \[3\]"), ([0.0, 1.0, 2.0], r"start \[3\]"), ([0, -1, 0], r"start\[1\] = -1"), ([0, 0, 1 << 32], r"start\[2\]")):
        with pytest.raises(ValueError, match=what):
            api.run_from_args(N, K, n, cts, bad, acc, tv)
    with pytest.raises(ValueError, match="needs acc_in"):
        api.run_from_args(N, K, n, cts, [0, 1, 0], None, tv)
    with pytest.raises(ValueError, match="acc_in"):
        api.run_from_args(N, K, n, cts, [0, 1, 0], acc[:2], tv)
    with pytest.raises(ValueError, match="accumulators must be True"):
        api._accs_out(np.zeros((3, n + 2, K, N), np.uint32), 3, n, K, N, "x")
    assert api._accs_out(False, 3, n, K, N, "x") is None and api._accs_out(True, 3, n, K, N, "x").shape == (3, n + 2, K, N)


def test_null_objects_are_refused_without_a_device():
    L = api.lib()
    calls = []
    cb = api.PBS_PROOF_FN(lambda *a: calls.append(a))
    err = C.create_string_buffer(512)
    cts, tv, ko = np.zeros((2, n + 1), np.uint64), np.zeros((2, N), np.uint64), np.zeros(2, np.uint32)
    out_ct, lwe_out = np.full((2, 2, N), 7, np.uint64), np.full((2, n + 1), 7, np.uint64)
    start, acc = np.array([1, 0], np.uint32), np.zeros((2, 2, N), np.uint64)
    v = lambda a: a.ctypes.data
    p = lambda a: a.ctypes.data_as(api.U64P)
    assert L.vpbs_bootstrapper_run_from(None, v(cts), 2, v(start), v(acc), v(tv), 1, v(out_ct), v(lwe_out), None, 0) == INVALID
    assert L.vpbs_keyring_run_from(None, v(cts), 2, v(ko), v(start), v(acc), v(tv), 1, v(out_ct), v(lwe_out), None, 0) == INVALID
    ptrs, lens, alive = api._checkpoint_arrays([b"\0" * 64, None])
    cp, ln = C.addressof(ptrs), C.addressof(lens)
    assert L.vpbs_pbs_prover_resume(None, p(cts), 2, p(tv), 1, cp, ln, 0, p(out_ct), p(lwe_out), cb, None, err, 512) == INVALID
    assert err.value == b"null prover"
    assert L.vpbs_ring_prover_resume(None, p(cts), 2, v(ko), p(tv), 1, cp, ln, 0, p(out_ct), p(lwe_out), cb, None, err, 512) == INVALID
    assert err.value == b"null prover"
    none = C.cast(None, api.PBS_PROOF_FN)
    assert L.vpbs_pbs_prover_resume(None, p(cts), 2, p(tv), 1, cp, ln, 0, p(out_ct), p(lwe_out), none, None, err, 512) == INVALID
    assert b"proof_fn" in err.value
    assert L.vpbs_ring_prover_resume(None, p(cts), 2, None, p(tv), 1, cp, ln, 0, p(out_ct), p(lwe_out), cb, None, err, 512) == INVALID
    assert b"key_of" in err.value
    assert L.vpbs_pbs_prover_resume(None, p(cts), 2, p(tv), 1, cp, None, 0, p(out_ct), p(lwe_out), cb, None, err, 512) == INVALID
    assert err.value == b"checkpoints without lens"
    assert L.vpbs_pbs_prover_resume(None, p(cts), 0, p(tv), 1, cp, ln, 0, p(out_ct), p(lwe_out), cb, None, err, 512) == INVALID   # null before empty
    assert calls == [] and (out_ct == 7).all() and (lwe_out == 7).all()
