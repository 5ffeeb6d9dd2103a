"""CPU tests of the key ring's surface (vpbs_keyring_*, api.KeyRing): the header, the generated Rust binding, the ctypes table and the
argument checks of api.KeyRing.run that need no device."""
import os
import re

import numpy as np
import pytest

from vpbs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["vpbs_keyring_create", "vpbs_keyring_add", "vpbs_keyring_remove", "vpbs_keyring_count", "vpbs_keyring_run", "vpbs_keyring_free"]


def test_header_declares_the_six_entries():
    text = open(os.path.join(ROOT, "include", "vpbs_prover.h")).read()
    assert "typedef struct vpbs_keyring vpbs_keyring;" in text
    for name in ENTRIES:
        assert re.search(r"^(int|long|void|size_t) %s\(" % name, text, re.M), name
        assert name in api.SIGNATURES, name
    run = re.search(r"long vpbs_keyring_run\((.*?)\);", text, re.S).group(1)
    assert "const uint32_t* key_of" in run and run.count(",") == 9


def test_rust_binding_carries_them():
    text = open(os.path.join(ROOT, "bindings", "rust", "vpbs_sys.rs")).read()
    assert "pub struct VpbsKeyring { _private: [u8; 0] }" in text
    for name in ENTRIES:
        assert "    pub fn %s(" % name in text, name
    assert "key_of: *const u32" in text


def test_library_exports_them():
    L = api.lib()
    for name in ENTRIES:
        assert getattr(L, name).argtypes == api.SIGNATURES[name][1], name


def test_run_arguments_are_checked_without_a_device():
    N, n, max_keys = 8, 6, 3
    cts, tv = np.zeros((4, n + 1), np.uint64), np.zeros(N, np.uint64)
    c, ko, t = api.keyring_run_args(N, n, max_keys, cts, [2, 0, 1, 0], tv)
    assert ko.dtype == np.uint32 and ko.tolist() == [2, 0, 1, 0] and ko.flags["C_CONTIGUOUS"] and c.shape == (4, n + 1)
    assert api.keyring_run_args(N, n, max_keys, cts, np.array([0, 1, 2, 2], np.int64)[::1], np.zeros((4, N), np.uint64))[2].shape == (4, N)
    assert api.keyring_run_args(N, n, max_keys, cts[:0], [], tv)[1].shape == (0,)                    # an empty batch is legal
    for bad_cts in (np.zeros((4, n), np.uint64), np.zeros(n + 1, np.uint64)):
        with pytest.raises(ValueError, match="cts"):
            api.keyring_run_args(N, n, max_keys, bad_cts, [0] * 4, tv)
    for bad_tv in (np.zeros(N + 1, np.uint64), np.zeros((3, N), np.uint64)):
        with pytest.raises(ValueError, match="testv"):
            api.keyring_run_args(N, n, max_keys, cts, [0] * 4, bad_tv)
    for bad, what in (([0, 1, 2], "key_of"), ([[0, 1], [2, 0]], "key_of"), ([0.0, 1.0, 2.0, 0.0], "integers"), ([True] * 4, "integers"),
                      ([0, 1, 3, 0], r"key_of\[2\] = 3"), ([0, -1, 0, 0], r"key_of\[1\] = -1"), ([0, 0, 0, 1 << 32], r"key_of\[3\]")):
        with pytest.raises(ValueError, match=what):
            api.keyring_run_args(N, n, max_keys, cts, bad, tv)
