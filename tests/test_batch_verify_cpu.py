"""CPU tests of the batch verifier's host side: the C ABI is exported and bound, blobs are packed with the offsets vpbs_proof_verifier_run
takes, the test layout helper agrees with the library's FRI proof size, and the library's one walk of a serialised proof agrees with the
helper's independent one."""
import ctypes as C

import numpy as np
import pytest

from batch_verify_layout import fri_rounds, proof_layout
from vpbs_amd import api


def test_batch_verifier_symbols_are_exported_and_bound():
    L = api.lib()
    for name in ("vpbs_proof_verifier_create", "vpbs_proof_verifier_run", "vpbs_proof_verifier_free"):
        assert name in api.SIGNATURES and getattr(L, name).argtypes == api.SIGNATURES[name][1]
    assert (api.VERIFY_OK, api.VERIFY_MALFORMED, api.VERIFY_VANISHING, api.VERIFY_POW, api.VERIFY_FRI, api.VERIFY_MERKLE) == tuple(range(6))


def test_pack_proofs():
    blobs = [b"abc", b"", bytes(range(9)), b"\xff"]
    buf, offs = api.pack_proofs(blobs)
    assert offs.dtype == np.uint64 and offs.tolist() == [0, 3, 3, 12, 13]
    assert buf.dtype == np.uint8 and bytes(buf) == b"".join(blobs)
    for i, b in enumerate(blobs):
        assert bytes(buf[offs[i]:offs[i + 1]]) == b
    buf, offs = api.pack_proofs([])
    assert buf.size == 0 and offs.tolist() == [0]


def test_layout_helper_matches_the_fri_proof_size():
    for log_n, ncols in ((10, [110, 135, 20, 16]), (13, [93, 135, 20, 16]), (15, [120, 135, 20, 16])):
        lay = proof_layout(ncols, log_n, 8)
        p = api.fri_params(log_n)
        fri_words = api.lib().vpbs_fri_proof_words(C.byref(p), log_n, (C.c_size_t * 4)(*ncols), 4)
        cap_words = 4 << 4
        words = 3 * cap_words + 2 * (sum(ncols) + 2) + fri_words   # the PoW witness is the last FRI word
        assert len(lay["words"]) + 1 == words
        assert lay["fixed_len"] == 8 * words + len(lay["len_bytes"])
        offs = sorted([o for _, o in lay["words"]] + [lay["pow"]])
        assert len(set(offs)) == words and offs[-1] == lay["fixed_len"] - 8


# (log_n, ncols, n_constants, num_challenges): no reduction round and an LDE barely taller than the cap (2^6 leaves over a cap of 2^4); two
# rounds whose last tree has paths of one sibling; the step circuit's shape; one challenge and another n_constants
WALK_SHAPES = [(3, [93, 135, 20, 16], 13, 2), (10, [110, 135, 20, 16], 8, 2), (13, [13 + 80, 135, 20, 16], 13, 2), (13, [85, 135, 10, 8], 5, 1)]


@pytest.mark.parametrize("pi_prefix", (1, 0))
@pytest.mark.parametrize("log_n,ncols,n_constants,nc", WALK_SHAPES)
def test_the_library_walk_matches_the_layout_helper(log_n, ncols, n_constants, nc, pi_prefix):
    """vpbs_test_proof_byte_tables: what walk_step_proof yields (the tables the device verifier uploads, the order the serialiser and the
    parser follow) against batch_verify_layout.proof_layout, for both layouts of the public-input tail (which the walk leaves alone)"""
    rounds, _ = fri_rounds(log_n)
    assert (len(rounds), log_n + 3 - 4 * len(rounds) - 4) == {3: (0, 2), 10: (2, 1), 13: (2, 4)}[log_n]   # rounds, siblings of the last tree
    lay = proof_layout(ncols, log_n, n_constants, num_challenges=nc)
    byte_order = [o for _, o in lay["words"]]
    cap_words, (n_cs, n_w, n_z, n_q) = 4 << 4, ncols
    # the arrays hold [constants_sigmas | wires | zs_partial_products | quotient | zs_next]; the bytes: .. wires | zs | zs_next | partial products | quotient
    cuts = np.cumsum([0, 3 * cap_words, 2 * (n_cs + n_w), 2 * nc, 2 * nc, 2 * (n_z - nc), 2 * n_q]).tolist()
    caps, cs_wires, zs, zs_next, pps, quot = (byte_order[a:b] for a, b in zip(cuts, cuts[1:]))
    want_src = caps + cs_wires + zs + pps + quot + zs_next + byte_order[cuts[-1]:] + [lay["pow"]]
    want_val = ([log_n + 3 - 4] * 4 + [log_n + 3 - 4 * (r + 1) - 4 for r in range(len(rounds))]) * 28

    k = api.compat(bytes_pi_len_prefix=pi_prefix)
    vi = api.VerifyInputsC(log_n=log_n, rate_bits=3, cap_height=4, n_constants_sigmas=n_cs, n_wires=n_w, n_zs_partial_products=n_z, n_quotient=n_q,
                           num_challenges=nc, n_constants=n_constants, compat=C.pointer(k))
    fn = api.lib().vpbs_test_proof_byte_tables
    fn.restype = C.c_long
    fn.argtypes = [C.POINTER(api.VerifyInputsC), C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8),
                   C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    src, off, val = np.zeros(len(want_src) + 16, np.uint32), np.zeros(len(want_val) + 16, np.uint32), np.zeros(len(want_val) + 16, np.uint8)
    n_src, n_lenb = C.c_size_t(), C.c_size_t()
    fixed = fn(C.byref(vi), src.size, off.size, src.ctypes.data_as(C.POINTER(C.c_uint32)), off.ctypes.data_as(C.POINTER(C.c_uint32)),
               val.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(n_src), C.byref(n_lenb))
    assert fixed == lay["fixed_len"]
    assert n_src.value == len(want_src) and src[:n_src.value].tolist() == want_src
    assert n_lenb.value == len(want_val) and off[:n_lenb.value].tolist() == lay["len_bytes"] and val[:n_lenb.value].tolist() == want_val
