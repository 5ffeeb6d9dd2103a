"""CPU tests of the batch verifier's host side: the C ABI is exported and bound, blobs are packed with the offsets vpbs_proof_verifier_run
takes, and the test layout helper agrees with the library's FRI proof size."""
import ctypes as C

import numpy as np

from batch_verify_layout import proof_layout
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
