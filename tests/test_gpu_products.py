"""GPU tests (-m gpu) of the chained product assemblies of csrc/gl.h -- mul_nc, mul2_nc (both streams), dot2_nc, mad_nc -- on the operand set of
tools/test_asm (every ordered pair of its 21 values around 0, 2^32 - 1, 2^32, p - 1, p, 2^64 - 2^32, 2^64 - 1, and 65 536 seeded random pairs)
against Python big-integer arithmetic mod p, and of the Poseidon permutation built on them, one lane per permutation and 16 lanes per
permutation, against the oracle's.  tools/test_products (built by __graft_entry__.build()) runs the kernels on the operands it is handed."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tools/test_asm.hip: edge[] and edge2[]
EDGE = [0, 1, P - 1, P, M64, M32, 1 << 32, 0xFFFFFFFF00000000, 1 << 63,
        P + 1, M64 - 1, 0xFFFFFFFF00000002, 0xFFFFFFFEFFFFFFFF, 0xFFFFFFFF7FFFFFFF, 0xFFFFFFFFFFFF0000, 2, 0xFFFFFFFE, 0x1FFFFFFFF, 0x7FFFFFFFFFFFFFFF,
        0x8000000000000001, 0xFFFFFFFE00000001]
N_RANDOM = 1 << 16


def _run(mode, words, tmp_path):
    import __graft_entry__ as entry
    exe = entry.build_product_tool()
    src, dst = str(tmp_path / (mode + ".in")), str(tmp_path / (mode + ".out"))
    np.ascontiguousarray(words, dtype=np.uint64).tofile(src)
    r = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PRODUCTS_DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return np.fromfile(dst, dtype=np.uint64)


def _chain_words(a, b, c=0):
    """what the chained assembly of a b + c passes through: the carry c of M, M's high word, and whether the reduction takes its borrow branch"""
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    t = a0 * b0 + c
    m = a0 * b1 + (t >> 32)
    assert m <= M64, "a0 b1 + E overflows"
    m += a1 * b0
    carry, m = m >> 64, m & M64
    h = a1 * b1 + (m >> 32) + (carry << 32)
    assert h <= M64, "a1 b1 + F overflows"
    lo = (t & M32) | ((m & M32) << 32)
    assert lo + (h << 64) == a * b + c
    u = ((h & M32) * M32 + lo) & M64
    return carry, m >> 32, u < (h >> 32)


def test_product_forms_on_edge_and_random_operands(tmp_path):
    """every case is checked: mul_nc(a, b), both results of mul2_nc(a, b, c, d), dot2_nc(a, b, c, d) and mad_nc(a, b, c), made canonical, equal
    a b, c d, a b + c d and a b + c mod p.  Each (a, b) pair of the set is run once as the first and once as the second product of the two-product
    forms, and every edge pair meets the addends 0, p, 2^64 - 1 and 2^64 - 2^32 in mad_nc (and those as the other product's operand in dot2_nc)."""
    rng = np.random.default_rng(20240607)
    pairs = [(x, y) for x in EDGE for y in EDGE]
    # the set reaches what the chained form can get wrong: both values of the carry, an all-ones high word of M, the reduction's borrow branch
    seen = [_chain_words(x, y) for x, y in pairs]
    assert {s[0] for s in seen} == {0, 1} and any(s[1] == M32 for s in seen) and any(s[2] for s in seen) and not all(s[2] for s in seen)
    assert {_chain_words(x, y, z)[0] for x, y in pairs for z in (0, M64)} == {0, 1}
    ra = [int(v) for v in rng.integers(0, 1 << 64, size=N_RANDOM, dtype=np.uint64)]
    rb = [int(v) for v in rng.integers(0, 1 << 64, size=N_RANDOM, dtype=np.uint64)]
    a = [x for x, _ in pairs] + ra
    b = [y for _, y in pairs] + rb
    m = len(a)
    c = [b[(i + 7) % m] for i in range(m)]
    d = [a[(i + 13) % m] for i in range(m)]
    A, B, C, D = a + c, b + d, c + a, d + b      # each pair once in each stream
    for z in (0, P, M64, 0xFFFFFFFF00000000):
        A += [x for x, _ in pairs]
        B += [y for _, y in pairs]
        C += [z] * len(pairs)
        D += [y for _, y in pairs]
    n = len(A)
    got = _run("forms", np.array(A + B + C + D, dtype=np.uint64), tmp_path)
    assert got.size == 5 * n
    got = [int(v) for v in got]
    bad = []
    for i in range(n):
        ab, cd = A[i] * B[i], C[i] * D[i]
        want = (ab % P, ab % P, cd % P, (ab + cd) % P, (ab + C[i]) % P)
        for k, name in enumerate(("mul_nc", "mul2_nc r", "mul2_nc q", "dot2_nc", "mad_nc")):
            if got[k * n + i] != want[k]:
                bad.append((name, hex(A[i]), hex(B[i]), hex(C[i]), hex(D[i]), hex(got[k * n + i]), hex(want[k])))
    assert not bad, (len(bad), bad[:8])


def test_permutation_in_both_shapes_matches_the_oracle(tmp_path):
    """the KAT inputs and 3 000 random states through poseidon::permute (one lane each) and poseidon::permute_wide (16 lanes each): both equal
    the oracle's permutation, word for word, and the KAT outputs"""
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_kat.json")))["kats"]
    rng = np.random.default_rng(3000)
    states = np.concatenate([np.array([[int(x) for x in v["input"]] for v in kat], np.uint64),
                             rng.integers(0, P, size=(3000, 12), dtype=np.uint64)])
    n = states.shape[0]
    want = np.stack([orc.poseidon(s) for s in states])
    for i, v in enumerate(kat):
        assert [int(x) for x in want[i]] == [int(x) for x in v["output"]]
    got = _run("perm", states.reshape(-1), tmp_path)
    assert got.size == 24 * n
    lane, wide = got[:12 * n].reshape(n, 12), got[12 * n:].reshape(n, 12)
    assert (lane == want).all(), ("permute", np.argwhere(lane != want)[:4])
    assert (wide == want).all(), ("permute_wide", np.argwhere(wide != want)[:4])
