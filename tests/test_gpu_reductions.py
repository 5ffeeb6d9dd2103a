"""GPU tests (-m gpu) of the reductions of csrc/gl.h and csrc/poseidon.h whose carry correction c (2^32 - 1) is one multiply-add: reduce128_asm and
reduce96_asm on constructed words, the tails of mul_nc, mul2_nc (both streams), dot2_nc and mad_nc, add_a, fold96 within its documented bounds, and the
permutation in both shapes.  The reference is Python big-integer arithmetic mod p (the permutation: the host's poseidon::permute, the C form of
the same header, and the stored KATs).  Every test computes the class of each of its operands with a host model of the form -- carry of
u = hi_lo (2^32 - 1) + lo, borrow of u - hi_hi -- and asserts that every class is there: it cannot pass by leaving one out.
tools/test_reductions (built by __graft_entry__.build()) runs the kernels on the operands it is handed; element i is thread i of 256-thread
blocks, so elements [64 k, 64 k + 64) are one wave."""
import json
import os
import subprocess

import numpy as np
import pytest

from test_gpu_products import EDGE as ASM_EDGE, _chain_words

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 1 << 16


def _run(mode, words, tmp_path):
    import __graft_entry__ as entry
    exe = entry.build_reduction_tool()
    src, dst = str(tmp_path / (mode + ".in")), str(tmp_path / (mode + ".out"))
    np.array(words, dtype=np.uint64).tofile(src)
    r = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "REDUCTIONS_DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return [int(v) for v in np.fromfile(dst, dtype=np.uint64)]


def _tail_class(value):
    """host model of the reduction tail on the integer lo + hi_lo 2^64 + hi_hi 2^96 (hi_hi may have 33 bits: dot2_nc): (carry of u, borrow of
    u - hi_hi)"""
    lo, hi_lo, hi_hi = value & M64, (value >> 64) & M32, value >> 96
    u = hi_lo * M32 + lo
    return u >> 64, int((u & M64) < hi_hi)


def _triple(cls, k):
    """the k-th (lo, hi_lo, hi_hi) of class (carry, borrow)"""
    k = k % 4096
    if cls == (0, 0):
        return (k * 0x9E3779B97F4A7C15 & (M64 >> 1)) | (1 << 40), k, k & 0xFFFF            # u < 2^63 + 2^44, and u >= 2^40 > hi_hi
    if cls == (1, 0):
        return M64 - k, M32 - (k & 7), k * 7 + 1                                             # u wraps to about 2^64 - 2^33
    if cls == (0, 1):
        return k, 0, k + 1 + (k * 2654435761 & 0x7FFFFFFF)                                   # u = lo < hi_hi
    h = 1 + (k & 0xFFFF)                                                                     # (1, 1): u = 2^64 + k, and k < hi_hi
    return (1 << 64) - h * M32 + k, h, M32 - (k & 3)


def test_reduce128_and_reduce96_in_every_class_of_carry_and_borrow(tmp_path):
    """reduce128_asm(lo, hi_lo, hi_hi) = lo + hi_lo 2^64 + hi_hi 2^96 and reduce96_asm(lo, hi_lo) = lo + hi_lo 2^64 (mod p).  Four waves uniform in
    their class (the borrow's correction sits behind a wave-level branch: taken by the whole wave, or by none of it), two mixed waves with the
    classes in turn (the branch taken with some lanes needing it and some not), then 65 536 random triples."""
    classes = [(0, 0), (1, 0), (0, 1), (1, 1)]
    triples = [_triple(c, k) for c in classes for k in range(64)]
    triples += [_triple(classes[i % 4], 64 + i) for i in range(128)]
    rng = np.random.default_rng(808)
    triples += list(zip((int(v) for v in rng.integers(0, 1 << 64, size=N_RANDOM, dtype=np.uint64)),
                        (int(v) for v in rng.integers(0, 1 << 32, size=N_RANDOM, dtype=np.uint64)),
                        (int(v) for v in rng.integers(0, 1 << 32, size=N_RANDOM, dtype=np.uint64))))
    assert all(0 <= lo <= M64 and 0 <= a <= M32 and 0 <= b <= M32 for lo, a, b in triples)
    n = len(triples)
    seen = [_tail_class(lo + (a << 64) + (b << 96)) for lo, a, b in triples]
    for w, c in enumerate(classes):
        assert set(seen[64 * w:64 * w + 64]) == {c}, (w, c)                  # a wave uniform in each class
    assert set(seen[256:320]) == set(classes) and set(seen[320:384]) == set(classes)   # mixed waves
    counts = {c: seen.count(c) for c in classes}
    print("reduce128_asm classes (carry, borrow):", counts)
    assert all(counts[c] >= 64 for c in classes), counts
    carry96 = [(a * M32 + lo) >> 64 for lo, a, _ in triples]
    assert carry96.count(0) >= 64 and carry96.count(1) >= 64
    got = _run("red", [t[0] for t in triples] + [t[1] for t in triples] + [t[2] for t in triples], tmp_path)
    assert len(got) == 2 * n
    bad = [(i, [hex(v) for v in triples[i]], hex(got[i]), hex(got[n + i])) for i, (lo, a, b) in enumerate(triples)
           if got[i] != (lo + (a << 64) + (b << 96)) % P or got[n + i] != (lo + (a << 64)) % P]
    assert not bad, (len(bad), bad[:8])


def test_product_tails_with_and_without_the_carry_correction(tmp_path):
    """mul_nc(a, b), both results of mul2_nc(a, b, c, d), dot2_nc(a, b, c, d), mad_nc(a, b, c) and add_a(a, b), made canonical, equal a b, c d,
    a b + c d, a b + c and a + b mod p on {0, 1, 2^32 - 1, 2^32, 2^32 + 1, p - 1, p, p + 1, 2^64 - 1}^2 and their neighbours, the operand set of the existing edge tests
    (which reaches the borrow) and 65 536 random pairs; each pair runs once in each stream of the two-product forms.  For every form the host model
    counts the cases that take the carry's correction and those that do not: at least 64 of each."""
    base = [0, 1, M32, 1 << 32, (1 << 32) + 1, P - 1, P, P + 1, M64]
    edge = sorted({(v + dv) & M64 for v in base for dv in (-1, 0, 1)})
    pairs = [(x, y) for x in edge for y in edge] + [(x, y) for x in ASM_EDGE for y in ASM_EDGE]
    rng = np.random.default_rng(20240608)
    a = [x for x, _ in pairs] + [int(v) for v in rng.integers(0, 1 << 64, size=N_RANDOM, dtype=np.uint64)]
    b = [y for _, y in pairs] + [int(v) for v in rng.integers(0, 1 << 64, size=N_RANDOM, dtype=np.uint64)]
    m = len(a)
    c = [b[(i + 7) % m] for i in range(m)]
    d = [a[(i + 13) % m] for i in range(m)]
    A, B, C, D = a + c, b + d, c + a, d + b      # each pair once in each stream
    n = len(A)
    values = {"mul_nc": [A[i] * B[i] for i in range(n)], "mul2_nc q": [C[i] * D[i] for i in range(n)],
              "dot2_nc": [A[i] * B[i] + C[i] * D[i] for i in range(n)], "mad_nc": [A[i] * B[i] + C[i] for i in range(n)]}
    for name, vals in values.items():
        seen = [_tail_class(v) for v in vals]
        carry = sum(s[0] for s in seen)
        print("%s: %d of %d take the carry's correction, %d reach the borrow" % (name, carry, n, sum(s[1] for s in seen)))
        assert carry >= 64 and n - carry >= 64, (name, carry, n)
    # the existing edge set reaches the borrow branch of the chained product (its own model of the chain)
    assert sum(1 for x in ASM_EDGE for y in ASM_EDGE if _chain_words(x, y)[2]) >= 1
    got = _run("forms", A + B + C + D, tmp_path)
    assert len(got) == 6 * n
    wraps = [(A[i] + B[i]) >> 64 for i in range(n)]
    twice = sum(1 for i in range(n) if wraps[i] and ((A[i] + B[i]) & M64) + M32 > M64)
    print("add_a: %d of %d sums wrap, %d of them once more under the correction" % (sum(wraps), n, twice))
    assert sum(wraps) >= 64 and n - sum(wraps) >= 64 and twice >= 1
    bad = []
    for i in range(n):
        want = (values["mul_nc"][i] % P, values["mul_nc"][i] % P, values["mul2_nc q"][i] % P, values["dot2_nc"][i] % P, values["mad_nc"][i] % P,
                (A[i] + B[i]) % P)
        for k, name in enumerate(("mul_nc", "mul2_nc r", "mul2_nc q", "dot2_nc", "mad_nc", "add_a")):
            if got[k * n + i] != want[k]:
                bad.append((name, hex(A[i]), hex(B[i]), hex(C[i]), hex(D[i]), hex(got[k * n + i]), hex(want[k])))
    assert not bad, (len(bad), bad[:8])


def test_fold96_with_and_without_the_carry_into_the_high_word(tmp_path):
    """fold96(acc_lo, acc_hi) = acc_lo + acc_hi 2^32 (mod p) within the bounds of the MDS rows (acc_lo < 2^58 + 2^41, acc_hi < 2^32 + 2^41): with
    T = hi_hi (2^32 - 1) + acc_lo, the cases where hi_lo carries out of T's high word (the correction) and where it does not, uniform waves and
    mixed ones, the largest T under hi_lo = 2^32 - 1, and 65 536 random pairs within the bounds."""
    LO_MAX, HI_MAX = (1 << 58) + (1 << 41) - 1, (1 << 32) + (1 << 41) - 1

    def carries(lo, hi):
        t = (hi >> 32) * M32 + lo
        assert t <= M64
        return ((t >> 32) + (hi & M32)) >> 32

    with_carry = [(LO_MAX - k * 0x1234567, HI_MAX - (k << 32) - k) for k in range(64)]            # hi_lo near 2^32 - 1, T's high word > 2^25
    without = [(k * 0x3FFFFFFFFFF & LO_MAX, (k % 513 << 32) + (k & 0xFFFF)) for k in range(64)]   # hi_lo < 2^16
    pairs = with_carry + without + [(with_carry if i & 1 else without)[i // 2] for i in range(128)]
    pairs += [(LO_MAX, HI_MAX), (LO_MAX, 512 << 32), (0, M32), (0, 0), (LO_MAX, M32), (M32 << 26, M32)]
    rng = np.random.default_rng(96)
    pairs += list(zip((int(v) for v in rng.integers(0, LO_MAX + 1, size=N_RANDOM, dtype=np.uint64)),
                      (int(v) for v in rng.integers(0, HI_MAX + 1, size=N_RANDOM, dtype=np.uint64))))
    assert all(0 <= lo <= LO_MAX and 0 <= hi <= HI_MAX for lo, hi in pairs)
    seen = [carries(lo, hi) for lo, hi in pairs]
    assert set(seen[:64]) == {1} and set(seen[64:128]) == {0} and set(seen[128:192]) == {0, 1}
    assert carries(LO_MAX, HI_MAX) == 1 and HI_MAX & M32 == M32
    print("fold96: %d of %d carry into the high word" % (sum(seen), len(seen)))
    assert sum(seen) >= 64 and len(seen) - sum(seen) >= 64
    got = _run("fold", [lo for lo, _ in pairs] + [hi for _, hi in pairs], tmp_path)
    bad = [(hex(lo), hex(hi), hex(got[i])) for i, (lo, hi) in enumerate(pairs) if got[i] != (lo + (hi << 32)) % P]
    assert len(got) == len(pairs) and not bad, (len(bad), bad[:8])


def test_permutation_in_both_shapes_matches_the_host_form(tmp_path):
    """the KAT inputs and 256 random states through poseidon::permute (one lane each) and poseidon::permute_wide (16 lanes each) on the device: both
    equal poseidon::permute on the host (plain C, no asm), word for word, and the host's results on the KAT inputs are the KAT outputs"""
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_kat.json")))["kats"]
    rng = np.random.default_rng(256)
    states = [[int(x) for x in v["input"]] for v in kat] + [[int(x) for x in row] for row in rng.integers(0, P, size=(256, 12), dtype=np.uint64)]
    n = len(states)
    got = _run("perm", [x for s in states for x in s], tmp_path)
    assert len(got) == 36 * n
    lane, wide, host = got[:12 * n], got[12 * n:24 * n], got[24 * n:]
    for i, v in enumerate(kat):
        assert host[12 * i:12 * i + 12] == [int(x) for x in v["output"]], i
    assert lane == host, [i for i in range(12 * n) if lane[i] != host[i]][:4]
    assert wide == host, [i for i in range(12 * n) if wide[i] != host[i]][:4]
