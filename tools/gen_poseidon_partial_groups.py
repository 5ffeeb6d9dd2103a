#!/usr/bin/env python3
"""Constants for the fused partial rounds of the product Poseidon (verifiable-fhe-paper_amd/csrc/poseidon.h).

The 22 partial rounds of Poseidon-Goldilocks apply the S-box to element 0 only; everything else is linear.  Because
the MDS entries are tiny (row sum 272 < 2^8.1), the integer matrices M^2 and M^3 still have entries < 2^25, so three
consecutive partial rounds can be evaluated with ONE dense 12x12 pass of 32x32->64-bit multiply-adds (M^3 on the state)
plus two extra rows (row 0 of M and of M^2) that feed the two inner S-boxes:

  y1 = x1 with y1[0] = sbox(x1[0])                                   (x1 already contains its round constants)
  x2_0 = (M y1)[0] + c2[0]                       d2 = sbox(x2_0) - x2_0
  x3_0 = (M^2 y1)[0] + M[0][0] d2 + (M c2)[0] + c3[0]      d3 = sbox(x3_0) - x3_0
  x1' = M^3 y1 + d2 (M^2 e0) + d3 (M e0) + (M^2 c2 + M c3 + c1')     (c1' = constants of the round after the group)

The hashing kernels close the partial rounds with ONE group of four (rounds 22..25) in place of the seventh group of three
and the lone round 25.  M^4 no longer fits the scheme as it stands: its row sums reach 264^4 ~ 2^32.18, so a sum of twelve
32-bit halves times a row of M^4 can pass 2^64.  But the powers of a positive circulant flatten out: every entry of row i
of M^4 lies within 2^24.1 of the row's smallest entry b_i (~ 2^28.4).  So M^4 = N + b 1^T with a small N >= 0, and

  x4_0 = (M^3 y1)[0] + M^2[0][0] d2 + M[0][0] d3 + (M^2 c2 + M c3)[0] + c4[0]       d4 = sbox(x4_0) - x4_0
  x1' = N y1 + b * fold(sum_j y1[j]) + d2 (M^3 e0) + d3 (M^2 e0) + d4 (M e0) + (M^3 c2 + M^2 c3 + M c4 + c1')

where the sum of the twelve words is taken and folded to one 64-bit residue ONCE; its halves then enter every row as two
more multiply-adds (by b_i).  Every accumulator stays below 2^61 and fold96 is used as it is: 288 (N) + 24 (the sum) +
24 (b) + 24 + 26 + 28 (row 0 of M, M^2, M^3) + 72 (three S-box corrections) = 486 multiply-adds and 16 folds, against
386 + 288 and 26 of a group of three and a plain round.

This script emits the integer matrices and, per group, the folded constants; it checks the fused forms against the
naive permutation on random states and on the three upstream KATs before writing anything, and prints the exact
worst-case value of every accumulator of the closing group and of fold96's intermediate T (`--bounds`: print only).
"""
import json
import math
import os
import random
import re
import sys

P = 0xFFFFFFFF00000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
DIAG = [8] + [0] * 11
N_GROUPS = 7  # 7 groups of 3 partial rounds + 1 plain partial round = 22


def load_rc():
    txt = open(os.path.join(ROOT, "oracle", "poseidon_constants.h")).read()
    rc = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{16})ULL", txt)]
    assert len(rc) == 360
    return rc


def matmul(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(12)) for j in range(12)] for i in range(12)]


def matvec(m, v):
    return [sum(m[i][j] * v[j] for j in range(12)) % P for i in range(12)]


M = [[CIRC[(j - i) % 12] + (DIAG[i] if i == j else 0) for j in range(12)] for i in range(12)]
M2 = matmul(M, M)
M3 = matmul(M2, M)
M4 = matmul(M3, M)
M4_BASE = [min(row) for row in M4]                                     # b
M4_REST = [[v - M4_BASE[i] for v in M4[i]] for i in range(12)]          # N
CLOSING_FIRST_ROUND = 22                                               # the closing group of four: rounds 22..25


def sbox(x):
    return pow(x, 7, P)


def naive(state, rc):
    s = list(state)
    for r in range(30):
        s = [(s[i] + rc[12 * r + i]) % P for i in range(12)]
        if r < 4 or r >= 26:
            s = [sbox(x) for x in s]
        else:
            s[0] = sbox(s[0])
        s = matvec(M, s)
    return s


def group_constants(rc):
    groups = []
    for g in range(N_GROUPS):
        r1 = 4 + 3 * g                      # first round of the group; its constants are already in x1
        c2 = rc[12 * (r1 + 1):12 * (r1 + 2)]
        c3 = rc[12 * (r1 + 2):12 * (r1 + 3)]
        c1n = rc[12 * (r1 + 3):12 * (r1 + 4)]
        kvec = [(a + b + c) % P for a, b, c in zip(matvec(M2, c2), matvec(M, c3), c1n)]
        k2 = c2[0]
        k3 = (matvec(M, c2)[0] + c3[0]) % P
        groups.append({"kvec": kvec, "k2": k2, "k3": k3})
    return groups


def closing_constants(rc):
    r1 = CLOSING_FIRST_ROUND
    c2, c3, c4, c1n = (rc[12 * (r1 + k):12 * (r1 + k + 1)] for k in (1, 2, 3, 4))
    kvec = [(a + b + c + d) % P for a, b, c, d in zip(matvec(M3, c2), matvec(M2, c3), matvec(M, c4), c1n)]
    return {"kvec": kvec, "k2": c2[0], "k3": (matvec(M, c2)[0] + c3[0]) % P, "k4": (matvec(M2, c2)[0] + matvec(M, c3)[0] + c4[0]) % P}


def closing_group(s, g):
    """rounds 22..25 on a state that holds round 22's constants; out: the state with round 26's constants (integers mod p)"""
    y = [sbox(s[0])] + list(s[1:])
    x2 = (sum(M[0][j] * y[j] for j in range(12)) + g["k2"]) % P
    d2 = (sbox(x2) - x2) % P
    x3 = (sum(M2[0][j] * y[j] for j in range(12)) + M[0][0] * d2 + g["k3"]) % P
    d3 = (sbox(x3) - x3) % P
    x4 = (sum(M3[0][j] * y[j] for j in range(12)) + M2[0][0] * d2 + M[0][0] * d3 + g["k4"]) % P
    d4 = (sbox(x4) - x4) % P
    total = sum(y) % P
    return [(sum(M4_REST[i][j] * y[j] for j in range(12)) + M4_BASE[i] * total + d2 * M3[i][0] + d3 * M2[i][0] + d4 * M[i][0] + g["kvec"][i]) % P
            for i in range(12)]


def closing_bounds():
    """[(name, largest value, what reaches it)]: every 64-bit accumulator of the closing group with all halves (of the state, of the folded sum,
    of d2, d3, d4) at 2^32 - 1 and the constant at 2^64 - 1, in the device's split of the constant (low: k mod 2^58, high: (k >> 58) << 26) and in
    the host's (low: k mod 2^32, high: k >> 32), and fold96's T = hi_hi (2^32 - 1) + acc_lo, which must stay below 2^64"""
    h = (1 << 32) - 1
    rows = []

    def both(name, weight):
        for form, k_lo, k_hi in (("device", (1 << 58) - 1, 63 << 26), ("host", h, h)):
            lo, hi = k_lo + h * weight, k_hi + h * weight
            rows.append(("%s, %s split" % (name, form), lo, hi, (hi >> 32) * h + lo))
    both("x2_0: row 0 of M", sum(M[0]))
    both("x3_0: row 0 of M^2 + d2", sum(M2[0]) + M[0][0])
    both("x4_0: row 0 of M^3 + d2, d3", sum(M3[0]) + M2[0][0] + M[0][0])
    rows.append(("sum of the twelve words (no constant)", 12 * h, 12 * h, ((12 * h) >> 32) * h + 12 * h))
    weights = [sum(M4_REST[i]) + M4_BASE[i] + M3[i][0] + M2[i][0] + M[i][0] for i in range(12)]
    heavy = max(range(12), key=lambda i: weights[i])
    both("closing row %d (the heaviest: weight %d)" % (heavy, weights[heavy]), weights[heavy])
    return rows, weights


def print_bounds():
    rows, _ = closing_bounds()
    for name, lo, hi, t in rows:
        assert lo < 1 << 64 and hi < 1 << 64 and t < 1 << 64, name
        print("%-62s acc_lo <= %d = 2^%.3f  acc_hi <= %d = 2^%.3f  T <= 2^%.3f" % (name, lo, math.log2(lo), hi, math.log2(hi), math.log2(t)))
    print("one accumulator for a row of M^4 itself would reach (2^32 - 1) x %d = 2^%.3f: the reason for N + b 1^T"
          % (max(sum(r) for r in M4), math.log2(((1 << 32) - 1) * max(sum(r) for r in M4))))


def fused(state, rc, groups, closing=None):
    s = [(state[i] + rc[i]) % P for i in range(12)]
    for r in range(4):
        s = [sbox(x) for x in s]
        s = [(a + b) % P for a, b in zip(matvec(M, s), rc[12 * (r + 1):12 * (r + 2)])]
    for g in groups[:6] if closing else groups:
        y = [sbox(s[0])] + s[1:]
        x2 = (sum(M[0][j] * y[j] for j in range(12)) + g["k2"]) % P
        d2 = (sbox(x2) - x2) % P
        x3 = (sum(M2[0][j] * y[j] for j in range(12)) + M[0][0] * d2 + g["k3"]) % P
        d3 = (sbox(x3) - x3) % P
        s = [(sum(M3[i][j] * y[j] for j in range(12)) + d2 * M2[i][0] + d3 * M[i][0] + g["kvec"][i]) % P for i in range(12)]
    if closing:
        s = closing_group(s, closing)
    else:
        # round 25: plain partial round, then the constants of round 26
        s[0] = sbox(s[0])
        s = [(a + b) % P for a, b in zip(matvec(M, s), rc[12 * 26:12 * 27])]
    for r in range(26, 30):
        s = [sbox(x) for x in s]
        s = matvec(M, s)
        if r + 1 < 30:
            s = [(a + b) % P for a, b in zip(s, rc[12 * (r + 1):12 * (r + 2)])]
    return s


def main():
    rc = load_rc()
    groups = group_constants(rc)
    closing = closing_constants(rc)
    print_bounds()
    if "--bounds" in sys.argv:
        return
    rnd = random.Random(7)
    cases = [[0] * 12, list(range(12)), [P - 1] * 12] + [[rnd.randrange(P) for _ in range(12)] for _ in range(20)]
    for st in cases:
        assert fused(st, rc, groups) == naive(st, rc)
        assert fused(st, rc, groups, closing) == naive(st, rc)
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_kat.json")))
    for k in kat["kats"]:
        assert fused(k["input"], rc, groups) == k["output"]
        assert fused(k["input"], rc, groups, closing) == k["output"]
    mx = max(max(r) for r in M3)
    row = max(sum(r) for r in M3)
    # accumulator bound: row_sum * 2^32 (state halves) + d2 * M2[i][0] + d3 * M[i][0] + constant < 2^64
    assert mx < 1 << 25 and (row + max(max(r) for r in M2) + 64 + 1) < 1 << 31, (mx, row)
    out = ["// GENERATED by tools/gen_poseidon_partial_groups.py -- do not edit.",
           "// Integer powers of the Poseidon MDS matrix M = circ(17,15,41,16,2,28,13,13,39,18,34,20) + diag(8,0..) and the folded",
           "// round constants of the 7 fused groups of 3 partial rounds (rounds 4..24); checked against the naive permutation.",
           "// max entry of M^3 = %d; max row sum = %d (< 2^25: 64-bit accumulators of 32-bit halves cannot overflow)" % (mx, row)]
    for name, mat in (("MDS1", M), ("MDS2", M2), ("MDS3", M3)):
        out.append("static constexpr unsigned %s[12][12] = {" % name)
        for row in mat:
            out.append("    {" + ", ".join(str(v) for v in row) + "},")
        out.append("};")
    out.append("struct PartialGroup { unsigned long long kvec[12]; unsigned long long k2, k3; };")
    out.append("#define POSEIDON_PARTIAL_GROUPS_INIT { \\")
    for g in groups:
        out.append("    {{" + ", ".join("0x%016xULL" % v for v in g["kvec"]) + "}, 0x%016xULL, 0x%016xULL}, \\" % (g["k2"], g["k3"]))
    out.append("}")
    out += ["// The closing group of four partial rounds (rounds 22..25) of the hashing kernels: M^4 = MDS4, written per row as MDS4_BASE[i] (the row's",
            "// smallest entry) + a rest below 2^%d, and the folded constants; the largest row sum of M^4 is %d > 2^32, of the rests %d."
            % (max(max(r) for r in M4_REST).bit_length(), max(sum(r) for r in M4), max(sum(r) for r in M4_REST)),
            "static constexpr unsigned MDS4[12][12] = {"]
    assert max(max(r) for r in M4) < 1 << 32
    for row in M4:
        out.append("    {" + ", ".join(str(v) for v in row) + "},")
    out.append("};")
    out.append("static constexpr unsigned MDS4_BASE[12] = {" + ", ".join(str(v) for v in M4_BASE) + "};")
    out.append("struct ClosingGroup { unsigned long long kvec[12]; unsigned long long k2, k3, k4; };")
    out.append("#define POSEIDON_CLOSING_GROUP_INIT {{" + ", ".join("0x%016xULL" % v for v in closing["kvec"]) + "}, 0x%016xULL, 0x%016xULL, 0x%016xULL}"
               % (closing["k2"], closing["k3"], closing["k4"]))
    path = os.path.join(ROOT, "verifiable-fhe-paper_amd", "csrc", "poseidon_partial_groups.inc")
    open(path, "w").write("\n".join(out) + "\n")
    print("wrote", path, "max M3 entry", mx)


if __name__ == "__main__":
    main()
