"""Operands, host model and big-integer references of the tests of the hashing permutation's new pieces (csrc/poseidon.h): the closing group of
four partial rounds (closing_group4_core / closing_row), the equality of "six groups of three + the closing group" with "seven groups of three +
round 25", and the permutation's head with the row subsets of its last layer.  In the manner of tests/layer_cases.py, whose runner, edge states
and helpers are used: one definition for tests/test_gpu_closing_group.py (tools/test_layers on the device) and tests/test_closing_group_cpu.py
(`test_layers host`); each check_* takes `run(mode, header, body) -> result words`, asserts with the host model that every class it names is
present BEFORE anything is launched, and compares every case it ran.

The closing group writes M^4 = N + b 1^T (b_i the smallest entry of row i) and takes the sum of the twelve words once, folded to a residue t
(tools/gen_poseidon_partial_groups.py).  The host model restates what the DEVICE form keeps in 64-bit registers:
    closing row i:  acc_lo = (k mod 2^58) + d4_lo M[i][0] + d3_lo M^2[i][0] + d2_lo M^3[i][0] + t_lo b_i + sum lo_j N[i][j],
                    acc_hi likewise with ((k >> 58) << 26) and the high halves
The reference is M^4 itself on integers mod p -- it knows nothing of the split.

Where the accumulators peak: every half 2^32 - 1, t's halves included.  t is no free operand (it is the fold of the state's own sum), but the
heaviest row has N[i][j] = 0 at one j, whose word is free to trim the sum: with eleven low halves 2^32 - 1, that one 10 and all high halves 0 the
fold is t_lo = 2^32 - 1; with eleven high halves 2^32 - 1, that one 1 and all low halves 0 it is t_hi = 2^32 - 1.  Together with d2 = d3 = d4 =
2^32 - 1 (low halves) or p - 1 (high halves), steered through the inverse S-box, and k = 2^64 - 1, acc_lo and acc_hi reach the generator's
largest values EXACTLY -- asserted below."""
import numpy as np

import layer_cases as lc
from layer_cases import M, M2, M3, M32, M58, M64, P, RC, gen, obj, u64

M4, M4_BASE, M4_REST = gen.M4, gen.M4_BASE, gen.M4_REST
CLOSING = gen.closing_constants(RC)
ONES = {"kvec": [M64] * 12, "k2": M64, "k3": M64, "k4": M64}          # every constant 2^64 - 1: the largest shares of both halves of the split
BOUNDS, WEIGHTS = gen.closing_bounds()
ROW = max(range(12), key=lambda i: WEIGHTS[i])                          # the heaviest row
W = WEIGHTS[ROW]
FREE = min(range(1, 12), key=lambda j: M4_REST[ROW][j])                 # the word that trims the sum (not word 0: that one is an S-box output)
TARGETS = lc.TARGETS


def header(G):
    return list(G["kvec"]) + [G["k2"], G["k3"], G["k4"]]


def fold96_device(acc_lo, acc_hi):
    """the 64-bit word the device's fold96 returns (integers in, T < 2^64 asserted)"""
    t = (acc_hi >> 32) * M32 + acc_lo
    assert t <= M64
    r = t + ((acc_hi & M32) << 32)
    return (r - (1 << 64) + M32) if r >> 64 else r


def closing_reference(states, w, G):
    """the four rounds on integers mod p with the S-box inputs w[0..4) (None: the computed value itself): state out, x2, x3, x4, d2, d3, d4, y0"""
    y = obj(states) % P
    y[:, 0] = lc._sbox(y[:, 0] if w[0] is None else w[0])
    x2 = (sum(M[0][j] * y[:, j] for j in range(12)) + G["k2"]) % P
    d2 = (lc._sbox(x2 if w[1] is None else w[1]) - x2) % P
    x3 = (sum(M2[0][j] * y[:, j] for j in range(12)) + M[0][0] * d2 + G["k3"]) % P
    d3 = (lc._sbox(x3 if w[2] is None else w[2]) - x3) % P
    x4 = (sum(M3[0][j] * y[:, j] for j in range(12)) + M2[0][0] * d2 + M[0][0] * d3 + G["k4"]) % P
    d4 = (lc._sbox(x4 if w[3] is None else w[3]) - x4) % P
    out = np.stack([(sum(M4[i][j] * y[:, j] for j in range(12)) + d2 * M3[i][0] + d3 * M2[i][0] + d4 * M[i][0] + G["kvec"][i]) % P
                    for i in range(12)], axis=1)
    return out, x2, x3, x4, d2, d3, d4, y[:, 0]


def peak_states():
    """(state for the largest acc_lo, state for the largest acc_hi) of the heaviest row; word 0 is replaced by the steered S-box output"""
    lo = [M32] * 12
    lo[FREE] = 10
    hi = [M32 << 32] * 12
    hi[FREE] = 1 << 32
    return lo, hi


def closing_records(G):
    """states, wires, kind, target.  kind 0: random wires; 1: the computed values as wires (the steered form is then the plain form); 2: wires
    steered so that d2 = d3 = d4 = target; 3 / 4: the peak records of acc_lo / acc_hi (d = 2^32 - 1 / p - 1, y0 likewise).  Waves (64 consecutive
    records): the base states carry the kinds and targets in turn (mixed waves); then one wave uniform in every target; one uniform in each peak;
    one that mixes both peaks with steered records."""
    base = lc.group_states()
    nb = base.shape[0]
    nb -= nb % 64                                                          # whole waves, so that the uniform ones below start on a wave
    base = base[:nb]
    rng = np.random.default_rng(4400)
    uni = rng.integers(0, 1 << 64, size=(64 * len(TARGETS), 12), dtype=np.uint64, endpoint=False)
    p_lo, p_hi = (u64(s) for s in peak_states())
    mix = [p_lo if i % 4 == 0 else p_hi if i % 4 == 1 else uni[i] for i in range(64)]
    states = np.concatenate([base, uni, np.tile(p_lo, (64, 1)), np.tile(p_hi, (64, 1)), np.stack(mix)])
    n = states.shape[0]
    kind = np.array([i % 3 for i in range(nb)] + [2] * len(uni) + [3] * 64 + [4] * 64 + [3 if i % 4 == 0 else 4 if i % 4 == 1 else 2 for i in range(64)])
    target = np.array([TARGETS[(i // 3) % len(TARGETS)] for i in range(nb)] + [TARGETS[i // 64] for i in range(len(uni))] + [M32] * 64 + [P - 1] * 64
                      + [M32 if i % 4 == 0 else P - 1 if i % 4 == 1 else TARGETS[i % len(TARGETS)] for i in range(64)], dtype=object)
    rand = rng.integers(0, P, size=(n, 4), dtype=np.uint64).astype(object)
    s = obj(states)
    steered = kind >= 2
    w0 = np.where(kind == 1, s[:, 0], rand[:, 0])
    w0[kind >= 3] = lc._root7(target[kind >= 3])                          # y0 = 2^32 - 1 (a low half) / p - 1 (a high half)
    # staged: x2 needs w0, x3 needs w1, x4 needs w2
    _, x2, _, _, _, _, _, _ = closing_reference(s, [w0, None, None, None], G)
    w1 = np.where(kind == 0, rand[:, 1], np.where(kind == 1, x2, lc._root7((x2 + target) % P)))
    _, _, x3, _, _, _, _, _ = closing_reference(s, [w0, w1, None, None], G)
    w2 = np.where(kind == 0, rand[:, 2], np.where(kind == 1, x3, lc._root7((x3 + target) % P)))
    _, _, _, x4, _, _, _, _ = closing_reference(s, [w0, w1, w2, None], G)
    w3 = np.where(kind == 0, rand[:, 3], np.where(kind == 1, x4, lc._root7((x4 + target) % P)))
    assert steered.sum() >= 64 * (len(TARGETS) + 3)
    return states, np.stack([w0, w1, w2, w3], axis=1), kind, target


def closing_row_model(state, y0, d2, d3, d4, G, i):
    """(acc_lo, acc_hi, t) of row i for ONE record in integers, as the device computes them: the state's words as they are (word 0: y0), the sum
    folded by the device's fold96, the constant in the device's split"""
    y = [int(y0)] + [int(v) for v in state[1:]]
    t = fold96_device(sum(v & M32 for v in y), sum(v >> 32 for v in y))
    k = G["kvec"][i]
    acc = []
    for part, k_part in ((lambda v: v & M32, k & M58), (lambda v: v >> 32, (k >> 58) << 26)):
        acc.append(k_part + part(int(d4)) * M[i][0] + part(int(d3)) * M2[i][0] + part(int(d2)) * M3[i][0] + part(t) * M4_BASE[i]
                   + sum(part(y[j]) * M4_REST[i][j] for j in range(12)))
    return acc[0], acc[1], t


def check_closing_group(run, G, name):
    """canon of closing_group4_core<false>(s, G, nullptr) and of closing_group4_core<true>(s, G, w) = the four rounds on integers mod p (M^4 itself).
    The model asserts first: every target is hit by d2, d3 and d4, in a wave uniform in it and in mixed waves; under k = 2^64 - 1 the peak records
    reach the generator's largest acc_lo and the largest acc_hi of the heaviest row (within 2^32 * 64: here exactly), in a uniform wave each and in a
    mixed one; T < 2^64 for every record of that row."""
    states, w, kind, target = closing_records(G)
    n = states.shape[0]
    plain, _, _, _, _, _, _, _ = closing_reference(states, [None] * 4, G)
    wired, _, _, _, d2, d3, d4, y0 = closing_reference(states, [w[:, k] for k in range(4)], G)
    steered = kind >= 2
    for d in (d2, d3, d4):
        assert (d[steered] == target[steered]).all()
        for t in TARGETS:
            assert (d[kind == 2] == t).sum() >= 64, t
    same = kind == 1
    assert (wired[same] == plain[same]).all() and same.sum() >= 1024
    nb = n - 64 * (len(TARGETS) + 3)
    for k, t in enumerate(TARGETS):                                      # the uniform waves
        assert set(target[nb + 64 * k:nb + 64 * k + 64]) == {t} and set(kind[nb + 64 * k:nb + 64 * k + 64]) == {2}
    assert set(kind[n - 192:n - 128]) == {3} and set(kind[n - 128:n - 64]) == {4} and set(kind[n - 64:]) == {2, 3, 4}
    k = G["kvec"][ROW]
    top_lo, top_hi = (k & M58) + M32 * W, ((k >> 58) << 26) + M32 * W
    best_lo = best_hi = t_max = 0
    for i in np.nonzero(steered)[0]:
        acc_lo, acc_hi, _ = closing_row_model(states[i], y0[i], d2[i], d3[i], d4[i], G, ROW)
        assert acc_lo <= top_lo and acc_hi <= top_hi
        t_row = (acc_hi >> 32) * M32 + acc_lo
        best_lo, best_hi, t_max = max(best_lo, acc_lo), max(best_hi, acc_hi), max(t_max, t_row)
    print("closing group (%s constants), row %d (weight %d): acc_lo up to 2^%.3f (largest possible - %d), acc_hi up to 2^%.3f (largest possible - %d), "
          "T up to 2^%.3f" % (name, ROW, W, np.log2(float(best_lo)), top_lo - best_lo, np.log2(float(best_hi)), top_hi - best_hi, np.log2(float(t_max))))
    assert top_lo - best_lo <= 64 << 32 and top_hi - best_hi <= 64 << 32
    assert t_max < 1 << 64
    if G is ONES:                                                         # the generator's table: the same two numbers
        named = [b for b in BOUNDS if b[0].startswith("closing row") and "device" in b[0]]
        assert len(named) == 1 and named[0][1] == top_lo and named[0][2] == top_hi, named
    body = np.concatenate([states, u64(w.reshape(-1)).reshape(-1, 4)], axis=1)
    got = run("group4", header(G), body)
    assert got.size == 24 * n
    bad, count = lc.mismatches(got, np.concatenate([plain.reshape(-1), wired.reshape(-1)]))
    assert not count, (name, count, [("plain" if i < 12 * n else "wired", i % (12 * n) // 12, i % 12, int(kind[i % (12 * n) // 12]), g, w_) for i, g, w_ in bad])


def check_tail(run):
    """rounds 4..25 both ways on the device: "six groups of three + the closing group" = "seven groups of three + round 25" = the 22 partial
    rounds on integers mod p, on the edge states and 4 096 random states (the words are round 4's input, constants included)"""
    states = lc.mds_states()
    assert states.shape[0] >= 4096 + len(lc.edge_states())
    s = obj(states) % P
    for r in range(4, 26):
        s[:, 0] = lc._sbox(s[:, 0])
        s = (lc.matvec_ref(M, s) + np.array(RC[12 * (r + 1):12 * (r + 2)], dtype=object)[None, :]) % P
    n = states.shape[0]
    got = run("tail", [], states)
    assert got.size == 24 * n
    assert (got[:12 * n] == got[12 * n:]).all(), "the closing group and the seventh group + round 25 disagree"
    bad, count = lc.mismatches(got, np.concatenate([s.reshape(-1), s.reshape(-1)]))
    assert not count, (count, [("closing" if i < 12 * n else "7 x 3 + 1", i % (12 * n) // 12, i % 12, g, w) for i, g, w in bad])


def check_head_and_rows(run, kats):
    """permute_head + last_rows<0, 12> = the permutation on the KATs, 3 000 random states and the non-canonical edge states; the digest rows of
    permute_digest and the capacity rows of permute_sponge between two full blocks are the same words of it"""
    rng = np.random.default_rng(2929)
    states = np.concatenate([u64([x for v in kats for x in v["input"]]).reshape(-1, 12), rng.integers(0, 1 << 64, size=(3000, 12), dtype=np.uint64, endpoint=False),
                             lc.noncanonical_states()])
    n = states.shape[0]
    want = lc.permutation_reference(states)
    for i, v in enumerate(kats):
        assert [int(x) for x in want[i]] == [int(x) for x in v["output"]], i
    got = run("perm", [], states)
    assert got.size == 20 * n
    for name, part, ref in (("head + last_rows<0, 12>", got[:12 * n], want), ("permute_digest rows 0..3", got[12 * n:16 * n], want[:, :4]),
                            ("permute_sponge rows 8..11", got[16 * n:], want[:, 8:])):
        bad, count = lc.mismatches(part, ref)
        assert not count, (name, count, bad)
