"""Operands, host models and big-integer references of the layer tests: the Poseidon layers of csrc/poseidon.h (mds_add_const / mds_row, the fused
partial-round groups partial_group3_core / group_row in their three forms) and gl::LazyAcc of csrc/gl.h, at the operands where the integers
their correctness rests on peak.  One definition for tests/test_gpu_layers.py (tools/test_layers on the device) and tests/test_layers_cpu.py
(`test_layers host`: the plain C forms of the same headers): each check_* below takes `run(mode, header, body) -> result words`, asserts with the
host model that every class it names is present BEFORE anything is launched, and compares every case it ran.

The matrices M, M^2, M^3, the group constants and the round constants come from tools/gen_poseidon_partial_groups.py, the script that generates
the header's tables; the reference is integers mod p throughout.  The host models restate what the DEVICE forms keep in 64-bit registers:
    MDS row r:        acc_lo = (k mod 2^58) + sum lo_j C_j,       acc_hi = ((k >> 58) << 26) + sum hi_j C_j            (C = row r of M)
    group row i:      acc_lo = (k mod 2^58) + d3_lo M[i][0] + d2_lo M^2[i][0] + sum lo_j M^3[i][j],   acc_hi likewise with ((k >> 58) << 26)
    fold96:           T = hi_hi (2^32 - 1) + acc_lo (its carry is discarded: T < 2^64 is what the form rests on), then hi_lo joins T's high word
    LazyAcc:          the four multiply-adds with their wrap counters, then reduce()'s 160-bit sum
The group model takes y_0 = sbox(w_0), d2 and d3 as canonical words.  The device holds them as residues, which differ from the canonical word only
for values below 2^32 - 1 (v + p < 2^64); the operands that reach the bounds, 2^32 - 1 and p - 1, have one 64-bit representation."""
import importlib.util
import os
import random
import subprocess

import numpy as np

from test_gpu_products import EDGE

P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
M58 = (1 << 58) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("gen_poseidon_partial_groups", os.path.join(ROOT, "tools", "gen_poseidon_partial_groups.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
M, M2, M3 = gen.M, gen.M2, gen.M3
RC = gen.load_rc()
GROUPS = gen.group_constants(RC)
INV7 = pow(7, -1, P - 1)                                  # x -> x^7 is a bijection of GF(p): 7 does not divide p - 1
MDS_ROW_SUMS = [sum(row) for row in M]                    # 264 for row 0 (its diagonal 8), 256 for the others
GROUP_WEIGHTS = [sum(M3[i]) + M2[i][0] + M[i][0] for i in range(12)]
GROUP_ROW = max(range(12), key=lambda i: GROUP_WEIGHTS[i])   # the row with the largest weight
GROUP_W = GROUP_WEIGHTS[GROUP_ROW]                        # 17 403 507


# ---------------------------------------------------------------------------------------------------------------- running the tools
def run_tool(exe, args, words, tmp_path, done):
    """one tool process at a time: operands to a file, results from a file"""
    tag = "_".join(args)
    src, dst = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".out"))
    np.ascontiguousarray(words, dtype=np.uint64).tofile(src)
    if os.path.exists(dst):
        os.remove(dst)
    r = subprocess.run([exe] + list(args) + [src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and done in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return np.fromfile(dst, dtype=np.uint64)


def layer_runner(tmp_path, host):
    import __graft_entry__ as entry
    exe = entry.build_layer_tool()

    def run(mode, header, body):
        words = np.concatenate([np.array(header, dtype=np.uint64).reshape(-1), np.ascontiguousarray(body, dtype=np.uint64).reshape(-1)])
        return run_tool(exe, (["host"] if host else []) + [mode], words, tmp_path, "LAYERS_DONE " + mode)
    return run


def u64(values):
    return np.array([int(v) for v in values], dtype=np.uint64)


def obj(a):
    """integers of any size, element by element"""
    return np.array(a, dtype=np.uint64).astype(object) if not (isinstance(a, np.ndarray) and a.dtype == object) else a


def mismatches(got, want, limit=8):
    got = np.asarray(got, dtype=np.uint64).reshape(-1)
    want = np.array([int(v) for v in np.asarray(want, dtype=object).reshape(-1)], dtype=np.uint64)      # (object: no detour through float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    return [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:limit]], len(bad)


def fold96_model(acc_lo, acc_hi):
    """(T, carry of hi_lo into T's high word) of the device's fold96, numpy uint64 in: T is computed in integers, so that T < 2^64 can be asserted"""
    lo, hi = obj(acc_lo), obj(acc_hi)
    t = (hi >> 32) * M32 + lo
    return t, ((t >> 32) + (hi & M32)) >> 32


# ---------------------------------------------------------------------------------------------------------------- the MDS layer
def mds_constant_sets():
    mix = [0, M64, P - 1, M58, 1 << 58, 0xFC00000000000000, RC[12], RC[12 * 26 + 5], P, 1, (1 << 58) + 1, 0x03FFFFFFFFFFFFFF ^ (1 << 31)]
    assert len(set(mix)) == 12
    return {"zero": [0] * 12, "ones": [M64] * 12, "p-1": [P - 1] * 12, "2^58-1": [M58] * 12, "2^58": [1 << 58] * 12,
            "top6": [0xFC00000000000000] * 12, "round1": RC[12:24], "round26": RC[12 * 26:12 * 27], "mixed": mix}


def edge_states():
    """every state with all twelve words equal to one edge value; the rotations of a single 2^64 - 1 and of a single 2^32 - 1; alternating halves"""
    states = [[v] * 12 for v in EDGE]
    for v in (M64, M32):
        states += [[v if j == r else 0 for j in range(12)] for r in range(12)]
    states.append([0xFFFFFFFF00000000 if j % 2 == 0 else 0x00000000FFFFFFFF for j in range(12)])
    return states


def mds_states():
    rng = np.random.default_rng(1212)
    return np.concatenate([u64(sum(edge_states(), [])).reshape(-1, 12), rng.integers(0, 1 << 64, size=(4096, 12), dtype=np.uint64, endpoint=False)])


def mds_model(states, kc):
    """acc_lo, acc_hi of every row (n x 12 each), exact in uint64: both stay below 2^59"""
    lo, hi = states & np.uint64(M32), states >> np.uint64(32)
    acc_lo, acc_hi = np.empty_like(states), np.empty_like(states)
    for r in range(12):
        k = kc[r] if kc is not None else 0
        acc_lo[:, r] = np.uint64(k & M58) + sum(lo[:, j] * np.uint64(M[r][j]) for j in range(12))
        acc_hi[:, r] = np.uint64((k >> 58) << 26) + sum(hi[:, j] * np.uint64(M[r][j]) for j in range(12))
    return acc_lo, acc_hi


def matvec_ref(mat, s):
    """mat s over the integers, column by column of an n x 12 object array"""
    return np.stack([sum(mat[i][j] * s[:, j] for j in range(12)) for i in range(12)], axis=1)


def check_mds(run):
    """canon of mds_add_const(s, kc) = M s + k and of mds_add_const(s, nullptr) = M s (mod p), row 0's diagonal 8 included, for every constant set
    on every state.  The model asserts, before the first launch: some case reaches the largest acc_lo and acc_hi a row can hold (all halves
    2^32 - 1 under k = 2^64 - 1) in row 0 and in another row; T < 2^64 everywhere; fold96's carry class occurs both ways."""
    sets, states = mds_constant_sets(), mds_states()
    ms = matvec_ref(M, obj(states) % P)
    top_lo = [M58 + M32 * w for w in MDS_ROW_SUMS]
    top_hi = [(63 << 26) + M32 * w for w in MDS_ROW_SUMS]
    reached_lo, reached_hi, carries, t_max = set(), set(), [0, 0], 0
    for name, kc in sets.items():
        for k in (kc, None):
            acc_lo, acc_hi = mds_model(states, k)
            t, carry = fold96_model(acc_lo, acc_hi)
            t_max = max(t_max, int(t.max()))
            c = int(carry.sum())
            carries[0] += carry.size - c
            carries[1] += c
            for r in range(12):
                if int(acc_lo[:, r].max()) == top_lo[r]:
                    reached_lo.add(r)
                if int(acc_hi[:, r].max()) == top_hi[r]:
                    reached_hi.add(r)
    print("mds rows: largest T = 2^%.3f; fold96 carries %d, none %d; rows at the largest acc_lo %s, acc_hi %s"
          % (np.log2(float(t_max)), carries[1], carries[0], sorted(reached_lo), sorted(reached_hi)))
    assert t_max < 1 << 64
    assert 0 in reached_lo and 0 in reached_hi and len(reached_lo) > 1 and len(reached_hi) > 1, (reached_lo, reached_hi)
    assert carries[0] >= 64 and carries[1] >= 64, carries
    n = states.shape[0]
    for name, kc in sets.items():
        got = run("mds", kc, states)
        assert got.size == 24 * n, (name, got.size)
        want = np.concatenate([((ms + np.array(kc, dtype=object)[None, :]) % P).reshape(-1), (ms % P).reshape(-1)])
        bad, count = mismatches(got, want)
        assert not count, (name, count, [(i // 12 % n, i % 12, "no constants" if i >= 12 * n else "constants", g, w) for i, g, w in bad])


# ---------------------------------------------------------------------------------------------------------------- the fused groups
TARGETS = [0, 1, P - 1, M32, 1 << 63]
_sbox = np.frompyfunc(lambda x: pow(int(x), 7, P), 1, 1)
_root7 = np.frompyfunc(lambda x: pow(int(x), INV7, P), 1, 1)


def group_states():
    rng = np.random.default_rng(333)
    return np.concatenate([mds_states(), rng.integers(0, 1 << 64, size=(4096, 12), dtype=np.uint64, endpoint=False)])


def group_reference(y_rest, w, g):
    """the three rounds on integers mod p with the S-box inputs w[0..3) (a column None: the computed value itself): state out, x2, x3, d2, d3"""
    G = GROUPS[g]
    y = y_rest.copy()
    y[:, 0] = _sbox(w[0])
    x2 = (sum(M[0][j] * y[:, j] for j in range(12)) + G["k2"]) % P
    d2 = (_sbox(x2 if w[1] is None else w[1]) - x2) % P
    x3 = (sum(M2[0][j] * y[:, j] for j in range(12)) + M[0][0] * d2 + G["k3"]) % P
    d3 = (_sbox(x3 if w[2] is None else w[2]) - x3) % P
    out = np.stack([(sum(M3[i][j] * y[:, j] for j in range(12)) + d2 * M2[i][0] + d3 * M[i][0] + G["kvec"][i]) % P for i in range(12)], axis=1)
    return out, x2, x3, d2, d3, y[:, 0]


def group_records(g):
    """states and wires of group g.  Wires in turn: random canonical words; the computed values themselves (the gate form then equals the plain
    form); steered words w1 = (x2 + t)^(1/7), w2 = (x3 + t)^(1/7), which make d2 = d3 = t for every target t.  Then, for every target and both
    all-ones states, records steered in w0 as well: sbox(w0) = t."""
    base = group_states()
    extreme = u64([M64] * 12 * len(TARGETS) + [M32] * 12 * len(TARGETS)).reshape(-1, 12)
    states = np.concatenate([base, extreme])
    n, nb = states.shape[0], base.shape[0]
    rng = np.random.default_rng(7000 + g)
    kind = np.array([i % 3 for i in range(nb)] + [2] * (n - nb))
    target = np.array([TARGETS[(i // 3) % len(TARGETS)] for i in range(nb)] + TARGETS * 2, dtype=object)
    rand = rng.integers(0, P, size=(n, 3), dtype=np.uint64).astype(object)
    s = obj(states)
    w0 = np.where(kind == 1, s[:, 0], rand[:, 0])
    w0[nb:] = _root7(target[nb:])
    # staged: x2 needs w0, x3 needs w1
    _, x2, _, _, _, _ = group_reference(s, [w0, None, None], g)
    w1 = np.where(kind == 0, rand[:, 1], np.where(kind == 1, x2, _root7((x2 + target) % P)))
    _, _, x3, _, _, _ = group_reference(s, [w0, w1, None], g)
    w2 = np.where(kind == 0, rand[:, 2], np.where(kind == 1, x3, _root7((x3 + target) % P)))
    return states, np.stack([w0, w1, w2], axis=1), kind, target


def group_row_model(states, y0, d2, d3, g, i):
    """acc_lo, acc_hi of row i of group g in uint64 (both below 2^59), from canonical y0, d2, d3"""
    k = GROUPS[g]["kvec"][i]
    st = states.copy()
    st[:, 0] = u64(y0)
    d2, d3 = u64(d2), u64(d3)
    acc = []
    for part, k_part in ((lambda v: v & np.uint64(M32), k & M58), (lambda v: v >> np.uint64(32), (k >> 58) << 26)):
        acc.append(np.uint64(k_part) + part(d3) * np.uint64(M[i][0]) + part(d2) * np.uint64(M2[i][0])
                   + sum(part(st[:, j]) * np.uint64(M3[i][j]) for j in range(12)))
    return acc


def check_group(run, g):
    """canon of partial_group3(s, g), of partial_group3_core<false>(s, g, nullptr, x_out) and of partial_group3_core<true>(s, g, w, x_out) = the
    three rounds on integers mod p, and x_out = exactly the canonical x2, x3 for the two forms that report them.  The model asserts first: every
    target is hit by d2 and by d3; some case comes within 2^32 * 64 of the largest acc_lo and of the largest acc_hi that the row with the largest
    weight can hold under its constant; T < 2^64 in that row for every case."""
    states, w, kind, target = group_records(g)
    n = states.shape[0]
    s = obj(states)
    plain, px2, px3, _, _, _ = group_reference(s, [s[:, 0], None, None], g)
    gate, gx2, gx3, d2, d3, y0 = group_reference(s, [w[:, 0], w[:, 1], w[:, 2]], g)
    steered = kind == 2
    assert (d2[steered] == target[steered]).all() and (d3[steered] == target[steered]).all()
    for t in TARGETS:
        assert (d2[steered] == t).sum() >= 64 and (d3[steered] == t).sum() >= 64, t
    same = kind == 1
    assert (gate[same] == plain[same]).all() and same.sum() >= 1024                      # wires = computed values: the gate form is the plain form
    acc_lo, acc_hi = group_row_model(states, y0, d2, d3, g, GROUP_ROW)
    k = GROUPS[g]["kvec"][GROUP_ROW]
    top_lo, top_hi = (k & M58) + M32 * GROUP_W, ((k >> 58) << 26) + M32 * GROUP_W
    t_row, _ = fold96_model(acc_lo, acc_hi)
    print("group %d row %d (weight %d): acc_lo up to 2^%.3f (largest possible - %d), acc_hi up to 2^%.3f (largest possible - %d), T up to 2^%.3f"
          % (g, GROUP_ROW, GROUP_W, np.log2(float(acc_lo.max())), top_lo - int(acc_lo.max()), np.log2(float(acc_hi.max())),
             top_hi - int(acc_hi.max()), np.log2(float(t_row.max()))))
    assert top_lo - int(acc_lo.max()) <= 64 << 32 and top_hi - int(acc_hi.max()) <= 64 << 32
    assert int(t_row.max()) < 1 << 64
    body = np.concatenate([states, u64(w.reshape(-1)).reshape(-1, 3)], axis=1)
    got = run("group", [g], body)
    assert got.size == 40 * n
    want = np.concatenate([plain.reshape(-1), np.concatenate([plain, px2[:, None], px3[:, None]], axis=1).reshape(-1),
                           np.concatenate([gate, gx2[:, None], gx3[:, None]], axis=1).reshape(-1)])
    bad, count = mismatches(got, want)

    def where(i):
        if i < 12 * n:
            return ("partial_group3", i // 12, i % 12)
        i -= 12 * n
        return ("core<false>" if i < 14 * n else "core<true>", i % (14 * n) // 14, i % 14)
    assert not count, (g, count, [(where(i), got_, want_) for i, got_, want_ in bad])


# ---------------------------------------------------------------------------------------------------------------- gl::LazyAcc
LAZY_VALUES = [0, 1, M32, 1 << 32, (1 << 32) + 1, P - 1, P, P + 1, M64 - 1, M64, 1 << 63, (1 << 64) - (1 << 32), 0x2FFFFFFFF, 0x200000000]
LAZY_CLASSES = [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 1), (0, 1, 0, 1), (1, 0, 0, 0), (1, 0, 0, 1), (1, 0, 1, 1), (1, 1, 0, 1)]
LAZY_TERMS = 6
LONG_LANES = 320     # lanes of the long sums: five waves in two blocks, the second one partly filled


def lazy_mac(st, c, a):
    e, m, h, ce, cm, ch = st
    c0, c1, a0, a1 = c & M32, c >> 32, a & M32, a >> 32
    e += c0 * a0
    m += c0 * a1
    cm += m >> 64
    m = (m & M64) + c1 * a0
    h += c1 * a1
    return e & M64, m & M64, h & M64, ce + (e >> 64), cm + (m >> 64), ch + (h >> 64)


def lazy_reduce_class(st):
    """reduce()'s steps on the six words: (lo < e, H < t, hh >> 32 != 0, top != 0); asserts what reduce() requires of them"""
    e, m, h, ce, cm, ch = st
    assert max(ce, cm, ch) <= M32
    lo = (e + (m << 32)) & M64
    t = (m >> 32) + ce + (1 if lo < e else 0)
    H = (h + t) & M64
    hh = (H >> 32) + cm
    top = ch + (1 if H < t else 0) + (hh >> 32)
    assert top < 1 << 32, "the precondition of reduce(): top is shifted by 32"
    return int(lo < e), int(H < t), int(hh >> 32 != 0), int(top != 0)


def lazy_state_value(st):
    e, m, h, ce, cm, ch = st
    return (e + (m << 32) + ((h + ce) << 64) + (cm << 96) + (ch << 128)) % P


def lazy_class(cs, as_):
    st = (0, 0, 0, 0, 0, 0)
    for c, a in zip(cs, as_):
        st = lazy_mac(st, c, a)
    assert lazy_state_value(st) == sum(c * a for c, a in zip(cs, as_)) % P
    return lazy_reduce_class(st)


def _waves(by_class):
    """a wave uniform in every class, then two waves with the classes in turn: distinct sequences throughout"""
    rows = [by_class[k][i] for k in LAZY_CLASSES for i in range(64)]
    rows += [by_class[LAZY_CLASSES[i % 8]][64 + i // 8] for i in range(128)]
    return rows


def _assert_waves(classes):
    for w, k in enumerate(LAZY_CLASSES):
        assert set(classes[64 * w:64 * w + 64]) == {k}, (w, k)
    assert set(classes[512:576]) == set(LAZY_CLASSES) and set(classes[576:640]) == set(LAZY_CLASSES)


def lazy_vector_sequences():
    """(c, a) sequences of at most six terms over LAZY_VALUES (shorter ones end in zero terms), found by a seeded search: 80 distinct ones of
    every class"""
    rnd = random.Random(160)
    by_class, seen = {k: [] for k in LAZY_CLASSES}, set()
    for _ in range(200000):
        if all(len(v) >= 80 for v in by_class.values()):
            break
        length = rnd.randint(1, LAZY_TERMS)
        cs = tuple(rnd.choice(LAZY_VALUES) for _ in range(length)) + (0,) * (LAZY_TERMS - length)
        as_ = tuple(rnd.choice(LAZY_VALUES) for _ in range(length)) + (0,) * (LAZY_TERMS - length)
        k = lazy_class(cs, as_)
        if (cs, as_) not in seen and len(by_class[k]) < 80:
            seen.add((cs, as_))
            by_class[k].append((cs, as_))
    assert all(len(v) >= 80 for v in by_class.values()), {k: len(v) for k, v in by_class.items()}
    return _waves(by_class)


def lazy_scalar_sequences():
    """one multiplicand sequence a (the launch's scalar operands) under which all eight classes are reached by 80 distinct c sequences each"""
    rnd = random.Random(161)
    for _ in range(400):
        as_ = tuple(rnd.choice(LAZY_VALUES) for _ in range(LAZY_TERMS))
        probe = {lazy_class(tuple(rnd.choice(LAZY_VALUES) for _ in range(LAZY_TERMS)), as_) for _ in range(400)}
        if len(probe) < 8:
            continue
        by_class, seen = {k: [] for k in LAZY_CLASSES}, set()
        for _ in range(60000):
            if all(len(v) >= 80 for v in by_class.values()):
                return as_, _waves(by_class)
            cs = tuple(rnd.choice(LAZY_VALUES) for _ in range(LAZY_TERMS))
            k = lazy_class(cs, as_)
            if cs not in seen and len(by_class[k]) < 80:
                seen.add(cs)
                by_class[k].append(cs)
    raise AssertionError("no multiplicand sequence reaches all eight classes")


def _long_operands(length, ones, seed):
    if ones:
        return np.full((length, LONG_LANES), M64, dtype=np.uint64), np.full((length, LONG_LANES), M64, dtype=np.uint64)
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 64, size=(length, LONG_LANES), dtype=np.uint64, endpoint=False),
            rng.integers(0, 1 << 64, size=(length, LONG_LANES), dtype=np.uint64, endpoint=False))


def _long_counters(c, a, lane):
    st = (0, 0, 0, 0, 0, 0)
    for j in range(c.shape[0]):
        st = lazy_mac(st, int(c[j, lane]), int(a[j, lane]))
    lazy_reduce_class(st)
    return st[3:]


def check_lazy_vector(run):
    """canon of reduce() after L calls of mac_v(c, a) = sum c a (mod p): all eight reachable classes of reduce()'s carries, each in a wave uniform
    in it and in mixed waves; sums of 135 and 4 096 products of random words and of 2^64 - 1 (wrap counters in the thousands)"""
    rows = lazy_vector_sequences()
    _assert_waves([lazy_class(cs, as_) for cs, as_ in rows])
    c = u64([cs[j] for j in range(LAZY_TERMS) for cs, _ in rows]).reshape(LAZY_TERMS, -1)
    a = u64([as_[j] for j in range(LAZY_TERMS) for _, as_ in rows]).reshape(LAZY_TERMS, -1)
    jobs = [("classes", c, a)]
    for length in (135, 4096):
        for ones in (False, True):
            cl, al = _long_operands(length, ones, 500 + length)
            counters = _long_counters(cl, al, LONG_LANES - 1)
            print("mac_v, %d products of %s: wrap counters %s" % (length, "2^64 - 1" if ones else "random words", counters))
            if length == 4096:
                assert min(counters) >= (4000 if ones else 900), counters          # about L wraps per word of 2^64 - 1, L / 4 of random halves
            jobs.append(("%d %s" % (length, "ones" if ones else "random"), cl, al))
    for name, cj, aj in jobs:
        got = run("lazyv", [cj.shape[0]], np.concatenate([cj.reshape(-1), aj.reshape(-1)]))
        bad, count = mismatches(got, (obj(cj) * obj(aj)).sum(axis=0) % P)
        assert not count, (name, count, bad)


def check_lazy_scalar(run):
    """the same through mac(c0, c1, a0, a1), whose multiplicand is a scalar operand: one sequence a per launch, every lane its own c"""
    as_, rows = lazy_scalar_sequences()
    _assert_waves([lazy_class(cs, as_) for cs in rows])
    jobs = [("classes", u64([cs[j] for j in range(LAZY_TERMS) for cs in rows]).reshape(LAZY_TERMS, -1), u64(as_))]
    for length in (135, 4096):
        for ones in (False, True):
            cl, al = _long_operands(length, ones, 900 + length)
            al = np.repeat(al[:, :1], LONG_LANES, axis=1)
            counters = _long_counters(cl, al, LONG_LANES - 1)
            print("mac, %d products of %s: wrap counters %s" % (length, "2^64 - 1" if ones else "random words", counters))
            if length == 4096:
                assert min(counters) >= (4000 if ones else 900), counters
            jobs.append(("%d %s" % (length, "ones" if ones else "random"), cl, al[:, 0]))
    for name, cj, aj in jobs:
        got = run("lazys", np.concatenate([u64([cj.shape[0]]), aj]), cj)
        bad, count = mismatches(got, (obj(cj) * obj(aj)[:, None]).sum(axis=0) % P)
        assert not count, (name, count, bad)


def lazy_reduce_states():
    """six-word states handed to reduce() directly: every combination of extreme words with the counters at 0, 1 and 2^31 - 1 (the count that
    2^31 products can leave in ce and ch), cm at its own limit 2^32 - 2, e = m = h = 2^64 - 1, and random words -- all inside top < 2^32"""
    words, counts = [0, 1, M32, 1 << 32, 1 << 63, M64 - M32, M64], [0, 1, (1 << 31) - 1]
    states = [(e, m, h, ce, cm, ch) for e in words for m in words for h in words for ce in counts for cm in counts for ch in counts]
    states += [(M64, M64, M64, ce, cm, ch) for ce in (0, M32) for cm in (0, (1 << 32) - 2, M32) for ch in (0, (1 << 31) - 1, M32 - 2)]
    rng = np.random.default_rng(6)
    w, k = rng.integers(0, 1 << 64, size=(4096, 3), dtype=np.uint64, endpoint=False), rng.integers(0, M32 - 1, size=(4096, 3), dtype=np.uint64)
    states += [tuple(int(v) for v in w[i]) + tuple(int(v) for v in k[i]) for i in range(4096)]
    return states


def check_lazy_reduce(run):
    """canon of LazyAcc{e, m, h, ce, cm, ch}.reduce() = e + 2^32 m + 2^64 (h + ce) + 2^96 cm + 2^128 ch (mod p); every reachable class of
    reduce()'s carries is among the states"""
    states = lazy_reduce_states()
    classes = [lazy_reduce_class(st) for st in states]
    counts = {k: classes.count(k) for k in sorted(set(classes))}
    print("reduce() classes (lo < e, H < t, hh >> 32, top != 0):", counts)
    assert set(LAZY_CLASSES) <= set(classes) and all(counts[k] >= 8 for k in LAZY_CLASSES), counts
    got = run("lazyred", [], u64([st[j] for j in range(6) for st in states]))
    bad, count = mismatches(got, [lazy_state_value(st) for st in states])
    assert not count, (count, [(states[i], g, w) for i, g, w in bad])


# ---------------------------------------------------------------------------------------------------------------- fold96 and the permutation
def fold96_group_pairs():
    """(acc_lo, acc_hi) over the range the fused group rows hand to fold96: acc_lo <= 2^58 - 1 + (2^32 - 1) W, acc_hi <= 0xFC000000 + (2^32 - 1) W,
    W the largest row weight.  A wave whose every lane carries from hi_lo into T's high word, one where none does, two mixed ones, the corners,
    65 536 random pairs."""
    lo_max, hi_max = M58 + M32 * GROUP_W, 0xFC000000 + M32 * GROUP_W
    top = hi_max >> 32
    with_carry = [(lo_max - k * 0x1234567, ((top - 1 - k) << 32) | (M32 - k)) for k in range(64)]      # hi_lo near 2^32 - 1, T's high word > 2^26
    without = [(k * 0x3FFFFFFFFFF & M58, ((k * 262139 % top) << 32) + (k & 0xFFFF)) for k in range(64)]   # hi_lo < 2^16, T's high word < 2^27
    pairs = with_carry + without + [(with_carry if i & 1 else without)[i // 2] for i in range(128)]
    pairs += [(lo_max, hi_max), (0, hi_max), (lo_max, 0), (0, 0), (lo_max, ((top - 1) << 32) | M32), (lo_max, M32), (0, M32), (M58, top << 32)]
    rng = np.random.default_rng(9658)
    pairs += list(zip((int(v) for v in rng.integers(0, lo_max, size=1 << 16, dtype=np.uint64, endpoint=True)),
                      (int(v) for v in rng.integers(0, hi_max, size=1 << 16, dtype=np.uint64, endpoint=True))))
    return pairs, lo_max, hi_max


def permutation_reference(states):
    """the permutation on integers mod p, round by round (constants, S-box on every word or on word 0, M), of an n x 12 array of any u64 words"""
    s = obj(states) % P
    for r in range(30):
        s = (s + np.array(RC[12 * r:12 * r + 12], dtype=object)[None, :]) % P
        if r < 4 or r >= 26:
            s = s ** 7 % P
        else:
            s[:, 0] = s[:, 0] ** 7 % P
        s = matvec_ref(M, s) % P
    return s


def noncanonical_states():
    """all twelve words one edge value (most of them >= p or next to it), 1 024 states drawn from the edge values, 1 024 over the whole u64 range"""
    rng = np.random.default_rng(4242)
    edge = u64(EDGE)
    return np.concatenate([np.repeat(edge[:, None], 12, axis=1), edge[rng.integers(0, len(EDGE), size=(1024, 12))],
                           rng.integers(0, 1 << 64, size=(1024, 12), dtype=np.uint64, endpoint=False)])


# ---------------------------------------------------------------------------------------------------------------- the table of bounds
def bounds_table():
    """per form: the largest acc_lo, acc_hi and T = hi_hi (2^32 - 1) + acc_lo, and the operand that reaches them"""
    def line(name, lo, hi, operand):
        t = (hi >> 32) * M32 + lo
        assert t < 1 << 64
        return "| %s | %d = 2^%.3f | %d = 2^%.3f | 2^%.3f | %s |" % (name, lo, np.log2(float(lo)), hi, np.log2(float(hi)), np.log2(float(t)), operand)
    rows = ["| form | largest `acc_lo` | largest `acc_hi` | `T` | reached by |", "|---|---|---|---|---|"]
    for r, label in ((0, "`mds_row`, row 0 (weight %d)" % MDS_ROW_SUMS[0]), (1, "`mds_row`, rows 1-11 (weight %d)" % MDS_ROW_SUMS[1])):
        rows.append(line(label, M58 + M32 * MDS_ROW_SUMS[r], (63 << 26) + M32 * MDS_ROW_SUMS[r], "every word 2^64 - 1, k = 2^64 - 1"))
    rows.append(line("`group_row`, row %d (weight %d)" % (GROUP_ROW, GROUP_W), M58 + M32 * GROUP_W, (63 << 26) + M32 * GROUP_W,
                     "every half, d2, d3 = 2^32 - 1, k = 2^64 - 1"))
    return "\n".join(rows)


if __name__ == "__main__":
    print(bounds_table())
