"""Forged step proofs that pass every check before the one under test (TEST INFRASTRUCTURE, not a conftest).

The verifiers check in a fixed order: parse, the vanishing identity at zeta, the proof of work, FRI consistency, the Merkle paths.  A
forger who controls the proof bytes but has no witness can still satisfy every check up to a chosen one, so a verifier must name exactly
the next check.  Three classes, each built from a circuit's shape alone (gates, n_constants, n_routed, ncols, the constants/sigmas cap
and the circuit digest):

  F1  openings from the edge pairs, one quotient chunk per challenge solved so that vanishing(zeta) = Z_H(zeta) sum_m zeta^(n m) t_m(zeta)
      holds exactly                                                                                              -> fails the PoW
  F2  F1 with the PoW witness ground for the transcript                                                          -> fails FRI
  F3  F2 with every query's leaves and folds FRI-consistent (one free slot per round solved: the folds before the
      last interpolate to edge values, the last to final_poly(x))                                              -> fails a Merkle path

and controls that move the reason one check earlier: a quotient opening + 1 (vanishing), F1's PoW witness in F3 (PoW), one fold slot + 1
and one final-polynomial coefficient + 1 (FRI).  The transcript is plonky2's (step_oracle.verify_step, orc_verify_fri), replayed with the
oracle's challenger; the gate part of the identity is oracle/gates.c, the permutation part and the FRI arithmetic are Python big-int
GF(p^2).  Nothing here reads the product library.
"""
import numpy as np

import edge_operands as eo
import oracle as orc
import step_oracle

P = orc.P
W = 7   # GF(p^2) = GF(p)[X] / (X^2 - 7)
RATE_BITS, CAP_HEIGHT, POW_BITS, DEG = 3, 4, 16, 8

# edge pairs for the openings, the folds and the final polynomial: (e, 0), (0, e), (e1, e2)
EDGE_PAIRS = [(e, 0) for e in eo.E_ROOTS] + [(0, e) for e in eo.E] + [(eo.E[i], eo.E[(5 * i + 3) % len(eo.E)]) for i in range(len(eo.E))]
# what the folds of every round but the last interpolate to: values with a second u64 alias (below 2^32 - 1) and p - 1
FOLD_TARGETS = [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), ((1 << 32) - 2, 0), (P - 1, 0), (0, P - 1)]
CLASSES = ("F1", "F2", "F3")


# ---- GF(p^2), big-int ----
def emul(x, y):
    return ((x[0] * y[0] + W * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def eadd(x, y):
    return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)


def esub(x, y):
    return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)


def einv(x):
    norm = (x[0] * x[0] - W * x[1] * x[1]) % P
    assert norm, "inverse of 0"
    i = pow(norm, P - 2, P)
    return (x[0] * i % P, (P - x[1]) * i % P)


def epow(x, k):
    r = (1, 0)
    while k:
        if k & 1:
            r = emul(r, x)
        x = emul(x, x)
        k >>= 1
    return r


def base(v):
    return (int(v) % P, 0)


def pairs(a):
    return [(int(x[0]), int(x[1])) for x in np.asarray(a).reshape(-1, 2)]


def edge_walk(n, offset, stride=1):
    return [EDGE_PAIRS[(offset + stride * k) % len(EDGE_PAIRS)] for k in range(n)]


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


class Shape:
    """what a forger knows of a circuit: gates is a gates_oracle.GateSet (None for a circuit of NoopGates or for fri_only)"""

    def __init__(self, name, log_n, ncols, n_constants, n_routed, num_challenges=2, gates=None, fri_only=False, compat=None, cap=None,
                 digest=None):
        self.name, self.log_n, self.ncols = name, log_n, [int(c) for c in ncols]
        self.n_constants, self.n_routed, self.nc, self.gates, self.fri_only = n_constants, n_routed, num_challenges, gates, fri_only
        self.compat = compat
        self.mul_final_by_x = int(compat.fri_mul_final_by_x) if compat is not None else 0
        self.cap = np.asarray(cap if cap is not None else eo.pattern(4 << CAP_HEIGHT, 5, 3), np.uint64).reshape(-1, 4)
        self.digest = np.asarray(digest if digest is not None else [eo.E[3], eo.E[5], eo.E[6], eo.E[9]], np.uint64)
        self.params = orc.fri_params(log_n, mul_final_by_x=self.mul_final_by_x)
        self.n_rounds = int(self.params.n_rounds)
        if not fri_only:
            assert ncols[2] == num_challenges * ((n_routed + DEG - 1) // DEG) and ncols[3] == num_challenges * DEG, (name, ncols)

    @classmethod
    def of_gates(cls, name, gates, log_n, n_routed=80, num_challenges=2, **kw):
        """a circuit over a gate set with the standard 135 wires: n_constants = selectors + gate constants"""
        n_constants = gates.num_selectors + gates.num_constants
        chunks = (n_routed + DEG - 1) // DEG
        return cls(name, log_n, [n_constants + n_routed, 135, num_challenges * chunks, num_challenges * DEG], n_constants, n_routed,
                   num_challenges, gates, **kw)

    def classes(self):
        """F3 needs a reduction round: with none, the final polynomial is checked against the combined leaves directly"""
        return CLASSES if self.n_rounds else CLASSES[:2]

    def controls(self):
        out = [] if self.fri_only else ["quotient+1"]
        return out + (["pow_of_F1", "fold+1", "final+1"] if self.n_rounds else ["pow_of_F1"])


class Forgery:
    """the forged proof pieces of one transcript: caps, openings, FRI words, public inputs; blob() serialises them"""

    def __init__(self, shape, kind, caps, openings, fri, pis):
        self.shape, self.kind, self.caps, self.openings, self.fri, self.pis = shape, kind, caps, openings, fri, pis

    def proof(self):
        return {"caps": self.caps, "openings": self.openings, "fri": self.fri}

    def blob(self):
        s = self.shape
        return step_oracle.to_bytes(self.proof(), s.ncols, s.n_constants, self.pis, s.log_n, s.nc, compat=s.compat)


class Forger:
    """one forged transcript of a shape: the openings (fill: "walk" of edge pairs, "zero", "minus1" = all (p - 1, p - 1)), the quotient
    chunk solve_chunk (0 or 7) solved"""

    def __init__(self, shape, seed, fill="walk", solve_chunk=0, public_inputs=None):
        s = self.shape = shape
        self.seed, self.fill, self.solve_chunk = seed, fill, solve_chunk
        self.pis = np.asarray(public_inputs if public_inputs is not None else eo.pattern(3 + seed % 6, seed, 1 + 2 * (seed % 3)), np.uint64)
        self.caps = np.stack([eo.pattern(4 << CAP_HEIGHT, 7 * seed + 11 * k, 1 + (seed + k) % 4).reshape(-1, 4) for k in range(3)])
        ch = orc.ChallengerState()
        ch.observe(s.digest)
        self.pi_hash = orc.hash_no_pad(self.pis)
        ch.observe(self.pi_hash)
        ch.observe(self.caps[0])
        self.betas, self.gammas = ch.get_n(s.nc), ch.get_n(s.nc)
        ch.observe(self.caps[1])
        self.alphas = ch.get_n(s.nc)
        ch.observe(self.caps[2])
        self.zeta = tuple(ch.get_n(2))
        self.zeta_next = emul(self.zeta, base(eo.root_of_unity(s.log_n)))
        self.ch_openings = ch   # before the openings are observed
        self.total = sum(s.ncols)
        n_open = self.total + s.nc
        if fill == "walk":
            op = edge_walk(n_open, 3 * seed, 1 + 2 * (seed % 5))
        elif fill == "zero":
            op = [(0, 0)] * n_open
        else:
            op = [(P - 1, P - 1)] * n_open
        self.open = op
        if not s.fri_only:
            self.solve_quotient()
        self.fri_alpha = self.betas_fri = None

    # ---- openings: index of each section ----
    def o_cs(self, j):
        return j

    def o_wire(self, j):
        return self.shape.ncols[0] + j

    def o_zs(self, j):
        return self.shape.ncols[0] + self.shape.ncols[1] + j

    def o_quot(self, j):
        return self.shape.ncols[0] + self.shape.ncols[1] + self.shape.ncols[2] + j

    def o_zs_next(self, c):
        return self.total + c

    def vanishing_sums(self):
        """per challenge a: the left side of the identity, gate terms alpha^T + sum_t alpha^t terms[t] (orc_check_vanishing_at_zeta
        restated; the gate terms from oracle/gates.c)"""
        s, op = self.shape, self.open
        zeta = self.zeta
        n_chunks = (s.n_routed + DEG - 1) // DEG
        num_prods = n_chunks - 1
        zeta_n = epow(zeta, 1 << s.log_n)
        z_h = esub(zeta_n, (1, 0))
        l0 = emul(z_h, einv(emul(esub(zeta, (1, 0)), base(1 << s.log_n))))
        k_is = [pow(W, j, P) for j in range(s.n_routed)]
        terms = []
        for c in range(s.nc):
            terms.append(emul(l0, esub(op[self.o_zs(c)], (1, 0))))
        for c in range(s.nc):
            beta, gamma = self.betas[c], self.gammas[c]
            for kk in range(n_chunks):
                num = den = (1, 0)
                for j in range(kk * DEG, min((kk + 1) * DEG, s.n_routed)):
                    wj = op[self.o_wire(j)]
                    num = emul(num, eadd(eadd(wj, emul(zeta, base(beta * k_is[j]))), base(gamma)))
                    den = emul(den, eadd(eadd(wj, emul(op[self.o_cs(s.n_constants + j)], base(beta))), base(gamma)))
                prev = op[self.o_zs(c)] if kk == 0 else op[self.o_zs(s.nc + c * num_prods + kk - 1)]
                nxt = op[self.o_zs_next(c)] if kk == num_prods else op[self.o_zs(s.nc + c * num_prods + kk)]
                terms.append(esub(emul(prev, num), emul(nxt, den)))
        if s.gates is not None:
            gt = pairs(s.gates.terms_zeta(np.array(op[:s.n_constants], np.uint64), np.array(op[s.ncols[0]:s.ncols[0] + s.ncols[1]], np.uint64),
                                          self.pi_hash, self.alphas))
        else:
            gt = [(0, 0)] * s.nc
        out = []
        for a in range(s.nc):
            acc = gt[a]
            for t in reversed(terms):
                acc = eadd(emul(acc, base(self.alphas[a])), t)
            out.append(acc)
        return out, z_h, zeta_n

    def solve_quotient(self):
        """t_{a, solve_chunk} such that sum_m zeta^(n m) t_{a,m} = vanishing_a / Z_H(zeta), the other chunks as filled"""
        sums, z_h, zeta_n = self.vanishing_sums()
        m0 = self.solve_chunk
        for a in range(self.shape.nc):
            want = emul(sums[a], einv(z_h))
            rest = (0, 0)
            for m in range(DEG):
                if m != m0:
                    rest = eadd(rest, emul(epow(zeta_n, m), self.open[self.o_quot(a * DEG + m)]))
            self.open[self.o_quot(a * DEG + m0)] = emul(esub(want, rest), einv(epow(zeta_n, m0)))

    def openings(self):
        return np.array(self.open, np.uint64)

    # ---- FRI ----
    def fri_transcript(self, final):
        """the challenger after the openings, the FRI caps and the final polynomial: (state before the PoW witness, fri caps)"""
        s = self.shape
        ch = self.ch_openings.clone()
        ch.observe(self.openings())
        self.fri_alpha = tuple(ch.get_n(2))
        fri_caps = [eo.pattern(4 << CAP_HEIGHT, 13 * self.seed + 5 * r, 3 + r % 3).reshape(-1, 4) for r in range(s.n_rounds)]
        self.betas_fri = []
        for c in fri_caps:
            ch.observe(c)
            self.betas_fri.append(tuple(ch.get_n(2)))
        ch.observe(np.array(final, np.uint64))
        return ch, fri_caps

    def final_poly(self):
        """E pairs; for the zero / minus1 fills a constant polynomial from FOLD_TARGETS, so that the last fold lands on an edge value"""
        s = self.shape
        n_final = 1 << (s.log_n - sum(s.params.arity_bits[r] for r in range(s.n_rounds)))
        if self.fill != "walk":
            return [FOLD_TARGETS[self.seed % len(FOLD_TARGETS)]] + [(0, 0)] * (n_final - 1)
        return edge_walk(n_final, 5 * self.seed + 1, 3)

    def combine_initial(self, leaves, x):
        """fri_combine_initial at subgroup point x for the base-field leaves of the four oracles"""
        s, alpha = self.shape, self.fri_alpha
        allv = [int(v) for o in range(4) for v in leaves[o]]
        acc, red, ap = (0, 0), (0, 0), (1, 0)
        for j, v in enumerate(allv):
            acc = eadd(acc, emul(ap, base(v)))
            red = eadd(red, emul(ap, self.open[j]))
            ap = emul(ap, alpha)
        total = emul(esub(acc, red), einv(esub(base(x), self.zeta)))
        acc, red, ap = (0, 0), (0, 0), (1, 0)
        for c in range(s.nc):
            acc = eadd(acc, emul(ap, base(int(leaves[2][c]))))
            red = eadd(red, emul(ap, self.open[self.o_zs_next(c)]))
            ap = emul(ap, alpha)
        total = eadd(emul(total, ap), emul(esub(acc, red), einv(esub(base(x), self.zeta_next))))
        if s.mul_final_by_x:
            total = emul(total, base(x))
        return total

    def query(self, q, x_index, final, consistent):
        """the words of one query round: leaves and paths of the four oracles, then per round the folds and a path"""
        s = self.shape
        log_lde = s.log_n + RATE_BITS
        nsib0 = log_lde - CAP_HEIGHT
        leaves = [eo.pattern(s.ncols[o], 17 * q + 5 * o + self.seed, 1 + (q + o) % 5) for o in range(4)]
        words = []
        for o in range(4):
            words += [int(v) for v in leaves[o]] + [int(v) for v in eo.pattern(4 * nsib0, q + o, 7)]
        x = 7 * pow(eo.root_of_unity(log_lde), bitrev(x_index, log_lde), P) % P
        old = self.combine_initial(leaves, x) if consistent else None
        lg = log_lde
        for r in range(s.n_rounds):
            ab = int(s.params.arity_bits[r])
            arity = 1 << ab
            within = x_index & (arity - 1)
            evals = edge_walk(arity, 11 * q + 3 * r + self.seed, 1 + 2 * ((q + r) % 4))
            if consistent:
                evals[within] = old
                g = eo.root_of_unity(ab)
                start = x * pow(g, arity - bitrev(within, ab), P) % P
                xs = [start * pow(g, i, P) % P for i in range(arity)]
                beta = self.betas_fri[r]
                lag = []
                for i in range(arity):
                    num, den = (1, 0), 1
                    for j in range(arity):
                        if j != i:
                            num = emul(num, esub(beta, base(xs[j])))
                            den = den * (xs[i] - xs[j]) % P
                    lag.append(emul(num, base(pow(den, P - 2, P))))
                x_next = pow(x, arity, P)
                free = (within + 1) % arity
                if r == s.n_rounds - 1:   # the free slot: interpolation at beta == final_poly(x^arity)
                    target = (0, 0)
                    for c in reversed(final):
                        target = eadd(emul(target, base(x_next)), c)
                else:                     # an edge value, which the next round compares with its `within` slot word for word
                    target = FOLD_TARGETS[(q + r + self.seed) % len(FOLD_TARGETS)]
                rest = (0, 0)
                for i in range(arity):
                    if bitrev(i, ab) != free:
                        rest = eadd(rest, emul(lag[i], evals[bitrev(i, ab)]))
                evals[free] = emul(esub(target, rest), einv(lag[bitrev(free, ab)]))
                old = (0, 0)
                for i in range(arity):
                    old = eadd(old, emul(lag[i], evals[bitrev(i, ab)]))
                x = x_next
            lg -= ab
            words += [v for e in evals for v in e] + [int(v) for v in eo.pattern(4 * (lg - CAP_HEIGHT), 3 * q + r, 5)]
            x_index >>= ab
        return words

    def fri_words(self, pow_witness, final_serialised, final_solved=None, consistent=False, ch=None, fri_caps=None):
        """the flat FRI proof: queries at the indices the transcript gives for this PoW witness, FRI-consistent if asked (solved against
        final_solved, which defaults to the serialised final polynomial)"""
        s = self.shape
        if ch is None:
            ch, fri_caps = self.fri_transcript(final_serialised)
        ch = ch.clone()
        ch.observe([pow_witness])
        ch.get()
        lde = 1 << (s.log_n + RATE_BITS)
        words = [int(v) for c in fri_caps for v in c.reshape(-1)]
        for q in range(int(s.params.num_query_rounds)):
            words += self.query(q, ch.get() % lde, final_solved or final_serialised, consistent)
        words += [v for e in final_serialised for v in e] + [int(pow_witness)]
        fri = np.array(words, np.uint64)
        want = orc.lib().orc_fri_proof_words(orc.C.byref(s.params), s.log_n, (orc.C.c_size_t * 4)(*s.ncols), 4)
        assert fri.size == want, (fri.size, want)
        return fri

    def failing_pow(self, ch):
        """a canonical witness from E that the PoW check rejects in state ch"""
        for w in eo.E[1:] + list(range(3, 1000)):
            c = ch.clone()
            c.observe([w])
            if c.get() >> (64 - POW_BITS):
                return w
        raise AssertionError("no failing PoW witness")

    def forge(self):
        """-> {name: Forgery} for the classes and controls of the shape"""
        s = self.shape
        final = self.final_poly()
        ch, fri_caps = self.fri_transcript(final)
        op = self.openings()
        mk = lambda kind, fri, openings=op: Forgery(s, kind, self.caps, openings, fri, self.pis)
        w1 = self.failing_pow(ch)
        w2 = orc.pow_grind(ch, POW_BITS)
        out = {"F1": mk("F1", self.fri_words(w1, final, ch=ch, fri_caps=fri_caps)),
               "F2": mk("F2", self.fri_words(w2, final, ch=ch, fri_caps=fri_caps))}
        if s.n_rounds:
            f3 = self.fri_words(w2, final, consistent=True, ch=ch, fri_caps=fri_caps)
            out["F3"] = mk("F3", f3)
            bad = f3.copy()
            bad[-1] = w1
            out["pow_of_F1"] = mk("pow_of_F1", bad)
            bad = f3.copy()   # the first query's first fold word behind the caps and the initial leaves and paths
            at = s.n_rounds * (4 << CAP_HEIGHT) + sum(s.ncols) + 4 * 4 * (s.log_n + RATE_BITS - CAP_HEIGHT) + 2 * int(self.seed % 16)
            bad[at] = (int(bad[at]) + 1) % P
            out["fold+1"] = mk("fold+1", bad)
            k = self.seed % len(final)
            final_bad = list(final)
            final_bad[k] = ((final[k][0] + 1) % P, final[k][1])
            ch_b, caps_b = self.fri_transcript(final_bad)
            out["final+1"] = mk("final+1", self.fri_words(orc.pow_grind(ch_b, POW_BITS), final_bad, final_solved=final, consistent=True,
                                                           ch=ch_b, fri_caps=caps_b))
        else:
            bad = out["F2"].fri.copy()
            bad[-1] = w1
            out["pow_of_F1"] = mk("pow_of_F1", bad)
        if not s.fri_only:
            src = out["F3"] if "F3" in out else out["F2"]
            q_op = op.copy()
            j = self.o_quot(self.solve_chunk)
            q_op[j, 0] = (int(q_op[j, 0]) + 1) % P
            out["quotient+1"] = mk("quotient+1", src.fri, q_op)
        return out


# ---- the oracle's verdict on a forgery ----
def oracle_checks(f):
    """-> (vanishing identity holds (None for fri_only), the set of failed FRI checks {"pow", "fri", "merkle"}, PoW response)"""
    s = f.shape
    ch = orc.ChallengerState()
    ch.observe(s.digest)
    ch.observe(orc.hash_no_pad(f.pis))
    ch.observe(f.caps[0])
    betas, gammas = ch.get_n(s.nc), ch.get_n(s.nc)
    ch.observe(f.caps[1])
    alphas = ch.get_n(s.nc)
    ch.observe(f.caps[2])
    zeta = ch.get_ext()
    op = f.openings
    van = None
    if not s.fri_only:
        n_cs, n_w, n_z, n_q = s.ncols
        cs_z, w_z = op[:n_cs], op[n_cs:n_cs + n_w]
        zs_all, q_z, zs_next = op[n_cs + n_w:n_cs + n_w + n_z], op[n_cs + n_w + n_z:n_cs + n_w + n_z + n_q], op[n_cs + n_w + n_z + n_q:]
        gt = s.gates.terms_zeta(cs_z[:s.n_constants], w_z, orc.hash_no_pad(f.pis), alphas) if s.gates is not None else None
        van = orc.check_vanishing_at_zeta(w_z[:s.n_routed], cs_z[s.n_constants:s.n_constants + s.n_routed], zs_all[:s.nc], zs_next,
                                          zs_all[s.nc:], q_z, s.log_n, betas, gammas, alphas, zeta, gate_terms_zeta=gt)
    batches, _ = step_oracle.step_batches(s.ncols, s.nc, zeta, s.log_n)
    ch.observe(op)
    pre = ch.clone()
    total = sum(s.ncols)
    caps = [s.cap, f.caps[0], f.caps[1], f.caps[2]]
    checks = orc.verify_fri_checks(caps, s.ncols, batches, [op[:total], op[total:]], ch, s.params, s.log_n, f.fri)
    # the PoW response on its own (orc_verify_fri_checks' transcript up to the witness)
    pre.get_n(2)
    for r in range(s.n_rounds):
        pre.observe(f.fri[r * (4 << CAP_HEIGHT):(r + 1) * (4 << CAP_HEIGHT)])
        pre.get_n(2)
    n_final = 2 << (s.log_n - sum(s.params.arity_bits[r] for r in range(s.n_rounds)))
    pre.observe(f.fri[-1 - n_final:-1])
    pre.observe(f.fri[-1:])
    return van, checks, pre.get()


def expected_reason(van, checks, reasons):
    """the first failing check in the verifiers' order; reasons = (OK, VANISHING, POW, FRI, MERKLE)"""
    ok, vanishing, pow_, fri, merkle = reasons
    if van is False:
        return vanishing
    return pow_ if "pow" in checks else fri if "fri" in checks else merkle if "merkle" in checks else ok


# what each class and control must come to (the verifiers' reason codes by name)
NOMINAL = {"F1": "POW", "F2": "FRI", "F3": "MERKLE", "quotient+1": "VANISHING", "pow_of_F1": "POW", "fold+1": "FRI", "final+1": "FRI"}


# ---- the shapes both test files cover ----
ALL = ["noop", "constant", "public_input", "arithmetic", "base_sum", "poseidon", "poseidon_mds", "arithmetic_ext", "mul_ext", "reducing",
       "reducing_ext", ("random_access", 4), "exponentiation", "coset_interpolation"]   # tests/test_gpu_edge_operands.py
SMALL_VARIANTS = [("base_sum", 10, 3), ("random_access", 1), ("random_access", 2), ("random_access", 3), ("random_access", 5),
                  ("coset_interpolation", 2), ("coset_interpolation", 3), ("coset_interpolation", 5), ("constant", 1), ("reducing", 5),
                  ("reducing_ext", 1), ("exponentiation", 7), ("mul_ext", 2), ("arithmetic", 3)]
STEP_SPEC = ["noop", "constant", "public_input", "arithmetic", "base_sum", "poseidon"]   # circuitgen/step_circuit.py GATE_SPEC


def _name(v):
    return "_".join(str(x) for x in v) if isinstance(v, tuple) else v


def shapes():
    """-> [(name, constructor kwargs for Shape.of_gates / Shape)]: the gate demo set, every small variant, the step_n8 and cyclic_n8
    circuits' shapes, 1 to 4 challenges, one chunk / a ragged chunk / 80 routed wires, 0 to 3 FRI rounds, fri_only, the compat positions"""
    out = [("all_log7", dict(spec=ALL, log_n=7))]
    out += [("small_%s" % _name(v), dict(spec=[v, "noop"], log_n=6)) for v in SMALL_VARIANTS]
    out += [("step_n8", dict(spec=STEP_SPEC, log_n=9)), ("cyclic_n8", dict(spec=ALL, log_n=13))]
    out += [("nc%d" % nc, dict(spec=ALL, log_n=6, num_challenges=nc)) for nc in (1, 3, 4)]
    out += [("routed%d" % r, dict(spec=ALL, log_n=6, n_routed=r)) for r in (8, 17)]
    out += [("log%d" % lg, dict(spec=STEP_SPEC, log_n=lg)) for lg in (5, 13, 16)]
    out += [("fri_only_log10", dict(fri_only=True, log_n=10)), ("fri_only_log4", dict(fri_only=True, log_n=4))]
    out += [("mul_final_by_x", dict(spec=ALL, log_n=6, compat=dict(fri_mul_final_by_x=1))),
            ("no_pi_len_prefix", dict(spec=STEP_SPEC, log_n=6, compat=dict(bytes_pi_len_prefix=0)))]
    return out


FRI_ONLY_NCOLS = [9, 135, 20, 16]


def make_shape(name, kw, **over):
    """Shape of one shapes() entry (its gate spec in shape.spec, its compat switches in shape.compat_over); over: cap / digest / ncols
    of a real circuit"""
    import gates_oracle as go
    kw = dict(kw, **over)
    spec, compat = kw.pop("spec", None), kw.pop("compat", None)
    if compat is not None:
        kw["compat"] = orc.compat(**compat)
    if kw.pop("fri_only", False):
        ncols = kw.pop("ncols", FRI_ONLY_NCOLS)
        s = Shape(name, kw.pop("log_n"), ncols, 0, 0, kw.pop("num_challenges", 2), fri_only=True, **kw)
    else:
        kw.pop("ncols", None)
        s = Shape.of_gates(name, go.GateSet(spec), kw.pop("log_n"), **kw)
    s.spec, s.compat_over = spec, compat or {}
    return s


def forger_variants(seed):
    """(fill, solved quotient chunk) of forger number `seed` of a shape"""
    return [("walk", 0), ("walk", 7), ("zero", 0), ("minus1", 7)][seed % 4]
