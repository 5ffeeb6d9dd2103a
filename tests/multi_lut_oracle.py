"""Restatement of multi-output lookup gates (TEST INFRASTRUCTURE): the snap, sample extraction at a coefficient, the packed test
vector, the wire numbering of a program whose gates have several outputs, and its evaluation as the composition snap -> Bootstrapper.run ->
extract_at in Python integers.  Built on tfhe_oracle, pbs_batch_oracle, lwe_client_oracle and program_oracle; nothing here calls
vpbs_lwe_snap, vpbs_lwe_extract_at, vpbs_lut_testv_multi or vpbs_program_*.

A gate is (terms, const, lut) or (terms, const, lut, log_slots, outputs); the short form is (.., 0, 1)."""
import numpy as np

import lwe_client_oracle as LC
import pbs_batch_oracle as B
import program_oracle as O
import tfhe_oracle as T  # noqa: F401 -- the ring and the keys of the callers

P = O.P


def mod_switch(w, log_n):
    """pb_mod_switch (csrc/pbs_chain.h): the top log2(2N) bits of the raw word, rounded with the next bit -> [0, 2N]"""
    L = log_n + 1
    return (w >> (64 - L)) + ((w >> (64 - L - 1)) & 1)


def snap_r(w, log_n, theta):
    """the rounded quotient r of the definition (theta >= 1)"""
    t = 64 - (log_n + 1) + theta
    w %= P
    return (w >> t) + ((w >> (t - 1)) & 1), t


def snap(w, log_n, theta):
    w = int(w) % P
    if theta == 0:
        return w
    r, t = snap_r(w, log_n, theta)
    return (r << t) % (1 << 64)


def snap_words(words, log_n, theta):
    a = np.asarray(words, np.uint64)
    return np.array([snap(int(v), log_n, theta) for v in a.reshape(-1)], np.uint64).reshape(a.shape)


def extract_at(ct, n_lwe, j):
    """ct: K polynomials (lists); over each mask polynomial a, full[c] = a[j - c] for c <= j, else -a[N + j - c]; then body[j]"""
    n = len(ct[0])
    full = []
    for a in ct[:-1]:
        full += [int(a[j - c]) if c <= j else (P - int(a[n + j - c])) % P for c in range(n)]
    assert n_lwe <= len(full)
    return full[:n_lwe] + [int(ct[-1][j])]


def lut_testv_multi(n, p, tables, delta):
    """testv[q s + j] = T_j[q s], T_j = lut_testv(table j)"""
    s = len(tables)
    Ts = [LC.lut_testv(n, p, t, delta) for t in tables]
    return [Ts[i % s][i - i % s] for i in range(n)]


def norm(gates):
    return [tuple(g) if len(g) == 5 else tuple(g) + (0, 1) for g in gates]


def out_first(gates):
    first = [0]
    for g in norm(gates):
        first.append(first[-1] + g[4])
    return first


def csr(gates):
    d = O.csr([g[:3] for g in gates])
    d["gate_log_slots"] = np.array([g[3] for g in norm(gates)], np.uint32)
    d["gate_outputs"] = np.array([g[4] for g in norm(gates)], np.uint32)
    return d


def gate_of_wire(n_inputs, gates):
    """wire -> (gate, j), inputs -> None"""
    m = [None] * n_inputs
    for g, gt in enumerate(norm(gates)):
        m += [(g, j) for j in range(gt[4])]
    return m


def levels(n_inputs, gates):
    owner = gate_of_wire(n_inputs, gates)
    lv = []
    for terms, *_ in gates:
        lv.append(1 + max([0] + [lv[owner[s][0]] for s, _ in terms if s >= n_inputs]))
    return lv, max([0] + lv)


def gate_input(wires, gate, words, log_n):
    terms, const, _, theta, _ = gate
    return [snap(v, log_n, theta) for v in O.combine(wires, terms, const, words)]


def gate_inputs(n_inputs, gates, wires, words, log_n):
    """the input ciphertext of every gate from a complete wire table (what a verifier recomputes)"""
    return np.array([gate_input(wires, g, words, log_n) for g in norm(gates)], np.uint64).reshape(len(gates), words)


def wires_of(inputs, gates, out_cts, n_lwe):
    """inputs | the extraction of coefficient j of every gate's output GLWE, j below the gate's outputs"""
    rows = [[int(v) for v in w] for w in np.asarray(inputs)]
    for g, o in zip(norm(gates), out_cts):
        rows += [extract_at(B.glwe_list(o), n_lwe, j) for j in range(g[4])]
    return np.array(rows, np.uint64).reshape(len(rows), n_lwe + 1)


def evaluate(bootstrapper, n_inputs, gates, inputs, testvs):
    """the composition: per level, combine and snap on the host, one Bootstrapper.run (in chunks of its max_batch), extract_at on the host
    -> (wires [n_inputs + sum outputs][n + 1], gate_cts [n_gates][n + 1], out_cts [n_gates][K][N])"""
    bs, G = bootstrapper, norm(gates)
    inputs, testvs = np.asarray(inputs, np.uint64), np.asarray(testvs, np.uint64)
    words, log_n = bs.n_lwe + 1, bs.N.bit_length() - 1
    first = out_first(G)
    lv, n_levels = levels(n_inputs, G)
    wires = np.zeros((n_inputs + first[-1], words), np.uint64)
    wires[:n_inputs] = inputs
    gate_cts = np.zeros((len(G), words), np.uint64)
    out_cts = np.zeros((len(G), bs.K, bs.N), np.uint64)
    for level in range(1, n_levels + 1):
        todo = [g for g in range(len(G)) if lv[g] == level]
        for g in todo:
            gate_cts[g] = np.array(gate_input(wires, G[g], words, log_n), np.uint64)
        for lo in range(0, len(todo), bs.max_batch):
            part = todo[lo:lo + bs.max_batch]
            out, _ = bs.run(gate_cts[part], testvs[[G[g][2] for g in part]])
            for k, g in enumerate(part):
                out_cts[g] = out[k]
                for j in range(G[g][4]):
                    wires[n_inputs + first[g] + j] = np.array(extract_at(B.glwe_list(out[k]), bs.n_lwe, j), np.uint64)
    return wires, gate_cts, out_cts
