"""Restatement of a program of lookup gates (TEST INFRASTRUCTURE): validation, levelisation, the gate-input combination in Python integers
mod p, and evaluation as the composition a user had to write before api.Program existed -- one Bootstrapper.run per level on combinations
formed on the host.  Nothing here calls vpbs_program_*.

A program is (n_inputs, gates, n_luts); gates is a list of (terms=[(src, coef), ..], const, lut) in the caller's order; wire w < n_inputs is
input w, wire n_inputs + g the output of gate g."""
import numpy as np

P = 0xFFFFFFFF00000001


def csr(gates):
    """-> dict of the CSR arrays api.Program also accepts"""
    first = [0]
    for terms, _, _ in gates:
        first.append(first[-1] + len(terms))
    return dict(gate_first=np.array(first, np.uint64), term_src=np.array([s for g in gates for s, _ in g[0]], np.uint32),
                term_coef=np.array([c for g in gates for _, c in g[0]], np.uint64), gate_const=np.array([g[1] for g in gates], np.uint64),
                gate_lut=np.array([g[2] for g in gates], np.uint32))


def validate(n_inputs, gates, n_luts):
    """-> None, or (gate, rule) of the first violated rule in gate order"""
    for g, (terms, const, lut) in enumerate(gates):
        if lut >= n_luts:
            return g, "lut"
        if const >= P:
            return g, "const"
        for src, coef in terms:
            if src >= n_inputs + g:
                return g, "order"
            if coef >= P:
                return g, "coef"
    return None


def levels(n_inputs, gates):
    """inputs are level 0; a gate is 1 + the highest level among its sources; a gate without terms is level 1 -> (levels, number of levels)"""
    lv = []
    for terms, _, _ in gates:
        lv.append(1 + max([0] + [lv[s - n_inputs] for s, _ in terms if s >= n_inputs]))
    return lv, max([0] + lv)


def combine(wires, terms, const, words):
    """const * (0, .., 0, 1) + sum coef * wire[src], word by word, canonical"""
    out = [0] * words
    out[-1] = const % P
    for src, coef in terms:
        w = wires[src]
        for j in range(words):
            out[j] = (out[j] + coef * int(w[j])) % P
    return out


def gate_inputs(n_inputs, gates, wires, words):
    """the input ciphertext of every gate from a complete wire table (what a verifier recomputes)"""
    return np.array([combine(wires, terms, const, words) for terms, const, _ in gates], np.uint64).reshape(len(gates), words)


def evaluate(bootstrapper, n_inputs, gates, inputs, testvs):
    """the composition: per level one Bootstrapper.run (in chunks of its max_batch) on host combinations
    -> (wires [n_inputs + n_gates][n + 1], gate_cts [n_gates][n + 1], out_cts [n_gates][K][N])"""
    inputs, testvs = np.asarray(inputs, np.uint64), np.asarray(testvs, np.uint64)
    words = inputs.shape[1] if n_inputs else bootstrapper.n_lwe + 1
    n_gates = len(gates)
    lv, n_levels = levels(n_inputs, gates)
    wires = np.zeros((n_inputs + n_gates, words), np.uint64)
    wires[:n_inputs] = inputs
    gate_cts = np.zeros((n_gates, words), np.uint64)
    out_cts = np.zeros((n_gates, bootstrapper.K, bootstrapper.N), np.uint64)
    for level in range(1, n_levels + 1):
        todo = [g for g in range(n_gates) if lv[g] == level]
        for g in todo:
            gate_cts[g] = np.array(combine(wires, gates[g][0], gates[g][1], words), np.uint64)
        for lo in range(0, len(todo), bootstrapper.max_batch):
            part = todo[lo:lo + bootstrapper.max_batch]
            out, lwe = bootstrapper.run(gate_cts[part], testvs[[gates[g][2] for g in part]])
            for k, g in enumerate(part):
                out_cts[g], wires[n_inputs + g] = out[k], lwe[k]
    return wires, gate_cts, out_cts


def random_dag(rng, n_inputs, n_gates, n_luts, max_fan_in=4):
    """a seeded DAG in topological order with fan-in 0 .. max_fan_in, coefficients and constants anywhere in the field"""
    gates = []
    for g in range(n_gates):
        fan = int(rng.integers(0, max_fan_in + 1))
        terms = [(int(rng.integers(0, n_inputs + g)), int(rng.integers(0, P, dtype=np.uint64))) for _ in range(fan)] if n_inputs + g else []
        gates.append((terms, int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, n_luts))))
    return gates
