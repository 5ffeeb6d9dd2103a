"""TEST INFRASTRUCTURE (stand-in for the Rust circuit builder): the AGGREGATION circuits -- a binary tree of recursive verifiers that folds
the vPBS proofs of a batch into one proof.

Level-l circuit A_l (l >= 1): two proof slots of the inner shape S_{l-1} (S_0: the cyclic step circuit's shape; S_l: Shape(api, A_l.log_n,
4 + 68 l)), `verify_proof` (cyclic_circuit.py, plonky2's recursion/recursive_verifier.rs) on both under the verifier data vk_{l-1}, and

    public inputs = root [4] | vk_0 [68] | ... | vk_{l-1} [68]            (each vk: circuit digest, then the constants/sigmas cap: vk_words)
    root          = hash_no_pad(s_left || s_right)
    s             = l == 1: the slot's in-circuit public-input hash (the leaf statement)       l >= 2: the slot's public inputs [0:4]

The verifier data are public inputs, never constants: at l = 1 the leaf's own last 68 public inputs (the cyclic proof's verifier data) are
connected to vk_0, at l >= 2 the child's public inputs [4:] to vk_0 .. vk_{l-2}; vk_{l-1} is the one both slots are verified under.  The
final verifier fixes vk_d from outside and the public inputs fix every vk below it.
"""
import numpy as np

import cyclic_circuit as cc

VK_WORDS = 68


def level_n_pi(level):
    """public inputs of A_level: the root and the verifier data of every level below"""
    return 4 + VK_WORDS * level


class AggregateCircuit:
    """A_level over two proofs of `inner_shape`.  Targets (the PartialWitness order of .positions / .values): slot 0 proof | slot 0 public
    inputs | slot 1 proof | slot 1 public inputs | vk_0 .. vk_{level-1}."""

    def __init__(self, api, inner_shape, level, min_log_n=5):
        assert level >= 1
        S = inner_shape
        if level == 1:
            assert S.n_pi >= VK_WORDS, "a leaf carries its own verifier data in its last 68 public inputs"
        else:
            assert S.n_pi == level_n_pi(level - 1), "the inner shape is not that of level %d" % (level - 1)
        cb = cc.ExtBuilder()
        self.level, self.inner_shape = level, S
        self.proofs = [cb.virtuals(S.proof_words) for _ in range(2)]
        self.pis = [cb.virtuals(S.n_pi) for _ in range(2)]
        self.vks = [cb.virtuals(VK_WORDS) for _ in range(level)]
        top = self.vks[level - 1]
        below = [t for vk in self.vks[:level - 1] for t in vk]
        statements = []
        for proof, pis in zip(self.proofs, self.pis):
            out = cc.verify_proof(cb, S, proof, pis, top[:4], [top[4 + 4 * i:8 + 4 * i] for i in range(S.cap_len)])
            if level == 1:
                statements.append(out["pi_hash"])
                for a, b in zip(pis[S.n_pi - VK_WORDS:], top):
                    cb.connect(a, b)
            else:
                statements.append(pis[:4])
                for a, b in zip(pis[4:], below):
                    cb.connect(a, b)
        self.root = cb.hash_no_pad(statements[0] + statements[1])
        cb.register_public_inputs(self.root)
        for vk in self.vks:
            cb.register_public_inputs(vk)
        self.built = cb.build(api, min_log_n)
        self.shape = cc.Shape(api, self.built.log_n, level_n_pi(level))
        assert len(self.built.public_inputs) == self.shape.n_pi
        self.targets = self.proofs[0] + self.pis[0] + self.proofs[1] + self.pis[1] + [t for vk in self.vks for t in vk]
        self.positions = [self.built.pos(t) for t in self.targets]

    def values(self, flat0, pis0, flat1, pis1, vks):
        """the PartialWitness of one node in the order of .targets: the two children (flat proof words, public inputs) and vk_0 .. vk_{l-1}"""
        v = np.concatenate([np.asarray(flat0, np.uint64), np.asarray(pis0, np.uint64), np.asarray(flat1, np.uint64),
                            np.asarray(pis1, np.uint64)] + [np.asarray(vk, np.uint64).reshape(-1) for vk in vks])
        assert v.size == len(self.targets) and len(vks) == self.level
        return v

    def public_inputs(self, wires):
        return self.built.values(wires, self.built.public_inputs)


def tree_depth(count):
    """d = max(1, ceil(log2 count))"""
    assert count >= 1
    return max(1, (count - 1).bit_length())


def tree_root(statements, hash_no_pad):
    """the root over leaf statements (4 words each): pad to 2^d by repeating the last leaf, fold pairs with hash_no_pad(left || right)"""
    level = [[int(x) for x in s] for s in statements]
    d = tree_depth(len(level))
    level += [level[-1]] * ((1 << d) - len(level))
    for _ in range(d):
        level = [[int(x) for x in hash_no_pad(level[i] + level[i + 1])] for i in range(0, len(level), 2)]
    return level[0]
