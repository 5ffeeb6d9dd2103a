"""GPU tests (-m gpu) of the forms whose correctness rests on an integer that never overflows, at the operands where that integer peaks:
poseidon::mds_add_const / mds_row and partial_group3_core / group_row (csrc/poseidon.h) called layer by layer on states and constants that no
whole permutation produces (all-ones halves, constants on both sides of the 58-bit split, steered d2 / d3), fold96 over the range the fused group
rows hand it, gl::LazyAcc (csrc/gl.h) in every class of reduce()'s carries, and both shapes of the permutation on words >= p.
tools/test_layers and tools/test_reductions (built by __graft_entry__.build()) run the device forms on the operands they are handed; element i is
thread i of 256-thread blocks, so elements [64 k, 64 k + 64) are one wave.  Operands, host models, class assertions and the big-integer
reference are those of tests/layer_cases.py, which tests/test_layers_cpu.py runs through the host forms of the same headers."""
import json
import os

import numpy as np
import pytest

import layer_cases as lc
from layer_cases import M32, M64, P

pytestmark = pytest.mark.gpu


@pytest.fixture
def run(tmp_path):
    return lc.layer_runner(tmp_path, host=False)


def _run_reductions(mode, words, tmp_path):
    import __graft_entry__ as entry
    return lc.run_tool(entry.build_reduction_tool(), [mode], words, tmp_path, "REDUCTIONS_DONE")


def test_mds_layer_at_the_accumulator_bounds(run):
    """mds_add_const with nine constant sets (zero, 2^64 - 1, p - 1, both sides of the 58-bit split, the top six bits alone, rounds 1 and 26, a
    mix) and without constants, on uniform edge states, single extreme words in every position, alternating halves and 4 096 random states"""
    lc.check_mds(run)


@pytest.mark.parametrize("g", range(7))
def test_fused_group_in_three_forms(run, g):
    """partial_group3, the witness generator's form and the PoseidonGate form of group g: random wires, the computed values as wires, and wires
    steered to d2, d3 in {0, 1, p - 1, 2^32 - 1, 2^63}"""
    lc.check_group(run, g)


def test_fold96_over_the_range_of_the_group_rows(tmp_path):
    """fold96(acc_lo, acc_hi) = acc_lo + acc_hi 2^32 (mod p) where the fused group rows reach: the device form discards the carry of
    T = hi_hi (2^32 - 1) + acc_lo, and the model asserts T < 2^64 for every pair handed in"""
    pairs, lo_max, hi_max = lc.fold96_group_pairs()
    assert all(0 <= lo <= lo_max and 0 <= hi <= hi_max for lo, hi in pairs)
    assert (lo_max, hi_max) in pairs and (lo_max, 0) in pairs and (0, hi_max) in pairs

    def carries(lo, hi):
        t = (hi >> 32) * M32 + lo
        assert t <= M64, "T overflows"
        return ((t >> 32) + (hi & M32)) >> 32
    seen = [carries(lo, hi) for lo, hi in pairs]
    t_max = max((hi >> 32) * M32 + lo for lo, hi in pairs)
    assert t_max == (hi_max >> 32) * M32 + lo_max
    assert set(seen[:64]) == {1} and set(seen[64:128]) == {0} and set(seen[128:192]) == {0, 1} and set(seen[192:256]) == {0, 1}
    print("fold96 on the group rows' range: acc_lo <= 2^%.3f, acc_hi <= 2^%.3f, T <= 2^%.3f; %d of %d carry into the high word"
          % (np.log2(float(lo_max)), np.log2(float(hi_max)), np.log2(float(t_max)), sum(seen), len(seen)))
    assert sum(seen) >= 64 and len(seen) - sum(seen) >= 64
    got = _run_reductions("fold", [lo for lo, _ in pairs] + [hi for _, hi in pairs], tmp_path)
    bad, count = lc.mismatches(got, [(lo + (hi << 32)) % P for lo, hi in pairs])
    assert not count, (count, [(hex(pairs[i][0]), hex(pairs[i][1]), g, w) for i, g, w in bad])


def test_lazy_accumulator_vector_form(run):
    lc.check_lazy_vector(run)


def test_lazy_accumulator_scalar_form(run):
    lc.check_lazy_scalar(run)


def test_lazy_accumulator_reduce_on_constructed_states(run):
    lc.check_lazy_reduce(run)


def test_permutation_of_non_canonical_states_in_both_shapes(tmp_path):
    """"in: any residues" is the contract of permute and permute_wide: states of words >= p (every edge value uniform, draws from the edge
    values, the whole u64 range) through both device shapes and the host form equal the big-integer permutation of the words mod p"""
    kat = json.load(open(os.path.join(lc.ROOT, "tests", "golden", "poseidon_kat.json")))["kats"]
    states = np.concatenate([lc.u64([x for v in kat for x in v["input"]]).reshape(-1, 12), lc.noncanonical_states()])
    n = states.shape[0]
    assert (states[len(kat):] >= np.uint64(P)).any(axis=1).sum() >= 1000                  # six uniform edge states and nearly every draw from the edge values
    want = lc.permutation_reference(states)
    for i, v in enumerate(kat):
        assert [int(x) for x in want[i]] == [int(x) for x in v["output"]], i               # the reference itself against the stored KATs
    got = _run_reductions("perm", states, tmp_path)
    assert got.size == 36 * n
    for k, shape in enumerate(("permute", "permute_wide", "permute on the host")):
        bad, count = lc.mismatches(got[12 * n * k:12 * n * (k + 1)], want)
        assert not count, (shape, count, [(i // 12, i % 12, g, w) for i, g, w in bad])
