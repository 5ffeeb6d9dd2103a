"""GPU tests (-m gpu) of the hashing permutation's closing group of four partial rounds (closing_group4_core / closing_row / halves_sum of
csrc/poseidon.h) at the operands where its accumulators peak, of its equality with the seventh group of three + round 25, and of the permutation's
head with the row subsets of its last layer.  tools/test_layers (built by __graft_entry__.build()) runs the device forms; element i is thread i of
256-thread blocks, so elements [64 k, 64 k + 64) are one wave.  Operands, host model, class assertions and the big-integer reference are those of
tests/closing_group_cases.py, which tests/test_closing_group_cpu.py runs through the host forms of the same header."""
import json
import os

import pytest

import closing_group_cases as cc
import layer_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture
def run(tmp_path):
    return lc.layer_runner(tmp_path, host=False)


@pytest.mark.parametrize("name", ["table", "ones"])
def test_closing_group_at_the_accumulator_bounds(run, name):
    """the plain form and the form with steered S-box inputs, under the table's constants and under k = 2^64 - 1: random wires, the computed values
    as wires, d2 = d3 = d4 in {0, 1, p - 1, 2^32 - 1, 2^63} in uniform and in mixed waves, and the records that put the heaviest row's acc_lo and
    acc_hi at the generator's largest values"""
    cc.check_closing_group(run, cc.CLOSING if name == "table" else cc.ONES, name)


def test_closing_group_equals_the_seventh_group_and_round_25(run):
    cc.check_tail(run)


def test_head_and_row_subsets_equal_the_permutation(run):
    kats = json.load(open(os.path.join(lc.ROOT, "tests", "golden", "poseidon_kat.json")))["kats"]
    cc.check_head_and_rows(run, kats)
