"""The operand sets, class assertions and big-integer references of tests/closing_group_cases.py run through `tools/test_layers host`: the plain C
forms of the closing group of four partial rounds, of the permutation's head and of the row subsets of its last layer (csrc/poseidon.h).  No GPU:
this keeps the host forms under the same net as the device forms (tests/test_gpu_closing_group.py) and proves the operand sets, the peak
records and the references before they are used on a device.  The generator's own table of bounds is checked here as well."""
import json
import os

import pytest

import closing_group_cases as cc
import layer_cases as lc


@pytest.fixture
def run(tmp_path):
    return lc.layer_runner(tmp_path, host=True)


def test_generated_bounds_leave_fold96_its_room():
    """every accumulator of the closing group and fold96's T below 2^64 (in fact below 2^62), while one accumulator for a row of M^4 itself would
    not be; the trimming word of the heaviest row costs nothing (N = 0 there), so the peak records reach the bounds exactly"""
    for name, lo, hi, t in cc.BOUNDS:
        assert lo < 1 << 62 and hi < 1 << 62 and t < 1 << 62, name
    assert max(sum(r) for r in cc.M4) * lc.M32 >= 1 << 64
    assert cc.M4_REST[cc.ROW][cc.FREE] == 0
    assert all(min(r) == 0 and max(r) < 1 << 25 for r in cc.M4_REST)
    assert all(cc.M4[i][j] == cc.M4_REST[i][j] + cc.M4_BASE[i] for i in range(12) for j in range(12))


@pytest.mark.parametrize("name", ["table", "ones"])
def test_host_closing_group_at_the_accumulator_bounds(run, name):
    cc.check_closing_group(run, cc.CLOSING if name == "table" else cc.ONES, name)


def test_host_closing_group_equals_the_seventh_group_and_round_25(run):
    cc.check_tail(run)


def test_host_head_and_row_subsets_equal_the_permutation(run):
    kats = json.load(open(os.path.join(lc.ROOT, "tests", "golden", "poseidon_kat.json")))["kats"]
    cc.check_head_and_rows(run, kats)
