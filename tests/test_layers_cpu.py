"""The operand sets, class assertions and big-integer references of the layer tests (tests/layer_cases.py) run through `tools/test_layers host`:
the plain C forms of csrc/poseidon.h (mds_add_const, partial_group3 and both forms of partial_group3_core) and of gl::LazyAcc (csrc/gl.h).
No GPU: this keeps the headers' host forms under the same net as the device forms (tests/test_gpu_layers.py) and proves the operand sets and
references before they are used on a device."""
import pytest

import layer_cases as lc


@pytest.fixture
def run(tmp_path):
    return lc.layer_runner(tmp_path, host=True)


def test_host_mds_layer_at_the_accumulator_bounds(run):
    lc.check_mds(run)


@pytest.mark.parametrize("g", range(7))
def test_host_fused_group_in_three_forms(run, g):
    lc.check_group(run, g)


def test_host_lazy_accumulator_vector_form(run):
    lc.check_lazy_vector(run)


def test_host_lazy_accumulator_scalar_form(run):
    lc.check_lazy_scalar(run)


def test_host_lazy_accumulator_reduce_on_constructed_states(run):
    lc.check_lazy_reduce(run)
