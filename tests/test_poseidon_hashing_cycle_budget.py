"""CPU test (needs hipcc, no GPU): the issue-cycle budget of the HASHING permutation -- the one a sponge runs between two full blocks, practically
every permutation of a step proof -- as tools/count_poseidon_isa.py prices the compiled ISA (4.4 cycles per half-rate, 2.5 per full-rate wave64
instruction).  tests/test_poseidon_cycle_budget.py keeps the budget of the whole permutation as it was; this one is lower by what the hashing
kernels no longer compute: eight rows of the last MDS layer (8 x (24 multiply-adds + a fold of 4) = 224 instructions) and the difference between
a seventh group of three + the plain round 25 (674 multiply-adds, 26 folds) and the closing group of four (486 multiply-adds, 16 folds; the compiler
saves a few moves on top: 234 instructions in all)."""
import contextlib
import importlib.util
import io
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the whole permutation's budget, 54 150 (444 cycles above its 53 706), less 4.4 cycles for each of the 224 + 234 half-rate instructions removed:
# 54 150 - 2 015 = 52 135; the same 444 above the hashing form's 51 689 is 52 133 -- the smaller of the two
CYCLE_BUDGET = 52133
ROWS_SKIPPED = 8 * (24 + 4)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc is absent")
def test_cycle_weighted_count_of_the_hashing_permutation_stays_within_the_budget(monkeypatch):
    if shutil.which("hipcc") is None:
        monkeypatch.setenv("PATH", os.environ.get("PATH", "") + os.pathsep + "/opt/rocm/bin")
    spec = importlib.util.spec_from_file_location("count_poseidon_isa", os.path.join(ROOT, "tools", "count_poseidon_isa.py"))
    counter = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(counter)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        counter.main()
    text = out.getvalue()
    print(text)
    cycles = re.search(r"hashing permutation: .*cycle-weighted ~ (\d+) SIMD cycles per wave64 permutation", text)
    dynamic = re.search(r"hashing permutation: dynamic VALU instructions per permutation ~ (\d+)", text)
    whole = re.search(r"^dynamic VALU instructions per permutation ~ (\d+)", text, re.M)
    assert cycles and dynamic and whole, text
    assert int(cycles.group(1)) <= CYCLE_BUDGET, text
    assert 11800 < int(dynamic.group(1)) < 12300, text      # three loop bodies found, every trip count applied
    assert int(whole.group(1)) - int(dynamic.group(1)) == ROWS_SKIPPED, text    # the same harness: the two forms differ by the rows and by nothing else
