"""CPU test (needs hipcc, no GPU): the issue-cycle budget of one Poseidon permutation in the lane-per-permutation form, as tools/count_poseidon_isa.py
prices the compiled ISA (4.4 cycles per half-rate, 2.5 per full-rate wave64 instruction: profiles/r07_microbench_valu2.txt).  The hashing kernels are
bound by VALU issue and by nothing else, so this number is their time."""
import contextlib
import importlib.util
import io
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 56 689 cycles before the carry corrections became multiply-adds (round 7), minus 4.5 %: one half-rate instruction less in each of the 472 products
# and 206 folds of a permutation is 678 x 4.4 = 2 983 cycles = 5.26 %, with a margin for what the compiler moves
CYCLE_BUDGET = 54150


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc is absent")
def test_cycle_weighted_count_per_permutation_stays_within_the_budget(monkeypatch):
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
    cycles = re.search(r"cycle-weighted ~ (\d+) SIMD cycles per wave64 permutation", text)
    dynamic = re.search(r"dynamic VALU instructions per permutation ~ (\d+)", text)
    assert cycles and dynamic, text
    assert int(cycles.group(1)) <= CYCLE_BUDGET, text
    assert 12000 < int(dynamic.group(1)) < 13000, text      # three loop bodies found, every trip count applied
