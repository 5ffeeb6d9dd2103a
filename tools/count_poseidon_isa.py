#!/usr/bin/env python3
"""Dynamic VALU-instruction count of the product Poseidon permutation on gfx950 (the number quoted in DESIGN.md / bench.py).

Compiles a one-permutation-per-lane kernel to ISA, counts VALU instructions per loop body and multiplies by the trip
counts (4 + 3 full rounds in loops, 6 fused partial groups of three; the closing group of four, the last round's S-boxes and
the last MDS layer stand outside the loops).  Needs hipcc only (no GPU).

Two forms are counted: the whole permutation (poseidon::permute, all twelve rows of the last MDS layer) and the HASHING
permutation, the one a sponge runs between two full blocks (the path poseidon::permute_sponge takes there: the head and
rows 8..11 of the last layer only; practically every permutation of a step proof) -- the same harness, so the
difference is the eight skipped rows.

Besides the plain sum (what bench.py's constant and the SQ_INSTS_VALU counter mean) the count is split by issue rate, as measured by
tools/microbench_valu2.hip (profiles/r07_microbench_valu2.txt, one SIMD with 4 waves): FULL-rate instructions take ~2.5 cycles per wave64
(v_mov_b32, v_add_u32, the two-operand logic and 32-bit shifts), everything else ~4.2-4.6 (v_mad_u64_u32, every carry add, v_cndmask, the
three-operand and 64-bit forms) -- priced here at 4.4 and 2.5."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "verifiable-fhe-paper_amd", "csrc")
SRC = r'''
#include "poseidon.h"
using gl::u64;
__global__ void __launch_bounds__(256) permute_batch_kernel(u64* states, size_t n) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    u64 s[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = states[12 * i + k];
    PERMUTE;
#pragma unroll
    for (int k = 0; k < 12; ++k) states[12 * i + k] = s[k];
}
'''
# (the hashing form canonicalises and stores its eight unwritten words too: the harness is for counting, and equal but for the rows)
FORMS = (("whole permutation", "poseidon::permute(s)"),
         ("hashing permutation", "poseidon::permute_head(s); poseidon::last_rows<8, 4>(s, poseidon::head_halves(s)); "
                                 "for (int k = 0; k < 12; ++k) s[k] = gl::canon(s[k])"))
TRIPS = (4, 6, 3)


FULL_RATE = re.compile(r"^\s+v_(mov_b32|add_u32|sub_u32|subrev_u32|xor_b32|and_b32|or_b32|not_b32|lshlrev_b32|lshrrev_b32|ashrrev_i32)(_e32)?\s")
HALF_CYCLES, FULL_CYCLES = 4.4, 2.5


def count(seg):
    """(VALU instructions, full-rate ones among them)"""
    valu = [x for x in seg if re.match(r"^\s+v_", x)]
    return len(valu), sum(1 for x in valu if FULL_RATE.match(x))


def measure(name, call):
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "t.hip"), os.path.join(d, "t.s")
        open(src, "w").write(SRC.replace("PERMUTE", call))
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, "-S", "--cuda-device-only", src, "-o", out],
                              stderr=subprocess.DEVNULL)
        # -S does not ASSEMBLE inline asm: an operand the assembler rejects (gfx950: VGPR pairs must be 64-bit aligned) only shows with -c
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, "-c", "--cuda-device-only", src, "-o",
                               os.path.join(d, "t.o")], stderr=subprocess.DEVNULL)
        lines = open(out).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z.*permute_batch_kernel.*:", l))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    body = lines[start:end]
    # the practically-never-taken second corrections of the asm arithmetic (gl.h: .Lgl_* labels): skipped by a forward wave-level branch --
    # not part of the dynamic count
    kept, skip_to, rare = [], None, 0
    for l in body:
        if skip_to is not None:
            if l.strip().startswith(skip_to + ":"):
                skip_to = None
            elif re.match(r"^\s+v_", l):
                rare += 1
            continue
        m = re.match(r"^\s+s_cbranch_\w+\s+(\.Lgl_\w+)", l)
        if m:
            skip_to = m.group(1)
            continue
        kept.append(l)
    print("VALU instructions behind never-taken forward branches (excluded):", rare)
    body = kept
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    loops = []
    for i, l in enumerate(body):
        m = re.match(r"^\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            seg = body[labels[m.group(1)]:i]
            loops.append(count(seg))
    total_static, total_full = count(body)
    print("static VALU instructions:", total_static, " loop bodies:", [n for n, _ in loops])
    if len(loops) == 3:
        in_loops = sum(n for n, _ in loops)
        rest = total_static - in_loops   # first constant layer, the plain partial round, the last round, canonicalisation, load/store
        dyn = sum(k * n for k, (n, _) in zip(TRIPS, loops)) + rest
        prefix = "" if name == "whole permutation" else name + ": "
        print("%sdynamic VALU instructions per permutation ~ %d  (%s + %d)" % (prefix, dyn, " + ".join("%d x %d" % (k, n) for k, (n, _) in zip(TRIPS, loops)), rest))
        full = sum(k * f for k, (_, f) in zip(TRIPS, loops)) + (total_full - sum(f for _, f in loops))
        half = dyn - full
        print("%sby issue rate: %d half-rate + %d full-rate;  cycle-weighted ~ %d SIMD cycles per wave64 permutation (%.1f / %.1f cycles)"
              % (prefix, half, full, round(half * HALF_CYCLES + full * FULL_CYCLES), HALF_CYCLES, FULL_CYCLES))
        return dyn
    return None


def main():
    counts = {}
    for name, call in FORMS:
        print("--", name, "--")
        counts[name] = measure(name, call)
    if all(counts.values()):
        print("the hashing permutation runs %d VALU instructions fewer than the whole one" % (counts["whole permutation"] - counts["hashing permutation"]))


if __name__ == "__main__":
    main()
