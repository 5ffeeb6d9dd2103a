"""FRI, commitment and step-proof shapes away from the standard configuration (rate_bits 3, cap_height 4, arities [4, 4, ...]): the case
tables shared by the CPU leg (test_oracle_cpu.py, test_host_cpu.py) and the GPU leg (test_gpu_fri_shapes.py).  TEST INFRASTRUCTURE ONLY; no
GPU import, nothing of the product package.
"""

FRI_COLS = (4, 6, 3, 2)   # the fourth batch is committed from coefficients, the others from values


def standard_arities(log_n, rate_bits=3, cap_height=4):
    """FriReductionStrategy::ConstantArityBits(4, 5) of standard_recursion_config under a FriConfig of this rate and cap height: reduce by
    arity 16 while the degree stays above 2^5 and the round's tree stays at least as tall as the cap.  Neither library's
    *_fri_params_standard takes a rate or a cap, so this is the tests' own statement of the rule."""
    bits, d = [], log_n
    while d > 5 and d + rate_bits - 4 >= cap_height:
        bits.append(4)
        d -= 4
    return bits


# (log_n, rate_bits, cap_height, arity_bits).  Arity bits 0-4 only: 0 folds nothing, 1 gives a 4-word leaf (not hashed), 3 and 4 give leaves
# of two and four absorb blocks.  Arity bits >= 5 are out of scope -- the oracle verifier's interpolation buffers hold 16 points -- and the
# prover's behaviour there is left as it is.
FRI_SHAPES_BY_GROUP = {
    "mixed arities, standard rate/cap": [(8, 3, 4, [1, 2, 3]), (8, 3, 4, [3, 2]), (9, 3, 4, [2, 2, 2]), (7, 3, 4, [1]), (8, 3, 4, []),
                                         (8, 3, 4, [0, 4]), (8, 3, 4, [4, 0])],
    # the second: 4 + 8 = MAX_OPEN_TREES trees and SHAPE_ROUNDS_MAX rounds
    "many rounds": [(8, 3, 4, [1] * 7), (8, 3, 3, [1] * 8)],
    "other rate/cap": [(8, 1, 0, [4]), (8, 2, 2, [3, 1]), (8, 0, 0, [4]), (8, 3, 7, [4]), (8, 2, 1, [2, 3, 1]), (8, 1, 3, [3, 3])],
    # the first has a round tree of ONE leaf, which is its own cap
    "smallest trees": [(4, 0, 0, [4]), (4, 1, 0, [4])],
    # the last round tree is exactly its cap
    "trees that just fit": [(4, 3, 3, [2, 2]), (4, 3, 3, [4])],
}
FRI_SHAPES = [s for group in FRI_SHAPES_BY_GROUP.values() for s in group]

# columns of the four batches at log_n = 6, standard parameters: 63 = one combine group, 64 = the first grouped count, 65 = empty trailing
# groups, 241 = a ragged last group
POLY_COUNTS = [(20, 28, 10, 5), (20, 29, 10, 5), (20, 30, 10, 5), (120, 100, 16, 5)]
POLY_COUNT_LOG_N = 6

# num_query_rounds at log_n = 6, pow_bits = 2; 128 = MAX_QUERIES
QUERY_COUNTS = [1, 128]
QUERY_COUNT_LOG_N, QUERY_COUNT_POW_BITS = 6, 2

# (log_n, rate_bits, cap_height) -> reduction rounds by the standard rule; (6, 3, 4) is the control, cap 8 the largest make_proof_shape takes
STEP_SHAPES = [((6, 3, 4), 1), ((6, 1, 4), 0), ((6, 1, 0), 1), ((7, 2, 2), 1), ((8, 0, 0), 1), ((6, 3, 7), 0), ((9, 2, 0), 1), ((7, 3, 8), 0),
               ((6, 2, 5), 0)]
STEP_COLS = {"constants_sigmas": 5, "wires": 9, "zs_partial_products": 4, "quotient": 3}

# every distinct (rate_bits, cap_height) of the two tables, in table order
RATE_CAPS = list(dict.fromkeys([(r, c) for _, r, c, _ in FRI_SHAPES] + [(r, c) for (_, r, c), _ in STEP_SHAPES]))

# Parameter sets the library refuses as a whole (VPBS_ERR_INVALID; vpbs_fri_proof_words = 0): (name, log_n, overrides of the standard params)
REFUSED_SHAPES = [
    ("17 rounds", 6, {"arity_bits": [0] * 17}),
    ("arities exceed the degree", 6, {"arity_bits": [4, 4]}),
    ("round tree shorter than its cap", 6, {"arity_bits": [4, 2]}),
    ("13 trees", 10, {"arity_bits": [1] * 9}),
    ("129 query rounds", 6, {"num_query_rounds": 129}),
]


def shape_id(s):
    log_n, rate, cap, bits = s
    return "n%d-r%d-c%d-[%s]" % (log_n, rate, cap, ",".join(map(str, bits)))
