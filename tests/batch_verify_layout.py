"""Byte layout of a serialised step proof (ProofWithPublicInputs, as vpbs_step_proof_to_bytes writes it): where every word of each section
sits, the Merkle-path length bytes, the PoW witness and the public-input count.  A helper module of the batch-verifier tests, not a conftest;
it restates the walk of vpbs_step_proof_from_bytes from the FRI parameters, so a test can aim a corruption at one section."""


def fri_rounds(log_n, rate_bits=3, cap_height=4):
    """FriReductionStrategy::ConstantArityBits(4, 5): the arity bits of the reduction rounds"""
    d, rounds = log_n, []
    while d > 5 and d + rate_bits >= cap_height + 4:
        rounds.append(4)
        d -= 4
    return rounds, d


def proof_layout(ncols, log_n, n_constants, num_challenges=2, rate_bits=3, cap_height=4, num_queries=28):
    """-> {"words": [(section, byte offset)], "len_bytes": [offset], "pow": offset, "fixed_len": bytes before the public-input count}"""
    words, len_bytes = [], []
    pos = 0
    cap_words = 4 << cap_height
    n_cs, n_w, n_z, n_q = ncols
    nc = num_challenges

    def put(section, n):
        nonlocal pos
        for k in range(n):
            words.append((section, pos + 8 * k))
        pos += 8 * n

    def length_byte():
        nonlocal pos
        len_bytes.append(pos)
        pos += 1
    put("caps", 3 * cap_words)
    put("openings", 2 * (n_cs + n_w + 2 * nc + (n_z - nc)))   # constants/sigmas, wires, Z, Z(g zeta), partial products
    put("openings_quotient", 2 * n_q)
    rounds, final_bits = fri_rounds(log_n, rate_bits, cap_height)
    put("fri_caps", len(rounds) * cap_words)
    log_lde = log_n + rate_bits
    for _ in range(num_queries):
        for o in range(4):
            put("leaf", ncols[o])
            length_byte()
            put("sibling", 4 * (log_lde - cap_height))
        lg = log_lde
        for ab in rounds:
            lg -= ab
            put("fold", 2 << ab)
            length_byte()
            put("sibling", 4 * (lg - cap_height))
    put("final", 2 << final_bits)
    pow_at = pos
    pos += 8
    return {"words": words, "len_bytes": len_bytes, "pow": pow_at, "fixed_len": pos}
