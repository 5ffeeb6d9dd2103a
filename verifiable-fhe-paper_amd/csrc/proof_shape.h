// The shape of a step proof of one circuit, stated once: which circuit descriptions are refused (make_proof_shape), where every word of a
// proof sits in the verifier's arrays (ProofShape) and in which order the words and the Merkle-path length bytes are serialised
// (walk_step_proof: ProofWithPublicInputs::to_bytes of plonky2 0.2.0 util/serialization, without the public-input tail).  The serialiser
// (prover.hip), the parser and the host verifier (verifier.hip) and the device verifier (verify_batch.hip) all read it from here.  Host only;
// the struct itself is plain data and travels to kernels by value.
#pragma once
#include <string>

#include "host/plonky2_mirror.h"
#include "kernels.h"

namespace vpbs {
constexpr unsigned SHAPE_ROUNDS_MAX = 8;   // FRI reduction rounds (log_n + rate_bits <= 24 with arity 16: at most 5)

// A proof's words in the unified order caps [3][cap] | openings | fri; the openings are [constants_sigmas | wires | zs_partial_products |
// quotient | zs_next][2], the FRI words are round caps | nq query records | final polynomial | PoW witness.
struct ProofShape {
    u32 ncols[4];                 // columns of the four oracles: constants_sigmas, wires, zs_partial_products, quotient
    u32 n_constants, n_routed, deg, num_selectors, n_gates;
    u32 cap_words, cap_height, nc, total_cols, n_open_words;
    u32 log_n, log_lde, rate_bits, pow_bits, nq, n_rounds, final_len;
    u32 ab[SHAPE_ROUNDS_MAX], nsib_r[SHAPE_ROUNDS_MAX], off_r[SHAPE_ROUNDS_MAX];   // per reduction round: arity bits, path length, offset in a query record
    u32 off_o[4], nsib0;          // the initial oracles' leaves in a query record, and their path length
    u32 query_words, o_queries;   // words of one query record; the first record's offset in the FRI words
    u32 fri_total;                // FRI words, the PoW witness (the last one) included
    u32 o_open, o_fri, n_fixed;   // unified order: where the openings and the FRI words start, and the word count
    u32 fixed_len;                // serialised bytes up to and including the PoW witness
    int pi_prefix, fri_only, mul_final_by_x;   // compat.bytes_pi_len_prefix, vpbs_verify_inputs.fri_only, compat.fri_mul_final_by_x
};

// What the caller is going to do with the shape: each entry point refuses what it needs to hold, no more.
//   SHAPE_PARSE   walking the serialised bytes (vpbs_step_proof_from_bytes / to_bytes): n_constants within the constants/sigmas columns
//   SHAPE_VERIFY  checking a proof (vpbs_verify_step): at least one challenge, and without fri_only the permutation argument's column
//                 counts and the gates.  A shape made for SHAPE_VERIFY alone is not meant to be walked.
// Both refuse rate_bits > 3, cap_height > 8, log_n = 0, an LDE above 2^24, more challenges than Z columns and a cap taller than a tree.
// Both also refuse what the struct cannot hold: more than SHAPE_ROUNDS_MAX reduction rounds (none of the shapes above has more than 5) and
// a proof of 2^32 bytes or more (its offsets are 32 bits wide; before the struct existed only the device verifier had this limit).
enum : unsigned { SHAPE_PARSE = 1, SHAPE_VERIFY = 2 };

// -> true and the shape, or false and in *why (if given) the reason the circuit description is refused.  more_limits() -> NULL or a reason:
// a caller's own limits (the device verifier's), asked where that caller has always asked them, behind the general shape checks.
template <class MoreLimits> bool make_proof_shape(const vpbs_verify_inputs& in, const vpbs_compat& compat, unsigned needs, ProofShape& s, std::string* why,
                                                  MoreLimits&& more_limits) {
    auto refuse = [&](const std::string& m) {
        if (why) *why = m;
        return false;
    };
    if ((needs & SHAPE_PARSE) && in.n_constants > in.n_constants_sigmas) return refuse("malformed circuit description");
    if (in.num_challenges > in.n_zs_partial_products) return refuse("malformed circuit description");
    if (in.rate_bits > 3 || in.cap_height > 8 || in.log_n == 0 || in.log_n + in.rate_bits > 24 || ((needs & SHAPE_VERIFY) && in.num_challenges == 0))
        return refuse("malformed circuit description (log_n, rate_bits, cap_height, num_challenges)");
    if (const char* m = more_limits()) return refuse(m);
    const bool has_gates = in.gates && in.n_gates;
    if ((needs & SHAPE_VERIFY) && !in.fri_only) {
        const unsigned deg = in.quotient_degree_factor;
        if (deg == 0 || in.n_routed == 0 || in.n_routed > in.n_wires || in.n_constants + in.n_routed > in.n_constants_sigmas ||
            in.n_zs_partial_products != in.num_challenges * ((in.n_routed + deg - 1) / deg) ||
            in.n_quotient != (in.num_challenges << in.rate_bits))
            return refuse("malformed circuit description (permutation argument shape)");
        if (has_gates) {
            if (in.num_selectors > in.n_constants) return refuse("more selectors than constants columns");
            try {
                validate_gates(in.gates, in.n_gates, in.num_selectors, in.n_constants, in.n_wires);
            } catch (const DeviceError& e) {
                return refuse(e.what);
            }
        }
    }
    const plonky2::FriParams fp = plonky2::FriParams::standard(in.log_n, in.rate_bits, in.cap_height);
    if (!fp.caps_fit()) return refuse("cap taller than a Merkle tree of the proof");
    if (fp.reduction_arity_bits.size() > SHAPE_ROUNDS_MAX) return refuse("too many FRI rounds");

    s = ProofShape{};
    s.ncols[0] = in.n_constants_sigmas;
    s.ncols[1] = in.n_wires;
    s.ncols[2] = in.n_zs_partial_products;
    s.ncols[3] = in.n_quotient;
    s.n_constants = in.n_constants;
    s.n_routed = in.n_routed;
    s.deg = in.quotient_degree_factor;
    s.num_selectors = has_gates ? in.num_selectors : 0;
    s.n_gates = (!in.fri_only && has_gates) ? in.n_gates : 0;
    s.cap_words = 4u << in.cap_height;
    s.cap_height = in.cap_height;
    s.nc = in.num_challenges;
    s.log_n = in.log_n;
    s.log_lde = fp.lde_bits();
    s.rate_bits = in.rate_bits;
    s.pow_bits = fp.config.proof_of_work_bits;
    s.nq = fp.config.num_query_rounds;
    s.n_rounds = (u32)fp.reduction_arity_bits.size();
    s.final_len = 1u << fp.final_poly_bits();
    s.pi_prefix = compat.bytes_pi_len_prefix != 0;
    s.fri_only = in.fri_only != 0;
    s.mul_final_by_x = compat.fri_mul_final_by_x != 0;
    // a query record: for each of the four oracles leaf | path, then for each reduction round the coset's evaluations | path
    s.nsib0 = s.log_lde - s.cap_height;
    u64 total_cols = 0, at = 0;
    for (int o = 0; o < 4; ++o) {
        total_cols += s.ncols[o];
        s.off_o[o] = (u32)at;
        at += (u64)s.ncols[o] + 4 * s.nsib0;
    }
    unsigned lg = s.log_lde;
    for (u32 r = 0; r < s.n_rounds; ++r) {
        s.ab[r] = fp.reduction_arity_bits[r];
        lg -= s.ab[r];
        s.nsib_r[r] = lg - s.cap_height;
        s.off_r[r] = (u32)at;
        at += (2u << s.ab[r]) + 4 * s.nsib_r[r];
    }
    const u64 o_queries = (u64)s.n_rounds * s.cap_words, fri_total = o_queries + s.nq * at + 2 * s.final_len + 1;
    const u64 n_open_words = 2 * (total_cols + s.nc), n_fixed = 3 * (u64)s.cap_words + n_open_words + fri_total;
    const u64 fixed_len = 8 * n_fixed + (u64)s.nq * (4 + s.n_rounds);   // one length byte per Merkle path
    if (fixed_len > 0xFFFFFFF0u) return refuse("proof larger than 2^32 bytes");
    s.total_cols = (u32)total_cols;
    s.n_open_words = (u32)n_open_words;
    s.query_words = (u32)at;
    s.o_queries = (u32)o_queries;
    s.fri_total = (u32)fri_total;
    s.o_open = 3 * s.cap_words;
    s.o_fri = s.o_open + s.n_open_words;
    s.n_fixed = (u32)n_fixed;
    s.fixed_len = (u32)fixed_len;
    if (why) why->clear();
    return true;
}
inline bool make_proof_shape(const vpbs_verify_inputs& in, const vpbs_compat& compat, unsigned needs, ProofShape& s) {
    return make_proof_shape(in, compat, needs, s, nullptr, []() -> const char* { return nullptr; });
}
inline vpbs_compat compat_of(const vpbs_verify_inputs& in) {   // the switch table of include/vpbs_prover.h (NULL = plonky2 0.2.0 as restated)
    vpbs_compat c;
    vpbs_compat_default(&c);
    if (in.compat) c = *in.compat;
    return c;
}

// Visits a serialised proof in byte order, up to and including the PoW witness (the public-input tail is the caller's):
//   v.words(dest_word, count, pow)  `count` little-endian u64 that go to the unified order from dest_word on (never across two of caps /
//                                   openings / fri); pow: the one word that is a plain u64, not a field element
//   v.length_byte(nsib)             the length byte in front of a Merkle path of nsib siblings
template <class V> void walk_step_proof(const ProofShape& s, V&& v) {
    v.words(0, 3 * s.cap_words, false);   // wires_cap, plonk_zs_partial_products_cap, quotient_polys_cap
    // OpeningSet field order: constants, plonk_sigmas, wires, plonk_zs, plonk_zs_next, partial_products, quotient_polys, lookup_zs (empty),
    // lookup_zs_next (empty); the arrays hold [cs | wires | zs_pp | quotient | zs_next]
    const u32 cs = s.o_open, wires = cs + 2 * s.ncols[0], zs_pp = wires + 2 * s.ncols[1], quot = zs_pp + 2 * s.ncols[2], zs_next = quot + 2 * s.ncols[3];
    v.words(cs, 2 * s.ncols[0], false);
    v.words(wires, 2 * s.ncols[1], false);
    v.words(zs_pp, 2 * s.nc, false);
    v.words(zs_next, 2 * s.nc, false);
    v.words(zs_pp + 2 * s.nc, 2 * (s.ncols[2] - s.nc), false);
    v.words(quot, 2 * s.ncols[3], false);
    // FriProof: commit-phase caps, query rounds, final polynomial, PoW witness
    v.words(s.o_fri, s.n_rounds * s.cap_words, false);
    for (u32 q = 0; q < s.nq; ++q) {
        const u32 qw = s.o_fri + s.o_queries + q * s.query_words;
        for (int o = 0; o < 4; ++o) {
            v.words(qw + s.off_o[o], s.ncols[o], false);
            v.length_byte(s.nsib0);
            v.words(qw + s.off_o[o] + s.ncols[o], 4 * s.nsib0, false);
        }
        for (u32 r = 0; r < s.n_rounds; ++r) {
            v.words(qw + s.off_r[r], 2u << s.ab[r], false);
            v.length_byte(s.nsib_r[r]);
            v.words(qw + s.off_r[r] + (2u << s.ab[r]), 4 * s.nsib_r[r], false);
        }
    }
    v.words(s.n_fixed - 1 - 2 * s.final_len, 2 * s.final_len, false);
    v.words(s.n_fixed - 1, 1, true);
}

// the three arrays of vpbs_verify_step behind the unified order
template <class T> struct ProofArrays {
    T *caps, *openings, *fri;
    T* at(const ProofShape& s, u32 word) const { return word < s.o_open ? caps + word : word < s.o_fri ? openings + (word - s.o_open) : fri + (word - s.o_fri); }
};
}  // namespace vpbs
