// The arithmetic checks of a step proof, written once for the host verifier (verifier.hip) and the device verifier (verify_batch.hip):
// plonky2 0.2.0 plonk/vanishing_poly.rs `eval_vanishing_poly` (permutation part) with plonk/verifier.rs `verify_with_challenges`, and
// fri/verifier.rs `PrecomputedReducedOpenings` / `fri_combine_initial` / `compute_evaluation` / `fri_verifier_query_round` (without the
// Merkle paths).  Pointers in, one bool out; no heap and no array sized by the circuit, so a GPU lane runs them as they stand.
#pragma once
#include "gl.h"
#include "proof_shape.h"

namespace vpbs {
GL_HD gl::Ext ext_at(const u64* p, size_t i) { return gl::Ext{p[2 * i], p[2 * i + 1]}; }

// PrecomputedReducedOpenings: r0 = every polynomial at zeta, r1 = the Z polynomials at g * zeta, each reduced with the powers of fri_alpha
GL_HD void reduced_openings(const ProofShape& s, const u64* open, gl::Ext fri_alpha, gl::Ext& r0, gl::Ext& r1) {
    r0 = r1 = gl::ext(0);
    for (u32 j = s.total_cols; j-- > 0;) r0 = gl::add(gl::mul(r0, fri_alpha), ext_at(open, j));
    for (u32 j = s.nc; j-- > 0;) r1 = gl::add(gl::mul(r1, fri_alpha), ext_at(open, s.total_cols + j));
}

// what the vanishing identity needs of zeta alone, shared by every challenge: zeta^n, Z_H(zeta) = zeta^n - 1 and L_0(zeta)
struct ZetaTerms {
    gl::Ext zeta_n, z_h, l0;
};
GL_HD ZetaTerms zeta_terms(const ProofShape& s, gl::Ext zeta) {
    ZetaTerms t;
    t.zeta_n = zeta;
    for (unsigned k = 0; k < s.log_n; ++k) t.zeta_n = gl::mul(t.zeta_n, t.zeta_n);
    t.z_h = gl::sub(t.zeta_n, gl::ext(1));
    t.l0 = gl::mul(t.z_h, gl::inv(gl::mul(gl::sub(zeta, gl::ext(1)), (u64)1 << s.log_n)));
    return t;
}

// vanishing(zeta) == Z_H(zeta) t(zeta) for challenge a: reduce_with_powers over [L_0 (Z_c - 1)]_c | [check_partial_products]_c,chunk with
// alpha = alphas[a], the gate terms (already folded with alpha by the caller) multiplied in behind them: sum_t alpha^t term_t + alpha^T gate_term_a.
// betas_gammas: [betas [nc] | gammas [nc]], the order the transcript yields them, behind one pointer (two pointers cost a GPU lane two more
// registers).  gate_term_a() -> that gate term; it is asked for last, when the permutation terms are summed, so what a caller needs to produce it (the
// device: a walk over its per-gate partials) is not kept alive through them.  zt = zeta_terms(s, zeta): it depends on zeta alone, so the
// caller makes it once for all challenges.
template <class GateTerm>
GL_HD bool vanishing_holds(const ProofShape& s, const u64* open, unsigned a, u64 alpha, const u64* betas_gammas, gl::Ext zeta,
                           const ZetaTerms& zt, GateTerm&& gate_term_a) {
    using gl::Ext;
    const unsigned nc = s.nc, n_routed = s.n_routed, deg = s.deg;
    const unsigned n_chunks = (n_routed + deg - 1) / deg, num_prods = n_chunks - 1;
    const u64* cs_z = open;
    const u64* wires_z = cs_z + 2 * (size_t)s.ncols[0];
    const u64* zs_pp_z = wires_z + 2 * (size_t)s.ncols[1];
    const u64* quot_z = zs_pp_z + 2 * (size_t)s.ncols[2];
    const u64* zs_next_z = quot_z + 2 * (size_t)s.ncols[3];
    const u64* sig_z = cs_z + 2 * (size_t)s.n_constants;
    const u64* pps_z = zs_pp_z + 2 * (size_t)nc;
    const Ext one = gl::ext(1);
    Ext sum = gl::ext(0);
    u64 apow = 1;
    for (unsigned c = 0; c < nc; ++c) {
        sum = gl::add(sum, gl::mul(gl::mul(zt.l0, gl::sub(ext_at(zs_pp_z, c), one)), apow));
        apow = gl::mul(apow, alpha);
    }
    for (unsigned c = 0; c < nc; ++c) {
        const u64 beta = betas_gammas[c];
        const Ext g = gl::ext(betas_gammas[nc + c]);
        u64 k = 1;   // k_is[j] = GENERATOR^j, alongside the loop
        for (unsigned kk = 0; kk < n_chunks; ++kk) {
            Ext num = one, den = one;
            for (unsigned j = kk * deg; j < (kk + 1) * deg && j < n_routed; ++j) {
                const Ext wj = ext_at(wires_z, j);
                num = gl::mul(num, gl::add(gl::add(wj, gl::mul(zeta, gl::mul(beta, k))), g));
                den = gl::mul(den, gl::add(gl::add(wj, gl::mul(ext_at(sig_z, j), beta)), g));
                k = gl::mul(k, gl::GENERATOR);
            }
            const Ext prev = kk == 0 ? ext_at(zs_pp_z, c) : ext_at(pps_z, c * num_prods + kk - 1);
            const Ext next = kk == num_prods ? ext_at(zs_next_z, c) : ext_at(pps_z, c * num_prods + kk);
            sum = gl::add(sum, gl::mul(gl::sub(gl::mul(prev, num), gl::mul(next, den)), apow));   // check_partial_products
            apow = gl::mul(apow, alpha);
        }
    }
    const Ext acc = gl::add(sum, gl::mul(gate_term_a(), apow));
    const unsigned chunks_per = 1u << s.rate_bits;
    Ext q = gl::ext(0);
    for (unsigned m = chunks_per; m-- > 0;) q = gl::add(gl::mul(q, zt.zeta_n), ext_at(quot_z, a * chunks_per + m));
    return gl::eq(acc, gl::mul(zt.z_h, q));
}

// One FRI query without its Merkle paths: fri_combine_initial over the leaves of the record qw, then for every reduction round the
// consistency of the coset's evaluations with the value carried so far and compute_evaluation at the round's beta, then the final polynomial
// `fin` at the last point.  r0, r1: reduced_openings; fri_betas [n_rounds][2].
GL_HD bool fri_query_holds(const ProofShape& s, gl::Ext r0, gl::Ext r1, const u64* qw, const u64* fin, u32 x_index, gl::Ext zeta, gl::Ext fri_alpha,
                           const u64* fri_betas) {
    using gl::Ext;
    const Ext zeta_next = gl::mul(zeta, gl::root_of_unity(s.log_n));
    u64 subgroup_x = gl::mul(gl::GENERATOR, gl::pow(gl::root_of_unity(s.log_lde), gl::bitrev32(x_index, s.log_lde)));
    Ext old_eval;
    {
        Ext acc = gl::ext(0), apow = gl::ext(1);
        for (u32 o = 0; o < 4; ++o) {
            const u64* leaf = qw + s.off_o[o];
            for (u32 p = 0; p < s.ncols[o]; ++p) {
                acc = gl::add(acc, gl::mul(apow, leaf[p]));
                apow = gl::mul(apow, fri_alpha);
            }
        }
        Ext sum = gl::mul(gl::sub(acc, r0), gl::inv(gl::sub(gl::ext(subgroup_x), zeta)));
        acc = gl::ext(0);
        apow = gl::ext(1);
        const u64* leaf2 = qw + s.off_o[2];
        for (u32 p = 0; p < s.nc; ++p) {
            acc = gl::add(acc, gl::mul(apow, leaf2[p]));
            apow = gl::mul(apow, fri_alpha);
        }
        sum = gl::add(gl::mul(sum, apow), gl::mul(gl::sub(acc, r1), gl::inv(gl::sub(gl::ext(subgroup_x), zeta_next))));
        // compat.fri_mul_final_by_x: the prover multiplied the final polynomial by X, so the combined value carries a factor subgroup_x
        if (s.mul_final_by_x) sum = gl::mul(sum, subgroup_x);
        old_eval = sum;
    }
    bool ok = true;
    for (u32 r = 0; r < s.n_rounds; ++r) {
        const unsigned ab = s.ab[r];
        const u32 arity = 1u << ab;
        const u64* evals = qw + s.off_r[r];
        const u32 coset_index = x_index >> ab, within = x_index & (arity - 1);
        if (evals[2 * within] != old_eval.c0 || evals[2 * within + 1] != old_eval.c1) ok = false;
        // compute_evaluation: interpolate {(coset_start g^i, evals[bitrev(i)])} at beta
        const u64 g = gl::root_of_unity(ab);
        const u64 coset_start = gl::mul(subgroup_x, gl::pow(g, arity - gl::bitrev32(within, ab)));
        const Ext beta = ext_at(fri_betas, r);
        Ext res = gl::ext(0);
        u64 xi = coset_start;
        for (u32 a = 0; a < arity; ++a) {
            Ext num = ext_at(evals, gl::bitrev32(a, ab));
            u64 den = 1, xj = coset_start;
            for (u32 b = 0; b < arity; ++b) {
                if (b != a) {
                    num = gl::mul(num, gl::sub(beta, gl::ext(xj)));
                    den = gl::mul(den, gl::sub(xi, xj));
                }
                xj = gl::mul(xj, g);
            }
            res = gl::add(res, gl::mul(num, gl::inv(den)));
            xi = gl::mul(xi, g);
        }
        old_eval = res;
        for (unsigned k = 0; k < ab; ++k) subgroup_x = gl::mul(subgroup_x, subgroup_x);
        x_index = coset_index;
    }
    Ext acc = gl::ext(0);
    for (u32 k = s.final_len; k-- > 0;) acc = gl::add(gl::mul(acc, subgroup_x), ext_at(fin, k));
    return ok && gl::eq(acc, old_eval);
}
}  // namespace vpbs
