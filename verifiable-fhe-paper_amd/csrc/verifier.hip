// Host-side verifier of step proofs (no device work): plonky2 0.2.0 plonk/verifier.rs `verify_with_challenges`, plonk/get_challenges.rs,
// fri/verifier.rs `verify_fri_proof` and hash/merkle_proofs.rs `verify_merkle_proof_to_cap`.  The reference calls it as `cd.verify(proof)` at
// /root/reference/src/vtfhe/ivc_based_vpbs.rs:443-447.  What this file owns is the order of the checks: the serial
// transcript, the vanishing identity right behind it, the proof of work before any query is looked at, and the Merkle paths collected and
// climbed last (eight side by side where the CPU has AVX-512).  The proof's layout and the refusal rules come from proof_shape.h, the
// vanishing identity and the arithmetic of a FRI query from verify_core.h -- the same code the device verifier (verify_batch.hip) runs.
// Product code: written against gl.h / poseidon.h, independent of the test oracle.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host/plonky2_mirror.h"
#include "kernels.h"
#include "poseidon.h"
#include "host/poseidon_x8.h"
#include "proof_shape.h"
#include "verify_core.h"

using gl::Ext;
using gl::u64;

namespace {
void two_to_one(const u64* l, const u64* r, u64* out) {
    u64 s[12] = {l[0], l[1], l[2], l[3], r[0], r[1], r[2], r[3], 0, 0, 0, 0};
    poseidon::permute_host(s);
    std::memcpy(out, s, 4 * sizeof(u64));
}
void hash_or_noop(const u64* leaf, size_t len, u64* out) {
    if (len <= 4) {
        std::memset(out, 0, 4 * sizeof(u64));
        std::memcpy(out, leaf, len * sizeof(u64));
    } else {
        poseidon::hash_no_pad_host(leaf, len, out);
    }
}
// verify_merkle_proof_to_cap
bool merkle_verify(const u64* leaf, size_t leaf_len, size_t idx, const u64* cap, const u64* siblings, size_t n_sib) {
    u64 cur[4], nxt[4];
    hash_or_noop(leaf, leaf_len, cur);
    for (size_t k = 0; k < n_sib; ++k) {
        if (idx & 1) two_to_one(siblings + 4 * k, cur, nxt);
        else two_to_one(cur, siblings + 4 * k, nxt);
        std::memcpy(cur, nxt, sizeof cur);
        idx >>= 1;
    }
    return std::memcmp(cur, cap + 4 * idx, sizeof cur) == 0;
}
// The Merkle checks of a proof are independent of each other and of the arithmetic checks: they are collected while the query rounds are
// replayed and verified together at the end -- eight paths of one shape (leaf length, path length) side by side, one per AVX-512 lane
// (host/poseidon_x8.h), where the CPU has them; one after the other otherwise.  4 oracles + 3 FRI rounds x 28 queries = 196 paths,
// ~3 200 permutations: two thirds of the verifier's time when done one by one.
struct MerkleJob {
    const u64* leaf;
    size_t leaf_len, idx;
    const u64* cap;
    const u64* siblings;
    size_t n_sib;
};
#if defined(VPBS_HAVE_POSEIDON_X8)
__attribute__((target("avx512f,avx512dq")))
bool merkle_verify_x8(const MerkleJob* jobs, unsigned cnt) {   // cnt <= 8 jobs of one shape
    using poseidon_x8::V;
    const size_t leaf_len = jobs[0].leaf_len, n_sib = jobs[0].n_sib;
    alignas(64) u64 lane[12][8];
    u64 cur[8][4];
    auto job = [&](unsigned l) -> const MerkleJob& { return jobs[l < cnt ? l : 0]; };   // spare lanes repeat the first job
    if (leaf_len <= 4) {   // hash_or_noop: padded, not hashed
        for (unsigned l = 0; l < 8; ++l)
            for (int i = 0; i < 4; ++i) cur[l][i] = (size_t)i < leaf_len ? job(l).leaf[i] : 0;
    } else {
        V st[12];
        for (int i = 0; i < 12; ++i) st[i] = _mm512_setzero_si512();
        for (size_t off = 0; off < leaf_len; off += 8) {   // overwrite-mode sponge, rate 8
            const size_t len = leaf_len - off < 8 ? leaf_len - off : 8;
            for (size_t i = 0; i < len; ++i) {
                for (unsigned l = 0; l < 8; ++l) lane[i][l] = job(l).leaf[off + i];
                st[i] = _mm512_load_si512(lane[i]);
            }
            poseidon_x8::permute(st, nullptr);
        }
        for (int i = 0; i < 4; ++i) {
            _mm512_store_si512(lane[i], st[i]);
            for (unsigned l = 0; l < 8; ++l) cur[l][i] = lane[i][l];
        }
    }
    size_t idx[8];
    for (unsigned l = 0; l < 8; ++l) idx[l] = job(l).idx;
    for (size_t k = 0; k < n_sib; ++k) {
        for (unsigned l = 0; l < 8; ++l) {
            const u64* sib = job(l).siblings + 4 * k;
            const bool right = idx[l] & 1;   // this node is the right child: two_to_one(sibling, node)
            for (int i = 0; i < 4; ++i) {
                lane[i][l] = right ? sib[i] : cur[l][i];
                lane[i + 4][l] = right ? cur[l][i] : sib[i];
            }
            idx[l] >>= 1;
        }
        V st[12];
        for (int i = 0; i < 8; ++i) st[i] = _mm512_load_si512(lane[i]);
        for (int i = 8; i < 12; ++i) st[i] = _mm512_setzero_si512();
        poseidon_x8::permute(st, nullptr);
        for (int i = 0; i < 4; ++i) {
            _mm512_store_si512(lane[i], st[i]);
            for (unsigned l = 0; l < 8; ++l) cur[l][i] = lane[i][l];
        }
    }
    for (unsigned l = 0; l < cnt; ++l)
        if (std::memcmp(cur[l], jobs[l].cap + 4 * idx[l], sizeof cur[l]) != 0) return false;
    return true;
}
#endif
bool merkle_verify_all(std::vector<MerkleJob>& jobs) {
#if defined(VPBS_HAVE_POSEIDON_X8)
    if (poseidon_x8::enabled()) {   // vpbs_host_set_poseidon_x8(0): one path after the other (A/B measurements, tests of that form)
        std::stable_sort(jobs.begin(), jobs.end(), [](const MerkleJob& a, const MerkleJob& b) {
            return a.leaf_len != b.leaf_len ? a.leaf_len < b.leaf_len : a.n_sib < b.n_sib;
        });
        for (size_t at = 0; at < jobs.size();) {
            size_t end = at + 1;
            while (end < jobs.size() && end - at < 8 && jobs[end].leaf_len == jobs[at].leaf_len && jobs[end].n_sib == jobs[at].n_sib) ++end;
            if (!merkle_verify_x8(jobs.data() + at, (unsigned)(end - at))) return false;
            at = end;
        }
        return true;
    }
#endif
    for (const MerkleJob& j : jobs)
        if (!merkle_verify(j.leaf, j.leaf_len, j.idx, j.cap, j.siblings, j.n_sib)) return false;
    return true;
}
}  // namespace

extern "C" int vpbs_verify_step(const vpbs_verify_inputs* in, const uint64_t* caps, const uint64_t* openings, const uint64_t* fri) {
    using namespace plonky2;
    if (!in || !caps || !openings || !fri || !in->constants_sigmas_cap || (in->n_public_inputs && !in->public_inputs)) return VPBS_ERR_INVALID;
    vpbs::ProofShape S;
    if (!vpbs::make_proof_shape(*in, vpbs::compat_of(*in), vpbs::SHAPE_VERIFY, S)) return VPBS_ERR_INVALID;
    const unsigned nc = S.nc;
    const size_t cap_words = S.cap_words;

    // ---- transcript (plonk/get_challenges.rs) ----
    HashOut pi_hash;
    vpbs_hash_no_pad(in->public_inputs, in->n_public_inputs, pi_hash.data());
    Challenger ch;
    ch.observe_elements(in->circuit_digest, 4);
    ch.observe_hash(pi_hash);
    ch.observe_cap(caps, cap_words / 4);
    const std::vector<u64> betas_gammas = ch.get_n_challenges(2 * (size_t)nc);   // betas [nc] | gammas [nc]
    ch.observe_cap(caps + cap_words, cap_words / 4);
    const std::vector<u64> alphas = ch.get_n_challenges(nc);
    ch.observe_cap(caps + 2 * cap_words, cap_words / 4);
    const Ext zeta = ch.get_extension_challenge();
    ch.observe_elements(openings, S.n_open_words);
    if (!S.fri_only) {
        // eval_vanishing_poly: the gate constraints at zeta come from the openings of the constants and the wires
        const u64* gate_terms = in->gate_terms_zeta;
        std::vector<u64> gt(2 * (size_t)nc);
        if (S.n_gates) {
            vpbs::gate_terms_at(in->gates, in->n_gates, in->num_selectors, openings, in->n_constants, openings + 2 * (size_t)in->n_constants_sigmas,
                                in->n_wires, pi_hash.data(), alphas.data(), nc, gt.data());
            gate_terms = gt.data();
        }
        const vpbs::ZetaTerms zt = vpbs::zeta_terms(S, zeta);
        for (unsigned a = 0; a < nc; ++a)
            if (!vpbs::vanishing_holds(S, openings, a, alphas[a], betas_gammas.data(), zeta, zt,
                                       [&] { return gate_terms ? vpbs::ext_at(gate_terms, a) : gl::ext(0); }))
                return 0;
    }

    // ---- FRI challenges ----
    const Ext fri_alpha = ch.get_extension_challenge();
    const u64* final_words = fri + S.fri_total - 1 - 2 * (size_t)S.final_len;
    const u64 pow_witness = fri[S.fri_total - 1];
    std::vector<u64> fri_betas(2 * (size_t)S.n_rounds);
    for (size_t r = 0; r < S.n_rounds; ++r) {
        ch.observe_cap(fri + r * cap_words, cap_words / 4);
        const Ext beta = ch.get_extension_challenge();
        fri_betas[2 * r] = beta.c0;
        fri_betas[2 * r + 1] = beta.c1;
    }
    ch.observe_elements(final_words, 2 * (size_t)S.final_len);
    if (pow_witness >= gl::P) return 0;
    ch.observe_element(pow_witness);
    const u64 pow_response = ch.get_challenge();
    if (S.pow_bits && (pow_response >> (64 - S.pow_bits)) != 0) return 0;

    // ---- query rounds: the arithmetic of each now, its Merkle paths (4 initial oracles, one per reduction round) collected for the end ----
    Ext reduced0, reduced1;
    vpbs::reduced_openings(S, openings, fri_alpha, reduced0, reduced1);
    const u64* oracle_caps[4] = {in->constants_sigmas_cap, caps, caps + cap_words, caps + 2 * cap_words};
    std::vector<MerkleJob> merkle_jobs;
    merkle_jobs.reserve((size_t)S.nq * (4 + S.n_rounds));
    for (unsigned q = 0; q < S.nq; ++q) {
        size_t x_index = (size_t)(ch.get_challenge() & (((u64)1 << S.log_lde) - 1));
        const u64* qw = fri + S.o_queries + (size_t)q * S.query_words;
        if (!vpbs::fri_query_holds(S, reduced0, reduced1, qw, final_words, (uint32_t)x_index, zeta, fri_alpha, fri_betas.data())) return 0;
        for (size_t o = 0; o < 4; ++o)   // fri_verify_initial_proof
            merkle_jobs.push_back({qw + S.off_o[o], S.ncols[o], x_index, oracle_caps[o], qw + S.off_o[o] + S.ncols[o], S.nsib0});
        for (size_t r = 0; r < S.n_rounds; ++r) {
            x_index >>= S.ab[r];
            const u64* evals = qw + S.off_r[r];
            merkle_jobs.push_back({evals, (size_t)2 << S.ab[r], x_index, fri + r * cap_words, evals + ((size_t)2 << S.ab[r]), S.nsib_r[r]});
        }
    }
    return merkle_verify_all(merkle_jobs) ? 1 : 0;
}

// The inverse of vpbs_step_proof_to_bytes (prover.hip): ProofWithPublicInputs bytes -> the flat arrays vpbs_verify_step takes.  The
// shape comes from `in` (column counts, n_constants, degree); a byte string of another shape is rejected, not guessed at.
extern "C" long vpbs_step_proof_from_bytes(const vpbs_verify_inputs* in, const uint8_t* bytes, size_t len, uint64_t* caps, uint64_t* openings, uint64_t* fri,
                                uint64_t* public_inputs_out, size_t public_inputs_capacity) {
    if (!in || !bytes || !caps || !openings || !fri) return VPBS_ERR_INVALID;
    vpbs::ProofShape S;
    if (!vpbs::make_proof_shape(*in, vpbs::compat_of(*in), vpbs::SHAPE_PARSE, S)) return VPBS_ERR_INVALID;
    struct Reader {   // copies in: bounds, canonical field elements, the expected length bytes
        const vpbs::ProofShape& S;
        const uint8_t* bytes;
        size_t len;
        vpbs::ProofArrays<uint64_t> to;
        size_t pos = 0;
        bool bad = false;
        void get(uint64_t* w, size_t cnt, bool pow) {
            if (bad || pos + 8 * cnt > len) {
                bad = true;
                return;
            }
            std::memcpy(w, bytes + pos, 8 * cnt);
            for (size_t i = 0; i < cnt && !pow; ++i)
                if (w[i] >= gl::P) bad = true;  // non-canonical field element
            pos += 8 * cnt;
        }
        void words(uint32_t dest, size_t cnt, bool pow) { get(to.at(S, dest), cnt, pow); }
        void length_byte(unsigned nsib) {
            if (bad || pos + 1 > len || bytes[pos] != (uint8_t)nsib) bad = true;
            ++pos;
        }
    } rd{S, bytes, len, {caps, openings, fri}};
    vpbs::walk_step_proof(S, rd);
    uint64_t n_pi = 0;
    if (!S.pi_prefix) {   // older layout: the public inputs run to the end of the buffer
        if (!rd.bad && (len - rd.pos) % 8 == 0) n_pi = (len - rd.pos) / 8;
        else rd.bad = true;
    } else {
        rd.get(&n_pi, 1, true);
    }
    if (rd.bad || n_pi > public_inputs_capacity || (n_pi && !public_inputs_out)) return VPBS_ERR_INVALID;
    rd.get(public_inputs_out, (size_t)n_pi, false);
    if (rd.bad || rd.pos != len) return VPBS_ERR_INVALID;
    return (long)n_pi;
}


// verify_pbs of the reference (/root/reference/src/vtfhe/ivc_based_vpbs.rs:388-489), check for check and in its order: the claimed test
// vector, the step counter, the output ciphertext, cd.verify(proof) (vpbs_verify_step, full check), check_cyclic_proof_verifier_data (the
// proof's last public inputs are the circuit's own digest and constants/sigmas cap), verify_hash_output over the bootstrapping / key
// switching keys and over the LWE masks.  The reference panics at the first failing check; here the verdict is returned and `why` names it.
// The prefix form (vpbs_verify_pbs_prefix, vpbs_ivc_resume_pbs) makes the same checks on the last proof of a chain of k = counter proofs: the
// hash chains run over the first k items of ggsw_of / mask_of (csrc/ivc.hip), out_ct is optional, and the key chain may be left to the caller.
namespace {
enum class PbsForm { whole, prefix, prefix_without_keys };

// key hash chain over ggsw_of(0 .. k-1) = [zeros, bsk_0 .. bsk_{k-2}] (+ ksk at k = n + 2), linked without materialising the items
bool key_chain_matches(const vpbs_verify_pbs_inputs* in, unsigned k, const uint64_t* claimed) {
    const size_t g = in->ggsw_len;
    const std::vector<uint64_t> zero(g, 0);
    std::vector<const uint64_t*> items(k);
    for (unsigned s = 0; s < k; ++s) items[s] = s == 0 ? zero.data() : (s <= in->n_lwe ? in->bsk + (size_t)(s - 1) * g : in->ksk);
    std::vector<uint64_t> links(4 * (size_t)k);
    const uint64_t h0[4] = {0, 0, 0, 0};
    if (vpbs_hash_chain_links(h0, items.data(), k, g, links.data()) != 0) return false;
    return std::memcmp(links.data() + 4 * ((size_t)k - 1), claimed, 32) == 0;
}

int verify_pbs_form(const vpbs_verify_pbs_inputs* in, const uint8_t* proof_bytes, size_t len, PbsForm form, unsigned* steps_done, char* why,
                    size_t why_len) {
    auto say = [&](const char* m) {
        if (why && why_len) {
            std::strncpy(why, m, why_len - 1);
            why[why_len - 1] = 0;
        }
    };
    say("");
    const bool whole = form == PbsForm::whole;
    // out_ct is part of the statement (the reference asserts it, :440-442): a verdict without it would not bind the proof to the ciphertext
    // the caller holds.  ggsw_len strides the caller's bsk / ksk arrays: it must be a whole number of [K][N] GLWE rows (K * ELL * K * N)
    // the form without the key chain never reads bsk / ksk: its internal callers (the batch provers' resume) hold no host keys
    const bool keys_read = form != PbsForm::prefix_without_keys;
    if (!in || !in->circuit || !proof_bytes || !in->testv || (whole && !in->out_ct) || !in->ct || (keys_read && (!in->ksk || (in->n_lwe && !in->bsk))) || in->N == 0 ||
        in->K == 0 || in->ggsw_len == 0 || in->ggsw_len % ((size_t)in->K * in->K * in->N) != 0) {
        say(whole ? "malformed arguments (testv, out_ct, ct, ksk, bsk are all required; ggsw_len = K * ELL * K * N)"
                  : "malformed arguments (testv, ct, ksk, bsk are all required; ggsw_len = K * ELL * K * N)");
        return VPBS_ERR_INVALID;
    }
    const vpbs_verify_inputs& c = *in->circuit;
    const size_t kn = (size_t)in->K * in->N, cap_words = (size_t)4 << c.cap_height;
    const size_t n_pi = 2 * kn + 1 + 8 + 4 + cap_words;   // acc_init | counter | acc | two hashes | verifier data (digest, cap)
    std::vector<uint64_t> caps(3 * cap_words),
        openings(2 * ((size_t)c.n_constants_sigmas + c.n_wires + c.n_zs_partial_products + c.n_quotient + c.num_challenges)), fri(len / 8 + 8), pis(n_pi);
    if (vpbs_step_proof_from_bytes(&c, proof_bytes, len, caps.data(), openings.data(), fri.data(), pis.data(), n_pi) != (long)n_pi) {
        say("the bytes are not a proof of this circuit (shape, canonical field elements, number of public inputs)");
        return 0;
    }
    // claimed test vector: K - 1 zero polynomials, then testv (:422-433)
    for (size_t i = 0; i < kn - in->N; ++i)
        if (pis[i] != 0) {
            say("claimed test vector: the mask polynomials are not zero");
            return 0;
        }
    if (std::memcmp(pis.data() + kn - in->N, in->testv, 8 * (size_t)in->N) != 0) {
        say("claimed test vector differs from testv");
        return 0;
    }
    const uint64_t total = (uint64_t)in->n_lwe + 2;
    if (whole && pis[kn] != total) {   // :435-438
        say("the counter is not n + 2");
        return 0;
    }
    if (!whole && (pis[kn] == 0 || pis[kn] > total)) {
        say("the counter is not in 1 .. n + 2");
        return 0;
    }
    const unsigned k = (unsigned)pis[kn];
    if (in->out_ct && std::memcmp(pis.data() + kn + 1, in->out_ct, 8 * kn) != 0) {   // :440-442
        say("the output ciphertext is not the proof's accumulator");
        return 0;
    }
    vpbs_verify_inputs v = c;   // cd.verify (:444-448)
    v.public_inputs = pis.data();
    v.n_public_inputs = n_pi;
    v.fri_only = 0;
    const int ok = vpbs_verify_step(&v, caps.data(), openings.data(), fri.data());
    if (ok < 0) {
        say("malformed circuit description");
        return ok;
    }
    if (ok != 1) {
        say("the proof does not verify");
        return 0;
    }
    // check_cyclic_proof_verifier_data (:449-453): the verifier data the chain was run with is this circuit's
    const uint64_t* vk = pis.data() + n_pi - 4 - cap_words;
    if (std::memcmp(vk, c.circuit_digest, 32) != 0 || !c.constants_sigmas_cap || std::memcmp(vk + 4, c.constants_sigmas_cap, 8 * cap_words) != 0) {
        say("the proof carries another circuit's verifier data");
        return 0;
    }
    // verify_hash_output (:454-481): dummy GGSW, the n bootstrapping keys, the key-switching key / ct[n], the n masks, zero -- the first k of them
    if (form != PbsForm::prefix_without_keys && !key_chain_matches(in, k, pis.data() + 2 * kn + 1)) {
        say("the key hash chain does not match");
        return 0;
    }
    std::vector<uint64_t> masks(k, 0);
    for (unsigned s = 0; s < k; ++s) masks[s] = s == 0 ? in->ct[in->n_lwe] : (s <= in->n_lwe ? in->ct[s - 1] : 0);
    if (vpbs_hash_chain(masks.data(), k, 1, pis.data() + 2 * kn + 5, nullptr) != 1) {
        say("the LWE hash chain does not match");
        return 0;
    }
    if (steps_done) *steps_done = k;
    return 1;
}
}  // namespace

namespace vpbs {
// vpbs_ivc_resume_pbs's two halves of the prefix form: every check but the key hash chain (a few ms), and that chain alone (seconds)
int verify_pbs_prefix_without_keys(const vpbs_verify_pbs_inputs* in, const uint8_t* bytes, size_t len, unsigned* steps_done, char* why, size_t why_len) {
    return verify_pbs_form(in, bytes, len, PbsForm::prefix_without_keys, steps_done, why, why_len);
}
bool pbs_key_chain_prefix_matches(const vpbs_verify_pbs_inputs* in, unsigned k, const uint64_t claimed[4]) { return key_chain_matches(in, k, claimed); }
}  // namespace vpbs

extern "C" int vpbs_verify_pbs(const vpbs_verify_pbs_inputs* in, const uint8_t* proof_bytes, size_t len, char* why, size_t why_len) {
    return verify_pbs_form(in, proof_bytes, len, PbsForm::whole, nullptr, why, why_len);
}

extern "C" int vpbs_verify_pbs_prefix(const vpbs_verify_pbs_inputs* in, const uint8_t* bytes, size_t len, unsigned* steps_done, char* why,
                                      size_t why_len) {
    return verify_pbs_form(in, bytes, len, PbsForm::prefix, steps_done, why, why_len);
}
