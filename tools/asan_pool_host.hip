// Stand-alone host program for tools/asan_pool_host.sh: the host code both batch provers share (csrc/pbs_prove_pool.hip, vpbs::key_hash_links)
// under AddressSanitizer and UBSan, without a device and without Python.  It walks the key links of host keys at item lengths on both sides
// of a sponge block against the public walker, and calls every run, resume and pass-through entry point of both provers in the refused
// forms that need no object: no proof_fn, null cts, checkpoints without lens, a null prover (with and without an empty batch).  The
// refusals that read an object (steps > n_lwe + 2, count == 0 on a live prover) need a device and are the GPU suite's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../verifiable-fhe-paper_amd/csrc/context.h"

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);    \
            ++failures;                                              \
        }                                                            \
    } while (0)

static void proof_fn(void*, size_t, const uint8_t*, size_t, const char*) { std::abort(); }   // a refused run calls nobody

int main() {
    using vpbs::u64;
    // ---- the key links ----
    u64 x = 0x9E3779B97F4A7C15ull;
    auto next = [&] {   // canonical words
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return x % 0xFFFFFFFF00000001ull;
    };
    for (unsigned n_lwe : {0u, 1u, 6u})
        for (size_t g : {(size_t)64, (size_t)65}) {
            std::vector<u64> bsk((size_t)n_lwe * g), ksk(g), zero(g, 0), links(4 * ((size_t)n_lwe + 2)), want(links.size());
            for (u64& v : bsk) v = next();
            for (u64& v : ksk) v = next();
            vpbs::key_hash_links(n_lwe ? bsk.data() : nullptr, ksk.data(), 0, n_lwe, g, links.data());
            std::vector<const u64*> items{zero.data()};
            for (unsigned k = 0; k < n_lwe; ++k) items.push_back(bsk.data() + (size_t)k * g);
            items.push_back(ksk.data());
            const u64 prefix[4] = {0, 0, 0, 0};
            CHECK(vpbs_hash_chain_links(prefix, items.data(), items.size(), g, want.data()) == VPBS_OK);
            CHECK(links == want);
            u64 kh[4];
            CHECK(vpbs_pbs_key_hash(n_lwe ? bsk.data() : nullptr, ksk.data(), n_lwe, g, kh) == VPBS_OK);
            CHECK(std::memcmp(kh, want.data() + 4 * ((size_t)n_lwe + 1), 32) == 0);
        }
    // ---- the refusals that need no object: outputs untouched, proof_fn not called ----
    u64 buf[8] = {7, 7, 7, 7, 7, 7, 7, 7};
    const uint32_t key_of[1] = {0};
    const uint8_t* cps[1] = {nullptr};
    const size_t lens[1] = {0};
    char err[64];
    struct Case {
        const u64 *cts, *testv;
        size_t count;
        const uint8_t* const* cps;
        const size_t* lens;
        vpbs_pbs_proof_fn fn;
        const char *pbs, *ring;   // the message of either prover
    };
    const Case cases[] = {
        {buf, buf, 1, nullptr, nullptr, nullptr, "no proof_fn: the proofs have nowhere to go", "no proof_fn: the proofs have nowhere to go"},
        {nullptr, buf, 1, nullptr, nullptr, proof_fn, "null cts or testv", "null cts, testv or key_of"},
        {buf, nullptr, 1, nullptr, nullptr, proof_fn, "null cts or testv", "null cts, testv or key_of"},
        {buf, buf, 1, cps, nullptr, proof_fn, "checkpoints without lens", "checkpoints without lens"},
        {buf, buf, 1, cps, lens, proof_fn, "null prover", "null prover"},
        {buf, buf, 1, nullptr, nullptr, proof_fn, "null prover", "null prover"},
        {nullptr, nullptr, 0, nullptr, nullptr, proof_fn, "null prover", "null prover"},
    };
    for (const Case& c : cases) {
        long rc = vpbs_pbs_prover_resume(nullptr, c.cts, c.count, c.testv, 0, c.cps, c.lens, 0, buf, buf, c.fn, nullptr, err, sizeof err);
        CHECK(rc == VPBS_ERR_INVALID && std::strcmp(err, c.pbs) == 0);
        rc = vpbs_ring_prover_resume(nullptr, c.cts, c.count, key_of, c.testv, 0, c.cps, c.lens, 0, buf, buf, c.fn, nullptr, err, sizeof err);
        CHECK(rc == VPBS_ERR_INVALID && std::strcmp(err, c.ring) == 0);
        if (!c.cps) {
            rc = vpbs_pbs_prover_run(nullptr, c.cts, c.count, c.testv, 0, 0, buf, buf, c.fn, nullptr, err, sizeof err);
            CHECK(rc == VPBS_ERR_INVALID && std::strcmp(err, c.pbs) == 0);
            rc = vpbs_ring_prover_run(nullptr, c.cts, c.count, key_of, c.testv, 0, 0, buf, buf, c.fn, nullptr, err, sizeof err);
            CHECK(rc == VPBS_ERR_INVALID && std::strcmp(err, c.ring) == 0);
        }
    }
    long rc = vpbs_ring_prover_run(nullptr, buf, 1, nullptr, buf, 0, 0, buf, buf, proof_fn, nullptr, err, sizeof err);
    CHECK(rc == VPBS_ERR_INVALID && std::strcmp(err, "null cts, testv or key_of") == 0);
    rc = vpbs_pbs_prover_run(nullptr, buf, 1, buf, 0, 0, buf, buf, proof_fn, nullptr, err, 5);   // a short buffer: truncated, terminated
    CHECK(rc == VPBS_ERR_INVALID && std::strcmp(err, "null") == 0);
    rc = vpbs_pbs_prover_run(nullptr, buf, 1, buf, 0, 0, buf, buf, proof_fn, nullptr, nullptr, 0);   // no buffer at all
    CHECK(rc == VPBS_ERR_INVALID);
    for (u64 v : buf) CHECK(v == 7);
    // ---- the pass-throughs of a null object ----
    uint64_t two[2];
    vpbs_pbs_run_stats st;
    CHECK(vpbs_pbs_prover_verifier_data(nullptr, buf, buf) == VPBS_ERR_INVALID && vpbs_ring_prover_verifier_data(nullptr, buf, buf) == VPBS_ERR_INVALID);
    CHECK(vpbs_pbs_prover_set_check_witness(nullptr, 1) == VPBS_ERR_INVALID && vpbs_ring_prover_set_check_witness(nullptr, 1) == VPBS_ERR_INVALID);
    CHECK(vpbs_pbs_prover_witness_checks(nullptr, two) == VPBS_ERR_INVALID && vpbs_ring_prover_witness_checks(nullptr, two) == VPBS_ERR_INVALID);
    CHECK(vpbs_pbs_prover_set_checkpoint(nullptr, 1, nullptr, nullptr) == VPBS_ERR_INVALID);
    CHECK(vpbs_ring_prover_set_checkpoint(nullptr, 1, nullptr, nullptr) == VPBS_ERR_INVALID);
    CHECK(vpbs_pbs_prover_last_run(nullptr, &st) == VPBS_ERR_INVALID && vpbs_ring_prover_last_run(nullptr, &st) == VPBS_ERR_INVALID);
    vpbs_pbs_prover_free(nullptr);
    vpbs_ring_prover_free(nullptr);
    std::printf(failures ? "%d checks failed\n" : "asan_pool_host: all checks passed\n", failures);
    return failures ? 1 : 0;
}
