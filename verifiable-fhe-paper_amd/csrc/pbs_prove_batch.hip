// Proving the bootstraps of a batch under ONE resident key set (vpbs_pbs_prover, include/vpbs_prover.h): a vpbs_bootstrapper and C chains of
// the device-witness pipeline (vpbs_ivc, csrc/ivc.hip) share the keys in device memory and the key hash chain, which is walked once when
// the object is made.  The chains, their queue and the kernels that assemble the preset matrices on the device are the worker pool of
// pbs_prove_pool.h; this file is the pool's key source with ONE key set: every chain is proven under the same resident bsk, ksk and key
// links, and a chain's accumulators come from a count-1 run of the object's Bootstrapper.
#include <memory>

#include "pbs_prove_pool.h"
#include "program_internal.h"
#include "test_entries.h"

using vpbs::DeviceError;
using vpbs::u64;

struct vpbs_pbs_prover {
    vpbs::ProvePool pool;
    vpbs_ctx* boot_ctx = nullptr;
    vpbs_bootstrapper* boot = nullptr;
    vpbs::KeySource keys;            // the one key set
    std::vector<u64> key_links;      // host [n_lwe + 2][4]
    static constexpr size_t BOOT_BATCH = 256;
    std::mutex run_mu;               // one run at a time

    ~vpbs_pbs_prover() {
        if (boot) vpbs_bootstrapper_free(boot);
        pool.destroy();
        if (boot_ctx) vpbs_ctx_destroy(boot_ctx);
    }
};

namespace vpbs {
vpbs_bootstrapper* pbs_prover_bootstrapper(vpbs_pbs_prover* p, std::mutex** boot_mu) {
    *boot_mu = &p->pool.boot_mu;
    return p->boot;
}
}  // namespace vpbs

extern "C" {

int vpbs_pbs_prover_create(int device_ordinal, const vpbs_ivc_circuit* cyclic, const vpbs_ivc_circuit* dummy, const vpbs_tfhe_params* prm,
                           unsigned n_lwe, const uint64_t* bsk, const uint64_t* ksk, int keys_on_device, unsigned chains, unsigned witness_batch,
                           vpbs_pbs_prover** out, char* err, size_t err_len) {
    using namespace vpbs;
    if (out) *out = nullptr;
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        return VPBS_ERR_INVALID;
    };
    if (!cyclic || !dummy || !prm || !bsk || !ksk || !out || !cyclic->circuit || !dummy->circuit) return refuse("null argument");
    if (chains == 0 || chains > 64) return refuse("chains must be 1 .. 64");
    if (witness_batch == 0) return refuse("witness_batch must be at least 1 (the batch prover runs the device-witness pipeline)");
    if (prm->log_N < 1 || prm->log_N > 11 || prm->K < 2 || prm->ELL < 1 || prm->LOGB < 1) return refuse("unsupported TFHE parameters");
    if (n_lwe == 0) return refuse("n_lwe must be at least 1");
    auto p = std::make_unique<vpbs_pbs_prover>();
    ProvePool& pool = p->pool;
    pool.device = device_ordinal;
    pool.n_lwe = n_lwe;
    pool.total = n_lwe + 2;
    const unsigned N = 1u << prm->log_N, K = prm->K;
    const size_t ggsw_len = (size_t)K * prm->ELL * K * N;
    const unsigned log_n_max = std::max(16u, cyclic->circuit->log_n);
    char e[512] = {0};
    int rc = vpbs_ctx_create(device_ordinal, log_n_max, 3, 4, &p->boot_ctx);
    if (rc != VPBS_OK) return report(err, err_len, "the bootstrap context could not be made (no such device?)"), rc;
    pool.boot_ctx = p->boot_ctx;
    rc = pool.create_chains(cyclic, dummy, prm, chains, witness_batch, log_n_max, err, err_len);
    if (rc != VPBS_OK) return rc;
    // ---- the resident key set, its hash chain, the Bootstrapper ----
    std::vector<u64> host_keys;   // device keys: downloaded once for the hash chain
    const u64 *h_bsk = bsk, *h_ksk = ksk;
    try {
        VPBS_HIP(hipSetDevice(device_ordinal));
        hipStream_t s = p->boot_ctx->stream;
        if (keys_on_device) {
            p->keys.d_bsk = bsk;
            p->keys.d_ksk = ksk;
            host_keys.resize((size_t)(n_lwe + 1) * ggsw_len);
            VPBS_HIP(hipMemcpyAsync(host_keys.data(), bsk, 8 * (size_t)n_lwe * ggsw_len, hipMemcpyDeviceToHost, s));
            VPBS_HIP(hipMemcpyAsync(host_keys.data() + (size_t)n_lwe * ggsw_len, ksk, 8 * ggsw_len, hipMemcpyDeviceToHost, s));
            VPBS_HIP(vpbs::stream_sync(s));
            h_bsk = host_keys.data();
            h_ksk = host_keys.data() + (size_t)n_lwe * ggsw_len;
        } else {
            u64 *d_b = pool.alloc((size_t)n_lwe * ggsw_len), *d_k = pool.alloc(ggsw_len);
            VPBS_HIP(hipMemcpyAsync(d_b, bsk, 8 * (size_t)n_lwe * ggsw_len, hipMemcpyHostToDevice, s));
            VPBS_HIP(hipMemcpyAsync(d_k, ksk, 8 * ggsw_len, hipMemcpyHostToDevice, s));
            p->keys.d_bsk = d_b;
            p->keys.d_ksk = d_k;
        }
        // the key hash chain over [0^ggsw_len, bsk_0 .. bsk_{n-1}, ksk], every link kept
        const std::vector<u64> zero(ggsw_len, 0);
        std::vector<const u64*> items(pool.total);
        items[0] = zero.data();
        for (unsigned x = 0; x < n_lwe; ++x) items[1 + x] = h_bsk + (size_t)x * ggsw_len;
        items[n_lwe + 1] = h_ksk;
        const u64 prefix[4] = {0, 0, 0, 0};
        p->key_links.resize(4 * (size_t)pool.total);
        if (vpbs_hash_chain_links(prefix, items.data(), pool.total, ggsw_len, p->key_links.data()) != 0)
            throw DeviceError{VPBS_ERR_INVALID, "hash chain of the keys: malformed arguments"};
        u64* d_links = pool.alloc(p->key_links.size());
        VPBS_HIP(hipMemcpyAsync(d_links, p->key_links.data(), 8 * p->key_links.size(), hipMemcpyHostToDevice, s));
        p->keys.d_key_links = d_links;
        p->keys.key_links = p->key_links.data();
        pool.alloc_buffers();   // waits: the caller's key arrays and the staging vectors may go away
    } catch (const DeviceError& x) {
        (void)vpbs::stream_sync(p->boot_ctx->stream);
        report(err, err_len, x.what);
        return x.status;
    }
    rc = vpbs_bootstrapper_create(p->boot_ctx, prm, n_lwe, p->keys.d_bsk, p->keys.d_ksk, 1, vpbs_pbs_prover::BOOT_BATCH, &p->boot, e, sizeof e);
    if (rc != VPBS_OK) return report(err, err_len, std::string("vpbs_bootstrapper_create: ") + e), rc;
    // the key source: one key set for every ciphertext, accumulators from a count-1 run of the Bootstrapper
    vpbs_pbs_prover* self = p.get();
    pool.keys_of = [self](size_t) { return self->keys; };
    pool.accumulators = [self](ProvePool::Worker& w, unsigned from, std::string& why) {
        const uint32_t start = from;
        if (vpbs_bootstrapper_run_from(self->boot, w.d_ct, 1, from ? &start : nullptr, w.d_acc_in, w.d_testv, 0, nullptr, nullptr, w.d_accs, 1) == 1)
            return true;
        why = vpbs_last_error(self->boot_ctx);
        return false;
    };
    *out = p.release();
    report(err, err_len, "");
    return VPBS_OK;
}

void vpbs_pbs_prover_free(vpbs_pbs_prover* p) { delete p; }

int vpbs_pbs_prover_key_hash(const vpbs_pbs_prover* p, uint64_t out[4]) {
    if (!p || !out) return VPBS_ERR_INVALID;
    std::memcpy(out, p->key_links.data() + 4 * (size_t)(p->pool.total - 1), 32);
    return VPBS_OK;
}

int vpbs_pbs_prover_verifier_data(const vpbs_pbs_prover* p, uint64_t* cyclic_vk, uint64_t* dummy_vk) {
    if (!p) return VPBS_ERR_INVALID;
    return vpbs_ivc_verifier_data(p->pool.workers[0].ivc, cyclic_vk, dummy_vk);
}

int vpbs_pbs_prover_set_check_witness(vpbs_pbs_prover* p, int on) {
    if (!p) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> run(p->run_mu);
    return p->pool.set_check_witness(on);
}

int vpbs_pbs_prover_witness_checks(const vpbs_pbs_prover* p, uint64_t out[2]) {
    if (!p || !out) return VPBS_ERR_INVALID;
    p->pool.witness_checks(out);
    return VPBS_OK;
}

int vpbs_pbs_prover_set_checkpoint(vpbs_pbs_prover* p, unsigned every, vpbs_pbs_checkpoint_fn fn, void* user) {
    if (!p) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> run(p->run_mu);
    p->pool.set_checkpoint(every, fn, user);
    return VPBS_OK;
}

}  // extern "C"

namespace vpbs {
namespace {
// vpbs_pbs_prover_run (checkpoints = null) and vpbs_pbs_prover_resume
long pbs_prover_run(vpbs_pbs_prover* p, const uint64_t* cts, size_t count, const uint64_t* testv, int testv_per_ct, const uint8_t* const* checkpoints,
                    const size_t* lens, unsigned steps, uint64_t* out_ct, uint64_t* lwe_out, vpbs_pbs_proof_fn proof_fn, void* user, char* err,
                    size_t err_len) {
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        return (long)VPBS_ERR_INVALID;
    };
    report(err, err_len, "");
    if (!proof_fn) return refuse("no proof_fn: the proofs have nowhere to go");
    if (count && (!cts || !testv)) return refuse("null cts or testv");
    if (count && checkpoints && !lens) return refuse("checkpoints without lens");
    if (!p) return refuse("null prover");
    ProvePool& pool = p->pool;
    if (steps > pool.total) return refuse("steps exceeds n_lwe + 2 = " + std::to_string(pool.total));
    if (count == 0) return 0;
    std::lock_guard<std::mutex> run(p->run_mu);
    const double t_call = now_s();
    pool.stats = vpbs_pbs_run_stats{};
    const unsigned N = pool.shape.N;
    const size_t kn = pool.shape.kn, ct_words = pool.n_lwe + 1;
    // ---- a resume: every checkpoint validated on the host before anything is queued ----
    ProvePool::Resume rs;
    if (checkpoints) pool.open_checkpoints(cts, count, testv, testv_per_ct, checkpoints, lens, steps, rs);
    // ---- every output first: one Bootstrapper launch per BOOT_BATCH ciphertexts; accepted rows enter at their checkpoint's step ----
    if (out_ct || lwe_out) {
        std::lock_guard<std::mutex> lk(pool.boot_mu);
        std::vector<uint32_t> start;
        std::vector<u64> acc_in;
        for (size_t i0 = 0; i0 < count; i0 += vpbs_pbs_prover::BOOT_BATCH) {
            const size_t c = std::min(vpbs_pbs_prover::BOOT_BATCH, count - i0);
            const bool from = rs.resumed && pool.start_rows(rs, i0, c, start, acc_in);
            const long rc = vpbs_bootstrapper_run_from(p->boot, cts + i0 * ct_words, c, from ? start.data() : nullptr, from ? acc_in.data() : nullptr,
                                                       testv + (testv_per_ct ? i0 * N : 0), testv_per_ct, out_ct ? out_ct + i0 * kn : nullptr,
                                                       lwe_out ? lwe_out + i0 * ct_words : nullptr, nullptr, 0);
            if (rc != (long)c) {
                report(err, err_len, std::string(from ? "vpbs_bootstrapper_run_from: " : "vpbs_bootstrapper_run: ") + vpbs_last_error(p->boot_ctx));
                return rc < 0 ? rc : (long)VPBS_ERR_DEVICE;
            }
        }
    }
    // ---- the proofs: the pool's workers take ciphertext indices from a queue ----
    pool.stats.outputs_seconds = out_ct || lwe_out ? now_s() - t_call : 0.0;
    return pool.prove(cts, count, testv, testv_per_ct, steps, t_call, proof_fn, user, checkpoints ? &rs : nullptr);
}
}  // namespace
}  // namespace vpbs

extern "C" {
long vpbs_pbs_prover_run(vpbs_pbs_prover* p, const uint64_t* cts, size_t count, const uint64_t* testv, int testv_per_ct, unsigned steps,
                         uint64_t* out_ct, uint64_t* lwe_out, vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len) {
    return vpbs::pbs_prover_run(p, cts, count, testv, testv_per_ct, nullptr, nullptr, steps, out_ct, lwe_out, proof_fn, user, err, err_len);
}

long vpbs_pbs_prover_resume(vpbs_pbs_prover* p, const uint64_t* cts, size_t count, const uint64_t* testv, int testv_per_ct,
                            const uint8_t* const* checkpoints, const size_t* lens, unsigned steps, uint64_t* out_ct, uint64_t* lwe_out,
                            vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len) {
    return vpbs::pbs_prover_run(p, cts, count, testv, testv_per_ct, checkpoints, lens, steps, out_ct, lwe_out, proof_fn, user, err, err_len);
}

int vpbs_pbs_prover_last_run(const vpbs_pbs_prover* p, vpbs_pbs_run_stats* out) {
    if (!p || !out) return VPBS_ERR_INVALID;
    *out = p->pool.stats;
    return VPBS_OK;
}

// ---- test entries (test_entries.h) ----
int vpbs_test_pbs_prover_dummy_proof(const vpbs_pbs_prover* p, uint64_t* out) {
    if (!p || !out) return VPBS_ERR_INVALID;
    std::memcpy(out, p->pool.shape.dummy_proof, 8 * p->pool.shape.proof_words);   // the vpbs_ivc's own copy, not the device block the kernels read
    return VPBS_OK;
}

int vpbs_test_pbs_prover_preset_matrix(vpbs_pbs_prover* p, const uint64_t* ct, const uint64_t* testv, unsigned first, unsigned count, uint64_t* out) {
    using namespace vpbs;
    if (!p || !ct || !testv || !out || count == 0 || first + count > p->pool.total || first + count < first) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> run(p->run_mu);
    ProvePool& pool = p->pool;
    ProvePool::Worker& w = pool.workers[0];
    w.index = 0;
    std::string why;
    int rc = pool.prepare_chain(w, ct, testv, why);
    if (rc != VPBS_OK) return p->boot_ctx->err = why, rc;
    std::lock_guard<std::mutex> lk(pool.boot_mu);
    u64* d_m = nullptr;
    try {
        VPBS_HIP(hipSetDevice(pool.device));
        const PresetArgs a = pool.preset_args(w, first, count, nullptr);
        const size_t words = a.n_preset() * count;
        d_m = p->boot_ctx->alloc_words(words);
        PresetArgs b = a;
        b.m = d_m;
        VPBS_HIP(hipMemsetAsync(d_m, 0xA5, 8 * words, p->boot_ctx->stream));   // a word the kernels leave out shows
        launch_preset(p->boot_ctx->stream, b);
        VPBS_HIP(hipGetLastError());
        VPBS_HIP(hipMemcpyAsync(out, d_m, 8 * words, hipMemcpyDeviceToHost, p->boot_ctx->stream));
        VPBS_HIP(vpbs::stream_sync(p->boot_ctx->stream));
    } catch (const DeviceError& e) {
        (void)vpbs::stream_sync(p->boot_ctx->stream);
        p->boot_ctx->err = e.what;
        rc = e.status;
    }
    if (d_m) p->boot_ctx->release(d_m);
    return rc;
}

size_t vpbs_test_pbs_prover_preset_words(const vpbs_pbs_prover* p) { return p ? p->pool.shape.n_preset : 0; }

}  // extern "C"
