// Proving the bootstraps of a batch under ONE resident key set (vpbs_pbs_prover, include/vpbs_prover.h): a vpbs_bootstrapper and C chains of
// the device-witness pipeline (vpbs_ivc, csrc/ivc.hip) share the keys in device memory and the key hash chain, which is walked once when
// the object is made.  The chains, their queue, the kernels that assemble the preset matrices on the device, and creation, run and the
// pass-through entry points as far as the ring prover has the same are the worker pool (pbs_prove_pool.h, pbs_prove_pool.hip); this file is
// the pool's key source with ONE key set: every chain is proven under the same resident bsk, ksk and key links, a chain's accumulators come
// from a count-1 run of the object's Bootstrapper and a run's outputs from its batched run.  The pool's test entries live here too.
#include <memory>

#include "pbs_prove_pool.h"
#include "program_internal.h"
#include "test_entries.h"

using vpbs::DeviceError;
using vpbs::ProvePool;
using vpbs::u64;

struct vpbs_pbs_prover {
    ProvePool pool;
    std::mutex run_mu;               // one run at a time
    vpbs_bootstrapper* boot = nullptr;
    vpbs::KeySource keys;            // the one key set
    std::vector<u64> key_links;      // host [n_lwe + 2][4]

    ~vpbs_pbs_prover() {
        if (boot) vpbs_bootstrapper_free(boot);   // then the pool: the chains, the device memory, the bootstrap context
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
    if (!bsk || !ksk || !out) return report(err, err_len, "null argument"), VPBS_ERR_INVALID;
    auto p = std::make_unique<vpbs_pbs_prover>();
    ProvePool& pool = p->pool;
    int rc = pool.create(device_ordinal, cyclic, dummy, prm, n_lwe, chains, witness_batch, err, err_len);
    if (rc != VPBS_OK) return rc;
    // ---- the resident key set and its hash chain: host keys are on their way to the device while the chain is walked ----
    const size_t ggsw_len = pool.shape.ggsw_len;
    try {
        VPBS_HIP(hipSetDevice(device_ordinal));
        hipStream_t s = pool.boot_ctx->stream;
        if (keys_on_device) {
            p->keys.d_bsk = bsk;
            p->keys.d_ksk = ksk;
        } else {
            u64 *d_b = pool.alloc((size_t)n_lwe * ggsw_len), *d_k = pool.alloc(ggsw_len);
            VPBS_HIP(hipMemcpyAsync(d_b, bsk, 8 * (size_t)n_lwe * ggsw_len, hipMemcpyHostToDevice, s));
            VPBS_HIP(hipMemcpyAsync(d_k, ksk, 8 * ggsw_len, hipMemcpyHostToDevice, s));
            p->keys.d_bsk = d_b;
            p->keys.d_ksk = d_k;
        }
        p->key_links.resize(4 * (size_t)pool.total);
        key_hash_links(bsk, ksk, keys_on_device, n_lwe, ggsw_len, p->key_links.data());
        u64* d_links = pool.alloc(p->key_links.size());
        VPBS_HIP(hipMemcpyAsync(d_links, p->key_links.data(), 8 * p->key_links.size(), hipMemcpyHostToDevice, s));
        p->keys.d_key_links = d_links;
        p->keys.key_links = p->key_links.data();
    } catch (const DeviceError& x) {
        (void)vpbs::stream_sync(pool.boot_ctx->stream);
        report(err, err_len, x.what);
        return x.status;
    }
    rc = pool.alloc_buffers(err, err_len);   // waits: the caller's key arrays may go away
    if (rc != VPBS_OK) return rc;
    char e[512] = {0};
    rc = vpbs_bootstrapper_create(pool.boot_ctx, prm, n_lwe, p->keys.d_bsk, p->keys.d_ksk, 1, ProvePool::OUT_BATCH, &p->boot, e, sizeof e);
    if (rc != VPBS_OK) return report(err, err_len, std::string("vpbs_bootstrapper_create: ") + e), rc;
    // the key source: one key set for every ciphertext, accumulators from a count-1 run of the Bootstrapper, outputs from its batched run
    vpbs_pbs_prover* self = p.get();
    pool.keys_of = [self](size_t) { return self->keys; };
    pool.accumulators = [self](ProvePool::Worker& w, unsigned from, std::string& why) {
        const uint32_t start = from;
        if (vpbs_bootstrapper_run_from(self->boot, w.d_ct, 1, from ? &start : nullptr, w.d_acc_in, w.d_testv, 0, nullptr, nullptr, w.d_accs, 1) == 1)
            return true;
        why = vpbs_last_error(self->pool.boot_ctx);
        return false;
    };
    pool.outputs_name = "vpbs_bootstrapper_run";
    pool.outputs = [self](size_t, size_t c, const u64* cts, const uint32_t* start, const u64* acc_in, const u64* testv, int testv_per_ct, u64* out_ct,
                          u64* lwe_out) {
        return vpbs_bootstrapper_run_from(self->boot, cts, c, start, acc_in, testv, testv_per_ct, out_ct, lwe_out, nullptr, 0);
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
    return ProvePool::verifier_data(vpbs::pool_ref(p), cyclic_vk, dummy_vk);
}

int vpbs_pbs_prover_set_check_witness(vpbs_pbs_prover* p, int on) { return ProvePool::set_check_witness(vpbs::pool_ref(p), on); }

int vpbs_pbs_prover_witness_checks(const vpbs_pbs_prover* p, uint64_t out[2]) { return ProvePool::witness_checks(vpbs::pool_ref(p), out); }

int vpbs_pbs_prover_set_checkpoint(vpbs_pbs_prover* p, unsigned every, vpbs_pbs_checkpoint_fn fn, void* user) {
    return ProvePool::set_checkpoint(vpbs::pool_ref(p), every, fn, user);
}

int vpbs_pbs_prover_last_run(const vpbs_pbs_prover* p, vpbs_pbs_run_stats* out) { return ProvePool::last_run(vpbs::pool_ref(p), out); }

// vpbs_pbs_prover_run is this with checkpoints = null
long vpbs_pbs_prover_resume(vpbs_pbs_prover* p, const uint64_t* cts, size_t count, const uint64_t* testv, int testv_per_ct,
                            const uint8_t* const* checkpoints, const size_t* lens, unsigned steps, uint64_t* out_ct, uint64_t* lwe_out,
                            vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len) {
    const long go = ProvePool::check_run(vpbs::pool_ref(p), cts, count, testv, nullptr, checkpoints, lens, steps, proof_fn, err, err_len);
    if (go <= 0) return go;
    std::lock_guard<std::mutex> run(p->run_mu);
    return p->pool.run(cts, count, testv, testv_per_ct, checkpoints, lens, steps, out_ct, lwe_out, proof_fn, user, err, err_len);
}

long vpbs_pbs_prover_run(vpbs_pbs_prover* p, const uint64_t* cts, size_t count, const uint64_t* testv, int testv_per_ct, unsigned steps,
                         uint64_t* out_ct, uint64_t* lwe_out, vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len) {
    return vpbs_pbs_prover_resume(p, cts, count, testv, testv_per_ct, nullptr, nullptr, steps, out_ct, lwe_out, proof_fn, user, err, err_len);
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
    vpbs_ctx* ctx = pool.boot_ctx;
    ProvePool::Worker& w = pool.workers[0];
    w.index = 0;
    std::string why;
    int rc = pool.prepare_chain(w, ct, testv, why);
    if (rc != VPBS_OK) return ctx->err = why, rc;
    std::lock_guard<std::mutex> lk(pool.boot_mu);
    u64* d_m = nullptr;
    try {
        VPBS_HIP(hipSetDevice(pool.device));
        const PresetArgs a = pool.preset_args(w, first, count, nullptr);
        const size_t words = a.n_preset() * count;
        d_m = ctx->alloc_words(words);
        PresetArgs b = a;
        b.m = d_m;
        VPBS_HIP(hipMemsetAsync(d_m, 0xA5, 8 * words, ctx->stream));   // a word the kernels leave out shows
        launch_preset(ctx->stream, b);
        VPBS_HIP(hipGetLastError());
        VPBS_HIP(hipMemcpyAsync(out, d_m, 8 * words, hipMemcpyDeviceToHost, ctx->stream));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
    } catch (const DeviceError& e) {
        (void)vpbs::stream_sync(ctx->stream);
        ctx->err = e.what;
        rc = e.status;
    }
    if (d_m) ctx->release(d_m);
    return rc;
}

size_t vpbs_test_pbs_prover_preset_words(const vpbs_pbs_prover* p) { return p ? p->pool.shape.n_preset : 0; }

}  // extern "C"
