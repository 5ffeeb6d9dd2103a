// Proving mixed batches under MANY resident key sets (vpbs_ring_prover, include/vpbs_prover.h): one object owns a key ring
// (pbs_keyring.hip), C chains of the device-witness pipeline and, per slot of the ring, the key hash chain of that slot's keys.  The chains,
// their queue and the kernels that assemble the preset matrices on the device are the worker pool of pbs_prove_pool.h; this file is the
// pool's key source with a key set PER CIPHERTEXT: the chain of ciphertext i is proven under the device bsk and ksk of slot key_of[i] and
// that slot's key links, and its accumulators come from a count-1 vpbs_keyring_run under that slot.  The proofs are those of a
// vpbs_pbs_prover made with that key set, byte for byte.
//
// The key hash chain stays on the host (vpbs_hash_chain_links: one sequential sponge per key set, eight AVX-512 lanes shared by concurrent
// callers); it is walked once per add, before the object's mutex is taken, so concurrent adds share the lanes.  The links live HERE, not in
// the ring: the ring is marked as owned and refuses vpbs_keyring_add / vpbs_keyring_remove from anybody else, so no slot can hold keys
// whose links this object does not have.  add, remove and run exclude each other under run_mu: no slot changes under a chain being proven.
#include <memory>

#include "pbs_prove_pool.h"
#include "program_internal.h"

using vpbs::DeviceError;
using vpbs::u64;

struct vpbs_ring_prover {
    vpbs::ProvePool pool;
    vpbs_ctx* boot_ctx = nullptr;   // the ring's context
    vpbs_keyring* ring = nullptr;
    size_t max_keys = 0, ggsw_len = 0;
    static constexpr size_t RING_BATCH = 256;   // the ring's max_batch: rows per launch of the outputs (the batch prover's BOOT_BATCH)
    struct Slot {
        std::vector<u64> links;   // host [n_lwe + 2][4]; empty: the slot holds no key set
        u64* d_links = nullptr;   // device, from boot_ctx's pool
        const u64 *d_bsk = nullptr, *d_ksk = nullptr;
    };
    std::vector<Slot> slots;
    std::mutex run_mu;                  // add, remove and run: one at a time
    const uint32_t* key_of = nullptr;   // of the run in progress

    ~vpbs_ring_prover() {
        pool.destroy();
        if (boot_ctx) {
            (void)hipSetDevice(boot_ctx->device);
            for (Slot& s : slots) boot_ctx->release(s.d_links);
        }
        if (ring) vpbs_keyring_free(ring);
        if (boot_ctx) vpbs_ctx_destroy(boot_ctx);
    }
    bool filled(unsigned slot) const { return slot < max_keys && !slots[slot].links.empty(); }
};

namespace vpbs {
std::mutex& ring_prover_mutex(vpbs_ring_prover* p) { return p->run_mu; }

long ring_prover_run_locked(vpbs_ring_prover* p, const uint64_t* cts, size_t count, const uint32_t* key_of, const uint64_t* testv, int testv_per_ct,
                            unsigned steps, uint64_t* out_ct, uint64_t* lwe_out, vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len,
                            const uint8_t* const* checkpoints, const size_t* lens) {
    const char* who = checkpoints ? "vpbs_ring_prover_resume" : "vpbs_ring_prover_run";
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        return (long)VPBS_ERR_INVALID;
    };
    ProvePool& pool = p->pool;
    {   // every index before anything is queued
        std::lock_guard<std::mutex> lk(keyring_mutex(p->ring));
        std::string msg;
        if (!keyring_check_slots(p->ring, key_of, count, who, "ciphertext", &msg)) return refuse(msg);
    }
    const double t_call = now_s();
    pool.stats = vpbs_pbs_run_stats{};
    const unsigned N = pool.shape.N;
    const size_t kn = pool.shape.kn, ct_words = pool.n_lwe + 1;
    // ---- a resume: every checkpoint validated on the host before anything is queued, its key hash against the links of the row's slot ----
    p->key_of = key_of;
    ProvePool::Resume rs;
    if (checkpoints) pool.open_checkpoints(cts, count, testv, testv_per_ct, checkpoints, lens, steps, rs);
    // ---- every output first: one key-ring launch per RING_BATCH ciphertexts; accepted rows enter at their checkpoint's step ----
    if (out_ct || lwe_out) {
        std::lock_guard<std::mutex> lk(pool.boot_mu);
        std::vector<uint32_t> start;
        std::vector<u64> acc_in;
        for (size_t i0 = 0; i0 < count; i0 += vpbs_ring_prover::RING_BATCH) {
            const size_t c = std::min(vpbs_ring_prover::RING_BATCH, count - i0);
            const bool from = rs.resumed && pool.start_rows(rs, i0, c, start, acc_in);
            const long rc = vpbs_keyring_run_from(p->ring, cts + i0 * ct_words, c, key_of + i0, from ? start.data() : nullptr,
                                                  from ? acc_in.data() : nullptr, testv + (testv_per_ct ? i0 * N : 0), testv_per_ct,
                                                  out_ct ? out_ct + i0 * kn : nullptr, lwe_out ? lwe_out + i0 * ct_words : nullptr, nullptr, 0);
            if (rc != (long)c) {
                report(err, err_len, std::string(from ? "vpbs_keyring_run_from: " : "vpbs_keyring_run: ") + vpbs_last_error(p->boot_ctx));
                p->key_of = nullptr;
                return rc < 0 ? rc : (long)VPBS_ERR_DEVICE;
            }
        }
    }
    // ---- the proofs: the pool's workers take ciphertext indices from a queue; each chain under the keys and links of its slot ----
    pool.stats.outputs_seconds = out_ct || lwe_out ? now_s() - t_call : 0.0;
    const long delivered = pool.prove(cts, count, testv, testv_per_ct, steps, t_call, proof_fn, user, checkpoints ? &rs : nullptr);
    p->key_of = nullptr;
    return delivered;
}
}  // namespace vpbs

extern "C" {

int vpbs_ring_prover_create(int device_ordinal, const vpbs_ivc_circuit* cyclic, const vpbs_ivc_circuit* dummy, const vpbs_tfhe_params* prm,
                            unsigned n_lwe, size_t max_keys, unsigned chains, unsigned witness_batch, vpbs_ring_prover** out, char* err,
                            size_t err_len) {
    using namespace vpbs;
    if (out) *out = nullptr;
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        return VPBS_ERR_INVALID;
    };
    if (!cyclic || !dummy || !prm || !out || !cyclic->circuit || !dummy->circuit) return refuse("null argument");
    if (chains == 0 || chains > 64) return refuse("chains must be 1 .. 64");
    if (witness_batch == 0) return refuse("witness_batch must be at least 1 (the batch prover runs the device-witness pipeline)");
    if (prm->log_N < 1 || prm->log_N > 11 || prm->K < 2 || prm->ELL < 1 || prm->LOGB < 1) return refuse("unsupported TFHE parameters");
    if (n_lwe == 0) return refuse("n_lwe must be at least 1");
    auto p = std::make_unique<vpbs_ring_prover>();
    ProvePool& pool = p->pool;
    pool.device = device_ordinal;
    pool.n_lwe = n_lwe;
    pool.total = n_lwe + 2;
    p->max_keys = max_keys;
    p->ggsw_len = (size_t)prm->K * prm->ELL * prm->K * ((size_t)1 << prm->log_N);
    const unsigned log_n_max = std::max(16u, cyclic->circuit->log_n);
    int rc = vpbs_ctx_create(device_ordinal, log_n_max, 3, 4, &p->boot_ctx);
    if (rc != VPBS_OK) return report(err, err_len, "the bootstrap context could not be made (no such device?)"), rc;
    pool.boot_ctx = p->boot_ctx;
    // the ring before the chains: its refusals (the shape, the LDS budget, max_keys) cost nothing, the chains are the large allocations
    char e[512] = {0};
    rc = vpbs_keyring_create(p->boot_ctx, prm, n_lwe, max_keys, vpbs_ring_prover::RING_BATCH, &p->ring, e, sizeof e);
    if (rc != VPBS_OK) return report(err, err_len, e), rc;
    keyring_set_owned(p->ring);
    p->slots.resize(max_keys);
    rc = pool.create_chains(cyclic, dummy, prm, chains, witness_batch, log_n_max, err, err_len);
    if (rc != VPBS_OK) return rc;
    try {
        VPBS_HIP(hipSetDevice(device_ordinal));
        pool.alloc_buffers();
    } catch (const DeviceError& x) {
        (void)vpbs::stream_sync(p->boot_ctx->stream);
        report(err, err_len, x.what);
        return x.status;
    }
    // the key source: the slot of the ciphertext, accumulators from a count-1 run of the ring under that slot (under the ring's own mutex)
    vpbs_ring_prover* self = p.get();
    pool.keys_of = [self](size_t index) {
        const vpbs_ring_prover::Slot& s = self->slots[self->key_of[index]];
        return KeySource{s.d_bsk, s.d_ksk, s.d_links, s.links.data()};
    };
    pool.accumulators = [self](ProvePool::Worker& w, unsigned from, std::string& why) {
        const uint32_t slot = self->key_of[w.index], start = from;
        if (vpbs_keyring_run_from(self->ring, w.d_ct, 1, &slot, from ? &start : nullptr, w.d_acc_in, w.d_testv, 0, nullptr, nullptr, w.d_accs, 1) == 1)
            return true;
        why = vpbs_last_error(self->boot_ctx);
        return false;
    };
    *out = p.release();
    report(err, err_len, "");
    return VPBS_OK;
}

void vpbs_ring_prover_free(vpbs_ring_prover* p) { delete p; }

int vpbs_ring_prover_add(vpbs_ring_prover* p, const uint64_t* bsk, const uint64_t* ksk, int keys_on_device, unsigned* slot_out, char* err,
                         size_t err_len) {
    using namespace vpbs;
    report(err, err_len, "");
    if (!p || !bsk || !ksk || !slot_out) return report(err, err_len, "null argument"), VPBS_ERR_INVALID;
    const unsigned n_lwe = p->pool.n_lwe, total = p->pool.total;
    const size_t g = p->ggsw_len;
    // ---- the key hash chain over [0^ggsw_len, bsk_0 .. bsk_{n-1}, ksk], every link kept: before the mutex, so that concurrent adds hash side by side ----
    vpbs_ring_prover::Slot fresh;
    fresh.links.resize(4 * (size_t)total);
    try {
        VPBS_HIP(hipSetDevice(p->pool.device));
        std::vector<u64> host_keys;   // device keys: downloaded once, for this
        const u64 *h_bsk = bsk, *h_ksk = ksk;
        if (keys_on_device) {
            host_keys.resize((size_t)(n_lwe + 1) * g);
            VPBS_HIP(hipMemcpy(host_keys.data(), bsk, 8 * (size_t)n_lwe * g, hipMemcpyDeviceToHost));
            VPBS_HIP(hipMemcpy(host_keys.data() + (size_t)n_lwe * g, ksk, 8 * g, hipMemcpyDeviceToHost));
            h_bsk = host_keys.data();
            h_ksk = host_keys.data() + (size_t)n_lwe * g;
        }
        const std::vector<u64> zero(g, 0);
        std::vector<const u64*> items(total);
        items[0] = zero.data();
        for (unsigned x = 0; x < n_lwe; ++x) items[1 + x] = h_bsk + (size_t)x * g;
        items[n_lwe + 1] = h_ksk;
        const u64 prefix[4] = {0, 0, 0, 0};
        if (vpbs_hash_chain_links(prefix, items.data(), total, g, fresh.links.data()) != 0)
            throw DeviceError{VPBS_ERR_INVALID, "hash chain of the keys: malformed arguments"};
    } catch (const DeviceError& x) {
        report(err, err_len, x.what);
        return x.status;
    }
    // ---- the slot: the ring's entry, then the links of exactly that entry ----
    std::lock_guard<std::mutex> run(p->run_mu);
    unsigned slot = 0;
    int rc = keyring_add(p->ring, bsk, ksk, keys_on_device, &slot, true);
    if (rc != VPBS_OK) return report(err, err_len, vpbs_last_error(p->boot_ctx)), rc;
    try {
        std::lock_guard<std::mutex> lk(keyring_mutex(p->ring));   // the context's pool is the ring's too
        keyring_slot_keys(p->ring, slot, &fresh.d_bsk, &fresh.d_ksk);
        fresh.d_links = p->boot_ctx->alloc_words(fresh.links.size());
        VPBS_HIP(hipMemcpyAsync(fresh.d_links, fresh.links.data(), 8 * fresh.links.size(), hipMemcpyHostToDevice, p->boot_ctx->stream));
        VPBS_HIP(vpbs::stream_sync(p->boot_ctx->stream));
    } catch (const DeviceError& x) {
        (void)vpbs::stream_sync(p->boot_ctx->stream);
        {
            std::lock_guard<std::mutex> lk(keyring_mutex(p->ring));
            p->boot_ctx->release(fresh.d_links);
        }
        (void)keyring_remove(p->ring, slot, true);
        report(err, err_len, x.what);
        return x.status;
    }
    p->slots[slot] = std::move(fresh);
    *slot_out = slot;
    return VPBS_OK;
}

int vpbs_ring_prover_remove(vpbs_ring_prover* p, unsigned slot, char* err, size_t err_len) {
    using namespace vpbs;
    report(err, err_len, "");
    if (!p) return report(err, err_len, "null prover"), VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> run(p->run_mu);   // no run is in flight: nothing reads the slot's links or keys any more
    if (!p->filled(slot)) return report(err, err_len, "vpbs_ring_prover_remove: slot " + std::to_string(slot) + " holds no key set"), VPBS_ERR_INVALID;
    const int rc = keyring_remove(p->ring, slot, true);
    if (rc != VPBS_OK) report(err, err_len, vpbs_last_error(p->boot_ctx));
    {
        std::lock_guard<std::mutex> lk(keyring_mutex(p->ring));   // the context's pool is the ring's too
        p->boot_ctx->release(p->slots[slot].d_links);
    }
    p->slots[slot] = vpbs_ring_prover::Slot{};   // a later add that gets this number starts from nothing
    return rc;
}

int vpbs_ring_prover_key_hash(vpbs_ring_prover* p, unsigned slot, uint64_t out[4]) {
    if (!p || !out) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> run(p->run_mu);
    if (!p->filled(slot)) return VPBS_ERR_INVALID;
    std::memcpy(out, p->slots[slot].links.data() + 4 * (size_t)(p->pool.total - 1), 32);
    return VPBS_OK;
}

vpbs_keyring* vpbs_ring_prover_keyring(vpbs_ring_prover* p) { return p ? p->ring : nullptr; }

vpbs_ctx* vpbs_ring_prover_context(vpbs_ring_prover* p) { return p ? p->boot_ctx : nullptr; }

int vpbs_ring_prover_verifier_data(const vpbs_ring_prover* p, uint64_t* cyclic_vk, uint64_t* dummy_vk) {
    if (!p) return VPBS_ERR_INVALID;
    return vpbs_ivc_verifier_data(p->pool.workers[0].ivc, cyclic_vk, dummy_vk);
}

int vpbs_ring_prover_set_check_witness(vpbs_ring_prover* p, int on) {
    if (!p) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> run(p->run_mu);
    return p->pool.set_check_witness(on);
}

int vpbs_ring_prover_witness_checks(const vpbs_ring_prover* p, uint64_t out[2]) {
    if (!p || !out) return VPBS_ERR_INVALID;
    p->pool.witness_checks(out);
    return VPBS_OK;
}

int vpbs_ring_prover_set_checkpoint(vpbs_ring_prover* p, unsigned every, vpbs_pbs_checkpoint_fn fn, void* user) {
    if (!p) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> run(p->run_mu);
    p->pool.set_checkpoint(every, fn, user);
    return VPBS_OK;
}

}  // extern "C"

namespace vpbs {
namespace {
// vpbs_ring_prover_run (checkpoints = null) and vpbs_ring_prover_resume
long ring_prover_run(vpbs_ring_prover* p, const uint64_t* cts, size_t count, const uint32_t* key_of, const uint64_t* testv, int testv_per_ct,
                     const uint8_t* const* checkpoints, const size_t* lens, unsigned steps, uint64_t* out_ct, uint64_t* lwe_out,
                     vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len) {
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        return (long)VPBS_ERR_INVALID;
    };
    report(err, err_len, "");
    if (!proof_fn) return refuse("no proof_fn: the proofs have nowhere to go");
    if (count && (!cts || !testv || !key_of)) return refuse("null cts, testv or key_of");
    if (count && checkpoints && !lens) return refuse("checkpoints without lens");
    if (!p) return refuse("null prover");
    if (steps > p->pool.total) return refuse("steps exceeds n_lwe + 2 = " + std::to_string(p->pool.total));
    if (count == 0) return 0;
    std::lock_guard<std::mutex> run(p->run_mu);
    return ring_prover_run_locked(p, cts, count, key_of, testv, testv_per_ct, steps, out_ct, lwe_out, proof_fn, user, err, err_len, checkpoints, lens);
}
}  // namespace
}  // namespace vpbs

extern "C" {
long vpbs_ring_prover_run(vpbs_ring_prover* p, const uint64_t* cts, size_t count, const uint32_t* key_of, const uint64_t* testv, int testv_per_ct,
                          unsigned steps, uint64_t* out_ct, uint64_t* lwe_out, vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len) {
    return vpbs::ring_prover_run(p, cts, count, key_of, testv, testv_per_ct, nullptr, nullptr, steps, out_ct, lwe_out, proof_fn, user, err, err_len);
}

long vpbs_ring_prover_resume(vpbs_ring_prover* p, const uint64_t* cts, size_t count, const uint32_t* key_of, const uint64_t* testv, int testv_per_ct,
                             const uint8_t* const* checkpoints, const size_t* lens, unsigned steps, uint64_t* out_ct, uint64_t* lwe_out,
                             vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len) {
    return vpbs::ring_prover_run(p, cts, count, key_of, testv, testv_per_ct, checkpoints, lens, steps, out_ct, lwe_out, proof_fn, user, err, err_len);
}

int vpbs_ring_prover_last_run(const vpbs_ring_prover* p, vpbs_pbs_run_stats* out) {
    if (!p || !out) return VPBS_ERR_INVALID;
    *out = p->pool.stats;
    return VPBS_OK;
}

}  // extern "C"
