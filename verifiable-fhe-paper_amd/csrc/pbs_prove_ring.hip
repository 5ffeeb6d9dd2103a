// Proving mixed batches under MANY resident key sets (vpbs_ring_prover, include/vpbs_prover.h): one object owns a key ring
// (pbs_keyring.hip), C chains of the device-witness pipeline and, per slot of the ring, the key hash chain of that slot's keys.  The chains,
// their queue, the kernels that assemble the preset matrices on the device, and creation, run and the pass-through entry points as far as
// the batch prover has the same are the worker pool (pbs_prove_pool.h, pbs_prove_pool.hip); this file is the pool's key source with a key
// set PER CIPHERTEXT: the chain of ciphertext i is proven under the device bsk and ksk of slot key_of[i] and that slot's key links, its
// accumulators come from a count-1 vpbs_keyring_run under that slot and a run's outputs from the ring's batched run.  The proofs are those
// of a vpbs_pbs_prover made with that key set, byte for byte.
//
// The key hash chain stays on the host (vpbs::key_hash_links: one sequential sponge per key set, eight AVX-512 lanes shared by concurrent
// callers); it is walked once per add, before the object's mutex is taken, so concurrent adds share the lanes.  The links live HERE, not in
// the ring: the ring is marked as owned and refuses vpbs_keyring_add / vpbs_keyring_remove from anybody else, so no slot can hold keys
// whose links this object does not have.  add, remove and run exclude each other under run_mu: no slot changes under a chain being proven.
#include <memory>

#include "pbs_prove_pool.h"
#include "program_internal.h"

using vpbs::DeviceError;
using vpbs::ProvePool;
using vpbs::u64;

struct vpbs_ring_prover {
    ProvePool pool;                 // its bootstrap context is the ring's context
    std::mutex run_mu;              // add, remove and run: one at a time
    vpbs_keyring* ring = nullptr;
    size_t max_keys = 0;
    struct Slot {
        std::vector<u64> links;   // host [n_lwe + 2][4]; empty: the slot holds no key set
        u64* d_links = nullptr;   // device, from the bootstrap context's pool
        const u64 *d_bsk = nullptr, *d_ksk = nullptr;
    };
    std::vector<Slot> slots;
    const uint32_t* key_of = nullptr;   // of the run in progress

    ~vpbs_ring_prover() {
        pool.destroy();   // the chains first; the pool frees the context after the ring
        if (pool.boot_ctx) {
            (void)hipSetDevice(pool.device);
            for (Slot& s : slots) pool.boot_ctx->release(s.d_links);
        }
        if (ring) vpbs_keyring_free(ring);
    }
    bool filled(unsigned slot) const { return slot < max_keys && !slots[slot].links.empty(); }
};

namespace vpbs {
std::mutex& ring_prover_mutex(vpbs_ring_prover* p) { return p->run_mu; }

// the ring prover's own refusal (every index names a filled slot, before anything is queued), then the pool's run under key_of
long ring_prover_run_locked(vpbs_ring_prover* p, const uint64_t* cts, size_t count, const uint32_t* key_of, const uint64_t* testv, int testv_per_ct,
                            unsigned steps, uint64_t* out_ct, uint64_t* lwe_out, vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len,
                            const uint8_t* const* checkpoints, const size_t* lens) {
    {
        std::lock_guard<std::mutex> lk(keyring_mutex(p->ring));
        std::string msg;
        if (!keyring_check_slots(p->ring, key_of, count, checkpoints ? "vpbs_ring_prover_resume" : "vpbs_ring_prover_run", "ciphertext", &msg))
            return report(err, err_len, msg), (long)VPBS_ERR_INVALID;
    }
    p->key_of = key_of;
    const long delivered = p->pool.run(cts, count, testv, testv_per_ct, checkpoints, lens, steps, out_ct, lwe_out, proof_fn, user, err, err_len);
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
    if (!out) return report(err, err_len, "null argument"), VPBS_ERR_INVALID;
    auto p = std::make_unique<vpbs_ring_prover>();
    vpbs_ring_prover* self = p.get();
    ProvePool& pool = p->pool;
    // the ring before the chains: its refusals (the shape, the LDS budget, max_keys) cost nothing, the chains are the large allocations
    int rc = pool.create(device_ordinal, cyclic, dummy, prm, n_lwe, chains, witness_batch, err, err_len, [&] {
        char e[512] = {0};
        const int r = vpbs_keyring_create(pool.boot_ctx, prm, n_lwe, max_keys, ProvePool::OUT_BATCH, &self->ring, e, sizeof e);
        if (r != VPBS_OK) return report(err, err_len, e), r;
        keyring_set_owned(self->ring);
        self->max_keys = max_keys;
        self->slots.resize(max_keys);
        return r;
    });
    if (rc == VPBS_OK) rc = pool.alloc_buffers(err, err_len);
    if (rc != VPBS_OK) return rc;
    // the key source: the slot of the ciphertext, accumulators from a count-1 run of the ring under that slot (under the ring's own mutex),
    // outputs from its batched run under the slots of the block
    pool.keys_of = [self](size_t index) {
        const vpbs_ring_prover::Slot& s = self->slots[self->key_of[index]];
        return KeySource{s.d_bsk, s.d_ksk, s.d_links, s.links.data()};
    };
    pool.accumulators = [self](ProvePool::Worker& w, unsigned from, std::string& why) {
        const uint32_t slot = self->key_of[w.index], start = from;
        if (vpbs_keyring_run_from(self->ring, w.d_ct, 1, &slot, from ? &start : nullptr, w.d_acc_in, w.d_testv, 0, nullptr, nullptr, w.d_accs, 1) == 1)
            return true;
        why = vpbs_last_error(self->pool.boot_ctx);
        return false;
    };
    pool.outputs_name = "vpbs_keyring_run";
    pool.outputs = [self](size_t i0, size_t c, const u64* cts, const uint32_t* start, const u64* acc_in, const u64* testv, int testv_per_ct,
                          u64* out_ct, u64* lwe_out) {
        return vpbs_keyring_run_from(self->ring, cts, c, self->key_of + i0, start, acc_in, testv, testv_per_ct, out_ct, lwe_out, nullptr, 0);
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
    vpbs_ctx* ctx = p->pool.boot_ctx;
    // ---- the key hash chain, every link kept: before the mutex, so that concurrent adds hash side by side ----
    vpbs_ring_prover::Slot fresh;
    fresh.links.resize(4 * (size_t)p->pool.total);
    try {
        VPBS_HIP(hipSetDevice(p->pool.device));
        key_hash_links(bsk, ksk, keys_on_device, p->pool.n_lwe, p->pool.shape.ggsw_len, fresh.links.data());
    } catch (const DeviceError& x) {
        report(err, err_len, x.what);
        return x.status;
    }
    // ---- the slot: the ring's entry, then the links of exactly that entry ----
    std::lock_guard<std::mutex> run(p->run_mu);
    unsigned slot = 0;
    int rc = keyring_add(p->ring, bsk, ksk, keys_on_device, &slot, true);
    if (rc != VPBS_OK) return report(err, err_len, vpbs_last_error(ctx)), rc;
    try {
        std::lock_guard<std::mutex> lk(keyring_mutex(p->ring));   // the context's pool is the ring's too
        keyring_slot_keys(p->ring, slot, &fresh.d_bsk, &fresh.d_ksk);
        fresh.d_links = ctx->alloc_words(fresh.links.size());
        VPBS_HIP(hipMemcpyAsync(fresh.d_links, fresh.links.data(), 8 * fresh.links.size(), hipMemcpyHostToDevice, ctx->stream));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
    } catch (const DeviceError& x) {
        (void)vpbs::stream_sync(ctx->stream);
        {
            std::lock_guard<std::mutex> lk(keyring_mutex(p->ring));
            ctx->release(fresh.d_links);
        }
        (void)keyring_remove(p->ring, slot, true);
        report(err, err_len, x.what);
        return x.status;
    }
    p->slots[slot] = std::move(fresh);
    *slot_out = slot;
    return VPBS_OK;
}

int vpbs_ring_prover_add_seeded(vpbs_ring_prover* p, uint64_t mask_seed, const uint64_t* bsk_bodies, const uint64_t* ksk_bodies, int bodies_on_device,
                                unsigned* slot_out, char* err, size_t err_len) {
    using namespace vpbs;
    report(err, err_len, "");
    if (!p || !bsk_bodies || !ksk_bodies || !slot_out) return report(err, err_len, "null argument"), VPBS_ERR_INVALID;
    vpbs_ctx* ctx = p->pool.boot_ctx;
    vpbs_ring_prover::Slot fresh;
    fresh.links.resize(4 * (size_t)p->pool.total);
    // ---- the slot first: the keys exist only once the ring has expanded them; then their hash chain as add walks it for device-only keys ----
    std::lock_guard<std::mutex> run(p->run_mu);
    unsigned slot = 0;
    int rc = keyring_add_seeded(p->ring, mask_seed, bsk_bodies, ksk_bodies, bodies_on_device, &slot, true);
    if (rc != VPBS_OK) return report(err, err_len, vpbs_last_error(ctx)), rc;
    try {
        VPBS_HIP(hipSetDevice(p->pool.device));
        keyring_slot_keys(p->ring, slot, &fresh.d_bsk, &fresh.d_ksk);   // no add or remove is under way: run_mu
        key_hash_links(fresh.d_bsk, fresh.d_ksk, 1, p->pool.n_lwe, p->pool.shape.ggsw_len, fresh.links.data());
        std::lock_guard<std::mutex> lk(keyring_mutex(p->ring));   // the context's pool is the ring's too
        fresh.d_links = ctx->alloc_words(fresh.links.size());
        VPBS_HIP(hipMemcpyAsync(fresh.d_links, fresh.links.data(), 8 * fresh.links.size(), hipMemcpyHostToDevice, ctx->stream));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
    } catch (const DeviceError& x) {
        (void)vpbs::stream_sync(ctx->stream);
        {
            std::lock_guard<std::mutex> lk(keyring_mutex(p->ring));
            ctx->release(fresh.d_links);
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
    vpbs_ctx* ctx = p->pool.boot_ctx;
    std::lock_guard<std::mutex> run(p->run_mu);   // no run is in flight: nothing reads the slot's links or keys any more
    if (!p->filled(slot)) return report(err, err_len, "vpbs_ring_prover_remove: slot " + std::to_string(slot) + " holds no key set"), VPBS_ERR_INVALID;
    const int rc = keyring_remove(p->ring, slot, true);
    if (rc != VPBS_OK) report(err, err_len, vpbs_last_error(ctx));
    {
        std::lock_guard<std::mutex> lk(keyring_mutex(p->ring));   // the context's pool is the ring's too
        ctx->release(p->slots[slot].d_links);
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

vpbs_ctx* vpbs_ring_prover_context(vpbs_ring_prover* p) { return p ? p->pool.boot_ctx : nullptr; }

int vpbs_ring_prover_verifier_data(const vpbs_ring_prover* p, uint64_t* cyclic_vk, uint64_t* dummy_vk) {
    return ProvePool::verifier_data(vpbs::pool_ref(p), cyclic_vk, dummy_vk);
}

int vpbs_ring_prover_set_check_witness(vpbs_ring_prover* p, int on) { return ProvePool::set_check_witness(vpbs::pool_ref(p), on); }

int vpbs_ring_prover_witness_checks(const vpbs_ring_prover* p, uint64_t out[2]) { return ProvePool::witness_checks(vpbs::pool_ref(p), out); }

int vpbs_ring_prover_set_checkpoint(vpbs_ring_prover* p, unsigned every, vpbs_pbs_checkpoint_fn fn, void* user) {
    return ProvePool::set_checkpoint(vpbs::pool_ref(p), every, fn, user);
}

int vpbs_ring_prover_last_run(const vpbs_ring_prover* p, vpbs_pbs_run_stats* out) { return ProvePool::last_run(vpbs::pool_ref(p), out); }

// vpbs_ring_prover_run is this with checkpoints = null
long vpbs_ring_prover_resume(vpbs_ring_prover* p, const uint64_t* cts, size_t count, const uint32_t* key_of, const uint64_t* testv, int testv_per_ct,
                             const uint8_t* const* checkpoints, const size_t* lens, unsigned steps, uint64_t* out_ct, uint64_t* lwe_out,
                             vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len) {
    const long go = ProvePool::check_run(vpbs::pool_ref(p), cts, count, testv, &key_of, checkpoints, lens, steps, proof_fn, err, err_len);
    if (go <= 0) return go;
    std::lock_guard<std::mutex> run(p->run_mu);
    return vpbs::ring_prover_run_locked(p, cts, count, key_of, testv, testv_per_ct, steps, out_ct, lwe_out, proof_fn, user, err, err_len, checkpoints,
                                        lens);
}

long vpbs_ring_prover_run(vpbs_ring_prover* p, const uint64_t* cts, size_t count, const uint32_t* key_of, const uint64_t* testv, int testv_per_ct,
                          unsigned steps, uint64_t* out_ct, uint64_t* lwe_out, vpbs_pbs_proof_fn proof_fn, void* user, char* err, size_t err_len) {
    return vpbs_ring_prover_resume(p, cts, count, key_of, testv, testv_per_ct, nullptr, nullptr, steps, out_ct, lwe_out, proof_fn, user, err, err_len);
}

}  // extern "C"
