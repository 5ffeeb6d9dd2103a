// Bootstrapping a mixed batch under MANY resident key sets in one launch (vpbs_keyring_*): the chain of pbs_batch.hip, one workgroup per
// ciphertext, but every workgroup takes ITS ciphertext's key set from a table in device memory.  Workgroup w handles ciphertext order[w]
// under slot key_of[order[w]]; the outputs go to the caller's positions, so the permutation never shows.  The chain itself is pb_chain of
// pbs_chain.h, the body of pbs_batch_kernel as well: the words are pbs_batch_kernel's because the code is.
//
// What is this file's own: the key source and the prefetch depth.  With one key set per launch the rows of bsk[x] are in L2 / the Infinity
// Cache after the first reader; with a key set per workgroup they come from HBM, so their latency has to be hidden inside the workgroup:
// pb_chain's PF = 4 or 8 requests the rows of an input polynomial into a register array before that polynomial is decomposed and
// transformed.  A shape that needs more entries per thread (ELL K N / (2 T) > 8) reads in the loop as pbs_batch_kernel does (PF = 0).  No
// workgroup waits for another.  On the host the ring keeps its mutex, its slot table, the dispatch order and the owner flag; the rest of a
// create and of a run is pbs_chain_host.h, shared with the Bootstrapper.
#define GL_ASM_SCRATCH_LOW 1  // as pbs_batch.hip
#include <cstring>
#include <mutex>
#include <vector>

#include "pbs_chain_host.h"

using vpbs::DeviceError;
using vpbs::u64;

namespace vpbs {
namespace {
struct KeySlot {
    const u64* bsk;   // [n_lwe][K][ELL][K][N], NTT domain; null: the slot is empty
    const u64* ksk;   // [K][ELL][K][N]
};

struct PbsKeyringArgs {
    const u64* cts;          // [count][n_lwe + 1]
    const u64* testv;        // [N] or [count][N]
    size_t testv_stride;     // 0 (shared) or N
    const KeySlot* table;    // [max_keys]
    const uint32_t* order;   // [count]: the ciphertext of workgroup w
    const uint32_t* key_of;  // [count]: the slot of ciphertext c (validated on the host)
    const u64* roots;        // ring_table: [ROOTS | INVROOTS]
    u64 ninv;
    u64* out_ct;             // [count][K][N] or null
    u64* lwe_out;            // [count][n_lwe + 1] or null
    u64* accs_out;           // [count][n_lwe + 2][K][N] or null
    unsigned log_n, K, ELL, LOGB, n_lwe;
    // the start mode, behind everything else: the fields above keep the offsets the kernels without it (FROM = false) were compiled for
    const uint32_t* start;   // [count] or null: ciphertext c enters the chain at step start[c] (0: from the rotated test vector)
    const u64* acc_in;       // [count][K][N] or null: the accumulator after step start[c] - 1 of the ciphertexts that enter late
};

// One workgroup per ciphertext.  PF: 16-byte key words a thread holds ahead per input polynomial, chosen by the host as the smallest of
// 4 and 8 that covers ELL * ceil(K N / (2 T)) (4 at the paper's shape with 1024 threads, 8 with 512); 0: no room, read in the loop.
// FROM: the start mode, an instantiation of its own as in pbs_batch_kernel.
template <unsigned T, unsigned PF, bool FROM>
__global__ void __launch_bounds__(T) pbs_keyring_kernel(PbsKeyringArgs a) {
    // wave-uniform: this workgroup's ciphertext and its key set
    const size_t b = a.order[blockIdx.x];
    const KeySlot key = a.table[a.key_of[b]];
    pb_chain<T, PF, FROM>(a, b, key.bsk, key.ksk);
}

template <unsigned PF>
struct RingKernel {
    template <unsigned T, bool FROM>
    struct Of {
        static constexpr auto fn = &pbs_keyring_kernel<T, PF, FROM>;
    };
};

// order[w]: the ciphertext of workgroup w.  A stable counting sort of the batch by slot, dealt so that the ciphertexts of one key set are
// neighbours in dispatch order.
void keyring_order(const uint32_t* key_of, size_t count, size_t max_keys, std::vector<uint32_t>& start, uint32_t* order) {
    start.assign(max_keys + 1, 0);
    for (size_t i = 0; i < count; ++i) ++start[key_of[i] + 1];
    for (size_t k = 0; k < max_keys; ++k) start[k + 1] += start[k];
    for (size_t i = 0; i < count; ++i) order[start[key_of[i]]++] = (uint32_t)i;
}
}  // namespace
}  // namespace vpbs

struct vpbs_keyring : vpbs::ChainHost {
    size_t max_keys = 0, ggsw_words = 0;
    std::mutex mu;   // add, remove and run: one at a time
    bool has_owner = false;   // the ring of a vpbs_ring_prover: key sets come and go through the prover alone (keyring_set_owned)
    struct Slot {
        bool used = false;
        u64 *own_bsk = nullptr, *own_ksk = nullptr;   // what add uploaded (null for adopted pointers)
        const u64 *bsk = nullptr, *ksk = nullptr;     // what the device table holds for the slot
    };
    std::vector<Slot> slots;
    size_t used = 0;
    vpbs::KeySlot* d_table = nullptr;   // [max_keys]
    uint32_t* d_index = nullptr;        // order [max_batch] | key_of [max_batch]
    std::vector<uint32_t> h_index, sort_start;

    ~vpbs_keyring() {   // the slots' own key sets; ~ChainHost releases the rest
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)vpbs::stream_sync(ctx->stream);
        for (Slot& s : slots) {
            ctx->release(s.own_bsk);
            ctx->release(s.own_ksk);
        }
    }
};

namespace vpbs {
void keyring_shape(const vpbs_keyring* r, KeyringShape* out) { *out = KeyringShape{r->ctx, r->prm, r->n_lwe, r->max_keys, r->max_batch}; }

std::mutex& keyring_mutex(vpbs_keyring* r) { return r->mu; }

bool keyring_check_slots(const vpbs_keyring* r, const uint32_t* key_of, size_t count, const char* who, const char* what, std::string* msg) {
    for (size_t i = 0; i < count; ++i) {
        const uint32_t s = key_of[i];
        if (s >= r->max_keys || !r->slots[s].used) {
            *msg = std::string(who) + ": key_of[" + std::to_string(i) + "] = " + std::to_string(s) +
                   (s >= r->max_keys ? ": slot out of range (max_keys " + std::to_string(r->max_keys) + ")" : ": slot " + std::to_string(s) + " is empty") +
                   "; " + what + " " + std::to_string(i) + " has no key set, nothing was launched";
            return false;
        }
    }
    return true;
}

void keyring_enqueue(vpbs_keyring* r, const uint64_t* d_cts, size_t count, const uint64_t* d_testv, int testv_per_ct, const uint32_t* d_order,
                     const uint32_t* d_key_of, uint64_t* d_out_ct, uint64_t* d_lwe_out, uint64_t* d_accs_out, const uint32_t* d_start,
                     const uint64_t* d_acc_in) {
    vpbs_ctx* ctx = r->ctx;
    PbsKeyringArgs a{};
    chain_fill_args(r, &a, d_cts, d_testv, testv_per_ct, d_out_ct, d_lwe_out, d_accs_out, d_start, d_acc_in);
    a.table = r->d_table;
    a.order = d_order;
    a.key_of = d_key_of;
    {
        vpbs::Timed t(ctx, "pbs_keyring");
        const unsigned threads = r->chain_threads(count);   // the Bootstrapper's rule
        const unsigned kn = a.K << a.log_n;
        const unsigned total = a.ELL * ((kn + 2 * threads - 1) / (2 * threads));   // 16-byte key words per thread and input polynomial
        if (total <= 4) chain_launch<RingKernel<4>::Of>(ctx->stream, a, count, threads, r->lds_bytes);
        else if (total <= 8) chain_launch<RingKernel<8>::Of>(ctx->stream, a, count, threads, r->lds_bytes);
        else chain_launch<RingKernel<0>::Of>(ctx->stream, a, count, threads, r->lds_bytes);
    }
    VPBS_HIP(hipGetLastError());
}
}  // namespace vpbs

extern "C" {
int vpbs_keyring_create(vpbs_ctx* ctx, const vpbs_tfhe_params* prm, unsigned n_lwe, size_t max_keys, size_t max_batch, vpbs_keyring** out,
                        char* err, size_t err_len) {
    using namespace vpbs;
    if (out) *out = nullptr;
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        if (ctx) ctx->err = m;
        return VPBS_ERR_INVALID;
    };
    if (!ctx || !prm || !out) return refuse("null argument");
    size_t lds_bytes = 0;
    unsigned threads = 0;
    std::string why;
    if (!chain_shape_check(prm, n_lwe, max_batch, &lds_bytes, &threads, &why)) return refuse(why);
    if (max_keys == 0 || max_keys > 65535) return refuse("max_keys must be 1 .. 65535");
    auto* r = new vpbs_keyring;
    r->ctx = ctx;
    r->prm = *prm;
    r->n_lwe = n_lwe;
    r->max_keys = max_keys;
    r->max_batch = max_batch;
    r->lds_bytes = lds_bytes;
    r->threads = threads;
    r->ggsw_words = ((size_t)prm->K * prm->ELL * prm->K) << prm->log_N;
    r->slots.resize(max_keys);
    r->h_index.resize(2 * max_batch);
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        r->d_table = reinterpret_cast<KeySlot*>(r->alloc((max_keys * sizeof(KeySlot) + 7) / 8));
        r->d_index = reinterpret_cast<uint32_t*>(r->alloc((2 * max_batch * sizeof(uint32_t) + 7) / 8));
        VPBS_HIP(hipMemsetAsync(r->d_table, 0, max_keys * sizeof(KeySlot), ctx->stream));
        r->alloc_staging();
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
    } catch (const DeviceError& e) {
        report(err, err_len, e.what);
        ctx->err = e.what;
        delete r;
        return e.status;
    }
    *out = r;
    report(err, err_len, "");
    return VPBS_OK;
}

void vpbs_keyring_free(vpbs_keyring* r) { delete r; }

int vpbs_keyring_add(vpbs_keyring* r, const uint64_t* bsk, const uint64_t* ksk, int keys_on_device, unsigned* slot_out) {
    return vpbs::keyring_add(r, bsk, ksk, keys_on_device, slot_out, false);
}

int vpbs_keyring_add_seeded(vpbs_keyring* r, uint64_t mask_seed, const uint64_t* bsk_bodies, const uint64_t* ksk_bodies, int bodies_on_device,
                            unsigned* slot_out) {
    return vpbs::keyring_add_seeded(r, mask_seed, bsk_bodies, ksk_bodies, bodies_on_device, slot_out, false);
}

int vpbs_keyring_remove(vpbs_keyring* r, unsigned slot) { return vpbs::keyring_remove(r, slot, false); }
}  // extern "C"

namespace vpbs {
namespace {
// a ring that a ring prover owns takes key sets from its owner alone: the prover keeps the key hash chain of every slot it filled
bool refuse_owned(vpbs_keyring* r, bool owner, const char* who) {
    if (!r->has_owner || owner) return false;
    r->ctx->err = std::string(who) + ": the ring belongs to a vpbs_ring_prover, which keeps the key hash chain of every slot: add and remove "
                  "key sets through vpbs_ring_prover_add / vpbs_ring_prover_remove";
    return true;
}
}  // namespace

void keyring_set_owned(vpbs_keyring* r) {
    std::lock_guard<std::mutex> lock(r->mu);
    r->has_owner = true;
}

void keyring_slot_keys(const vpbs_keyring* r, unsigned slot, const uint64_t** d_bsk, const uint64_t** d_ksk) {
    const bool used = slot < r->max_keys && r->slots[slot].used;
    *d_bsk = used ? r->slots[slot].bsk : nullptr;
    *d_ksk = used ? r->slots[slot].ksk : nullptr;
}

int keyring_add(vpbs_keyring* r, const uint64_t* bsk, const uint64_t* ksk, int keys_on_device, unsigned* slot_out, bool owner) {
    if (!r || !bsk || !ksk || !slot_out) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(r->mu);
    vpbs_ctx* ctx = r->ctx;
    if (refuse_owned(r, owner, "vpbs_keyring_add")) return VPBS_ERR_INVALID;
    size_t s = 0;
    while (s < r->max_keys && r->slots[s].used) ++s;
    if (s == r->max_keys) {
        ctx->err = "vpbs_keyring_add: all " + std::to_string(r->max_keys) + " slots of the ring are taken (max_keys)";
        return VPBS_ERR_INVALID;
    }
    vpbs_keyring::Slot fresh;
    fresh.used = true;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        KeySlot entry{bsk, ksk};
        if (!keys_on_device) {
            fresh.own_bsk = ctx->alloc_words((size_t)r->n_lwe * r->ggsw_words);
            fresh.own_ksk = ctx->alloc_words(r->ggsw_words);
            VPBS_HIP(hipMemcpyAsync(fresh.own_bsk, bsk, sizeof(u64) * r->n_lwe * r->ggsw_words, hipMemcpyHostToDevice, ctx->stream));
            VPBS_HIP(hipMemcpyAsync(fresh.own_ksk, ksk, sizeof(u64) * r->ggsw_words, hipMemcpyHostToDevice, ctx->stream));
            entry = KeySlot{fresh.own_bsk, fresh.own_ksk};
        }
        fresh.bsk = entry.bsk;
        fresh.ksk = entry.ksk;
        VPBS_HIP(hipMemcpyAsync(r->d_table + s, &entry, sizeof entry, hipMemcpyHostToDevice, ctx->stream));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));   // the caller's key arrays, and `entry`, may go away
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        (void)vpbs::stream_sync(ctx->stream);
        ctx->release(fresh.own_bsk);
        ctx->release(fresh.own_ksk);
        return e.status;
    }
    r->slots[s] = fresh;
    ++r->used;
    *slot_out = (unsigned)s;
    return VPBS_OK;
}

int keyring_add_seeded(vpbs_keyring* r, uint64_t mask_seed, const uint64_t* bsk_bodies, const uint64_t* ksk_bodies, int bodies_on_device,
                       unsigned* slot_out, bool owner) {
    if (!r || !bsk_bodies || !ksk_bodies || !slot_out) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(r->mu);
    vpbs_ctx* ctx = r->ctx;
    if (refuse_owned(r, owner, "vpbs_keyring_add_seeded")) return VPBS_ERR_INVALID;
    size_t s = 0;
    while (s < r->max_keys && r->slots[s].used) ++s;
    if (s == r->max_keys) {
        ctx->err = "vpbs_keyring_add_seeded: all " + std::to_string(r->max_keys) + " slots of the ring are taken (max_keys)";
        return VPBS_ERR_INVALID;
    }
    if (bodies_on_device && ((((uintptr_t)bsk_bodies) | ((uintptr_t)ksk_bodies)) & 15)) {
        ctx->err = "vpbs_keyring_add_seeded: device pointers must be 16-byte aligned";
        return VPBS_ERR_INVALID;
    }
    vpbs_keyring::Slot fresh;
    fresh.used = true;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        // the slot owns the expanded key set exactly as it owns an uploaded one
        fresh.own_bsk = ctx->alloc_words((size_t)r->n_lwe * r->ggsw_words);
        fresh.own_ksk = ctx->alloc_words(r->ggsw_words);
        key_expand_device(ctx, r->prm, r->n_lwe, mask_seed, bsk_bodies, ksk_bodies, bodies_on_device, fresh.own_bsk, fresh.own_ksk);
        fresh.bsk = fresh.own_bsk;
        fresh.ksk = fresh.own_ksk;
        const KeySlot entry{fresh.bsk, fresh.ksk};
        VPBS_HIP(hipMemcpyAsync(r->d_table + s, &entry, sizeof entry, hipMemcpyHostToDevice, ctx->stream));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        (void)vpbs::stream_sync(ctx->stream);
        ctx->release(fresh.own_bsk);
        ctx->release(fresh.own_ksk);
        return e.status;
    }
    r->slots[s] = fresh;
    ++r->used;
    *slot_out = (unsigned)s;
    return VPBS_OK;
}

int keyring_remove(vpbs_keyring* r, unsigned slot, bool owner) {
    if (!r) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(r->mu);
    vpbs_ctx* ctx = r->ctx;
    if (refuse_owned(r, owner, "vpbs_keyring_remove")) return VPBS_ERR_INVALID;
    if (slot >= r->max_keys || !r->slots[slot].used) {
        ctx->err = "vpbs_keyring_remove: slot " + std::to_string(slot) + " holds no key set";
        return VPBS_ERR_INVALID;
    }
    int rc = VPBS_OK;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        const KeySlot empty{nullptr, nullptr};
        VPBS_HIP(hipMemcpyAsync(r->d_table + slot, &empty, sizeof empty, hipMemcpyHostToDevice, ctx->stream));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        rc = e.status;
    }
    // no run is in flight (the mutex; a run returns after its wait), so nothing reads the slot's memory any more
    ctx->release(r->slots[slot].own_bsk);
    ctx->release(r->slots[slot].own_ksk);
    r->slots[slot] = vpbs_keyring::Slot{};
    --r->used;
    return rc;
}
}  // namespace vpbs

extern "C" {
size_t vpbs_keyring_count(vpbs_keyring* r) {
    if (!r) return 0;
    std::lock_guard<std::mutex> lock(r->mu);
    return r->used;
}

}  // extern "C"

namespace vpbs {
namespace {
// vpbs_keyring_run (start = null) and vpbs_keyring_run_from
long keyring_run(vpbs_keyring* r, const uint64_t* cts, size_t count, const uint32_t* key_of, const uint32_t* start, const uint64_t* acc_in,
                 const uint64_t* testv, int testv_per_ct, uint64_t* out_ct, uint64_t* lwe_out, uint64_t* accs_out, int on_device) {
    if (!r) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(r->mu);
    vpbs_ctx* ctx = r->ctx;
    const char* who = start ? "vpbs_keyring_run_from" : "vpbs_keyring_run";
    if (!cts || !testv || (!out_ct && !lwe_out && !accs_out) || count > r->max_batch || (count && !key_of)) {
        ctx->err = std::string(who) + ": null cts / testv / key_of, no output, or count above max_batch";
        return VPBS_ERR_INVALID;
    }
    // every index and every start step before anything is queued
    if (!keyring_check_slots(r, key_of, count, who, "ciphertext", &ctx->err)) return VPBS_ERR_INVALID;
    if (start && !check_start_steps(start, count, r->n_lwe, acc_in, who, &ctx->err)) return VPBS_ERR_INVALID;
    if (count == 0) return 0;
    uint32_t* h_order = r->h_index.data();
    uint32_t* h_key_of = h_order + r->max_batch;
    keyring_order(key_of, count, r->max_keys, r->sort_start, h_order);
    std::memcpy(h_key_of, key_of, count * sizeof(uint32_t));
    return chain_run(r, cts, count, start, acc_in, testv, testv_per_ct, out_ct, lwe_out, accs_out, on_device,
                     [&](const u64* d_cts, const u64* d_testv, u64* d_out_ct, u64* d_lwe_out, u64* d_accs_out, const uint32_t* d_start, const u64* d_acc_in) {
                         uint32_t *d_order = r->d_index, *d_key_of = r->d_index + r->max_batch;
                         VPBS_HIP(hipMemcpyAsync(d_order, h_order, sizeof(uint32_t) * count, hipMemcpyHostToDevice, ctx->stream));
                         VPBS_HIP(hipMemcpyAsync(d_key_of, h_key_of, sizeof(uint32_t) * count, hipMemcpyHostToDevice, ctx->stream));
                         keyring_enqueue(r, d_cts, count, d_testv, testv_per_ct, d_order, d_key_of, d_out_ct, d_lwe_out, d_accs_out, d_start, d_acc_in);
                     });
}
}  // namespace
}  // namespace vpbs

extern "C" {
long vpbs_keyring_run(vpbs_keyring* r, const uint64_t* cts, size_t count, const uint32_t* key_of, const uint64_t* testv, int testv_per_ct,
                      uint64_t* out_ct, uint64_t* lwe_out, uint64_t* accs_out, int on_device) {
    return vpbs::keyring_run(r, cts, count, key_of, nullptr, nullptr, testv, testv_per_ct, out_ct, lwe_out, accs_out, on_device);
}

long vpbs_keyring_run_from(vpbs_keyring* r, const uint64_t* cts, size_t count, const uint32_t* key_of, const uint32_t* start, const uint64_t* acc_in,
                           const uint64_t* testv, int testv_per_ct, uint64_t* out_ct, uint64_t* lwe_out, uint64_t* accs_out, int on_device) {
    return vpbs::keyring_run(r, cts, count, key_of, start, acc_in, testv, testv_per_ct, out_ct, lwe_out, accs_out, on_device);
}
}  // extern "C"
