// Bootstrapping a mixed batch under MANY resident key sets in one launch (vpbs_keyring_*): the chain of pbs_batch.hip, one workgroup per
// ciphertext, but every workgroup takes ITS ciphertext's key set from a table in device memory.  Workgroup w handles ciphertext order[w]
// under slot key_of[order[w]]; the outputs go to the caller's positions, so the permutation never shows.  LDS as pbs_batch.hip:
// acc [K][N] | out [K][N] | limbs [ELL][N]; transforms, mod switch and rotation are the shared ones of pbs_chain.h, and every value goes
// through the same canonical-in, canonical-out field operations in the same order, so the words are pbs_batch_kernel's.
//
// Key rows.  With one key set per launch the rows of bsk[x] are in L2 / the Infinity Cache after the first reader; with a key set per
// workgroup they come from HBM, so their latency has to be hidden inside the workgroup: the ELL K N words g[p][.][.] that the product loop
// of input polynomial p consumes are requested into a register array BEFORE that polynomial is decomposed and transformed, and consumed
// after; the rows of p = 0 of the next step are requested before the inverse transform of this one.  The array has 4 or 8 16-byte entries
// per thread; a shape that needs more (ELL K N / (2 T) > 8) reads in the loop as pbs_batch_kernel does.  No workgroup waits for another.
#define GL_ASM_SCRATCH_LOW 1  // as pbs_batch.hip
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "context.h"
#include "pbs_chain.h"
#include "program_internal.h"

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

// Request the rows g[p][l][.] at this thread's points into pf: entry trip * ELL + l for the trip-th pair of points.  Branch-free, so that
// the loads go out back to back: an entry beyond the thread's last pair (idx >= kn) reads pair 0 of its row instead and is never used.
template <unsigned T, unsigned PF>
__device__ __forceinline__ void kr_prefetch(ulonglong2 (&pf)[PF ? PF : 1], const u64* __restrict__ gp, unsigned kn, unsigned ELL) {
    unsigned l = 0, idx = 2 * threadIdx.x;
#pragma unroll
    for (unsigned j = 0; j < PF; ++j) {
        pf[j] = *reinterpret_cast<const ulonglong2*>(gp + (size_t)l * kn + (idx < kn ? idx : 0));
        if (++l == ELL) {
            l = 0;
            idx += 2 * T;
        }
    }
}

// One workgroup per ciphertext.  PF: 16-byte key words a thread holds ahead per input polynomial, chosen by the host as the smallest of
// 4 and 8 that covers ELL * ceil(K N / (2 T)) (4 at the paper's shape with 1024 threads, 8 with 512); 0: no room, read in the loop.
// FROM: the start mode (a.start, a.acc_in), an instantiation of its own as in pbs_batch_kernel.
template <unsigned T, unsigned PF, bool FROM>
__global__ void __launch_bounds__(T) pbs_keyring_kernel(PbsKeyringArgs a) {
    extern __shared__ __align__(16) u64 lds[];
    const unsigned log_n = a.log_n, n = 1u << log_n, K = a.K, ELL = a.ELL, LOGB = a.LOGB, n_lwe = a.n_lwe;
    const unsigned kn = K * n;
    u64* acc = lds;             // [K][N]
    u64* out = acc + kn;        // [K][N]
    u64* limbs = out + kn;      // [ELL][N]
    // wave-uniform: this workgroup's ciphertext and its key set
    const size_t b = a.order[blockIdx.x];
    const KeySlot key = a.table[a.key_of[b]];
    const u64* ct = a.cts + b * (n_lwe + 1);
    const u64* tv = a.testv + b * a.testv_stride;
    u64* accs = a.accs_out ? a.accs_out + b * (size_t)(n_lwe + 2) * kn : nullptr;
    const size_t ggsw_words = (size_t)K * ELL * kn;
    const unsigned nl = (64 + LOGB - 1) / LOGB, tb = nl * LOGB;
    constexpr bool ahead = PF != 0;
    ulonglong2 pf[PF ? PF : 1];
    // the step this ciphertext enters at (pbs_batch_kernel): uniform over the workgroup
    const unsigned k0 = FROM ? a.start[b] : 0;
    const unsigned first = FROM && k0 ? k0 : 1;

    // the rows of the first step that runs, ahead of the accumulator's load (k0 = n_lwe + 2 runs no step: the rows of ksk, never used)
    if constexpr (ahead) kr_prefetch<T, PF>(pf, FROM && first > n_lwe ? key.ksk : key.bsk + (size_t)(first - 1) * ggsw_words, kn, ELL);
    if (FROM && k0) {   // a resumed ciphertext: the accumulator after step k0 - 1 (slots below k0 - 1 are not written)
        const u64* in = a.acc_in + b * kn;
        u64* slot = accs ? accs + (size_t)(k0 - 1) * kn : nullptr;
        for (unsigned idx = threadIdx.x; idx < kn; idx += T) {
            const u64 v = in[idx];
            acc[idx] = v;
            if (slot) slot[idx] = v;
        }
    } else {   // step 0: acc_init = (0, .., 0, testv) rotated by -body (ivc_based_vpbs.rs:106-111,122)
        const unsigned shift = pb_mod_switch(gl::neg(ct[n_lwe]), log_n);
        for (unsigned idx = threadIdx.x; idx < kn; idx += T) {
            const unsigned i = idx & (n - 1);
            const u64 v = idx >= kn - n ? pb_rotated_coeff(tv, n, shift, i) : 0;
            acc[idx] = v;
            if (accs) accs[idx] = v;
        }
    }
    __syncthreads();

    for (unsigned step = first; step <= n_lwe + 1; ++step) {
        const bool last = step == n_lwe + 1;
        const u64* g = last ? key.ksk : key.bsk + (size_t)(step - 1) * ggsw_words;
        const unsigned shift = last ? 0 : pb_mod_switch(ct[step - 1], log_n);
        for (unsigned p = 0; p < K; ++p) {
            const u64* gp = g + (size_t)p * ELL * kn;
            if (ahead && p) kr_prefetch<T, PF>(pf, gp, kn, ELL);   // p = 0 was requested before the previous inverse transform
            const u64* poly = acc + (size_t)p * n;
            for (unsigned i = threadIdx.x; i < n; i += T) {
                // xprod_in = last ? acc : rotate(acc, mask) - acc (ivc_based_vpbs.rs:113-116), decomposed (glwe_poly.rs:28-50)
                const u64 x = last ? poly[i] : gl::sub(pb_rotated_coeff(poly, n, shift, i), poly[i]);
                const unsigned sgn = tb <= 64 ? (unsigned)((x >> (tb - 1)) & 1) : 0;
                const u64 xc = sgn ? gl::neg(x) : x;
                unsigned carry = 0;
                for (unsigned l = 0; l < nl; ++l) {
                    const unsigned lo_bit = l * LOGB;
                    const u64 k = (lo_bit < 64 ? (xc >> lo_bit) : 0) & (((u64)1 << LOGB) - 1);
                    const u64 kw = k + carry;
                    carry = (unsigned)((k >> (LOGB - 1)) & 1);
                    const u64 bal = gl::sub(kw, (u64)carry << LOGB);
                    if (l + ELL >= nl) limbs[(l + ELL - nl) * n + i] = sgn ? gl::neg(bal) : bal;
                }
            }
            __syncthreads();
            pb_forward<T>(limbs, log_n, ELL, a.roots);
            // out[r] (+/-)= sum_l limbs_hat[l] * g[p][l][r]: + for the last GLEV, - for the others (ggsw_ct.rs:109-111); two points per thread
            const bool plus = p + 1 == K;
            auto store = [&](unsigned idx, u64 s0, u64 s1) {
                if (p == 0) {
                    out[idx] = plus ? s0 : gl::neg(s0);
                    out[idx + 1] = plus ? s1 : gl::neg(s1);
                } else {
                    out[idx] = plus ? gl::add(out[idx], s0) : gl::sub(out[idx], s0);
                    out[idx + 1] = plus ? gl::add(out[idx + 1], s1) : gl::sub(out[idx + 1], s1);
                }
            };
            if constexpr (ahead) {
                unsigned l = 0, idx = 2 * threadIdx.x;
                u64 s0 = 0, s1 = 0;
#pragma unroll
                for (unsigned j = 0; j < PF; ++j) {
                    const ulonglong2 kv = pf[j];
                    const ulonglong2 lv = *reinterpret_cast<const ulonglong2*>(limbs + l * n + (idx & (n - 1)));
                    s0 = gl::add(s0, gl::mul(lv.x, kv.x));
                    s1 = gl::add(s1, gl::mul(lv.y, kv.y));
                    if (++l == ELL) {
                        if (idx < kn) store(idx, s0, s1);
                        l = 0;
                        idx += 2 * T;
                        s0 = s1 = 0;
                    }
                }
            } else {
                for (unsigned idx = 2 * threadIdx.x; idx < kn; idx += 2 * T) {
                    const unsigned i = idx & (n - 1);
                    u64 s0 = 0, s1 = 0;
                    for (unsigned l = 0; l < ELL; ++l) {
                        const ulonglong2 kv = *reinterpret_cast<const ulonglong2*>(gp + (size_t)l * kn + idx);
                        const ulonglong2 lv = *reinterpret_cast<const ulonglong2*>(limbs + l * n + i);
                        s0 = gl::add(s0, gl::mul(lv.x, kv.x));
                        s1 = gl::add(s1, gl::mul(lv.y, kv.y));
                    }
                    store(idx, s0, s1);
                }
            }
            __syncthreads();
        }
        // the first rows of the next step, ahead of the inverse transform
        if (ahead && !last) kr_prefetch<T, PF>(pf, step == n_lwe ? key.ksk : g + ggsw_words, kn, ELL);
        u64* accs_step = accs ? accs + (size_t)step * kn : nullptr;
        pb_inverse<T>(out, log_n, K, a.roots + n, a.ninv, [&](unsigned idx, u64 v) {
            const u64 r = last ? v : gl::add(v, acc[idx]);   // CMUX add
            acc[idx] = r;
            if (accs_step) accs_step[idx] = r;
        });
    }

    if (a.out_ct)
        for (unsigned idx = threadIdx.x; idx < kn; idx += T) a.out_ct[b * kn + idx] = acc[idx];
    if (a.lwe_out) {   // partial_sample_extract(n_lwe): a_j[0], -a_j[N-1], .., -a_j[1] over the mask polynomials, then body[0]
        u64* lw = a.lwe_out + b * (n_lwe + 1);
        for (unsigned j = threadIdx.x; j < n_lwe; j += T) {
            const unsigned poly = j >> log_n, c = j & (n - 1);
            lw[j] = c == 0 ? acc[poly * n] : gl::neg(acc[poly * n + n - c]);
        }
        if (threadIdx.x == 0) lw[n_lwe] = acc[kn - n];
    }
}

template <unsigned T, unsigned PF, bool FROM>
void launch_pbs_keyring_from(hipStream_t s, const PbsKeyringArgs& a, size_t count, size_t lds_bytes) {
    // a workgroup's dynamic LDS above the default limit is announced once per kernel
    static const hipError_t announced = hipFuncSetAttribute(reinterpret_cast<const void*>(&pbs_keyring_kernel<T, PF, FROM>),
                                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)PBS_LDS_BUDGET);
    if (announced != hipSuccess) (void)hipGetLastError();   // the launch below reports what matters
    hipLaunchKernelGGL((pbs_keyring_kernel<T, PF, FROM>), dim3((unsigned)count), dim3(T), lds_bytes, s, a);
}

template <unsigned T, unsigned PF>
void launch_pbs_keyring_pf(hipStream_t s, const PbsKeyringArgs& a, size_t count, size_t lds_bytes) {
    if (a.start) launch_pbs_keyring_from<T, PF, true>(s, a, count, lds_bytes);
    else launch_pbs_keyring_from<T, PF, false>(s, a, count, lds_bytes);
}

template <unsigned T>
void launch_pbs_keyring(hipStream_t s, const PbsKeyringArgs& a, size_t count, size_t lds_bytes) {
    const unsigned kn = a.K << a.log_n;
    const unsigned total = a.ELL * ((kn + 2 * T - 1) / (2 * T));   // 16-byte key words per thread and input polynomial
    if (total <= 4) launch_pbs_keyring_pf<T, 4>(s, a, count, lds_bytes);
    else if (total <= 8) launch_pbs_keyring_pf<T, 8>(s, a, count, lds_bytes);
    else launch_pbs_keyring_pf<T, 0>(s, a, count, lds_bytes);
}

void report(char* err, size_t err_len, const std::string& m) {
    if (err && err_len) {
        std::strncpy(err, m.c_str(), err_len - 1);
        err[err_len - 1] = 0;
    }
}

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

struct vpbs_keyring {
    vpbs_ctx* ctx = nullptr;
    vpbs_tfhe_params prm{};
    unsigned n_lwe = 0, threads = 0, cus = 256;   // threads: 0 = chosen per run
    size_t max_keys = 0, max_batch = 0, lds_bytes = 0, ggsw_words = 0;
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
    uint32_t* d_index = nullptr;        // order [max_batch] | key_of [max_batch] | start [max_batch]
    std::vector<uint32_t> h_index, sort_start;
    u64 *d_cts = nullptr, *d_testv = nullptr, *d_out = nullptr, *d_lwe = nullptr;   // staging for host callers
    std::vector<void*> owned;

    u64* alloc(size_t words) {
        u64* d = ctx->alloc_words(words);
        owned.push_back(d);
        return d;
    }
    ~vpbs_keyring() {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)vpbs::stream_sync(ctx->stream);
        for (void* p : owned) ctx->release(p);
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
    const unsigned log_n = r->prm.log_N;
    const size_t n = (size_t)1 << log_n;
    PbsKeyringArgs a{};
    a.cts = d_cts;
    a.testv = d_testv;
    a.testv_stride = testv_per_ct ? n : 0;
    a.table = r->d_table;
    a.order = d_order;
    a.key_of = d_key_of;
    a.roots = ctx->ring_table(log_n);
    a.ninv = gl::inv((u64)n);
    a.out_ct = d_out_ct;
    a.lwe_out = d_lwe_out;
    a.accs_out = d_accs_out;
    a.start = d_start;
    a.acc_in = d_acc_in;
    a.log_n = log_n;
    a.K = r->prm.K;
    a.ELL = r->prm.ELL;
    a.LOGB = r->prm.LOGB;
    a.n_lwe = r->n_lwe;
    {
        vpbs::Timed t(ctx, "pbs_keyring");
        // the Bootstrapper's rule: 1024 threads while every ciphertext has a CU of its own, two 512-thread workgroups
        // per CU above that where two fit the LDS
        const unsigned threads = r->threads ? r->threads : (count > r->cus && 2 * r->lds_bytes <= PBS_LDS_BUDGET ? 512u : 1024u);
        if (threads == 256) launch_pbs_keyring<256>(ctx->stream, a, count, r->lds_bytes);
        else if (threads == 512) launch_pbs_keyring<512>(ctx->stream, a, count, r->lds_bytes);
        else launch_pbs_keyring<1024>(ctx->stream, a, count, r->lds_bytes);
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
    const unsigned log_n = prm->log_N, K = prm->K, ELL = prm->ELL, LOGB = prm->LOGB;
    if (log_n < 1 || log_n > 11 || K < 2 || K > 8 || LOGB < 1 || LOGB > 32) return refuse("unsupported TFHE parameters");
    if (ELL < 1 || ELL > (64 + LOGB - 1) / LOGB) return refuse("ELL exceeds the number of limbs");
    const size_t n = (size_t)1 << log_n;
    if (n_lwe == 0 || n_lwe > (K - 1) * n) return refuse("n_lwe must be 1 .. (K - 1) N: the output is extracted under a partial key");
    if (max_batch == 0 || max_batch > 65535) return refuse("max_batch must be 1 .. 65535");
    if (max_keys == 0 || max_keys > 65535) return refuse("max_keys must be 1 .. 65535");
    const size_t lds_bytes = (2 * (size_t)K + ELL) * n * sizeof(u64);
    if (lds_bytes > PBS_LDS_BUDGET)
        return refuse("accumulator + outputs + limbs = (2 K + ELL) N words = " + std::to_string(lds_bytes) +
                      " bytes of LDS per ciphertext, above the " + std::to_string(PBS_LDS_BUDGET) + "-byte budget of a workgroup");
    unsigned threads = 0;
    if (const char* e = getenv("VPBS_PBS_BATCH_THREADS")) {   // as the Bootstrapper: never changes a result
        const int t = atoi(e);
        if (t != 256 && t != 512 && t != 1024) return refuse("VPBS_PBS_BATCH_THREADS must be 256, 512 or 1024");
        threads = (unsigned)t;
    }
    auto* r = new vpbs_keyring;
    r->ctx = ctx;
    r->prm = *prm;
    r->n_lwe = n_lwe;
    r->max_keys = max_keys;
    r->max_batch = max_batch;
    r->lds_bytes = lds_bytes;
    r->threads = threads;
    r->ggsw_words = (size_t)K * ELL * K * n;
    r->slots.resize(max_keys);
    r->h_index.resize(2 * max_batch);
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        int cus = 0;
        VPBS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        if (cus > 0) r->cus = (unsigned)cus;
        r->d_table = reinterpret_cast<KeySlot*>(r->alloc((max_keys * sizeof(KeySlot) + 7) / 8));
        r->d_index = reinterpret_cast<uint32_t*>(r->alloc((3 * max_batch * sizeof(uint32_t) + 7) / 8));
        VPBS_HIP(hipMemsetAsync(r->d_table, 0, max_keys * sizeof(KeySlot), ctx->stream));
        r->d_cts = r->alloc(max_batch * (n_lwe + 1));
        r->d_testv = r->alloc(max_batch * n);
        r->d_out = r->alloc(max_batch * K * n);
        r->d_lwe = r->alloc(max_batch * (n_lwe + 1));
        (void)ctx->ring_table(log_n);
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
    const unsigned log_n = r->prm.log_N, K = r->prm.K, n_lwe = r->n_lwe;
    const size_t n = (size_t)1 << log_n, kn = K * n, ct_words = n_lwe + 1;
    uint32_t* h_order = r->h_index.data();
    uint32_t* h_key_of = h_order + r->max_batch;
    keyring_order(key_of, count, r->max_keys, r->sort_start, h_order);
    std::memcpy(h_key_of, key_of, count * sizeof(uint32_t));
    u64 *d_accs = nullptr, *d_acc_stage = nullptr;
    uint32_t* d_start = r->d_index + 2 * r->max_batch;
    int rc = VPBS_OK;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        const u64 *d_cts = cts, *d_testv = testv, *d_acc_in = acc_in;
        u64 *d_out_ct = out_ct, *d_lwe_out = lwe_out, *d_accs_out = accs_out;
        VPBS_HIP(hipMemcpyAsync(r->d_index, h_order, sizeof(uint32_t) * count, hipMemcpyHostToDevice, ctx->stream));
        VPBS_HIP(hipMemcpyAsync(r->d_index + r->max_batch, h_key_of, sizeof(uint32_t) * count, hipMemcpyHostToDevice, ctx->stream));
        if (start) VPBS_HIP(hipMemcpyAsync(d_start, start, sizeof(uint32_t) * count, hipMemcpyHostToDevice, ctx->stream));
        if (!on_device) {
            VPBS_HIP(hipMemcpyAsync(r->d_cts, cts, sizeof(u64) * count * ct_words, hipMemcpyHostToDevice, ctx->stream));
            VPBS_HIP(hipMemcpyAsync(r->d_testv, testv, sizeof(u64) * (testv_per_ct ? count : 1) * n, hipMemcpyHostToDevice, ctx->stream));
            d_cts = r->d_cts;
            d_testv = r->d_testv;
            d_out_ct = out_ct ? r->d_out : nullptr;
            d_lwe_out = lwe_out ? r->d_lwe : nullptr;
            if (accs_out) {
                d_accs_out = d_accs = ctx->alloc_words(count * (n_lwe + 2) * kn);
                // a resumed row leaves the slots below its start as the caller has them
                if (start) VPBS_HIP(hipMemcpyAsync(d_accs, accs_out, sizeof(u64) * count * (n_lwe + 2) * kn, hipMemcpyHostToDevice, ctx->stream));
            }
            if (start && acc_in) {
                d_acc_in = d_acc_stage = ctx->alloc_words(count * kn);
                upload_acc_in(ctx, d_acc_stage, acc_in, start, count, kn);
            }
        }
        keyring_enqueue(r, d_cts, count, d_testv, testv_per_ct, r->d_index, r->d_index + r->max_batch, d_out_ct, d_lwe_out, d_accs_out,
                        start ? d_start : nullptr, start ? d_acc_in : nullptr);
        if (!on_device) {
            if (out_ct) VPBS_HIP(hipMemcpyAsync(out_ct, r->d_out, sizeof(u64) * count * kn, hipMemcpyDeviceToHost, ctx->stream));
            if (lwe_out) VPBS_HIP(hipMemcpyAsync(lwe_out, r->d_lwe, sizeof(u64) * count * ct_words, hipMemcpyDeviceToHost, ctx->stream));
            if (accs_out)
                VPBS_HIP(hipMemcpyAsync(accs_out, d_accs, sizeof(u64) * count * (n_lwe + 2) * kn, hipMemcpyDeviceToHost, ctx->stream));
        }
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        rc = e.status == VPBS_ERR_OOM ? VPBS_ERR_OOM : VPBS_ERR_DEVICE;
    }
    if (d_accs || d_acc_stage) {
        (void)vpbs::stream_sync(ctx->stream);
        ctx->release(d_accs);
        ctx->release(d_acc_stage);
    }
    return rc == VPBS_OK ? (long)count : rc;
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
