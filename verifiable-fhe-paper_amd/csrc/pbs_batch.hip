// Batched, key-resident bootstrap on gfx950: ONE launch walks the whole accumulator chain of verified_pbs
// (/root/reference/src/vtfhe/ivc_based_vpbs.rs:280-371) for a batch of LWE ciphertexts -- body rotation, n CMUX steps with bsk[x], the
// key-switching step with ksk -- one workgroup per ciphertext, and closes the loop with Glwe::partial_sample_extract
// (crypto/glwe.rs:96-113).  The arithmetic is that of the per-step kernels in tfhe.hip (mod_switch, rotated_coeff, the signed decomposition
// keeping the top ELL limbs, the reference's negacyclic NTT, glev_muls[K-1] - sum of the others, N^-1, CMUX add): exact field arithmetic on
// canonical words, so the accumulators are the same words whatever the scheduling; tfhe.hip stays the parity yardstick.
//
// LDS of a workgroup (words): acc [K][N] | out [K][N] | limbs [ELL][N].  One input polynomial at a time is decomposed into `limbs` and
// transformed; its products with the GGSW rows are accumulated into the K polynomials of `out`; after the last input polynomial `out` goes
// through the inverse transform, whose last pass multiplies by N^-1 and adds into `acc`.  Only the key rows come from memory (every
// workgroup reads the same bsk[x] at about the same time: L2 / Infinity Cache after the first).  No workgroup ever waits for another.
//
// The transforms are radix-2 butterflies in the reference's order, two stages per pass in registers (a quad of points per thread), one
// __syncthreads() per pass: 5 passes instead of 10 barriers at N = 1024, 5 + 1 at N = 2048 (pbs_chain.h, shared with pbs_keyring.hip).
#define GL_ASM_SCRATCH_LOW 1  // as tfhe.hip: few registers of its own, so the asm scratch block sits low (occupancy)
#include <cstdlib>
#include <cstring>

#include "context.h"
#include "pbs_chain.h"
#include "program_internal.h"

using vpbs::DeviceError;
using vpbs::u64;

namespace vpbs {
namespace {
struct PbsBatchArgs {
    const u64* cts;       // [count][n_lwe + 1]
    const u64* testv;     // [N] or [count][N]
    size_t testv_stride;  // 0 (shared) or N
    const u64* bsk;       // [n_lwe][K][ELL][K][N], NTT domain
    const u64* ksk;       // [K][ELL][K][N]
    const u64* roots;     // ring_table: [ROOTS | INVROOTS]
    u64 ninv;
    u64* out_ct;          // [count][K][N] or null
    u64* lwe_out;         // [count][n_lwe + 1] or null
    u64* accs_out;        // [count][n_lwe + 2][K][N] or null
    unsigned log_n, K, ELL, LOGB, n_lwe;
    // the start mode, behind everything else: the fields above keep the offsets the kernels without it (FROM = false) were compiled for
    const uint32_t* start;   // [count] or null: row b enters the chain at step start[b] (0: from the rotated test vector, as without it)
    const u64* acc_in;       // [count][K][N] or null: the accumulator after step start[b] - 1 of the rows that enter late
};

// one workgroup per ciphertext.  FROM: the start mode (a.start, a.acc_in) is an instantiation of its own, and its two arguments sit behind
// the older ones: with FROM = false the kernel compiles to the instructions it had before the start mode existed (moved
// argument offsets renumber the scalar registers, and the launches that start every row at step 0 lost 0.6 - 0.8 %)
template <unsigned T, bool FROM>
__global__ void __launch_bounds__(T) pbs_batch_kernel(PbsBatchArgs a) {
    extern __shared__ __align__(16) u64 lds[];
    const unsigned log_n = a.log_n, n = 1u << log_n, K = a.K, ELL = a.ELL, LOGB = a.LOGB, n_lwe = a.n_lwe;
    const unsigned kn = K * n;
    u64* acc = lds;             // [K][N]
    u64* out = acc + kn;        // [K][N]
    u64* limbs = out + kn;      // [ELL][N]
    const size_t b = blockIdx.x;
    const u64* ct = a.cts + b * (n_lwe + 1);
    const u64* tv = a.testv + b * a.testv_stride;
    u64* accs = a.accs_out ? a.accs_out + b * (size_t)(n_lwe + 2) * kn : nullptr;
    const size_t ggsw_words = (size_t)K * ELL * kn;
    const unsigned nl = (64 + LOGB - 1) / LOGB, tb = nl * LOGB;
    // the step this row enters at: uniform over the workgroup, so the loop bounds below stay scalar and every barrier uniform
    const unsigned k0 = FROM ? a.start[b] : 0;

    if (FROM && k0) {   // a resumed row: the accumulator after step k0 - 1, as this kernel had stored it (slots below k0 - 1 are not written)
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

    for (unsigned step = FROM && k0 ? k0 : 1; step <= n_lwe + 1; ++step) {   // k0 = n_lwe + 2: no step, the outputs are acc_in's
        const bool last = step == n_lwe + 1;
        const u64* g = last ? a.ksk : a.bsk + (size_t)(step - 1) * ggsw_words;
        const unsigned shift = last ? 0 : pb_mod_switch(ct[step - 1], log_n);
        for (unsigned p = 0; p < K; ++p) {
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
            const u64* gp = g + (size_t)p * ELL * kn;
            const bool plus = p + 1 == K;
            for (unsigned idx = 2 * threadIdx.x; idx < kn; idx += 2 * T) {
                const unsigned i = idx & (n - 1);
                u64 s0 = 0, s1 = 0;
                for (unsigned l = 0; l < ELL; ++l) {
                    const ulonglong2 kv = *reinterpret_cast<const ulonglong2*>(gp + (size_t)l * kn + idx);
                    const ulonglong2 lv = *reinterpret_cast<const ulonglong2*>(limbs + l * n + i);
                    s0 = gl::add(s0, gl::mul(lv.x, kv.x));
                    s1 = gl::add(s1, gl::mul(lv.y, kv.y));
                }
                if (p == 0) {
                    out[idx] = plus ? s0 : gl::neg(s0);
                    out[idx + 1] = plus ? s1 : gl::neg(s1);
                } else {
                    out[idx] = plus ? gl::add(out[idx], s0) : gl::sub(out[idx], s0);
                    out[idx + 1] = plus ? gl::add(out[idx + 1], s1) : gl::sub(out[idx + 1], s1);
                }
            }
            __syncthreads();
        }
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

// grid: count; GLWEs [count][K][N] in device memory
__global__ void __launch_bounds__(256) lwe_extract_kernel(const u64* __restrict__ glwe, unsigned log_n, unsigned K, unsigned n_lwe,
                                                          u64* __restrict__ lwe_out) {
    const unsigned n = 1u << log_n;
    const u64* ct = glwe + (size_t)blockIdx.x * K * n;
    u64* lw = lwe_out + (size_t)blockIdx.x * (n_lwe + 1);
    for (unsigned j = threadIdx.x; j < n_lwe; j += 256) {
        const unsigned poly = j >> log_n, c = j & (n - 1);
        lw[j] = c == 0 ? ct[(size_t)poly * n] : gl::neg(ct[(size_t)poly * n + n - c]);
    }
    if (threadIdx.x == 0) lw[n_lwe] = ct[(size_t)(K - 1) * n];
}

void report(char* err, size_t err_len, const std::string& m) {
    if (err && err_len) {
        std::strncpy(err, m.c_str(), err_len - 1);
        err[err_len - 1] = 0;
    }
}

template <unsigned T, bool FROM>
void launch_pbs_batch_from(hipStream_t s, const PbsBatchArgs& a, size_t count, size_t lds_bytes) {
    // a workgroup's dynamic LDS above the default limit is announced once per kernel
    static const hipError_t announced = hipFuncSetAttribute(reinterpret_cast<const void*>(&pbs_batch_kernel<T, FROM>),
                                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)PBS_LDS_BUDGET);
    if (announced != hipSuccess) (void)hipGetLastError();   // the launch below reports what matters
    hipLaunchKernelGGL((pbs_batch_kernel<T, FROM>), dim3((unsigned)count), dim3(T), lds_bytes, s, a);
}

template <unsigned T>
void launch_pbs_batch(hipStream_t s, const PbsBatchArgs& a, size_t count, size_t lds_bytes) {
    if (a.start) launch_pbs_batch_from<T, true>(s, a, count, lds_bytes);
    else launch_pbs_batch_from<T, false>(s, a, count, lds_bytes);
}
}  // namespace
}  // namespace vpbs

struct vpbs_bootstrapper {
    vpbs_ctx* ctx = nullptr;
    vpbs_tfhe_params prm{};
    unsigned n_lwe = 0, threads = 0, cus = 256;   // threads: 0 = chosen per run
    size_t max_batch = 0, lds_bytes = 0;
    const u64 *d_bsk = nullptr, *d_ksk = nullptr;
    u64 *d_cts = nullptr, *d_testv = nullptr, *d_out = nullptr, *d_lwe = nullptr;   // staging for host callers
    uint32_t* d_start = nullptr;   // [max_batch]: the start steps of a run_from (a host array in every mode)
    std::vector<void*> owned;

    u64* alloc(size_t words) {
        u64* d = ctx->alloc_words(words);
        owned.push_back(d);
        return d;
    }
    ~vpbs_bootstrapper() {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)vpbs::stream_sync(ctx->stream);
        for (void* p : owned) ctx->release(p);
    }
};

namespace vpbs {
void bootstrapper_shape(const vpbs_bootstrapper* b, BootstrapperShape* out) { *out = BootstrapperShape{b->ctx, b->prm, b->n_lwe, b->max_batch}; }

void bootstrapper_enqueue(vpbs_bootstrapper* b, const uint64_t* d_cts, size_t count, const uint64_t* d_testv, int testv_per_ct, uint64_t* d_out_ct,
                          uint64_t* d_lwe_out, uint64_t* d_accs_out, const uint32_t* d_start, const uint64_t* d_acc_in) {
    vpbs_ctx* ctx = b->ctx;
    const unsigned log_n = b->prm.log_N;
    const size_t n = (size_t)1 << log_n;
    PbsBatchArgs a{};
    a.cts = d_cts;
    a.testv = d_testv;
    a.out_ct = d_out_ct;
    a.lwe_out = d_lwe_out;
    a.accs_out = d_accs_out;
    a.start = d_start;
    a.acc_in = d_acc_in;
    a.testv_stride = testv_per_ct ? n : 0;
    a.bsk = b->d_bsk;
    a.ksk = b->d_ksk;
    a.roots = ctx->ring_table(log_n);
    a.ninv = gl::inv((u64)n);
    a.log_n = log_n;
    a.K = b->prm.K;
    a.ELL = b->prm.ELL;
    a.LOGB = b->prm.LOGB;
    a.n_lwe = b->n_lwe;
    {
        vpbs::Timed t(ctx, "pbs_batch");
        // Measured: 1024 threads are fastest while every ciphertext has a CU of its own; with more ciphertexts than CUs,
        // two 512-thread workgroups per CU (where two fit the LDS) overlap each other's barriers and beat one of 1024.
        const unsigned threads = b->threads ? b->threads : (count > b->cus && 2 * b->lds_bytes <= PBS_LDS_BUDGET ? 512u : 1024u);
        if (threads == 256) launch_pbs_batch<256>(ctx->stream, a, count, b->lds_bytes);
        else if (threads == 512) launch_pbs_batch<512>(ctx->stream, a, count, b->lds_bytes);
        else launch_pbs_batch<1024>(ctx->stream, a, count, b->lds_bytes);
    }
    VPBS_HIP(hipGetLastError());
}

void lwe_extract_enqueue(void* stream, const uint64_t* d_glwe, unsigned log_N, unsigned K, unsigned n_lwe, size_t count, uint64_t* d_lwe_out) {
    hipLaunchKernelGGL(lwe_extract_kernel, dim3((unsigned)count), dim3(256), 0, static_cast<hipStream_t>(stream), d_glwe, log_N, K, n_lwe, d_lwe_out);
    VPBS_HIP(hipGetLastError());
}
}  // namespace vpbs

extern "C" {
int vpbs_bootstrapper_create(vpbs_ctx* ctx, const vpbs_tfhe_params* prm, unsigned n_lwe, const uint64_t* bsk, const uint64_t* ksk,
                             int keys_on_device, size_t max_batch, vpbs_bootstrapper** out, char* err, size_t err_len) {
    using namespace vpbs;
    if (out) *out = nullptr;
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        if (ctx) ctx->err = m;
        return VPBS_ERR_INVALID;
    };
    if (!ctx || !prm || !bsk || !ksk || !out) return refuse("null argument");
    const unsigned log_n = prm->log_N, K = prm->K, ELL = prm->ELL, LOGB = prm->LOGB;
    if (log_n < 1 || log_n > 11 || K < 2 || K > 8 || LOGB < 1 || LOGB > 32) return refuse("unsupported TFHE parameters");
    if (ELL < 1 || ELL > (64 + LOGB - 1) / LOGB) return refuse("ELL exceeds the number of limbs");
    const size_t n = (size_t)1 << log_n;
    if (n_lwe == 0 || n_lwe > (K - 1) * n) return refuse("n_lwe must be 1 .. (K - 1) N: the output is extracted under a partial key");
    if (max_batch == 0 || max_batch > 65535) return refuse("max_batch must be 1 .. 65535");
    const size_t lds_bytes = (2 * (size_t)K + ELL) * n * sizeof(u64);
    if (lds_bytes > PBS_LDS_BUDGET)
        return refuse("accumulator + outputs + limbs = (2 K + ELL) N words = " + std::to_string(lds_bytes) +
                      " bytes of LDS per ciphertext, above the " + std::to_string(PBS_LDS_BUDGET) + "-byte budget of a workgroup");
    unsigned threads = 0;
    if (const char* e = getenv("VPBS_PBS_BATCH_THREADS")) {   // 256 / 512 / 1024 threads per ciphertext for every run (never changes a result)
        const int t = atoi(e);
        if (t != 256 && t != 512 && t != 1024) return refuse("VPBS_PBS_BATCH_THREADS must be 256, 512 or 1024");
        threads = (unsigned)t;
    }
    auto* b = new vpbs_bootstrapper;
    b->ctx = ctx;
    b->prm = *prm;
    b->n_lwe = n_lwe;
    b->max_batch = max_batch;
    b->lds_bytes = lds_bytes;
    b->threads = threads;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        int cus = 0;
        VPBS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        if (cus > 0) b->cus = (unsigned)cus;
        const size_t ggsw_words = (size_t)K * ELL * K * n;
        if (keys_on_device) {
            b->d_bsk = bsk;
            b->d_ksk = ksk;
        } else {
            u64* d_b = b->alloc((size_t)n_lwe * ggsw_words);
            u64* d_k = b->alloc(ggsw_words);
            VPBS_HIP(hipMemcpyAsync(d_b, bsk, sizeof(u64) * n_lwe * ggsw_words, hipMemcpyHostToDevice, ctx->stream));
            VPBS_HIP(hipMemcpyAsync(d_k, ksk, sizeof(u64) * ggsw_words, hipMemcpyHostToDevice, ctx->stream));
            b->d_bsk = d_b;
            b->d_ksk = d_k;
        }
        b->d_cts = b->alloc(max_batch * (n_lwe + 1));
        b->d_testv = b->alloc(max_batch * n);
        b->d_out = b->alloc(max_batch * K * n);
        b->d_lwe = b->alloc(max_batch * (n_lwe + 1));
        b->d_start = reinterpret_cast<uint32_t*>(b->alloc((max_batch * sizeof(uint32_t) + 7) / 8));
        (void)ctx->ring_table(log_n);
        VPBS_HIP(vpbs::stream_sync(ctx->stream));   // the caller's key arrays may go away
    } catch (const DeviceError& e) {
        report(err, err_len, e.what);
        ctx->err = e.what;
        delete b;
        return e.status;
    }
    *out = b;
    report(err, err_len, "");
    return VPBS_OK;
}

void vpbs_bootstrapper_free(vpbs_bootstrapper* b) { delete b; }

}  // extern "C"

namespace vpbs {
bool check_start_steps(const uint32_t* start, size_t count, unsigned n_lwe, const uint64_t* acc_in, const char* who, std::string* msg) {
    for (size_t i = 0; i < count; ++i) {
        if (start[i] > n_lwe + 2) {
            *msg = std::string(who) + ": start[" + std::to_string(i) + "] = " + std::to_string(start[i]) + " is beyond n_lwe + 2 = " +
                   std::to_string(n_lwe + 2) + "; ciphertext " + std::to_string(i) + " has no such step, nothing was launched";
            return false;
        }
        if (start[i] && !acc_in) {
            *msg = std::string(who) + ": start[" + std::to_string(i) + "] = " + std::to_string(start[i]) + " but acc_in is null; nothing was launched";
            return false;
        }
    }
    return true;
}

// the rows of a host acc_in that enter late, in runs of neighbours (rows with start 0 are not read)
void upload_acc_in(vpbs_ctx* ctx, u64* d_acc_in, const uint64_t* acc_in, const uint32_t* start, size_t count, size_t kn) {
    for (size_t i = 0; i < count;) {
        if (!start[i]) {
            ++i;
            continue;
        }
        size_t j = i + 1;
        while (j < count && start[j]) ++j;
        VPBS_HIP(hipMemcpyAsync(d_acc_in + i * kn, acc_in + i * kn, sizeof(u64) * (j - i) * kn, hipMemcpyHostToDevice, ctx->stream));
        i = j;
    }
}

namespace {
// vpbs_bootstrapper_run (start = null) and vpbs_bootstrapper_run_from
long bootstrapper_run(vpbs_bootstrapper* b, const uint64_t* cts, size_t count, const uint32_t* start, const uint64_t* acc_in, const uint64_t* testv,
                      int testv_per_ct, uint64_t* out_ct, uint64_t* lwe_out, uint64_t* accs_out, int on_device) {
    if (!b || !cts || !testv || (!out_ct && !lwe_out && !accs_out) || count > b->max_batch) return VPBS_ERR_INVALID;
    vpbs_ctx* ctx = b->ctx;
    // every start step before anything is queued
    if (start && !check_start_steps(start, count, b->n_lwe, acc_in, "vpbs_bootstrapper_run_from", &ctx->err)) return VPBS_ERR_INVALID;
    if (count == 0) return 0;
    const unsigned log_n = b->prm.log_N, K = b->prm.K, n_lwe = b->n_lwe;
    const size_t n = (size_t)1 << log_n, kn = K * n, ct_words = n_lwe + 1;
    u64 *d_accs = nullptr, *d_acc_stage = nullptr;
    int rc = VPBS_OK;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        const u64 *d_cts = cts, *d_testv = testv, *d_acc_in = acc_in;
        u64 *d_out_ct = out_ct, *d_lwe_out = lwe_out, *d_accs_out = accs_out;
        if (start) VPBS_HIP(hipMemcpyAsync(b->d_start, start, sizeof(uint32_t) * count, hipMemcpyHostToDevice, ctx->stream));
        if (!on_device) {
            VPBS_HIP(hipMemcpyAsync(b->d_cts, cts, sizeof(u64) * count * ct_words, hipMemcpyHostToDevice, ctx->stream));
            VPBS_HIP(hipMemcpyAsync(b->d_testv, testv, sizeof(u64) * (testv_per_ct ? count : 1) * n, hipMemcpyHostToDevice, ctx->stream));
            d_cts = b->d_cts;
            d_testv = b->d_testv;
            d_out_ct = out_ct ? b->d_out : nullptr;
            d_lwe_out = lwe_out ? b->d_lwe : nullptr;
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
        bootstrapper_enqueue(b, d_cts, count, d_testv, testv_per_ct, d_out_ct, d_lwe_out, d_accs_out, start ? b->d_start : nullptr, start ? d_acc_in : nullptr);
        if (!on_device) {
            if (out_ct) VPBS_HIP(hipMemcpyAsync(out_ct, b->d_out, sizeof(u64) * count * kn, hipMemcpyDeviceToHost, ctx->stream));
            if (lwe_out) VPBS_HIP(hipMemcpyAsync(lwe_out, b->d_lwe, sizeof(u64) * count * ct_words, hipMemcpyDeviceToHost, ctx->stream));
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
long vpbs_bootstrapper_run(vpbs_bootstrapper* b, const uint64_t* cts, size_t count, const uint64_t* testv, int testv_per_ct, uint64_t* out_ct,
                           uint64_t* lwe_out, uint64_t* accs_out, int on_device) {
    return vpbs::bootstrapper_run(b, cts, count, nullptr, nullptr, testv, testv_per_ct, out_ct, lwe_out, accs_out, on_device);
}

long vpbs_bootstrapper_run_from(vpbs_bootstrapper* b, const uint64_t* cts, size_t count, const uint32_t* start, const uint64_t* acc_in,
                                const uint64_t* testv, int testv_per_ct, uint64_t* out_ct, uint64_t* lwe_out, uint64_t* accs_out, int on_device) {
    return vpbs::bootstrapper_run(b, cts, count, start, acc_in, testv, testv_per_ct, out_ct, lwe_out, accs_out, on_device);
}

int vpbs_lwe_extract(vpbs_ctx* ctx, unsigned log_N, unsigned K, unsigned n_lwe, const uint64_t* glwe, size_t count, uint64_t* lwe_out,
                     int on_device) {
    using namespace vpbs;
    if (!ctx || !glwe || !lwe_out) return VPBS_ERR_INVALID;
    auto refuse = [&](const char* m) {
        ctx->err = m;
        return VPBS_ERR_INVALID;
    };
    if (log_N < 1 || log_N > 11 || K < 2 || K > 8) return refuse("unsupported TFHE parameters");
    const size_t n = (size_t)1 << log_N;
    if (n_lwe == 0 || n_lwe > (K - 1) * n) return refuse("n_lwe must be 1 .. (K - 1) N");
    if (count == 0) return VPBS_OK;
    if (count > 0x7fffffff) return refuse("too many ciphertexts in one call");
    u64 *d_in = nullptr, *d_out = nullptr;
    int rc = VPBS_OK;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        const u64* src = glwe;
        u64* dst = lwe_out;
        if (!on_device) {
            d_in = ctx->alloc_words(count * K * n);
            d_out = ctx->alloc_words(count * (n_lwe + 1));
            VPBS_HIP(hipMemcpyAsync(d_in, glwe, sizeof(u64) * count * K * n, hipMemcpyHostToDevice, ctx->stream));
            src = d_in;
            dst = d_out;
        }
        hipLaunchKernelGGL(lwe_extract_kernel, dim3((unsigned)count), dim3(256), 0, ctx->stream, src, log_N, K, n_lwe, dst);
        VPBS_HIP(hipGetLastError());
        if (!on_device) VPBS_HIP(hipMemcpyAsync(lwe_out, d_out, sizeof(u64) * count * (n_lwe + 1), hipMemcpyDeviceToHost, ctx->stream));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        rc = e.status;
    }
    if (d_in || d_out) {
        (void)vpbs::stream_sync(ctx->stream);
        ctx->release(d_in);
        ctx->release(d_out);
    }
    return rc;
}

int vpbs_lwe_decrypt(const uint64_t* s_lwe, const uint64_t* ct, unsigned n_lwe, uint64_t* m_out) {
    if (!s_lwe || !ct || !m_out) return VPBS_ERR_INVALID;
    u64 ip = 0;   // inner_product(s, mask), lwe.rs:4-8
    for (unsigned i = 0; i < n_lwe; ++i) ip = gl::add(ip, gl::mul(gl::canon(s_lwe[i]), gl::canon(ct[i])));
    *m_out = gl::sub(gl::canon(ct[n_lwe]), ip);
    return VPBS_OK;
}
}  // extern "C"
