// Batched, key-resident bootstrap on gfx950: ONE launch walks the whole accumulator chain of verified_pbs (the reference's
// src/vtfhe/ivc_based_vpbs.rs:280-371) for a batch of LWE ciphertexts -- body rotation, n CMUX steps with bsk[x], the key-switching step
// with ksk -- one workgroup per ciphertext, and closes the loop with Glwe::partial_sample_extract (crypto/glwe.rs:96-113).  The chain
// itself -- LDS layout, decomposition, transforms, GGSW products, extraction -- is pb_chain of pbs_chain.h, shared with pbs_keyring.hip;
// its arithmetic is that of the per-step kernels in tfhe.hip: exact field arithmetic on canonical words, so the accumulators are the same
// words whatever the scheduling; tfhe.hip stays the parity yardstick.
//
// What is this file's own: the key source.  One key set per launch, in the argument struct: every workgroup reads the same bsk[x] at about
// the same time, so after the first reader the rows come from L2 / the Infinity Cache and nothing is requested ahead (pb_chain's PF = 0).
// No workgroup ever waits for another.  The host side of a run -- create's refusals, the thread rule, the launch ladder, staging -- is
// pbs_chain_host.h, shared with the key ring as well.
#define GL_ASM_SCRATCH_LOW 1  // as tfhe.hip: few registers of its own, so the asm scratch block sits low (occupancy)
#include "pbs_chain_host.h"

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

// one workgroup per ciphertext: workgroup b walks ciphertext b under the launch's key set.  FROM: the start mode, an instantiation of its
// own (pb_chain; DESIGN.md 8.12: moved argument offsets renumber the scalar registers, and the launches that start every row at step 0
// lost 0.6 - 0.8 %)
template <unsigned T, bool FROM>
__global__ void __launch_bounds__(T) pbs_batch_kernel(PbsBatchArgs a) {
    pb_chain<T, 0, FROM>(a, blockIdx.x, a.bsk, a.ksk);   // PF = 0: every workgroup reads the same rows, from L2 after the first
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

template <unsigned T, bool FROM>
struct BatchKernel {
    static constexpr auto fn = &pbs_batch_kernel<T, FROM>;
};
}  // namespace
}  // namespace vpbs

struct vpbs_bootstrapper : vpbs::ChainHost {
    const u64 *d_bsk = nullptr, *d_ksk = nullptr;
};

namespace vpbs {
void bootstrapper_shape(const vpbs_bootstrapper* b, BootstrapperShape* out) { *out = BootstrapperShape{b->ctx, b->prm, b->n_lwe, b->max_batch}; }

void bootstrapper_enqueue(vpbs_bootstrapper* b, const uint64_t* d_cts, size_t count, const uint64_t* d_testv, int testv_per_ct, uint64_t* d_out_ct,
                          uint64_t* d_lwe_out, uint64_t* d_accs_out, const uint32_t* d_start, const uint64_t* d_acc_in) {
    vpbs_ctx* ctx = b->ctx;
    PbsBatchArgs a{};
    chain_fill_args(b, &a, d_cts, d_testv, testv_per_ct, d_out_ct, d_lwe_out, d_accs_out, d_start, d_acc_in);
    a.bsk = b->d_bsk;
    a.ksk = b->d_ksk;
    {
        vpbs::Timed t(ctx, "pbs_batch");
        chain_launch<BatchKernel>(ctx->stream, a, count, b->chain_threads(count), b->lds_bytes);
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
    size_t lds_bytes = 0;
    unsigned threads = 0;
    std::string why;
    if (!chain_shape_check(prm, n_lwe, max_batch, &lds_bytes, &threads, &why)) return refuse(why);
    auto* b = new vpbs_bootstrapper;
    b->ctx = ctx;
    b->prm = *prm;
    b->n_lwe = n_lwe;
    b->max_batch = max_batch;
    b->lds_bytes = lds_bytes;
    b->threads = threads;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        const size_t ggsw_words = ((size_t)prm->K * prm->ELL * prm->K) << prm->log_N;
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
        b->alloc_staging();
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
    // every start step before anything is queued
    if (start && !check_start_steps(start, count, b->n_lwe, acc_in, "vpbs_bootstrapper_run_from", &b->ctx->err)) return VPBS_ERR_INVALID;
    if (count == 0) return 0;
    return chain_run(b, cts, count, start, acc_in, testv, testv_per_ct, out_ct, lwe_out, accs_out, on_device,
                     [&](const u64* d_cts, const u64* d_testv, u64* d_out_ct, u64* d_lwe_out, u64* d_accs_out, const uint32_t* d_start, const u64* d_acc_in) {
                         bootstrapper_enqueue(b, d_cts, count, d_testv, testv_per_ct, d_out_ct, d_lwe_out, d_accs_out, d_start, d_acc_in);
                     });
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
        lwe_extract_enqueue(ctx->stream, src, log_N, K, n_lwe, count, dst);
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
