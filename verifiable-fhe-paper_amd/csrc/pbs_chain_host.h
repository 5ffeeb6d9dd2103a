// The host side of a bootstrap-chain launch, stated once for the Bootstrapper (pbs_batch.hip) and the key ring (pbs_keyring.hip): what the two
// objects hold in common (shape, launch geometry, staging buffers for host callers), the refusals of a create, the thread rule, the launch
// ladder over a kernel's instantiations and the run itself -- stage, enqueue, download, wait, release.  What differs stays in the two files:
// where the keys come from and what the launch is called.  Library-internal, like program_internal.h.
#pragma once
#include <cstdlib>
#include <string>
#include <vector>

#include "context.h"
#include "pbs_chain.h"
#include "program_internal.h"

namespace vpbs {
struct ChainHost {
    vpbs_ctx* ctx = nullptr;
    vpbs_tfhe_params prm{};
    unsigned n_lwe = 0, threads = 0, cus = 256;   // threads: 0 = chosen per run
    size_t max_batch = 0, lds_bytes = 0;
    u64 *d_cts = nullptr, *d_testv = nullptr, *d_out = nullptr, *d_lwe = nullptr;   // staging for host callers
    uint32_t* d_start = nullptr;   // [max_batch]: the start steps of a run_from (a host array in every mode)
    std::vector<void*> owned;

    u64* alloc(size_t words) {
        u64* d = ctx->alloc_words(words);
        owned.push_back(d);
        return d;
    }
    // the CU count and the staging buffers of a create; the caller holds the device
    void alloc_staging() {
        int n_cus = 0;
        VPBS_HIP(hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        if (n_cus > 0) cus = (unsigned)n_cus;
        const size_t n = (size_t)1 << prm.log_N;
        d_cts = alloc(max_batch * (n_lwe + 1));
        d_testv = alloc(max_batch * n);
        d_out = alloc(max_batch * prm.K * n);
        d_lwe = alloc(max_batch * (n_lwe + 1));
        d_start = reinterpret_cast<uint32_t*>(alloc((max_batch * sizeof(uint32_t) + 7) / 8));
        (void)ctx->ring_table(prm.log_N);
    }
    // Measured: 1024 threads are fastest while every ciphertext has a CU of its own; with more ciphertexts than CUs,
    // two 512-thread workgroups per CU (where two fit the LDS) overlap each other's barriers and beat one of 1024.
    unsigned chain_threads(size_t count) const { return threads ? threads : (count > cus && 2 * lds_bytes <= PBS_LDS_BUDGET ? 512u : 1024u); }
    ~ChainHost() {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)stream_sync(ctx->stream);
        for (void* p : owned) ctx->release(p);
    }
};

// The refusals of vpbs_bootstrapper_create and vpbs_keyring_create: false with the message in *msg; else the LDS bytes of a workgroup and the
// thread count the environment fixes (0: chosen per run).
inline bool chain_shape_check(const vpbs_tfhe_params* prm, unsigned n_lwe, size_t max_batch, size_t* lds_bytes, unsigned* threads, std::string* msg) {
    const unsigned log_n = prm->log_N, K = prm->K, ELL = prm->ELL, LOGB = prm->LOGB;
    auto refuse = [&](const std::string& m) {
        *msg = m;
        return false;
    };
    if (log_n < 1 || log_n > 11 || K < 2 || K > 8 || LOGB < 1 || LOGB > 32) return refuse("unsupported TFHE parameters");
    if (ELL < 1 || ELL > (64 + LOGB - 1) / LOGB) return refuse("ELL exceeds the number of limbs");
    const size_t n = (size_t)1 << log_n;
    if (n_lwe == 0 || n_lwe > (K - 1) * n) return refuse("n_lwe must be 1 .. (K - 1) N: the output is extracted under a partial key");
    if (max_batch == 0 || max_batch > 65535) return refuse("max_batch must be 1 .. 65535");
    *lds_bytes = (2 * (size_t)K + ELL) * n * sizeof(u64);
    if (*lds_bytes > PBS_LDS_BUDGET)
        return refuse("accumulator + outputs + limbs = (2 K + ELL) N words = " + std::to_string(*lds_bytes) +
                      " bytes of LDS per ciphertext, above the " + std::to_string(PBS_LDS_BUDGET) + "-byte budget of a workgroup");
    *threads = 0;
    if (const char* e = getenv("VPBS_PBS_BATCH_THREADS")) {   // 256 / 512 / 1024 threads per ciphertext for every run (never changes a result)
        const int t = atoi(e);
        if (t != 256 && t != 512 && t != 1024) return refuse("VPBS_PBS_BATCH_THREADS must be 256, 512 or 1024");
        *threads = (unsigned)t;
    }
    return true;
}

// the fields PbsBatchArgs and PbsKeyringArgs have in common (the ones pb_chain reads)
template <class Args>
void chain_fill_args(const ChainHost* h, Args* a, const uint64_t* d_cts, const uint64_t* d_testv, int testv_per_ct, uint64_t* d_out_ct,
                     uint64_t* d_lwe_out, uint64_t* d_accs_out, const uint32_t* d_start, const uint64_t* d_acc_in) {
    const unsigned log_n = h->prm.log_N;
    const size_t n = (size_t)1 << log_n;
    a->cts = d_cts;
    a->testv = d_testv;
    a->testv_stride = testv_per_ct ? n : 0;
    a->roots = h->ctx->ring_table(log_n);
    a->ninv = gl::inv((u64)n);
    a->out_ct = d_out_ct;
    a->lwe_out = d_lwe_out;
    a->accs_out = d_accs_out;
    a->log_n = log_n;
    a->K = h->prm.K;
    a->ELL = h->prm.ELL;
    a->LOGB = h->prm.LOGB;
    a->n_lwe = h->n_lwe;
    a->start = d_start;
    a->acc_in = d_acc_in;
}

// The launch ladder.  Kernel<T, FROM>::fn is a __global__ function of one Args by value, for T = 256, 512, 1024 threads and both start modes;
// the start mode is the instantiation with FROM = (a.start != null).
template <class Args, void (*Fn)(Args)>
void chain_launch_one(hipStream_t s, const Args& a, size_t count, unsigned threads, size_t lds_bytes) {
    // a workgroup's dynamic LDS above the default limit is announced once per kernel
    static const hipError_t announced = hipFuncSetAttribute(reinterpret_cast<const void*>(Fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PBS_LDS_BUDGET);
    if (announced != hipSuccess) (void)hipGetLastError();   // the launch below reports what matters
    hipLaunchKernelGGL(Fn, dim3((unsigned)count), dim3(threads), lds_bytes, s, a);
}

template <template <unsigned, bool> class Kernel, unsigned T, class Args>
void chain_launch_from(hipStream_t s, const Args& a, size_t count, size_t lds_bytes) {
    if (a.start) chain_launch_one<Args, Kernel<T, true>::fn>(s, a, count, T, lds_bytes);
    else chain_launch_one<Args, Kernel<T, false>::fn>(s, a, count, T, lds_bytes);
}

template <template <unsigned, bool> class Kernel, class Args>
void chain_launch(hipStream_t s, const Args& a, size_t count, unsigned threads, size_t lds_bytes) {
    if (threads == 256) chain_launch_from<Kernel, 256>(s, a, count, lds_bytes);
    else if (threads == 512) chain_launch_from<Kernel, 512>(s, a, count, lds_bytes);
    else chain_launch_from<Kernel, 1024>(s, a, count, lds_bytes);
}

// One run for a caller whose arguments are checked and whose count is not 0 (start = null: every row from step 0): with host arrays, upload
// cts / testv / start (and accs_out, acc_in of a run_from) into the staging buffers, then
//   enqueue(d_cts, d_testv, d_out_ct, d_lwe_out, d_accs_out, d_start, d_acc_in)
// queues the launch on the context's stream, then download the outputs asked for; wait; release what was staged for this run alone.
// -> count, or VPBS_ERR_OOM / VPBS_ERR_DEVICE with the message in the context.
template <class Enqueue>
long chain_run(ChainHost* h, const uint64_t* cts, size_t count, const uint32_t* start, const uint64_t* acc_in, const uint64_t* testv, int testv_per_ct,
               uint64_t* out_ct, uint64_t* lwe_out, uint64_t* accs_out, int on_device, Enqueue enqueue) {
    vpbs_ctx* ctx = h->ctx;
    const unsigned n_lwe = h->n_lwe;
    const size_t n = (size_t)1 << h->prm.log_N, kn = h->prm.K * n, ct_words = n_lwe + 1;
    u64 *d_accs = nullptr, *d_acc_stage = nullptr;
    int rc = VPBS_OK;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        const u64 *d_cts = cts, *d_testv = testv, *d_acc_in = acc_in;
        u64 *d_out_ct = out_ct, *d_lwe_out = lwe_out, *d_accs_out = accs_out;
        if (start) VPBS_HIP(hipMemcpyAsync(h->d_start, start, sizeof(uint32_t) * count, hipMemcpyHostToDevice, ctx->stream));
        if (!on_device) {
            VPBS_HIP(hipMemcpyAsync(h->d_cts, cts, sizeof(u64) * count * ct_words, hipMemcpyHostToDevice, ctx->stream));
            VPBS_HIP(hipMemcpyAsync(h->d_testv, testv, sizeof(u64) * (testv_per_ct ? count : 1) * n, hipMemcpyHostToDevice, ctx->stream));
            d_cts = h->d_cts;
            d_testv = h->d_testv;
            d_out_ct = out_ct ? h->d_out : nullptr;
            d_lwe_out = lwe_out ? h->d_lwe : nullptr;
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
        enqueue(d_cts, d_testv, d_out_ct, d_lwe_out, d_accs_out, start ? h->d_start : nullptr, start ? d_acc_in : nullptr);
        if (!on_device) {
            if (out_ct) VPBS_HIP(hipMemcpyAsync(out_ct, h->d_out, sizeof(u64) * count * kn, hipMemcpyDeviceToHost, ctx->stream));
            if (lwe_out) VPBS_HIP(hipMemcpyAsync(lwe_out, h->d_lwe, sizeof(u64) * count * ct_words, hipMemcpyDeviceToHost, ctx->stream));
            if (accs_out)
                VPBS_HIP(hipMemcpyAsync(accs_out, d_accs, sizeof(u64) * count * (n_lwe + 2) * kn, hipMemcpyDeviceToHost, ctx->stream));
        }
        VPBS_HIP(stream_sync(ctx->stream));
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        rc = e.status == VPBS_ERR_OOM ? VPBS_ERR_OOM : VPBS_ERR_DEVICE;
    }
    if (d_accs || d_acc_stage) {
        (void)stream_sync(ctx->stream);
        ctx->release(d_accs);
        ctx->release(d_acc_stage);
    }
    return rc == VPBS_OK ? (long)count : rc;
}
}  // namespace vpbs
