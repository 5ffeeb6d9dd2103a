// Multi-output lookup gates: the primitives around the unchanged bootstrap.
//   vpbs_lwe_snap         every word of a ciphertext rounded to a multiple of 2^(64 - log2(2N) + slots_log): one lane per word, grid stride.
//   vpbs_lwe_extract_at   row i = sample extraction of coefficient index[i] of GLWE src[i]: one workgroup per output row, lanes on
//                         consecutive output words (a coalesced store; the reads of a mask polynomial run backwards through one row of N
//                         words, so a wave still touches 512 contiguous bytes but for the one wrap).
//   vpbs_lut_testv_multi  (host) the test vector that interleaves 2^slots_log tables in groups of 2^slots_log coefficients.
// With ctx NULL the first two run on the host from the same word-level functions (multi_lut.h); the CPU suite and the GPU tests' second
// yardstick.  Nothing of the bootstrap, the circuits, the provers or the verifiers changes: a snapped ciphertext is a ciphertext.
#include <algorithm>
#include <string>
#include <vector>

#include "context.h"
#include "multi_lut.h"
#include "program_internal.h"

using vpbs::DeviceError;
using vpbs::u64;
using u32 = uint32_t;

namespace vpbs {
namespace {
__global__ void __launch_bounds__(256) lwe_snap_kernel(const u64* __restrict__ in, size_t count, unsigned log_n, unsigned slots_log,
                                                       u64* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) out[i] = multi_lut::snap(in[i], log_n, slots_log);
}

// grid: rows; GLWEs [..][K][N] in device memory, index / src [rows] (wave-uniform loads: they depend on blockIdx.x alone)
__global__ void __launch_bounds__(256) lwe_extract_at_kernel(const u64* __restrict__ glwe, const u32* __restrict__ index, const u32* __restrict__ src,
                                                             unsigned log_n, unsigned K, unsigned n_lwe, u64* __restrict__ lwe_out) {
    const unsigned n = 1u << log_n, j = index[blockIdx.x];
    const u64* ct = glwe + (size_t)src[blockIdx.x] * K * n;
    u64* lw = lwe_out + (size_t)blockIdx.x * (n_lwe + 1);
    for (unsigned c = threadIdx.x; c <= n_lwe; c += 256) lw[c] = multi_lut::extract_at_word(ct, log_n, K, n_lwe, j, c);
}

int refuse(vpbs_ctx* c, const std::string& what) {
    if (c) c->err = what;
    return VPBS_ERR_INVALID;
}

// device scratch of one call, released after the stream has drained
struct Scratch {
    vpbs_ctx* c;
    std::vector<u64*> bufs;
    explicit Scratch(vpbs_ctx* ctx) : c(ctx) {}
    u64* words(size_t n) {
        bufs.push_back(c->alloc_words(n ? n : 1));
        return bufs.back();
    }
    ~Scratch() {
        if (bufs.empty()) return;
        (void)vpbs::stream_sync(c->stream);
        for (u64* p : bufs) c->release(p);
    }
};
}  // namespace

void lwe_extract_at_enqueue(void* stream, const uint64_t* d_glwe, const uint32_t* d_index, const uint32_t* d_src, unsigned log_N, unsigned K,
                            unsigned n_lwe, size_t rows, uint64_t* d_lwe_out) {
    if (rows == 0) return;
    hipLaunchKernelGGL(lwe_extract_at_kernel, dim3((unsigned)rows), dim3(256), 0, static_cast<hipStream_t>(stream), d_glwe, d_index, d_src, log_N, K,
                       n_lwe, d_lwe_out);
    VPBS_HIP(hipGetLastError());
}
}  // namespace vpbs

extern "C" {
int vpbs_lwe_snap(vpbs_ctx* c, unsigned log_N, unsigned log_slots, const uint64_t* words_in, size_t count_words, uint64_t* words_out,
                  int on_device) {
    using namespace vpbs;
    const char* who = "vpbs_lwe_snap: ";
    if (log_N < 1 || log_N > 11) return refuse(c, std::string(who) + "unsupported TFHE parameters");
    if (log_slots > log_N) return refuse(c, std::string(who) + "log_slots " + std::to_string(log_slots) + " exceeds log_N");
    if (count_words && (!words_in || !words_out)) return refuse(c, std::string(who) + "null pointer");
    if (!c && on_device) return refuse(c, std::string(who) + "device pointers need a context");
    if (count_words == 0) return VPBS_OK;
    if (!c) {
        for (size_t i = 0; i < count_words; ++i) words_out[i] = multi_lut::snap(words_in[i], log_N, log_slots);
        return VPBS_OK;
    }
    try {
        VPBS_HIP(hipSetDevice(c->device));
        Scratch tmp(c);
        const u64* d_in = words_in;
        u64* d_out = words_out;
        if (!on_device) {
            u64* d = tmp.words(count_words);
            VPBS_HIP(hipMemcpyAsync(d, words_in, sizeof(u64) * count_words, hipMemcpyHostToDevice, c->stream));
            d_in = d;
            d_out = tmp.words(count_words);
        }
        const unsigned blocks = (unsigned)std::min<size_t>((count_words + 255) / 256, 4096);
        hipLaunchKernelGGL(lwe_snap_kernel, dim3(blocks), dim3(256), 0, c->stream, d_in, count_words, log_N, log_slots, d_out);
        VPBS_HIP(hipGetLastError());
        if (!on_device) VPBS_HIP(hipMemcpyAsync(words_out, d_out, sizeof(u64) * count_words, hipMemcpyDeviceToHost, c->stream));
        VPBS_HIP(vpbs::stream_sync(c->stream));
        return VPBS_OK;
    } catch (const DeviceError& e) {
        c->err = e.what;
        return e.status;
    }
}

int vpbs_lwe_extract_at(vpbs_ctx* c, unsigned log_N, unsigned K, unsigned n_lwe, const uint64_t* glwe, size_t count, const uint32_t* index,
                        const uint32_t* src, size_t rows, uint64_t* lwe_out, int on_device) {
    using namespace vpbs;
    const char* who = "vpbs_lwe_extract_at: ";
    if (log_N < 1 || log_N > 11 || K < 2 || K > 8) return refuse(c, std::string(who) + "unsupported TFHE parameters");
    const size_t n = (size_t)1 << log_N, kn = K * n, ct_words = (size_t)n_lwe + 1;
    if (n_lwe == 0 || n_lwe > (K - 1) * n) return refuse(c, std::string(who) + "n_lwe must be 1 .. (K - 1) N");
    if (rows && (!glwe || !index || !src || !lwe_out)) return refuse(c, std::string(who) + "null pointer");
    if (!c && on_device) return refuse(c, std::string(who) + "device pointers need a context");
    if (count > 0x7fffffff || rows > 0x7fffffff) return refuse(c, std::string(who) + "too many ciphertexts in one call");
    // index and src are HOST arrays in every mode (as key_of of the key ring): they are checked before anything is queued
    for (size_t i = 0; i < rows; ++i) {
        if (index[i] >= n) return refuse(c, std::string(who) + "row " + std::to_string(i) + ": index " + std::to_string(index[i]) + " is not below N");
        if (src[i] >= count)
            return refuse(c, std::string(who) + "row " + std::to_string(i) + ": src " + std::to_string(src[i]) + " is not below count " + std::to_string(count));
    }
    if (rows == 0) return VPBS_OK;
    if (!c) {
        for (size_t i = 0; i < rows; ++i)
            for (unsigned w = 0; w <= n_lwe; ++w) lwe_out[i * ct_words + w] = multi_lut::extract_at_word(glwe + src[i] * kn, log_N, K, n_lwe, index[i], w);
        return VPBS_OK;
    }
    try {
        VPBS_HIP(hipSetDevice(c->device));
        Scratch tmp(c);
        u32* d_idx = reinterpret_cast<u32*>(tmp.words(rows));   // index [rows] | src [rows]
        VPBS_HIP(hipMemcpyAsync(d_idx, index, sizeof(u32) * rows, hipMemcpyHostToDevice, c->stream));
        VPBS_HIP(hipMemcpyAsync(d_idx + rows, src, sizeof(u32) * rows, hipMemcpyHostToDevice, c->stream));
        const u64* d_in = glwe;
        u64* d_out = lwe_out;
        if (!on_device) {
            u64* d = tmp.words(count * kn);
            VPBS_HIP(hipMemcpyAsync(d, glwe, sizeof(u64) * count * kn, hipMemcpyHostToDevice, c->stream));
            d_in = d;
            d_out = tmp.words(rows * ct_words);
        }
        lwe_extract_at_enqueue(c->stream, d_in, d_idx, d_idx + rows, log_N, K, n_lwe, rows, d_out);
        if (!on_device) VPBS_HIP(hipMemcpyAsync(lwe_out, d_out, sizeof(u64) * rows * ct_words, hipMemcpyDeviceToHost, c->stream));
        VPBS_HIP(vpbs::stream_sync(c->stream));   // index and src may go away
        return VPBS_OK;
    } catch (const DeviceError& e) {
        c->err = e.what;
        return e.status;
    }
}

int vpbs_lut_testv_multi(unsigned log_N, unsigned p, unsigned log_slots, const uint64_t* tables, uint64_t delta, uint64_t* testv) {
    if (!tables || !testv || log_N < 1 || log_N > 16 || log_slots > log_N) return VPBS_ERR_INVALID;
    const size_t n = (size_t)1 << log_N, s = (size_t)1 << log_slots;
    // the half-block shift N / (2 p) must stay a multiple of s; s = 1 leaves vpbs_lut_testv's own rule, p <= N
    if (log_slots && s * 2 * (size_t)p > n) return VPBS_ERR_INVALID;
    std::vector<u64> t(n), packed(n);
    for (size_t j = 0; j < s; ++j) {
        if (int rc = vpbs_lut_testv(log_N, p, tables + j * p, delta, t.data())) return rc;   // its refusals; testv is not written
        for (size_t q = 0; q < n; q += s) packed[q + j] = t[q];
    }
    std::copy(packed.begin(), packed.end(), testv);
    return VPBS_OK;
}
}  // extern "C"
