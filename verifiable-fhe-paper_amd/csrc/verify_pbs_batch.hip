// Batch verifier of whole vPBS proofs on the device: vpbs_verify_pbs (verifier.hip) for many last proofs of IVC chains at once, all made
// under one key set, with the host's verdict and the host's first failing check for every one of them.
//
// The proof itself is the batch verifier's (verify_batch.hip): this object owns one, created with max_public_inputs = n_pi, and runs its
// stages (vpbs::proof_verifier_enqueue) on the context's stream; what they leave on the device -- the parsed words, stride W, the public
// inputs from n_fixed, the per-proof reason -- is what the stages here read.  Per proof the public inputs are
//   acc_init [K N] (K - 1 zero polynomials, then testv) | counter | accumulator [K N] | key hash [4] | LWE hash [4] | digest [4] | cap
// Stages:
//   upload       one pinned copy per run: ct [count][n + 1] | out_ct [count][K N] | testv [1 or count][N]
//   vp_lwe_chain one 16-lane group per proof (poseidon::permute_wide), on a second stream beside the proof's stages up to FORK_MAX
//                proofs, on the context's stream after the upload above that: the n + 2 dependent
//                links hash_no_pad(h || item) over [ct[n], ct[0] .. ct[n-1], 0] -> the chain's end [4]
//   vp_statement one lane per (proof, public-input word): public-input count, mask zeros, testv, counter, out_ct, key hash, digest and cap
//                against the statement -> one flag bit per check
//   vp_result    one lane per proof, after the join: the flags, the batch verifier's reason and the LWE chain's end to one verdict, one
//                vpbs_pbs_reason and one vpbs_verify_reason, in vpbs_verify_pbs's order.
// The key hash chain (n + 2 links over GGSW-sized items) depends on the keys only: the host computes it once (vpbs_pbs_key_hash) and the
// object compares every proof against it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gl.h"
#include "poseidon.h"
#include "context.h"
#include "verify_batch.h"
#include "program_internal.h"

namespace {
using vpbs::DeviceError;
using u32 = uint32_t;
using u64 = uint64_t;

constexpr size_t FORK_MAX = 64;   // largest batch whose LWE chain runs on the second stream (measured: faster at 1 and 64 proofs, slower at 256)
constexpr u32 PF_COUNT = 1, PF_MASK = 2, PF_TESTV = 4, PF_COUNTER = 8, PF_OUT_CT = 16, PF_KEY_HASH = 32, PF_VERIFIER_DATA = 64;

struct PbsShape {
    u32 N, kn, n_lwe, n_pi, cap_words;
    u32 W, n_fixed;               // the batch verifier's slot: words per proof, public inputs from n_fixed
    int testv_per_proof;
};

// statement: grid (n_pi / 256, proofs).  stmt: key hash [4] | digest [4] | cap [cap_words]; words compared raw, as the host's memcmp does
__global__ __launch_bounds__(256) void vp_statement(const u64* __restrict__ words, const u32* __restrict__ n_pi, const u64* __restrict__ stmt,
                                                    const u64* __restrict__ testv, const u64* __restrict__ out_ct, PbsShape P,
                                                    u32* __restrict__ flags) {
    const u32 i = blockIdx.y;
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P.n_pi) return;
    const u64 v = words[(u64)i * P.W + P.n_fixed + j];
    u32 f = 0;
    if (j == 0 && n_pi[i] != P.n_pi) f |= PF_COUNT;   // from_bytes must return exactly n_pi
    if (j < P.kn - P.N) {
        if (v != 0) f |= PF_MASK;
    } else if (j < P.kn) {
        if (v != testv[(P.testv_per_proof ? (u64)i * P.N : 0) + j - (P.kn - P.N)]) f |= PF_TESTV;
    } else if (j == P.kn) {
        if (v != (u64)P.n_lwe + 2) f |= PF_COUNTER;
    } else if (j <= 2 * P.kn) {
        if (v != out_ct[(u64)i * P.kn + j - P.kn - 1]) f |= PF_OUT_CT;
    } else if (j < 2 * P.kn + 5) {
        if (v != stmt[j - 2 * P.kn - 1]) f |= PF_KEY_HASH;
    } else if (j >= 2 * P.kn + 9) {   // (the LWE hash [4] in between: vp_lwe_chain)
        if (v != stmt[4 + j - 2 * P.kn - 9]) f |= PF_VERIFIER_DATA;
    }
    if (f) atomicOr(&flags[i], f);
}

// the LWE hash chain: one proof per 16-lane block, lane l < 12 owns sponge element l (the permute_wide layout).  A link is hash_no_pad of
// five elements, h || item: one permutation of [h0 h1 h2 h3 item 0 ...].  vpbs_hash_chain's permutation takes any residue, so a word of ct
// at or above p enters as its residue (canonicalised here: what permute_wide's first addition expects).
__global__ __launch_bounds__(16) void vp_lwe_chain(const u64* __restrict__ ct, u32 n_lwe, u64* __restrict__ out) {
    __shared__ u64 sh[poseidon::WIDE_LDS_WORDS];
    const unsigned l = threadIdx.x;
    const u32 i = blockIdx.x;
    const u64* c = ct + (u64)i * (n_lwe + 1);
    u64 x = 0;
    u64 next = c[n_lwe];   // item k + 1 is loaded while link k runs: the load is off the dependent chain
    for (u32 k = 0; k < n_lwe + 2; ++k) {
        const u64 item = next;
        next = k < n_lwe ? c[k] : 0;
        if (l == 4) x = gl::canon(item);
        else if (l > 4) x = 0;
        x = poseidon::permute_wide(x, sh, l);
    }
    if (l < 4) out[(u64)i * 4 + l] = x;
}

// the first failing check in vpbs_verify_pbs's order -> out: verdicts [count] | reasons [count] | proof reasons [count]
__global__ __launch_bounds__(256) void vp_result(const u32* __restrict__ flags, const uint8_t* __restrict__ proof_reason,
                                                 const u64* __restrict__ words, const u64* __restrict__ lwe, PbsShape P, u32 count,
                                                 uint8_t* __restrict__ out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const u32 f = flags[i];
    const uint8_t pr = proof_reason[i];
    const u64* claimed = words + (u64)i * P.W + P.n_fixed + 2 * P.kn + 5;
    bool lwe_bad = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) lwe_bad = lwe_bad || lwe[(u64)i * 4 + k] != claimed[k];
    const uint8_t reason = (pr == VPBS_VERIFY_MALFORMED || (f & PF_COUNT)) ? VPBS_PBS_MALFORMED
                           : (f & PF_MASK)                                 ? VPBS_PBS_TESTV_MASK
                           : (f & PF_TESTV)                                ? VPBS_PBS_TESTV
                           : (f & PF_COUNTER)                              ? VPBS_PBS_COUNTER
                           : (f & PF_OUT_CT)                               ? VPBS_PBS_OUT_CT
                           : pr != VPBS_VERIFY_OK                          ? VPBS_PBS_PROOF
                           : (f & PF_VERIFIER_DATA)                        ? VPBS_PBS_VERIFIER_DATA
                           : (f & PF_KEY_HASH)                             ? VPBS_PBS_KEY_HASH
                           : lwe_bad                                       ? VPBS_PBS_LWE_HASH
                                                                           : VPBS_PBS_OK;
    out[i] = reason == VPBS_PBS_OK ? 1 : 0;
    out[count + i] = reason;
    out[2 * (u64)count + i] = reason == VPBS_PBS_PROOF ? pr : VPBS_VERIFY_OK;
}

void report(char* err, size_t err_len, const std::string& m) {
    if (err && err_len) {
        std::strncpy(err, m.c_str(), err_len - 1);
        err[err_len - 1] = 0;
    }
}
}  // namespace

struct vpbs_pbs_verifier {
    vpbs_ctx* ctx = nullptr;
    vpbs_proof_verifier* proofs = nullptr;
    PbsShape P{};
    size_t max_batch = 0;
    u64 *d_stmt = nullptr, *d_in = nullptr, *d_lwe = nullptr;   // d_in: ct | out_ct | testv, as uploaded
    u32* d_flags = nullptr;
    uint8_t* d_out = nullptr;
    u64* h_in = nullptr;              // pinned, the same layout as d_in
    uint8_t* h_out = nullptr;         // pinned [3][max_batch]
    hipStream_t chain_stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    std::vector<void*> owned;

    size_t in_words() const { return max_batch * ((size_t)P.n_lwe + 1 + P.kn + P.N); }
    ~vpbs_pbs_verifier() {
        if (!ctx) return;
        (void)hipSetDevice(ctx->device);
        (void)vpbs::stream_sync(ctx->stream);
        if (chain_stream) {
            (void)hipStreamSynchronize(chain_stream);
            (void)hipStreamDestroy(chain_stream);
        }
        if (fork) (void)hipEventDestroy(fork);
        if (join) (void)hipEventDestroy(join);
        for (void* p : owned) ctx->release(p);
        if (h_in) (void)hipHostFree(h_in);
        if (h_out) (void)hipHostFree(h_out);
        vpbs_proof_verifier_free(proofs);
    }
};

namespace vpbs {
void pbs_verifier_shape(const vpbs_pbs_verifier* v, PbsVerifierShape* out) {
    *out = PbsVerifierShape{v->ctx, v->P.N, v->P.kn / v->P.N, v->P.n_lwe, v->max_batch};
}
}  // namespace vpbs

extern "C" {
int vpbs_pbs_key_hash(const uint64_t* bsk, const uint64_t* ksk, unsigned n_lwe, size_t ggsw_len, uint64_t out[4]) {
    if (!ksk || !out || ggsw_len == 0 || (n_lwe && !bsk)) return VPBS_ERR_INVALID;
    // [dummy GGSW (zeros), bsk_0 .. bsk_{n-1}, ksk] as vpbs_verify_pbs hashes them, without materialising the items
    const size_t steps = (size_t)n_lwe + 2;
    const std::vector<u64> zero(ggsw_len, 0);
    std::vector<const u64*> items(steps);
    items[0] = zero.data();
    for (unsigned k = 0; k < n_lwe; ++k) items[k + 1] = bsk + (size_t)k * ggsw_len;
    items[steps - 1] = ksk;
    std::vector<u64> links(4 * steps);
    const u64 h0[4] = {0, 0, 0, 0};
    vpbs::hash_links_shared(h0, items.data(), steps, ggsw_len, links.data());
    std::memcpy(out, links.data() + 4 * (steps - 1), 32);
    return VPBS_OK;
}

const char* vpbs_pbs_reason_text(int reason) {
    switch (reason) {
        case VPBS_PBS_OK: return "";
        case VPBS_PBS_MALFORMED: return "the bytes are not a proof of this circuit (shape, canonical field elements, number of public inputs)";
        case VPBS_PBS_TESTV_MASK: return "claimed test vector: the mask polynomials are not zero";
        case VPBS_PBS_TESTV: return "claimed test vector differs from testv";
        case VPBS_PBS_COUNTER: return "the counter is not n + 2";
        case VPBS_PBS_OUT_CT: return "the output ciphertext is not the proof's accumulator";
        case VPBS_PBS_PROOF: return "the proof does not verify";
        case VPBS_PBS_VERIFIER_DATA: return "the proof carries another circuit's verifier data";
        case VPBS_PBS_KEY_HASH: return "the key hash chain does not match";
        case VPBS_PBS_LWE_HASH: return "the LWE hash chain does not match";
        default: return nullptr;
    }
}

int vpbs_pbs_verifier_create(vpbs_ctx* ctx, const vpbs_verify_pbs_inputs* shape, const uint64_t key_hash[4], size_t max_batch,
                             vpbs_pbs_verifier** out, char* err, size_t err_len) {
    if (out) *out = nullptr;
    auto refuse = [&](const char* m) {
        report(err, err_len, m);
        return VPBS_ERR_INVALID;
    };
    if (!ctx || !shape || !shape->circuit || !key_hash || !out || !shape->circuit->constants_sigmas_cap) return refuse("null argument");
    // what vpbs_verify_pbs refuses of the shape (its testv, ct, out_ct, bsk and ksk are per proof here, or in key_hash)
    if (shape->N == 0 || shape->K == 0 || shape->ggsw_len == 0 || shape->ggsw_len % ((size_t)shape->K * shape->K * shape->N) != 0)
        return refuse("malformed shape (N, K > 0; ggsw_len = K * ELL * K * N)");
    if ((size_t)shape->K * shape->N > (1u << 20) || shape->n_lwe > (1u << 24)) return refuse("N, K or n_lwe out of range");
    const vpbs_verify_inputs& c = *shape->circuit;
    if (c.cap_height > 8) return refuse("malformed circuit description (cap_height)");
    const size_t kn = (size_t)shape->K * shape->N, cap_words = (size_t)4 << c.cap_height;
    const size_t n_pi = 2 * kn + 1 + 8 + 4 + cap_words;
    vpbs_verify_inputs full = c;   // cd.verify: the full check, whatever the caller's struct says
    full.fri_only = 0;
    full.public_inputs = nullptr;
    full.n_public_inputs = 0;
    auto* v = new vpbs_pbs_verifier;
    const int rc = vpbs_proof_verifier_create(ctx, &full, max_batch, n_pi, &v->proofs, err, err_len);
    if (rc) {
        delete v;
        return rc;
    }
    v->ctx = ctx;
    v->max_batch = max_batch;
    PbsShape& P = v->P;
    P.N = shape->N;
    P.kn = (u32)kn;
    P.n_lwe = shape->n_lwe;
    P.n_pi = (u32)n_pi;
    P.cap_words = (u32)cap_words;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        std::vector<u64> stmt(8 + cap_words);
        std::memcpy(stmt.data(), key_hash, 32);
        std::memcpy(stmt.data() + 4, c.circuit_digest, 32);
        std::memcpy(stmt.data() + 8, c.constants_sigmas_cap, 8 * cap_words);
        auto alloc = [&](size_t bytes) {
            void* d = ctx->alloc_bytes(std::max<size_t>(1, bytes));
            v->owned.push_back(d);
            return d;
        };
        v->d_stmt = static_cast<u64*>(alloc(8 * stmt.size()));
        VPBS_HIP(hipMemcpyAsync(v->d_stmt, stmt.data(), 8 * stmt.size(), hipMemcpyHostToDevice, ctx->stream));
        v->d_in = static_cast<u64*>(alloc(8 * v->in_words()));
        v->d_lwe = static_cast<u64*>(alloc(32 * max_batch));
        v->d_flags = static_cast<u32*>(alloc(4 * max_batch));
        v->d_out = static_cast<uint8_t*>(alloc(3 * max_batch));
        VPBS_HIP(hipHostMalloc((void**)&v->h_in, 8 * v->in_words(), hipHostMallocDefault));
        VPBS_HIP(hipHostMalloc((void**)&v->h_out, 3 * max_batch, hipHostMallocDefault));
        VPBS_HIP(hipStreamCreateWithFlags(&v->chain_stream, hipStreamNonBlocking));
        VPBS_HIP(hipEventCreateWithFlags(&v->fork, hipEventDisableTiming));
        VPBS_HIP(hipEventCreateWithFlags(&v->join, hipEventDisableTiming));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));   // `stmt` goes out of scope
    } catch (const DeviceError& e) {
        report(err, err_len, e.what);
        ctx->err = e.what;
        delete v;
        return e.status;
    }
    *out = v;
    report(err, err_len, "");
    return VPBS_OK;
}

long vpbs_pbs_verifier_run(vpbs_pbs_verifier* v, const uint8_t* bytes, const size_t* offsets, size_t count, const uint64_t* testv,
                           int testv_per_proof, const uint64_t* ct, const uint64_t* out_ct, uint8_t* verdicts, uint8_t* reasons,
                           uint8_t* proof_reasons) {
    if (!v || !offsets || !testv || !ct || !out_ct || !verdicts || count > v->max_batch) return VPBS_ERR_INVALID;
    if (count == 0) return 0;
    if (!bytes) return VPBS_ERR_INVALID;
    vpbs_ctx* ctx = v->ctx;
    PbsShape P = v->P;
    P.testv_per_proof = testv_per_proof != 0;
    const size_t n_ct = count * ((size_t)P.n_lwe + 1), n_out = count * (size_t)P.kn, n_tv = (P.testv_per_proof ? count : 1) * (size_t)P.N;
    const u32 n = (u32)count;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        // the statement's inputs first: the LWE chain needs nothing else and, on its own stream, starts while the proofs are uploaded
        std::memcpy(v->h_in, ct, 8 * n_ct);
        std::memcpy(v->h_in + n_ct, out_ct, 8 * n_out);
        std::memcpy(v->h_in + n_ct + n_out, testv, 8 * n_tv);
        VPBS_HIP(hipMemcpyAsync(v->d_in, v->h_in, 8 * (n_ct + n_out + n_tv), hipMemcpyHostToDevice, s));
        VPBS_HIP(hipMemsetAsync(v->d_flags, 0, 4 * count, s));
        // up to FORK_MAX proofs the chain runs on its own stream beside the proof's stages; above, after the upload on the context's stream
        // (both kernels are 16-lane permute_wide chains and slow each other down where they share the CUs: DESIGN.md section 8.2)
        const bool fork = count <= FORK_MAX;
        hipStream_t cs = fork ? v->chain_stream : s;
        if (fork) {
            VPBS_HIP(hipEventRecord(v->fork, s));
            VPBS_HIP(hipStreamWaitEvent(cs, v->fork, 0));
        }
        {
            int id = -1;
            hipEvent_t t0 = nullptr;
            if (ctx->timing && (ctx->timing_only.empty() || ctx->timing_only == "vp_lwe_chain")) {
                id = ctx->timer_id("vp_lwe_chain");
                t0 = ctx->get_event();
                VPBS_HIP(hipEventRecord(t0, cs));
            }
            vp_lwe_chain<<<n, 16, 0, cs>>>(v->d_in, P.n_lwe, v->d_lwe);
            if (id >= 0) {
                hipEvent_t t1 = ctx->get_event();
                VPBS_HIP(hipEventRecord(t1, cs));
                ctx->pending.push_back({id, t0, t1});
            }
        }
        VPBS_HIP(hipGetLastError());
        if (fork) VPBS_HIP(hipEventRecord(v->join, cs));
        vpbs::ProofBatchView pv{};
        const int rc = vpbs::proof_verifier_enqueue(v->proofs, bytes, offsets, count, &pv);
        if (rc) {   // (offsets that decrease): the chain kernel is left to finish before the inputs may change
            VPBS_HIP(hipStreamSynchronize(v->chain_stream));
            return rc;
        }
        P.W = pv.W;
        P.n_fixed = pv.n_fixed;
        {
            vpbs::Timed t(ctx, "vp_statement");
            vp_statement<<<dim3((P.n_pi + 255) / 256, n), 256, 0, s>>>(pv.words, pv.n_pi, v->d_stmt, v->d_in + n_ct + n_out, v->d_in + n_ct, P,
                                                                       v->d_flags);
        }
        if (fork) VPBS_HIP(hipStreamWaitEvent(s, v->join, 0));
        vp_result<<<(n + 255) / 256, 256, 0, s>>>(v->d_flags, pv.reasons, pv.words, v->d_lwe, P, n, v->d_out);
        VPBS_HIP(hipGetLastError());
        VPBS_HIP(hipMemcpyAsync(v->h_out, v->d_out, 3 * count, hipMemcpyDeviceToHost, s));
        VPBS_HIP(vpbs::stream_sync(s));
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        (void)hipStreamSynchronize(v->chain_stream);
        return VPBS_ERR_DEVICE;
    }
    long accepted = 0;
    for (size_t k = 0; k < count; ++k) {
        verdicts[k] = v->h_out[k];
        accepted += v->h_out[k];
        if (reasons) reasons[k] = v->h_out[count + k];
        if (proof_reasons) proof_reasons[k] = v->h_out[2 * count + k];
    }
    return accepted;
}

void vpbs_pbs_verifier_free(vpbs_pbs_verifier* v) { delete v; }
}  // extern "C"
