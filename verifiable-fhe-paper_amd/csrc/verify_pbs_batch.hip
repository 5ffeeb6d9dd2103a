// Batch verifier of whole vPBS proofs on the device: vpbs_verify_pbs (verifier.hip) for many last proofs of IVC chains at once, with the
// host's verdict and the host's first failing check for every one of them.  Two objects share one core (vpbs::PbsVerifyCore, the seam in
// program_internal.h): vpbs_pbs_verifier, all proofs under ONE key set, and vpbs_ring_verifier, proof i under the key hash of slot key_of[i].
//
// The proof itself is the batch verifier's (verify_batch.hip): the core owns one, created with max_public_inputs = n_pi, and runs its
// stages (vpbs::proof_verifier_enqueue) on the context's stream; what they leave on the device -- the parsed words, stride W, the public
// inputs from n_fixed, the per-proof reason -- is what the stages here read.  Per proof the public inputs are
//   acc_init [K N] (K - 1 zero polynomials, then testv) | counter | accumulator [K N] | key hash [4] | LWE hash [4] | digest [4] | cap
// The core (vpbs::pbs_verify_enqueue) takes DEVICE pointers -- ct [count][n + 1], out_ct [count][K N], a table of test vectors with
// testv_of [count], a table of key hashes with key_of [count] -- and queues:
//   vp_lwe_chain one 16-lane group per proof (poseidon::permute_wide), on a second stream beside the proof's stages up to FORK_MAX
//                proofs, on the context's stream above that: the n + 2 dependent
//                links hash_no_pad(h || item) over [ct[n], ct[0] .. ct[n-1], 0] -> the chain's end [4]
//   vp_statement one lane per (proof, public-input word): public-input count, mask zeros, testvs[testv_of[i]], counter, out_ct,
//                key_hashes[key_of[i]], digest and cap against the statement -> one flag bit per check.  ONE statement for both objects.
//   vp_result    one lane per proof, after the join: the flags, the batch verifier's reason and the LWE chain's end to one verdict, one
//                vpbs_pbs_reason and one vpbs_verify_reason, in vpbs_verify_pbs's order, left on the device: the read-back and its wait
//                are the caller's (vpbs::pbs_verify_collect).
// The objects stage host arrays with one pinned copy per run: ct | out_ct | testvs | testv_of | key_of.
// The key hash chain (n + 2 links over GGSW-sized items) depends on the keys only: the host computes it once per key set
// (vpbs_pbs_key_hash, or the ring prover's links) and the objects compare every proof against the entry of its slot.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "gl.h"
#include "poseidon.h"
#include "context.h"
#include "verify_batch.h"
#include "program_internal.h"

namespace {
using vpbs::DeviceError;
using vpbs::report;
using u32 = uint32_t;
using u64 = uint64_t;

constexpr size_t FORK_MAX = 64;   // largest batch whose LWE chain runs on the second stream (measured: faster at 1 and 64 proofs, slower at 256)
constexpr u32 PF_COUNT = 1, PF_MASK = 2, PF_TESTV = 4, PF_COUNTER = 8, PF_OUT_CT = 16, PF_KEY_HASH = 32, PF_VERIFIER_DATA = 64;

struct PbsShape {
    u32 N, kn, n_lwe, n_pi, cap_words;
    u32 W, n_fixed;               // the batch verifier's slot: words per proof, public inputs from n_fixed
};

// statement: grid (n_pi / 256, proofs).  stmt: digest [4] | cap [cap_words], shared by all proofs; the test vector of proof i is row
// testv_of[i] of `testvs`, its key hash row key_of[i] of `key_hashes`.  Both indices depend on blockIdx.y alone: their loads, and the
// table rows' bases, are wave-uniform.  Words are compared raw, as the host's memcmp does.
__global__ __launch_bounds__(256) void vp_statement(const u64* __restrict__ words, const u32* __restrict__ n_pi, const u64* __restrict__ stmt,
                                                    const u64* __restrict__ testvs, const u32* __restrict__ testv_of,
                                                    const u64* __restrict__ key_hashes, const u32* __restrict__ key_of,
                                                    const u64* __restrict__ out_ct, PbsShape P, u32* __restrict__ flags) {
    const u32 i = blockIdx.y;
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P.n_pi) return;
    const u64 v = words[(u64)i * P.W + P.n_fixed + j];
    u32 f = 0;
    if (j == 0 && n_pi[i] != P.n_pi) f |= PF_COUNT;   // from_bytes must return exactly n_pi
    if (j < P.kn - P.N) {
        if (v != 0) f |= PF_MASK;
    } else if (j < P.kn) {
        if (v != testvs[(u64)testv_of[i] * P.N + j - (P.kn - P.N)]) f |= PF_TESTV;
    } else if (j == P.kn) {
        if (v != (u64)P.n_lwe + 2) f |= PF_COUNTER;
    } else if (j <= 2 * P.kn) {
        if (v != out_ct[(u64)i * P.kn + j - P.kn - 1]) f |= PF_OUT_CT;
    } else if (j < 2 * P.kn + 5) {
        if (v != key_hashes[(u64)key_of[i] * 4 + j - 2 * P.kn - 1]) f |= PF_KEY_HASH;
    } else if (j >= 2 * P.kn + 9) {   // (the LWE hash [4] in between: vp_lwe_chain)
        if (v != stmt[j - 2 * P.kn - 9]) f |= PF_VERIFIER_DATA;
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
}  // namespace

namespace vpbs {
// What both objects are built on: the batch verifier of the proofs, the statement's shared words, the per-run buffers of max_batch proofs
// and the staging area of an object that takes host arrays.
struct PbsVerifyCore {
    vpbs_ctx* ctx = nullptr;
    vpbs_proof_verifier* proofs = nullptr;
    PbsShape P{};
    size_t max_batch = 0;
    u64 *d_stmt = nullptr, *d_in = nullptr, *d_lwe = nullptr;   // d_stmt: digest [4] | cap; d_in: ct | out_ct | testvs | testv_of | key_of, as uploaded
    u32* d_flags = nullptr;
    uint8_t* d_out = nullptr;
    u64* h_in = nullptr;              // pinned, the same layout as d_in
    uint8_t* h_out = nullptr;         // pinned [3][max_batch]
    hipStream_t chain_stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    std::vector<void*> owned;

    // at most max_batch test vectors per run; the two index arrays are uint32: max_batch words together
    size_t in_words() const { return max_batch * ((size_t)P.n_lwe + 1 + P.kn + P.N + 1); }
    void* alloc(size_t bytes) {
        void* d = ctx->alloc_bytes(std::max<size_t>(1, bytes));
        owned.push_back(d);
        return d;
    }
    ~PbsVerifyCore() {
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

int pbs_verify_enqueue(PbsVerifyCore* c, const uint8_t* bytes, const size_t* offsets, size_t count, const uint64_t* d_ct, const uint64_t* d_out_ct,
                       const uint64_t* d_testvs, const uint32_t* d_testv_of, const uint64_t* d_key_hashes, const uint32_t* d_key_of) {
    vpbs_ctx* ctx = c->ctx;
    PbsShape P = c->P;
    const u32 n = (u32)count;
    hipStream_t s = ctx->stream;
    VPBS_HIP(hipMemsetAsync(c->d_flags, 0, 4 * count, s));
    // up to FORK_MAX proofs the chain runs on its own stream beside the proof's stages; above, on the context's stream before them
    // (both kernels are 16-lane permute_wide chains and slow each other down where they share the CUs: DESIGN.md section 8.2).  The
    // chain needs the ciphertexts alone: on its own stream it starts while the proofs are uploaded.
    const bool fork = count <= FORK_MAX;
    hipStream_t cs = fork ? c->chain_stream : s;
    if (fork) {
        VPBS_HIP(hipEventRecord(c->fork, s));
        VPBS_HIP(hipStreamWaitEvent(cs, c->fork, 0));
    }
    {
        int id = -1;
        hipEvent_t t0 = nullptr;
        if (ctx->timing && (ctx->timing_only.empty() || ctx->timing_only == "vp_lwe_chain")) {
            id = ctx->timer_id("vp_lwe_chain");
            t0 = ctx->get_event();
            VPBS_HIP(hipEventRecord(t0, cs));
        }
        vp_lwe_chain<<<n, 16, 0, cs>>>(d_ct, P.n_lwe, c->d_lwe);
        if (id >= 0) {
            hipEvent_t t1 = ctx->get_event();
            VPBS_HIP(hipEventRecord(t1, cs));
            ctx->pending.push_back({id, t0, t1});
        }
    }
    VPBS_HIP(hipGetLastError());
    if (fork) VPBS_HIP(hipEventRecord(c->join, cs));
    vpbs::ProofBatchView pv{};
    const int rc = vpbs::proof_verifier_enqueue(c->proofs, bytes, offsets, count, &pv);
    if (rc) {   // (offsets that decrease): the chain kernel is left to finish before the inputs may change
        VPBS_HIP(hipStreamSynchronize(c->chain_stream));
        return rc;
    }
    P.W = pv.W;
    P.n_fixed = pv.n_fixed;
    {
        vpbs::Timed t(ctx, "vp_statement");
        vp_statement<<<dim3((P.n_pi + 255) / 256, n), 256, 0, s>>>(pv.words, pv.n_pi, c->d_stmt, d_testvs, d_testv_of, d_key_hashes, d_key_of, d_out_ct, P,
                                                                   c->d_flags);
    }
    if (fork) VPBS_HIP(hipStreamWaitEvent(s, c->join, 0));
    vp_result<<<(n + 255) / 256, 256, 0, s>>>(c->d_flags, pv.reasons, pv.words, c->d_lwe, P, n, c->d_out);
    VPBS_HIP(hipGetLastError());
    return VPBS_OK;
}

long pbs_verify_collect(PbsVerifyCore* c, size_t count, uint8_t* verdicts, uint8_t* reasons, uint8_t* proof_reasons) {
    VPBS_HIP(hipMemcpyAsync(c->h_out, c->d_out, 3 * count, hipMemcpyDeviceToHost, c->ctx->stream));
    VPBS_HIP(vpbs::stream_sync(c->ctx->stream));
    long accepted = 0;
    for (size_t k = 0; k < count; ++k) {
        verdicts[k] = c->h_out[k];
        accepted += c->h_out[k];
        if (reasons) reasons[k] = c->h_out[count + k];
        if (proof_reasons) proof_reasons[k] = c->h_out[2 * count + k];
    }
    return accepted;
}

void pbs_verify_abandon(PbsVerifyCore* c, const DeviceError& e) {
    c->ctx->err = e.what;
    (void)hipStreamSynchronize(c->chain_stream);
}
}  // namespace vpbs

namespace {
using vpbs::PbsVerifyCore;

// what vpbs_pbs_verifier_create and vpbs_ring_verifier_create share: the refusals of the shape, the batch verifier of the proofs, the buffers
int core_create(vpbs_ctx* ctx, const vpbs_verify_pbs_inputs* shape, size_t max_batch, PbsVerifyCore* v, char* err, size_t err_len) {
    auto refuse = [&](const char* m) {
        report(err, err_len, m);
        return VPBS_ERR_INVALID;
    };
    if (!ctx || !shape || !shape->circuit || !shape->circuit->constants_sigmas_cap) return refuse("null argument");
    // what vpbs_verify_pbs refuses of the shape (its testv, ct, out_ct, bsk and ksk are per proof here, or in the key hash)
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
    const int rc = vpbs_proof_verifier_create(ctx, &full, max_batch, n_pi, &v->proofs, err, err_len);
    if (rc) return rc;
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
        std::vector<u64> stmt(4 + cap_words);
        std::memcpy(stmt.data(), c.circuit_digest, 32);
        std::memcpy(stmt.data() + 4, c.constants_sigmas_cap, 8 * cap_words);
        v->d_stmt = static_cast<u64*>(v->alloc(8 * stmt.size()));
        VPBS_HIP(hipMemcpyAsync(v->d_stmt, stmt.data(), 8 * stmt.size(), hipMemcpyHostToDevice, ctx->stream));
        v->d_in = static_cast<u64*>(v->alloc(8 * v->in_words()));
        v->d_lwe = static_cast<u64*>(v->alloc(32 * max_batch));
        v->d_flags = static_cast<u32*>(v->alloc(4 * max_batch));
        v->d_out = static_cast<uint8_t*>(v->alloc(3 * max_batch));
        VPBS_HIP(hipHostMalloc((void**)&v->h_in, 8 * v->in_words(), hipHostMallocDefault));
        VPBS_HIP(hipHostMalloc((void**)&v->h_out, 3 * max_batch, hipHostMallocDefault));
        VPBS_HIP(hipStreamCreateWithFlags(&v->chain_stream, hipStreamNonBlocking));
        VPBS_HIP(hipEventCreateWithFlags(&v->fork, hipEventDisableTiming));
        VPBS_HIP(hipEventCreateWithFlags(&v->join, hipEventDisableTiming));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));   // `stmt` goes out of scope
    } catch (const DeviceError& e) {
        report(err, err_len, e.what);
        ctx->err = e.what;
        return e.status;
    }
    return VPBS_OK;
}

// One run on HOST arrays: the statement's inputs in one pinned copy, the core, the read-back.  testv_of null: proof i takes test vector i
// of n_testv == count, or the one of n_testv == 1; key_of null: every proof takes entry 0 of the key table.  The caller has checked the
// indices, count in 1 .. max_batch and n_testv <= max_batch.
long core_run_host(PbsVerifyCore* c, const uint8_t* bytes, const size_t* offsets, size_t count, const u32* key_of, const u64* testvs, size_t n_testv,
                   const u32* testv_of, const u64* ct, const u64* out_ct, const u64* d_key_hashes, uint8_t* verdicts, uint8_t* reasons,
                   uint8_t* proof_reasons) {
    const PbsShape& P = c->P;
    const size_t n_ct = count * ((size_t)P.n_lwe + 1), n_out = count * (size_t)P.kn, n_tv = n_testv * (size_t)P.N, n_idx = count;
    try {
        VPBS_HIP(hipSetDevice(c->ctx->device));
        std::memcpy(c->h_in, ct, 8 * n_ct);
        std::memcpy(c->h_in + n_ct, out_ct, 8 * n_out);
        std::memcpy(c->h_in + n_ct + n_out, testvs, 8 * n_tv);
        u32* idx = reinterpret_cast<u32*>(c->h_in + n_ct + n_out + n_tv);
        for (size_t i = 0; i < count; ++i) {
            idx[i] = testv_of ? testv_of[i] : (n_testv == 1 ? 0 : (u32)i);
            idx[count + i] = key_of ? key_of[i] : 0;
        }
        VPBS_HIP(hipMemcpyAsync(c->d_in, c->h_in, 8 * (n_ct + n_out + n_tv + n_idx), hipMemcpyHostToDevice, c->ctx->stream));
        const u32* d_idx = reinterpret_cast<const u32*>(c->d_in + n_ct + n_out + n_tv);
        const int rc = vpbs::pbs_verify_enqueue(c, bytes, offsets, count, c->d_in, c->d_in + n_ct, c->d_in + n_ct + n_out, d_idx, d_key_hashes, d_idx + count);
        if (rc) return rc;
        return vpbs::pbs_verify_collect(c, count, verdicts, reasons, proof_reasons);
    } catch (const DeviceError& e) {
        vpbs::pbs_verify_abandon(c, e);
        return VPBS_ERR_DEVICE;
    }
}
}  // namespace

struct vpbs_pbs_verifier {
    PbsVerifyCore core;
    u64* d_key = nullptr;   // a key table of one entry
};

struct vpbs_ring_verifier {
    PbsVerifyCore core;
    size_t max_keys = 0, filled = 0;
    std::vector<uint8_t> used;   // [max_keys]
    u64* d_keys = nullptr;       // [max_keys][4]: 32 bytes per slot, zeros in an empty one
    u64* h_key = nullptr;        // pinned [4]: what set_key uploads
    std::mutex mu;               // set_key, clear_key and run exclude each other
    ~vpbs_ring_verifier() {
        if (h_key) (void)hipHostFree(h_key);
    }
};

namespace vpbs {
void pbs_verifier_shape(const vpbs_pbs_verifier* v, PbsVerifierShape* out) {
    const PbsShape& P = v->core.P;
    *out = PbsVerifierShape{v->core.ctx, P.N, P.kn / P.N, P.n_lwe, v->core.max_batch};
}
void ring_verifier_shape(const vpbs_ring_verifier* v, RingVerifierShape* out) {
    const PbsShape& P = v->core.P;
    *out = RingVerifierShape{v->core.ctx, P.N, P.kn / P.N, P.n_lwe, v->max_keys, v->core.max_batch};
}
PbsVerifyCore* pbs_verifier_core(vpbs_pbs_verifier* v) { return &v->core; }
const uint64_t* pbs_verifier_key_table(const vpbs_pbs_verifier* v) { return v->d_key; }
std::mutex& ring_verifier_mutex(vpbs_ring_verifier* v) { return v->mu; }
PbsVerifyCore* ring_verifier_core(vpbs_ring_verifier* v) { return &v->core; }
const uint64_t* ring_verifier_key_table(const vpbs_ring_verifier* v) { return v->d_keys; }
bool ring_verifier_check_slots(const vpbs_ring_verifier* v, const uint32_t* key_of, size_t count, const char* who, const char* what,
                               std::string* msg) {
    for (size_t i = 0; i < count; ++i) {
        const uint32_t s = key_of[i];
        if (s >= v->max_keys || !v->used[s]) {
            *msg = std::string(who) + ": key_of[" + std::to_string(i) + "] = " + std::to_string(s) +
                   (s >= v->max_keys ? ": slot out of range (max_keys " + std::to_string(v->max_keys) + ")" : ": slot " + std::to_string(s) + " is empty") +
                   "; " + what + " " + std::to_string(i) + " has no key hash, nothing was queued";
            return false;
        }
    }
    return true;
}
}  // namespace vpbs

extern "C" {
int vpbs_pbs_key_hash(const uint64_t* bsk, const uint64_t* ksk, unsigned n_lwe, size_t ggsw_len, uint64_t out[4]) {
    if (!ksk || !out || ggsw_len == 0 || (n_lwe && !bsk)) return VPBS_ERR_INVALID;
    std::vector<u64> links(4 * ((size_t)n_lwe + 2));   // the last link of the chain the batch provers keep whole
    vpbs::key_hash_links(bsk, ksk, 0, n_lwe, ggsw_len, links.data());
    std::memcpy(out, links.data() + 4 * ((size_t)n_lwe + 1), 32);
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
    if (!key_hash || !out) return report(err, err_len, "null argument"), VPBS_ERR_INVALID;
    auto* v = new vpbs_pbs_verifier;
    const int rc = core_create(ctx, shape, max_batch, &v->core, err, err_len);
    if (rc) {
        delete v;
        return rc;
    }
    try {
        v->d_key = static_cast<u64*>(v->core.alloc(32));
        VPBS_HIP(hipMemcpy(v->d_key, key_hash, 32, hipMemcpyHostToDevice));
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
    if (!v || !offsets || !testv || !ct || !out_ct || !verdicts || count > v->core.max_batch) return VPBS_ERR_INVALID;
    if (count == 0) return 0;
    if (!bytes) return VPBS_ERR_INVALID;
    // the core with a key table of one entry: key_of all zero, testv_of[i] = i or 0
    return core_run_host(&v->core, bytes, offsets, count, nullptr, testv, testv_per_proof ? count : 1, nullptr, ct, out_ct, v->d_key, verdicts, reasons,
                         proof_reasons);
}

void vpbs_pbs_verifier_free(vpbs_pbs_verifier* v) { delete v; }

int vpbs_ring_verifier_create(vpbs_ctx* ctx, const vpbs_verify_pbs_inputs* shape, unsigned max_keys, size_t max_batch, vpbs_ring_verifier** out,
                              char* err, size_t err_len) {
    if (out) *out = nullptr;
    if (!out) return report(err, err_len, "null argument"), VPBS_ERR_INVALID;
    if (max_keys == 0 || max_keys > 65535) return report(err, err_len, "max_keys must be 1 .. 65535"), VPBS_ERR_INVALID;
    auto* v = new vpbs_ring_verifier;
    const int rc = core_create(ctx, shape, max_batch, &v->core, err, err_len);
    if (rc) {
        delete v;
        return rc;
    }
    v->max_keys = max_keys;
    v->used.assign(max_keys, 0);
    try {
        v->d_keys = static_cast<u64*>(v->core.alloc(32 * (size_t)max_keys));
        VPBS_HIP(hipMemsetAsync(v->d_keys, 0, 32 * (size_t)max_keys, ctx->stream));
        VPBS_HIP(hipHostMalloc((void**)&v->h_key, 32, hipHostMallocDefault));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
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

int vpbs_ring_verifier_set_key(vpbs_ring_verifier* v, unsigned slot, const uint64_t key_hash[4]) {
    if (!v || !key_hash || slot >= v->max_keys) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(v->mu);
    vpbs_ctx* ctx = v->core.ctx;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        std::memcpy(v->h_key, key_hash, 32);
        VPBS_HIP(hipMemcpyAsync(v->d_keys + 4 * (size_t)slot, v->h_key, 32, hipMemcpyHostToDevice, ctx->stream));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));   // h_key is free for the next call
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        return VPBS_ERR_DEVICE;
    }
    if (!v->used[slot]) ++v->filled;
    v->used[slot] = 1;
    return VPBS_OK;
}

int vpbs_ring_verifier_clear_key(vpbs_ring_verifier* v, unsigned slot) {
    if (!v || slot >= v->max_keys) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(v->mu);
    if (!v->used[slot]) return VPBS_ERR_INVALID;
    vpbs_ctx* ctx = v->core.ctx;
    try {
        VPBS_HIP(hipSetDevice(ctx->device));
        VPBS_HIP(hipMemsetAsync(v->d_keys + 4 * (size_t)slot, 0, 32, ctx->stream));
        VPBS_HIP(vpbs::stream_sync(ctx->stream));
    } catch (const DeviceError& e) {
        ctx->err = e.what;
        return VPBS_ERR_DEVICE;
    }
    v->used[slot] = 0;
    --v->filled;
    return VPBS_OK;
}

long vpbs_ring_verifier_count(vpbs_ring_verifier* v) {
    if (!v) return VPBS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(v->mu);
    return (long)v->filled;
}

long vpbs_ring_verifier_run(vpbs_ring_verifier* v, const uint8_t* bytes, const size_t* offsets, size_t count, const uint32_t* key_of,
                            const uint64_t* testvs, size_t n_testv, const uint32_t* testv_of, const uint64_t* ct, const uint64_t* out_ct,
                            uint8_t* verdicts, uint8_t* reasons, uint8_t* proof_reasons, char* err, size_t err_len) {
    const std::string who = "vpbs_ring_verifier_run";
    auto refuse = [&](const std::string& m) {
        report(err, err_len, m);
        return (long)VPBS_ERR_INVALID;
    };
    report(err, err_len, "");
    if (!v) return refuse(who + ": null ring verifier");
    if (!offsets || !key_of || !testvs || !ct || !out_ct || !verdicts) return refuse(who + ": null offsets, key_of, testvs, ct, out_ct or verdicts");
    std::lock_guard<std::mutex> lock(v->mu);   // from the check of the slots to the read-back: no slot changes under a run
    if (count > v->core.max_batch)
        return refuse(who + ": count " + std::to_string(count) + " exceeds max_batch " + std::to_string(v->core.max_batch));
    if (n_testv > v->core.max_batch)
        return refuse(who + ": n_testv " + std::to_string(n_testv) + " exceeds max_batch " + std::to_string(v->core.max_batch));
    if (!testv_of && n_testv != count && n_testv != 1)
        return refuse(who + ": testv_of is null and n_testv " + std::to_string(n_testv) + " is neither count " + std::to_string(count) + " nor 1");
    std::string msg;
    if (!vpbs::ring_verifier_check_slots(v, key_of, count, who.c_str(), "proof", &msg)) return refuse(msg);
    if (testv_of)
        for (size_t i = 0; i < count; ++i)
            if (testv_of[i] >= n_testv)
                return refuse(who + ": testv_of[" + std::to_string(i) + "] = " + std::to_string(testv_of[i]) + " is not below n_testv " +
                              std::to_string(n_testv) + "; proof " + std::to_string(i) + " has no test vector, nothing was queued");
    if (count == 0) return 0;
    if (!bytes) return refuse(who + ": null bytes");
    const long rc = core_run_host(&v->core, bytes, offsets, count, key_of, testvs, n_testv, testv_of, ct, out_ct, v->d_keys, verdicts, reasons,
                                  proof_reasons);
    if (rc == VPBS_ERR_DEVICE) report(err, err_len, who + ": " + v->core.ctx->err);
    else if (rc < 0) report(err, err_len, who + ": malformed offsets");
    return rc;
}

void vpbs_ring_verifier_free(vpbs_ring_verifier* v) { delete v; }
}  // extern "C"
