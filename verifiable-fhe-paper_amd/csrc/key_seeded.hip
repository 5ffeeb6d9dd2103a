// Seeded key sets, expanded where the server needs them (vpbs_key_expand; vpbs_keyring_add_seeded and vpbs_ring_prover_add_seeded through
// key_expand_device).  Under the split generator (keygen_streams.h) K - 1 of the K polynomials of every GLWE of a bootstrapping or key
// switching key are public uniform masks that ONE 64-bit mask_seed determines; a client ships the last polynomial of every GLWE
// (vpbs_keygen_seeded: [n_lwe][K][ELL][N] and [K][ELL][N], 1 / K of the key set) and the device rebuilds vpbs_keygen's layout word for word.
//
// key_expand_kernel gives ONE WORKGROUP to a polynomial of the output, blockIdx = ((g K + p) ELL + l) K + r:
//   r < K - 1   the N coefficients of the mask are drawn into LDS (N words, at most 16 KiB) exactly as ggsw_fill_kernel draws them, transformed
//               there by pb_forward of pbs_chain.h -- the butterflies of launch_negacyclic in the same order, canonical in and canonical
//               out, so the words are vpbs_keygen's -- with the twiddles of ctx->ring_table, and stored with 16-byte vector stores;
//   r = K - 1   the body is copied from the compact array with 16-byte loads and stores.
// The key is written once and 1 / K of it is read, where vpbs_keygen passes three times over the same memory (fill, transform in place,
// body).  No workgroup waits for another; the loops stride by the workgroup, so N = 8 (fewer points than lanes) needs no case of its own.
// mix64 is not a cryptographic generator: this separates public from private, it does not make the streams fit for production.
#include <string>

#include "context.h"
#include "keygen_streams.h"
#include "pbs_chain.h"
#include "program_internal.h"

using vpbs::DeviceError;
using vpbs::u64;

namespace vpbs {
namespace {
constexpr unsigned THREADS = 256, MAX_N = 2048;

struct KeyExpandJob {
    u64 mask_seed, kind;   // kind: BSK_MASK or KSK_MASK
    unsigned log_n, K, ELL;
    size_t n_poly;         // n_ggsw K ELL K
};

__global__ void __launch_bounds__(THREADS) key_expand_kernel(KeyExpandJob j, const u64* __restrict__ roots, const u64* __restrict__ bodies,
                                                             u64* __restrict__ out) {
    using namespace keygen;
    __shared__ __attribute__((aligned(16))) u64 t[MAX_N];
    const size_t q = blockIdx.x;
    if (q >= j.n_poly) return;   // the same for the whole workgroup
    const unsigned n = 1u << j.log_n, half = n >> 1;
    const unsigned r = (unsigned)(q % j.K);
    const size_t glwe = q / j.K;
    ulonglong2* dst = reinterpret_cast<ulonglong2*>(out + q * n);
    if (r + 1 == j.K) {   // the body: glwe < n_poly / K, the length of the compact array
        const ulonglong2* src = reinterpret_cast<const ulonglong2*>(bodies + glwe * n);
        for (unsigned i = threadIdx.x; i < half; i += THREADS) dst[i] = src[i];
        return;
    }
    const u64 pl = glwe % ((size_t)j.K * j.ELL), g = glwe / ((size_t)j.K * j.ELL);
    const u64 key = stream(j.mask_seed, tag(j.kind, g, pl, r));   // a mask kind: keyed by mask_seed
    for (unsigned i = threadIdx.x; i < n; i += THREADS) t[i] = field(draw(key, i));
    __syncthreads();
    pb_forward<THREADS>(t, j.log_n, 1, roots);   // ends behind a barrier
    const ulonglong2* src = reinterpret_cast<const ulonglong2*>(t);
    for (unsigned i = threadIdx.x; i < half; i += THREADS) dst[i] = src[i];
}

void enqueue(vpbs_ctx* c, const vpbs_tfhe_params& prm, size_t n_ggsw, u64 kind, u64 mask_seed, const u64* d_bodies, u64* d_out) {
    const KeyExpandJob job{mask_seed, kind, prm.log_N, prm.K, prm.ELL, n_ggsw * prm.K * prm.ELL * prm.K};
    VPBS_REQUIRE(prm.log_N >= 1 && (1u << prm.log_N) <= MAX_N && job.n_poly >= 1 && job.n_poly < ((size_t)1 << 31), "key_expand: unsupported shape");
    vpbs::Timed t(c, "key_expand");
    hipLaunchKernelGGL(key_expand_kernel, dim3((unsigned)job.n_poly), dim3(THREADS), 0, c->stream, job, c->ring_table(prm.log_N), d_bodies, d_out);
    VPBS_HIP(hipGetLastError());
}
}  // namespace

bool key_expand_shape_ok(const vpbs_tfhe_params* prm, unsigned n_lwe, std::string* why) {
    if (!prm || prm->log_N < 1 || prm->log_N > 11 || prm->K < 2 || prm->K > 8 || prm->ELL < 1 || prm->ELL > 16) {
        *why = "unsupported parameters (log_N 1 .. 11, K 2 .. 8, ELL 1 .. 16)";
        return false;
    }
    // g < 2^24 is the tag's field; a grid has fewer than 2^31 workgroups
    if (n_lwe < 1 || n_lwe >= (1u << 24) || (size_t)n_lwe * prm->K * prm->ELL * prm->K >= ((size_t)1 << 31)) {
        *why = "n_lwe = " + std::to_string(n_lwe) + " is 0, or at least 2^24, or gives 2^31 polynomials or more";
        return false;
    }
    return true;
}

void key_expand_device(vpbs_ctx* c, const vpbs_tfhe_params& prm, unsigned n_lwe, uint64_t mask_seed, const uint64_t* bsk_bodies,
                       const uint64_t* ksk_bodies, int bodies_on_device, uint64_t* d_bsk, uint64_t* d_ksk) {
    const size_t body_words = ((size_t)prm.K * prm.ELL) << prm.log_N;   // of one GGSW
    u64* tmp[2] = {nullptr, nullptr};
    try {
        const struct {
            const u64* bodies;
            u64* out;
            size_t n_ggsw;
            u64 kind;
        } parts[2] = {{bsk_bodies, d_bsk, n_lwe, keygen::BSK_MASK}, {ksk_bodies, d_ksk, 1, keygen::KSK_MASK}};
        for (unsigned i = 0; i < 2; ++i) {
            if (!parts[i].bodies || !parts[i].out) continue;
            const u64* d_bodies = parts[i].bodies;
            if (!bodies_on_device) {
                tmp[i] = c->alloc_words(parts[i].n_ggsw * body_words);
                VPBS_HIP(hipMemcpyAsync(tmp[i], parts[i].bodies, sizeof(u64) * parts[i].n_ggsw * body_words, hipMemcpyHostToDevice, c->stream));
                d_bodies = tmp[i];
            }
            enqueue(c, prm, parts[i].n_ggsw, parts[i].kind, mask_seed, d_bodies, parts[i].out);
        }
        VPBS_HIP(vpbs::stream_sync(c->stream));   // the caller's bodies may go away
    } catch (...) {
        (void)vpbs::stream_sync(c->stream);
        c->release(tmp[0]);
        c->release(tmp[1]);
        throw;
    }
    c->release(tmp[0]);
    c->release(tmp[1]);
}
}  // namespace vpbs

extern "C" {

int vpbs_key_expand(vpbs_ctx* c, const vpbs_tfhe_params* prm, unsigned n_lwe, uint64_t mask_seed, const uint64_t* bsk_bodies,
                    const uint64_t* ksk_bodies, int bodies_on_device, uint64_t* bsk, uint64_t* ksk, int keys_on_device) {
    using namespace vpbs;
    if (!c) return VPBS_ERR_INVALID;
    auto refuse = [&](const std::string& what) {
        c->err = "vpbs_key_expand: " + what;
        return VPBS_ERR_INVALID;
    };
    std::string why;
    if (!key_expand_shape_ok(prm, n_lwe, &why)) return refuse(why);
    if (!bsk_bodies != !bsk || !ksk_bodies != !ksk) return refuse("bsk_bodies and bsk, and ksk_bodies and ksk, are given or NULL together");
    if ((bodies_on_device && ((((uintptr_t)bsk_bodies) | ((uintptr_t)ksk_bodies)) & 15)) || (keys_on_device && ((((uintptr_t)bsk) | ((uintptr_t)ksk)) & 15)))
        return refuse("device pointers must be 16-byte aligned");
    if (!bsk && !ksk) return VPBS_OK;
    const size_t ggsw_words = ((size_t)prm->K * prm->ELL * prm->K) << prm->log_N;
    u64 *d_bsk = nullptr, *d_ksk = nullptr;
    int rc = VPBS_OK;
    try {
        VPBS_HIP(hipSetDevice(c->device));
        d_bsk = !bsk ? nullptr : keys_on_device ? bsk : c->alloc_words((size_t)n_lwe * ggsw_words);
        d_ksk = !ksk ? nullptr : keys_on_device ? ksk : c->alloc_words(ggsw_words);
        key_expand_device(c, *prm, n_lwe, mask_seed, bsk_bodies, ksk_bodies, bodies_on_device, d_bsk, d_ksk);
        if (!keys_on_device) {
            if (bsk) VPBS_HIP(hipMemcpyAsync(bsk, d_bsk, sizeof(u64) * n_lwe * ggsw_words, hipMemcpyDeviceToHost, c->stream));
            if (ksk) VPBS_HIP(hipMemcpyAsync(ksk, d_ksk, sizeof(u64) * ggsw_words, hipMemcpyDeviceToHost, c->stream));
            VPBS_HIP(vpbs::stream_sync(c->stream));
        }
    } catch (const DeviceError& e) {
        (void)vpbs::stream_sync(c->stream);
        c->err = e.what;
        rc = e.status;
    }
    if (!keys_on_device) {
        c->release(d_bsk);
        c->release(d_ksk);
    }
    return rc;
}

}  // extern "C"
