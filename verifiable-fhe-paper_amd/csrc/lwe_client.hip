// The client side of an FHE program in batches: seeded LWE encryption of `count` messages, test vectors of arbitrary lookup
// tables, and decoding with exact noise statistics -- on gfx950 when a context is given, on the host when it is NULL (the second yardstick of
// the GPU tests, and what the CPU suite runs).
//
// Both kernels give ONE WAVE to a ciphertext, four waves to a workgroup, and walk the batch with a grid stride.  A batch worth a launch has
// thousands of rows, so the parallelism is in `count`; a row of n + 1 <= 16385 words is 12 trips of a wave at n = 728.  With the row inside one
// wave the inner product is summed by five xor shuffles and a lane-0 epilogue: no LDS, no barrier, and three idle waves less than a
// workgroup per row would have on the epilogue (a 64-bit division, the tallies).  Lane l touches words l, l + 64, ..: every load and store
// of a wave is 512 contiguous bytes.  Field addition is associative and commutative on canonical values, so the butterfly gives the host's word.
//   encrypt: 8 (n + 1) bytes written per row, none read but the key (n words, shared by all rows: L2); ~2 mix64 + 1 product per word.
//   decode:  8 (n + 1) bytes read per row, each word once; the key again from L2.  Statistics: lane 0 of a wave keeps limb sums in registers
//            over its rows, the workgroup combines them in LDS (ds atomics), and 76 global vector atomics per workgroup -- at most, zero words
//            are skipped -- add them to the launch's tally.  No workgroup waits for another; the host folds the tally into the caller's struct.
//   rotation: vpbs_lwe_rotation_batch is decode's shape and traffic with the chain's own rounding in the place of the inner
//            product: every word snapped and mod-switched by itself (rotation.h), the lane sums in u32, the same tally.
//   seeded:  vpbs_lwe_encrypt_seeded_batch is encrypt without the row -- 8 bytes written per ciphertext, its body -- and vpbs_lwe_expand_batch
//            writes the row back from a public mask_seed, the nonce and that body: 8 (n + 1) bytes written, 8 read, one mix64 per word.  The
//            split generator of keygen_streams.h; mix64 is not a cryptographic generator.
#include <algorithm>
#include <string>
#include <vector>

#include "context.h"
#include "kernels.h"
#include "keygen_streams.h"
#include "rotation.h"

namespace vpbs {
namespace lwe_client {
constexpr unsigned THREADS = 256, WAVE = 64, WAVES = THREADS / WAVE, MAX_BLOCKS = 2048;

// ---- one decoded ciphertext, in integers (include/vpbs_prover.h states the definitions) ----
struct Decoded {
    u64 msg, err, abs;   // err: two's complement; abs = |err| <= (p - 1) / 2
    bool neg, fail;
};
GL_HD Decoded decode_one(u64 phase, u64 delta, u64 modulus, bool has_expected, u64 expected) {
    Decoded d;
    // floor((phase + floor(delta / 2)) / delta) without the 65-bit sum: the quotient of phase, plus one when the remainder reaches delta - half
    u64 q = phase / delta;
    if (phase % delta >= delta - (delta >> 1)) ++q;          // q <= phase < p: no overflow
    d.msg = q % modulus;
    const u64 ref = has_expected ? expected : d.msg;
    const u64 diff = gl::sub(phase, gl::mul(gl::canon(ref), gl::canon(delta)));
    d.neg = diff > (gl::P - 1) / 2;                          // centred into (-p/2, p/2]
    d.abs = d.neg ? gl::P - diff : diff;
    d.err = d.neg ? (u64)0 - d.abs : d.abs;
    d.fail = has_expected && d.msg != expected % modulus;
    return d;
}

// ---- the tally of one launch: 32-bit limbs summed in 64-bit counters (a launch has fewer than 2^31 rows, so none overflows) ----
enum Tally : unsigned { T_COUNT = 0, T_FAIL = 1, T_MAX = 2, T_ABS = 3 /* 2 limbs */, T_SQ = 5 /* 4 limbs */, T_NEG = 9 /* |err| of the negative ones, 2 limbs */,
                        T_HIST = 11 /* 65 bins */, T_WORDS = 76 };
GL_HD unsigned bit_length(u64 v) { return v ? 64u - (unsigned)__builtin_clzll(v) : 0u; }
// everything but the histogram bin
GL_HD void tally_add(u64* t, const Decoded& d) {
    t[T_COUNT] += 1;
    t[T_FAIL] += d.fail ? 1 : 0;
    t[T_MAX] = d.abs > t[T_MAX] ? d.abs : t[T_MAX];
    t[T_ABS] += d.abs & 0xFFFFFFFFull;
    t[T_ABS + 1] += d.abs >> 32;
    const unsigned __int128 sq = (unsigned __int128)d.abs * d.abs;
    const u64 lo = (u64)sq, hi = (u64)(sq >> 64);
    t[T_SQ] += lo & 0xFFFFFFFFull;
    t[T_SQ + 1] += lo >> 32;
    t[T_SQ + 2] += hi & 0xFFFFFFFFull;
    t[T_SQ + 3] += hi >> 32;
    if (d.neg) {
        t[T_NEG] += d.abs & 0xFFFFFFFFull;
        t[T_NEG + 1] += d.abs >> 32;
    }
}

// w (n little-endian words) += v << bit, carries dropped past the top word (two's complement for sum_signed)
inline void add_at(u64* w, unsigned n, u64 v, unsigned bit) {
    unsigned __int128 carry = (unsigned __int128)v << (bit % 64);
    for (unsigned i = bit / 64; i < n; ++i) {
        carry += w[i];
        w[i] = (u64)carry;
        carry >>= 64;
    }
}
inline void sub_words(u64* w, const u64* v, unsigned n) {
    unsigned borrow = 0;
    for (unsigned i = 0; i < n; ++i) {
        const unsigned __int128 d = (unsigned __int128)w[i] - v[i] - borrow;
        w[i] = (u64)d;
        borrow = (unsigned)((d >> 64) & 1);
    }
}
void fold(const u64* t, vpbs_noise_stats* s) {
    s->count += t[T_COUNT];
    s->failures += t[T_FAIL];
    s->max_abs = std::max<u64>(s->max_abs, t[T_MAX]);
    for (unsigned l = 0; l < 2; ++l) add_at(s->sum_abs, 2, t[T_ABS + l], 32 * l);
    for (unsigned l = 0; l < 4; ++l) add_at(s->sum_sq, 3, t[T_SQ + l], 32 * l);
    // sum_signed += sum |err| - 2 sum over the negative ones of |err|
    u64 neg[2] = {0, 0};
    for (unsigned l = 0; l < 2; ++l) {
        add_at(s->sum_signed, 2, t[T_ABS + l], 32 * l);
        add_at(neg, 2, t[T_NEG + l], 32 * l);
    }
    sub_words(s->sum_signed, neg, 2);
    sub_words(s->sum_signed, neg, 2);
    for (unsigned b = 0; b < 65; ++b) s->hist[b] += t[T_HIST + b];
}

// ---- device ----
__device__ __forceinline__ u64 shfl_xor64(u64 x, int mask) {
    const u32 lo = (u32)__shfl_xor((int)(u32)x, mask, WAVE), hi = (u32)__shfl_xor((int)(u32)(x >> 32), mask, WAVE);
    return ((u64)hi << 32) | lo;
}
// the field sum of the wave's 64 canonical values, in every lane
__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) v = gl::add(v, shfl_xor64(v, m));
    return v;
}

struct EncryptJob {
    u64 seed, m_sigma, nonce0;
    unsigned n_lwe;
    size_t count;
};
// row c = vpbs_lwe_encrypt(params, s_lwe, messages[c], nonce0 + c); a message at or above p leaves its row untouched and its index in *first_bad
__global__ void __launch_bounds__(THREADS) lwe_encrypt_batch_kernel(EncryptJob j, const u64* __restrict__ s_lwe, const u64* __restrict__ messages,
                                                                    u64* __restrict__ cts, unsigned long long* __restrict__ first_bad) {
    using namespace keygen;
    const unsigned lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    for (size_t c = (size_t)blockIdx.x * WAVES + wave; c < j.count; c += (size_t)gridDim.x * WAVES) {
        const u64 m = messages[c];
        if (m >= gl::P) {   // the same for every lane of the wave
            if (lane == 0) atomicMin(first_bad, (unsigned long long)c);
            continue;
        }
        const u64 km = stream(j.seed, tag(LWE_MASK, j.nonce0 + c, 0, 0));
        u64* row = cts + c * ((size_t)j.n_lwe + 1);
        u64 acc = 0;
        for (unsigned i = lane; i < j.n_lwe; i += WAVE) {
            const u64 a = field(draw(km, i));
            row[i] = a;
            acc = gl::add(acc, gl::mul(a, gl::canon(s_lwe[i])));   // canon(w) = w % p for a 64-bit word
        }
        acc = wave_sum(acc);
        if (lane == 0) {
            const u64 ke = stream(j.seed, tag(LWE_NOISE, j.nonce0 + c, 0, 0));
            row[j.n_lwe] = gl::add(acc, gl::add(m, noise(ke, 0, j.m_sigma)));
        }
    }
}

// ---- seeded ciphertexts (the split generator of keygen_streams.h): the client keeps the body word, the server rebuilds the mask ----
struct SeededJob {
    u64 seed, mask_seed, m_sigma, nonce0;
    unsigned n_lwe;
    size_t count;
};
// the body word of one seeded ciphertext on the host, and of lwe_encrypt_seeded_kernel's lane 0 up to the inner product
GL_HD u64 seeded_body_tail(const SeededJob& j, size_t c, u64 m) {
    return gl::add(m, keygen::noise(keygen::split_stream(j.seed, j.mask_seed, keygen::LWE_NOISE, j.nonce0 + c, 0, 0), 0, j.m_sigma));
}
// bodies[c] = word n_lwe of lwe_encrypt_batch_kernel's row c under the split generator; the mask is drawn, used and never stored
__global__ void __launch_bounds__(THREADS) lwe_encrypt_seeded_kernel(SeededJob j, const u64* __restrict__ s_lwe, const u64* __restrict__ messages,
                                                                     u64* __restrict__ bodies, unsigned long long* __restrict__ first_bad) {
    using namespace keygen;
    const unsigned lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    for (size_t c = (size_t)blockIdx.x * WAVES + wave; c < j.count; c += (size_t)gridDim.x * WAVES) {
        const u64 m = messages[c];
        if (m >= gl::P) {   // the same for every lane of the wave
            if (lane == 0) atomicMin(first_bad, (unsigned long long)c);
            continue;
        }
        const u64 km = split_stream(j.seed, j.mask_seed, LWE_MASK, j.nonce0 + c, 0, 0);
        u64 acc = 0;
        for (unsigned i = lane; i < j.n_lwe; i += WAVE) acc = gl::add(acc, gl::mul(field(draw(km, i)), gl::canon(s_lwe[i])));
        acc = wave_sum(acc);
        if (lane == 0) bodies[c] = gl::add(acc, seeded_body_tail(j, c, m));
    }
}
// row c = the n_lwe mask words of nonce nonce0 + c under mask_seed, then bodies[c] unchanged; lane l writes words l, l + 64, ..
__global__ void __launch_bounds__(THREADS) lwe_expand_kernel(u64 mask_seed, u64 nonce0, unsigned n_lwe, size_t count, const u64* __restrict__ bodies,
                                                             u64* __restrict__ cts) {
    using namespace keygen;
    const unsigned lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    for (size_t c = (size_t)blockIdx.x * WAVES + wave; c < count; c += (size_t)gridDim.x * WAVES) {
        const u64 km = stream(mask_seed, tag(LWE_MASK, nonce0 + c, 0, 0));
        u64* row = cts + c * ((size_t)n_lwe + 1);
        for (unsigned i = lane; i <= n_lwe; i += WAVE) row[i] = i < n_lwe ? field(draw(km, i)) : bodies[c];
    }
}

// ---- the tally of a launch, shared by the decode and the rotation kernel: lane 0 of a wave keeps the sums over its rows in registers
// (tally_add) and the histogram bin in LDS; the workgroup combines in LDS and adds its nonzero words to the launch's tally ----
__device__ __forceinline__ void tally_open(unsigned long long* lds) {
    for (unsigned i = threadIdx.x; i < T_WORDS; i += THREADS) lds[i] = 0;
    __syncthreads();
}
__device__ __forceinline__ void tally_row(u64* mine, unsigned long long* lds, const Decoded& d) {
    tally_add(mine, d);
    atomicAdd(&lds[T_HIST + bit_length(d.abs)], 1ull);
}
__device__ __forceinline__ void tally_close(const u64* mine, unsigned long long* lds, unsigned long long* __restrict__ tally, unsigned lane) {
    if (lane == 0) {
#pragma unroll
        for (unsigned i = 0; i < T_HIST; ++i) {
            if (i == T_MAX) atomicMax(&lds[i], (unsigned long long)mine[i]);
            else if (mine[i]) atomicAdd(&lds[i], (unsigned long long)mine[i]);
        }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < T_WORDS; i += THREADS) {
        const unsigned long long v = lds[i];
        if (!v) continue;
        if (i == T_MAX) atomicMax(&tally[i], v);
        else atomicAdd(&tally[i], v);
    }
}

struct DecodeJob {
    u64 delta, modulus;
    unsigned n_lwe;
    size_t count;
};
__global__ void __launch_bounds__(THREADS) lwe_decode_batch_kernel(DecodeJob j, const u64* __restrict__ s_lwe, const u64* __restrict__ cts,
                                                                   const u64* __restrict__ expected, u64* __restrict__ phase_out,
                                                                   u64* __restrict__ msg_out, u64* __restrict__ err_out,
                                                                   unsigned long long* __restrict__ tally) {
    __shared__ unsigned long long lds[T_WORDS];
    const unsigned lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    if (tally) tally_open(lds);
    u64 mine[T_HIST] = {};   // lane 0's sums over the rows of this wave
    for (size_t c = (size_t)blockIdx.x * WAVES + wave; c < j.count; c += (size_t)gridDim.x * WAVES) {
        const u64* row = cts + c * ((size_t)j.n_lwe + 1);
        u64 acc = 0, body = 0;
#pragma unroll 4
        for (unsigned i = lane; i <= j.n_lwe; i += WAVE) {
            const u64 w = gl::canon(row[i]);
            if (i < j.n_lwe) acc = gl::add(acc, gl::mul(gl::canon(s_lwe[i]), w));
            else body = w;   // one lane of the wave
        }
        acc = wave_sum(acc);
        body = wave_sum(body);
        if (lane == 0) {
            const u64 phase = gl::sub(body, acc);
            const Decoded d = decode_one(phase, j.delta, j.modulus, expected != nullptr, expected ? expected[c] : 0);
            if (phase_out) phase_out[c] = phase;
            if (msg_out) msg_out[c] = d.msg;
            if (err_out) err_out[c] = d.err;
            if (tally) tally_row(mine, lds, d);
        }
    }
    if (tally) tally_close(mine, lds, tally, lane);
}

// ---- rotation margins (rotation.h states the definitions): the decode kernel's shape with integer lane sums ----
// a margin in the tally's terms: msg = idx, err = dev
GL_HD Decoded as_decoded(const rotation::Margin& m) {
    Decoded d;
    d.msg = m.idx;
    d.abs = m.abs;
    d.neg = m.neg;
    d.err = m.neg ? (u64)0 - m.abs : m.abs;
    d.fail = m.fail;
    return d;
}
struct RotationJob {
    unsigned n_lwe, log_n, log_slots, p;
    size_t count;
};
// One wave per row, every row word read once, the key from L2.  A lane adds the rotations of its words -- the body's, and a mask word's when
// its key bit is 1 -- in u32 (2N divides 2^32); five xor shuffles give every lane the sum; lane 0 writes mu, idx and dev and tallies.  A key
// word that is neither 0 nor 1 after reduction leaves the lowest such index in *first_bad (the same words for every row).
__global__ void __launch_bounds__(THREADS) lwe_rotation_batch_kernel(RotationJob j, const u64* __restrict__ s_lwe, const u64* __restrict__ cts,
                                                                     const u64* __restrict__ expected, u64* __restrict__ rot_out,
                                                                     u64* __restrict__ idx_out, u64* __restrict__ dev_out,
                                                                     unsigned long long* __restrict__ tally,
                                                                     unsigned long long* __restrict__ first_bad) {
    __shared__ unsigned long long lds[T_WORDS];
    const unsigned lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    if (tally) tally_open(lds);
    u64 mine[T_HIST] = {};   // lane 0's sums over the rows of this wave
    for (size_t c = (size_t)blockIdx.x * WAVES + wave; c < j.count; c += (size_t)gridDim.x * WAVES) {
        const u64* row = cts + c * ((size_t)j.n_lwe + 1);
        unsigned acc = 0;
#pragma unroll 4
        for (unsigned i = lane; i <= j.n_lwe; i += WAVE) {
            const u64 w = row[i];
            if (i < j.n_lwe) {
                const u64 s = gl::canon(s_lwe[i]);
                if (s > 1) atomicMin(first_bad, (unsigned long long)i);
                acc += s == 1 ? rotation::word_rotation(w, j.log_n, j.log_slots, false) : 0u;
            } else {
                acc += rotation::word_rotation(w, j.log_n, j.log_slots, true);   // one lane of the wave
            }
        }
#pragma unroll
        for (int m = WAVE / 2; m >= 1; m >>= 1) acc += (unsigned)__shfl_xor((int)acc, m, WAVE);
        if (lane == 0) {
            const rotation::Margin m = rotation::margin(acc, j.log_n, j.p, expected != nullptr, expected ? expected[c] : 0);
            const Decoded d = as_decoded(m);
            if (rot_out) rot_out[c] = m.mu;
            if (idx_out) idx_out[c] = m.idx;
            if (dev_out) dev_out[c] = d.err;
            if (tally) tally_row(mine, lds, d);
        }
    }
    if (tally) tally_close(mine, lds, tally, lane);
}

unsigned blocks_for(size_t count) { return (unsigned)std::min<size_t>((count + WAVES - 1) / WAVES, MAX_BLOCKS); }

// device scratch of one call, released after the stream has drained
struct Scratch {
    vpbs_ctx* c;
    std::vector<u64*> bufs;
    explicit Scratch(vpbs_ctx* ctx) : c(ctx) {}
    u64* words(size_t n) {
        bufs.push_back(c->alloc_words(n ? n : 1));
        return bufs.back();
    }
    // a device copy of a host array
    const u64* upload(const u64* host, size_t n) {
        u64* d = words(n);
        VPBS_HIP(hipMemcpyAsync(d, host, sizeof(u64) * n, hipMemcpyHostToDevice, c->stream));
        return d;
    }
    ~Scratch() {
        if (bufs.empty()) return;
        (void)vpbs::stream_sync(c->stream);
        for (u64* p : bufs) c->release(p);
    }
};
int refuse(vpbs_ctx* c, const std::string& what) {
    if (c) c->err = what;
    return VPBS_ERR_INVALID;
}
constexpr size_t MAX_COUNT = (size_t)1 << 31;
}  // namespace lwe_client
}  // namespace vpbs

using vpbs::u64;

extern "C" {

int vpbs_lwe_encrypt_batch(vpbs_ctx* c, const vpbs_keygen_params* k, const uint64_t* s_lwe, int key_on_device, const uint64_t* messages,
                           size_t count, uint64_t nonce0, uint64_t* cts_out, int on_device) {
    using namespace vpbs;
    using namespace vpbs::lwe_client;
    const char* who = "vpbs_lwe_encrypt_batch: ";
    if (!keygen::params_ok(k)) return refuse(c, std::string(who) + "unsupported parameters");
    if (!s_lwe || (count && (!messages || !cts_out))) return refuse(c, std::string(who) + "null pointer");
    if (!c && (key_on_device || on_device)) return refuse(c, std::string(who) + "device pointers need a context");
    if (nonce0 > ((u64)1 << 24) || count > ((u64)1 << 24) - nonce0)
        return refuse(c, std::string(who) + "nonce0 + count exceeds 2^24: ciphertext " +
                             std::to_string(((u64)1 << 24) - std::min<u64>(nonce0, (u64)1 << 24)) + " is the first without a nonce");
    if (count == 0) return VPBS_OK;
    const size_t ct_words = (size_t)k->n_lwe + 1;
    auto bad_message = [&](size_t i) { return refuse(c, std::string(who) + "message " + std::to_string(i) + " is not below p"); };
    if (!on_device)
        for (size_t i = 0; i < count; ++i)
            if (messages[i] >= gl::P) return bad_message(i);
    if (!c) {
        for (size_t i = 0; i < count; ++i)
            if (int rc = vpbs_lwe_encrypt(k, s_lwe, messages[i], nonce0 + i, cts_out + i * ct_words)) return rc;
        return VPBS_OK;
    }
    try {
        VPBS_HIP(hipSetDevice(c->device));
        Scratch tmp(c);
        const u64* d_key = key_on_device ? s_lwe : tmp.upload(s_lwe, k->n_lwe);
        const u64* d_msg = on_device ? messages : tmp.upload(messages, count);
        u64* d_out = on_device ? cts_out : tmp.words(count * ct_words);
        u64* d_bad = tmp.words(1);
        VPBS_HIP(hipMemsetAsync(d_bad, 0xFF, sizeof(u64), c->stream));
        const EncryptJob job{k->seed, keygen::sigma_to_int(k->sigma_lwe), nonce0, k->n_lwe, count};
        hipLaunchKernelGGL(lwe_encrypt_batch_kernel, dim3(blocks_for(count)), dim3(THREADS), 0, c->stream, job, d_key, d_msg, d_out,
                           (unsigned long long*)d_bad);
        VPBS_HIP(hipGetLastError());
        u64 bad = 0;
        VPBS_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        if (!on_device) VPBS_HIP(hipMemcpyAsync(cts_out, d_out, sizeof(u64) * count * ct_words, hipMemcpyDeviceToHost, c->stream));
        VPBS_HIP(vpbs::stream_sync(c->stream));
        if (bad != ~(u64)0) return bad_message((size_t)bad);
        return VPBS_OK;
    } catch (const DeviceError& e) {
        c->err = e.what;
        return e.status;
    }
}

int vpbs_lwe_encrypt_seeded_batch(vpbs_ctx* c, const vpbs_keygen_params* k, uint64_t mask_seed, const uint64_t* s_lwe, int key_on_device,
                                  const uint64_t* messages, size_t count, uint64_t nonce0, uint64_t* bodies_out, int on_device) {
    using namespace vpbs;
    using namespace vpbs::lwe_client;
    const char* who = "vpbs_lwe_encrypt_seeded_batch: ";
    // the refusals of vpbs_lwe_encrypt_batch
    if (!keygen::params_ok(k)) return refuse(c, std::string(who) + "unsupported parameters");
    if (!s_lwe || (count && (!messages || !bodies_out))) return refuse(c, std::string(who) + "null pointer");
    if (!c && (key_on_device || on_device)) return refuse(c, std::string(who) + "device pointers need a context");
    if (nonce0 > ((u64)1 << 24) || count > ((u64)1 << 24) - nonce0)
        return refuse(c, std::string(who) + "nonce0 + count exceeds 2^24: ciphertext " +
                             std::to_string(((u64)1 << 24) - std::min<u64>(nonce0, (u64)1 << 24)) + " is the first without a nonce");
    if (count == 0) return VPBS_OK;
    auto bad_message = [&](size_t i) { return refuse(c, std::string(who) + "message " + std::to_string(i) + " is not below p"); };
    if (!on_device)
        for (size_t i = 0; i < count; ++i)
            if (messages[i] >= gl::P) return bad_message(i);
    const SeededJob job{k->seed, mask_seed, keygen::sigma_to_int(k->sigma_lwe), nonce0, k->n_lwe, count};
    if (!c) {
        for (size_t i = 0; i < count; ++i) {
            const u64 km = keygen::split_stream(job.seed, job.mask_seed, keygen::LWE_MASK, nonce0 + i, 0, 0);
            u64 body = seeded_body_tail(job, i, messages[i]);
            for (unsigned x = 0; x < k->n_lwe; ++x)
                if (s_lwe[x]) body = gl::add(body, gl::mul(keygen::field(keygen::draw(km, x)), s_lwe[x] % gl::P));
            bodies_out[i] = body;
        }
        return VPBS_OK;
    }
    try {
        VPBS_HIP(hipSetDevice(c->device));
        Scratch tmp(c);
        const u64* d_key = key_on_device ? s_lwe : tmp.upload(s_lwe, k->n_lwe);
        const u64* d_msg = on_device ? messages : tmp.upload(messages, count);
        u64* d_out = on_device ? bodies_out : tmp.words(count);
        u64* d_bad = tmp.words(1);
        VPBS_HIP(hipMemsetAsync(d_bad, 0xFF, sizeof(u64), c->stream));
        hipLaunchKernelGGL(lwe_encrypt_seeded_kernel, dim3(blocks_for(count)), dim3(THREADS), 0, c->stream, job, d_key, d_msg, d_out,
                           (unsigned long long*)d_bad);
        VPBS_HIP(hipGetLastError());
        u64 bad = 0;
        VPBS_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        if (!on_device) VPBS_HIP(hipMemcpyAsync(bodies_out, d_out, sizeof(u64) * count, hipMemcpyDeviceToHost, c->stream));
        VPBS_HIP(vpbs::stream_sync(c->stream));
        if (bad != ~(u64)0) return bad_message((size_t)bad);
        return VPBS_OK;
    } catch (const DeviceError& e) {
        c->err = e.what;
        return e.status;
    }
}

int vpbs_lwe_expand_batch(vpbs_ctx* c, unsigned n_lwe, uint64_t mask_seed, uint64_t nonce0, const uint64_t* bodies, size_t count, uint64_t* cts_out,
                          int on_device) {
    using namespace vpbs;
    using namespace vpbs::lwe_client;
    const char* who = "vpbs_lwe_expand_batch: ";
    if (n_lwe < 1 || n_lwe >= (1u << 24)) return refuse(c, std::string(who) + "n_lwe must be 1 .. 2^24 - 1");
    if (count && (!bodies || !cts_out)) return refuse(c, std::string(who) + "null pointer");
    if (!c && on_device) return refuse(c, std::string(who) + "device pointers need a context");
    if (nonce0 > ((u64)1 << 24) || count > ((u64)1 << 24) - nonce0)
        return refuse(c, std::string(who) + "nonce0 + count exceeds 2^24: ciphertext " +
                             std::to_string(((u64)1 << 24) - std::min<u64>(nonce0, (u64)1 << 24)) + " is the first without a nonce");
    if (count == 0) return VPBS_OK;
    const size_t ct_words = (size_t)n_lwe + 1;
    if (!c) {
        for (size_t i = 0; i < count; ++i) {
            const u64 km = keygen::stream(mask_seed, keygen::tag(keygen::LWE_MASK, nonce0 + i, 0, 0));
            u64* row = cts_out + i * ct_words;
            for (unsigned x = 0; x < n_lwe; ++x) row[x] = keygen::field(keygen::draw(km, x));
            row[n_lwe] = bodies[i];
        }
        return VPBS_OK;
    }
    try {
        VPBS_HIP(hipSetDevice(c->device));
        Scratch tmp(c);
        const u64* d_bodies = on_device ? bodies : tmp.upload(bodies, count);
        u64* d_out = on_device ? cts_out : tmp.words(count * ct_words);
        hipLaunchKernelGGL(lwe_expand_kernel, dim3(blocks_for(count)), dim3(THREADS), 0, c->stream, mask_seed, nonce0, n_lwe, count, d_bodies, d_out);
        VPBS_HIP(hipGetLastError());
        if (!on_device) VPBS_HIP(hipMemcpyAsync(cts_out, d_out, sizeof(u64) * count * ct_words, hipMemcpyDeviceToHost, c->stream));
        VPBS_HIP(vpbs::stream_sync(c->stream));
        return VPBS_OK;
    } catch (const DeviceError& e) {
        c->err = e.what;
        return e.status;
    }
}

int vpbs_lut_testv(unsigned log_N, unsigned p, const uint64_t* table, uint64_t delta, uint64_t* testv) {
    if (!table || !testv || log_N < 1 || log_N > 16 || p < 1 || (p & (p - 1)) || p > (1u << log_N)) return VPBS_ERR_INVALID;
    for (unsigned i = 0; i < p; ++i)
        if (table[i] >= 2 * (u64)p) return VPBS_ERR_INVALID;
    // vpbs_testv with table[i] in the place of i: blocks of N / p equal coefficients, then Poly::left_shift(block / 2), wrapped terms negated
    const size_t n = (size_t)1 << log_N, block = n / p, s = block / 2;
    const u64 d = gl::canon(delta);
    auto coeff = [&](size_t i) { return gl::mul(table[i / block], d); };
    for (size_t i = 0; i < n; ++i) testv[i] = i + s < n ? coeff(i + s) : gl::neg(coeff(i + s - n));
    return VPBS_OK;
}

int vpbs_lwe_decode_batch(vpbs_ctx* c, const uint64_t* s_lwe, int key_on_device, const uint64_t* cts, size_t count, unsigned n_lwe, uint64_t delta,
                          uint64_t modulus, const uint64_t* expected, uint64_t* phase_out, uint64_t* msg_out, uint64_t* err_out,
                          vpbs_noise_stats* stats, int on_device) {
    using namespace vpbs;
    using namespace vpbs::lwe_client;
    const char* who = "vpbs_lwe_decode_batch: ";
    if (!s_lwe || (count && !cts)) return refuse(c, std::string(who) + "null pointer");
    if (n_lwe < 1 || n_lwe >= (1u << 24) || delta < 1 || modulus < 1) return refuse(c, std::string(who) + "n_lwe, delta and modulus must be at least 1");
    if (on_device < 0 || on_device > VPBS_DECODE_OUTPUTS_TO_HOST) return refuse(c, std::string(who) + "on_device must be 0, 1 or 2");
    if (!c && (key_on_device || on_device)) return refuse(c, std::string(who) + "device pointers need a context");
    if (count > MAX_COUNT) return refuse(c, std::string(who) + "more than 2^31 ciphertexts in one call");
    if (count == 0) return VPBS_OK;
    const size_t ct_words = (size_t)n_lwe + 1;
    if (!c) {
        u64 t[T_WORDS] = {};
        for (size_t i = 0; i < count; ++i) {
            u64 phase = 0;
            if (int rc = vpbs_lwe_decrypt(s_lwe, cts + i * ct_words, n_lwe, &phase)) return rc;
            const Decoded d = decode_one(phase, delta, modulus, expected != nullptr, expected ? expected[i] : 0);
            if (phase_out) phase_out[i] = phase;
            if (msg_out) msg_out[i] = d.msg;
            if (err_out) err_out[i] = d.err;
            tally_add(t, d);
            t[T_HIST + bit_length(d.abs)] += 1;
        }
        if (stats) fold(t, stats);
        return VPBS_OK;
    }
    try {
        VPBS_HIP(hipSetDevice(c->device));
        Scratch tmp(c);
        const bool in_dev = on_device != 0, out_dev = on_device == 1;
        const u64* d_key = key_on_device ? s_lwe : tmp.upload(s_lwe, n_lwe);
        const u64* d_cts = in_dev ? cts : tmp.upload(cts, count * ct_words);
        const u64* d_exp = !expected ? nullptr : in_dev ? expected : tmp.upload(expected, count);
        u64* host_out[3] = {phase_out, msg_out, err_out};
        u64* d_out[3];
        for (unsigned o = 0; o < 3; ++o) d_out[o] = !host_out[o] ? nullptr : out_dev ? host_out[o] : tmp.words(count);
        u64* d_tally = nullptr;
        if (stats) {
            d_tally = tmp.words(T_WORDS);
            VPBS_HIP(hipMemsetAsync(d_tally, 0, sizeof(u64) * T_WORDS, c->stream));
        }
        const DecodeJob job{delta, modulus, n_lwe, count};
        hipLaunchKernelGGL(lwe_decode_batch_kernel, dim3(blocks_for(count)), dim3(THREADS), 0, c->stream, job, d_key, d_cts, d_exp, d_out[0], d_out[1],
                           d_out[2], (unsigned long long*)d_tally);
        VPBS_HIP(hipGetLastError());
        u64 t[T_WORDS] = {};
        if (stats) VPBS_HIP(hipMemcpyAsync(t, d_tally, sizeof(u64) * T_WORDS, hipMemcpyDeviceToHost, c->stream));
        if (!out_dev)
            for (unsigned o = 0; o < 3; ++o)
                if (host_out[o]) VPBS_HIP(hipMemcpyAsync(host_out[o], d_out[o], sizeof(u64) * count, hipMemcpyDeviceToHost, c->stream));
        VPBS_HIP(vpbs::stream_sync(c->stream));
        if (stats) fold(t, stats);
        return VPBS_OK;
    } catch (const DeviceError& e) {
        c->err = e.what;
        return e.status;
    }
}

int vpbs_lwe_rotation_batch(vpbs_ctx* c, const uint64_t* s_lwe, int key_on_device, const uint64_t* cts, size_t count, unsigned n_lwe, unsigned log_N,
                            unsigned log_slots, unsigned p, const uint64_t* expected, uint64_t* rot_out, uint64_t* idx_out, uint64_t* dev_out,
                            vpbs_noise_stats* stats, int on_device) {
    using namespace vpbs;
    using namespace vpbs::lwe_client;
    const char* who = "vpbs_lwe_rotation_batch: ";
    if (!s_lwe || (count && !cts)) return refuse(c, std::string(who) + "null pointer");
    if (n_lwe < 1 || n_lwe >= (1u << 24)) return refuse(c, std::string(who) + "n_lwe must be 1 .. 2^24 - 1");
    if (log_N < 1 || log_N > 16) return refuse(c, std::string(who) + "log_N must be 1 .. 16");
    if (log_slots > log_N) return refuse(c, std::string(who) + "log_slots exceeds log_N");
    if (p < 1 || (p & (p - 1)) || p > (1u << log_N)) return refuse(c, std::string(who) + "p must be a power of two, 1 .. N");
    if (on_device < 0 || on_device > VPBS_DECODE_OUTPUTS_TO_HOST) return refuse(c, std::string(who) + "on_device must be 0, 1 or 2");
    if (!c && (key_on_device || on_device)) return refuse(c, std::string(who) + "device pointers need a context");
    if (count > MAX_COUNT) return refuse(c, std::string(who) + "more than 2^31 ciphertexts in one call");
    auto bad_key = [&](size_t i) { return refuse(c, std::string(who) + "key word " + std::to_string(i) + " is neither 0 nor 1"); };
    if (!key_on_device)
        for (unsigned i = 0; i < n_lwe; ++i)
            if (gl::canon(s_lwe[i]) > 1) return bad_key(i);
    if (count == 0) return VPBS_OK;
    const size_t ct_words = (size_t)n_lwe + 1;
    if (!c) {
        u64 t[T_WORDS] = {};
        for (size_t r = 0; r < count; ++r) {
            const u64* row = cts + r * ct_words;
            unsigned acc = rotation::word_rotation(row[n_lwe], log_N, log_slots, true);
            for (unsigned i = 0; i < n_lwe; ++i)
                if (gl::canon(s_lwe[i])) acc += rotation::word_rotation(row[i], log_N, log_slots, false);
            const rotation::Margin m = rotation::margin(acc, log_N, p, expected != nullptr, expected ? expected[r] : 0);
            const Decoded d = as_decoded(m);
            if (rot_out) rot_out[r] = m.mu;
            if (idx_out) idx_out[r] = m.idx;
            if (dev_out) dev_out[r] = d.err;
            tally_add(t, d);
            t[T_HIST + bit_length(d.abs)] += 1;
        }
        if (stats) fold(t, stats);
        return VPBS_OK;
    }
    try {
        VPBS_HIP(hipSetDevice(c->device));
        Scratch tmp(c);
        const bool in_dev = on_device != 0, out_dev = on_device == 1;
        const u64* d_key = key_on_device ? s_lwe : tmp.upload(s_lwe, n_lwe);
        const u64* d_cts = in_dev ? cts : tmp.upload(cts, count * ct_words);
        const u64* d_exp = !expected ? nullptr : in_dev ? expected : tmp.upload(expected, count);
        u64* host_out[3] = {rot_out, idx_out, dev_out};
        u64* d_out[3];
        for (unsigned o = 0; o < 3; ++o) d_out[o] = !host_out[o] ? nullptr : out_dev ? host_out[o] : tmp.words(count);
        u64* d_tally = nullptr;
        if (stats) {
            d_tally = tmp.words(T_WORDS);
            VPBS_HIP(hipMemsetAsync(d_tally, 0, sizeof(u64) * T_WORDS, c->stream));
        }
        u64* d_bad = tmp.words(1);
        VPBS_HIP(hipMemsetAsync(d_bad, 0xFF, sizeof(u64), c->stream));
        const RotationJob job{n_lwe, log_N, log_slots, p, count};
        hipLaunchKernelGGL(lwe_rotation_batch_kernel, dim3(blocks_for(count)), dim3(THREADS), 0, c->stream, job, d_key, d_cts, d_exp, d_out[0],
                           d_out[1], d_out[2], (unsigned long long*)d_tally, (unsigned long long*)d_bad);
        VPBS_HIP(hipGetLastError());
        u64 t[T_WORDS] = {}, bad = 0;
        VPBS_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        if (stats) VPBS_HIP(hipMemcpyAsync(t, d_tally, sizeof(u64) * T_WORDS, hipMemcpyDeviceToHost, c->stream));
        if (!out_dev)
            for (unsigned o = 0; o < 3; ++o)
                if (host_out[o]) VPBS_HIP(hipMemcpyAsync(host_out[o], d_out[o], sizeof(u64) * count, hipMemcpyDeviceToHost, c->stream));
        VPBS_HIP(vpbs::stream_sync(c->stream));
        if (bad != ~(u64)0) return bad_key((size_t)bad);   // a key on the device: found there; the struct is left as it was
        if (stats) fold(t, stats);
        return VPBS_OK;
    } catch (const DeviceError& e) {
        c->err = e.what;
        return e.status;
    }
}

}  // extern "C"
