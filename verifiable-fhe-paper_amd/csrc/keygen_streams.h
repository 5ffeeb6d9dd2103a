// The seeded generator of csrc/keygen.hip (its header states the spec; tests/tfhe_oracle.py `Seeded` restates it bit for bit), in a header
// so that the batched client side (csrc/lwe_client.hip) draws from the very same functions as vpbs_keygen and vpbs_lwe_encrypt.
#pragma once
#include <cmath>

#include "../../include/vpbs_prover.h"
#include "gl.h"

namespace vpbs {
namespace keygen {
using u64 = gl::u64;
constexpr u64 G = 0x9E3779B97F4A7C15ull;
enum Kind : u64 { S_TO = 1, S_GLWE = 2, BSK_MASK = 3, BSK_NOISE = 4, KSK_MASK = 5, KSK_NOISE = 6, LWE_MASK = 7, LWE_NOISE = 8 };

GL_HD u64 mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
GL_HD u64 tag(u64 kind, u64 a, u64 b, u64 c) { return (kind << 56) | (a << 32) | (b << 16) | c; }
GL_HD u64 stream(u64 seed, u64 t) { return mix64(seed + G * (t + 1)); }
GL_HD u64 draw(u64 stream_key, u64 i) { return mix64(stream_key + G * (i + 1)); }
// The SPLIT generator of the seeded calls (vpbs_keygen_seeded, vpbs_key_expand, vpbs_lwe_encrypt_seeded_batch, vpbs_lwe_expand_batch), stated
// once: the streams of the three MASK kinds are keyed by a public mask_seed, the streams of every other kind (the secrets, the noise) by the
// private seed.  Tags, draw, field and noise are the ones above and below; with mask_seed == seed this is the one-seed generator.
// mix64 is NOT a cryptographic generator: the split says who may know which seed, it does not make the noise stream fit for production.
GL_HD bool is_mask_kind(u64 kind) { return kind == BSK_MASK || kind == KSK_MASK || kind == LWE_MASK; }
GL_HD u64 split_stream(u64 seed, u64 mask_seed, u64 kind, u64 a, u64 b, u64 c) { return stream(is_mask_kind(kind) ? mask_seed : seed, tag(kind, a, b, c)); }
GL_HD u64 field(u64 u) { return u >= gl::P ? u - gl::P : u; }
GL_HD u64 noise(u64 stream_key, u64 i, u64 m_sigma) {
    u64 s = 0;
#pragma unroll
    for (unsigned k = 0; k < 6; ++k) {
        const u64 d = draw(stream_key, 6 * i + k);
        s += (d & 0xFFFFFFFFull) + (d >> 32);
    }
    const long long t = (long long)s - (6ll << 32);                     // |t| <= 6 2^32
    const __int128 prod = (__int128)t * (__int128)m_sigma;              // m_sigma < 2^62
    const long long e = (long long)(prod >> 32);                        // arithmetic shift = floor
    return e < 0 ? gl::P - (u64)(-e) : (u64)e;
}

inline u64 sigma_to_int(double sigma) {
    const double q = (double)gl::P;  // 18446744069414584320.0, as `F::ORDER as f64`
    return (u64)std::floor(sigma * q + 0.5);
}
inline bool params_ok(const vpbs_keygen_params* k) {
    if (!k || k->log_N < 1 || k->log_N > 11 || k->K < 2 || k->K > 8 || k->LOGB < 1 || k->LOGB > 32) return false;
    const unsigned nl = (64 + k->LOGB - 1) / k->LOGB;
    if (k->ELL < 1 || k->ELL > nl || k->ELL > 16) return false;
    if (k->n_lwe < 1 || k->n_lwe > (k->K << k->log_N) || k->n_lwe >= (1u << 24)) return false;
    if (!(k->sigma_glwe >= 0.0) || !(k->sigma_lwe >= 0.0) || k->sigma_glwe > 0.2 || k->sigma_lwe > 0.2) return false;
    return true;
}
}  // namespace keygen
}  // namespace vpbs
