// The bootstrap chain of every one-workgroup-per-ciphertext kernel, stated once: the mod switch, the rotated coefficient, the digits of the
// signed decomposition, the two negacyclic transforms in LDS (two stages per pass, one __syncthreads() per pass) and pb_chain, the whole
// walk of one ciphertext -- LDS carve-up, step 0 or the resumed accumulator, the n + 1 steps with their GGSW products, out_ct and the
// sample extraction.  pbs_batch.hip (one key set per launch) and pbs_keyring.hip (a key set per workgroup) hold the two __global__
// kernels, which resolve their ciphertext and its key pointers and call pb_chain: canonical-in, canonical-out field operations in one
// order, so the words of the two kernels are the same because the code is.  tfhe.hip's per-step kernels stay the parity yardstick.
#pragma once
#include <cstddef>

#include "gl.h"

namespace vpbs {
using gl::u64;

constexpr size_t PBS_LDS_BUDGET = 160 * 1024;   // what one workgroup may declare on gfx950

// rotation amount in [0, 2N]: top log2(2N) bits of the mask, rounded with the next bit (mod.rs:85-106); as tfhe.hip.  Host and device:
// rotation.h predicts the chain's rotation from this very function (the kernels inline it to the instructions they had as a device function)
GL_HD unsigned pb_mod_switch(u64 mask, unsigned log_n_ring) {
    const unsigned log2n = log_n_ring + 1;
    return (unsigned)(mask >> (64 - log2n)) + (unsigned)((mask >> (64 - log2n - 1)) & 1);
}
// coefficient i of poly * X^shift mod X^N + 1, 0 <= shift <= 2N; as tfhe.hip
__device__ __forceinline__ u64 pb_rotated_coeff(const u64* poly, unsigned n, unsigned shift, unsigned i) {
    const unsigned src = (i + 2 * n - shift) & (2 * n - 1);
    const u64 c = poly[src & (n - 1)];
    return src >= n ? gl::neg(c) : c;
}

// The signed decomposition of one coefficient x (glwe_poly.rs:28-50) takes nl = ceil(64 / LOGB) balanced digits of xc = |x| (x negated when
// bit nl * LOGB - 1 is set), least significant first, and puts the sign back on each; the top ELL are the limbs.  This is digit l, balanced
// and as a field element, with the carry of the digit below in `carry` and its own left there.  (The loop over l stays with the
// caller: a helper for the whole coefficient compiles to another digit loop in pb_chain than the kernels had before they shared it.)
__device__ __forceinline__ u64 pb_decompose_digit(u64 xc, unsigned l, unsigned LOGB, unsigned& carry) {
    const unsigned lo_bit = l * LOGB;
    const u64 k = (lo_bit < 64 ? (xc >> lo_bit) : 0) & (((u64)1 << LOGB) - 1);
    const u64 kw = k + carry;
    carry = (unsigned)((k >> (LOGB - 1)) & 1);
    return gl::sub(kw, (u64)carry << LOGB);
}

// forward negacyclic NTT (crypto/poly.rs:9-34) of `cnt` polynomials back to back in LDS; ends behind a barrier
template <unsigned T>
__device__ __forceinline__ void pb_forward(u64* t, unsigned log_n, unsigned cnt, const u64* __restrict__ roots) {
    const unsigned n = 1u << log_n;
    unsigned m = 1, stages = log_n;
    while (stages >= 2) {   // stages m and 2m on the points j, j + h, j + len, j + len + h
        const unsigned len = n / (2 * m), h = len >> 1, log_h = stages - 2;
        for (unsigned q = threadIdx.x; q < cnt * (n >> 2); q += T) {
            const unsigned poly = q >> (log_n - 2), qq = q & ((n >> 2) - 1);
            const unsigned i = qq >> log_h, off = qq & (h - 1);
            u64* p = t + (size_t)poly * n + 2 * i * len + off;
            const u64 x0 = p[0], x1 = p[h], x2 = p[len], x3 = p[len + h];
            const u64 w = roots[m + i], w0 = roots[2 * m + 2 * i], w1 = roots[2 * m + 2 * i + 1];
            const u64 v2 = gl::mul(x2, w), v3 = gl::mul(x3, w);
            const u64 a0 = gl::add(x0, v2), a2 = gl::sub(x0, v2), a1 = gl::add(x1, v3), a3 = gl::sub(x1, v3);
            const u64 u1 = gl::mul(a1, w0), u3 = gl::mul(a3, w1);
            p[0] = gl::add(a0, u1);
            p[h] = gl::sub(a0, u1);
            p[len] = gl::add(a2, u3);
            p[len + h] = gl::sub(a2, u3);
        }
        __syncthreads();
        m <<= 2;
        stages -= 2;
    }
    if (stages == 1) {   // the last stage alone (odd log_n): m = n / 2, neighbours
        for (unsigned k = threadIdx.x; k < cnt * (n >> 1); k += T) {
            const unsigned poly = k >> (log_n - 1), i = k & ((n >> 1) - 1);
            u64* p = t + (size_t)poly * n + 2 * i;
            const u64 u = p[0], v = gl::mul(p[1], roots[m + i]);
            p[0] = gl::add(u, v);
            p[1] = gl::sub(u, v);
        }
        __syncthreads();
    }
}

// Inverse transform (crypto/poly.rs:36-64) of the `cnt` polynomials of t, in place; the LAST pass multiplies by N^-1 and hands each point
// to `finish(index in [cnt][N], value)` instead of storing it (the CMUX add into the accumulator).  Ends behind a barrier.
template <unsigned T, class Finish>
__device__ __forceinline__ void pb_inverse(u64* t, unsigned log_n, unsigned cnt, const u64* __restrict__ invroots, u64 ninv, Finish finish) {
    const unsigned n = 1u << log_n;
    unsigned m = n >> 1, stages = log_n, log_len = 0;
    while (stages >= 2) {   // stages m and m / 2 on the points j, j + len, j + 2 len, j + 3 len
        const unsigned len = 1u << log_len, m2 = m >> 1;
        const bool fin = stages == 2;
        for (unsigned q = threadIdx.x; q < cnt * (n >> 2); q += T) {
            const unsigned poly = q >> (log_n - 2), qq = q & ((n >> 2) - 1);
            const unsigned i2 = qq >> log_len, off = qq & (len - 1);
            const unsigned base = poly * n + 4 * i2 * len + off;
            u64* p = t + base;
            const u64 x0 = p[0], x1 = p[len], x2 = p[2 * len], x3 = p[3 * len];
            const u64 w0 = invroots[m + 2 * i2], w1 = invroots[m + 2 * i2 + 1], w = invroots[m2 + i2];
            const u64 a0 = gl::add(x0, x1), a1 = gl::mul(gl::sub(x0, x1), w0);
            const u64 a2 = gl::add(x2, x3), a3 = gl::mul(gl::sub(x2, x3), w1);
            const u64 y0 = gl::add(a0, a2), y2 = gl::mul(gl::sub(a0, a2), w);
            const u64 y1 = gl::add(a1, a3), y3 = gl::mul(gl::sub(a1, a3), w);
            if (fin) {
                finish(base, gl::mul(y0, ninv));
                finish(base + len, gl::mul(y1, ninv));
                finish(base + 2 * len, gl::mul(y2, ninv));
                finish(base + 3 * len, gl::mul(y3, ninv));
            } else {
                p[0] = y0;
                p[len] = y1;
                p[2 * len] = y2;
                p[3 * len] = y3;
            }
        }
        __syncthreads();
        m >>= 2;
        stages -= 2;
        log_len += 2;
    }
    if (stages == 1) {   // the last stage alone (odd log_n): m = 1, halves
        const unsigned len = n >> 1;
        const u64 w = invroots[1];
        for (unsigned k = threadIdx.x; k < cnt * len; k += T) {
            const unsigned poly = k >> (log_n - 1), i = k & (len - 1);
            const unsigned base = poly * n + i;
            const u64 u = t[base], v = t[base + len];
            finish(base, gl::mul(gl::add(u, v), ninv));
            finish(base + len, gl::mul(gl::mul(gl::sub(u, v), w), ninv));
        }
        __syncthreads();
    }
}

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

// The chain of ciphertext b under the key set (bsk [n_lwe][K][ELL][K][N], ksk [K][ELL][K][N], NTT domain), by one workgroup of T threads:
// the body of pbs_batch_kernel and pbs_keyring_kernel.  Args is PbsBatchArgs or PbsKeyringArgs; what is read of it here are the fields the
// two have in common (cts, testv, testv_stride, roots, ninv, out_ct, lwe_out, accs_out, log_n .. n_lwe, start, acc_in).  b, bsk and ksk are
// uniform over the workgroup.
// LDS (words): acc [K][N] | out [K][N] | limbs [ELL][N].  One input polynomial at a time is decomposed into `limbs` and transformed; its
// products with the GGSW rows are accumulated into the K polynomials of `out`; after the last input polynomial `out` goes through the
// inverse transform, whose last pass multiplies by N^-1 and adds into `acc`.
// PF: 16-byte key words a thread holds ahead per input polynomial: the ELL K N words g[p][.][.] that the product loop of input polynomial
// p consumes are requested into a register array BEFORE that polynomial is decomposed and transformed, and consumed after; the rows of
// p = 0 of the next step are requested before the inverse transform of this one.  0: no register array, the rows are read in the product
// loop (the Bootstrapper, whose rows sit in L2, and the ring's shapes that would need more than 8 entries).
// FROM: the start mode (a.start, a.acc_in) is an instantiation of its own, and its two arguments sit behind the older ones: with
// FROM = false a kernel compiles to the instructions it had before the start mode existed.
template <unsigned T, unsigned PF, bool FROM, class Args>
__device__ __forceinline__ void pb_chain(const Args a, const size_t b, const u64* bsk, const u64* ksk) {
    extern __shared__ __align__(16) u64 lds[];
    const unsigned log_n = a.log_n, n = 1u << log_n, K = a.K, ELL = a.ELL, LOGB = a.LOGB, n_lwe = a.n_lwe;
    const unsigned kn = K * n;
    u64* acc = lds;             // [K][N]
    u64* out = acc + kn;        // [K][N]
    u64* limbs = out + kn;      // [ELL][N]
    const u64* ct = a.cts + b * (n_lwe + 1);
    const u64* tv = a.testv + b * a.testv_stride;
    u64* accs = a.accs_out ? a.accs_out + b * (size_t)(n_lwe + 2) * kn : nullptr;
    const size_t ggsw_words = (size_t)K * ELL * kn;
    const unsigned nl = (64 + LOGB - 1) / LOGB, tb = nl * LOGB;
    constexpr bool ahead = PF != 0;
    ulonglong2 pf[PF ? PF : 1];
    // the step this ciphertext enters at: uniform over the workgroup, so the loop bounds below stay scalar and every barrier uniform
    const unsigned k0 = FROM ? a.start[b] : 0;
    const unsigned first = FROM && k0 ? k0 : 1;

    // the rows of the first step that runs, ahead of the accumulator's load (k0 = n_lwe + 2 runs no step: the rows of ksk, never used)
    if constexpr (ahead) kr_prefetch<T, PF>(pf, FROM && first > n_lwe ? ksk : bsk + (size_t)(first - 1) * ggsw_words, kn, ELL);
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

    for (unsigned step = first; step <= n_lwe + 1; ++step) {   // k0 = n_lwe + 2: no step, the outputs are acc_in's
        const bool last = step == n_lwe + 1;
        const u64* g = last ? ksk : bsk + (size_t)(step - 1) * ggsw_words;
        const unsigned shift = last ? 0 : pb_mod_switch(ct[step - 1], log_n);
        for (unsigned p = 0; p < K; ++p) {
            const u64* gp = g + (size_t)p * ELL * kn;
            if (ahead && p) kr_prefetch<T, PF>(pf, gp, kn, ELL);   // p = 0 was requested before the previous inverse transform
            const u64* poly = acc + (size_t)p * n;
            for (unsigned i = threadIdx.x; i < n; i += T) {
                // xprod_in = last ? acc : rotate(acc, mask) - acc (ivc_based_vpbs.rs:113-116), decomposed
                const u64 x = last ? poly[i] : gl::sub(pb_rotated_coeff(poly, n, shift, i), poly[i]);
                const unsigned sgn = tb <= 64 ? (unsigned)((x >> (tb - 1)) & 1) : 0;
                const u64 xc = sgn ? gl::neg(x) : x;
                unsigned carry = 0;
                for (unsigned l = 0; l < nl; ++l) {
                    const u64 bal = pb_decompose_digit(xc, l, LOGB, carry);
                    if (l + ELL >= nl) limbs[(l + ELL - nl) * n + i] = sgn ? gl::neg(bal) : bal;
                }
            }
            __syncthreads();
            pb_forward<T>(limbs, log_n, ELL, a.roots);
            // out[r] (+/-)= sum_l limbs_hat[l] * g[p][l][r]: + for the last GLEV, - for the others (ggsw_ct.rs:109-111); two points per thread
            const bool plus = p + 1 == K;
            if constexpr (ahead) {
                auto store = [&](unsigned idx, u64 s0, u64 s1) {
                    if (p == 0) {
                        out[idx] = plus ? s0 : gl::neg(s0);
                        out[idx + 1] = plus ? s1 : gl::neg(s1);
                    } else {
                        out[idx] = plus ? gl::add(out[idx], s0) : gl::sub(out[idx], s0);
                        out[idx + 1] = plus ? gl::add(out[idx + 1], s1) : gl::sub(out[idx + 1], s1);
                    }
                };
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
                    // the same store, written out: through the closure this loop compiles to other instructions than the Bootstrapper's
                    // kernel had before the body was shared, and its launches measured 0.6 - 1.0 % slower
                    if (p == 0) {
                        out[idx] = plus ? s0 : gl::neg(s0);
                        out[idx + 1] = plus ? s1 : gl::neg(s1);
                    } else {
                        out[idx] = plus ? gl::add(out[idx], s0) : gl::sub(out[idx], s0);
                        out[idx + 1] = plus ? gl::add(out[idx + 1], s1) : gl::sub(out[idx + 1], s1);
                    }
                }
            }
            __syncthreads();
        }
        // the first rows of the next step, ahead of the inverse transform
        if (ahead && !last) kr_prefetch<T, PF>(pf, step == n_lwe ? ksk : g + ggsw_words, kn, ELL);
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
}  // namespace vpbs
